// Activity gate of resident-recording inference (inference.py predict_recording, gate_db): an energy detector in
// front of the classifier.  The models have no "nothing is happening" class, so the windows of a recording that hold
// only background noise are found by their power and never reach the model.
//
// window_power: P[n] = (1 / C) sum_c mean over window n of (x - mu_c)^2, mu_c the window's own mean in channel c --
//   sample_power (augment.hip) applied to a window: two passes with fp64 accumulators, one block per window, a fixed
//   reduction order, one fp32 rounding on the store.
// select_windows: window n of [lo, hi) is active iff !(P[n] < floor[n / nt] * ratio) -- one fp32 multiply; a NaN
//   power is active -- and the active window numbers are written to sel[] in ascending order, their number to a
//   device count.  Three launches -- flags and block counts, an exclusive scan of the block counts by one block,
//   the ranked scatter (ballot / mbcnt inside a wave) -- so no block waits on another and no atomic decides a
//   position: the result is the same on every run.
//   The scan launch is live_gate.hip's live_select's too (launch_select_scan).
// What the selection numbers -- the batch rows of gather_windows / window_probs -- is window.hip's, which takes it as
// WindowArgs::s.
#include "window_batch.h"

namespace mda {

namespace {

// the resident recording [C][F][T] as the source of window_power_body: time t is column t
struct LinearSource {
  const float* rec;
  int T;
  DEV int64_t column(int t) const { return t; }
  DEV const float* base() const { return rec; }
  DEV int64_t pitch() const { return T; }
};

// One block per window, grid-stride over the windows; element e of a window's plane is (e / Wt, e % Wt), threads
// along time.  A window that does not lie inside the recording has no power: NaN, which the selection keeps.
__global__ __launch_bounds__(256) void window_power_kernel(PowerArgs a) {
  __shared__ double s_red[256];
  const int64_t N = (int64_t)a.nf * a.nt;
  for (int64_t n = blockIdx.x; n < N; n += gridDim.x) {
    const int wa = (int)(n / a.nt), wb = (int)(n - (int64_t)wa * a.nt);
    const int f0 = a.fs[wa], t0 = a.ts[wb];
    if (f0 < 0 || f0 + a.Wf > a.F || t0 < 0 || t0 + a.Wt > a.T) {
      if (threadIdx.x == 0) a.power[n] = __builtin_nanf("");
      continue;
    }
    const float p = window_power_body(LinearSource{a.rec, a.T}, a.C, a.F, a.Wf, a.Wt, f0, t0, s_red);
    if (threadIdx.x == 0) a.power[n] = p;
  }
}

// Block i owns windows 256 i .. 256 i + 255: their flags and how many are set.
__global__ __launch_bounds__(256) void select_flags_kernel(SelectArgs a) {
  __shared__ int s_wave[4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool on = false;
  if (n < a.N) {
    on = n >= a.lo && n < a.hi && !(a.power[n] < a.floor[n / a.nt] * a.ratio);
    a.active[n] = on ? 1 : 0;
  }
  const int set = block_flag_count(on, s_wave);
  if (threadIdx.x == 0) a.offs[blockIdx.x] = (int64_t)set;
}

// One block: the block counts become their exclusive prefix sums (in place, 256 at a time with a carry), the total
// becomes the count.
__global__ __launch_bounds__(256) void select_scan_kernel(int64_t* __restrict__ offs, int64_t nblocks,
                                                          int64_t* __restrict__ count) {
  __shared__ int64_t s_sum[256];
  int64_t carry = 0;
  for (int64_t base = 0; base < nblocks; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int64_t own = i < nblocks ? offs[i] : 0;
    s_sum[threadIdx.x] = own;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
      const int64_t v = threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0;
      __syncthreads();
      s_sum[threadIdx.x] += v;
      __syncthreads();
    }
    if (i < nblocks) offs[i] = carry + s_sum[threadIdx.x] - own;
    carry += s_sum[255];
    __syncthreads();  // (s_sum[255] is read before the next round overwrites it)
  }
  if (threadIdx.x == 0) *count = carry;
}

// Block i writes its active windows from sel[offs[i]] on: a window's place is the number of active windows before
// it -- those of the blocks before (offs), of the block's waves before (the ballots' counts), of the wave's lanes
// below (mbcnt).
__global__ __launch_bounds__(256) void select_scatter_kernel(SelectArgs a) {
  __shared__ int s_wave[4];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = n < a.N && a.active[n] != 0;
  const int64_t at = ranked_place(on, a.offs[blockIdx.x], s_wave);
  if (on && at < a.cap) a.sel[at] = n;  // (at < count <= hi - lo <= cap: the launcher checks the capacity)
}

}  // namespace

int launch_window_power(const PowerArgs& a, hipStream_t st) {
  if (!a.rec || !a.fs || !a.ts || !a.power || a.C < 1 || a.F < 1 || a.T < 1 || a.nf < 1 || a.nt < 1 || a.Wf < 1 ||
      a.Wt < 1 || a.Wf > a.F || a.Wt > a.T || (int64_t)a.Wf * a.Wt >= (1ll << 31))
    return -2;
  const int64_t N = (int64_t)a.nf * a.nt;
  hipLaunchKernelGGL(window_power_kernel, dim3((unsigned)std::min<int64_t>(N, 65535)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int64_t select_blocks(int64_t N) { return (N + 255) / 256; }

void launch_select_scan(int64_t* offs, int64_t nblocks, int64_t* count, hipStream_t st) {
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, st, offs, nblocks, count);
}

int launch_select_windows(const SelectArgs& a, int64_t* count, int64_t noffs, hipStream_t st) {
  // sel takes every window of [lo, hi) if all are active; offs holds one entry per block of 256 windows
  if (!a.power || !a.floor || !a.active || !a.sel || !a.offs || !count || a.N < 1 || a.nt < 1 || a.lo < 0 ||
      a.lo > a.hi || a.hi > a.N || a.cap < a.hi - a.lo || a.nfloor < (a.N + a.nt - 1) / a.nt ||
      noffs < select_blocks(a.N) || select_blocks(a.N) >= (1ll << 31))
    return -2;
  const unsigned blocks = (unsigned)select_blocks(a.N);
  hipLaunchKernelGGL(select_flags_kernel, dim3(blocks), dim3(256), 0, st, a);
  launch_select_scan(a.offs, (int64_t)blocks, count, st);
  hipLaunchKernelGGL(select_scatter_kernel, dim3(blocks), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mda
