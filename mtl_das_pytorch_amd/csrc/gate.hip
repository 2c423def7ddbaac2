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
// gather_windows_sel / window_probs_sel: gather_windows / window_probs (window.hip) with the batch rows numbered by
//   the selection: in replay cur, row r holds window sel[cur * B + r] while cur * B + r < *count, and is padding
//   beyond.  The count is read on the device, so one captured graph serves any selection.  The gather body and the
//   probability element are window_batch.h's.
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

// One block: select_scan_body (window_batch.h).
__global__ __launch_bounds__(256) void select_scan_kernel(int64_t* __restrict__ offs, int64_t nblocks,
                                                          int64_t* __restrict__ count) {
  __shared__ int64_t s_sum[256];
  select_scan_body(offs, nblocks, count, s_sum);
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

// The selection as a gather source: batch row b of replay cur is entry cur * B + b of sel, while that is below the
// count; the window has to be one of [lo, hi) and end inside the recording, as window.hip's.
struct SelectedSource {
  using time_type = int;
  const WindowSelArgs& a;
  const int64_t cur, count;
  DEV bool window(int b, int& f0, int& t0) const {
    const int64_t n = selected_window(a, cur, count, b);
    if (n < 0) return false;
    const int wa = (int)(n / a.nt), wb = (int)(n - (int64_t)wa * a.nt);
    f0 = a.g.fs[wa];
    t0 = a.ts[wb];
    return t0 >= 0 && t0 + a.g.Wt <= a.T;
  }
  DEV int64_t column(int t) const { return t; }
  DEV const float* base() const { return a.rec; }
  DEV int64_t pitch() const { return a.T; }

  // the window number of batch row r, -1 for padding (an entry past the count or the capacity, a number outside
  // [lo, hi))
  static DEV int64_t selected_window(const WindowSelArgs& a, int64_t cur, int64_t count, int r) {
    const int64_t i = cur * a.g.B + r;
    if (cur < 0 || i >= count || i >= a.cap) return -1;
    const int64_t n = a.sel[i];
    return (n >= a.lo && n < a.hi) ? n : -1;
  }
};

__global__ __launch_bounds__(256) void gather_windows_sel_kernel(WindowSelArgs a, bf16_t* __restrict__ out,
                                                                 int64_t* __restrict__ lab_out, int lab_w) {
  gather_windows_body(a.g, SelectedSource{a, *a.cursor, *a.count}, out, lab_out, lab_w);
}

// window_probs_kernel (window.hip) over the selection: one block; the cursor is advanced by thread 0 after every
// thread has read it.
__global__ __launch_bounds__(256) void window_probs_sel_kernel(WindowSelArgs a, const float* __restrict__ src,
                                                               int softmax, int T, int4 ncls, int K,
                                                               float* __restrict__ probs) {
  const int64_t cur = *a.cursor, count = *a.count;
  const int nc[4] = {ncls.x, ncls.y, ncls.z, ncls.w};
  for (int i = threadIdx.x; i < a.g.B * K; i += 256) {
    const int r = i / K, c = i - r * K;
    const int64_t n = SelectedSource::selected_window(a, cur, count, r);
    if (n < 0) continue;
    probs[n * K + c] = window_prob(src, softmax, T, nc, K, a.g.B, r, c);
  }
  __syncthreads();
  if (threadIdx.x == 0) *a.cursor = cur + 1;
}

// what both selected launches need of the numbering: the cursor form of WindowArgs plus the selection
bool selection_ok(const WindowSelArgs& a) {
  return a.g.B >= 1 && a.lo >= 0 && a.lo <= a.hi && !a.idx && a.cursor && a.sel && a.count && a.cap >= 0;
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

int launch_select_windows(const SelectArgs& a, int64_t* count, int64_t noffs, hipStream_t st) {
  // sel takes every window of [lo, hi) if all are active; offs holds one entry per block of 256 windows
  if (!a.power || !a.floor || !a.active || !a.sel || !a.offs || !count || a.N < 1 || a.nt < 1 || a.lo < 0 ||
      a.lo > a.hi || a.hi > a.N || a.cap < a.hi - a.lo || a.nfloor < (a.N + a.nt - 1) / a.nt ||
      noffs < select_blocks(a.N) || select_blocks(a.N) >= (1ll << 31))
    return -2;
  const unsigned blocks = (unsigned)select_blocks(a.N);
  hipLaunchKernelGGL(select_flags_kernel, dim3(blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, st, a.offs, (int64_t)blocks, count);
  hipLaunchKernelGGL(select_scatter_kernel, dim3(blocks), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int launch_gather_windows_sel(const WindowSelArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  if (!gather_geom_ok(a.g, out, lab_out, lab_w) || !selection_ok(a) || !a.rec || !a.ts || a.nt < 1 ||
      a.hi > (int64_t)a.g.nf * a.nt || a.g.Wt > a.T)
    return -2;
  return launch_gather(gather_windows_sel_kernel, a, out, lab_out, lab_w, st);
}

int launch_window_probs_sel(const WindowSelArgs& a, const float* src, int softmax, int T, const int* ncls, int K,
                            float* probs, int64_t nprobs, hipStream_t st) {
  int4 nc;
  if (!src || !probs || K < 1 || !selection_ok(a) || a.hi > nprobs || (int64_t)a.g.B * K >= (1ll << 31) ||
      !pack_ncls(softmax, T, ncls, K, nc))
    return -2;
  hipLaunchKernelGGL(window_probs_sel_kernel, dim3(1), dim3(256), 0, st, a, src, softmax, T, nc, K, probs);
  return (int)hipGetLastError();
}

}  // namespace mda
