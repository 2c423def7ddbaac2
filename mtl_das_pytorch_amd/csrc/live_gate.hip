// Activity gate of live inference (inference.py LiveRecording, gate_db): the energy detector of gate.hip in front of
// a recording that is still growing.  The whole-recording median of the offline gate needs the end of the time axis;
// here the noise floor runs along with the stream.
//
// Three rings of Jcap time indices hold, at row (j mod Jcap) * nf + a like the probability table, the power of window
// (j, a), its noise floor and its flag.  For every appended piece the host launches, for the new window numbers
// [n0, n1) (whole time indices; the host mirrors the counters, LiveBook):
//
// ring_window_power: window_power_body (window_batch.h) read through RingSource -- the accumulation, the mapping of
//   threads to elements and the reduction tree of gate.hip's window_power, so the fp32 power has the same bits as on
//   the linear recording.
// running_floor: one block per window (j, a).  The m = min(history, j + 1) powers of column a at indices
//   j - m + 1 .. j (row j included: causal, no look-ahead) go to LDS, every thread counts the elements ordered before
//   its own -- smaller, or equal and older; NaN after every number -- and the one of rank (m - 1) / 2, the lower
//   median, is the floor; 0 ("no floor yet") while m < warmup.  No atomics, no block waits on another.
// live_select: flags !(power < floor * ratio) as select_windows, and the ordered selection of the active window
//   numbers by the same three launches (block counts, one-block scan, ranked scatter).  The flags launch also zeroes
//   the table rows of the range: ring-table rows are recycled, and a quiet window must not inherit the probabilities
//   of the window Jcap indices earlier.  The scatter sets the batch cursor to 0 and LIVE_NEXT to n1.
// What the selection numbers -- the batch rows of the captured step's gather_windows_ring / live_probs -- is live.hip's,
// which takes it as LiveArgs::s and cursor.
#include "window_batch.h"

namespace mda {

namespace {

DEV int64_t ring_row(const LiveGateArgs& a, int64_t n) { return mda::ring_row(a.live.g.nf, a.Jcap, n); }

// One block per window, grid-stride over [n0, n1).  A window that cannot be read -- not available yet, outside the
// fiber, or no longer (not yet) inside the ring's R newest samples -- has no power: NaN, which the selection keeps.
__global__ __launch_bounds__(256) void ring_window_power_kernel(LiveGateArgs a) {
  __shared__ double s_red[256];
  const int64_t total = a.live.state[LIVE_TOTAL];
  const WindowGeom& g = a.live.g;
  const RingSource src(a.live);
  for (int64_t n = a.n0 + blockIdx.x; n < a.n1; n += gridDim.x) {
    int f0;
    int64_t t0;
    float p = __builtin_nanf("");
    if (src.numbered(n, f0, t0) && f0 >= 0 && f0 + g.Wf <= g.F && t0 + g.Wt <= total && total - t0 <= a.live.R)
      p = window_power_body(src, g.C, g.F, g.Wf, g.Wt, f0, t0, s_red);  // (the condition is the block's)
    if (threadIdx.x == 0) a.power[ring_row(a, n)] = p;
  }
}

// v[k] is ordered before v[i]: smaller, or equal and older (k < i); NaN after every number, two NaNs by age
DEV bool ordered_before(float vk, int k, float vi, int i) {
  const bool nk = vk != vk, ni = vi != vi;
  if (nk || ni) return nk == ni ? k < i : ni;
  return vk < vi || (vk == vi && k < i);
}

__global__ __launch_bounds__(256) void running_floor_kernel(LiveGateArgs a, int history, int warmup) {
  __shared__ float s_v[1024];
  const int nf = a.live.g.nf;
  for (int64_t n = a.n0 + blockIdx.x; n < a.n1; n += gridDim.x) {
    const int64_t wj = n / nf;
    const int wa = (int)(n - wj * nf);
    const int m = (int)(wj + 1 < history ? wj + 1 : history);
    if (m < warmup) {
      if (threadIdx.x == 0) a.floor[ring_row(a, n)] = 0.f;
      continue;
    }
    for (int i = threadIdx.x; i < m; i += 256) s_v[i] = a.power[((wj - m + 1 + i) % a.Jcap) * nf + wa];  // by age
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 256) {
      const float v = s_v[i];
      int rank = 0;
      for (int k = 0; k < m; ++k) rank += ordered_before(s_v[k], k, v, i) ? 1 : 0;
      if (rank == (m - 1) / 2) a.floor[ring_row(a, n)] = v;  // the order is total: exactly one element
    }
    __syncthreads();  // (s_v is read before the next window overwrites it)
  }
}

// Block i owns windows n0 + 256 i .. n0 + 256 i + 255: their flags, how many are set, and their table rows zeroed.
__global__ __launch_bounds__(256) void live_flags_kernel(LiveGateArgs a, float ratio, float* __restrict__ table,
                                                         int pitch, int64_t* __restrict__ offs) {
  __shared__ int s_wave[4];
  const int64_t first = a.n0 + (int64_t)blockIdx.x * 256;
  const int64_t n = first + threadIdx.x;
  bool on = false;
  if (n < a.n1) {
    const int64_t row = ring_row(a, n);
    on = n < a.live.state[LIVE_AVAIL] && !(a.power[row] < a.floor[row] * ratio);
    a.active[row] = on ? 1 : 0;
  }
  const int set = block_flag_count(on, s_wave);
  if (threadIdx.x == 0) offs[blockIdx.x] = (int64_t)set;
  for (int e = threadIdx.x; e < 256 * pitch; e += 256) {
    const int r = e / pitch;
    if (first + r < a.n1) table[ring_row(a, first + r) * pitch + (e - r * pitch)] = 0.f;
  }
}

// Block i writes its active windows from sel[offs[i]] on (ranked_place); the step's counters start over.
__global__ __launch_bounds__(256) void live_scatter_kernel(LiveGateArgs a, const int64_t* __restrict__ offs) {
  __shared__ int s_wave[4];
  const int64_t n = a.n0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool on = n < a.n1 && a.active[ring_row(a, n)] != 0;
  const int64_t at = ranked_place(on, offs[blockIdx.x], s_wave);
  if (on && at < a.live.s.cap) a.live.s.sel[at] = n;  // (at < count <= n1 - n0 <= cap: the launcher's check)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *a.live.cursor = 0;
    a.live.state[LIVE_NEXT] = a.n1;
  }
}

// [n0, n1) is a range of whole time indices that fits the rings
bool range_ok(const LiveGateArgs& a) {
  const int nf = a.live.g.nf;
  return nf >= 1 && a.Jcap >= 1 && a.n0 >= 0 && a.n0 <= a.n1 && a.n0 % nf == 0 && a.n1 % nf == 0 &&
         (a.n1 - a.n0) / nf <= a.Jcap;
}

unsigned window_blocks(const LiveGateArgs& a) { return (unsigned)std::min<int64_t>(a.n1 - a.n0, 65535); }

}  // namespace

int launch_ring_window_power(const LiveGateArgs& a, hipStream_t st) {
  const WindowGeom& g = a.live.g;
  if (!live_args_ok(a.live) || !g.fs || !a.power || !range_ok(a) || g.Wf < 1 || g.Wf > g.F ||
      (int64_t)g.Wf * g.Wt >= (1ll << 31))
    return -2;
  if (a.n1 == a.n0) return 0;
  hipLaunchKernelGGL(ring_window_power_kernel, dim3(window_blocks(a)), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

int launch_running_floor(const LiveGateArgs& a, int history, int warmup, hipStream_t st) {
  // rows j0 - (history - 1) .. j1 - 1 of the power ring are distinct
  if (!a.power || !a.floor || !range_ok(a) || history < 1 || history > 1024 || warmup < 1 || warmup > history ||
      a.Jcap < history - 1 + (a.n1 - a.n0) / a.live.g.nf)
    return -2;
  if (a.n1 == a.n0) return 0;
  hipLaunchKernelGGL(running_floor_kernel, dim3(window_blocks(a)), dim3(256), 0, st, a, history, warmup);
  return (int)hipGetLastError();
}

int launch_live_select(const LiveGateArgs& a, float ratio, float* table, int64_t nrows, int pitch, int64_t* offs,
                       int64_t noffs, hipStream_t st) {
  // the selection is written here: it has to be there, whole
  if (!a.live.state || !a.live.s.sel || !live_selection_ok(a.live) || !a.power || !a.floor || !a.active || !table ||
      !offs || !range_ok(a) || a.live.s.cap < a.n1 - a.n0 || pitch < 1 || pitch > (1 << 16) ||
      nrows < (int64_t)a.Jcap * a.live.g.nf || noffs < select_blocks(a.n1 - a.n0) ||
      select_blocks(a.n1 - a.n0) >= (1ll << 31))
    return -2;
  if (a.n1 == a.n0) return 0;
  const unsigned blocks = (unsigned)select_blocks(a.n1 - a.n0);
  hipLaunchKernelGGL(live_flags_kernel, dim3(blocks), dim3(256), 0, st, a, ratio, table, pitch, offs);
  launch_select_scan(offs, (int64_t)blocks, a.live.s.count, st);
  hipLaunchKernelGGL(live_scatter_kernel, dim3(blocks), dim3(256), 0, st, a, (const int64_t*)offs);
  return (int)hipGetLastError();
}

}  // namespace mda
