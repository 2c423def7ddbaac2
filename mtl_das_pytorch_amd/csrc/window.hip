// Resident-recording inference (inference.py predict_recording, windows="resident").
//
// gather_windows: cuts the batch's sliding windows out of an HBM-resident fp32 [C, F, T] recording straight
//   into the stem's bf16 NHWC-8 input (the layout gather_batch writes, vertical tap packing included), so the
//   [N, C, Wf, Wt] window stack -- (Wf * Wt) / (stride_f * stride_t) times the recording -- never exists.
// window_probs: after the eval forward, writes each valid batch row's class probabilities into its row of a
//   resident [N, K] table and, in cursor form, advances the batch cursor: ceil((hi - lo) / B) replays of one
//   captured graph need no host copy between them.
// window_map: a sample's value is the mean of the windows covering it, a cell's the mean of its samples; computed
//   in gather form (one thread per output, fixed summation order): deterministic, no atomics.
//
// Both launches take the batch rows numbered by an on-device selection (WindowArgs::s, written by gate.hip's
// select_windows) in place of idx or the consecutive cursor form: the launcher sees it from the pointers, the kernel
// branches on them.  The count is read on the device, so one captured graph serves any selection.
//
// The gather body, the selected numbering, the probability element, the covering windows and weight bands of a cell,
// and the launchers' common checks are window_batch.h's, shared with live.hip.
#include "window_batch.h"

namespace mda {

// The window number of batch row r: the selection's entry, idx[r], or lo + cursor * B + r.  Numbers outside
// [lo, hi) are padding.
struct WindowNumbering {
  const WindowArgs& a;
  const int64_t cur, count;
  DEV explicit WindowNumbering(const WindowArgs& a)
      : a(a), cur(a.cursor ? *a.cursor : 0), count(a.s.sel ? *a.s.count : 0) {}
  DEV int64_t operator()(int r) const {
    if (a.s.sel) return selected_number(a.s, cur, count, a.g.B, r);
    return a.idx ? a.idx[r] : a.lo + cur * a.g.B + r;
  }
};

// The recording as a gather source: window n = a * nt + b of [lo, hi) starts at (fs[a], ts[b]) and has to end inside
// the recording; time t is column t.
struct RecordingSource {
  using time_type = int;
  const WindowArgs& a;
  DEV bool numbered(int64_t n, int& f0, int& t0) const {
    if (n < a.lo || n >= a.hi) return false;
    const int wa = (int)(n / a.nt), wb = (int)(n - (int64_t)wa * a.nt);
    f0 = a.g.fs[wa];
    t0 = a.ts[wb];
    return t0 >= 0 && t0 + a.g.Wt <= a.T;
  }
  DEV int64_t column(int t) const { return t; }
  DEV const float* base() const { return a.rec; }
  DEV int64_t pitch() const { return a.T; }
};

__global__ __launch_bounds__(256) void gather_windows_kernel(WindowArgs a, bf16_t* __restrict__ out,
                                                             int64_t* __restrict__ lab_out, int lab_w) {
  gather_windows_body(a.g, RecordingSource{a}, WindowNumbering(a), out, lab_out, lab_w);
}

// what gather_windows and window_probs both need of the numbering: exactly one of idx / cursor, and a selection
// only whole and with the cursor (so without idx)
static bool numbering_ok(const WindowArgs& a) {
  return a.g.B >= 1 && a.lo >= 0 && a.lo <= a.hi && (a.idx == nullptr) != (a.cursor == nullptr) &&
         selection_ok(a.s) && !(a.s.sel && !a.cursor);
}

int launch_gather_windows(const WindowArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  if (!gather_geom_ok(a.g, out, lab_out, lab_w) || !numbering_ok(a) || !a.rec || !a.ts || a.nt < 1 ||
      a.hi > (int64_t)a.g.nf * a.nt || a.g.Wt > a.T)
    return -2;
  return launch_gather(gather_windows_kernel, a, out, lab_out, lab_w, st);
}

// One block, sized for a head's output (B * K around a thousand; window_batch.h window_prob).  The cursor is
// advanced by thread 0 after every thread has read it (the block barrier).
__global__ __launch_bounds__(256) void window_probs_kernel(WindowArgs a, const float* __restrict__ src, int softmax,
                                                           int T, int4 ncls, int K, float* __restrict__ probs) {
  const WindowNumbering num(a);
  const int nc[4] = {ncls.x, ncls.y, ncls.z, ncls.w};
  for (int i = threadIdx.x; i < a.g.B * K; i += 256) {
    const int r = i / K, c = i - r * K;
    const int64_t n = num(r);
    if (n < a.lo || n >= a.hi) continue;
    probs[n * K + c] = window_prob(src, softmax, T, nc, K, a.g.B, r, c);
  }
  if (a.cursor) {
    __syncthreads();
    if (threadIdx.x == 0) *a.cursor = num.cur + 1;
  }
}

int launch_window_probs(const WindowArgs& a, const float* src, int softmax, int T, const int* ncls, int K,
                        float* probs, int64_t nprobs, hipStream_t st) {
  // rows [lo, hi) of the table are written: hi may not pass its nprobs rows
  int4 nc;
  if (!src || !probs || K < 1 || !numbering_ok(a) || a.hi > nprobs || (int64_t)a.g.B * K >= (1ll << 31) ||
      !pack_ncls(softmax, T, ncls, K, nc))
    return -2;
  hipLaunchKernelGGL(window_probs_kernel, dim3(1), dim3(256), 0, st, a, src, softmax, T, nc, K, probs);
  return (int)hipGetLastError();
}

// One thread per (cell row i, cell column j, class k), k fastest (the probability rows are read contiguously).
// A sample's value is the mean of the windows that cover it and a cell's value the mean of its samples; the
// windows covering a sample are (windows covering its row) x (windows covering its time), so
//   map[k][i][j] = sum_a sum_b wf[a,i] wt[b,j] probs[a nt + b][k]
// with wf[a,i] = (1 / rows of cell i) * sum over the rows f that window a shares with cell i of 1 / (windows
// covering f), and wt likewise in time: each axis' weights of a cell sum to 1 (bands: window_batch.h band_weight).
// The sums run in (a, b) order over the cell's covering windows.
__global__ __launch_bounds__(256) void window_map_kernel(MapArgs a) {
  const int64_t total = (int64_t)a.nfc * a.ntc * a.K;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int k = (int)(g % a.K);
    const int64_t cell = g / a.K;
    const int i = (int)(cell / a.ntc), j = (int)(cell - (int64_t)i * a.ntc);
    const int r0 = i * a.cf, r1 = min(r0 + a.cf, a.F);
    const int c0 = j * a.ct, c1 = min(c0 + a.ct, a.T);
    int a0, a1, b0, b1;
    covering_range(a.fs, a.nf, a.Wf, r0, r1, a0, a1);
    covering_range(a.ts, a.nt, a.Wt, c0, c1, b0, b1);
    float acc = 0.f;
    for (int wa = a0; wa < a1; ++wa) {
      float wf, wt;
      if (!band_weight(a.fs, a.wf, a.mf, a.cf, wa, i, wf)) continue;
      const float* row = a.probs + ((int64_t)wa * a.nt) * a.K + k;
      for (int b = b0; b < b1; ++b)
        if (band_weight(a.ts, a.wt, a.mt, a.ct, b, j, wt)) acc += (wf * wt) * row[(int64_t)b * a.K];
    }
    a.map[((int64_t)k * a.nfc + i) * a.ntc + j] = acc;
  }
}

int launch_window_map(const MapArgs& a, const int* h_fs, const int* h_ts, hipStream_t st) {
  if (!a.probs || !a.map || !a.fs || !a.ts || !a.wf || !a.wt || !h_fs || !h_ts || a.K < 1 || a.cf < 1 || a.ct < 1 ||
      a.F < 1 || a.T < 1)
    return -2;
  if (a.mf != (a.Wf - 1) / a.cf + 2 || a.mt != (a.Wt - 1) / a.ct + 2) return -2;  // the weight bands' widths
  if (a.nfc != (a.F + a.cf - 1) / a.cf || a.ntc != (a.T + a.ct - 1) / a.ct) return -2;
  // a sample no window covers has no value
  if (!starts_cover(h_fs, a.nf, a.Wf, a.F) || !starts_cover(h_ts, a.nt, a.Wt, a.T)) return -2;
  const int64_t total = (int64_t)a.nfc * a.ntc * a.K;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(window_map_kernel, dim3(blocks), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mda
