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
#include "kernels.h"

namespace mda {

// The window number of batch row r: idx[r], or lo + cursor * B + r.  Rows outside [lo, hi) are padding.
DEV int64_t window_number(const int64_t* __restrict__ idx, int64_t cur, int64_t lo, int B, int r) {
  return idx ? idx[r] : lo + cur * B + r;
}

// One thread per output pixel, threads along t (the recording's contiguous axis).  The padding of the tap
// packing is the window's: channel j of pixel (h, w) is x[h - off + j][w] inside the window, zero outside it even
// where the recording has rows there.  Padding rows of the batch are written as zeros and read nothing; so is a
// row whose table entry would put the window outside the recording.
__global__ __launch_bounds__(256) void gather_windows_kernel(WindowArgs a, bf16_t* __restrict__ out,
                                                             int64_t* __restrict__ lab_out, int lab_w) {
  const int64_t cur = a.cursor ? *a.cursor : 0;
  const int HW = a.Wf * a.Wt;
  const int64_t M = (int64_t)a.B * HW;
  const int64_t FT = (int64_t)a.F * a.T;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < M; p += (int64_t)gridDim.x * 256) {
    const int b = (int)p / HW;  // M < 2^31 (checked by the launcher)
    const int r = (int)p - b * HW;
    const int h = r / a.Wt, w = r - h * a.Wt;
    const int64_t n = window_number(a.idx, cur, a.lo, a.B, b);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (n >= a.lo && n < a.hi) {
      const int wa = (int)(n / a.nt), wb = (int)(n - (int64_t)wa * a.nt);
      const int f0 = a.fs[wa], t0 = a.ts[wb];
      if (f0 >= 0 && f0 + a.Wf <= a.F && t0 >= 0 && t0 + a.Wt <= a.T) {
        if (a.taps > 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int hh = h - a.off + j;
            if (j < a.taps && hh >= 0 && hh < a.Wf) v[j] = a.rec[(int64_t)(f0 + hh) * a.T + t0 + w];
          }
        } else {
          const int64_t src = (int64_t)(f0 + h) * a.T + t0 + w;
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (c < a.C) v[c] = a.rec[c * FT + src];
        }
      }
    }
    store8(out + p * 8, v);
  }
  // the head kernels read labels for their metrics: inference has none
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.B * lab_w; i += 256) lab_out[i] = 0;
}

static bool window_args_ok(const WindowArgs& a) {
  return a.B > 0 && a.nf > 0 && a.nt > 0 && a.lo >= 0 && a.lo <= a.hi && a.hi <= (int64_t)a.nf * a.nt &&
         (a.idx == nullptr) != (a.cursor == nullptr) && a.fs && a.ts;
}

int launch_gather_windows(const WindowArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  if (!window_args_ok(a) || !a.rec || a.C < 1 || a.C > 8 || a.taps < 0 || a.taps > 8 || (a.taps > 0 && a.C != 1) ||
      a.Wf < 1 || a.Wt < 1 || a.Wf > a.F || a.Wt > a.T || lab_w < 0 ||
      (int64_t)a.B * a.Wf * a.Wt >= (1ll << 31))
    return -2;
  const int64_t M = (int64_t)a.B * a.Wf * a.Wt;
  const int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
  hipLaunchKernelGGL(gather_windows_kernel, dim3(blocks), dim3(256), 0, st, a, out, lab_out, lab_w);
  return (int)hipGetLastError();
}

// One block, sized for a head's output (B * K around a thousand: every thread of the softmax form recomputes its
// row's max and sum, 2 K expf).  softmax = 0 (Models A/B): src is logp [T][B][16] and column c of a row is exp(logp[t][r][c - c0_t])
// of the task t that owns it (ncls[t] columns each, side by side).  softmax = 1 (Model C): src is logits [B][K]
// and the row is their max-subtracted softmax; every thread of a row sums in the same order.  The cursor is
// advanced by thread 0 after every thread has read it (the block barrier).
__global__ __launch_bounds__(256) void window_probs_kernel(WindowArgs a, const float* __restrict__ src, int softmax,
                                                           int T, int4 ncls, int K, float* __restrict__ probs) {
  const int64_t cur = a.cursor ? *a.cursor : 0;
  const int nc[4] = {ncls.x, ncls.y, ncls.z, ncls.w};
  for (int i = threadIdx.x; i < a.B * K; i += 256) {
    const int r = i / K, c = i - r * K;
    const int64_t n = window_number(a.idx, cur, a.lo, a.B, r);
    if (n < a.lo || n >= a.hi) continue;
    float p;
    if (softmax) {
      const float* x = src + (int64_t)r * K;
      float mx = x[0];
      for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
      float s = 0.f;
      for (int k = 0; k < K; ++k) s += expf(x[k] - mx);
      p = expf(x[c] - mx) / s;
    } else {
      int t = 0, c0 = 0;
      while (t + 1 < T && c >= c0 + nc[t]) c0 += nc[t++];
      p = expf(src[((int64_t)t * a.B + r) * 16 + (c - c0)]);
    }
    probs[n * K + c] = p;
  }
  if (a.cursor) {
    __syncthreads();
    if (threadIdx.x == 0) *a.cursor = cur + 1;
  }
}

int launch_window_probs(const WindowArgs& a, const float* src, int softmax, int T, const int* ncls, int K,
                        float* probs, int64_t nprobs, hipStream_t st) {
  // rows [lo, hi) of the table are written: hi may not pass its nprobs rows
  if (!src || !probs || K < 1 || a.B < 1 || a.lo < 0 || a.lo > a.hi || a.hi > nprobs ||
      (a.idx == nullptr) == (a.cursor == nullptr) || (int64_t)a.B * K >= (1ll << 31))
    return -2;
  int4 nc = make_int4(0, 0, 0, 0);
  if (!softmax) {
    if (T < 1 || T > 4) return -2;
    int sum = 0, v[4] = {0, 0, 0, 0};
    for (int t = 0; t < T; ++t) {
      if (ncls[t] < 1 || ncls[t] > 16) return -2;
      v[t] = ncls[t];
      sum += ncls[t];
    }
    if (sum != K) return -2;
    nc = make_int4(v[0], v[1], v[2], v[3]);
  }
  hipLaunchKernelGGL(window_probs_kernel, dim3(1), dim3(256), 0, st, a, src, softmax, T, nc, K, probs);
  return (int)hipGetLastError();
}

// The windows overlapping [r0, r1) of one axis: starts are strictly increasing, so they are the contiguous
// range first(s + win > r0) .. last(s < r1), found by bisection.
DEV void covering_range(const int* __restrict__ s, int n, int win, int r0, int r1, int& a0, int& a1) {
  int lo = 0, hi = n;  // first index with s[i] > r0 - win
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (s[m] > r0 - win) hi = m; else lo = m + 1;
  }
  a0 = lo;
  hi = n;  // first index with s[i] >= r1
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (s[m] >= r1) hi = m; else lo = m + 1;
  }
  a1 = lo;  // exclusive
}

// One thread per (cell row i, cell column j, class k), k fastest (the probability rows are read contiguously).
// A sample's value is the mean of the windows that cover it and a cell's value the mean of its samples; the
// windows covering a sample are (windows covering its row) x (windows covering its time), so
//   map[k][i][j] = sum_a sum_b wf[a,i] wt[b,j] probs[a nt + b][k]
// with wf[a,i] = (1 / rows of cell i) * sum over the rows f that window a shares with cell i of 1 / (windows
// covering f), and wt likewise in time: each axis' weights of a cell sum to 1.  The host computes them in fp64
// and passes them as bands: window a reaches at most mf = (Wf - 1) / cf + 2 cell rows from fs[a] / cf on, and its
// weights for them are wf[a * mf ..].  The sums run in (a, b) order over the cell's covering windows.
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
      const int di = i - a.fs[wa] / a.cf;
      if (di < 0 || di >= a.mf) continue;  // (a covering window's cell is inside its band)
      const float wf = a.wf[(int64_t)wa * a.mf + di];
      const float* row = a.probs + ((int64_t)wa * a.nt) * a.K + k;
      for (int b = b0; b < b1; ++b) {
        const int dj = j - a.ts[b] / a.ct;
        if (dj < 0 || dj >= a.mt) continue;
        acc += (wf * a.wt[(int64_t)b * a.mt + dj]) * row[(int64_t)b * a.K];
      }
    }
    a.map[((int64_t)k * a.nfc + i) * a.ntc + j] = acc;
  }
}

// every sample of [0, len) is inside a window: starts strictly increasing, first at 0, no gap, last reaches len
static bool starts_cover(const int* s, int n, int win, int len) {
  if (n < 1 || win < 1 || s[0] != 0 || s[n - 1] + (int64_t)win < len) return false;
  for (int i = 0; i < n; ++i) {
    if (s[i] < 0 || s[i] + (int64_t)win > len) return false;
    if (i && (s[i] <= s[i - 1] || s[i] > s[i - 1] + (int64_t)win)) return false;
  }
  return true;
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
