// Pieces shared by the two sliding-window inference paths: the resident recording (window.hip) and the growing
// recording whose time axis is a ring (live.hip).  One copy of
//
//   * the gather body: the NHWC-8 pixel loop with the stem's tap packing and the window-edge padding, a template
//     over two separate things: the numbering (which window number batch row b holds, or that it is padding) and
//     the source (where window n starts, which column holds time t, base pointer and row pitch); the pixel itself
//     -- 8 tap-packed channels of a column, or C channels padded to 8 -- is the batch gather's (stem_gather.h);
//   * the selected numbering, the one both sources and both probability kernels use when the launch carries a
//     Selection: entry cur * B + r of sel while below the count and the capacity;
//   * the ring as a source (RingSource) and its table row, the window power body (a template over the source, so
//     the ring's powers have the bits of the linear recording's) and the ordered selection's count / scan / rank
//     pieces, shared by the two activity gates (gate.hip, live_gate.hip);
//   * the probability element: softmax of a logits row, or exp of the owning task's log-probability;
//   * the fiber side of the maps: the windows covering a cell (bisection) and the weight-band lookup;
//   * the launchers' common checks: the batch geometry, the selection, the ncls packing, "the starts cover the axis".
//
// What differs stays in the kernels: the unselected numberings (idx / cursor in window.hip, next in live.hip), where
// a row's probabilities go, the counter advance, and the maps' time loops (bands over ts in window.hip, per-column
// weight vectors over the ring table in live.hip).  The maps' sums `acc += (wf * wt) * p` are written out in each
// kernel: their rounding is the kernel's.
#pragma once
#include "kernels.h"
#include "stem_gather.h"

namespace mda {

// The selected numbering: the window number of batch row r in replay cur, -1 for padding (an entry past the count
// or the capacity).  count is *s.count, read once by the kernel.
DEV int64_t selected_number(const Selection& s, int64_t cur, int64_t count, int B, int r) {
  const int64_t i = cur * B + r;
  return (cur < 0 || i >= count || i >= s.cap) ? -1 : s.sel[i];
}

// sel and count come together (the launcher adds what it requires of the cursor)
inline bool selection_ok(const Selection& s) { return (s.sel == nullptr) == (s.count == nullptr) && s.cap >= 0; }

// One thread per output pixel, threads along t (the source's contiguous axis).  The padding of the tap packing is
// the window's: channel j of pixel (h, w) is x[h - off + j][w] inside the window, zero outside it even where the
// source has rows there.  A batch row that is no window (padding, a number the source does not have, or a start
// outside the source) is written as zeros and reads nothing.
//   int64_t num(int b)                           the window number of batch row b; padding is a number no source has
//   bool src.numbered(int64_t n, int& f0, T& t0) window n exists, starting at fiber row f0 and time t0
//   int64_t src.column(t)                        the column of the source that holds time t
//   const float* src.base(); int64_t src.pitch() the source is [C][F][pitch] fp32
template <class Source, class Numbering>
DEV void gather_windows_body(const WindowGeom& g, const Source& src, const Numbering& num, bf16_t* __restrict__ out,
                             int64_t* __restrict__ lab_out, int lab_w) {
  const int HW = g.Wf * g.Wt;
  const int64_t M = (int64_t)g.B * HW;
  const float* __restrict__ x = src.base();
  const int64_t pitch = src.pitch(), plane = (int64_t)g.F * pitch;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < M; p += (int64_t)gridDim.x * 256) {
    const int b = (int)p / HW;  // M < 2^31 (gather_geom_ok)
    const int r = (int)p - b * HW;
    const int h = r / g.Wt, w = r - h * g.Wt;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    int f0;
    typename Source::time_type t0;
    if (src.numbered(num(b), f0, t0) && f0 >= 0 && f0 + g.Wf <= g.F) {
      const float* at = x + (int64_t)(f0 + h) * pitch + src.column(t0 + w);  // the pixel's element of channel 0
      if (g.taps > 0) stem_taps(at, pitch, h, g.Wf, g.taps, g.off, v);
      else stem_channels(at, plane, g.C, v);
    }
    store8(out + p * 8, v);
  }
  // the head kernels read labels for their metrics: inference has none
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < g.B * lab_w; i += 256) lab_out[i] = 0;
}

// What both gather launchers require of the geometry and the outputs.
inline bool gather_geom_ok(const WindowGeom& g, const bf16_t* out, const int64_t* lab_out, int lab_w) {
  return g.fs && out && lab_out && lab_w >= 0 && g.B >= 1 && g.nf >= 1 && g.C >= 1 && g.C <= 8 && g.taps >= 0 &&
         g.taps <= 8 && !(g.taps > 0 && g.C != 1) && g.Wf >= 1 && g.Wt >= 1 && g.Wf <= g.F &&
         (int64_t)g.B * g.Wf * g.Wt < (1ll << 31);
}

template <class Kernel, class Args>
int launch_gather(Kernel kernel, const Args& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  const int64_t M = (int64_t)a.g.B * a.g.Wf * a.g.Wt;
  const int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, st, a, out, lab_out, lab_w);
  return (int)hipGetLastError();
}

// The ring as a source (live.hip, live_gate.hip): window n = (j, a) exists while n is in [0, avail); it starts at
// fiber row fs[a] and time j * st (tend for the end-aligned index jend); time t is column t mod R.
struct RingSource {
  using time_type = int64_t;
  const LiveArgs& a;
  const int64_t avail, jend, tend;
  DEV explicit RingSource(const LiveArgs& a)
      : a(a), avail(a.state[LIVE_AVAIL]), jend(a.state[LIVE_JEND]), tend(a.state[LIVE_TEND]) {}
  DEV bool numbered(int64_t n, int& f0, int64_t& t0) const {
    if (n < 0 || n >= avail) return false;
    const int64_t wj = n / a.g.nf;
    f0 = a.g.fs[(int)(n - wj * a.g.nf)];
    t0 = wj == jend ? tend : wj * a.st;
    return t0 >= 0;
  }
  DEV int64_t column(int64_t t) const { return t % a.R; }
  DEV const float* base() const { return a.ring; }
  DEV int64_t pitch() const { return a.R; }
};

// the row of window n = (j, a) in a ring of Jcap time indices (the probability table, the gate's rings)
DEV int64_t ring_row(int nf, int Jcap, int64_t n) {
  const int64_t wj = n / nf;
  return (wj % Jcap) * nf + (n - wj * nf);
}

// what every launch over the ring requires of it
inline bool live_args_ok(const LiveArgs& a) {
  return a.state && a.ring && a.g.C >= 1 && a.g.F >= 1 && a.g.nf >= 1 && a.st >= 1 && a.g.Wt >= 1 &&
         a.R >= (int64_t)a.g.Wt + 1;
}

// the ring's selection brings its own batch cursor: all of sel, count and cursor, or none
inline bool live_selection_ok(const LiveArgs& a) {
  return selection_ok(a.s) && (a.s.sel == nullptr) == (a.cursor == nullptr);
}

// the 256 partial sums in a fixed tree order; every thread returns the total
DEV double block_sum(double v, double* s_red) {
  __syncthreads();  // (the previous sum's readers)
  s_red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
    __syncthreads();
  }
  return s_red[0];
}

// The power of the window at (f0, t0) of a source [C][F][pitch], by one block of 256 threads (s_red: 256 doubles of
// LDS): (1 / C) sum_c mean over the window of (x - mu_c)^2, mu_c the window's own mean in channel c.  Two passes with
// fp64 accumulators; element e of a plane is (e / Wt, e % Wt), threads along time; a fixed reduction order and one
// fp32 rounding, so the result does not depend on where the source keeps time t (src.column).  Every thread
// returns it.
template <class Source, class Time>
DEV float window_power_body(const Source& src, int C, int F, int Wf, int Wt, int f0, Time t0, double* s_red) {
  const int HW = Wf * Wt;
  const float* __restrict__ x = src.base();
  const int64_t pitch = src.pitch(), plane = (int64_t)F * pitch;
  double total = 0.0;
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ xc = x + c * plane + (int64_t)f0 * pitch;
    double acc = 0.0;
    for (int e = threadIdx.x; e < HW; e += 256) {
      const int h = e / Wt;
      acc += (double)xc[(int64_t)h * pitch + src.column(t0 + (e - h * Wt))];
    }
    const double mean = block_sum(acc, s_red) / (double)HW;
    acc = 0.0;
    for (int e = threadIdx.x; e < HW; e += 256) {
      const int h = e / Wt;
      const double d = (double)xc[(int64_t)h * pitch + src.column(t0 + (e - h * Wt))] - mean;
      acc += d * d;
    }
    total += block_sum(acc, s_red) / (double)HW;
  }
  return (float)(total / (double)C);
}

// The ordered selection's pieces (gate.hip select_windows, live_gate.hip live_select): blocks of 256 candidates
// count their set flags, one block turns the counts into exclusive prefix sums, and a candidate's place is the
// number of set flags before it.  No atomics, no block waits on another.

// lanes of the wave below this one whose bit is set in the ballot
DEV int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the number of set flags of the block (every thread of the 256 calls it; s_wave: 4 ints of LDS); thread 0's value
DEV int block_flag_count(bool on, int* s_wave) {
  const unsigned long long m = __ballot(on);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// The second of the three launches, one block (select_scan_kernel, gate.hip): the block counts become their exclusive
// prefix sums, the total becomes the count.
void launch_select_scan(int64_t* offs, int64_t nblocks, int64_t* count, hipStream_t st);

// The place of this thread's candidate among the set flags: those of the blocks before (block_off), of the block's
// waves before (the ballots' counts), of the wave's lanes below (mbcnt).  Every thread of the 256 calls it; the
// value is meaningful where ``on``.
DEV int64_t ranked_place(bool on, int64_t block_off, int* s_wave) {
  const unsigned long long m = __ballot(on);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int64_t at = block_off + lanes_below(m);
  for (int w = 0; w < wave; ++w) at += s_wave[w];
  return at;
}

// Column c of batch row r of the probability table.  softmax = 0 (Models A/B): src is logp [T][B][16] and the
// column is exp(logp[t][r][c - c0_t]) of the task t that owns it (nc[t] columns each, side by side).  softmax = 1
// (Model C): src is logits [B][K] and the row is their max-subtracted softmax; every thread of a row recomputes its
// max and sum (2 K expf) in the same order.
DEV float window_prob(const float* __restrict__ src, int softmax, int T, const int (&nc)[4], int K, int B, int r,
                      int c) {
  if (softmax) {
    const float* x = src + (int64_t)r * K;
    float mx = x[0];
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, x[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(x[k] - mx);
    return expf(x[c] - mx) / s;
  }
  int t = 0, c0 = 0;
  while (t + 1 < T && c >= c0 + nc[t]) c0 += nc[t++];
  return expf(src[((int64_t)t * B + r) * 16 + (c - c0)]);
}

// The class counts of the T <= 4 tasks as the probability kernels take them; false unless every count is in
// 1 .. 16 and they sum to K.  The softmax form has no tasks and packs zeros.
inline bool pack_ncls(int softmax, int T, const int* ncls, int K, int4& nc) {
  int sum = 0, v[4] = {0, 0, 0, 0};
  if (!softmax) {
    if (T < 1 || T > 4 || !ncls) return false;
    for (int t = 0; t < T; ++t) {
      if (ncls[t] < 1 || ncls[t] > 16) return false;
      v[t] = ncls[t];
      sum += ncls[t];
    }
    if (sum != K) return false;
  }
  nc = make_int4(v[0], v[1], v[2], v[3]);
  return true;
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

// The weight of window a in cell i of its axis.  The host computes a window's weights in fp64 and passes them as
// bands: window a reaches at most m = (win - 1) / cell + 2 cells from s[a] / cell on, and its weights for them are
// band[a * m ..].  False outside the band (a covering window's cell is inside it).
DEV bool band_weight(const int* __restrict__ s, const float* __restrict__ band, int m, int cell, int a, int i,
                     float& w) {
  const int d = i - s[a] / cell;
  if (d < 0 || d >= m) return false;
  w = band[(int64_t)a * m + d];
  return true;
}

// every sample of [0, len) is inside a window: starts strictly increasing, first at 0, no gap, last reaches len
inline bool starts_cover(const int* s, int n, int win, int len) {
  if (n < 1 || win < 1 || s[0] != 0 || s[n - 1] + (int64_t)win < len) return false;
  for (int i = 0; i < n; ++i) {
    if (s[i] < 0 || s[i] + (int64_t)win > len) return false;
    if (i && (s[i] <= s[i - 1] || s[i] > s[i - 1] + (int64_t)win)) return false;
  }
  return true;
}

}  // namespace mda
