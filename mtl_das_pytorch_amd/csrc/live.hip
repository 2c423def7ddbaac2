// Live inference on a growing recording (inference.py LiveRecording): the time axis of the recording is a ring.
//
// ring_append: a staged chunk [C][F][n] goes into the fp32 ring [C][F][R], time sample t at column t mod R, and the
//   device scalars total (samples received) and avail (window numbers that can be evaluated) advance.
// gather_windows_ring: the gather body of window_batch.h with the time column taken mod R.  Windows are numbered
//   time-major, n = j * nf + a (time index j starts at j * st, fiber start fs[a]), so new windows append at the end;
//   batch row r holds window next + r when that is below avail and is padding otherwise.
// live_probs: the probability element of window_batch.h for that numbering, into a ring table [Jcap * nf][K] at row
//   (j mod Jcap) * nf + a; it then advances next by the number of valid rows, so the replays of one captured graph
//   need no host copy between them.
// Both take the batch rows numbered by a live selection (LiveArgs::s and cursor, written by live_gate.hip's
//   live_select) instead: row r is window sel[cursor * B + r] while that entry is below the count.  The gated table
//   has K + 1 columns -- the probabilities and 1.0 for an evaluated window, so live_map serves the gated map with
//   K + 1 classes -- and the store advances the cursor by one.
// live_map: the gather form of the cell map (window.hip window_map_kernel) for a range of final cell columns, read
//   from the ring table.
//
// The end of the stream (flush) adds one end-aligned time index when (T - Wt) mod st != 0: its number jend and its
// start tend are device scalars too, so the captured gather serves it unchanged.
#include "window_batch.h"

namespace mda {

// threads along the chunk's (and the ring's) contiguous time axis; the wrap at R falls where it falls
__global__ __launch_bounds__(256) void ring_append_kernel(LiveArgs a, const float* __restrict__ chunk, int n) {
  const int64_t total = a.state[LIVE_TOTAL];
  const int64_t M = (int64_t)a.g.C * a.g.F * n;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < M; g += (int64_t)gridDim.x * 256) {
    const int64_t row = g / n;
    const int i = (int)(g - row * n);
    a.ring[row * a.R + (total + i) % a.R] = chunk[g];
  }
}

// One thread, after the copy (every block of the copy reads total): total += n, avail from the new total.
__global__ void ring_advance_kernel(LiveArgs a, int n, int flush) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t total = a.state[LIVE_TOTAL] + n;
  const int64_t nj = total >= a.g.Wt ? (total - a.g.Wt) / a.st + 1 : 0;
  int64_t avail = nj * a.g.nf;
  if (flush && total >= a.g.Wt && (total - a.g.Wt) % a.st != 0) {  // the end-aligned time index
    a.state[LIVE_JEND] = nj;
    a.state[LIVE_TEND] = total - a.g.Wt;
    avail += a.g.nf;
  }
  a.state[LIVE_TOTAL] = total;
  a.state[LIVE_AVAIL] = avail;
}

int launch_ring_append(const LiveArgs& a, const float* chunk, int n, int flush, hipStream_t st) {
  if (!live_args_ok(a) || n < 0 || (n > 0 && !chunk) || (n == 0 && !flush) || n > a.R - a.g.Wt) return -2;
  if (n > 0) {
    const int64_t M = (int64_t)a.g.C * a.g.F * n;
    const int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
    hipLaunchKernelGGL(ring_append_kernel, dim3(blocks), dim3(256), 0, st, a, chunk, n);
  }
  hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(64), 0, st, a, n, flush);
  return (int)hipGetLastError();
}

// The window number of batch row r: next + r, or the selection's entry in replay *cursor (-1: padding).
struct RingNumbering {
  const LiveArgs& a;
  const int64_t first, count;  // next, or the selection's batch cursor and count
  DEV explicit RingNumbering(const LiveArgs& a)
      : a(a), first(a.s.sel ? *a.cursor : a.state[LIVE_NEXT]), count(a.s.sel ? *a.s.count : 0) {}
  DEV int64_t operator()(int r) const {
    return a.s.sel ? selected_number(a.s, first, count, a.g.B, r) : first + r;
  }
};

// The ring as a gather source is window_batch.h's RingSource.
__global__ __launch_bounds__(256) void gather_windows_ring_kernel(LiveArgs a, bf16_t* __restrict__ out,
                                                                  int64_t* __restrict__ lab_out, int lab_w) {
  gather_windows_body(a.g, RingSource(a), RingNumbering(a), out, lab_out, lab_w);
}

int launch_gather_windows_ring(const LiveArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  if (!live_args_ok(a) || !gather_geom_ok(a.g, out, lab_out, lab_w) || !live_selection_ok(a)) return -2;
  return launch_gather(gather_windows_ring_kernel, a, out, lab_out, lab_w, st);
}

// One block, as window_probs_kernel.  Row r of the batch is window (j, a) and goes to table row
// (j mod Jcap) * nf + a; padding rows are skipped.  Without a selection the table's pitch is K and next advances by
// the valid rows; with one it is K + 1, column K of an evaluated window is 1, and the cursor advances by one.
// Thread 0 advances after every thread has read the counter (the block barrier).
__global__ __launch_bounds__(256) void live_probs_kernel(LiveArgs a, const float* __restrict__ src, int softmax, int T,
                                                         int4 ncls, int K, float* __restrict__ table, int pitch,
                                                         int Jcap) {
  const RingNumbering num(a);
  const int64_t avail = a.state[LIVE_AVAIL];
  const int nc[4] = {ncls.x, ncls.y, ncls.z, ncls.w};
  for (int i = threadIdx.x; i < a.g.B * pitch; i += 256) {
    const int r = i / pitch, c = i - r * pitch;
    const int64_t n = num(r);
    if (n < 0 || n >= avail) continue;
    table[ring_row(a.g.nf, Jcap, n) * pitch + c] = c < K ? window_prob(src, softmax, T, nc, K, a.g.B, r, c) : 1.f;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (a.s.sel) {
    *a.cursor = num.first + 1;
  } else {
    const int64_t left = avail - num.first;
    a.state[LIVE_NEXT] = num.first + (left < 0 ? 0 : left < a.g.B ? left : a.g.B);
  }
}

int launch_live_probs(const LiveArgs& a, const float* src, int softmax, int T, const int* ncls, int K, float* table,
                      int64_t nrows, int pitch, int Jcap, hipStream_t st) {
  int4 nc;
  if (!a.state || !live_selection_ok(a) || !src || !table || K < 1 || pitch != K + (a.s.sel ? 1 : 0) || a.g.B < 1 ||
      a.g.nf < 1 || Jcap < 1 || nrows < (int64_t)Jcap * a.g.nf || (int64_t)a.g.B * pitch >= (1ll << 31) ||
      !pack_ncls(softmax, T, ncls, K, nc))
    return -2;
  hipLaunchKernelGGL(live_probs_kernel, dim3(1), dim3(256), 0, st, a, src, softmax, T, nc, K, table, pitch, Jcap);
  return (int)hipGetLastError();
}

// One thread per (cell row i, final cell column q, class k), k fastest.  As window_map_kernel,
//   map[k][i][q] = sum_a sum_j wf[a, i] wt[q, j] table[(j mod Jcap) nf + a][k]
// in (a, j) order over the cell's covering fiber windows, found and weighted as there.  The time weights come per
// column: column q's covering time indices are the contiguous jlo[q] .. jlo[q] + jn[q] - 1 (the end-aligned index is
// the last regular one + 1) and their weights wt[q * mw ..].
__global__ __launch_bounds__(256) void live_map_kernel(LiveMapArgs a) {
  const int64_t total = (int64_t)a.nfc * a.ncol * a.K;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int k = (int)(g % a.K);
    const int64_t cell = g / a.K;
    const int i = (int)(cell / a.ncol), q = (int)(cell - (int64_t)i * a.ncol);
    const int r0 = i * a.cf, r1 = min(r0 + a.cf, a.F);
    const int64_t j0 = a.jlo[q];
    const int nj = a.jn[q];
    const float* wt = a.wt + (int64_t)q * a.mw;
    int a0, a1;
    covering_range(a.fs, a.nf, a.Wf, r0, r1, a0, a1);
    float acc = 0.f;
    for (int wa = a0; wa < a1; ++wa) {
      float wf;
      if (!band_weight(a.fs, a.wf, a.mf, a.cf, wa, i, wf)) continue;
      for (int jj = 0; jj < nj; ++jj) {
        const int64_t row = ((j0 + jj) % a.Jcap) * a.nf + wa;
        acc += (wf * wt[jj]) * a.table[row * a.K + k];
      }
    }
    a.map[((int64_t)k * a.nfc + i) * a.ncol + q] = acc;
  }
}

int launch_live_map(const LiveMapArgs& a, int64_t nrows, const int* h_fs, const int64_t* h_jlo, const int* h_jn,
                    hipStream_t st) {
  if (!a.table || !a.map || !a.fs || !a.wf || !a.wt || !a.jlo || !a.jn || !h_fs || !h_jlo || !h_jn || a.K < 1 ||
      a.cf < 1 || a.F < 1 || a.ncol < 1 || a.mw < 1 || a.Jcap < 1 || nrows < (int64_t)a.Jcap * a.nf)
    return -2;
  if (a.mf != (a.Wf - 1) / a.cf + 2 || a.nfc != (a.F + a.cf - 1) / a.cf) return -2;
  // every fiber row is inside a window (as window_map requires), and a window is inside the recording
  if (!starts_cover(h_fs, a.nf, a.Wf, a.F)) return -2;
  // a column's time indices are distinct rows of the ring table
  for (int q = 0; q < a.ncol; ++q)
    if (h_jlo[q] < 0 || h_jn[q] < 1 || h_jn[q] > a.mw || h_jn[q] > a.Jcap) return -2;
  const int64_t total = (int64_t)a.nfc * a.ncol * a.K;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(live_map_kernel, dim3(blocks), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mda
