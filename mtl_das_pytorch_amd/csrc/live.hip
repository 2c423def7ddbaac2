// Live inference on a growing recording (inference.py LiveRecording): the time axis of the recording is a ring.
//
// ring_append: a staged chunk [C][F][n] goes into the fp32 ring [C][F][R], time sample t at column t mod R, and the
//   device scalars total (samples received) and avail (window numbers that can be evaluated) advance.
// gather_windows_ring: gather_windows (window.hip) with the time column taken mod R.  Windows are numbered
//   time-major, n = j * nf + a (time index j starts at j * st, fiber start fs[a]), so new windows append at the end;
//   batch row r holds window next + r when that is below avail and is padding otherwise.
// live_probs: window_probs for that numbering, into a ring table [Jcap * nf][K] at row (j mod Jcap) * nf + a; it then
//   advances next by the number of valid rows, so the replays of one captured graph need no host copy between them.
// live_map: window_map's gather form for a range of final cell columns, read from the ring table.
//
// The end of the stream (flush) adds one end-aligned time index when (T - Wt) mod st != 0: its number jend and its
// start tend are device scalars too, so the captured gather serves it unchanged.
#include "kernels.h"

namespace mda {

// threads along the chunk's (and the ring's) contiguous time axis; the wrap at R falls where it falls
__global__ __launch_bounds__(256) void ring_append_kernel(LiveArgs a, const float* __restrict__ chunk, int n) {
  const int64_t total = a.state[LIVE_TOTAL];
  const int64_t M = (int64_t)a.C * a.F * n;
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
  const int64_t nj = total >= a.Wt ? (total - a.Wt) / a.st + 1 : 0;
  int64_t avail = nj * a.nf;
  if (flush && total >= a.Wt && (total - a.Wt) % a.st != 0) {  // the end-aligned time index
    a.state[LIVE_JEND] = nj;
    a.state[LIVE_TEND] = total - a.Wt;
    avail += a.nf;
  }
  a.state[LIVE_TOTAL] = total;
  a.state[LIVE_AVAIL] = avail;
}

static bool live_args_ok(const LiveArgs& a) {
  return a.state && a.C >= 1 && a.F >= 1 && a.nf >= 1 && a.st >= 1 && a.Wt >= 1 && a.R >= (int64_t)a.Wt + 1;
}

int launch_ring_append(const LiveArgs& a, const float* chunk, int n, int flush, hipStream_t st) {
  if (!live_args_ok(a) || !a.ring || n < 0 || (n > 0 && !chunk) || (n == 0 && !flush) || n > a.R - a.Wt) return -2;
  if (n > 0) {
    const int64_t M = (int64_t)a.C * a.F * n;
    const int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
    hipLaunchKernelGGL(ring_append_kernel, dim3(blocks), dim3(256), 0, st, a, chunk, n);
  }
  hipLaunchKernelGGL(ring_advance_kernel, dim3(1), dim3(64), 0, st, a, n, flush);
  return (int)hipGetLastError();
}

// The start of time index j: j * st, or tend for the end-aligned index.
DEV int64_t live_time_start(int64_t j, int st, int64_t jend, int64_t tend) { return j == jend ? tend : j * st; }

// gather_windows_kernel's pixel loop, tap packing and window-edge padding; the time column is taken mod R.  A
// padding row (window number at or past avail) is written as zeros and reads nothing.
__global__ __launch_bounds__(256) void gather_windows_ring_kernel(LiveArgs a, bf16_t* __restrict__ out,
                                                                  int64_t* __restrict__ lab_out, int lab_w) {
  const int64_t next = a.state[LIVE_NEXT], avail = a.state[LIVE_AVAIL];
  const int64_t jend = a.state[LIVE_JEND], tend = a.state[LIVE_TEND];
  const int HW = a.Wf * a.Wt;
  const int64_t M = (int64_t)a.B * HW;
  const int64_t FR = (int64_t)a.F * a.R;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < M; p += (int64_t)gridDim.x * 256) {
    const int b = (int)p / HW;  // M < 2^31 (checked by the launcher)
    const int r = (int)p - b * HW;
    const int h = r / a.Wt, w = r - h * a.Wt;
    const int64_t n = next + b;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (n >= 0 && n < avail) {
      const int64_t wj = n / a.nf;
      const int wa = (int)(n - wj * a.nf);
      const int f0 = a.fs[wa];
      const int64_t t0 = live_time_start(wj, a.st, jend, tend);
      if (f0 >= 0 && f0 + a.Wf <= a.F && t0 >= 0) {
        const int64_t col = (t0 + w) % a.R;
        if (a.taps > 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int hh = h - a.off + j;
            if (j < a.taps && hh >= 0 && hh < a.Wf) v[j] = a.ring[(int64_t)(f0 + hh) * a.R + col];
          }
        } else {
          const int64_t src = (int64_t)(f0 + h) * a.R + col;
#pragma unroll
          for (int c = 0; c < 8; ++c)
            if (c < a.C) v[c] = a.ring[c * FR + src];
        }
      }
    }
    store8(out + p * 8, v);
  }
  // the head kernels read labels for their metrics: inference has none
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.B * lab_w; i += 256) lab_out[i] = 0;
}

int launch_gather_windows_ring(const LiveArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st) {
  if (!live_args_ok(a) || !a.ring || !a.fs || !out || !lab_out || a.B < 1 || a.C > 8 || a.taps < 0 || a.taps > 8 ||
      (a.taps > 0 && a.C != 1) || a.Wf < 1 || a.Wf > a.F || lab_w < 0 || (int64_t)a.B * a.Wf * a.Wt >= (1ll << 31))
    return -2;
  const int64_t M = (int64_t)a.B * a.Wf * a.Wt;
  const int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
  hipLaunchKernelGGL(gather_windows_ring_kernel, dim3(blocks), dim3(256), 0, st, a, out, lab_out, lab_w);
  return (int)hipGetLastError();
}

// window_probs_kernel's two forms (one block; see there).  Row r of the batch is window next + r = (j, a) and goes to
// table row (j mod Jcap) * nf + a; padding rows are skipped.  next is advanced by thread 0 after every thread has
// read it (the block barrier).
__global__ __launch_bounds__(256) void live_probs_kernel(LiveArgs a, const float* __restrict__ src, int softmax, int T,
                                                         int4 ncls, int K, float* __restrict__ table, int Jcap) {
  const int64_t next = a.state[LIVE_NEXT], avail = a.state[LIVE_AVAIL];
  const int nc[4] = {ncls.x, ncls.y, ncls.z, ncls.w};
  for (int i = threadIdx.x; i < a.B * K; i += 256) {
    const int r = i / K, c = i - r * K;
    const int64_t n = next + r;
    if (n < 0 || n >= avail) continue;
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
    const int64_t wj = n / a.nf;
    const int64_t row = (wj % Jcap) * a.nf + (n - wj * a.nf);
    table[row * K + c] = p;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t left = avail - next;
    a.state[LIVE_NEXT] = next + (left < 0 ? 0 : left < a.B ? left : a.B);
  }
}

int launch_live_probs(const LiveArgs& a, const float* src, int softmax, int T, const int* ncls, int K, float* table,
                      int64_t nrows, int Jcap, hipStream_t st) {
  if (!a.state || !src || !table || K < 1 || a.B < 1 || a.nf < 1 || Jcap < 1 || nrows < (int64_t)Jcap * a.nf ||
      (int64_t)a.B * K >= (1ll << 31))
    return -2;
  int4 nc = make_int4(0, 0, 0, 0);
  if (!softmax) {
    if (T < 1 || T > 4 || !ncls) return -2;
    int sum = 0, v[4] = {0, 0, 0, 0};
    for (int t = 0; t < T; ++t) {
      if (ncls[t] < 1 || ncls[t] > 16) return -2;
      v[t] = ncls[t];
      sum += ncls[t];
    }
    if (sum != K) return -2;
    nc = make_int4(v[0], v[1], v[2], v[3]);
  }
  hipLaunchKernelGGL(live_probs_kernel, dim3(1), dim3(256), 0, st, a, src, softmax, T, nc, K, table, Jcap);
  return (int)hipGetLastError();
}

// One thread per (cell row i, final cell column q, class k), k fastest.  As window_map_kernel,
//   map[k][i][q] = sum_a sum_j wf[a, i] wt[q, j] table[(j mod Jcap) nf + a][k]
// in (a, j) order.  The fiber weights are window_map's bands; the time weights come per column: column q's covering
// time indices are the contiguous jlo[q] .. jlo[q] + jn[q] - 1 (the end-aligned index is the last regular one + 1)
// and their weights wt[q * mw ..].
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
    float acc = 0.f;
    for (int wa = 0; wa < a.nf; ++wa) {
      const int f0 = a.fs[wa];
      if (f0 + a.Wf <= r0 || f0 >= r1) continue;  // window a shares no row with the cell
      const int di = i - f0 / a.cf;
      if (di < 0 || di >= a.mf) continue;  // (a covering window's cell is inside its band)
      const float wf = a.wf[(int64_t)wa * a.mf + di];
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
      a.cf < 1 || a.F < 1 || a.Wf < 1 || a.nf < 1 || a.ncol < 1 || a.mw < 1 || a.Jcap < 1 ||
      nrows < (int64_t)a.Jcap * a.nf)
    return -2;
  if (a.mf != (a.Wf - 1) / a.cf + 2 || a.nfc != (a.F + a.cf - 1) / a.cf) return -2;
  // every fiber row is inside a window (as window_map requires), and a window is inside the recording
  if (h_fs[0] != 0 || h_fs[a.nf - 1] + (int64_t)a.Wf < a.F) return -2;
  for (int i = 0; i < a.nf; ++i) {
    if (h_fs[i] < 0 || h_fs[i] + (int64_t)a.Wf > a.F) return -2;
    if (i && (h_fs[i] <= h_fs[i - 1] || h_fs[i] > h_fs[i - 1] + (int64_t)a.Wf)) return -2;
  }
  // a column's time indices are distinct rows of the ring table
  for (int q = 0; q < a.ncol; ++q)
    if (h_jlo[q] < 0 || h_jn[q] < 1 || h_jn[q] > a.mw || h_jn[q] > a.Jcap) return -2;
  const int64_t total = (int64_t)a.nfc * a.ncol * a.K;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 65535);
  hipLaunchKernelGGL(live_map_kernel, dim3(blocks), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mda
