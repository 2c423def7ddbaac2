// Raw-rate recordings (data/resample.py): an anti-alias FIR and decimation by an integer factor along time, ahead
// of the ring of live.hip.  With the taps h[0 .. L-1] and the factor D,
//
//   y[row][k] = sum_{i = 0}^{L-1} h[i] * s[row][k D + (L - 1) - i]
//
// in the "valid" form.  A launch serves one piece of a stream: its samples s are the carried tail of the pieces
// before it (carry_in, carry_len columns per row: the raw samples from the next output's support on) followed by
// raw[skip ..] (skip > 0 only when D > L, and then nothing is carried).  It writes the m outputs that s completes
// and the new tail s[m D ..] into carry_out, another buffer than carry_in: the host flips the two.
//
// fir_decimate_kernel: one block per (row, tile of DECIMATE_TILE outputs).  The tile's span of
//   (DECIMATE_TILE - 1) D + L samples is read once, coalesced along time (fp32, or int16 converted exactly), and
//   stored in LDS de-interleaved by phase, s_x[p][q] = s[base + q D + p]: tap j = a D + p of output k is
//   s_x[p][k + a], so for every tap the lanes' reads are unit stride whatever D is.  The row length Q is odd, which
//   spreads the staging writes (lane stride Q or 1) over the banks.  The taps sit in LDS behind the tile.  A thread
//   owns DECIMATE_TILE / DECIMATE_THREADS outputs one thread count apart and reads each tap once for all of them.
//   Every output is one fp32 fma chain over the taps in the order i = 0 .. L-1, from 0: the bits of an output do
//   not depend on the tile, the piece or the launch that produces it.
// fir_tail_kernel: the new tail, rows x (at most L - 1) columns.
#include "kernels.h"

namespace mda {

namespace {

constexpr int FIR_OPT = DECIMATE_TILE / DECIMATE_THREADS;  // outputs per thread

// length of a phase row of the staged tile: the span's ceil(. / D), made odd
__host__ __device__ inline int fir_phase_row(int D, int L) { return (((DECIMATE_TILE - 1) * D + L + D - 1) / D) | 1; }

// sample g of row `row` of the piece's stream: the carry first, then the raw samples from `skip` on
template <typename T>
DEV float fir_sample(const FirArgs& a, const T* __restrict__ raw, int64_t row, int64_t g) {
  return g < a.carry_len ? a.carry_in[row * (a.L - 1) + g] : (float)raw[row * a.pitch + a.skip + (g - a.carry_len)];
}

template <typename T>
__global__ __launch_bounds__(DECIMATE_THREADS) void fir_decimate_kernel(FirArgs a, const T* __restrict__ raw) {
  extern __shared__ float s_fir[];
  const int D = a.D, L = a.L;
  const int Q = fir_phase_row(D, L);
  float* s_x = s_fir;          // [D][Q]
  float* s_h = s_fir + D * Q;  // [L]
  const int tiles = (int)((a.m + DECIMATE_TILE - 1) / DECIMATE_TILE);
  const int64_t row = (int64_t)blockIdx.x / tiles;
  const int k0 = (int)((int64_t)blockIdx.x - row * tiles) * DECIMATE_TILE;
  const int64_t ns = a.carry_len + (a.n > a.skip ? a.n - a.skip : 0);  // samples of the piece's stream
  const int64_t base = (int64_t)k0 * D;
  const int span = (DECIMATE_TILE - 1) * D + L;
  const int cnt = (int)(ns - base < span ? ns - base : span);

  for (int i = threadIdx.x; i < L; i += DECIMATE_THREADS) s_h[i] = a.taps[i];
  {  // r = q D + p walks the span DECIMATE_THREADS at a time; (q, p) follow without a division per sample
    const int dq = DECIMATE_THREADS / D, dp = DECIMATE_THREADS % D;
    int q = threadIdx.x / D, p = threadIdx.x % D;
    for (int r = threadIdx.x; r < cnt; r += DECIMATE_THREADS) {
      s_x[p * Q + q] = fir_sample(a, raw, row, base + r);
      q += dq;
      p += dp;
      if (p >= D) { p -= D; ++q; }
    }
  }
  __syncthreads();

  float acc[FIR_OPT];
#pragma unroll
  for (int u = 0; u < FIR_OPT; ++u) acc[u] = 0.f;
  const float* x0 = s_x + threadIdx.x;
  int i = 0;
  int p = (L - 1) % D;
  for (int t = (L - 1) / D; t >= 0; --t) {  // tap j = t D + p, from L - 1 down: i = L - 1 - j goes up
    for (; p >= 0; --p, ++i) {
      const float h = s_h[i];
      const float* x = x0 + p * Q + t;
#pragma unroll
      for (int u = 0; u < FIR_OPT; ++u) acc[u] = fmaf(h, x[u * DECIMATE_THREADS], acc[u]);
    }
    p = D - 1;
  }
#pragma unroll
  for (int u = 0; u < FIR_OPT; ++u) {
    const int k = k0 + u * DECIMATE_THREADS + threadIdx.x;
    if (k < a.m) a.out[row * a.m + k] = acc[u];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fir_tail_kernel(FirArgs a, const T* __restrict__ raw, int len) {
  const int64_t total = a.rows * len;
  const int64_t first = a.m * a.D;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
    const int64_t row = g / len;
    const int c = (int)(g - row * len);
    a.carry_out[row * (a.L - 1) + c] = fir_sample(a, raw, row, first + c);
  }
}

template <typename T>
int launch_fir(const FirArgs& a, int tail, hipStream_t st) {
  const T* raw = static_cast<const T*>(a.raw);
  if (a.m > 0) {
    const int64_t blocks = a.rows * ((a.m + DECIMATE_TILE - 1) / DECIMATE_TILE);
    const size_t lds = sizeof(float) * ((size_t)a.D * fir_phase_row(a.D, a.L) + a.L);
    hipLaunchKernelGGL(fir_decimate_kernel<T>, dim3((unsigned)blocks), dim3(DECIMATE_THREADS), lds, st, a, raw);
  }
  if (tail > 0) {
    const int blocks = (int)std::min<int64_t>((a.rows * tail + 255) / 256, 65535);
    hipLaunchKernelGGL(fir_tail_kernel<T>, dim3(blocks), dim3(256), 0, st, a, raw, tail);
  }
  return (int)hipGetLastError();
}

}  // namespace

int64_t fir_output_count(int64_t carry_len, int64_t skip, int64_t n, int L, int D) {
  const int64_t ns = carry_len + (n > skip ? n - skip : 0);
  return ns >= L ? (ns - L) / D + 1 : 0;
}

int launch_fir_decimate(const FirArgs& a, int itype, hipStream_t st) {
  if (a.D < 1 || a.D > DECIMATE_MAX_FACTOR || a.L < 1 || a.L > DECIMATE_MAX_TAPS) return -2;
  if (itype != FIR_F32 && itype != FIR_I16) return -2;
  if (a.rows < 1 || a.n < 0 || a.pitch < a.n || a.n >= (1ll << 31) || a.skip < 0 || a.carry_len < 0 ||
      a.carry_len > a.L - 1 || (a.skip > 0 && a.carry_len > 0))
    return -2;
  if (a.m < 0 || a.m != fir_output_count(a.carry_len, a.skip, a.n, a.L, a.D)) return -2;
  const int64_t ns = a.carry_len + (a.n > a.skip ? a.n - a.skip : 0);
  const int64_t left = ns - a.m * a.D;  // below L by the count; negative: the next support starts later
  const int tail = (int)(left > 0 ? left : 0);
  if (!a.taps || (a.n > 0 && !a.raw) || (a.m > 0 && !a.out) || (a.carry_len > 0 && !a.carry_in) ||
      (tail > 0 && !a.carry_out))
    return -2;
  if (a.carry_len > 0 && tail > 0 && a.carry_in == a.carry_out) return -2;  // read and written by different blocks
  if (a.rows * ((a.m + DECIMATE_TILE - 1) / DECIMATE_TILE) >= (1ll << 31)) return -2;
  if (a.m == 0 && tail == 0) return 0;
  return itype == FIR_I16 ? launch_fir<int16_t>(a, tail, st) : launch_fir<float>(a, tail, st);
}

}  // namespace mda
