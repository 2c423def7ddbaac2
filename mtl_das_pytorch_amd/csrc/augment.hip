// SNR noise injected by the batch gather (training augmentation with fresh noise every step, SNR sweeps of one
// clean resident test set).  The definition lives in data/noise.py (numpy fp64); this file evaluates it in fp32.
//
// sample_power: P[s, c] = mean over the plane of (x - mean(x))^2, once per resident set, outside the step.
// gather_batch_noise: gather_batch (misc.hip) -- row selection by index or schedule cursor, bf16 NHWC-8 output with
//   the stem's vertical tap packing, label gather, ZeroRanges clear -- with every real element stored as
//   bf16(x + sigma * g); padding channels and out-of-image taps stay 0.
//     g(s, c, h, w) = BoxMuller(philox((h >> 2) * W + w, c | stream << 8, s, draw; seed))[h & 3]
//     sigma[s, c]   = sqrt(P[s, c] * 10^(-snr_s / 10)),  snr_s = lo + (hi - lo) * u01(philox(0, 1 << 8, s, draw).x)
//   One Philox call yields a VERTICAL quad of Gaussians, and one thread writes a vertical quad of output pixels:
//   the 4 + taps - 1 consecutive rows of its column that their tap-packed channels hold lie in at most four quads,
//   so a 7-tap pixel costs 3/4 of a Philox call (one pixel per thread would cost 2.5: every quad recomputed by the
//   ten pixels whose taps reach it).  The noise depends on (seed, draw, dataset row, c, h, w) only -- not on the
//   batch position or the launch geometry.  The levels, the draw number and the power table are device values.
//   The arguments are the clean gather's GatherArgs plus NoiseArgs; the schedule row, the clear, the label gather and
//   the limits both launchers share are stem_gather.h's.  The tap-packed store stays here (store_packed): it reads a
//   thread's 16-row register array, not the column.
// noise_advance: draw += 1 by one thread, launched after the gather (whose blocks all read the draw).
#include "kernels.h"
#include "philox.h"
#include "stem_gather.h"

namespace mda {

namespace {

// Box-Muller as in synth.hip: words (x, y) give m0 cos, m0 sin; words (z, w) give m1 cos, m1 sin
DEV void gauss_pair(uint32_t a, uint32_t b, float& gc, float& gs) {
  const float m = sqrtf(-2.f * logf(u01(a)));
  float s, c;
  sincosf(6.283185307179586f * u01(b), &s, &c);
  gc = m * c;
  gs = m * s;
}

DEV void gauss4(uint4 r, float* g) {
  gauss_pair(r.x, r.y, g[0], g[1]);
  gauss_pair(r.z, r.w, g[2], g[3]);
}

// sigma == 0 (a constant plane) returns x itself: the clean gather's bits, the sign of a zero included
DEV float noisy(float x, float sigma, float g) { return sigma > 0.f ? fmaf(sigma, g, x) : x; }

DEV float sigma_of(float P, const float* __restrict__ snr, uint32_t s, uint32_t d, uint2 key) {
  const float lo = snr[0], hi = snr[1];
  float level = lo;
  if (lo != hi) level = fmaf(hi - lo, u01(philox4x32_10(make_uint4(0u, 1u << 8, s, d), key).x), lo);
  return P > 0.f ? sqrtf(P * exp10f(-level / 10.f)) : 0.f;
}

__global__ __launch_bounds__(256) void sample_power_kernel(const float* __restrict__ X, float* __restrict__ power,
                                                           int HW) {
  // two passes with fp64 accumulators: the data is scaled by 100 and need not be centred
  const float* x = X + (int64_t)blockIdx.x * HW;
  __shared__ double s_red[256];
  double acc = 0.0;
  for (int e = threadIdx.x; e < HW; e += 256) acc += (double)x[e];
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
    __syncthreads();
  }
  const double mean = s_red[0] / (double)HW;
  __syncthreads();
  acc = 0.0;
  for (int e = threadIdx.x; e < HW; e += 256) {
    const double d = (double)x[e] - mean;
    acc += d * d;
  }
  s_red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) power[blockIdx.x] = (float)(s_red[0] / (double)HW);
}

// The tap-packed channels of the thread's four pixels (rows 4q + i) from Y, the noisy rows 4 qb .. 4 qb + 15 of the
// column (0 outside the image): channel j of pixel i is row 4q + i - off + j = 4 qb + C0 + i + j, C0 = (-off) mod 4
// (the same for every thread of the launch: all of Y's indices are compile-time).
template <int C0>
DEV void store_packed(const float* Y, int taps, int rows, bf16_t* __restrict__ out, int W) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i >= rows) break;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < taps ? Y[C0 + i + j] : 0.f;
    store8(out + (int64_t)i * W * 8, v);
  }
}

// One thread per (batch row, vertical quad q, column w), threads along w.  The 256 quads of a block belong to few
// batch rows (two at the models' image sizes): their sigmas -- one Philox call for the SNR draw, exp10f, sqrtf -- are
// computed once per block into LDS.
__global__ __launch_bounds__(256) void gather_batch_noise_kernel(GatherArgs a, NoiseArgs nz) {
  // (read before the clear, with the kernel's first argument loads: see gather_batch_kernel)
  const float* __restrict__ X = a.X;
  bf16_t* __restrict__ out = a.out;
  const int B = a.B, Cin = a.Cin, H = a.H, W = a.W, taps = a.taps, off = a.off;
  const int64_t* __restrict__ idx = schedule_row(a);
  clear_ranges(a.zero);
  const int HW = H * W;
  const int QW = ((H + 3) >> 2) * W;  // quads of one sample
  const int64_t M = (int64_t)B * QW;  // < 2^31 (the launcher checks B * H * W)
  const uint2 key = make_uint2((uint32_t)nz.seed, (uint32_t)(nz.seed >> 32));
  const uint32_t d32 = (uint32_t)*nz.draw;
  const uint32_t kword = (uint32_t)nz.stream << 8;
  const int c0 = (4 - (off & 3)) & 3;  // (-off) mod 4
  const int dq = (off + c0) >> 2;      // Y starts at quad q - dq: 4 (q - dq) = 4 q - off - c0
  __shared__ float s_sigma[256 * 8];   // [batch rows of the block's quads (<= 256)][Cin]
  for (int64_t base = (int64_t)blockIdx.x * 256; base < M; base += (int64_t)gridDim.x * 256) {
    const int b0 = (int)(base / QW);
    const int b1 = (int)(min(base + 255, M - 1) / QW);
    __syncthreads();  // (the previous round's readers)
    for (int i = threadIdx.x; i < (b1 - b0 + 1) * Cin; i += 256) {
      const int64_t src = idx[b0 + i / Cin];
      s_sigma[i] = sigma_of(nz.power[src * Cin + i % Cin], nz.snr, (uint32_t)src, d32, key);
    }
    __syncthreads();
    const int64_t p = base + threadIdx.x;
    if (p >= M) continue;
    const int b = (int)p / QW;
    const int r = (int)p - b * QW;
    const int q = r / W, w = r - q * W;
    const int rows = min(4, H - 4 * q);  // the thread's pixels: rows 4q .. 4q + rows - 1
    const int64_t src = idx[b];
    const uint32_t s32 = (uint32_t)src;
    const float* sg = s_sigma + (b - b0) * Cin;
    bf16_t* o = out + ((int64_t)b * HW + (int64_t)4 * q * W + w) * 8;
    if (taps > 0) {
      const float* x = X + src * (int64_t)HW + w;
      const float sig = sg[0];
      const int qb = q - dq;
      // the rows the four pixels' channels hold end at Y index c0 + 3 + taps - 1 (<= 13); the test hook also wants
      // the pixels' own rows, Y index c0 + off + i
      const int e_max = c0 + 3 + max(taps - 1, nz.dbg ? off : 0);
      float Y[16];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row0 = 4 * (qb + t);
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        const bool need = 4 * t <= e_max && row0 + 3 >= 0 && row0 < H;
        if (need && sig > 0.f)
          gauss4(philox4x32_10(make_uint4((uint32_t)((qb + t) * W + w), kword, s32, d32), key), g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = row0 + i;
          Y[4 * t + i] = (need && row >= 0 && row < H) ? noisy(x[row * W], sig, g[i]) : 0.f;
        }
      }
      switch (c0) {
        case 0: store_packed<0>(Y, taps, rows, o, W); break;
        case 1: store_packed<1>(Y, taps, rows, o, W); break;
        case 2: store_packed<2>(Y, taps, rows, o, W); break;
        default: store_packed<3>(Y, taps, rows, o, W); break;
      }
      if (nz.dbg) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (i >= rows) break;
          const int e = c0 + off + i;  // <= 13
          float val = 0.f;
#pragma unroll
          for (int k = 0; k < 16; ++k) val = e == k ? Y[k] : val;
          nz.dbg[(int64_t)b * HW + (4 * q + i) * W + w] = val;
        }
      }
    } else {
      float v[4][8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        const float sig = c < Cin ? sg[c] : 0.f;
        if (sig > 0.f) gauss4(philox4x32_10(make_uint4((uint32_t)r, (uint32_t)c | kword, s32, d32), key), g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float val = 0.f;
          if (c < Cin && i < rows) {
            val = noisy(X[(src * Cin + c) * (int64_t)HW + (4 * q + i) * W + w], sig, g[i]);
            if (nz.dbg) nz.dbg[((int64_t)b * Cin + c) * HW + (4 * q + i) * W + w] = val;
          }
          v[i][c] = val;
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < rows) store8(o + (int64_t)i * W * 8, v[i]);
    }
  }
  gather_labels(a, idx);
}

__global__ void noise_advance_kernel(int64_t* draw) { *draw += 1; }

}  // namespace

int launch_sample_power(const float* X, float* power, int64_t planes, int HW, hipStream_t st) {
  if (!X || !power || planes <= 0 || planes >= (1ll << 31) || HW <= 0) return -2;
  hipLaunchKernelGGL(sample_power_kernel, dim3((unsigned)planes), dim3(256), 0, st, X, power, HW);
  return (int)hipGetLastError();
}

int launch_gather_batch_noise(const GatherArgs& a, const NoiseArgs& noise, hipStream_t st) {
  if (!gather_args_ok(a)) return -2;  // (B, Cin >= 1: the block's sigma table has at least one entry)
  if (!noise.power || !noise.snr || !noise.draw || noise.stream < 0 || noise.stream > 255) return -2;
  if (a.taps > 0 && (a.off < 0 || a.off > 7)) return -2;  // the 16 rows a thread holds reach the taps (and the own rows)
  const int64_t M = (int64_t)a.B * ((a.H + 3) / 4) * a.W;  // one thread per vertical quad of pixels
  int blocks = (int)std::min<int64_t>((M + 255) / 256, 65535);
  hipLaunchKernelGGL(gather_batch_noise_kernel, dim3(blocks), dim3(256), 0, st, a, noise);
  return (int)hipGetLastError();
}

int launch_noise_advance(int64_t* draw, hipStream_t st) {
  if (!draw) return -2;
  hipLaunchKernelGGL(noise_advance_kernel, dim3(1), dim3(1), 0, st, draw);
  return (int)hipGetLastError();
}

}  // namespace mda
