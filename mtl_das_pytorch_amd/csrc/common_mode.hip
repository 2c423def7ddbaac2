// Common-mode removal ahead of the windows (data/common_mode.py): for every channel c and time sample t one value
// m[c][t] over the fiber is subtracted from all F positions,
//
//   out[c][f][t] = x[c][f][t] - m[c][t]        (one fp32 subtraction)
//
// m is the lower median, sorted(x[c][:][t])[(F - 1) / 2] with NaN last and a zero of either sign taken as +0, or
// the mean, an fp64 sum over f = 0 .. F-1 in that order divided by F and rounded to fp32.  Both are exactly the
// definition's bits: the median is an element of its column, the mean the same additions in the same order.
//
// common_mode_kernel: one block per (channel, tile of COMMON_MODE_TILE consecutive time columns); a thread is
//   (column tx, row group ty), so a wave reads two rows' segments of the tile, each coalesced along time.  A block
//   owns its columns in all three steps, so out may be x: no block reads what another writes.
//   median: a radix selection on the order-preserving 32-bit key of the float (NaN: the largest key), four 8-bit
//     passes from the top.  Each pass counts, per column, the digits of the keys that share the prefix found so
//     far -- integer LDS atomics into s_w[digit][column], where the lanes of a row land on different banks whatever
//     their digits -- then finds the digit that holds the wanted rank: every thread sums one group of digits, the
//     column's first thread walks the groups and then the group's digits.  The work is linear in F, and x is read
//     from memory (from L2 after the first pass) four times and once more to subtract.
//   mean: slabs of 256 rows are staged in s_w, coalesced, and the column's first thread adds them in row order to
//     its fp64 accumulator.
#include "kernels.h"

namespace mda {

namespace {

constexpr int CM_TILE = COMMON_MODE_TILE;
constexpr int CM_THREADS = COMMON_MODE_THREADS;
constexpr int CM_GROUPS = CM_THREADS / CM_TILE;  // row groups of the block; digit groups of the scan
constexpr int CM_BINS = 256;                     // digits of a pass; rows of a slab of the mean
constexpr int CM_PER_GROUP = CM_BINS / CM_GROUPS;

// ascending keys for ascending floats: -inf < .. < -0 < +0 < .. < +inf < NaN (all NaNs share the largest key)
DEV uint32_t cm_key(uint32_t u) {
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the float of a key; the largest key gives 0x7fffffff, a NaN
DEV uint32_t cm_unkey(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

template <int HOW>
__global__ __launch_bounds__(CM_THREADS) void common_mode_kernel(CommonModeArgs a) {
  __shared__ uint32_t s_w[CM_BINS * CM_TILE];  // median: counts [digit][column]; mean: sample bits [row][column]
  __shared__ uint32_t s_part[CM_GROUPS * CM_TILE];
  __shared__ uint32_t s_prefix[CM_TILE], s_rank[CM_TILE];
  __shared__ float s_m[CM_TILE];
  const int tx = threadIdx.x % CM_TILE, ty = threadIdx.x / CM_TILE;
  const int64_t tiles = (a.n + CM_TILE - 1) / CM_TILE;
  const int64_t c = (int64_t)blockIdx.x / tiles;
  const int64_t t = ((int64_t)blockIdx.x - c * tiles) * CM_TILE + tx;
  const bool live = t < a.n;  // the other threads touch no memory but keep the barriers
  const int64_t F = a.F;
  const int64_t xo = c * F * a.pitch + t, oo = c * F * a.out_pitch + t;
  const uint32_t* xb = reinterpret_cast<const uint32_t*>(a.x);

  if (HOW == COMMON_MODE_MEDIAN) {
    if (ty == 0) {
      s_prefix[tx] = 0u;
      s_rank[tx] = (uint32_t)((F - 1) / 2);
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = threadIdx.x; i < CM_BINS * CM_TILE; i += CM_THREADS) s_w[i] = 0u;
      __syncthreads();
      const uint32_t prefix = s_prefix[tx];
      const uint32_t mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);  // the digits already found
      if (live) {
#pragma unroll 4
        for (int64_t f = ty; f < F; f += CM_GROUPS) {
          const uint32_t key = cm_key(xb[xo + f * a.pitch]);
          if ((key & mask) == prefix) atomicAdd(&s_w[((key >> shift) & 255u) * CM_TILE + tx], 1u);
        }
      }
      __syncthreads();
      {
        uint32_t s = 0u;
        for (int b = 0; b < CM_PER_GROUP; ++b) s += s_w[(ty * CM_PER_GROUP + b) * CM_TILE + tx];
        s_part[ty * CM_TILE + tx] = s;
      }
      __syncthreads();
      if (ty == 0) {  // the keys counted number more than the rank left, so both walks stop inside their range
        uint32_t k = s_rank[tx];
        int g = 0;
        for (; g < CM_GROUPS - 1; ++g) {
          const uint32_t s = s_part[g * CM_TILE + tx];
          if (k < s) break;
          k -= s;
        }
        int b = g * CM_PER_GROUP;
        for (; b < g * CM_PER_GROUP + CM_PER_GROUP - 1; ++b) {
          const uint32_t s = s_w[b * CM_TILE + tx];
          if (k < s) break;
          k -= s;
        }
        s_prefix[tx] = prefix | ((uint32_t)b << shift);
        s_rank[tx] = k;
      }
      __syncthreads();  // the next pass clears the counts this one walked
    }
    if (ty == 0) {
      uint32_t u = cm_unkey(s_prefix[tx]);
      if ((u & 0x7fffffffu) == 0u) u = 0u;  // a zero of either sign: +0
      s_m[tx] = __uint_as_float(u);
    }
  } else {
    double acc = 0.0;
    for (int64_t f0 = 0; f0 < F; f0 += CM_BINS) {
      const int rows = (int)(F - f0 < CM_BINS ? F - f0 : CM_BINS);
      if (live) {
#pragma unroll 4
        for (int r = ty; r < rows; r += CM_GROUPS) s_w[r * CM_TILE + tx] = xb[xo + (f0 + r) * a.pitch];
      }
      __syncthreads();
      if (ty == 0 && live) {
        for (int r = 0; r < rows; ++r) acc += (double)__uint_as_float(s_w[r * CM_TILE + tx]);
      }
      __syncthreads();
    }
    if (ty == 0) s_m[tx] = (float)(acc / (double)F);
  }
  __syncthreads();

  if (live) {
    const float m = s_m[tx];
#pragma unroll 4
    for (int64_t f = ty; f < F; f += CM_GROUPS) a.out[oo + f * a.out_pitch] = a.x[xo + f * a.pitch] - m;
    if (ty == 0 && a.trace) a.trace[c * a.n + t] = m;
  }
}

// do [p, p + np) and [q, q + nq) floats share an address
bool cm_overlap(const float* p, int64_t np, const float* q, int64_t nq) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)nq * sizeof(float) && b < a + (uintptr_t)np * sizeof(float);
}

}  // namespace

int launch_common_mode(const CommonModeArgs& a, int how, hipStream_t st) {
  if (how != COMMON_MODE_MEDIAN && how != COMMON_MODE_MEAN) return -2;
  if (a.rows < 1 || a.F < 1 || a.F > COMMON_MODE_MAX_F || a.n < 0 || a.n >= (1ll << 31) || a.pitch < a.n ||
      a.out_pitch < a.n)
    return -2;
  const int64_t tiles = (a.n + CM_TILE - 1) / CM_TILE;
  if (a.rows >= (1ll << 31) || a.rows * tiles >= (1ll << 31)) return -2;
  // element offsets stay below 2^63
  if (a.rows * a.F >= (1ll << 32) || a.pitch >= (1ll << 31) || a.out_pitch >= (1ll << 31)) return -2;
  if (!a.x || !a.out) return -2;
  if (a.n == 0) return 0;
  // the floats from the first live one to the last
  const int64_t xs = (a.rows * a.F - 1) * a.pitch + a.n, os = (a.rows * a.F - 1) * a.out_pitch + a.n;
  if (a.out == a.x ? a.out_pitch != a.pitch : cm_overlap(a.x, xs, a.out, os)) return -2;  // in place, or apart
  if (a.trace && (cm_overlap(a.trace, a.rows * a.n, a.x, xs) || cm_overlap(a.trace, a.rows * a.n, a.out, os)))
    return -2;
  const dim3 grid((unsigned)(a.rows * tiles)), block(CM_THREADS);
  if (how == COMMON_MODE_MEDIAN)
    hipLaunchKernelGGL(common_mode_kernel<COMMON_MODE_MEDIAN>, grid, block, 0, st, a);
  else
    hipLaunchKernelGGL(common_mode_kernel<COMMON_MODE_MEAN>, grid, block, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace mda
