// Pieces shared by the forward / data-gradient convolution kernels: conv_igemm_kernel (conv.hip),
// conv_lds_kernel and conv_glds_kernel (conv_lds.hip), conv_patch_kernel and conv_patchp_kernel
// (conv_patch.hip); the weight-gradient kernels of conv.hip use the normalise-on-load transform (wgrad_lean.hip
// keeps its own copy: through the helper its 128x64 batched kernel grows from 216 to 236 VGPRs, 2 -> 1 waves).
//
//   * the dynamic-LDS layout of each kernel family: ONE function gives the offset of every region and the
//     total bytes, called by the kernel's carve-up and by its host launcher, so the two cannot disagree;
//   * prologue: operand base pointers, the k-group encoder of the im2col kernels (weight gradients included) with
//     its field widths, the BN-backward constants of the fused-statistics data gradient;
//   * main loop: accumulator zero, the FN x FM MFMA step (MFMA_STEP), the 8-wide normalise-on-load transform;
//   * epilogue: the block reduction of the statistics with the fp64 replica atomics, and the output tile of the
//     LDS-staged kernels (split-K ticket reduction, stores, dz of a BN tail and its three sums).
#pragma once
#include "kernels.h"

namespace mda {

template <int MODE>
constexpr bool is_fwd() { return MODE == MODE_FWD || MODE == MODE_FWD_NOL; }

// ---------------------------------------------------------------------------------------------
// Dynamic LDS layouts (byte offsets)
// ---------------------------------------------------------------------------------------------
constexpr int CONV_LDS_MAX = 160 * 1024;  // LDS of a CU: the most one block may ask for

// floats of per-block constants: normalise-on-load [2][Cs] scale, shift / fused BN statistics [8][BN]
__host__ __device__ constexpr int conv_nconst(int mode, int Cs, int BN) {
  return mode == MODE_FWD_NOL ? 2 * Cs : (mode == MODE_DGRAD_BNS ? 8 * BN : 0);
}

// tail of every family's layout: [WAM][BN][3] epilogue sums, the constants, the split-K arrival flag (16 bytes)
struct TileLds { int st, k, flag, bytes; };
__host__ __device__ constexpr TileLds tile_lds(int off, int WAM, int BN, int nconst) {
  const int k = off + WAM * BN * 3 * 4, flag = k + nconst * 4;
  return TileLds{off, k, flag, flag + 16};
}

// conv_lds_kernel (nst = 2, KC = 64 / 128) and conv_glds_kernel (nst ring stages, KC = 64): the stages of
// (BN + BM) rows x KC bf16, then the two k-group tables of ntab entries (input coordinates, weight column)
struct IgemmLds { int tx, tw; TileLds t; };
__host__ __device__ constexpr IgemmLds igemm_lds(int BM, int BN, int WAM, int KC, int nst, int ntab, int nconst) {
  const int tx = nst * (BN + BM) * KC * 2, tw = tx + ntab * 4;
  return IgemmLds{tx, tw, tile_lds(tw + ntab * 4, WAM, BN, nconst)};
}

// patch kernels: K steps of a 9-tap x CB-channel weight slice, and its LDS row pitch (elements)
__host__ __device__ constexpr int pt_ksteps(int CB) { return (9 * CB + 31) / 32; }
__host__ __device__ constexpr int pt_wkp(int CB) { return pt_ksteps(CB) * 32 + 8; }
// conv_patch_kernel: one strip of (R + 2) x (Wout + 2) pixels with rows padded to CB + 8 channels
__host__ __device__ constexpr int patch_strip_bytes(int R, int Wout, int CB) { return (R + 2) * (Wout + 2) * (CB + 8) * 2; }
// conv_patchp_kernel: one dense strip buffer, whole 1-KB DMA instructions (it has two)
__host__ __device__ constexpr int patchp_strip_bytes(int R, int Wout, int CB) {
  return ((R + 2) * (Wout + 2) * (CB / 8) + 63) / 64 * 1024;
}
// strip_bytes of strip buffers (all of them), then the weight slice [BN][pt_wkp(CB)]
struct PatchLds { int w; TileLds t; };
__host__ __device__ constexpr PatchLds patch_lds(int strip_bytes, int BN, int WAM, int CB, int nconst) {
  return PatchLds{strip_bytes, tile_lds(strip_bytes + BN * pt_wkp(CB) * 2, WAM, BN, nconst)};
}

// ---------------------------------------------------------------------------------------------
// Prologue
// ---------------------------------------------------------------------------------------------
// group z's weight image and the (up to two) segments of the source
struct ConvBases {
  const bf16_t *wz, *base0, *base1;
  int ld0, ld1;
};
DEV ConvBases conv_bases(const ConvArgs& a, int z) {
  const bf16_t* base0 = a.src.p[0] + a.src.gs[0] * z;
  return ConvBases{a.w + a.wgs * z, base0, a.src.p[1] ? a.src.p[1] + a.src.gs[1] * z : base0, a.src.ld[0], a.src.ld[1]};
}
// 16 bytes of source pixel (b, ih, iw), channel c of segment seg
DEV const bf16_t* conv_src(const ConvArgs& a, const ConvBases& s, int seg, int b, int ih, int iw, int c) {
  return (seg ? s.base1 : s.base0) + ((int64_t)(b * a.Hs + ih) * a.Ws + iw) * (seg ? s.ld1 : s.ld0) + c;
}

// im2col column group i (8 channels of one tap) as conv_igemm and the im2col weight-gradient blocks table it:
// channel offset within its source segment | kw << 14 | kh << 21 | segment << 28 | valid << 29 (0: the group lies
// past the reduction -- stages zeros).  The decoders spell the masks out (e & 16383, (e >> 14) & 127).
constexpr int KG_CH_BITS = 14, KG_TAP_BITS = 7;
constexpr int KG_KW_SHIFT = KG_CH_BITS, KG_KH_SHIFT = KG_KW_SHIFT + KG_TAP_BITS, KG_SEG_SHIFT = KG_KH_SHIFT + KG_TAP_BITS;
DEV int encode_kg(int i, int Ktot, int Cs8, int KW, int C0) {
  if (i * 8 >= Ktot) return 0;
  int tap = i / Cs8, c = (i - tap * Cs8) * 8;
  int kh = tap / KW, kw = tap - kh * KW;
  int seg = c >= C0;
  if (seg) c -= C0;
  return c | (kw << KG_KW_SHIFT) | (kh << KG_KH_SHIFT) | (seg << KG_SEG_SHIFT) | (1 << (KG_SEG_SHIFT + 1));
}
// host: every value encode_kg packs for this conv fits its field -- the last group's offset in the wider segment
// (offsets below min(C0, Cs) in segment 0, below Cs - C0 in segment 1) and the last tap's kh, kw
inline bool kg_fits(int Cs, int C0, int KH, int KW) {
  const int w0 = C0 < Cs ? C0 : Cs, w1 = Cs - w0;
  return (w0 > w1 ? w0 : w1) - 8 < (1 << KG_CH_BITS) && KH - 1 < (1 << KG_TAP_BITS) && KW - 1 < (1 << KG_TAP_BITS);
}

// fused BN statistics: the channels of the tail this data gradient feeds (a concat gradient has more)
DEV int bns_channels(const ConvArgs& a) { return a.bN > 0 ? a.bN : a.N; }

// BN-backward constants of the block's BN channels nbase .. +BN into s_k[8][BN]: scale, shift, mean, invstd of
// the tail's BN, then of its residual's BN2 (zero past the tail's channels).  One tail shared by every group
// (bpgs == 0): its constants are group 0's.  Expands in the kernel body (ConvArgs a in scope).  A macro, not a
// function: inside a helper the two bn_channel_bwd expansions are optimised before they meet the kernel; their
// multiply-adds then contract differently (the statistics of a third of the LDS-staged configs changed in the last
// bits) and conv_igemm's MODE_DGRAD_BNS tiles grew from 105 to 136 VGPRs, one wave per SIMD less.
#define BNS_CONSTANTS(BN_, z_, nbase_, s_k_)                                              \
  do {                                                                                    \
    const int bN_ = bns_channels(a), zb_ = a.bpgs == 0 ? 0 : (z_);                        \
    for (int i_ = threadIdx.x; i_ < (BN_); i_ += 256) {                                   \
      const int n_ = (nbase_) + i_;                                                       \
      float k_[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                             \
      if (n_ < bN_) {                                                                     \
        bn_channel_bwd(a.bbn, zb_, n_, k_[0], k_[1], k_[2], k_[3]);                       \
        if (a.br_bn) bn_channel_bwd(a.bbn2, zb_, n_, k_[4], k_[5], k_[6], k_[7]);         \
      }                                                                                   \
      _Pragma("unroll") for (int q_ = 0; q_ < 8; ++q_) (s_k_)[q_ * (BN_) + i_] = k_[q_];  \
    }                                                                                     \
  } while (0)

// ---------------------------------------------------------------------------------------------
// Main loop
// ---------------------------------------------------------------------------------------------
template <int FN, int FM>
DEV void acc_zero(f32x4 (&acc)[FN][FM]) {
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int f = 0; f < FM; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// One K step of 32: every weight fragment (A: bf16x8 afr[FN], 16 channels) against every pixel fragment (B: bf16x8
// bfr[FM], 16 pixels) into f32x4 acc[FN][FM].  A macro, not a function: fragment arrays passed by reference stay
// in memory until the helper is inlined, the K loops are then scheduled differently, and the LDS-DMA kernels
// came out 4 VGPRs larger -- one wave per SIMD less on the 64-register tiles.
#define MFMA_STEP(acc, afr, bfr)                                  \
  _Pragma("unroll") for (int i_ = 0; i_ < FN; ++i_)               \
  _Pragma("unroll") for (int f_ = 0; f_ < FM; ++f_)               \
    acc[i_][f_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[i_], bfr[f_], acc[i_][f_], 0, 0, 0)

// Normalise-on-load of 8 channels: the staged values are pre-BN conv outputs y, the operand is
// act(y * scale + shift) (act = ReLU or identity), rounded to bf16 once, exactly as the BN tail that used to
// materialise it.  sc / sh: the 8 channels' constants.
DEV uint4 nol8(uint4 u, const float* sc, const float* sh, bool relu) {
  uint32_t w4[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    float lo = __uint_as_float(w4[h] << 16) * sc[2 * h] + sh[2 * h];
    float hi = __uint_as_float(w4[h] & 0xffff0000u) * sc[2 * h + 1] + sh[2 * h + 1];
    if (relu) { lo = fmaxf(lo, 0.f); hi = fmaxf(hi, 0.f); }
    w4[h] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
  }
  return make_uint4(w4[0], w4[1], w4[2], w4[3]);
}

// ---------------------------------------------------------------------------------------------
// Epilogue
// ---------------------------------------------------------------------------------------------
// stats_to_lds (conv_igemm's epilogue) works on ONE channel and takes scalars by value: with the sums handed over
// as pointers into the caller's float[4] arrays (or as f32x4: 4 consecutive registers) the forward conv_igemm tiles
// came out 5 VGPRs + 4 AGPRs larger, one wave per SIMD less.

// Statistics flush, first half: one channel's three sums over the 16 pixels of a lane row (-> lane 15: DPP,
// common.h) into dst = &s_st[wave row][channel][0].  third: the s2 row is in use.
DEV void stats_to_lds(float s0, float s1, float s2, bool third, float* dst, int l16) {
  s0 = row16_sum(s0);
  s1 = row16_sum(s1);
  if (third) s2 = row16_sum(s2);
  if (l16 == 15) {
    dst[0] = s0;
    dst[1] = s1;
    dst[2] = s2;
  }
}

// Second half (after a barrier): the WAM wave rows summed, one fp64 atomic per (channel, statistic) into replica
// bx % nrep: forward (sum y, sum y^2) rows of [G][NREP][2][N], or the fused BN-backward rows 0/1 (2 with a BN2
// residual) of the tail's [G][NREP][3][bN].
template <bool BNS, int BN, int WAM>
DEV void stats_publish(const ConvArgs& a, int z, int bx, int nbase, int bN, const float* s_st) {
  const int rep = bx % (BNS ? a.bbn.pnrep : a.stats_nrep);
  double* dst = BNS ? a.bpart : a.stats;
  const int rows = BNS ? 3 : 2, nrow = BNS && a.br_bn ? 3 : 2, nlim = BNS ? bN : a.N;
  const int64_t gb = BNS ? (a.bpgs < 0 ? (int64_t)z * NREP * 3 * bN : (int64_t)z * a.bpgs) : (int64_t)z * NREP * 2 * a.N;
  for (int q = threadIdx.x; q < BN * 3; q += 256) {
    const int c = q / 3, which = q - c * 3;
    const int n = nbase + c;
    if (n < nlim && which < nrow) {
      float v = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < WAM; ++w2) v += s_st[(w2 * BN + c) * 3 + which];
      atomicAdd(dst + gb + ((int64_t)rep * rows + which) * nlim + n, (double)v);
    }
  }
}

// Cross-block split-K reduction and epilogue of one output tile, shared by conv_lds_kernel, conv_glds_kernel and
// the patch kernels.  Lane: pixel l16 of each fragment, channels 4*kgl .. +3 of each 16-channel fragment.
//
// tile_store and the first half of tile_flush are open-coded (dz of the BN tail and its three sums, the row
// reduction), as is the dz block of conv_igemm's own epilogue: whether the sums' multiply-adds are fused depends on
// how the code around them is optimised.  Behind shared helpers (pointer, struct and by-value forms, explicit fmaf
// included), or with qy / qx moved from LdsPlan into TileCtx, the fp64 statistic rows of the large tiles (BN = 128,
// 256-pixel tiles, the CB = 32 persistent patch) changed in the last bits, and a training step with them.
struct TileCtx {
  int tid, lane, wid, wn, wm, l16, kgl, S, split, nt, ntn, z, mbase, nbase, Mq, HWq, Wq, oy0, ox0, bN;
  int bx, gx;  // logical block x (block_coords) and the grid's x extent: split-K tile id, BN replica
};

// Epilogue stores of one output tile (lane: pixel l16 of each fragment, channels 4*kgl .. +3): bias + bf16
// store (forward) / extra gradient sources + bf16 store (data gradient), and this lane's share of the BN
// statistics accumulated into st[i][stat][r] (summed over the tiles of a persistent block before the flush).
template <bool FWD, bool BNS, int BN, int WM, int WN, int FN, int FM>
DEV void tile_store(const ConvArgs& a, const LdsPlan& pl, const TileCtx& t, f32x4 (&acc)[FN][FM], const float* s_k,
                    float (&st)[FN][3][4]) {
  int orow[FM];
  bool pv[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    const int m = t.mbase + t.wm * WM + f * 16 + t.l16;
    pv[f] = m < t.Mq;
    const int mm = pv[f] ? m : 0;
    const int b = mm / t.HWq, r = mm - b * t.HWq;
    const int i = r / t.Wq, jj = r - i * t.Wq;
    orow[f] = (b * a.Ho + t.oy0 + i * pl.qy) * a.Wo + t.ox0 + jj * pl.qx;
  }
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int n0 = t.nbase + t.wn * WN + i * 16 + 4 * t.kgl;
    const int cl = t.wn * WN + i * 16 + 4 * t.kgl;
    const bool nok = n0 < a.N;
    float bias[4] = {0.f, 0.f, 0.f, 0.f};
    if (FWD && a.bias && nok) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bias[r] = a.bias[a.bgs * t.z + n0 + r];
    }
#pragma unroll
    for (int f = 0; f < FM; ++f) {
      if (!(nok && pv[f])) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][f][r] + bias[r];
      if (FWD) {
        bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + a.ogs * t.z + (int64_t)orow[f] * a.ldo + n0;
        uint2 w;
        w.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
        w.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
        *reinterpret_cast<uint2*>(o) = w;
#pragma unroll
        for (int r = 0; r < 4; ++r) { st[i][0][r] += v[r]; st[i][1][r] += v[r] * v[r]; }
      } else {
        bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + a.ogs * t.z + (int64_t)orow[f] * a.ldo + n0;
        add_sources(a, t.z, (int64_t)orow[f], n0, v);
        store4(o, v);
        if (BNS && n0 < t.bN) {  // dz of the BN tail this gradient feeds, and its statistics
          const uint2 u = *reinterpret_cast<const uint2*>(a.by + a.bygs * t.z + (int64_t)orow[f] * a.ldby + n0);
          const float yv[4] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                               __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
          uint2 q = make_uint2(0, 0);
          if (a.bkind == ADD_RELU) q = *reinterpret_cast<const uint2*>(a.br + a.brgs * t.z + (int64_t)orow[f] * a.ldbr + n0);
          const float rv[4] = {__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xffff0000u),
                               __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float tv = yv[r] * s_k[cl + r] + s_k[BN + cl + r];
            float dz = rbf(v[r]), xh2 = 0.f;  // the stored gradient: the apply pass recomputes dz from it
            if (a.bkind == ACT_RELU) {
              dz = tv > 0.f ? dz : 0.f;
            } else if (a.bkind == ACT_SIGMOID) {
              const float sg = sigmoidf_(tv);
              dz *= sg * (1.f - sg);
            } else if (a.bkind == ADD_RELU) {
              float rr = rv[r];
              if (a.br_bn) {
                xh2 = (rr - s_k[6 * BN + cl + r]) * s_k[7 * BN + cl + r];
                rr = rr * s_k[4 * BN + cl + r] + s_k[5 * BN + cl + r];
              }
              dz = (tv + rr) > 0.f ? dz : 0.f;
            }
            const float xh = (yv[r] - s_k[2 * BN + cl + r]) * s_k[3 * BN + cl + r];
            st[i][0][r] += dz;
            st[i][1][r] += dz * xh;
            st[i][2][r] += dz * xh2;
          }
        }
      }
    }
  }
}

// Block reduction of the accumulated statistics and one fp64 atomic per (channel, statistic) into replica
// blockIdx.x % nrep: forward (sum y, sum y^2) rows of [G][NREP][2][N], or the fused BN-backward rows 0/1 (2
// with a BN2 residual) of the tail's [G][NREP][3][bN].
template <bool FWD, bool BNS, int BN, int WAM, int WN, int FN>
DEV void tile_flush(const ConvArgs& a, const TileCtx& t, float (&st)[FN][3][4], float* s_st) {
  const bool want_red = (FWD && a.stats != nullptr) || BNS;
  if (!want_red) return;
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int cl = t.wn * WN + i * 16 + 4 * t.kgl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {  // the 16 pixels of a lane row -> lane 15 (DPP, common.h)
      st[i][0][r] = row16_sum(st[i][0][r]);
      st[i][1][r] = row16_sum(st[i][1][r]);
      if (BNS) st[i][2][r] = row16_sum(st[i][2][r]);
    }
    if (t.l16 == 15) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s_st[(t.wm * BN + cl + r) * 3 + 0] = st[i][0][r];
        s_st[(t.wm * BN + cl + r) * 3 + 1] = st[i][1][r];
        s_st[(t.wm * BN + cl + r) * 3 + 2] = BNS ? st[i][2][r] : 0.f;
      }
    }
  }
  __syncthreads();
  stats_publish<BNS, BN, WAM>(a, t.z, t.bx, t.nbase, t.bN, s_st);
}

template <bool FWD, bool BNS, int BM, int BN, int WAM, int WM, int WN, int FN, int FM>
DEV void tile_epilogue(const ConvArgs& a, const LdsPlan& pl, const TileCtx& t, f32x4 (&acc)[FN][FM], float* s_st,
                       const float* s_k, int* s_flag) {
  // ---- cross-block split of K: deterministic last-arriver reduction.  The fp32 partial tiles are stored
  // WRITE-THROUGH (sc1 buffer stores: they leave the XCD's L2 at once, so no agent-scope release fence --
  // an L2 write-back of ~6.5 us with 16 KB dirtied per block), every wave drains them, one lane draws the
  // tile's arrival ticket (agent-scope atomic), and the last arriver reads all partials with sc1 loads
  // (L1 bypassed: no acquire fence either) in split order.
  if (t.S > 1) {
    const int64_t tile = ((int64_t)t.z * t.gx + t.bx) * t.ntn + t.nt;
    const uint64_t base = reinterpret_cast<uint64_t>(a.ws + tile * t.S * (BM * BN));
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, t.S * BM * BN * 4, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const u32x4 v = {__float_as_uint(acc[i][f][0]), __float_as_uint(acc[i][f][1]), __float_as_uint(acc[i][f][2]),
                         __float_as_uint(acc[i][f][3])};
        const int off = ((t.split * (BM * BN / 4) + ((t.wid * FN + i) * FM + f) * 64 + t.lane)) * 16;
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, 16);  // aux 16 = sc1
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its partial tile
    __syncthreads();
    if (t.tid == 0) {
      const unsigned tk = __hip_atomic_fetch_add(a.cnt + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_flag[0] = tk == (unsigned)(t.S - 1);
    }
    __syncthreads();
    if (!s_flag[0]) return;
    if (t.tid == 0) __hip_atomic_store(a.cnt + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // reusable
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the ticket
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int sp = 0; sp < t.S; ++sp) {
          const int off = ((sp * (BM * BN / 4) + ((t.wid * FN + i) * FM + f) * 64 + t.lane)) * 16;
          const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
          v[0] += __uint_as_float(u[0]); v[1] += __uint_as_float(u[1]);
          v[2] += __uint_as_float(u[2]); v[3] += __uint_as_float(u[3]);
        }
        acc[i][f] = v;
      }
  }

  float st[FN][3][4] = {};
  tile_store<FWD, BNS, BN, WM, WN, FN, FM>(a, pl, t, acc, s_k, st);
  tile_flush<FWD, BNS, BN, WAM, WN, FN>(a, t, st, s_st);
}

}  // namespace mda
