// Patch convolution (cfg in [CONV_PATCH_CFG0, +CONV_PATCH_NCFG) and [CONV_PATCHP_CFG0, +CONV_PATCHP_NCFG)): 3x3 /
// stride-1 forward and data gradient of the wide maps (Model C's 49x124 / 47x122 / 23x60 stem, Model A's
// 33x83 / 17x42 stages).  The im2col forms of conv_lds.hip fetch every input element once per tap (9x); here a
// block owns a STRIP of R whole output rows of one image (M tile = R * Wout pixels, row-major, so the shared
// tile_epilogue of conv_tile.h applies unchanged) and stages the strip's input rows with halo -- (R + 2) rows x
// (Wout + 2) columns x CB channels -- in LDS ONCE per channel slice, together with the slice's weights
// [BN][9 * CB].  Every tap's MFMA operand is then a shifted read of the same strip: lane (pixel p, k-group q) of
// tap (dh, dw) reads the 16 bytes at strip row r(p) + dh, column c(p) + dw, channels 8q'.. -- no im2col gather,
// no per-tap bounds checks (padding is zero in the strip), and a normalise-on-load input is transformed once per
// element instead of 9 times.  The data gradient is the same kernel over dy with the taps flipped (dh = 2 - kh)
// and the halo offsets of the transposed conv.
//
// LDS rows are padded to CBP = CB + 8 channels and the weight rows to WKP = 9 CB (rounded up to 32) + 8, so
// the row pitches are odd multiples of 16 bytes: the 16 lanes of each ds_read_b128 group hit 16 distinct
// 16-byte slots of a 256-byte bank row (conflict-free).
//
// This file: conv_patch_kernel (one strip per block), conv_patchp_kernel (persistent, LDS-DMA pipelined), the
// weight-slice staging and tap arithmetic they share, the strip plan and the launchers.  LDS layout (patch_lds),
// prologue helpers and the epilogue come from conv_tile.h.
#include "conv_tile.h"

namespace mda {

namespace {

constexpr int PT_NT = 5;  // tile configs: BM pixels (strip capacity) x BN channels, WAM waves along M
constexpr int PT_BM[PT_NT] = {256, 256, 256, 128, 128};
constexpr int PT_BN[PT_NT] = {16, 32, 64, 32, 64};
constexpr int PT_WAM[PT_NT] = {4, 4, 4, 4, 2};
constexpr int PT_CB[3] = {16, 32, 64};
static_assert(PT_NT * 3 == CONV_PATCH_NCFG && PT_NT * 3 == CONV_PATCHP_NCFG, "cfg = CFG0 + 3 * tile + cb");

__device__ uint4 g_zero16[4];  // never written: the source of every padding lane

typedef __attribute__((address_space(3))) void* lds_vptr;
typedef __attribute__((address_space(1))) void* glb_vptr;

// Weight slice [BN][WKP] of channels cs0 .. +CB: 16-byte unit w < BN * (WKP / 8 - 1) is k-group g of row n; k-group
// g = tap g / CG, channels 8 (g % CG) (zero past 9 CB / Npad).  patch_w_load fetches it, patch_w_slot is its s_w
// element offset.
template <int CB>
DEV uint4 patch_w_load(const ConvArgs& a, const bf16_t* wz, int nbase, int cs0, int w) {
  constexpr int CG = CB / 8, NGW = pt_wkp(CB) / 8 - 1;
  const int g = w % NGW, n = nbase + w / NGW;
  const int tap = g / CG;
  if (tap < 9 && n < a.Npad)
    return *reinterpret_cast<const uint4*>(wz + (int64_t)n * a.Kpad + tap * a.Cs + cs0 + (g - tap * CG) * 8);
  return make_uint4(0, 0, 0, 0);
}
template <int CB>
DEV int patch_w_slot(int w) {
  constexpr int NGW = pt_wkp(CB) / 8 - 1;
  return (w / NGW) * pt_wkp(CB) + (w % NGW) * 8;
}

// Strip pixel offset (strip of WP columns) of the tap of k-group g = tap g / CG, channel group g % CG -- the taps
// flipped for the data gradient.  k past 9 CB: zero weights, any strip element.  Returned by value: outputs through
// reference parameters kept the unrolled K loop's offsets in memory until inlining and cost up to 74 VGPRs.
template <bool FWD, int CG>
DEV int patch_tap_offset(int g, int WP) {
  const int tap = g / CG < 9 ? g / CG : 0;
  const int kh = tap / 3, kw = tap - kh * 3;
  return (FWD ? kh : 2 - kh) * WP + (FWD ? kw : 2 - kw);
}

template <int MODE, int BM, int BN, int WAM, int CB>
__global__ __launch_bounds__(256) void conv_patch_kernel(ConvArgs a, PatchPlan pp) {
  const Blk blk = block_coords(a.xcd);
  constexpr int WAN = 4 / WAM;
  constexpr int WM = BM / WAM, WN = BN / WAN, FM = WM / 16, FN = WN / 16;
  static_assert(FM >= 1 && FN >= 1 && WM % 16 == 0 && WN % 16 == 0, "wave tile");
  constexpr int CBP = CB + 8, KS = pt_ksteps(CB), WKP = pt_wkp(CB);
  constexpr int CG = CB / 8;  // 16-byte channel groups of a strip pixel
  static_assert(256 % CG == 0, "a thread's strip units keep one channel group");
  constexpr int NU = 8;       // staging units per thread per round
  constexpr bool FWD = is_fwd<MODE>();
  constexpr bool NOL = MODE == MODE_FWD_NOL;
  constexpr bool BNS = MODE == MODE_DGRAD_BNS;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int WP = pp.Wout + 2;  // strip columns
  const int SR = pp.R + 2;     // strip rows
  const PatchLds L = patch_lds(patch_strip_bytes(pp.R, pp.Wout, CB), BN, WAM, CB, conv_nconst(MODE, a.Cs, BN));
  bf16_t* s_x = reinterpret_cast<bf16_t*>(smem);
  bf16_t* s_w = reinterpret_cast<bf16_t*>(smem + L.w);
  float* s_st = reinterpret_cast<float*>(smem + L.t.st);
  float* s_k = reinterpret_cast<float*>(smem + L.t.k);
  int* s_flag = reinterpret_cast<int*>(smem + L.t.flag);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kgl = lane >> 4;
  const int wn = wid % WAN, wm = wid / WAN;
  const int z = blk.z, nt = blk.y, ntn = gridDim.y;
  const int b = blk.x / pp.nstrip, oh0 = (blk.x - b * pp.nstrip) * pp.R;
  const int rows = min(pp.R, pp.Hout - oh0);
  const int HWo = pp.Hout * pp.Wout;
  const int mbase = b * HWo + oh0 * pp.Wout, nbase = nt * BN;
  const int Mtile = mbase + rows * pp.Wout;  // pixels of this strip end here (the next strip / image starts)

  if (NOL) bn_prepare(a.nbn, z, s_k, s_k + a.Cs, nullptr, nullptr, blk.x == 0 && blk.y == 0);
  if (BNS) BNS_CONSTANTS(BN, z, nbase, s_k);

  const ConvBases sb = conv_bases(a, z);
  const int row0 = oh0 + pp.dy0, col0 = pp.dx0;  // source pixel of strip (0, 0)
  const int nux = SR * WP * CG, nuw = BN * (WKP - 8) / 8, nut = nux + nuw;

  // fragment bases: this lane's pixel of each M fragment -> strip element offset of tap (0, 0), channel 0
  int pbase[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    int p = wm * WM + f * 16 + l16;
    p = mbase + p < Mtile ? p : 0;  // rows past the strip: any in-LDS address (the epilogue drops them)
    const int r = p / pp.Wout, c = p - r * pp.Wout;
    pbase[f] = (r * WP + c) * CBP;
  }

  f32x4 acc[FN][FM];
  acc_zero(acc);

  __syncthreads();  // NOL / BNS constants
  for (int sl = 0; sl < pp.nslice; ++sl) {
    const int cs0 = sl * CB;
    // NOL: a thread's strip units all carry channel group tid % CG (CG divides 256), so its 8 scale and
    // 8 shift constants live in registers for the whole slice (an LDS read per element cost ~17 us on
    // the 47x122 stem conv)
    float nsc[8], nsh[8];
    if (NOL) {
      const int c = cs0 + (tid % CG) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) { nsc[j] = s_k[c + j]; nsh[j] = s_k[a.Cs + c + j]; }
    }
    // ---- stage the strip slice and the weight slice: unit u < nux -> strip (row j, column q, group g),
    // else weight unit u - nux
    for (int u0 = 0; u0 < nut; u0 += 256 * NU) {
      uint4 v[NU];
      uint32_t okm = 0;
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = u0 + tid + 256 * i;
        v[i] = make_uint4(0, 0, 0, 0);
        if (u < nux) {
          const int g = u % CG, q = (u / CG) % WP, j = u / (CG * WP);
          const int ih = row0 + j, iw = col0 + q;
          if (ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
            const int c = cs0 + g * 8;
            const int seg = (a.src.C1 > 0 && c >= a.src.C0) ? 1 : 0;
            v[i] = *reinterpret_cast<const uint4*>(conv_src(a, sb, seg, b, ih, iw, c - seg * a.src.C0));
            okm |= 1u << i;
          }
        } else if (u < nut) {
          v[i] = patch_w_load<CB>(a, sb.wz, nbase, cs0, u - nux);
        }
      }
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        const int u = u0 + tid + 256 * i;
        if (u < nux) {
          const int g = u % CG, pix = u / CG;
          uint4 x = v[i];
          if (NOL && ((okm >> i) & 1)) x = nol8(x, nsc, nsh, a.nol_kind == ACT_RELU);  // once per element
          *reinterpret_cast<uint4*>(s_x + pix * CBP + g * 8) = x;
        } else if (u < nut) {
          *reinterpret_cast<uint4*>(s_w + patch_w_slot<CB>(u - nux)) = v[i];
        }
      }
    }
    __syncthreads();
    // ---- 9 taps x CB channels: k-group g = 4 ks + kgl
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int g = 4 * ks + kgl;
      const int off = patch_tap_offset<FWD, CG>(g, WP) * CBP + (g - (g / CG) * CG) * 8;
      bf16x8 afr[FN], bfr[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i)
        afr[i] = *reinterpret_cast<const bf16x8*>(s_w + (wn * WN + i * 16 + l16) * WKP + g * 8);
#pragma unroll
      for (int f = 0; f < FM; ++f) bfr[f] = *reinterpret_cast<const bf16x8*>(s_x + pbase[f] + off);
      MFMA_STEP(acc, afr, bfr);
    }
    __syncthreads();  // the next slice overwrites the strip and the weights
  }

  LdsPlan pl{};
  pl.qy = 1; pl.qx = 1;
  const TileCtx tc{tid, lane, wid, wn, wm, l16, kgl, 1, 0, nt, ntn, z, mbase, nbase, Mtile, HWo, pp.Wout, 0, 0,
                   bns_channels(a), blk.x, (int)gridDim.x};
  tile_epilogue<FWD, BNS, BM, BN, WAM, WM, WN, FN, FM>(a, pl, tc, acc, s_st, s_k, s_flag);
}

// Persistent, software-pipelined patch conv (cfg CONV_PATCHP_CFG0 + 3 * tile + cb; one channel slice,
// Cs == CB).  The one-strip-per-block form above stages, then computes: its blocks expose the load latency
// and only the 2-3 co-resident blocks hide it.  Here a block stages its BN x 9 CB weights once, then loops
// over strips u = blockIdx.x, + gridDim.x, ...: the next strip goes global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, no registers) into the other of two strip buffers while the MFMAs of the
// current one run; the BN statistics are summed in registers over all of the block's strips and flushed
// once.  Strip image: dense [pixel q][CG 16-byte groups], group g of pixel q in slot g ^ ((q / (16 / CG)) %
// CG): the 16 pixels of an MFMA fragment read (16 consecutive q, one g) hit 16 distinct slots of the
// 256-byte bank rows.  Padding / halo bytes are DMA'd from a zero page.
template <int MODE, int BM, int BN, int WAM, int CB>
__global__ __launch_bounds__(256) void conv_patchp_kernel(ConvArgs a, PatchPlan pp) {
  constexpr int WAN = 4 / WAM;
  constexpr int WM = BM / WAM, WN = BN / WAN, FM = WM / 16, FN = WN / 16;
  static_assert(FM >= 1 && FN >= 1 && WM % 16 == 0 && WN % 16 == 0, "wave tile");
  constexpr int KS = pt_ksteps(CB), WKP = pt_wkp(CB);
  constexpr int CG = CB / 8, PPR = 16 / CG;  // 16-byte groups per pixel, pixels per 256-byte bank row
  constexpr bool FWD = MODE == MODE_FWD;
  constexpr bool BNS = MODE == MODE_DGRAD_BNS;
  static_assert(MODE != MODE_FWD_NOL, "the DMA bypasses registers: no on-load transform");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int WP = pp.Wout + 2, SR = pp.R + 2;
  const int nq = SR * WP;                                   // strip pixels
  const int SBP = patchp_strip_bytes(pp.R, pp.Wout, CB);    // bytes of one strip buffer
  const int nins = SBP / 1024;                              // 1-KB DMA instructions per strip
  const PatchLds L = patch_lds(2 * SBP, BN, WAM, CB, conv_nconst(MODE, a.Cs, BN));
  bf16_t* s_w = reinterpret_cast<bf16_t*>(smem + L.w);
  float* s_st = reinterpret_cast<float*>(smem + L.t.st);
  float* s_k = reinterpret_cast<float*>(smem + L.t.k);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kgl = lane >> 4;
  const int wn = wid % WAN, wm = wid / WAN;
  const int z = blockIdx.z, nt = blockIdx.y, ntn = gridDim.y;
  const int nbase = nt * BN;
  const int HWo = pp.Hout * pp.Wout;
  const int U = a.B * pp.nstrip;
  const int bN = bns_channels(a);
  if (BNS) BNS_CONSTANTS(BN, z, nbase, s_k);
  const ConvBases sb = conv_bases(a, z);
  const void* zero = &g_zero16[0];

  // ---- strip DMA: instruction j of wave w writes strip bytes [(4j + w) KB, +1 KB); lane l fetches 16-byte
  // unit v = 64 (4j + w) + l = (pixel q, slot): the pixel's channel group slot ^ swz(q)
  auto issue = [&](int u, char* buf) {
    const int b = u / pp.nstrip, oh0 = (u - b * pp.nstrip) * pp.R;
    const int row0 = oh0 + pp.dy0;
    for (int j = 0; 4 * j + wid < nins; ++j) {
      const int v = 64 * (4 * j + wid) + lane;
      const int q = v / CG, slot = v - q * CG;
      const void* src = zero;
      if (q < nq) {
        const int jr = q / WP, qc = q - jr * WP;
        const int ih = row0 + jr, iw = pp.dx0 + qc;
        if (ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws) {
          const int c = (slot ^ ((q / PPR) % CG)) * 8;
          const int seg = (a.src.C1 > 0 && c >= a.src.C0) ? 1 : 0;
          src = conv_src(a, sb, seg, b, ih, iw, c - seg * a.src.C0);
        }
      }
      __builtin_amdgcn_global_load_lds((glb_vptr)src, (lds_vptr)(buf + (4 * j + wid) * 1024), 16, 0, 0);
    }
  };

  // ---- weights once
  for (int w = tid; w < BN * (WKP / 8 - 1); w += 256)
    *reinterpret_cast<uint4*>(s_w + patch_w_slot<CB>(w)) = patch_w_load<CB>(a, sb.wz, nbase, 0, w);

  // fragment bases: strip pixel of tap (0, 0) for this lane's pixel of each M fragment
  int q0[FM];
#pragma unroll
  for (int f = 0; f < FM; ++f) {
    int p = wm * WM + f * 16 + l16;
    p = p < pp.R * pp.Wout ? p : 0;  // past the strip: any in-LDS pixel (the epilogue drops them)
    const int r = p / pp.Wout, c = p - r * pp.Wout;
    q0[f] = r * WP + c;
  }

  float st[FN][3][4] = {};
  LdsPlan pl{};
  pl.qy = 1; pl.qx = 1;
  int cur = 0;
  if ((int)blockIdx.x < U) issue(blockIdx.x, smem);
  __syncthreads();  // weights and constants
  for (int u = blockIdx.x; u < U; u += gridDim.x) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMAs of strip u (and its last stores)
    __builtin_amdgcn_s_barrier();                      // ... and every wave's; strip u - grid fully read
    asm volatile("" ::: "memory");
    if (u + (int)gridDim.x < U) issue(u + gridDim.x, smem + (cur ^ 1) * SBP);
    const char* X = smem + cur * SBP;
    f32x4 acc[FN][FM];
    acc_zero(acc);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const int g = 4 * ks + kgl;
      const int dq = patch_tap_offset<FWD, CG>(g, WP);
      const int cg = g - (g / CG) * CG;
      bf16x8 afr[FN], bfr[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i)
        afr[i] = *reinterpret_cast<const bf16x8*>(s_w + (wn * WN + i * 16 + l16) * WKP + g * 8);
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const int q = q0[f] + dq;
        bfr[f] = *reinterpret_cast<const bf16x8*>(X + (q * CG + (cg ^ ((q / PPR) % CG))) * 16);
      }
      MFMA_STEP(acc, afr, bfr);
    }
    const int b = u / pp.nstrip, oh0 = (u - b * pp.nstrip) * pp.R;
    const int rows = min(pp.R, pp.Hout - oh0);
    const int mbase = b * HWo + oh0 * pp.Wout;
    const TileCtx tc{tid, lane, wid, wn, wm, l16, kgl, 1, 0, nt, ntn, z, mbase, nbase, mbase + rows * pp.Wout, HWo,
                     pp.Wout, 0, 0, bN, (int)blockIdx.x, (int)gridDim.x};
    tile_store<FWD, BNS, BN, WM, WN, FN, FM>(a, pl, tc, acc, s_k, st);
    cur ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the strip buffers are dead; s_st lives past the weights
  const TileCtx tf{tid, lane, wid, wn, wm, l16, kgl, 1, 0, nt, ntn, z, 0, nbase, 0, HWo, pp.Wout, 0, 0, bN,
                   (int)blockIdx.x, (int)gridDim.x};
  tile_flush<FWD, BNS, BN, WAM, WN, FN>(a, tf, st, s_st);
}

// patch conv config -> (tile, channel slice, persistent form)
void patch_cfg(int cfg, int& tile, int& cbi, bool& pers) {
  pers = cfg >= CONV_PATCHP_CFG0;
  const int k = cfg - (pers ? CONV_PATCHP_CFG0 : CONV_PATCH_CFG0);
  tile = k / 3;
  cbi = k % 3;
}

// Strip plan and LDS bytes of a patch launch (host); returns 0, or -2 when the conv is not a 3x3 / stride-1 conv
// this tile can take.  FWD: output Ho x Wo from the input (Hs, Ws); DGRAD: dx (Ho, Wo) from dy (Hs, Ws).
int patch_plan(int mode, const ConvArgs& a, int tile, int cbi, bool pers, PatchPlan& pp, size_t& lds) {
  const bool fwd = mode == MODE_FWD || mode == MODE_FWD_NOL;
  const int CB = PT_CB[cbi], BM = PT_BM[tile];
  if (a.KH != 3 || a.KW != 3 || a.sh != 1 || a.sw != 1) return -2;
  if (a.Cs % CB || a.Cs > 16383) return -2;
  if (a.src.C1 > 0 && a.src.C0 % CB) return -2;  // a channel slice may not straddle the two segments
  pp.Wout = a.Wo;
  pp.Hout = a.Ho;
  if (pp.Wout > BM || pp.Wout < 1) return -2;
  pp.R = std::min(BM / pp.Wout, pp.Hout);
  pp.nstrip = (pp.Hout + pp.R - 1) / pp.R;
  pp.nslice = a.Cs / CB;
  if (fwd) { pp.dy0 = -a.ph; pp.dx0 = -a.pw; }
  else { pp.dy0 = a.ph - 2; pp.dx0 = a.pw - 2; }
  if (fwd ? (a.Hs + 2 * a.ph - 2 != a.Ho || a.Ws + 2 * a.pw - 2 != a.Wo)
          : (a.Ho + 2 * a.ph - 2 != a.Hs || a.Wo + 2 * a.pw - 2 != a.Ws)) return -2;
  // the persistent form has one channel slice and no on-load transform; its two dense strip buffers are never
  // smaller than the one padded strip of the one-strip form
  if (pers && (mode == MODE_FWD_NOL || pp.nslice != 1)) return -2;
  const int strip = pers ? 2 * patchp_strip_bytes(pp.R, pp.Wout, CB) : patch_strip_bytes(pp.R, pp.Wout, CB);
  lds = patch_lds(strip, PT_BN[tile], PT_WAM[tile], CB, conv_nconst(mode, a.Cs, PT_BN[tile])).t.bytes;
  return lds > CONV_LDS_MAX ? -2 : 0;
}

template <int MODE>
int launch_patchp(const ConvArgs& a, int G, int tile, int cbi, hipStream_t st) {
  if constexpr (MODE == MODE_FWD_NOL) {
    return -2;
  } else {
    PatchPlan pp;
    size_t lds;
    int rc = patch_plan(MODE, a, tile, cbi, true, pp, lds);
    if (rc) return rc;
    const int ntn = (a.N + PT_BN[tile] - 1) / PT_BN[tile];
    const int per_cu = std::max<int>(1, (int)(CONV_LDS_MAX / lds));
    const int U = a.B * pp.nstrip;
    const int nblk = std::max(1, std::min(U, (256 * per_cu + ntn * G - 1) / (ntn * G)));
    dim3 grid(nblk, ntn, G);
#define PP_LAUNCH(T, C)                                                                                     \
  if (tile == T && cbi == C) {                                                                              \
    hipLaunchKernelGGL((conv_patchp_kernel<MODE, PT_BM[T], PT_BN[T], PT_WAM[T], PT_CB[C]>), grid, dim3(256), lds, \
                       st, a, pp);                                                                          \
    return (int)hipGetLastError();                                                                          \
  }
#define PP_TILE(T) PP_LAUNCH(T, 0) PP_LAUNCH(T, 1) PP_LAUNCH(T, 2)
    PP_TILE(0) PP_TILE(1) PP_TILE(2) PP_TILE(3) PP_TILE(4)
#undef PP_TILE
#undef PP_LAUNCH
    return -1;
  }
}

template <int MODE>
int launch_patch(const ConvArgs& a, int G, int tile, int cbi, hipStream_t st) {
  PatchPlan pp;
  size_t lds;
  int rc = patch_plan(MODE, a, tile, cbi, false, pp, lds);
  if (rc) return rc;
  dim3 grid(a.B * pp.nstrip, (a.N + PT_BN[tile] - 1) / PT_BN[tile], G);
#define PT_LAUNCH(T, C)                                                                                     \
  if (tile == T && cbi == C) {                                                                              \
    hipLaunchKernelGGL((conv_patch_kernel<MODE, PT_BM[T], PT_BN[T], PT_WAM[T], PT_CB[C]>), grid, dim3(256), lds, \
                       st, a, pp);                                                                          \
    return (int)hipGetLastError();                                                                          \
  }
#define PT_TILE(T) PT_LAUNCH(T, 0) PT_LAUNCH(T, 1) PT_LAUNCH(T, 2)
  PT_TILE(0) PT_TILE(1) PT_TILE(2) PT_TILE(3) PT_TILE(4)
#undef PT_TILE
#undef PT_LAUNCH
  return -1;
}

}  // namespace

int conv_patch_check(int mode, const ConvArgs& a, int cfg) {
  if (!conv_patch_cfg(cfg)) return -1;
  int tile, cbi;
  bool pers;
  patch_cfg(cfg, tile, cbi, pers);
  PatchPlan pp;
  size_t lds;
  return patch_plan(mode, a, tile, cbi, pers, pp, lds);
}

int launch_conv_patch(int mode, const ConvArgs& a, int G, int cfg, hipStream_t st) {
  if (!conv_patch_cfg(cfg)) return -1;
  int tile, cbi;
  bool pers;
  patch_cfg(cfg, tile, cbi, pers);
  switch (mode) {
    case MODE_FWD: return pers ? launch_patchp<MODE_FWD>(a, G, tile, cbi, st) : launch_patch<MODE_FWD>(a, G, tile, cbi, st);
    case MODE_FWD_NOL: return pers ? -2 : launch_patch<MODE_FWD_NOL>(a, G, tile, cbi, st);
    case MODE_DGRAD: return pers ? launch_patchp<MODE_DGRAD>(a, G, tile, cbi, st) : launch_patch<MODE_DGRAD>(a, G, tile, cbi, st);
    case MODE_DGRAD_BNS:
      return pers ? launch_patchp<MODE_DGRAD_BNS>(a, G, tile, cbi, st) : launch_patch<MODE_DGRAD_BNS>(a, G, tile, cbi, st);
    default: return -1;
  }
}

}  // namespace mda
