// LDS-staged implicit-GEMM convolution on gfx950 MFMA (v_mfma_f32_16x16x32_bf16): forward and data
// gradient, NHWC bf16 operands, fp32 accumulation.  Replaces the same reference ops as conv.hip
// (every nn.Conv2d of model/modelA_MTL.py, model/modelB_singleTask.py and the Inception blocks of
// model/modelC_multiClassifier.py, and their autograd grad_input).
//
// Why a second conv kernel: conv.hip's conv_igemm loads every wave's MFMA fragments straight from
// global memory, 32 k at a time, two stages deep.  On Model C's deep layers (M = B*H*W of 192..8960
// pixels, K = 576..4032) a launch is a chain of ~10-40 dependent load round trips per wave and ran at
// 25..150 TF/s (profiles/r2_conv_layer_times_before.txt).  Here
//
//   * a block's whole K chunk (KC = 64 or 128) of BOTH operands is staged in LDS: 256 threads issue
//     16-byte loads cooperatively (8 pixels x 128 contiguous bytes per wave instruction: full lines),
//     the im2col gather / zero padding / normalise-on-load BN+ReLU happens once per element while
//     storing, and every wave reads its fragments with conflict-free ds_read_b128 -- the tile is read
//     from global memory once per block instead of once per wave;
//   * the next chunk's loads are in flight while the MFMAs of the current one run (double-buffered
//     LDS, one barrier per chunk);
//   * K is split ACROSS blocks (splits = 1..8): short dependency chains and enough blocks to fill the
//     256 CUs on small-M layers.  Partial fp32 tiles go to a workspace; the last block to arrive at a
//     tile (agent-scope release/acquire ticket) sums them in split order -- deterministic -- and runs
//     the epilogue;
//   * a stride-2 data gradient is decomposed into its sub-pixel phases (output parities): each phase
//     reduces over the taps that actually hit a dy element, instead of the gather form's masking of
//     3/4 of the MFMA work (conv.hip conv_load_stage).
//
// LDS image of an operand chunk: [k-group g (8 channels)][row][8 bf16] (16-byte units).  The MFMA
// fragment read of lane (r = lane & 15, q = lane >> 4) at k-step s is row r, group 4s + q: within a
// ds_read_b128 lane group the 16 rows are distinct, so each group touches 16 distinct 16-byte slots of
// a 256-byte bank row (conflict-free).  Staging writes go 8 consecutive lanes -> 8 consecutive rows
// (one 128-byte ds_write_b128 group, conflict-free); the matching global loads read 8 pixels x 8
// k-groups = 8 full 128-byte lines per wave instruction.
//
// Modes: MODE_FWD, MODE_FWD_NOL (normalise-on-load of the input), MODE_DGRAD, MODE_DGRAD_BNS (fused
// BN-backward statistics in the epilogue).
//
// This file: conv_lds_kernel (register-staged) and conv_glds_kernel (LDS-DMA), the block setup they share
// (igemm_block_setup) and their host plan and launchers.  The LDS layout, the split-K reduction and the
// epilogue (tile_epilogue: bias, bf16 store, fp64 replica BN sums / bf16 gradient store, dz statistics) are in
// conv_tile.h; the 3x3 / stride-1 patch kernels, which share them, are in conv_patch.hip.
#include "conv_tile.h"

namespace mda {

namespace {

// (BM pixels, BN channels, waves along M, waves along N) of each tile config
constexpr int LDS_BM[8] = {64, 128, 64, 128, 32, 64, 32, 128};
constexpr int LDS_BN[8] = {64, 64, 128, 128, 64, 32, 32, 16};
constexpr int LDS_WAM[8] = {2, 2, 2, 2, 2, 2, 2, 4};

// The phase of logical block x (wave-uniform), by value, from the kernel's by-value argument `pl`.  Every field is
// picked by a chain of constant-index reads: a dynamic index would copy the argument struct to scratch memory.  A
// macro, not a function: through a reference parameter the optimiser merges the twelve chains into ONE selected
// pointer into the argument, which is such a dynamic index (240 bytes of scratch per lane in every kernel).
#define PSEL(f) (p == 0 ? pl.ph[0].f : p == 1 ? pl.ph[1].f : p == 2 ? pl.ph[2].f : pl.ph[3].f)
#define SELECT_PHASE(bx)                                                                                  \
  ({                                                                                                      \
    int p = 0;                                                                                            \
    _Pragma("unroll") for (int q = 1; q < 4; ++q) if (q < pl.nph && (bx) >= pl.ph[q].m0) p = q;           \
    LdsPhase{PSEL(oy0), PSEL(ox0), PSEL(Hq), PSEL(Wq), PSEL(rh), PSEL(nh), PSEL(rw), PSEL(nw),            \
             PSEL(ay), PSEL(ax), PSEL(m0), PSEL(Kp)};                                                     \
  })

// Geometry of one block of an implicit-GEMM launch: its phase's output grid, its tile and its share
// [cb, ce) of the phase's K chunks.
struct IgemmBlk {
  int oy0, ox0, Wq, HWq, Mq;
  int S, ntn, nt, split, z, mbase, nbase, cb, ce;
};

// Block setup shared by conv_lds_kernel and conv_glds_kernel; fills the per-block k-group tables of this
// split's chunks: s_tx (input coordinates / channel) and s_tw (weight column, -1: none).
template <int BM, int BN, int KC>
DEV IgemmBlk igemm_block_setup(const ConvArgs& a, const LdsPlan& pl, const LdsPhase& P, const Blk& blk, int* s_tx,
                               int* s_tw) {
  constexpr int NG = KC / 8;
  IgemmBlk k;
  k.oy0 = P.oy0; k.ox0 = P.ox0; k.Wq = P.Wq;
  k.S = pl.splits;
  k.ntn = (a.N + BN - 1) / BN;
  k.nt = blk.y / k.S; k.split = blk.y - k.nt * k.S;
  k.z = blk.z;
  k.HWq = P.Hq * P.Wq;
  k.Mq = a.B * k.HWq;
  k.mbase = (blk.x - P.m0) * BM; k.nbase = k.nt * BN;
  const int nch = P.Kp / KC;
  const int cps = (nch + k.S - 1) / k.S;
  k.cb = min(nch, k.split * cps); k.ce = min(nch, k.cb + cps);

  const int cs8 = a.Cs >> 3, ntap = P.nh * P.nw;
  const int ng = (k.ce - k.cb) * NG;
  for (int i = threadIdx.x; i < ng; i += 256) {
    const int gabs = k.cb * NG + i;
    const int t = gabs / cs8;
    const int c = (gabs - t * cs8) * 8;
    int ex = 0, ew = -1;
    if (t < ntap) {
      const int u = t / P.nw, v = t - u * P.nw;
      const int kh = P.rh + pl.th * u, kw = P.rw + pl.tw * v;
      const int dyo = P.ay + pl.by * u, dxo = P.ax + pl.bx * v;
      const int seg = (a.src.C1 > 0 && c >= a.src.C0) ? 1 : 0;
      ex = (c - seg * a.src.C0) | ((dyo + 64) << 14) | ((dxo + 64) << 21) | (seg << 28) | (1 << 29);
      ew = (kh * a.KW + kw) * a.Cs + c;
    }
    s_tx[i] = ex;
    s_tw[i] = ew;
  }
  return k;
}

// Tile row `row` of the block (inb: the row exists) -> image pb (-1: past the phase's pixels) and the input
// coordinates (pih, piw) of its tap (0, 0)
DEV void igemm_row_pixel(const IgemmBlk& k, const LdsPlan& pl, int row, bool inb, int& pb, int& pih, int& piw) {
  const int m = k.mbase + row;
  const bool ok = inb && m < k.Mq;
  const int mm = ok ? m : 0;
  const int b = mm / k.HWq, r = mm - b * k.HWq;
  const int i = r / k.Wq, jj = r - i * k.Wq;
  pb = ok ? b : -1;
  pih = i * pl.mh;
  piw = jj * pl.mw;
}

// The 16 source bytes of k-group table entry e at a row's pixel; false: zero padding
DEV bool igemm_src(const ConvArgs& a, const ConvBases& s, int e, int pb, int pih, int piw, const bf16_t*& src) {
  const int ih = pih + ((e >> 14) & 127) - 64, iw = piw + ((e >> 21) & 127) - 64;
  const bool ok = ((e >> 29) & 1) && pb >= 0 && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws;
  if (ok) src = conv_src(a, s, (e >> 28) & 1, pb, ih, iw, e & 16383);
  return ok;
}

DEV TileCtx igemm_tile_ctx(const ConvArgs& a, const IgemmBlk& k, const Blk& blk, int tid, int wid, int wn, int wm) {
  const int lane = tid & 63;
  return TileCtx{tid, lane, wid, wn, wm, lane & 15, lane >> 4, k.S, k.split, k.nt, k.ntn, k.z, k.mbase, k.nbase,
                 k.Mq, k.HWq, k.Wq, k.oy0, k.ox0, bns_channels(a), blk.x, (int)gridDim.x};
}

template <int MODE, int BM, int BN, int WAM, int KC>
__global__ __launch_bounds__(256) void conv_lds_kernel(ConvArgs a, LdsPlan pl) {
  const Blk blk = block_coords(a.xcd);
  constexpr int WAN = 4 / WAM;
  constexpr int WM = BM / WAM, WN = BN / WAN, FM = WM / 16, FN = WN / 16;
  static_assert(FM >= 1 && FN >= 1 && WM % 16 == 0 && WN % 16 == 0, "wave tile");
  constexpr int NG = KC / 8, NKS = KC / 32;
  constexpr int UA = BN * NG, UB = BM * NG;  // 16-byte staging units of a chunk
  constexpr int NA = (UA + 255) / 256, NB = (UB + 255) / 256;
  constexpr int BUF = (BN + BM) * KC;       // bf16 elements of one stage buffer
  constexpr bool NOL = MODE == MODE_FWD_NOL;
  constexpr bool BNS = MODE == MODE_DGRAD_BNS;
  constexpr bool FWD = is_fwd<MODE>();

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const IgemmLds L = igemm_lds(BM, BN, WAM, KC, 2, pl.ntab, conv_nconst(MODE, a.Cs, BN));
  bf16_t* s_buf = reinterpret_cast<bf16_t*>(smem);
  int* s_tx = reinterpret_cast<int*>(smem + L.tx);
  int* s_tw = reinterpret_cast<int*>(smem + L.tw);
  float* s_st = reinterpret_cast<float*>(smem + L.t.st);
  float* s_k = reinterpret_cast<float*>(smem + L.t.k);
  int* s_flag = reinterpret_cast<int*>(smem + L.t.flag);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int l16 = lane & 15, kgl = lane >> 4;
  const int wn = wid % WAN, wm = wid / WAN;
  const IgemmBlk k = igemm_block_setup<BM, BN, KC>(a, pl, SELECT_PHASE(blk.x), blk, s_tx, s_tw);
  const int cb = k.cb, ce = k.ce;
  if (NOL) bn_prepare(a.nbn, k.z, s_k, s_k + a.Cs, nullptr, nullptr, blk.x == 0 && blk.y == 0);
  if (BNS) BNS_CONSTANTS(BN, k.z, k.nbase, s_k);

  // ---- staging units: unit u -> (row = 8 * (u / (8 NG)) + (u & 7), k-group g = (u >> 3) % NG)
  const ConvBases sb = conv_bases(a, k.z);
  int an[NA], aoff[NA];  // weight row (-1: none), LDS offset (16-byte units)
  int ag[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int u = tid + 256 * j;
    const int rest = u >> 3, g = rest % NG, row = (rest / NG) * 8 + (u & 7);
    const int n = k.nbase + row;
    an[j] = (u < UA && n < a.Npad) ? n : -1;
    ag[j] = g;
    aoff[j] = g * BN + row;
  }
  int pb[NB], pih[NB], piw[NB], bg[NB], boff[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int u = tid + 256 * j;
    const int rest = u >> 3, g = rest % NG, row = (rest / NG) * 8 + (u & 7);
    igemm_row_pixel(k, pl, row, u < UB, pb[j], pih[j], piw[j]);
    bg[j] = g;
    boff[j] = g * BM + row;
  }

  uint4 ra[NA], rb[NB];
  uint32_t bok = 0;
  auto load_chunk = [&](int ch) {
    const int t0 = (ch - cb) * NG;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int e = s_tw[t0 + ag[j]];
      ra[j] = (an[j] >= 0 && e >= 0) ? *reinterpret_cast<const uint4*>(sb.wz + (int64_t)an[j] * a.Kpad + e)
                                      : make_uint4(0, 0, 0, 0);
    }
    bok = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const bf16_t* src;
      const bool ok = igemm_src(a, sb, s_tx[t0 + bg[j]], pb[j], pih[j], piw[j], src);
      rb[j] = make_uint4(0, 0, 0, 0);
      if (ok) rb[j] = *reinterpret_cast<const uint4*>(src);
      bok |= (uint32_t)ok << j;
    }
  };
  const bool nol_relu = a.nol_kind == ACT_RELU;
  auto store_chunk = [&](int buf, int ch) {
    bf16_t* A = s_buf + buf * BUF;
    bf16_t* B = A + BN * KC;
#pragma unroll
    for (int j = 0; j < NA; ++j)
      if (tid + 256 * j < UA) *reinterpret_cast<uint4*>(A + aoff[j] * 8) = ra[j];
    const int t0 = (ch - cb) * NG;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (tid + 256 * j >= UB) continue;
      uint4 v = rb[j];
      if (NOL && ((bok >> j) & 1)) {
        const int c = s_tx[t0 + bg[j]] & 16383;
        v = nol8(v, s_k + c, s_k + a.Cs + c, nol_relu);
      }
      *reinterpret_cast<uint4*>(B + boff[j] * 8) = v;
    }
  };

  f32x4 acc[FN][FM];
  acc_zero(acc);

  __syncthreads();  // tables and constants
  if (cb < ce) {
    load_chunk(cb);
    store_chunk(0, cb);
  }
  __syncthreads();
  for (int ch = cb; ch < ce; ++ch) {
    const int cur = (ch - cb) & 1;
    if (ch + 1 < ce) load_chunk(ch + 1);  // in flight during this chunk's MFMAs
    const bf16_t* A = s_buf + cur * BUF;
    const bf16_t* B = A + BN * KC;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      bf16x8 afr[FN], bfr[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i)
        afr[i] = *reinterpret_cast<const bf16x8*>(A + ((s * 4 + kgl) * BN + wn * WN + i * 16 + l16) * 8);
#pragma unroll
      for (int f = 0; f < FM; ++f)
        bfr[f] = *reinterpret_cast<const bf16x8*>(B + ((s * 4 + kgl) * BM + wm * WM + f * 16 + l16) * 8);
      MFMA_STEP(acc, afr, bfr);
    }
    if (ch + 1 < ce) store_chunk(cur ^ 1, ch + 1);  // that buffer's last reader finished before the barrier
    __syncthreads();
  }

  const TileCtx tc = igemm_tile_ctx(a, k, blk, tid, wid, wn, wm);
  tile_epilogue<FWD, BNS, BM, BN, WAM, WM, WN, FN, FM>(a, pl, tc, acc, s_st, s_k, s_flag);
}

// ================================================================================================
// LDS-DMA variant (cfg >= CONV_GLDS_CFG0): the operand tiles go global -> LDS with
// global_load_lds_dwordx4 (no register hop, no ds_write pass), through a 3-stage ring of LDS buffers with
// one raw s_barrier per K chunk and a counted vmcnt that keeps the next chunk's DMAs in flight ACROSS the
// barrier (a __syncthreads() would emit vmcnt(0) and drain them).
//
// LDS image of an operand chunk (KC = 64): [row][8 k-groups] with 128-byte rows; k-group g of row r sits
// in 16-byte slot g ^ ((r >> 1) & 7).  An LDS-DMA instruction writes 64 lanes x 16 B contiguously (8 rows),
// so the swizzle is applied on the per-lane SOURCE address (lane l of the instruction fetches k-group
// (l & 7) ^ ((row >> 1) & 7) of row 8i + (l >> 3)) and again on the fragment read; with it the four 16-lane
// groups of every ds_read_b128 of a 16x16x32 MFMA fragment (16 rows, one k-group each) hit 16 distinct
// 16-byte slots of the 256-byte bank row -- conflict-free.  Padding (zero rows / taps outside the image /
// k beyond K) is a DMA from a 16-byte zero page, so every lane always issues its instruction.
constexpr int GL_NT = 8;  // tile configs: BM pixels x BN channels, WAM waves along M
constexpr int GL_BM[GL_NT] = {64, 128, 64, 128, 256, 128, 256, 64};
constexpr int GL_BN[GL_NT] = {64, 64, 128, 128, 64, 32, 128, 32};
constexpr int GL_WAM[GL_NT] = {2, 2, 2, 2, 4, 4, 2, 4};
constexpr int GL_KC = 64, GL_STAGES = 3;
// ring stages of the deep configs: as many 128-byte-row stages as fit ~150 KB of LDS, at most 8, and at
// most 2 + 63 / NPER (the counted vmcnt of NST - 2 chunks in flight must fit the 6-bit counter); 3 = none
constexpr int GL_NST_DEEP[GL_NT] = {8, 6, 6, 4, 3, 7, 3, 8};

__device__ uint4 g_zero16[4];  // never written: the source of every padding lane

typedef __attribute__((address_space(3))) void* lds_vptr;
typedef __attribute__((address_space(1))) void* glb_vptr;

DEV int gl_swz(int r, int g) { return g ^ ((r >> 1) & 7); }

// wait until at most `ahead` chunks (NPER DMA instructions each) of this wave are still in flight
template <int NPER, int NST>
DEV void gl_wait_ahead(int ahead) {
  static_assert((NST - 2) * NPER <= 63, "vmcnt is a 6-bit counter");
  switch (ahead) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NPER) : "memory"); break;
    case 2: if constexpr (NST > 3) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NPER) : "memory"); break; }
            [[fallthrough]];
    case 3: if constexpr (NST > 4) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * NPER) : "memory"); break; }
            [[fallthrough]];
    case 4: if constexpr (NST > 5) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * NPER) : "memory"); break; }
            [[fallthrough]];
    case 5: if constexpr (NST > 6) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * NPER) : "memory"); break; }
            [[fallthrough]];
    default: if constexpr (NST > 7) { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * NPER) : "memory"); break; }
             asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

// NST = stages of the LDS ring: 3 (GL_STAGES, the streaming configs) or up to 8 for the "deep" configs,
// whose blocks issue the DMAs of up to NST - 1 K chunks before waiting for the first -- a block of a
// small-M, long-K layer (Model C's 4x13 / 1x6 Inception convs) pays ONE load latency instead of a chain
// of them.
template <int MODE, int BM, int BN, int WAM, int NST>
__global__ __launch_bounds__(256) void conv_glds_kernel(ConvArgs a, LdsPlan pl) {
  const Blk blk = block_coords(a.xcd);
  constexpr int WAN = 4 / WAM;
  constexpr int WM = BM / WAM, WN = BN / WAN, FM = WM / 16, FN = WN / 16;
  static_assert(FM >= 1 && FN >= 1 && WM % 16 == 0 && WN % 16 == 0, "wave tile");
  constexpr int KC = GL_KC, NG = KC / 8, NKS = KC / 32, ROWB = KC * 2;  // 128-byte rows
  constexpr int IA = BN / 32, IB = BM / 32;  // DMA instructions per wave per chunk (8 rows each)
  static_assert(IA >= 1 && IB >= 1, "tile too small for 4 waves x 8 rows");
  constexpr int NPER = IA + IB;
  constexpr int BUF = (BN + BM) * ROWB;  // bytes of one stage
  constexpr bool BNS = MODE == MODE_DGRAD_BNS;
  constexpr bool FWD = MODE == MODE_FWD;
  static_assert(MODE != MODE_FWD_NOL, "the DMA bypasses registers: no on-load transform");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const IgemmLds L = igemm_lds(BM, BN, WAM, KC, NST, pl.ntab, conv_nconst(MODE, a.Cs, BN));
  int* s_tx = reinterpret_cast<int*>(smem + L.tx);
  int* s_tw = reinterpret_cast<int*>(smem + L.tw);
  float* s_st = reinterpret_cast<float*>(smem + L.t.st);
  float* s_k = reinterpret_cast<float*>(smem + L.t.k);
  int* s_flag = reinterpret_cast<int*>(smem + L.t.flag);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, kgl = lane >> 4;
  const int wn = wid % WAN, wm = wid / WAN;
  const IgemmBlk k = igemm_block_setup<BM, BN, KC>(a, pl, SELECT_PHASE(blk.x), blk, s_tx, s_tw);
  const int cb = k.cb, ce = k.ce;
  if (BNS) BNS_CONSTANTS(BN, k.z, k.nbase, s_k);

  // ---- per-lane DMA sources: instruction j of wave w covers rows 8 (4j + w) .. +7; this lane fetches
  // k-group ga / gb (swizzled) of row 8 (4j + w) + (lane >> 3)
  const ConvBases sb = conv_bases(a, k.z);
  const void* zero = &g_zero16[0];
  int an[IA], ga[IA];
#pragma unroll
  for (int j = 0; j < IA; ++j) {
    const int row = 8 * (4 * j + wid) + (lane >> 3);
    const int n = k.nbase + row;
    an[j] = n < a.Npad ? n : -1;
    ga[j] = gl_swz(row, lane & 7);
  }
  int pb[IB], pih[IB], piw[IB], gb[IB];
#pragma unroll
  for (int j = 0; j < IB; ++j) {
    const int row = 8 * (4 * j + wid) + (lane >> 3);
    igemm_row_pixel(k, pl, row, true, pb[j], pih[j], piw[j]);
    gb[j] = gl_swz(row, lane & 7);
  }
  auto issue = [&](int ch, int buf) {
    char* A = smem + buf * BUF;
    char* Bq = A + BN * ROWB;
    const int t0 = (ch - cb) * NG;
#pragma unroll
    for (int j = 0; j < IA; ++j) {
      const int e = s_tw[t0 + ga[j]];
      const void* src = (an[j] >= 0 && e >= 0) ? (const void*)(sb.wz + (int64_t)an[j] * a.Kpad + e) : zero;
      __builtin_amdgcn_global_load_lds((glb_vptr)src, (lds_vptr)(A + (4 * j + wid) * 8 * ROWB), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < IB; ++j) {
      const bf16_t* px;
      const void* src = zero;
      if (igemm_src(a, sb, s_tx[t0 + gb[j]], pb[j], pih[j], piw[j], px)) src = px;
      __builtin_amdgcn_global_load_lds((glb_vptr)src, (lds_vptr)(Bq + (4 * j + wid) * 8 * ROWB), 16, 0, 0);
    }
  };

  f32x4 acc[FN][FM];
  acc_zero(acc);

  __syncthreads();  // tables and constants (no DMA in flight yet)
#pragma unroll
  for (int j = 0; j < NST - 1; ++j)
    if (cb + j < ce) issue(cb + j, j);
  for (int ch = cb; ch < ce; ++ch) {
    const int kc = ch - cb;
    // this wave's DMAs of chunk ch have landed (the up to NST - 2 later chunks may still fly), then every
    // wave's have, and every wave is done reading chunk ch - 1 (whose buffer chunk ch + NST - 1 overwrites)
    gl_wait_ahead<NPER, NST>(min(ce - 1, ch + NST - 2) - ch);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (ch + NST - 1 < ce) issue(ch + NST - 1, (kc + NST - 1) % NST);
    const char* A = smem + (kc % NST) * BUF;
    const char* Bq = A + BN * ROWB;
#pragma unroll
    for (int s = 0; s < NKS; ++s) {
      const int g = 4 * s + kgl;
      bf16x8 afr[FN], bfr[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const int row = wn * WN + i * 16 + l16;
        afr[i] = *reinterpret_cast<const bf16x8*>(A + row * ROWB + gl_swz(row, g) * 16);
      }
#pragma unroll
      for (int f = 0; f < FM; ++f) {
        const int row = wm * WM + f * 16 + l16;
        bfr[f] = *reinterpret_cast<const bf16x8*>(Bq + row * ROWB + gl_swz(row, g) * 16);
      }
      MFMA_STEP(acc, afr, bfr);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the stage buffers are dead; s_st / s_flag live past them
  const TileCtx tc = igemm_tile_ctx(a, k, blk, tid, wid, wn, wm);
  tile_epilogue<FWD, BNS, BM, BN, WAM, WM, WN, FN, FM>(a, pl, tc, acc, s_st, s_k, s_flag);
}

#undef SELECT_PHASE
#undef PSEL

// ---- host-side plan
struct LdsCfg {
  int tile, BM, BN, WAM, KC, splits;
  bool glds;  // LDS-DMA kernel (conv_glds_kernel)
  int nst;    // stage buffers: its ring stages, 2 for conv_lds_kernel
};

int decode_cfg(int cfg, LdsCfg& c) {
  const bool deep = cfg >= CONV_GDEEP_CFG0 && cfg < CONV_GDEEP_CFG0 + CONV_GDEEP_NCFG;
  c.glds = deep || (cfg >= CONV_GLDS_CFG0 && cfg < CONV_GLDS_CFG0 + CONV_GLDS_NCFG);
  if (c.glds) {  // cfg = CONV_GLDS_CFG0 (or CONV_GDEEP_CFG0) + 4 * tile + log2(splits)
    const int k = cfg - (deep ? CONV_GDEEP_CFG0 : CONV_GLDS_CFG0);
    c.tile = k / 4;
    c.KC = GL_KC;
    c.splits = 1 << (k % 4);
    c.BM = GL_BM[c.tile]; c.BN = GL_BN[c.tile]; c.WAM = GL_WAM[c.tile];
    c.nst = deep ? GL_NST_DEEP[c.tile] : GL_STAGES;
    if (deep && c.nst <= GL_STAGES) return -2;  // no deeper ring fits this tile
    return 0;
  }
  const int k = cfg - CONV_LDS_CFG0;
  if (k < 0 || k >= CONV_LDS_NCFG) return -1;
  c.tile = k / 8;
  c.KC = (k / 4) % 2 ? 128 : 64;
  c.splits = 1 << (k % 4);
  c.BM = LDS_BM[c.tile]; c.BN = LDS_BN[c.tile]; c.WAM = LDS_WAM[c.tile];
  c.nst = 2;
  if (c.KC == 128 && c.BM + c.BN > 192) return -2;  // LDS: two 128-deep stages of a 256-row tile
  return 0;
}

// Phases, grid, table size and LDS bytes of a launch.  dgrad: ConvArgs Hs/Ws = dy, Ho/Wo = dx (the conv's input).
int make_plan(int mode, const ConvArgs& a, const LdsCfg& c, LdsPlan& pl, int& gx, size_t& lds) {
  pl = LdsPlan{};
  pl.splits = c.splits;
  int maxch = 0;
  if (mode == MODE_FWD || mode == MODE_FWD_NOL) {
    pl.nph = 1;
    pl.mh = a.sh; pl.mw = a.sw; pl.by = 1; pl.bx = 1; pl.th = 1; pl.tw = 1; pl.qy = 1; pl.qx = 1;
    LdsPhase& P = pl.ph[0];
    P.oy0 = 0; P.ox0 = 0; P.Hq = a.Ho; P.Wq = a.Wo;
    P.rh = 0; P.nh = a.KH; P.rw = 0; P.nw = a.KW;
    P.ay = -a.ph; P.ax = -a.pw;
  } else {
    pl.mh = 1; pl.mw = 1; pl.by = -1; pl.bx = -1; pl.th = a.sh; pl.tw = a.sw; pl.qy = a.sh; pl.qx = a.sw;
    const int nphy = std::min(a.sh, a.Ho), nphx = std::min(a.sw, a.Wo);
    if (nphy < 1 || nphx < 1 || nphy * nphx > 4) return -2;  // pl.ph holds 4 phases (stride 3 would write 9)
    int n = 0;
    for (int py = 0; py < nphy; ++py)
      for (int px = 0; px < nphx; ++px) {
        LdsPhase& P = pl.ph[n++];
        P.oy0 = py; P.ox0 = px;
        P.Hq = (a.Ho - py + a.sh - 1) / a.sh;
        P.Wq = (a.Wo - px + a.sw - 1) / a.sw;
        P.rh = (py + a.ph) % a.sh;
        P.rw = (px + a.pw) % a.sw;
        P.nh = P.rh < a.KH ? (a.KH - P.rh + a.sh - 1) / a.sh : 0;
        P.nw = P.rw < a.KW ? (a.KW - P.rw + a.sw - 1) / a.sw : 0;
        P.ay = (py + a.ph - P.rh) / a.sh;
        P.ax = (px + a.pw - P.rw) / a.sw;
      }
    pl.nph = n;
  }
  gx = 0;
  for (int p = 0; p < pl.nph; ++p) {
    LdsPhase& P = pl.ph[p];
    const int k = P.nh * P.nw * a.Cs;
    P.Kp = (k + c.KC - 1) / c.KC * c.KC;
    P.m0 = gx;
    gx += (a.B * P.Hq * P.Wq + c.BM - 1) / c.BM;
    maxch = std::max(maxch, (P.Kp / c.KC + c.splits - 1) / c.splits);
    if (std::abs(P.ay) > 56 || std::abs(P.ax) > 56 || a.KH > 56 || a.KW > 56) return -2;
  }
  pl.ntab = std::max(4, maxch * (c.KC / 8));
  if (c.glds && mode == MODE_FWD_NOL) return -2;  // the DMA bypasses registers: no on-load transform
  lds = igemm_lds(c.BM, c.BN, c.WAM, c.KC, c.nst, pl.ntab, conv_nconst(mode, a.Cs, c.BN)).t.bytes;
  return lds > CONV_LDS_MAX ? -2 : 0;
}

template <int MODE>
int launch_glds(const ConvArgs& a, const LdsCfg& c, const LdsPlan& pl, dim3 grid, size_t lds, hipStream_t st) {
  if constexpr (MODE == MODE_FWD_NOL) {
    return -2;  // make_plan rejects it (conv_lds_kernel / conv_igemm normalise on load)
  } else {
#define GL_LAUNCH_N(T, NS)                                                                                \
  if (c.tile == T && c.nst == NS) {                                                                       \
    hipLaunchKernelGGL((conv_glds_kernel<MODE, GL_BM[T], GL_BN[T], GL_WAM[T], NS>), grid, dim3(256), lds, st, a, pl); \
    return (int)hipGetLastError();                                                                        \
  }
#define GL_LAUNCH(T) GL_LAUNCH_N(T, GL_STAGES) if constexpr (GL_NST_DEEP[T] > GL_STAGES) { GL_LAUNCH_N(T, GL_NST_DEEP[T]) }
    GL_LAUNCH(0) GL_LAUNCH(1) GL_LAUNCH(2) GL_LAUNCH(3) GL_LAUNCH(4) GL_LAUNCH(5) GL_LAUNCH(6) GL_LAUNCH(7)
#undef GL_LAUNCH
#undef GL_LAUNCH_N
    return -1;
  }
}

template <int MODE>
int launch_mode(const ConvArgs& a, int G, const LdsCfg& c, hipStream_t st) {
  LdsPlan pl;
  int gx;
  size_t lds;
  int rc = make_plan(MODE, a, c, pl, gx, lds);
  if (rc) return rc;
  if (c.splits > 1 && (!a.ws || !a.cnt)) return -3;
  dim3 grid(gx, (a.N + c.BN - 1) / c.BN * c.splits, G);
  if (c.glds) return launch_glds<MODE>(a, c, pl, grid, lds, st);
#define LDS_LAUNCH(T, KC_)                                                                               \
  if (c.tile == T && c.KC == KC_) {                                                                      \
    hipLaunchKernelGGL((conv_lds_kernel<MODE, LDS_BM[T], LDS_BN[T], LDS_WAM[T], KC_>), grid, dim3(256), lds, st, a, pl); \
    return (int)hipGetLastError();                                                                       \
  }
  LDS_LAUNCH(0, 64) LDS_LAUNCH(0, 128) LDS_LAUNCH(1, 64) LDS_LAUNCH(1, 128) LDS_LAUNCH(2, 64) LDS_LAUNCH(2, 128)
  LDS_LAUNCH(3, 64) LDS_LAUNCH(4, 64) LDS_LAUNCH(4, 128) LDS_LAUNCH(5, 64) LDS_LAUNCH(5, 128) LDS_LAUNCH(6, 64)
  LDS_LAUNCH(6, 128) LDS_LAUNCH(7, 64) LDS_LAUNCH(7, 128)
#undef LDS_LAUNCH
  return -1;
}

}  // namespace

int conv_lds_workspace(int mode, const ConvArgs& a, int G, int cfg, int64_t& ws_floats, int64_t& ntickets) {
  cfg &= ~CONV_XCD;
  if (mode == MODE_FWD && a.nol) mode = MODE_FWD_NOL;  // the launch mode launch_conv will pick
  if (mode == MODE_DGRAD && a.bpart) mode = MODE_DGRAD_BNS;
  if (conv_patch_cfg(cfg)) {
    ws_floats = 0;
    ntickets = 0;
    return conv_patch_check(mode, a, cfg);
  }
  LdsCfg c;
  int rc = decode_cfg(cfg, c);
  if (rc) return rc;
  LdsPlan pl;
  int gx;
  size_t lds;
  rc = make_plan(mode, a, c, pl, gx, lds);
  if (rc) return rc;
  const int64_t tiles = (int64_t)G * gx * ((a.N + c.BN - 1) / c.BN);
  ws_floats = c.splits > 1 ? tiles * c.splits * c.BM * c.BN : 0;
  ntickets = c.splits > 1 ? tiles : 0;
  return 0;
}

int launch_conv_lds(int mode, const ConvArgs& a, int G, int cfg, hipStream_t st) {
  if (conv_patch_cfg(cfg)) return launch_conv_patch(mode, a, G, cfg, st);
  LdsCfg c;
  int rc = decode_cfg(cfg, c);
  if (rc) return rc;
  switch (mode) {
    case MODE_FWD: return launch_mode<MODE_FWD>(a, G, c, st);
    case MODE_FWD_NOL: return launch_mode<MODE_FWD_NOL>(a, G, c, st);
    case MODE_DGRAD: return launch_mode<MODE_DGRAD>(a, G, c, st);
    case MODE_DGRAD_BNS: return launch_mode<MODE_DGRAD_BNS>(a, G, c, st);
    default: return -1;
  }
}

}  // namespace mda
