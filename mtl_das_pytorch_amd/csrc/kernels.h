// Kernel argument structs and host launch entry points of the mtl_das_pytorch_amd HIP library.
// Every launcher enqueues on the given stream (PyTorch's current stream, so HIP-graph capture works)
// and returns hipGetLastError() (negative = rejected arguments).
#pragma once
#include "common.h"

namespace mda {

// 2: dgrad + fused BN-backward statistics; 3: forward with normalise-on-load of its input
enum { MODE_FWD = 0, MODE_DGRAD = 1, MODE_DGRAD_BNS = 2, MODE_FWD_NOL = 3 };

struct ConvArgs {
  Src2 src;
  const bf16_t* w;  // packed [Npad][Kpad] (+ z * wgs)
  int64_t wgs;
  const float* bias;  // FWD only, may be null
  int64_t bgs;
  void* out;  // bf16 [M][ldo] (+ z * ogs): FWD the pre-BN y, DGRAD the data gradient
  int64_t ogs;
  int ldo;
  double* stats;  // FWD: [G][NREP][2][N] fp64 (may be null); replica blockIdx.x % stats_nrep
  int stats_nrep;
  int B, Hs, Ws, Ho, Wo;
  int N, Npad, Cs;
  int KH, KW, sh, sw, ph, pw;
  int Kpad;
  // DGRAD only, optional (bpart null = off): fused BN-backward statistics.  When this dgrad's output is
  // the ONLY gradient source of a BN tail with an elementwise activation (ACT_NONE / ACT_RELU /
  // ACT_SIGMOID), the epilogue recomputes that tail's dz from the stored pre-BN y and accumulates
  // sum(dz), sum(dz * xhat) per channel into the tail's fp64 replica rows ([G][NREP][3][N], rows 0/1) --
  // the tail backward then runs its apply pass only (bn.hip launch_tail_bwd, fused == 2).
  const bf16_t* by; int64_t bygs; int ldby;
  BNArgs bbn;
  double* bpart;
  int bkind;
  // ... generalised to ONE OF SEVERAL gradient sources (statistics are linear in the gradient, so every
  // producer adds its share): bkind ACT_RELU or ADD_RELU, whose dz mask is relu'(BN(y) + r') with the
  // residual r' = r (identity shortcut) or BN2(r) (projection, br_bn = 1: third row sum(dz * xhat2)).
  // bN = the tail's channels (a concatenation gradient may have more: channels >= bN are not the tail's),
  // bpgs = group stride of bpart (-1: z * NREP * 3 * bN; 0: every group adds into the ONE tail of a
  // shared feature, whose BN constants are then group 0's).
  const bf16_t* br; int64_t brgs; int ldbr;
  BNArgs bbn2;
  int br_bn, bN;
  int64_t bpgs;
  // FWD only, optional (nol = 0 off): normalise-on-load.  The (single-segment) input is the previous
  // conv's pre-BN output y and the im2col operand is act(BN(y)) computed on load (act = nol_kind: ACT_NONE
  // or ACT_RELU), so the forward BN tail that materialised act(BN(y)) is not launched.  Block (0, 0) of each
  // group updates that BN's running statistics and publishes its constants (BNArgs::consts).
  BNArgs nbn;
  int nol, nol_kind;
  // DGRAD only, optional (nadd = 0 off): up to 3 more bf16 gradient sources of the same [M][N] tensor
  // ([M][ldadd] + z * addgs) added (in fp32, before the one rounding) in the epilogue, so the output is the
  // WHOLE gradient of the BN tail it feeds (one source: its statistics can then be fused above, and the
  // tail runs apply-only)
  const bf16_t* add[3];
  int64_t addgs[3];
  int ldadd[3];
  int nadd;
  // LDS-staged kernels (cfg >= CONV_LDS_CFG0, conv_lds.hip) with a cross-block split of K: fp32 partial
  // tiles [G][tiles][splits][BM*BN] and one arrival ticket per output tile (zero-initialised; the reducing
  // block resets it), sized by conv_lds_workspace
  float* ws;
  unsigned* cnt;
  int xcd;  // block_coords remap (common.h): XCD-contiguous tile order (set from the CONV_XCD cfg flag)
  uint64_t* ptm;  // optional per-block phase timers (common.h ptick; profiling only)
};

// ConvArgs::add: the extra gradient sources of output element (row m, channels n0 .. n0+3), added in order
DEV void add_sources(const ConvArgs& a, int z, int64_t m, int n0, float* v) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (s < a.nadd) {
      float q[4];
      load4(a.add[s] + a.addgs[s] * z + m * a.ldadd[s] + n0, q);
      v[0] += q[0]; v[1] += q[1]; v[2] += q[2]; v[3] += q[3];
    }
  }
}

// One output-pixel phase of an LDS-staged conv launch (conv_lds.hip): output pixels (b, oy0 + i*qy,
// ox0 + j*qx) for i < Hq, j < Wq, reduced over taps (kh, kw) = (rh + th*u, rw + tw*v), u < nh, v < nw,
// whose input pixel is (i*mh + ay + by*u, j*mw + ax + bx*v).  The forward is one phase; a strided data
// gradient has one phase per output parity (sub-pixel decomposition: only the taps that hit a real dy).
struct LdsPhase {
  int oy0, ox0, Hq, Wq;
  int rh, nh, rw, nw;
  int ay, ax;
  int m0;   // first blockIdx.x of the phase
  int Kp;   // nh * nw * Cs padded to the K chunk
};
// Strip plan of a patch conv launch (conv_patch.hip conv_patch_kernel): R output rows per block, nstrip strips
// per image, nslice channel slices; source pixel of strip element (j, q) = (oh0 + dy0 + j, dx0 + q).
struct PatchPlan {
  int R, nstrip, nslice, Hout, Wout, dy0, dx0;
};
struct LdsPlan {
  LdsPhase ph[4];
  int nph;
  int mh, mw, by, bx, th, tw, qy, qx;
  int splits;  // cross-block split of the K chunks
  int ntab;    // per-block k-group table entries (LDS)
};

// ------------------------------------------------------------------------------------------------
// Weight gradient
// ------------------------------------------------------------------------------------------------
struct WgradArgs {
  Src2 src;          // forward input (bf16)
  const bf16_t* dy;  // [M][ldd] (+ z * dgs)
  int64_t dgs;
  int ldd;
  float* slab;       // [G][splits][Npad][Kpad]
  int splits, m_per_split;
  int B, Hi, Wi, Ho, Wo;
  int Co, Npad, Cs;
  int KH, KW, sh, sw, ph, pw;
  int Kpad;
  // optional (nol = 0 off): the forward conv normalised its input on load (ConvArgs::nol); the x operand is
  // rebuilt the same way from the BN constants the forward published ([G][4][Cs]: scale, shift, ...)
  const float* nol_consts;
  int nol, nol_kind;
};

// One conv of a horizontally batched weight-gradient launch (device table, built by wgrad_table).
struct WgradJob {
  WgradArgs a;
  int ntiles;      // (Npad / TN) * (Kpad / TK)
  int G;
  int64_t block0;  // first block of this job in the batched grid
};

// Sums the split-M partial slabs of many convolutions and scatters them into the flat fp32 gradient
// buffer in the reference weight layout [Cout][Cin][KH][KW] (deterministic, one launch per backward).
struct WgFinDesc {
  const float* slab;  // [G][splits][Npad][Kpad]
  float* grad;        // NCHW weight grad of group 0
  int64_t ggs;        // element stride between groups in the flat grad buffer
  int G, splits, Npad, Kpad, Co, Ci, Cs, KH, KW;
  int lanes;          // threads per weight (power of two <= 16): the splits are summed in lanes x parallel
  int order;          // 1: output (NCHW) order, lanes == 1, FIN_EPT weights per thread; 0: slab order
  int _pad;
  int64_t elems;      // G * Co * Ci * KH * KW (order 1); G * Co * KH * KW * Cs (order 0)
  int64_t block0;     // first block index of this descriptor
};
// weights per thread of wgrad_finalize's output-order mapping (order 1): a block owns FIN_EPT * 256
// consecutive NCHW weights
constexpr int FIN_EPT = 2;  // measured 1 / 2 / 4 / 8: C 130 / 101 / 105 / 160 us, A 18.4 / 18.2 / 21.1 / - us

enum TailKind { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2, SIGMUL = 3, ADD_RELU = 4, POOL_RELU = 5 };

struct TailArgs {
  const bf16_t* y; int64_t ygs; int ldy;
  BNArgs bn;
  const bf16_t* r; int64_t rgs; int ldr;  // SIGMUL: multiplier; ADD_RELU: residual (raw x or y2)
  BNArgs bn2; int r_bn;
  bf16_t* out; int64_t ogs; int ldo;
  int B, H, W, C;
  // backward only
  GradSrcs g;                       // upstream bf16 gradient(s) on the tail's output grid
  double* part; int chunk_px;       // [G][NREP][3][C] fp64 replica sums (zeroed per step); pixels per chunk
  bf16_t* dzbuf; int64_t dzgs; int lddz;  // optional dz store (reduce) / load (apply), bf16
  bf16_t* side; int64_t sgs; int lds;     // side gradient output (bf16)
  bf16_t* dy; int64_t dgs; int ldd;
  bf16_t* dy2; int64_t d2gs; int ldd2;
  float* dgamma; float* dbeta; float* dgamma2; float* dbeta2; int64_t pgs;
  uint64_t* tsc;                    // optional phase timestamps (profiling; null in production)
  uint64_t* ptm;                    // optional per-block phase timers (common.h ptick; profiling only)
  // apply-only backward (fused = 2) of a multi-source tail: no reduce pass ran, so the apply pass stores
  // the side output itself (apply_side)
  int apply_side;
  float gscale;                     // factor on the d(gamma), d(beta) the apply writes (SyncBN: 1 / world)
};

struct TailJob {  // one tail of a batched forward-tail launch (bn.hip tail_fwd_batched_kernel)
  TailArgs a;
  int blocks;      // blocks of this tail (its grid x), one group (z = 0)
  int block0;      // first block of this tail in the batched grid
};

struct HeadArgs {
  const bf16_t* feat; int64_t fgs; int ldf;  // per task [B*HW][C] (+ t * fgs)
  const int64_t* labels; int lab_stride, lab_off;  // label of (b, t) = labels[b*lab_stride + lab_off + t]
  int T, B, HW, C;
  int ncls[4];
  float w[4];
  float* logp;      // [T][B][16]
  bf16_t* dfeat;    // [T][B*HW][C] bf16 (+ t * dgs), may be null (eval)
  int64_t dgs;
  float* metrics;   // [T][4]: loss_sum, correct, count, abs_err_sum
  int* confusion;   // [T][16][16]
  // samples b >= *nvalid are padding (may be null: none): they are left out of metrics and confusion only.
  // logp and the gradient are written for all B rows, the gradient scaled by 1/B; training always runs with
  // *nvalid == B
  const int64_t* nvalid;
};

struct ClsArgs {
  const bf16_t* x; int ldx;      // [B*HW][C] last feature map
  const float* W; const float* bias;  // fc [N][C], [N]
  const int64_t* labels;         // joint labels [B]
  int B, HW, C, N;
  float p_drop;                  // dropout probability (0 in eval)
  const int64_t* seed;           // device counter (advanced by cls_wgrad each training step)
  float* feat;                   // [B][C] post-dropout features (fp32)
  float* logits;                 // [B][N]
  float* dlogits;                // [B][N] (training)
  bf16_t* dx;                    // [B*HW][C] bf16 grad (training), may be null
  float* metrics;                // [3][4]: joint, distance, event -> loss, correct, count, abs_err
  int* confusion;                // [2][16][16]: distance, event
  float* dW; float* db;          // flat-grad slots (cls_wgrad)
  // samples b >= *nvalid are padding (may be null: none): they are left out of metrics and confusion only.
  // logits and the gradients are written for all B rows, the gradients scaled by 1/B; training always runs
  // with *nvalid == B
  const int64_t* nvalid;
};

// ------------------------------------------------------------------------------------------------
struct PoolArgs {
  const bf16_t* x; int ldx;     // input [B*H*W][C] (bf16)
  bf16_t* y; int ldy;           // output [B*Ho*Wo][C]
  GradSrcs g;                   // backward: grad of output = sum of bf16 sources (concat consumers)
  bf16_t* dx; int lddx;         // backward: grad of input (bf16)
  int B, H, W, C, Ho, Wo;
  uint8_t* am;                  // optional max-pool argmax (window position 0..8) [B*Ho*Wo][C]: written by
                                // the training forward, read by the backward instead of re-reading the windows
};

struct OptSeg {
  int64_t off, n;
  int kind;  // 0 = plain flat range, 3 = conv weight with both images (optim.hip adam_pack_kernel)
  bf16_t* wf;
  bf16_t* wd;
  int Co, Ci, KH, KW, Cs, Kpad_f, Kpad_d;
  // members of a horizontally fused conv (engine/core.py ConvLayer concat): the member's image is a window of
  // the group's -- kext_f = forward-image columns this member writes per row (its own taps, embedded at the
  // group's tap offset by the wf pointer; 0 = Kpad_f), tap_ld = data-gradient-image column stride between taps
  // (the group's Cout; 0 = Co)
  int kext_f, tap_ld;
  int64_t block0;
};

// Conv-weight tiles of the fused Adam + pack (optim.hip adam_pack_kernel): PACK_TCO co x pack_tile_ci(taps) ci x
// all taps (~2K elements: 256 ci of a 1x1, 24 of a 3x3, 8 of a 7x7), staged in LDS rows of at most
// PACK_TILE_FLOATS floats; keep in sync with engine/core.py build_optseg_table.
constexpr int PACK_TCO = 8, PACK_TILE_FLOATS = 512;
__host__ __device__ inline int pack_tile_ci(int taps) { return std::max(8, (256 / taps) & ~7); }

struct AdamArgs {
  float* p; const float* g; float* m; float* v;
  int64_t n;  // flat buffer length (multiple of 4)
  const float* lr; const float* step;  // device scalars (step = number of completed steps)
  float b1, b2, eps, wd, grad_scale;
  int update;  // 0: pack only
  int inc_step;  // advance the step counter after the update (0: a partial update -- another launch of the step does)
  int t_pre;     // 1: this step already advanced the counter (launch_step_inc at the step's start): t = step, else
                 // t = step + 1
  int64_t* cursor;  // optional: the batch-index schedule's cursor (gather_batch), advanced with the step counter
};
// the step counter (+ the schedule cursor) advanced by one thread: after the update (launch_adam_pack, inc_step)
// or early in the step on a side stream (AdamArgs::t_pre)
int launch_step_inc(float* step, int64_t* cursor, hipStream_t st);

int launch_conv(int mode, const ConvArgs& a, int G, int cfg, hipStream_t st);
// LDS-staged implicit GEMM (conv_lds.hip): cfg = CONV_LDS_CFG0 + 8 * tile + 4 * (KC == 128) + log2(splits)
constexpr int CONV_LDS_CFG0 = 16, CONV_LDS_NCFG = 64;
// register-pipelined conv_igemm tiles 0-13 at pipeline depth 4 (conv.hip): cfg = CONV_DEEP_CFG0 + tile
constexpr int CONV_DEEP_CFG0 = 128, CONV_DEEP_NCFG = 14;
// LDS-DMA implicit GEMM (conv_lds.hip conv_glds_kernel): cfg = CONV_GLDS_CFG0 + 4 * tile + log2(splits)
constexpr int CONV_GLDS_CFG0 = 160, CONV_GLDS_NCFG = 32;
// patch conv for 3x3 / stride-1 layers (conv_patch.hip conv_patch_kernel): cfg = CONV_PATCH_CFG0 + 3 * tile + cb
// (tile: BM x BN of PT_BM / PT_BN, cb: channel slice 16 / 32 / 64)
constexpr int CONV_PATCH_CFG0 = 192, CONV_PATCH_NCFG = 15;
// deep-ring LDS-DMA configs (conv_glds_kernel with up to 8 stages): cfg = CONV_GDEEP_CFG0 + 4 * tile + log2(splits)
constexpr int CONV_GDEEP_CFG0 = 208, CONV_GDEEP_NCFG = 32;
// persistent, DMA-pipelined patch conv (one channel slice): cfg = CONV_PATCHP_CFG0 + 3 * tile + cb
constexpr int CONV_PATCHP_CFG0 = 240, CONV_PATCHP_NCFG = 15;
// cfg flag of any conv config: launch it in XCD-contiguous tile order (ConvArgs::xcd, common.h block_coords)
constexpr int CONV_XCD = 4096;
// every LDS-staged config (mode: the kernel mode, MODE_FWD_NOL / MODE_DGRAD_BNS resolved); patch configs go on to
// launch_conv_patch
int launch_conv_lds(int mode, const ConvArgs& a, int G, int cfg, hipStream_t st);
inline bool conv_patch_cfg(int cfg) {
  return (cfg >= CONV_PATCH_CFG0 && cfg < CONV_PATCH_CFG0 + CONV_PATCH_NCFG) ||
         (cfg >= CONV_PATCHP_CFG0 && cfg < CONV_PATCHP_CFG0 + CONV_PATCHP_NCFG);
}
int launch_conv_patch(int mode, const ConvArgs& a, int G, int cfg, hipStream_t st);  // conv_patch.hip
int conv_patch_check(int mode, const ConvArgs& a, int cfg);  // 0, or < 0: the patch cfg cannot take this conv
// fp32 workspace floats and ticket count a cfg needs (0 when it does not split K); < 0: cfg invalid for a
int conv_lds_workspace(int mode, const ConvArgs& a, int G, int cfg, int64_t& ws_floats, int64_t& ntickets);
int launch_wgrad(const WgradArgs& a, int G, int cfg, hipStream_t st);
// weight-gradient configs: wgrad_tile.h; tiles per group of a wgrad launch, < 0: cfg invalid for a
int wgrad_ntiles(int cfg, const WgradArgs& a);
// cap > 0: at most cap hardware blocks walk the nblocks virtual blocks (persistent grid)
int launch_wgrad_batched(int cfg, const WgradJob* d_jobs, int nj, int64_t nblocks, hipStream_t st, int64_t cap = 0);
int launch_wgrad_finalize(const WgFinDesc* d_descs, int nd, int64_t nblocks, float scale, hipStream_t st);
int launch_tail_fwd(int kind, const TailArgs& a, int G, int blocks, hipStream_t st);
int launch_tail_fwd_batched(int kind, const TailJob* d_jobs, int nj, int nblocks, int maxC, hipStream_t st);
int launch_tail_bwd_batched(int kind, int cgb, int reduce, const TailJob* d_jobs, int nj, int nblocks, hipStream_t st);
int launch_tail_bwd(int kind, const TailArgs& a, int G, int blocks, int fused, hipStream_t st);
int launch_mtl_head(const HeadArgs& a, hipStream_t st);
int launch_cls_head(const ClsArgs& a, int64_t* seed_mut, hipStream_t st);
struct ZeroRanges {  // up to 4 16-byte-aligned regions a launch zeroes (gather_batch: the arena's zeroed buffers)
  uint4* p[4];
  int64_t n16[4];     // 16-byte units
  int n;
};
// The batch gather's arguments, the clean kernel's (misc.hip) and the noisy one's (augment.hip).  What both kernels
// and the window gathers share -- the schedule row, the clear, the label gather, the stem pixel and the limits
// gather_args_ok -- is in stem_gather.h.
struct GatherArgs {
  const float* X;         // resident dataset [N][Cin][H][W] fp32
  const int64_t* idx;     // [B] dataset rows, or with cursor a [nrows][B] schedule
  const int64_t* lab;     // [N][lab_w]
  int lab_w;
  bf16_t* out;            // [B][H][W][8]
  int64_t* lab_out;       // [B][lab_w]
  int B, Cin, H, W;
  int taps, off;          // vertical tap packing of a 1-channel stem (0: Cin real channels padded to 8)
  ZeroRanges zero;
  const int64_t* cursor;  // optional: the step gathers schedule row *cursor mod nrows
  int nrows;
};
// -2 on gather_args_ok
int launch_gather_batch(const GatherArgs& a, hipStream_t st);
// augment.hip: SNR noise injected by the batch gather (definition: data/noise.py).  Every level a run may change
// is a device value, so a captured step never needs re-capture.
struct NoiseArgs {
  const float* power;    // [N][Cin] mean power of each clean plane of the bound set (launch_sample_power)
  const float* snr;      // device (lo, hi) in dB: lo == hi is a fixed level, otherwise a per-sample uniform draw
  const int64_t* draw;   // device draw number (training: advanced once per step by launch_noise_advance)
  uint64_t seed;         // Philox key
  int stream;            // stream id of the Gaussian: 0 training, 2 evaluation (1 is the training SNR draw)
  float* dbg;            // test hook (null in the engine): the unrounded fp32 noisy values [B][Cin][H][W]
};
int launch_sample_power(const float* X, float* power, int64_t planes, int HW, hipStream_t st);
// launch_gather_batch with bf16(x + sigma * g) for every real element; -2 on gather_args_ok, a null noise input, a
// stream id outside 0..255 or a tap offset outside 0..7
int launch_gather_batch_noise(const GatherArgs& a, const NoiseArgs& noise, hipStream_t st);
int launch_noise_advance(int64_t* draw, hipStream_t st);
int launch_pool3(int is_max, int backward, const PoolArgs& a, hipStream_t st);
// window.hip / live.hip: sliding-window inference over a resident and over a growing recording.  What the two share
// -- the batch geometry and the selection below, the gather body, the selected numbering, the probability element,
// the fiber side of the maps and the launchers' common checks -- is in window_batch.h.
struct WindowGeom {
  const int* fs;      // window starts along the fiber [nf]
  int C, F, nf;       // channels and fiber rows of the source, fiber window count
  int B, Wf, Wt;      // batch rows, window size
  int taps, off;      // vertical tap packing of a 1-channel stem (gather_batch)
};
// The batch rows of a gather / probability launch numbered by an on-device selection (select_windows, live_select):
// in replay cur of a batch cursor, row r holds window sel[cur * B + r] while cur * B + r < min(*count, cap), and is
// padding beyond: gathered as zeros, skipped by the store, which advances the cursor by one.  sel and count come
// together; both null: no selection.
struct Selection {
  int64_t* sel;       // [cap]: the active window numbers, ascending
  int64_t* count;     // device scalar, read by every replay
  int64_t cap;
};
// window.hip: windows cut on the device from a recording [C][F][T], probabilities into a resident table,
// overlapping windows averaged into a cell map
struct WindowArgs {
  WindowGeom g;
  const float* rec;   // recording [C][F][T] fp32 (gather_windows only)
  const int* ts;      // window starts along time [nt]; window n = a * nt + b
  int T, nt;
  // batch row r holds window idx[r], or lo + *cursor * B + r (exactly one of idx / cursor is set), or the entry of
  // the selection s (with the cursor); a row whose window number is outside [lo, hi) is padding: gathered as zeros,
  // skipped by window_probs
  const int64_t* idx;
  int64_t* cursor;    // advanced by window_probs
  int64_t lo, hi;
  Selection s;
};
int launch_gather_windows(const WindowArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st);
// softmax = 0: src = logp [T][B][16], ncls[t] columns per task side by side (their sum is K); 1: src = logits [B][K]
int launch_window_probs(const WindowArgs& a, const float* src, int softmax, int T, const int* ncls, int K,
                        float* probs, int64_t nprobs, hipStream_t st);
struct MapArgs {
  const float* probs;  // [nf * nt][K]
  const int* fs;       // device copies of the start tables
  const int* ts;
  float* map;          // [K][nfc][ntc]
  // per-axis weights of a window in the cells it reaches, as bands (window_batch.h band_weight): wf [nf][mf] from
  // cell row fs[a] / cf on, wt [nt][mt] from cell column ts[b] / ct on; mf = (Wf - 1) / cf + 2, mt likewise
  const float* wf;
  const float* wt;
  int mf, mt;
  int nf, nt, K, F, T, Wf, Wt, cf, ct, nfc, ntc;
};
// h_fs / h_ts: host copies of the start tables, checked to cover [0, F) x [0, T) (-2 otherwise)
int launch_window_map(const MapArgs& a, const int* h_fs, const int* h_ts, hipStream_t st);
// gate.hip: the activity gate of resident-recording inference -- the windows' power and the ordered selection of the
// active ones, which gather_windows / window_probs take as WindowArgs::s
struct PowerArgs {
  const float* rec;   // recording [C][F][T] fp32
  const int* fs;      // window starts [nf], [nt]; window n = a * nt + b
  const int* ts;
  float* power;       // [nf * nt]: (1 / C) sum_c mean over the window of (x - the window's mean in c)^2
  int C, F, T, nf, nt, Wf, Wt;
};
int launch_window_power(const PowerArgs& a, hipStream_t st);
struct SelectArgs {
  const float* power;  // [N]
  const float* floor;  // [nfloor >= ceil(N / nt)]: the noise floor of fiber start n / nt
  float ratio;         // 10^(gate_db / 10): window n of [lo, hi) is active iff !(power[n] < floor[n / nt] * ratio)
  int64_t N, lo, hi, nfloor;
  int nt;
  uint8_t* active;     // [N]: the flags, zero outside [lo, hi)
  int64_t* sel;        // [cap >= hi - lo]: the active window numbers in ascending order; entries past the count
  int64_t cap;         // are left untouched
  int64_t* offs;       // workspace, one entry per block of 256 windows (select_blocks)
};
int64_t select_blocks(int64_t N);
// three launches (flags + block counts, scan of the counts, ranked scatter); count: device int64, the active windows
int launch_select_windows(const SelectArgs& a, int64_t* count, int64_t noffs, hipStream_t st);
// live.hip: inference on a growing recording -- the time axis as a ring of R columns, windows numbered time-major
// (n = j * nf + a: time index j starts at j * st), probabilities into a ring table, final map columns
enum { LIVE_TOTAL = 0, LIVE_AVAIL, LIVE_NEXT, LIVE_JEND, LIVE_TEND, LIVE_NSTATE };
struct LiveArgs {
  WindowGeom g;
  float* ring;        // [C][F][R] fp32: time sample t at column t mod R
  // device scalars [LIVE_NSTATE]: total = time samples received; avail = window numbers that can be evaluated;
  // next = the first window number not evaluated yet (batch row r holds window next + r, padding from avail on);
  // jend / tend = number and start of the end-aligned time index (jend = -1 until the stream is flushed)
  int64_t* state;
  int R, st;
  // a gated step (live_gate.hip): the rows are numbered by the selection and its own batch cursor, a device scalar
  // beside count (state stays LIVE_NSTATE scalars); s and cursor come together
  Selection s;
  int64_t* cursor;
};
// chunk [C][F][n] (n <= R - Wt) -> ring, total += n, avail from the new total; flush: the stream ends at the new
// total (n may be 0) and the end-aligned index, if there is one, becomes available.  -2 on bad arguments, as below.
int launch_ring_append(const LiveArgs& a, const float* chunk, int n, int flush, hipStream_t st);
int launch_gather_windows_ring(const LiveArgs& a, bf16_t* out, int64_t* lab_out, int lab_w, hipStream_t st);
// launch_window_probs' two forms; table [nrows][pitch], nrows >= Jcap * nf.  Without a selection pitch = K and next
// advances by the valid rows; with one pitch = K + 1 -- columns 0 .. K - 1 the probabilities, column K 1.0,
// "evaluated" -- and the cursor advances by one
int launch_live_probs(const LiveArgs& a, const float* src, int softmax, int T, const int* ncls, int K, float* table,
                      int64_t nrows, int pitch, int Jcap, hipStream_t st);
struct LiveMapArgs {
  const float* table;  // ring table [Jcap * nf][K]
  const int* fs;       // device copy of the fiber start table
  float* map;          // [K][nfc][ncol]: the cell columns q0 .. q0 + ncol - 1
  const float* wf;     // fiber weight bands [nf][mf], as MapArgs
  const float* wt;     // [ncol][mw]: weights of column q's time indices jlo[q] .. jlo[q] + jn[q] - 1
  const int64_t* jlo;  // [ncol]
  const int* jn;       // [ncol]
  int mf, mw, nf, K, F, Wf, cf, nfc, ncol, Jcap;
};
// h_*: host copies of fs / jlo / jn, checked (fs covers [0, F); 1 <= jn <= min(mw, Jcap); jlo >= 0)
int launch_live_map(const LiveMapArgs& a, int64_t nrows, const int* h_fs, const int64_t* h_jlo, const int* h_jn,
                    hipStream_t st);
// live_gate.hip: the activity gate of a growing recording.  Three rings of Jcap time indices, row
// (j mod Jcap) * nf + a like the probability table: the windows' powers, their noise floors (the causal running lower
// median of the last `history` powers of the fiber start, 0 before `warmup` of them exist) and their flags.
struct LiveGateArgs {
  LiveArgs live;       // live_select writes the selection live.s of the range and resets live.cursor
  float* power;        // [Jcap * nf]
  float* floor;        // [Jcap * nf]
  uint8_t* active;     // [Jcap * nf]
  int Jcap;
  int64_t n0, n1;      // the window numbers of the launch: whole time indices, n0 = j0 * nf, n1 = j1 * nf
};
// power ring rows of windows [n0, n1) read through the ring (window_power's accumulation: the same bits)
int launch_ring_window_power(const LiveGateArgs& a, hipStream_t st);
// floor ring rows of [n0, n1) from the power ring; history in 1 .. 1024, 1 <= warmup <= history,
// Jcap >= history - 1 + the time indices of the range
int launch_running_floor(const LiveGateArgs& a, int history, int warmup, hipStream_t st);
// flags of [n0, n1) (!(power < floor * ratio), as select_windows) into the active ring; their table rows
// [Jcap * nf][pitch] zeroed; sel / count as select_windows; then cursor = 0 and LIVE_NEXT = n1.  offs: workspace of
// select_blocks(n1 - n0) entries
int launch_live_select(const LiveGateArgs& a, float ratio, float* table, int64_t nrows, int pitch, int64_t* offs,
                       int64_t noffs, hipStream_t st);
// resample.hip: raw-rate recordings -- a FIR and decimation by D along time, one piece of a stream per launch
// (data/resample.py is the definition).  The piece's samples are carry_in's live columns followed by raw[skip ..];
// out gets the m outputs they complete, in ring_append's chunk layout, carry_out the new tail.
constexpr int DECIMATE_TILE = 128;        // outputs of one block
constexpr int DECIMATE_THREADS = 64;
constexpr int DECIMATE_MAX_FACTOR = 64;   // 1 <= D
constexpr int DECIMATE_MAX_TAPS = 1025;   // 1 <= L
enum { FIR_F32 = 0, FIR_I16 = 1 };        // the type of raw
struct FirArgs {
  const void* raw;        // [rows][pitch], n live columns: fp32 or int16
  const float* carry_in;  // [rows][L - 1], carry_len live columns: the raw samples from the next output's support on
  const float* taps;      // [L]
  float* out;             // [rows][m]
  float* carry_out;       // [rows][L - 1]: the tail after this piece, not carry_in
  int64_t rows, n, pitch, m;
  int carry_len, skip;    // skip: raw samples before the next output's support (D > L only; then carry_len = 0)
  int D, L;
};
// outputs that a piece of n raw samples completes
int64_t fir_output_count(int64_t carry_len, int64_t skip, int64_t n, int L, int D);
// -2 unless 1 <= D <= 64, 1 <= L <= 1025, 0 <= carry_len <= L - 1, skip >= 0, m = fir_output_count(..), every
// pointer the launch uses is non-null and carry_out is not carry_in
int launch_fir_decimate(const FirArgs& a, int itype, hipStream_t st);
// common_mode.hip: the common mode -- per channel and time sample one value over the fiber, the lower median or the
// mean -- subtracted from every fiber position (data/common_mode.py is the definition).  Columns are independent.
constexpr int COMMON_MODE_TILE = 32;      // consecutive time columns of one block
constexpr int COMMON_MODE_THREADS = 256;  // COMMON_MODE_TILE columns x 8 row groups
// 1 <= F: the selection's counters are 32-bit and would hold more; one block walks all F rows of its columns four
// times, and beyond this length a selection split along the fiber is the kernel to write
constexpr int COMMON_MODE_MAX_F = 1 << 20;
enum { COMMON_MODE_MEDIAN = 0, COMMON_MODE_MEAN = 1 };
struct CommonModeArgs {
  const float* x;  // [rows][F][pitch], n live columns
  float* out;      // [rows][F][out_pitch]; x itself (then out_pitch = pitch) or apart from it
  float* trace;    // [rows][n]: the value subtracted; may be null
  int64_t rows, F, n, pitch, out_pitch;
};
// -2 unless how is one of the two, rows >= 1, 1 <= F <= COMMON_MODE_MAX_F, 0 <= n < 2^31, n <= both pitches < 2^31,
// rows F < 2^32, the grid is below 2^31 blocks, x and out are non-null, out is x with x's pitch or does not overlap it, and trace overlaps
// neither; n = 0 launches nothing
int launch_common_mode(const CommonModeArgs& a, int how, hipStream_t st);
// synth.hip: on-device synthetic DAS samples (data/synthetic.py physical model, Philox noise)
constexpr int SYNTH_NPARAM = 9;  // per sample: distance, event, x0, t0, jitter[4], snr_db
struct SynthArgs {
  const float* params;  // [n][SYNTH_NPARAM]
  float* out;           // [n][C][H][W] fp32
  int C, H, W;
  int noise;            // 0: clean signal only
  uint64_t key;         // Philox key (the draw's noise seed)
  int64_t sample0;      // global index of sample 0 (Philox counter)
};
int launch_synth_das(const SynthArgs& a, int n, hipStream_t st);
int launch_philox_kat(const uint32_t* ctr, uint64_t key, uint32_t* out, int n, hipStream_t st);
int launch_tick(uint64_t* buf, uint64_t* q, int i, hipStream_t st);
int launch_adam_pack(const AdamArgs& a, const OptSeg* d_segs, int ns, int64_t nblocks, hipStream_t st);

}  // namespace mda
