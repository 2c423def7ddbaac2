// Weight-gradient tile configurations: the one list of what a config id means, and everything derived from it --
// the host shape lookup (wgrad_shape), the dispatch from an id to its block type (wgrad_dispatch) and the two
// kernel entry points every family shares.  The ids are stored in engine/tuned_cfgs.json and in the profiles, so
// they never change.  ops/functional.py WGRAD_CONFIGS is the Python copy (the package lowers programs where the
// extension is absent); tests/test_wgrad_configs.py compares the two row by row, and the argument checks of
// wgrad_ntiles (conv.hip) with their Python mirror.
#pragma once
#include "conv_tile.h"

namespace mda {

enum WgFamily { WG_SMALL, WG_WHOLE, WG_PATCH, WG_BIG, WG_LEAN, WG_LEANBIG };
struct WgradShape { int cfg, family, TN, TK, MCH, CB, W8, R; };  // im2col: CB = W8 = R = 0; patch: TK = MCH = 0

// A block type per family: its static run(a, tile, split, z) calls the family's block function and is defined
// beside it (WgTile, WgPatch, WgBig: conv.hip; WgLean: wgrad_lean.hip; WgPatch's run is the block function).
// The type is the kernels' template argument, so the family and the tile sizes show in every kernel's symbol name.
// im2col tile of TN output channels x TK reduction columns, MCH pixels per LDS chunk (wgrad_block)
template <int TN, int TK, int MCH>
struct WgTile {
  static constexpr WgradShape shape(int cfg, int fam) { return {cfg, fam, TN, TK, MCH, 0, 0, 0}; }
  static DEV void run(const WgradArgs& a, int tile, int split, int z);
};
// 3x3 / stride 1 patch tile: TN output channels x 9 taps x CB input channels, rows of at most W8 padded output
// pixels, strips of R output rows
template <int TN, int CB, int W8, int R>
struct WgPatch {
  static constexpr WgradShape shape(int cfg, int fam) { return {cfg, fam, TN, 0, 0, CB, W8, R}; }
  static DEV void run(const WgradArgs& a, int tile, int split, int z);
};
// large tile on the 32x32x16 MFMA, 64-pixel chunks (wgrad_big_block)
template <int TN, int TK>
struct WgBig {
  static constexpr WgradShape shape(int cfg, int fam) { return {cfg, fam, TN, TK, 64, 0, 0, 0}; }
  static DEV void run(const WgradArgs& a, int tile, int split, int z);
};
// lean-staging im2col tile; BIG: under the large tiles' 32x32x16 MFMA compute (wgrad_lean_block)
template <int TN, int TK, int MCH, bool BIG>
struct WgLean {
  static constexpr WgradShape shape(int cfg, int fam) { return {cfg, fam, TN, TK, MCH, 0, 0, 0}; }
  static DEV void run(const WgradArgs& a, int tile, int split, int z);
};

// X(id, family, block type): every config exactly once, split by the translation unit that holds the block.
// Configs 8-11 cover the whole reduction of a small-Cout layer in one tile: dy is read once per pixel and the
// im2col taps of neighbouring pixels re-hit L1, instead of every 32-wide K tile re-reading dy and its im2col slice
// from L2 (Model A's 16-channel 33x83 layers moved ~50 MB of L2 traffic each with TK = 32).  The small and
// whole-reduction K tiles must cover Kpad exactly; the last K tile of the big and lean families may be partial.
#define WGRAD_CONFIGS_CONV(X)                                                                                  \
  X(0, WG_SMALL, WgTile<16, 32, 128>) X(1, WG_SMALL, WgTile<32, 32, 128>) X(2, WG_SMALL, WgTile<32, 64, 64>)   \
  X(3, WG_SMALL, WgTile<64, 64, 64>) X(4, WG_SMALL, WgTile<16, 64, 128>) X(5, WG_SMALL, WgTile<16, 32, 256>)   \
  X(6, WG_SMALL, WgTile<32, 32, 256>) X(7, WG_SMALL, WgTile<64, 32, 64>)                                       \
  X(8, WG_WHOLE, WgTile<16, 192, 64>) X(9, WG_WHOLE, WgTile<16, 128, 64>) X(10, WG_WHOLE, WgTile<32, 192, 64>) \
  X(11, WG_WHOLE, WgTile<32, 320, 32>)                                                                         \
  X(12, WG_PATCH, WgPatch<16, 16, 88, 4>) X(13, WG_PATCH, WgPatch<32, 16, 88, 4>)                              \
  X(14, WG_PATCH, WgPatch<32, 32, 48, 4>) X(15, WG_PATCH, WgPatch<64, 32, 24, 4>)                              \
  X(16, WG_PATCH, WgPatch<32, 32, 128, 2>) X(17, WG_PATCH, WgPatch<64, 32, 128, 2>)                            \
  X(18, WG_PATCH, WgPatch<64, 16, 128, 2>) X(19, WG_PATCH, WgPatch<32, 16, 128, 2>)                            \
  X(32, WG_BIG, WgBig<64, 64>) X(33, WG_BIG, WgBig<64, 128>) X(34, WG_BIG, WgBig<128, 64>)                     \
  X(35, WG_BIG, WgBig<128, 128>)
// 44-47: the big config 12 below on lean staging (same tile, same M split)
#define WGRAD_CONFIGS_LEAN(X)                                                                                  \
  X(36, WG_LEAN, WgLean<16, 64, 256, false>) X(37, WG_LEAN, WgLean<16, 144, 128, false>)                       \
  X(38, WG_LEAN, WgLean<32, 64, 256, false>) X(39, WG_LEAN, WgLean<32, 144, 128, false>)                       \
  X(40, WG_LEAN, WgLean<64, 64, 128, false>) X(41, WG_LEAN, WgLean<64, 128, 128, false>)                       \
  X(42, WG_LEAN, WgLean<128, 64, 128, false>) X(43, WG_LEAN, WgLean<128, 128, 64, false>)                      \
  X(44, WG_LEANBIG, WgLean<64, 64, 64, true>) X(45, WG_LEANBIG, WgLean<64, 128, 64, true>)                     \
  X(46, WG_LEANBIG, WgLean<128, 64, 64, true>) X(47, WG_LEANBIG, WgLean<128, 128, 64, true>)
#define WGRAD_CONFIGS(X) WGRAD_CONFIGS_CONV(X) WGRAD_CONFIGS_LEAN(X)

#define WGRAD_SHAPE_ROW(ID, FAM, ...) __VA_ARGS__::shape(ID, FAM),
constexpr WgradShape WGRAD_SHAPES[] = {WGRAD_CONFIGS(WGRAD_SHAPE_ROW)};
#undef WGRAD_SHAPE_ROW

inline bool wgrad_shape(int cfg, WgradShape& s) {
  for (const WgradShape& r : WGRAD_SHAPES)
    if (r.cfg == cfg) { s = r; return true; }
  return false;
}

// f(Block{}) for the block type of cfg; -1: no such config
template <class F>
int wgrad_dispatch(int cfg, F&& f) {
#define WGRAD_CASE(ID, FAM, ...) case ID: return f(__VA_ARGS__{});
  switch (cfg) {
    WGRAD_CONFIGS(WGRAD_CASE)
    default: return -1;
  }
#undef WGRAD_CASE
}

// wgrad_lean_block packs two words per 16-byte staging unit with a channel in the low LEAN_CH_BITS -- the x
// unit's offset within its segment, as encode_kg gives it, or the dy unit's channel n0 + 8 * cg, which runs up to
// the padded end of the last row tile -- below the unit's LDS destination (element offset, LEAN_DST_BITS).
// wgrad_ntiles refuses a conv whose dy channels do not fit; the block asserts that its destinations do.
constexpr int LEAN_CH_BITS = KG_CH_BITS, LEAN_DST_BITS = 31 - LEAN_CH_BITS;

template <class Block>
__global__ __launch_bounds__(256) void wgrad_kernel(WgradArgs a) {
  Block::run(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Horizontally batched weight gradients: every conv of a backward pass that uses this tile config, in
// ONE launch.  The weight gradient of a layer only needs its dy and forward input, both resident until
// the step ends, so all of them are deferred to the end of the backward pass; the ~40 (Model A) / ~90
// (Model C) small launches become <= 8 large ones that fill the 256 CUs (the deep, small-M layers run
// side by side instead of one after another).  Block -> job by binary search over the jobs' first blocks.
// The batched launches walk nvb virtual blocks with a grid of at most nvb hardware blocks: a side stream's
// batch may run on a capped, persistent grid (launch_wgrad_batched ``cap``), so that it never fills every CU
// slot while the critical data-gradient chain needs blocks (tools/kernel_phases.py: chain kernels waited up
// to 16 us for their blocks to start beside an uncapped batch).
// (The walk is open text in the one kernel: as a function template taking the body it cost the batched kernels
// up to 2 VGPRs and 4 SGPRs, and one of them an SGPR spill.)
template <class Block>
__global__ __launch_bounds__(256) void wgrad_batched_kernel(const WgradJob* __restrict__ jobs, int nj, int64_t nvb) {
  for (int64_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
    int lo = 0, hi = nj - 1;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (jobs[mid].block0 <= vb) lo = mid; else hi = mid - 1; }
    const WgradJob& J = jobs[lo];
    const int local = (int)(vb - J.block0);
    const int per_z = J.ntiles * J.a.splits;
    const int z = local / per_z, r = local - z * per_z;
    Block::run(J.a, r % J.ntiles, r / J.ntiles, z);
    __syncthreads();  // the next virtual block re-stages the LDS tiles
  }
}

// the lean blocks' kernels are instantiated in wgrad_lean.hip; conv.hip, which holds the launchers, only calls them
// (EXT = extern here, empty there)
#define WGRAD_KERNELS(EXT, ...)                                      \
  EXT template __global__ void wgrad_kernel<__VA_ARGS__>(WgradArgs); \
  EXT template __global__ void wgrad_batched_kernel<__VA_ARGS__>(const WgradJob*, int, int64_t);
#define WGRAD_EXTERN_KERNELS(ID, FAM, ...) WGRAD_KERNELS(extern, __VA_ARGS__)
WGRAD_CONFIGS_LEAN(WGRAD_EXTERN_KERNELS)
#undef WGRAD_EXTERN_KERNELS

}  // namespace mda
