// What every writer of the stem's input shares: the batch gather (misc.hip), the noisy batch gather (augment.hip)
// and the window gathers (window_batch.h gather_windows_body).  One copy of
//
//   * the schedule row of the step: idx advanced by *cursor mod nrows rows of B;
//   * the ZeroRanges clear a training step's gather carries;
//   * the label gather of block 0;
//   * the batch gathers' limits (gather_args_ok), the ones both launchers refuse with -2;
//   * the stem pixel: 8 channels from a column with tap packing, or C real channels padded to 8.
//
// What differs stays in the kernels: the thread mapping (one pixel per thread in misc.hip and the window gathers, one
// vertical quad per thread in augment.hip, whose store_packed reads its taps from a 16-row register array), the
// noise, and the window gathers' numbering and sources.
#pragma once
#include "kernels.h"

namespace mda {

// batch-index schedule (cursor set): this step's indices are row (*cursor mod nrows) of a [nrows][B] table; the
// optimizer's step-counter kernel advances the cursor at the end of the step, so no host copy of the indices
// precedes each replay
DEV const int64_t* schedule_row(const GatherArgs& a) {
  return a.cursor ? a.idx + (*a.cursor % a.nrows) * (int64_t)a.B : a.idx;
}

// the arena's zeroed regions (BN statistic replicas, backward workspaces) cleared by the same launch at the start of
// a training step -- one dependent launch instead of a gather plus a fill per dtype; every block of 256 takes part
DEV void clear_ranges(const ZeroRanges& zero) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, nt = (int64_t)gridDim.x * 256;
  for (int r = 0; r < zero.n; ++r)
    for (int64_t i = t; i < zero.n16[r]; i += nt) zero.p[r][i] = make_uint4(0, 0, 0, 0);
}

// block 0 gathers the labels of the batch rows (idx: the step's row of the schedule)
DEV void gather_labels(const GatherArgs& a, const int64_t* __restrict__ idx) {
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < a.B * a.lab_w; i += 256) {
      const int b = i / a.lab_w, k = i - b * a.lab_w;
      a.lab_out[i] = a.lab[idx[b] * a.lab_w + k];
    }
}

// What both batch gathers require: every pointer, a batch and an image, at most 8 stored channels, tap packing only
// of a single channel, 32-bit pixel indices, and a row count with a cursor.  (No limit on off here: the clean kernel
// bounds-checks every tap row.)
inline bool gather_args_ok(const GatherArgs& a) {
  return a.X && a.idx && a.lab && a.out && a.lab_out && a.B >= 1 && a.Cin >= 1 && a.H >= 1 && a.W >= 1 &&
         a.Cin <= 8 && a.taps >= 0 && a.taps <= 8 && !(a.taps > 0 && a.Cin != 1) &&
         (int64_t)a.B * a.H * a.W < (1ll << 31) && !(a.cursor && a.nrows <= 0);
}

// Vertical tap packing of a single-channel stem: channel j of the pixel in row h holds row h - off + j of its column
// (zero outside the rows [0, H) and for j >= taps), so a KHxKW stem over 1 channel runs as a 1xKW conv over KH real
// channels (engine/core.py stem_pack_geom) instead of wasting 7/8 of its K on zero padding channels.
// x: the pixel's own element; pitch: elements between the column's rows.
DEV void stem_taps(const float* __restrict__ x, int64_t pitch, int h, int H, int taps, int off, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int hh = h - off + j;
    v[j] = (j < taps && hh >= 0 && hh < H) ? x[(hh - h) * pitch] : 0.f;
  }
}

// C real channels zero-padded to 8.  x: the pixel's element of channel 0; plane: elements between channels.
DEV void stem_channels(const float* __restrict__ x, int64_t plane, int C, float (&v)[8]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) v[c] = c < C ? x[c * plane] : 0.f;
}

}  // namespace mda
