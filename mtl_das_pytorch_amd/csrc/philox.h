// Counter-based Philox-4x32-10 (Salmon et al., SC'11) and the uniform it feeds, shared by the on-device
// synthetic generator (synth.hip) and the SNR noise of the batch gather (augment.hip).
#pragma once
#include "common.h"

namespace mda {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

DEV uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(PHILOX_M0, ctr.x), lo0 = PHILOX_M0 * ctr.x;
    const uint32_t hi1 = __umulhi(PHILOX_M1, ctr.z), lo1 = PHILOX_M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += PHILOX_W0;
    key.y += PHILOX_W1;
  }
  return ctr;
}

// uniform in (0, 1]: never 0, so log() is finite
DEV float u01(uint32_t x) { return ((float)(x >> 8) + 1.f) * (1.f / 16777216.f); }

}  // namespace mda
