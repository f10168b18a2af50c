// Host-only: when ONE linear texel index, formed in fp32, addresses every plane a "full rect" tap of the REBLUR spatial passes reads
// (csrc/hip/kernels_reblur_spatial.hip FetchTapGuidesFullRect, FR == 3). No HIP in here: tests/test_div_table.py builds it with a host compiler alone.
#pragma once

#include <cstdint>

namespace nrdhip {

// The tap's clamped coordinate is an integer-valued float pair (x, y); the kernel forms index = fma(y, pitchInTexels, x), converts it once and scales it by each
// plane's texel size. That is the byte offset y * pitch + x * bytesPerTexel of every plane iff
//   * all planes have the SAME pitch in texels: pitchBytes[i] == pitchInTexels * texelBytes[i] (plane 0 defines pitchInTexels; its pitch must be a whole number of texels), and
//   * the fma is exact: every index is an integer below 2^24, the largest one being (h - 1) * pitchInTexels + (w - 1) < pitchInTexels * h.
// Pool planes pad their rows to 256 bytes per plane (executor.hip PlanPool), so planes of different texel sizes agree only at some widths (a multiple of 64 texels for 4-byte
// planes); a user plane may carry any pitch. Where this returns false the launcher takes the variants that multiply per plane.
inline bool TapIndexAddressesAllPlanes(int32_t w, int32_t h, const uint32_t* pitchBytes, const uint32_t* texelBytes, uint32_t planesNum) {
    if (w <= 0 || h <= 0 || planesNum == 0 || texelBytes[0] == 0 || pitchBytes[0] % texelBytes[0] != 0)
        return false;
    const uint64_t pitchInTexels = pitchBytes[0] / texelBytes[0];
    if (pitchInTexels < (uint64_t)w || pitchInTexels * (uint64_t)h > (1ull << 24))
        return false;
    for (uint32_t i = 1; i < planesNum; i++)
        if ((uint64_t)pitchBytes[i] != pitchInTexels * texelBytes[i])
            return false;
    return true;
}

} // namespace nrdhip
