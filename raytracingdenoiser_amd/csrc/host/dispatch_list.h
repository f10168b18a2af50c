// The one reader of a dispatch list (nrd::GetComputeDispatches): which family a pass belongs to, its constant block as a typed, size-checked view, and one scan of a whole
// list for what the HIP executor (csrc/hip/executor*.hip) asks of it. Host-only, like the sharding planner: plain C++, no HIP header (tests/cpp/dispatch_list_host.cpp).
#pragma once

#include "NRD.h"

#include "../common/pass_constants.h"

#include <cstddef>
#include <cstdint>

namespace nrdhip {

enum class Family : uint8_t { NONE, REBLUR, RELAX, SIGMA, REFERENCE };

// by the prefix of the shader file name ("REBLUR_", "RELAX_", "SIGMA_", "REFERENCE_"); NONE: Clear_*, null
Family FamilyOf(const char* shaderFileName);

// the shader file name of a dispatch; "" (family NONE) for a pipeline index the instance does not have
inline const char* ShaderOf(const nrd::InstanceDesc& idesc, const nrd::DispatchDesc& d) { return d.pipelineIndex < idesc.pipelinesNum ? idesc.pipelines[d.pipelineIndex].shaderFileName : ""; }

// "the constants of this pass as T, or null if the family or the size does not fit": the only way a block is cast to a struct. T = the shared block of `family` (or one that
// begins with it). The block is read in place: it has to be 4-byte aligned, as the blocks of nrd::GetComputeDispatches are.
template <typename T> const T* ConstantsAs(Family family, const char* shader, const void* constants, uint32_t constantsSize) {
    return constants && constantsSize >= sizeof(T) && FamilyOf(shader) == family ? (const T*)constants : nullptr;
}

// byte offsets of gRectOrigin (uint2) and gRectOffset (float2) in the shared block of the pass's family; false = it has none (REFERENCE, NONE) or the block is too short
bool RectOriginOffsets(const char* shader, uint32_t constantsSize, size_t& origin, size_t& offset);

constexpr size_t kUserSlots = (size_t)nrd::ResourceType::MAX_NUM;

// What one walk over a whole list finds. Fixed-size: scanning allocates nothing.
struct ListScan {
    // the first block of each family in list order (null: the list has none that fits); of REFERENCE only the rect is kept, below
    const nrdc::ReblurConstants* reblur = nullptr;
    const nrdc::RelaxConstants* relax = nullptr;
    const nrdc::SigmaConstants* sigma = nullptr;
    // which family's block came first overall, and which first among the families that carry a rect origin and reproject (REBLUR, RELAX, SIGMA)
    Family first = Family::NONE, firstWithOrigin = Family::NONE;
    int originX = 0, originY = 0; // gRectOrigin of the firstWithOrigin block
    // the frame as the first block overall states it (every block of a list carries the same CommonSettings); the defaults stand for a list without any block
    int rectW = 0, rectH = 0;
    float viewZScale = 1.0f, denoisingRange = 0.0f;
    uint32_t frameIndex = 0, diffCell = 2, specCell = 2; // cells: gDiffCheckerboard / gSpecCheckerboard, 2 = no checkerboard (REBLUR and RELAX blocks only)
    // per user slot: bound by any dispatch / by one that is not a REBLUR pass (both: of a pipeline the instance has, as the input audit asks) / as TEXTURE / as STORAGE_TEXTURE
    bool named[kUserSlots] = {}, namedOutsideReblur[kUserSlots] = {}, read[kUserSlots] = {}, written[kUserSlots] = {};
    uint8_t slots[kUserSlots] = {}; // the slots some dispatch binds, in the order the list first binds them
    uint32_t slotsNum = 0;
    const uint8_t* bindsNormalRoughness = nullptr; // per dispatch, != 0: it binds IN_NORMAL_ROUGHNESS. The caller's array (num bytes) if it handed one in, else null
};

ListScan ScanDispatchList(const nrd::InstanceDesc& idesc, const nrd::DispatchDesc* descs, uint32_t num, uint8_t* bindsNormalRoughness = nullptr);

} // namespace nrdhip
