// The one reader of a dispatch list: every family test lives here (dispatch_list.h).
#include "dispatch_list.h"

#include <cmath>
#include <cstring>

namespace nrdhip {

Family FamilyOf(const char* shader) {
    static const struct { const char* prefix; Family family; } kPrefixes[] = {{"REBLUR_", Family::REBLUR}, {"RELAX_", Family::RELAX}, {"SIGMA_", Family::SIGMA}, {"REFERENCE_", Family::REFERENCE}};
    for (const auto& p : kPrefixes)
        if (shader && !strncmp(shader, p.prefix, strlen(p.prefix)))
            return p.family;
    return Family::NONE;
}

template <typename T> static bool OffsetsIn(uint32_t constantsSize, size_t& origin, size_t& offset) {
    origin = offsetof(T, gRectOrigin), offset = offsetof(T, gRectOffset);
    return constantsSize >= sizeof(T);
}
bool RectOriginOffsets(const char* shader, uint32_t size, size_t& origin, size_t& offset) {
    const Family f = FamilyOf(shader);
    return f == Family::REBLUR ? OffsetsIn<nrdc::ReblurConstants>(size, origin, offset) : f == Family::RELAX ? OffsetsIn<nrdc::RelaxConstants>(size, origin, offset) : f == Family::SIGMA && OffsetsIn<nrdc::SigmaConstants>(size, origin, offset);
}

// If this pass holds the first block of `family` (REBLUR, RELAX, SIGMA) in the list -- a null or short block is skipped, the next one of the family taken -- remembers it in
// `slot`; returns it if it also is the first block overall, after taking the frame from it (the fields the three shared blocks have in common), else null
template <typename T> static const T* TakeBlock(ListScan& s, const T*& slot, Family family, const char* shader, const nrd::DispatchDesc& d) {
    const T* c = slot ? nullptr : ConstantsAs<T>(family, shader, d.constantBufferData, d.constantBufferDataSize);
    if (!c)
        return nullptr;
    slot = c;
    if (s.firstWithOrigin == Family::NONE)
        s.firstWithOrigin = family, s.originX = (int)c->gRectOrigin.x, s.originY = (int)c->gRectOrigin.y;
    if (s.first != Family::NONE)
        return nullptr;
    s.first = family;
    s.rectW = (int)c->gRectSize.x, s.rectH = (int)c->gRectSize.y;
    s.viewZScale = c->gViewZScale, s.denoisingRange = c->gDenoisingRange;
    s.frameIndex = c->gFrameIndex;
    return c;
}

ListScan ScanDispatchList(const nrd::InstanceDesc& idesc, const nrd::DispatchDesc* descs, uint32_t num, uint8_t* bindsNormalRoughness) {
    ListScan s;
    s.bindsNormalRoughness = bindsNormalRoughness;
    for (uint32_t i = 0; i < num; i++) {
        const nrd::DispatchDesc& d = descs[i];
        const char* shader = ShaderOf(idesc, d);
        const bool knownPipeline = d.pipelineIndex < idesc.pipelinesNum, reblurPass = FamilyOf(shader) == Family::REBLUR;
        bool normalRoughness = false;
        for (uint32_t r = 0; r < d.resourcesNum; r++) {
            const nrd::ResourceDesc& res = d.resources[r];
            const size_t t = (size_t)res.type;
            if (t >= (size_t)nrd::ResourceType::TRANSIENT_POOL)
                continue; // a pool plane, not a user slot
            if (!s.read[t] && !s.written[t])
                s.slots[s.slotsNum++] = (uint8_t)t;
            (res.descriptorType == nrd::DescriptorType::TEXTURE ? s.read : s.written)[t] = true;
            s.named[t] = s.named[t] || knownPipeline;
            s.namedOutsideReblur[t] = s.namedOutsideReblur[t] || (knownPipeline && !reblurPass);
            normalRoughness = normalRoughness || res.type == nrd::ResourceType::IN_NORMAL_ROUGHNESS;
        }
        if (bindsNormalRoughness)
            bindsNormalRoughness[i] = normalRoughness;

        if (const auto* c = TakeBlock(s, s.reblur, Family::REBLUR, shader, d))
            s.diffCell = c->gDiffCheckerboard, s.specCell = c->gSpecCheckerboard;
        if (const auto* c = TakeBlock(s, s.relax, Family::RELAX, shader, d))
            s.diffCell = c->gDiffCheckerboard, s.specCell = c->gSpecCheckerboard;
        TakeBlock(s, s.sigma, Family::SIGMA, shader, d);
        if (const auto* c = s.first != Family::NONE || strcmp(shader, "REFERENCE_Copy.cs") ? nullptr : ConstantsAs<nrdc::ReferenceCopyConstants>(Family::REFERENCE, shader, d.constantBufferData, d.constantBufferDataSize)) {
            // REFERENCE has no shared block, and its copy pass carries the rect only as its inverse: 1 / ( 1 / n ) rounds back to n for every 16-bit n. No origin (its kernels
            // address IN_SIGNAL at the pixel itself), no range
            s.first = Family::REFERENCE;
            s.rectW = (int)std::lround(1.0f / c->gRectSizeInv.x), s.rectH = (int)std::lround(1.0f / c->gRectSizeInv.y);
        }
    }
    return s;
}

} // namespace nrdhip
