// HIP executor: owns the pool planes in HBM and turns an nrd::DispatchDesc list into kernel launches on one stream.
// Plays the role of the reference integration layer (reference Integration/NRDIntegration.hpp:292-454 pool creation,
// :516-623 Denoise, :625-803 Dispatch) -- without descriptor sets, barriers or a constant ring buffer: planes are raw
// pointers, constants travel as kernel arguments, ordering is stream order. This unit: creation, destruction, binding, pool queries, ExecuteRange.
#include "executor.h"

#include "nrdmath.h" // NRD_NORMAL_ENCODING

#include "../host/halo_plan.h" // the host-only sharding planner: GuideReachRows, OwnedRowRanges

namespace nrd { // csrc/host/instance.h (the host side of this library; not part of the public API)
uint16_t TransientAliasOf(const Instance& instance, Identifier identifier, uint16_t indexInPool);
}

#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace nrdhip;

static_assert((uint32_t)nrd::Format::RGBA8_UNORM == FORMAT_RGBA8_UNORM && (uint32_t)nrd::Format::R16_UNORM == FORMAT_R16_UNORM && (uint32_t)nrd::Format::RGBA16_SNORM == FORMAT_RGBA16_SNORM && (uint32_t)nrd::Format::RGBA16_SFLOAT == FORMAT_RGBA16_SFLOAT,
    "passes.h format constants");

uint32_t nrdhip::BytesPerTexel(nrd::Format f) {
    using F = nrd::Format;
    switch (f) {
        case F::R8_UNORM: case F::R8_SNORM: case F::R8_UINT: case F::R8_SINT:
            return 1;
        case F::RG8_UNORM: case F::RG8_SNORM: case F::RG8_UINT: case F::RG8_SINT:
        case F::R16_UNORM: case F::R16_SNORM: case F::R16_UINT: case F::R16_SINT: case F::R16_SFLOAT:
            return 2;
        case F::RGBA8_UNORM: case F::RGBA8_SNORM: case F::RGBA8_UINT: case F::RGBA8_SINT: case F::RGBA8_SRGB:
        case F::RG16_UNORM: case F::RG16_SNORM: case F::RG16_UINT: case F::RG16_SINT: case F::RG16_SFLOAT:
        case F::R32_UINT: case F::R32_SINT: case F::R32_SFLOAT:
        case F::R10_G10_B10_A2_UNORM: case F::R10_G10_B10_A2_UINT: case F::R11_G11_B10_UFLOAT: case F::R9_G9_B9_E5_UFLOAT:
            return 4;
        case F::RGBA16_UNORM: case F::RGBA16_SNORM: case F::RGBA16_UINT: case F::RGBA16_SINT: case F::RGBA16_SFLOAT:
        case F::RG32_UINT: case F::RG32_SINT: case F::RG32_SFLOAT:
            return 8;
        case F::RGB32_UINT: case F::RGB32_SINT: case F::RGB32_SFLOAT:
            return 12;
        case F::RGBA32_UINT: case F::RGBA32_SINT: case F::RGBA32_SFLOAT:
            return 16;
        default:
            return 0;
    }
}

nrd::Format nrdhip::ExpectedUserFormat(nrd::ResourceType t, bool translucentShadow) {
    using R = nrd::ResourceType;
    using F = nrd::Format;
    switch (t) {
        case R::IN_MV: return F::RGBA16_SFLOAT;
        case R::IN_NORMAL_ROUGHNESS: // the format of the library's normal encoding (nrdmath.h NRD_NORMAL_ENCODING, nrd::GetLibraryDesc().normalEncoding; reblur_device.h NrRaw)
            return NRD_NORMAL_ENCODING == 0 ? F::RGBA8_UNORM : NRD_NORMAL_ENCODING == 1 ? F::RGBA8_SNORM : NRD_NORMAL_ENCODING == 2 ? F::R10_G10_B10_A2_UNORM : NRD_NORMAL_ENCODING == 3 ? F::RGBA16_UNORM : F::RGBA16_SNORM;
        case R::IN_VIEWZ: return F::R32_SFLOAT;
        case R::IN_DIFF_CONFIDENCE: case R::IN_SPEC_CONFIDENCE: case R::IN_DISOCCLUSION_THRESHOLD_MIX: return F::R8_UNORM;
        case R::IN_DIFF_RADIANCE_HITDIST: case R::IN_SPEC_RADIANCE_HITDIST: return F::RGBA16_SFLOAT;
        case R::OUT_DIFF_RADIANCE_HITDIST: case R::OUT_SPEC_RADIANCE_HITDIST: return F::RGBA16_SFLOAT;
        case R::IN_DIFF_SH0: case R::IN_DIFF_SH1: case R::IN_SPEC_SH0: case R::IN_SPEC_SH1: return F::RGBA16_SFLOAT;
        case R::OUT_DIFF_SH0: case R::OUT_DIFF_SH1: case R::OUT_SPEC_SH0: case R::OUT_SPEC_SH1: return F::RGBA16_SFLOAT;
        case R::IN_DIFF_DIRECTION_HITDIST: case R::OUT_DIFF_DIRECTION_HITDIST: return F::RGBA16_SNORM; // REBLUR_DIFFUSE_DIRECTIONAL_OCCLUSION
        case R::IN_DIFF_HITDIST: case R::IN_SPEC_HITDIST: case R::OUT_DIFF_HITDIST: case R::OUT_SPEC_HITDIST: return F::R16_UNORM; // REBLUR occlusion family
        case R::IN_PENUMBRA: return F::R16_SFLOAT;
        case R::IN_TRANSLUCENCY: case R::IN_BASECOLOR_METALNESS: return F::RGBA8_UNORM;
        case R::OUT_SHADOW_TRANSLUCENCY: return translucentShadow ? F::RGBA8_UNORM : F::R8_UNORM;
        case R::IN_SIGNAL: case R::OUT_SIGNAL: return F::RGBA32_SFLOAT;
        case R::OUT_VALIDATION: return F::RGBA8_UNORM;
        default: return F::MAX_NUM;
    }
}

Ensured nrdhip::EnsurePlane(Plane& plane, const Plane& geometry) {
    if (plane.ptr && plane.w == geometry.w && plane.h == geometry.h && plane.pitch == geometry.pitch)
        return Ensured::PRESENT;
    if (plane.ptr)
        (void)hipFree(plane.ptr);
    plane = geometry;
    plane.ptr = nullptr;
    if (hipMalloc((void**)&plane.ptr, (size_t)plane.pitch * (size_t)plane.h) == hipSuccess)
        return Ensured::REALLOCATED;
    plane = Plane{};
    return Ensured::FAILED;
}

// layers > 1 (nrdHipCreateExecutorLayered): every plane is followed by its layers 1 .. layers - 1, each `strides[i]` -- the plane's 256-byte aligned size -- behind the last
static bool PlanPool(const nrd::TextureDesc* descs, uint32_t num, uint16_t w, uint16_t h, uint32_t layers, std::vector<Plane>& planes, std::vector<nrd::Format>& formats,
    std::vector<uint64_t>& strides, uint64_t& offset) {
    planes.resize(num);
    formats.resize(num);
    strides.resize(num);
    for (uint32_t i = 0; i < num; i++) {
        uint32_t bpt = BytesPerTexel(descs[i].format);
        if (!bpt)
            return false;
        int pw = (w + descs[i].downsampleFactor - 1) / descs[i].downsampleFactor;
        int ph = (h + descs[i].downsampleFactor - 1) / descs[i].downsampleFactor;
        uint32_t pitch = ((uint32_t)pw * bpt + 255u) & ~255u;
        planes[i] = Plane{(uint8_t*)(uintptr_t)offset, pitch, pw, ph}; // (ptr: patched to a real pointer once the arena exists)
        formats[i] = descs[i].format;
        strides[i] = ((uint64_t)pitch * (uint64_t)ph + 255u) & ~(uint64_t)255u;
        offset += strides[i] * layers;
    }
    return true;
}

static bool PlanPools(const nrd::InstanceDesc& desc, uint16_t w, uint16_t h, NrdHipExecutor& e) {
    uint64_t offset = 0;
    bool ok = PlanPool(desc.permanentPool, desc.permanentPoolSize, w, h, e.layersNum, e.permanent, e.permanentFormat, e.permanentStride, offset);
    e.permanentBytes = offset;
    ok = ok && PlanPool(desc.transientPool, desc.transientPoolSize, w, h, e.layersNum, e.transient, e.transientFormat, e.transientStride, offset);
    e.transientBytes = offset - e.permanentBytes;
    return ok;
}

static uint32_t CreateExecutorImpl(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, uint32_t layersNum, void* hipStream, void* userArena, uint64_t userArenaSize,
    NrdHipExecutor** executor) {
    if (!instance || !executor || !resourceWidth || !resourceHeight || !layersNum || layersNum > NRD_HIP_MAX_SHADOW_LIGHTS)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    *executor = nullptr;
    if (layersNum > 1) { // the layers share every constant, which only SIGMA's passes allow (include/NRDHip.h "layered executor")
        const nrd::InstanceDesc& desc = nrd::GetInstanceDesc(*(nrd::Instance*)instance);
        for (uint32_t p = 0; p < desc.pipelinesNum; p++)
            if (strncmp(desc.pipelines[p].shaderFileName, "SIGMA_", 6) != 0 && strncmp(desc.pipelines[p].shaderFileName, "Clear_", 6) != 0) {
                fprintf(stderr, "nrdHipCreateExecutorLayered: %u layers need an instance of SIGMA denoisers only; this one holds the pass %s\n", layersNum, desc.pipelines[p].shaderFileName);
                return (uint32_t)nrd::Result::UNSUPPORTED;
            }
    }
    if (!PlaneAddressable(((uint64_t)resourceWidth * 16u + 255u) & ~255ull, resourceHeight)) {
        fprintf(stderr, "nrdHipCreateExecutor: %u x %u is beyond the 4 GiB a plane of 16-byte texels may span (32-bit byte offsets)\n", resourceWidth, resourceHeight);
        return (uint32_t)nrd::Result::UNSUPPORTED;
    }

    int deviceCount = 0;
    if (hipGetDeviceCount(&deviceCount) != hipSuccess || deviceCount == 0) {
        fprintf(stderr, "nrdHipCreateExecutor: no HIP device available -- the NRD HIP back-end has no CPU fallback\n");
        return (uint32_t)nrd::Result::FAILURE;
    }

    NrdHipExecutor* e = new NrdHipExecutor;
    e->instance = (nrd::Instance*)instance;
    e->stream = (hipStream_t)hipStream;
    e->width = resourceWidth;
    e->height = resourceHeight;
    e->layersNum = layersNum;

    const nrd::InstanceDesc& desc = nrd::GetInstanceDesc(*e->instance);

    const bool ok = PlanPools(desc, resourceWidth, resourceHeight, *e);
    const uint64_t offset = e->permanentBytes + e->transientBytes;
    auto fail = [&](nrd::Result r) { // (destruction releases whatever is owned so far)
        nrdHipDestroyExecutor(e);
        return (uint32_t)r;
    };
    if (!ok)
        return fail(nrd::Result::UNSUPPORTED);

    if (offset) {
        e->ownsArena = !userArena;
        if (userArena && (userArenaSize < offset || ((uintptr_t)userArena & 255u) != 0))
            return fail(nrd::Result::INVALID_ARGUMENT);
        if (userArena)
            e->arena = (uint8_t*)userArena;
        else if (hipMalloc((void**)&e->arena, offset) != hipSuccess) {
            e->arena = nullptr;
            return fail(nrd::Result::FAILURE);
        }
        (void)hipMemsetAsync(e->arena, 0, offset, e->stream);
        for (Plane& p : e->permanent)
            p.ptr = e->arena + (uintptr_t)p.ptr;
        for (Plane& p : e->transient)
            p.ptr = e->arena + (uintptr_t)p.ptr;
    }

    // per-tile flags of the passes that run as a fast kernel plus a fallback kernel for the tiles the fast one declines (tiny: one byte per 32x8 pixels)
    const int tilesW = (resourceWidth + 31) / 32;
    const uint32_t tilesPitch = ((uint32_t)tilesW + (uint32_t)TILE_FLAG_GROUP - 1u) / (uint32_t)TILE_FLAG_GROUP * (uint32_t)TILE_FLAG_GROUP; // the fallback kernels read whole groups of flags (planes.h AnyTileFlagUniform)
    if (EnsurePlane(e->tileFlags, Plane{nullptr, tilesPitch, tilesW, (resourceHeight + 7) / 8}) == Ensured::FAILED)
        return fail(nrd::Result::FAILURE);
    (void)hipMemsetAsync(e->tileFlags.ptr, 0, (size_t)e->tileFlags.pitch * (size_t)e->tileFlags.h, e->stream);

    // pipeline index -> launcher
    e->launchers.assign(desc.pipelinesNum, nullptr);
    uint32_t counts[5];
    const PassEntry* tables[5] = {GetCommonPasses(counts[0]), GetReblurPasses(counts[1]), GetSigmaPasses(counts[2]), GetRelaxPasses(counts[3]), GetValidationPasses(counts[4])};
    for (uint32_t p = 0; p < desc.pipelinesNum; p++) {
        for (int t = 0; t < 5; t++)
            for (uint32_t i = 0; i < counts[t]; i++)
                if (!strcmp(tables[t][i].shaderFileName, desc.pipelines[p].shaderFileName))
                    e->launchers[p] = tables[t][i].launch;
        e->translucentShadow |= strstr(desc.pipelines[p].shaderFileName, "SIGMA_ShadowTranslucency_") != nullptr;
    }

    *executor = e;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCreateExecutor(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, NrdHipExecutor** executor) {
    return CreateExecutorImpl(instance, resourceWidth, resourceHeight, 1, hipStream, nullptr, 0, executor);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCreateExecutorLayered(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, uint32_t layersNum, void* hipStream,
    NrdHipExecutor** executor) {
    return CreateExecutorImpl(instance, resourceWidth, resourceHeight, layersNum, hipStream, nullptr, 0, executor);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCreateExecutorWithArena(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, void* arena, uint64_t arenaSize,
    NrdHipExecutor** executor) {
    if (!arena)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    return CreateExecutorImpl(instance, resourceWidth, resourceHeight, 1, hipStream, arena, arenaSize, executor);
}

extern "C" __attribute__((visibility("default"))) uint64_t nrdHipGetArenaSize(void* instance, uint16_t resourceWidth, uint16_t resourceHeight) {
    if (!instance || !resourceWidth || !resourceHeight)
        return 0;
    NrdHipExecutor plan; // (only its pool layout is filled)
    return PlanPools(nrd::GetInstanceDesc(*(nrd::Instance*)instance), resourceWidth, resourceHeight, plan) ? plan.permanentBytes + plan.transientBytes : 0;
}

extern "C" __attribute__((visibility("default"))) void nrdHipDestroyExecutor(NrdHipExecutor* e) {
    if (!e)
        return;
    (void)hipStreamSynchronize(e->stream);
    for (auto& b : e->brackets)
        e->eventPool.insert(e->eventPool.end(), {b.start, b.stop});
    for (hipEvent_t ev : e->eventPool)
        (void)hipEventDestroy(ev);
    for (auto& g : e->graphs) {
        if (g.exec)
            (void)hipGraphExecDestroy(g.exec);
        if (g.graph)
            (void)hipGraphDestroy(g.graph);
    }
    // every allocation the executor owns
    std::vector<void*> owned = {e->ownsArena ? e->arena : nullptr, e->decodedNormalRoughness.ptr, e->worldPosViewZ.ptr, e->viewPos.ptr, e->roughnessWord.ptr, e->tileFlags.ptr, e->motionBits, e->inputReport};
    for (const Plane& twin : e->shifted)
        owned.push_back(twin.ptr);
    for (void* p : owned)
        if (p)
            (void)hipFree(p);
    delete e;
}

// the slots of which every layer of a layered executor has its own plane (SIGMA's noisy inputs and its output); every other slot is one plane read by all layers
static bool IsPerLayerSlot(uint32_t t) {
    using R = nrd::ResourceType;
    return t == (uint32_t)R::IN_PENUMBRA || t == (uint32_t)R::IN_TRANSLUCENCY || t == (uint32_t)R::OUT_SHADOW_TRANSLUCENCY;
}

// nrdHipBindResource (layerBytes = 0) and nrdHipBindResourceLayers: the same rules for the plane, which describes layer 0
static uint32_t BindPlane(NrdHipExecutor* e, uint32_t resourceType, const NrdHipPlaneDesc* plane, uint64_t layerBytes) {

    nrd::Format expected = ExpectedUserFormat((nrd::ResourceType)resourceType, e->translucentShadow);
    if (expected == nrd::Format::MAX_NUM)
        return e->Fail(nrd::Result::UNSUPPORTED, std::string("nrdHipBindResource: slot not supported in this build: ") + nrd::GetResourceTypeString((nrd::ResourceType)resourceType));
    if (plane->format != (uint32_t)expected)
        return e->Fail(nrd::Result::UNSUPPORTED, std::string("nrdHipBindResource: unexpected format for ") + nrd::GetResourceTypeString((nrd::ResourceType)resourceType));

    uint32_t bpt = BytesPerTexel(expected);
    if (!plane->data || plane->width != e->width || plane->height != e->height || plane->rowPitchBytes < plane->width * bpt || (plane->rowPitchBytes % bpt) != 0 ||
        ((uintptr_t)plane->data % bpt) != 0)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResource: bad pointer, size or pitch");
    if (!PlaneAddressable(plane->rowPitchBytes, plane->height))
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipBindResource: row pitch >= 16 MiB or plane > 4 GiB (planes are addressed with 32-bit byte offsets)");

    Plane& p = e->user[resourceType];
    p.ptr = (uint8_t*)plane->data;
    p.pitch = plane->rowPitchBytes;
    p.w = plane->width;
    p.h = plane->height;
    e->userBound[resourceType] = true;
    e->userLayerBytes[resourceType] = layerBytes;
    if (resourceType == (uint32_t)nrd::ResourceType::IN_NORMAL_ROUGHNESS || resourceType == (uint32_t)nrd::ResourceType::IN_VIEWZ)
        e->decodedFresh = false;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipBindResource(NrdHipExecutor* e, uint32_t resourceType, const NrdHipPlaneDesc* plane) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (resourceType >= (uint32_t)nrd::ResourceType::TRANSIENT_POOL)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResource: not a user slot");
    if (e->layersNum > 1 && IsPerLayerSlot(resourceType))
        return e->Fail(nrd::Result::INVALID_ARGUMENT, std::string("nrdHipBindResource: on a layered executor every layer has its own ") + nrd::GetResourceTypeString((nrd::ResourceType)resourceType) +
                                                          "; bind the stack with nrdHipBindResourceLayers");
    return BindPlane(e, resourceType, plane, 0);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipBindResourceLayers(NrdHipExecutor* e, uint32_t resourceType, const NrdHipPlaneDesc* plane, uint64_t layerBytes) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (e->layersNum <= 1)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResourceLayers: the executor has no layers (nrdHipCreateExecutorLayered with layersNum > 1); use nrdHipBindResource");
    if (resourceType >= (uint32_t)nrd::ResourceType::TRANSIENT_POOL || !IsPerLayerSlot(resourceType))
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResourceLayers: not a per-layer slot (IN_PENUMBRA, IN_TRANSLUCENCY, OUT_SHADOW_TRANSLUCENCY); the other slots are shared: nrdHipBindResource");
    if (layerBytes < (uint64_t)plane->rowPitchBytes * plane->height || (layerBytes & 3u) != 0)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResourceLayers: layerBytes must be >= rowPitchBytes x height and a multiple of 4");
    return BindPlane(e, resourceType, plane, layerBytes);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetPoolPlane(NrdHipExecutor* e, uint32_t resourceType, uint32_t indexInPool, NrdHipPlaneDesc* plane) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const bool permanent = resourceType == (uint32_t)nrd::ResourceType::PERMANENT_POOL;
    const std::vector<Plane>& pool = permanent ? e->permanent : e->transient;
    if ((!permanent && resourceType != (uint32_t)nrd::ResourceType::TRANSIENT_POOL) || indexInPool >= pool.size())
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipGetPoolPlane: bad pool or index");
    const Plane& p = pool[indexInPool];
    plane->data = p.ptr;
    plane->rowPitchBytes = p.pitch;
    plane->format = (uint32_t)(permanent ? e->permanentFormat : e->transientFormat)[indexInPool];
    plane->width = (uint16_t)p.w;
    plane->height = (uint16_t)p.h;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetOwnedRows(NrdHipExecutor* e, uint32_t rowBegin, uint32_t rowEnd) {
    if (!e || rowBegin > rowEnd)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (e->layersNum > 1 && (rowBegin != 0 || rowEnd < e->height))
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipSetOwnedRows: a layered executor runs whole frames only (no row strips)");
    e->ownedRowBegin = (int)rowBegin;
    e->ownedRowEnd = rowEnd >= e->height ? INT_MAX : (int)rowEnd;
    return (uint32_t)nrd::Result::SUCCESS;
}

// the inputs the reference addresses at rectOrigin + pixel (Common.hlsli WithRectOrigin / WithRectOffset call sites)
static bool IsGuideInput(nrd::ResourceType t) {
    using R = nrd::ResourceType;
    return t == R::IN_MV || t == R::IN_NORMAL_ROUGHNESS || t == R::IN_VIEWZ || t == R::IN_DIFF_CONFIDENCE || t == R::IN_SPEC_CONFIDENCE || t == R::IN_DISOCCLUSION_THRESHOLD_MIX ||
           t == R::IN_BASECOLOR_METALNESS;
}

// ---- ExecuteRange in three steps: plan the guides (PlanGuides), pre-flight and record every launch (RecordRange), enqueue the records (EnqueueRange) ------------------------------
namespace {

constexpr uint32_t kSuccess = (uint32_t)nrd::Result::SUCCESS;
bool TraceGuideRows() { static const bool trace = getenv("NRD_HIP_TRACE_GUIDE_ROWS") != nullptr; return trace; } // debugging aid of the sharding tests (read once)

struct Range { // what one call executes (ExecuteRange)
    const nrd::InstanceDesc& idesc;
    const nrd::DispatchDesc* descs;
    uint32_t num, first, count;
    const int32_t *rowBegin, *rowEnd;
};

// Step 1's result: where the passes of this call find their guides, and what has to be launched in front of / behind them to make that true
struct GuidePlan {
    bool shiftedRect = false;           // rectOrigin != 0 (e->originX / originY): the guide inputs are read from rect-at-origin twins (kernels_common.hip "shifted rect")
    uint32_t twins[kUserSlots] = {}, twinsNum = 0; // the guide slots of this list that get a twin, in the order the list names them
    bool writesMv = false;              // a pass of the list rewrites IN_MV (REBLUR specular MV modification): the twin goes back into the user's plane behind the last pass
    // a dispatch reads IN_NORMAL_ROUGHNESS (decoded.w != 0): the bound plane is decoded once per list into the planes of the families the list holds. `decoded` = their common
    // geometry (float4 texels at the packed plane's size); its ptr -- the float4 (normal, roughness | material) cache -- is set for RELAX lists only, the one family that reads it
    Plane decoded = {}, viewPos = {}, worldPos = {};
    const void *reblurConstants = nullptr, *relaxConstants = nullptr; // the frame's constants the decode kernels take: the first block of either family in the WHOLE list
    bool decodeNow = false;             // the guide planes are (re)written in front of the first pass of this call ...
    int guideRow0 = 0, guideRow1 = INT_MAX; // ... on these rows ...
    uint32_t fuseDispatch = UINT32_MAX; // ... by this dispatch, the tile classification, instead of a decode kernel (UINT32_MAX: by the decode kernels)
};

static const Plane& GuidePlane(const NrdHipExecutor* e, const GuidePlan& plan, nrd::ResourceType t) { return plan.shiftedRect && e->shifted[(uint32_t)t].ptr ? e->shifted[(uint32_t)t] : e->user[(uint32_t)t]; }

// shifted rect: makes the rect-at-origin twins of the guide inputs this list binds exist
static uint32_t EnsureTwins(NrdHipExecutor* e, const ListScan& scan, GuidePlan& plan) {
    for (uint32_t k = 0; k < scan.slotsNum; k++) {
        const uint32_t t = scan.slots[k];
        if (!IsGuideInput((nrd::ResourceType)t) || !e->userBound[t])
            continue;
        if (e->originX >= e->user[t].w || e->originY >= e->user[t].h)
            return e->Fail(nrd::Result::INVALID_ARGUMENT, "CommonSettings::rectOrigin lies outside the bound planes; nothing was launched");
        Plane& twin = e->shifted[t];
        const Ensured ensured = EnsurePlane(twin, e->user[t]); // (the user's pitch too)
        if (ensured == Ensured::FAILED)
            return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate a shifted-rect guide plane");
        if (ensured == Ensured::REALLOCATED) {
            // cleared at once (a pre-flight failure further down used to leave the new twin uninitialised for the next call); a memset of
            // a private buffer enqueues no pass work, so "nothing is launched before the pre-flight has passed" still holds
            (void)hipMemsetAsync(twin.ptr, 0, (size_t)twin.pitch * (size_t)twin.h, e->stream);
            e->decodedFresh = false;
        }
        plan.twins[plan.twinsNum++] = t;
    }
    plan.writesMv = scan.written[(size_t)nrd::ResourceType::IN_MV] && e->userBound[(size_t)nrd::ResourceType::IN_MV];
    return kSuccess;
}

// Guide planes of the families the list holds, all at the geometry of `decoded`: REBLUR reads (normal, viewZ) + the roughness word, RELAX (normal, roughness | material) + (world
// position, viewZ). Independent of each other: one list may hold both families (e.g. REBLUR_DIFFUSE + RELAX_SPECULAR in one instance), and then both sets are written.
static uint32_t EnsureGuidePlanes(NrdHipExecutor* e, const ListScan& scan, uint32_t first, GuidePlan& plan) {
    const uint32_t slot = (uint32_t)nrd::ResourceType::IN_NORMAL_ROUGHNESS, slotZ = (uint32_t)nrd::ResourceType::IN_VIEWZ;
    if (!scan.read[slot] || !e->userBound[slot])
        return kSuccess;
    Plane& decoded = plan.decoded;
    decoded = Plane{nullptr, ((uint32_t)e->user[slot].w * 16u + 255u) & ~255u, e->user[slot].w, e->user[slot].h};
    // first == 0 starts a new list (= a new frame); a later range decodes only if nothing valid is there (rebound plane, new cache,
    // or a caller that skipped the first range)
    plan.decodeNow = first == 0 || !e->decodedFresh;
    plan.reblurConstants = scan.reblur;
    plan.relaxConstants = scan.relax;
    if (!scan.reblur && !scan.relax)
        return kSuccess; // (SIGMA, REFERENCE: they read the packed plane themselves)
    // the kernels of both families read normal + roughness from these planes only (reblur_device.h NormalRoughnessGuide): they have to exist, and need IN_VIEWZ
    if (!e->userBound[slotZ])
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "resource not bound: IN_VIEWZ; nothing was launched");
    if (e->user[slotZ].w != decoded.w || e->user[slotZ].h != decoded.h)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "IN_VIEWZ and IN_NORMAL_ROUGHNESS differ in size; nothing was launched");
    Plane word = decoded; // viewPos' companion, a quarter of the size: the w word of the decoded normals alone (same texel grid, a quarter of the pitch)
    word.pitch = decoded.pitch / 4u;
    const struct { bool wanted; Plane& plane; const Plane& geometry; const char* what; } planes[] = {
        {scan.reblur != nullptr, e->viewPos, decoded, "view-position guide plane"}, {scan.reblur != nullptr, e->roughnessWord, word, "roughness-word guide plane"},
        {scan.relax != nullptr, e->decodedNormalRoughness, decoded, "decoded normal/roughness cache"}, {scan.relax != nullptr, e->worldPosViewZ, decoded, "world-position guide plane"}};
    for (const auto& p : planes) {
        const Ensured ensured = p.wanted ? EnsurePlane(p.plane, p.geometry) : Ensured::PRESENT;
        if (ensured == Ensured::REALLOCATED) // what the list's planes held is gone: decode again, now
            e->decodedFresh = false, plan.decodeNow = true;
        if (ensured == Ensured::FAILED) {
            if (&p.plane == &e->roughnessWord) { // the two live and die together: a later call starts over
                (void)hipFree(e->viewPos.ptr);
                e->viewPos = Plane{};
            }
            return e->Fail(nrd::Result::FAILURE, std::string("nrdHipExecuteDispatches: cannot allocate the ") + p.what);
        }
    }
    plan.viewPos = scan.reblur ? e->viewPos : Plane{};
    plan.worldPos = scan.relax ? e->worldPosViewZ : Plane{};
    decoded.ptr = scan.relax ? e->decodedNormalRoughness.ptr : nullptr;
    return kSuccess;
}

// multi-GPU: the guide planes are needed on the rows the passes of this rank read them at -- every dispatch's rows widened by its guide reach, rounded out to the
// 16-row tile grid; the rest of the planes keeps whatever it held (nothing of this list reads it). Whole frame when any dispatch runs on the whole frame.
static void PlanGuideRows(const NrdHipExecutor* e, const Range& range, const ListScan& scan, GuidePlan& plan) {
    int lo = INT_MAX, hi = 0;
    bool whole = range.num == 0;
    for (uint32_t i = 0; i < range.num && !whole; i++) {
        // the guide planes stand in for IN_NORMAL_ROUGHNESS (and IN_VIEWZ next to it): a pass that does not bind it (tile classification) reads none of them
        if (!scan.bindsNormalRoughness[i])
            continue;
        const char* shader = ShaderOf(range.idesc, range.descs[i]);
        const int reach = *shader ? GuideReachRows(shader, range.descs[i].constantBufferData, range.descs[i].constantBufferDataSize) : -1;
        whole = range.rowBegin[i] < 0 || reach < 0;
        if (!whole) {
            lo = std::min(lo, (int)range.rowBegin[i] - reach);
            hi = std::max(hi, (int)range.rowEnd[i] + reach);
        }
    }
    if (!whole && hi > lo) {
        plan.guideRow0 = std::max(lo, 0) & ~15;
        plan.guideRow1 = (hi + 15) & ~15;
    }
    if (TraceGuideRows())
        fprintf(stderr, "[nrdhip] guide planes decoded on rows [%d, %d) of %d\n", plan.guideRow0, plan.guideRow1 == INT_MAX ? (int)e->height : std::min(plan.guideRow1, (int)e->height), (int)e->height);
}

// Whole-frame decode of a single-family list that starts (behind its clears, if any) with that family's tile classification: the classification kernel writes the guide
// planes too (kernels_common.hip DecodeGuidesClassifyKernel) and no decode kernel is launched here. Not with a shifted rect (the twins are prepared first), not
// under row sharding (the strips decode only their rows), not with both families in one list. NRD_HIP_FUSE_CLASSIFY=0: the two separate kernels (A/B switch).
static void PlanFuseDispatch(const Range& range, GuidePlan& plan) {
    static const bool fuseClassify = !(getenv("NRD_HIP_FUSE_CLASSIFY") && atoi(getenv("NRD_HIP_FUSE_CLASSIFY")) == 0);
    if (!(fuseClassify && plan.decodeNow && !plan.shiftedRect && !range.rowBegin && (plan.viewPos.ptr != nullptr) != (plan.worldPos.ptr != nullptr)))
        return;
    const char* classify = plan.viewPos.ptr ? "REBLUR_ClassifyTiles.cs" : "RELAX_ClassifyTiles.cs";
    for (uint32_t i = range.first; i < range.first + range.count; i++) {
        const char* shader = ShaderOf(range.idesc, range.descs[i]);
        if (!strncmp(shader, "Clear_", 6))
            continue;
        if (!strcmp(shader, classify) && (plan.viewPos.ptr ? (const void*)ConstantsAs<nrdc::ReblurConstants>(Family::REBLUR, shader, range.descs[i].constantBufferData, range.descs[i].constantBufferDataSize)
                                                        : (const void*)ConstantsAs<nrdc::RelaxConstants>(Family::RELAX, shader, range.descs[i].constantBufferData, range.descs[i].constantBufferDataSize)))
            plan.fuseDispatch = i;
        break;
    }
    if (TraceGuideRows() && plan.fuseDispatch != UINT32_MAX)
        fprintf(stderr, "[nrdhip] guide planes written by the tile classification kernel (dispatch %u)\n", plan.fuseDispatch);
}

// Step 1, plan guides, from ONE scan of the WHOLE list (not of the range): origin, constants, guide use. Allocates the private planes the list needs, enqueues no pass work.
static uint32_t PlanGuides(NrdHipExecutor* e, const Range& range, GuidePlan& plan) {
    std::vector<uint8_t> bindsNormalRoughness(range.rowBegin ? range.num : 0); // (row sharding only)
    const ListScan scan = ScanDispatchList(range.idesc, range.descs, range.num, range.rowBegin ? bindsNormalRoughness.data() : nullptr);
    e->originX = scan.originX, e->originY = scan.originY;
    plan.shiftedRect = e->originX != 0 || e->originY != 0;
    uint32_t r = plan.shiftedRect ? EnsureTwins(e, scan, plan) : kSuccess;
    if (r == kSuccess)
        r = EnsureGuidePlanes(e, scan, range.first, plan);
    if (r != kSuccess)
        return r;
    if (range.rowBegin && range.rowEnd && plan.decodeNow)
        PlanGuideRows(e, range, scan, plan);
    PlanFuseDispatch(range, plan);
    return kSuccess;
}

// Step 2's result: every launch of the call as data
struct Recording {
    LaunchRecorder recorder;
    // records [0, end[0]): the shift / decode kernels in front of the first pass; [end[k], end[k + 1]): pass first + k; [end.back(), all): the IN_MV twin back into the user's plane
    std::vector<uint32_t> end;
};

// back = false, once per list in front of its first pass: the rect-at-origin twins of the guide inputs (shifted rect only: there are none otherwise), then the decoded guides;
// back = true, behind its last pass: the IN_MV twin into the user's plane
static void RecordGuideKernels(NrdHipExecutor* e, const GuidePlan& plan, LaunchRecorder* rec, bool back) {
    PassArgs args = {};
    args.stream = e->stream;
    args.recorder = rec;
    for (uint32_t k = 0; k < plan.twinsNum; k++) {
        const uint32_t t = plan.twins[k];
        if (!back || t == (uint32_t)nrd::ResourceType::IN_MV)
            LaunchShiftPlane(args, e->user[t], e->shifted[t], e->originX, e->originY, BytesPerTexel(ExpectedUserFormat((nrd::ResourceType)t, e->translucentShadow)), back);
    }
    if (back || !plan.decodeNow || plan.fuseDispatch != UINT32_MAX)
        return;
    args.rowBegin = plan.guideRow0;
    args.rowEnd = plan.guideRow1;
    const Plane &packed = GuidePlane(e, plan, nrd::ResourceType::IN_NORMAL_ROUGHNESS), &viewZ = GuidePlane(e, plan, nrd::ResourceType::IN_VIEWZ);
    if (plan.worldPos.ptr)
        LaunchDecodeGuidesRelax(args, packed, viewZ, plan.decoded, plan.worldPos, plan.relaxConstants);
    if (plan.viewPos.ptr)
        LaunchDecodeGuides(args, packed, viewZ, plan.viewPos, e->roughnessWord, plan.reblurConstants);
}

// Resolves the resources of dispatch i and fills the launcher arguments (no launch). Returns nullptr or an error text.
static const char* FillPassArgs(NrdHipExecutor* e, const Range& range, const GuidePlan& plan, uint32_t i, PassArgs& args, std::string& msg) {
    const nrd::DispatchDesc& d = range.descs[i];
    e->scratchPlanes.resize(d.resourcesNum);
    e->scratchBytesPerTexel.resize(d.resourcesNum);
    e->scratchFormats.resize(d.resourcesNum);
    e->scratchLayerStrides.resize(d.resourcesNum);
    auto use = [&](uint32_t r, const Plane& plane, nrd::Format format, uint64_t layerStride) {
        e->scratchPlanes[r] = plane;
        e->scratchLayerStrides[r] = e->layersNum > 1 ? layerStride : 0;
        e->scratchBytesPerTexel[r] = (uint8_t)BytesPerTexel(format);
        e->scratchFormats[r] = (uint8_t)format;
    };
    for (uint32_t r = 0; r < d.resourcesNum; r++) {
        const nrd::ResourceDesc& res = d.resources[r];
        if (res.type == nrd::ResourceType::PERMANENT_POOL) {
            if (res.indexInPool >= e->permanent.size())
                return "permanent pool index out of range";
            use(r, e->permanent[res.indexInPool], e->permanentFormat[res.indexInPool], e->permanentStride[res.indexInPool]);
        } else if (res.type == nrd::ResourceType::TRANSIENT_POOL) {
            if (res.indexInPool >= e->transient.size())
                return "transient pool index out of range";
            // (the identity, except for an instance created under NRD_HIP_REFERENCE_QUIRKS: csrc/host/instance.h)
            const uint16_t index = nrd::TransientAliasOf(*e->instance, d.identifier, res.indexInPool);
            if (index >= e->transient.size())
                return "transient pool index out of range";
            use(r, e->transient[index], e->transientFormat[index], e->transientStride[index]);
        } else {
            uint32_t t = (uint32_t)res.type;
            if (t >= (uint32_t)nrd::ResourceType::MAX_NUM || !e->userBound[t]) {
                msg = std::string("resource not bound: ") + (nrd::GetResourceTypeString(res.type) ? nrd::GetResourceTypeString(res.type) : "?");
                return msg.c_str();
            }
            if (e->layersNum > 1 && IsPerLayerSlot(t) && !e->userLayerBytes[t]) { // (unreachable through the entry points: nrdHipBindResource refuses these slots)
                msg = std::string("not bound as a stack of layers: ") + nrd::GetResourceTypeString(res.type);
                return msg.c_str();
            }
            use(r, (e->originX || e->originY) && IsGuideInput(res.type) && e->shifted[t].ptr ? e->shifted[t] : e->user[t], ExpectedUserFormat(res.type, e->translucentShadow), e->userLayerBytes[t]);
        }
    }
    args.planes = e->scratchPlanes.data();
    args.planesNum = d.resourcesNum;
    args.bytesPerTexel = e->scratchBytesPerTexel.data();
    args.formats = e->scratchFormats.data();
    args.layersNum = e->layersNum;
    args.layerStrides = e->layersNum > 1 ? e->scratchLayerStrides.data() : nullptr;
    args.constants = d.constantBufferData;
    args.constantsSize = d.constantBufferDataSize;
    args.gridWidth = d.gridWidth;
    args.gridHeight = d.gridHeight;
    args.stream = e->stream;
    size_t oo, of;
    if (plan.shiftedRect && d.constantBufferData && RectOriginOffsets(ShaderOf(range.idesc, d), d.constantBufferDataSize, oo, of)) {
        // the passes run on rect-at-origin guides: they must see rectOrigin = rectOffset = 0
        std::vector<uint8_t>& copy = e->patchedConstants[i - range.first];
        copy.assign((const uint8_t*)d.constantBufferData, (const uint8_t*)d.constantBufferData + d.constantBufferDataSize);
        memset(copy.data() + oo, 0, 8);
        memset(copy.data() + of, 0, 8);
        args.constants = copy.data();
    }
    const bool strip = range.rowBegin && range.rowBegin[i] >= 0;
    args.rowBegin = strip ? range.rowBegin[i] : 0;
    args.rowEnd = strip ? range.rowEnd[i] : INT_MAX;
    args.decodedNormalRoughness = plan.decoded;
    args.worldPosViewZ = plan.worldPos;
    args.viewPos = plan.viewPos;
    args.roughnessWord = plan.viewPos.ptr ? e->roughnessWord : Plane{};
    args.tileFlags = e->tileFlags;
    args.historyReachWord = e->historyReachWord;
    args.windowRegion = e->windowRegion;
    if (i == plan.fuseDispatch)
        args.fuseGuidesFrom = GuidePlane(e, plan, nrd::ResourceType::IN_NORMAL_ROUGHNESS);
    return nullptr;
}

static std::string PassName(const Range& range, const nrd::DispatchDesc& d) {
    return std::string("'") + (d.name ? d.name : "?") + "' (" + (d.pipelineIndex < range.idesc.pipelinesNum ? range.idesc.pipelines[d.pipelineIndex].shaderFileName : "?") + ")";
}

// Step 2, pre-flight and record: every pass of the range must have a launcher, bound resources and pass its own support checks BEFORE anything is enqueued
// (the reference integration's contract: a Denoise call either runs completely or not at all). The same walk records every launch (kernel, grid,
// arguments); the records are then either turned into / matched against a graph or launched one by one -- the launchers run once per frame.
static uint32_t RecordRange(NrdHipExecutor* e, const Range& range, const GuidePlan& plan, Recording& rec) {
    rec.recorder.keep = true;
    const bool prepareNow = plan.decodeNow || (plan.shiftedRect && (range.first == 0 || !e->decodedFresh));
    if (prepareNow)
        RecordGuideKernels(e, plan, &rec.recorder, false);
    rec.end.assign(1, (uint32_t)rec.recorder.records.size());
    e->patchedConstants.assign(plan.shiftedRect ? range.count : 0, std::vector<uint8_t>());
    for (uint32_t i = range.first; i < range.first + range.count; i++) {
        const nrd::DispatchDesc& d = range.descs[i];
        if (d.pipelineIndex >= e->launchers.size())
            return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipExecuteDispatches: pipeline index out of range");
        PassLauncher launch = e->launchers[d.pipelineIndex];
        if (!launch)
            return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipExecuteDispatches: no HIP kernel for pass " + PassName(range, d) + "; nothing was launched");
        if (e->layersNum > 1 && strncmp(ShaderOf(range.idesc, d), "SIGMA_", 6) != 0 && strncmp(ShaderOf(range.idesc, d), "Clear_", 6) != 0)
            return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipExecuteDispatches: a layered executor runs SIGMA and Clear passes only, not " + PassName(range, d) + "; nothing was launched");
        if (d.constantBufferDataSize && !d.constantBufferData)
            return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipExecuteDispatches: pass " + PassName(range, d) + " has no constant data (constant arena overflow?); nothing was launched");
        PassArgs args = {};
        std::string msg;
        if (const char* err = FillPassArgs(e, range, plan, i, args, msg))
            return e->Fail(nrd::Result::INVALID_ARGUMENT, std::string(err) + " in pass " + PassName(range, d) + "; nothing was launched");
        args.recorder = &rec.recorder;
        if (const char* err = launch(args))
            return e->Fail(nrd::Result::UNSUPPORTED, std::string(err) + " [pass " + PassName(range, d) + "; nothing was launched]");
        rec.end.push_back((uint32_t)rec.recorder.records.size());
    }
    if (plan.shiftedRect && plan.writesMv && range.first + range.count == range.num)
        RecordGuideKernels(e, plan, &rec.recorder, true);
    return kSuccess;
}

// Step 3, enqueue: the records as one graph launch (graph mode, unless profiling: events cannot bracket graph nodes) or one by one
static uint32_t EnqueueRange(NrdHipExecutor* e, const Range& range, Recording& rec) {
    if (e->graphMode && !e->profiling)
        return LaunchAsGraph(e, rec.recorder.records);
    // launches records [begin, end); timed: between two events, as the row `pipelineIndex` of nrdHipCollectPassTimings. Launch-configuration errors are returned (no synchronisation)
    auto enqueue = [&](uint32_t begin, uint32_t end, bool timed, uint32_t pipelineIndex) {
        NrdHipExecutor::Bracket bracket = {};
        if (timed) {
            for (hipEvent_t* ev : {&bracket.start, &bracket.stop}) // a recycled event, or a new one
                if (e->eventPool.empty())
                    (void)hipEventCreate(ev);
                else
                    *ev = e->eventPool.back(), e->eventPool.pop_back();
            bracket.pipelineIndex = pipelineIndex;
            (void)hipEventRecord(bracket.start, e->stream);
        }
        for (uint32_t k = begin; k < end; k++)
            rec.recorder.records[k].launch(rec.recorder.records[k], e->stream);
        const hipError_t error = hipGetLastError();
        if (timed) {
            (void)hipEventRecord(bracket.stop, e->stream);
            e->brackets.push_back(bracket);
        }
        return error;
    };
    // the guide preparation: outside the timing bracket of the first pass; profiled as a row of its own (pipeline index == number of pipelines: include/NRDHip.h nrdHipCollectPassTimings)
    if (enqueue(0, rec.end[0], e->profiling && rec.end[0] > 0, (uint32_t)e->launchers.size()) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "HIP launch failed while preparing the guide planes");
    for (uint32_t k = 0; k < range.count; k++) {
        const nrd::DispatchDesc& d = range.descs[range.first + k];
        const hipError_t launchError = enqueue(rec.end[k], rec.end[k + 1], e->profiling, d.pipelineIndex);
        if (launchError != hipSuccess)
            return e->Fail(nrd::Result::FAILURE, "HIP launch failed in pass " + PassName(range, d) + ": " + hipGetErrorString(launchError));
    }
    if (enqueue(rec.end.back(), (uint32_t)rec.recorder.records.size(), false, 0) != hipSuccess) // the IN_MV twin back into the user's plane
        return e->Fail(nrd::Result::FAILURE, "HIP launch failed while copying IN_MV back");
    return kSuccess;
}

} // namespace

// Executes dispatches [first, first + count) of the list. rowBegin / rowEnd (indexed by absolute dispatch index, may be null = whole
// frame; rowBegin[i] < 0 = whole frame for that dispatch) give the rows each pass has to produce. The per-list caches (decoded
// normal/roughness, a-trous world positions) are (re)built when first == 0.
static uint32_t ExecuteRange(NrdHipExecutor* e, const nrd::DispatchDesc* descs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count, const int32_t* rowBegin, const int32_t* rowEnd) {
    const Range range = {nrd::GetInstanceDesc(*e->instance), descs, dispatchDescsNum, first, count, rowBegin, rowEnd};
    GuidePlan plan;
    Recording rec;
    uint32_t r = PlanGuides(e, range, plan);
    if (r == kSuccess)
        r = RecordRange(e, range, plan, rec);
    if (r == kSuccess) // ---- from here on work is enqueued
        r = EnqueueRange(e, range, rec);
    if (r != kSuccess)
        return r;
    if (plan.decoded.w || plan.shiftedRect)
        e->decodedFresh = first + count < dispatchDescsNum; // the list is complete: the next call belongs to another frame
    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, std::string("HIP launch failed: ") + hipGetErrorString(err));
    return kSuccess;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipExecuteDispatchRange(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count,
    const int32_t* rowBegin, const int32_t* rowEnd) {
    if (!e || (!dispatchDescs && dispatchDescsNum) || first > dispatchDescsNum || count > dispatchDescsNum - first || (rowBegin == nullptr) != (rowEnd == nullptr))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (e->layersNum > 1 && rowBegin)
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipExecuteDispatchRange: a layered executor runs whole frames only (pass NULL row arrays); nothing was launched");
    return ExecuteRange(e, (const nrd::DispatchDesc*)dispatchDescs, dispatchDescsNum, first, count, rowBegin, rowEnd);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipExecuteDispatches(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum) {
    if (!e || (!dispatchDescs && dispatchDescsNum))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const nrd::DispatchDesc* descs = (const nrd::DispatchDesc*)dispatchDescs;
    if (e->ownedRowBegin <= 0 && e->ownedRowEnd == INT_MAX)
        return ExecuteRange(e, descs, dispatchDescsNum, 0, dispatchDescsNum, nullptr, nullptr);
    // row-strip sharding (nrdHipSetOwnedRows): every pass on the strip extended by the reach of the passes behind it
    std::vector<int32_t> rowBegin(dispatchDescsNum), rowEnd(dispatchDescsNum);
    OwnedRowRanges(*e->instance, descs, dispatchDescsNum, e->ownedRowBegin, e->ownedRowEnd, rowBegin.data(), rowEnd.data());
    return ExecuteRange(e, descs, dispatchDescsNum, 0, dispatchDescsNum, rowBegin.data(), rowEnd.data());
}

// Multi-GPU: where the temporal passes report how far (rows) they read last frame's planes from a pixel's own row (include/NRDHip.h). The word belongs to the caller, who clears
// it (in stream order) before a frame and reads / all-reduces it after; nullptr switches the tracking off (the default: the kernels then skip it on a uniform branch).
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetHistoryReachWord(NrdHipExecutor* e, void* deviceWord) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->historyReachWord = (uint32_t*)deviceWord; // (graph mode: a kernel argument like any other -- the node parameters are updated when they change)
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipDenoise(NrdHipExecutor* e, const uint32_t* identifiers, uint32_t identifiersNum) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const nrd::DispatchDesc* descs = nullptr;
    uint32_t num = 0;
    nrd::Result r = nrd::GetComputeDispatches(*e->instance, identifiers, identifiersNum, descs, num);
    if (r != nrd::Result::SUCCESS)
        return e->Fail(r, "nrd::GetComputeDispatches failed");
    return nrdHipExecuteDispatches(e, descs, num);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetPoolMemoryUsage(const NrdHipExecutor* e, uint64_t* permanentBytes, uint64_t* transientBytes) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (permanentBytes)
        *permanentBytes = e->permanentBytes;
    if (transientBytes)
        *transientBytes = e->transientBytes;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) const char* nrdHipGetLastError(const NrdHipExecutor* e) { return e ? e->lastError.c_str() : "null executor"; }
