// HIP executor: owns the pool planes in HBM and turns an nrd::DispatchDesc list into kernel launches on one stream.
// Plays the role of the reference integration layer (reference Integration/NRDIntegration.hpp:292-454 pool creation,
// :516-623 Denoise, :625-803 Dispatch) -- without descriptor sets, barriers or a constant ring buffer: planes are raw
// pointers, constants travel as kernel arguments, ordering is stream order.
#include "NRD.h"
#include "NRDHip.h"

#include "nrdmath.h" // NRD_NORMAL_ENCODING
#include "passes.h"

#include "../common/pass_constants.h"
#include "../host/halo_plan.h" // the host-only sharding planner: GuideReachRows, OwnedRowRanges

namespace nrd { // csrc/host/instance.h (the host side of this library; not part of the public API)
uint16_t TransientAliasOf(const Instance& instance, Identifier identifier, uint16_t indexInPool);
}

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace nrdhip;

namespace {

static_assert((uint32_t)nrd::Format::RGBA8_UNORM == FORMAT_RGBA8_UNORM && (uint32_t)nrd::Format::R16_UNORM == FORMAT_R16_UNORM && (uint32_t)nrd::Format::RGBA16_SNORM == FORMAT_RGBA16_SNORM && (uint32_t)nrd::Format::RGBA16_SFLOAT == FORMAT_RGBA16_SFLOAT,
    "passes.h format constants");

uint32_t BytesPerTexel(nrd::Format f) {
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

// Format each user slot must have in this build (MAX_NUM = slot not supported)
// translucentShadow: the instance holds SIGMA_SHADOW_TRANSLUCENCY, whose output is (shadow, translucent colour) in RGBA8
nrd::Format ExpectedUserFormat(nrd::ResourceType t, bool translucentShadow) {
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

} // namespace

struct NrdHipExecutor {
    nrd::Instance* instance = nullptr;
    hipStream_t stream = nullptr;
    uint16_t width = 0, height = 0;

    uint8_t* arena = nullptr;
    bool ownsArena = true;
    int ownedRowBegin = 0, ownedRowEnd = INT_MAX;
    bool profiling = false;
    struct Bracket {
        hipEvent_t start, stop;
        uint16_t pipelineIndex;
    };
    std::vector<Bracket> brackets;   // recorded since the last collect
    std::vector<hipEvent_t> eventPool; // recycled events
    uint64_t permanentBytes = 0, transientBytes = 0;
    std::vector<Plane> permanent, transient;
    Plane decodedNormalRoughness = {}; // internal float4 cache of IN_NORMAL_ROUGHNESS (not an NRD pool plane; own allocation)
    Plane worldPosViewZ = {};          // internal float4 scratch of the RELAX a-trous chain (world position + viewZ per pixel)
    int windowRegion[3] = {0, 0, 0};   // {tile columns, first tile row, end tile row} of the last window-kernel launch (passes.h PassArgs::windowRegion)
    Plane tileFlags = {};              // one byte per 32x8-pixel workgroup tile: hand-over between the two kernels of a split pass (kernels_reblur_ta.hip "window")
    Plane viewPos = {};                // internal float4 guide plane of the REBLUR lists (decoded normal + viewZ per pixel)
    Plane roughnessWord = {};          // internal 4-B/px copy of the decoded normals' w word, written with viewPos (passes.h PassArgs::roughnessWord)
    uint32_t* historyReachWord = nullptr; // nrdHipSetHistoryReachWord: the CALLER'S device word the temporal passes report their history reach into (passes.h); null = not tracked
    uint32_t* motionBits = nullptr;    // nrdHipMeasureMotionRows: the reduction's result (float bits), own 4-byte allocation made on first use
    uint32_t* inputReport = nullptr;   // nrdHipCheckInputs: the device copy of the NrdHipInputReport, own allocation made on first use
    std::vector<nrd::Format> permanentFormat, transientFormat;

    Plane user[(size_t)nrd::ResourceType::MAX_NUM] = {};
    bool userBound[(size_t)nrd::ResourceType::MAX_NUM] = {};
    // CommonSettings::rectOrigin != 0: rect-at-origin copies of the guide inputs (kernels_common.hip "shifted rect"); own allocations, made on demand
    Plane shifted[(size_t)nrd::ResourceType::MAX_NUM] = {};
    int originX = 0, originY = 0;   // origin of the list being executed
    std::vector<std::vector<uint8_t>> patchedConstants; // per dispatch of the range: the constant block with gRectOrigin / gRectOffset zeroed

    std::vector<PassLauncher> launchers; // per pipeline index (nullptr = pass not implemented in this build)
    std::vector<Plane> scratchPlanes;
    std::vector<uint8_t> scratchBytesPerTexel, scratchFormats;
    bool translucentShadow = false; // a SIGMA_ShadowTranslucency_* pipeline exists: OUT_SHADOW_TRANSLUCENCY is RGBA8
    std::string lastError;
    // per-list caches (decoded guides, a-trous world positions) are valid for the dispatch list being executed: cleared when a list
    // completes, when IN_NORMAL_ROUGHNESS is rebound and when the cache is (re)allocated, so a range with first > 0 never reads stale guides
    bool decodedFresh = false;

    // graph mode (nrdHipSetGraphMode): the launches of a dispatch range become the kernel nodes of a hipGraph that is instantiated once per
    // topology (sequence of kernels) and re-launched with updated node parameters (constants, ping-pong planes) on the following frames
    bool graphMode = false;
    struct CachedGraph {
        std::vector<const void*> funcs; // topology key
        std::vector<LaunchRecord> records; // parameters the executable graph currently holds
        std::vector<hipGraphNode_t> nodes;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        uint64_t lastUse = 0;
    };
    std::vector<CachedGraph> graphs;
    uint64_t graphClock = 0, graphLaunches = 0, graphBuilds = 0, graphNodeUpdates = 0;

    uint32_t Fail(nrd::Result r, const std::string& msg) {
        lastError = msg;
        return (uint32_t)r;
    }
};

static bool PlanPool(const nrd::TextureDesc* descs, uint32_t num, uint16_t w, uint16_t h, std::vector<Plane>& planes, std::vector<nrd::Format>& formats, uint64_t& offset) {
    planes.resize(num);
    formats.resize(num);
    for (uint32_t i = 0; i < num; i++) {
        uint32_t bpt = BytesPerTexel(descs[i].format);
        if (!bpt)
            return false;
        int pw = (w + descs[i].downsampleFactor - 1) / descs[i].downsampleFactor;
        int ph = (h + descs[i].downsampleFactor - 1) / descs[i].downsampleFactor;
        uint32_t pitch = ((uint32_t)pw * bpt + 255u) & ~255u;
        planes[i].ptr = (uint8_t*)(uintptr_t)offset; // patched to a real pointer once the arena exists
        planes[i].pitch = pitch;
        planes[i].w = pw;
        planes[i].h = ph;
        formats[i] = descs[i].format;
        offset += ((uint64_t)pitch * (uint64_t)ph + 255u) & ~(uint64_t)255u;
    }
    return true;
}

// The kernels address a plane with 32-bit byte offsets built by a 24-bit multiply (planes.h TexelOffset): row pitch < 2^24 bytes, pitch x rows < 2^32 bytes (strictly: the offset of the row one past the end must not wrap either). Every frame size a
// 16-bit resource size can name stays below that except the very largest with 16-byte texels (RGBA32F pool planes, the decoded-guide cache: 16384 x 16384 texels and more) -- refused
// at creation / binding instead of wrapping around.
static bool PlaneAddressable(uint64_t pitchBytes, uint64_t rows) { return pitchBytes < (1ull << 24) && pitchBytes * rows < (1ull << 32); }

static uint32_t CreateExecutorImpl(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, void* userArena, uint64_t userArenaSize, NrdHipExecutor** executor) {
    if (!instance || !executor || !resourceWidth || !resourceHeight)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    *executor = nullptr;
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

    const nrd::InstanceDesc& desc = nrd::GetInstanceDesc(*e->instance);

    uint64_t offset = 0;
    bool ok = PlanPool(desc.permanentPool, desc.permanentPoolSize, resourceWidth, resourceHeight, e->permanent, e->permanentFormat, offset);
    e->permanentBytes = offset;
    ok = ok && PlanPool(desc.transientPool, desc.transientPoolSize, resourceWidth, resourceHeight, e->transient, e->transientFormat, offset);
    e->transientBytes = offset - e->permanentBytes;
    if (!ok) {
        delete e;
        return (uint32_t)nrd::Result::UNSUPPORTED;
    }

    if (offset) {
        if (userArena) {
            if (userArenaSize < offset || ((uintptr_t)userArena & 255u) != 0) {
                delete e;
                return (uint32_t)nrd::Result::INVALID_ARGUMENT;
            }
            e->arena = (uint8_t*)userArena;
            e->ownsArena = false;
        } else if (hipMalloc((void**)&e->arena, offset) != hipSuccess) {
            delete e;
            return (uint32_t)nrd::Result::FAILURE;
        }
        (void)hipMemsetAsync(e->arena, 0, offset, e->stream);
        for (Plane& p : e->permanent)
            p.ptr = e->arena + (uintptr_t)p.ptr;
        for (Plane& p : e->transient)
            p.ptr = e->arena + (uintptr_t)p.ptr;
    }

    // per-tile flags of the passes that run as a fast kernel plus a fallback kernel for the tiles the fast one declines (tiny: one byte per 32x8 pixels)
    e->tileFlags.w = (resourceWidth + 31) / 32;
    e->tileFlags.h = (resourceHeight + 7) / 8;
    e->tileFlags.pitch = ((uint32_t)e->tileFlags.w + (uint32_t)TILE_FLAG_GROUP - 1u) / (uint32_t)TILE_FLAG_GROUP * (uint32_t)TILE_FLAG_GROUP; // the fallback kernels read whole groups of flags (planes.h AnyTileFlagUniform)
    if (hipMalloc((void**)&e->tileFlags.ptr, (size_t)e->tileFlags.pitch * (size_t)e->tileFlags.h) != hipSuccess) {
        if (e->arena && e->ownsArena)
            (void)hipFree(e->arena);
        delete e;
        return (uint32_t)nrd::Result::FAILURE;
    }
    (void)hipMemsetAsync(e->tileFlags.ptr, 0, (size_t)e->tileFlags.pitch * (size_t)e->tileFlags.h, e->stream);

    // pipeline index -> launcher
    e->launchers.assign(desc.pipelinesNum, nullptr);
    const PassEntry* tables[5];
    uint32_t counts[5];
    tables[0] = GetCommonPasses(counts[0]);
    tables[1] = GetReblurPasses(counts[1]);
    tables[2] = GetSigmaPasses(counts[2]);
    tables[3] = GetRelaxPasses(counts[3]);
    tables[4] = GetValidationPasses(counts[4]);
    for (uint32_t p = 0; p < desc.pipelinesNum; p++)
        for (int t = 0; t < 5; t++)
            for (uint32_t i = 0; i < counts[t]; i++)
                if (!strcmp(tables[t][i].shaderFileName, desc.pipelines[p].shaderFileName))
                    e->launchers[p] = tables[t][i].launch;
    for (uint32_t p = 0; p < desc.pipelinesNum; p++)
        e->translucentShadow |= strstr(desc.pipelines[p].shaderFileName, "SIGMA_ShadowTranslucency_") != nullptr;

    *executor = e;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCreateExecutor(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, NrdHipExecutor** executor) {
    return CreateExecutorImpl(instance, resourceWidth, resourceHeight, hipStream, nullptr, 0, executor);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCreateExecutorWithArena(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, void* arena, uint64_t arenaSize,
    NrdHipExecutor** executor) {
    if (!arena)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    return CreateExecutorImpl(instance, resourceWidth, resourceHeight, hipStream, arena, arenaSize, executor);
}

extern "C" __attribute__((visibility("default"))) uint64_t nrdHipGetArenaSize(void* instance, uint16_t resourceWidth, uint16_t resourceHeight) {
    if (!instance || !resourceWidth || !resourceHeight)
        return 0;
    const nrd::InstanceDesc& desc = nrd::GetInstanceDesc(*(nrd::Instance*)instance);
    std::vector<Plane> planes;
    std::vector<nrd::Format> formats;
    uint64_t offset = 0;
    if (!PlanPool(desc.permanentPool, desc.permanentPoolSize, resourceWidth, resourceHeight, planes, formats, offset))
        return 0;
    if (!PlanPool(desc.transientPool, desc.transientPoolSize, resourceWidth, resourceHeight, planes, formats, offset))
        return 0;
    return offset;
}

extern "C" __attribute__((visibility("default"))) void nrdHipDestroyExecutor(NrdHipExecutor* e) {
    if (!e)
        return;
    (void)hipStreamSynchronize(e->stream);
    for (auto& b : e->brackets) {
        (void)hipEventDestroy(b.start);
        (void)hipEventDestroy(b.stop);
    }
    for (hipEvent_t ev : e->eventPool)
        (void)hipEventDestroy(ev);
    for (auto& g : e->graphs) {
        if (g.exec)
            (void)hipGraphExecDestroy(g.exec);
        if (g.graph)
            (void)hipGraphDestroy(g.graph);
    }
    if (e->arena && e->ownsArena)
        (void)hipFree(e->arena);
    if (e->decodedNormalRoughness.ptr)
        (void)hipFree(e->decodedNormalRoughness.ptr);
    if (e->worldPosViewZ.ptr)
        (void)hipFree(e->worldPosViewZ.ptr);
    if (e->viewPos.ptr)
        (void)hipFree(e->viewPos.ptr);
    if (e->roughnessWord.ptr)
        (void)hipFree(e->roughnessWord.ptr);
    if (e->tileFlags.ptr)
        (void)hipFree(e->tileFlags.ptr);
    if (e->motionBits)
        (void)hipFree(e->motionBits);
    if (e->inputReport)
        (void)hipFree(e->inputReport);
    for (Plane& p : e->shifted)
        if (p.ptr)
            (void)hipFree(p.ptr);
    delete e;
}

static hipEvent_t AcquireEvent(NrdHipExecutor* e) {
    if (!e->eventPool.empty()) {
        hipEvent_t ev = e->eventPool.back();
        e->eventPool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    (void)hipEventCreate(&ev);
    return ev;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetProfiling(NrdHipExecutor* e, uint32_t enable) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->profiling = enable != 0;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCollectPassTimings(NrdHipExecutor* e, uint32_t* pipelineIndices, double* milliseconds, uint32_t* launches, uint32_t capacity, uint32_t* written) {
    if (!e || !pipelineIndices || !milliseconds || !launches || !written)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (hipStreamSynchronize(e->stream) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "hipStreamSynchronize failed");
    // (one slot more than there are pipelines: index == pipelinesNum is the per-frame guide preparation -- decode / shift kernels in front of the first pass)
    std::vector<double> ms(e->launchers.size() + 1, 0.0);
    std::vector<uint32_t> n(e->launchers.size() + 1, 0);
    for (auto& b : e->brackets) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, b.start, b.stop) == hipSuccess && b.pipelineIndex < ms.size()) {
            ms[b.pipelineIndex] += t;
            n[b.pipelineIndex]++;
        }
        e->eventPool.push_back(b.start);
        e->eventPool.push_back(b.stop);
    }
    e->brackets.clear();
    uint32_t k = 0;
    for (size_t i = 0; i < ms.size() && k < capacity; i++)
        if (n[i]) {
            pipelineIndices[k] = (uint32_t)i;
            milliseconds[k] = ms[i];
            launches[k] = n[i];
            k++;
        }
    *written = k;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipBindResource(NrdHipExecutor* e, uint32_t resourceType, const NrdHipPlaneDesc* plane) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (resourceType >= (uint32_t)nrd::ResourceType::TRANSIENT_POOL)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipBindResource: not a user slot");

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
    if (resourceType == (uint32_t)nrd::ResourceType::IN_NORMAL_ROUGHNESS || resourceType == (uint32_t)nrd::ResourceType::IN_VIEWZ)
        e->decodedFresh = false;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetPoolPlane(NrdHipExecutor* e, uint32_t resourceType, uint32_t indexInPool, NrdHipPlaneDesc* plane) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const std::vector<Plane>* pool = nullptr;
    const std::vector<nrd::Format>* formats = nullptr;
    if (resourceType == (uint32_t)nrd::ResourceType::PERMANENT_POOL) {
        pool = &e->permanent;
        formats = &e->permanentFormat;
    } else if (resourceType == (uint32_t)nrd::ResourceType::TRANSIENT_POOL) {
        pool = &e->transient;
        formats = &e->transientFormat;
    }
    if (!pool || indexInPool >= pool->size())
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipGetPoolPlane: bad pool or index");
    const Plane& p = (*pool)[indexInPool];
    plane->data = p.ptr;
    plane->rowPitchBytes = p.pitch;
    plane->format = (uint32_t)(*formats)[indexInPool];
    plane->width = (uint16_t)p.w;
    plane->height = (uint16_t)p.h;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetOwnedRows(NrdHipExecutor* e, uint32_t rowBegin, uint32_t rowEnd) {
    if (!e || rowBegin > rowEnd)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->ownedRowBegin = (int)rowBegin;
    e->ownedRowEnd = rowEnd >= e->height ? INT_MAX : (int)rowEnd;
    return (uint32_t)nrd::Result::SUCCESS;
}

// Executes dispatches [first, first + count) of the list. rowBegin / rowEnd (indexed by absolute dispatch index, may be null = whole
// frame; rowBegin[i] < 0 = whole frame for that dispatch) give the rows each pass has to produce. The per-list caches (decoded
// normal/roughness, a-trous world positions) are (re)built when first == 0.
static uint32_t ExecuteRange(NrdHipExecutor* e, const nrd::DispatchDesc* descs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count, const int32_t* rowBegin, const int32_t* rowEnd);

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipExecuteDispatchRange(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count,
    const int32_t* rowBegin, const int32_t* rowEnd) {
    if (!e || (!dispatchDescs && dispatchDescsNum) || first > dispatchDescsNum || count > dispatchDescsNum - first || (rowBegin == nullptr) != (rowEnd == nullptr))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
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

// the inputs the reference addresses at rectOrigin + pixel (Common.hlsli WithRectOrigin / WithRectOffset call sites)
static bool IsGuideInput(nrd::ResourceType t) {
    using R = nrd::ResourceType;
    return t == R::IN_MV || t == R::IN_NORMAL_ROUGHNESS || t == R::IN_VIEWZ || t == R::IN_DIFF_CONFIDENCE || t == R::IN_SPEC_CONFIDENCE || t == R::IN_DISOCCLUSION_THRESHOLD_MIX ||
           t == R::IN_BASECOLOR_METALNESS;
}
// byte offsets of gRectOrigin (uint2) and gRectOffset (float2) in the shared constant block of a pass family, by shader name; false = the family has none
static bool RectOriginOffsets(const char* shader, uint32_t size, size_t& origin, size_t& offset) {
    if (!strncmp(shader, "REBLUR_", 7) && size >= sizeof(nrdc::ReblurConstants)) {
        origin = offsetof(nrdc::ReblurConstants, gRectOrigin), offset = offsetof(nrdc::ReblurConstants, gRectOffset);
        return true;
    }
    if (!strncmp(shader, "RELAX_", 6) && size >= sizeof(nrdc::RelaxConstants)) {
        origin = offsetof(nrdc::RelaxConstants, gRectOrigin), offset = offsetof(nrdc::RelaxConstants, gRectOffset);
        return true;
    }
    if (!strncmp(shader, "SIGMA_", 6) && size >= sizeof(nrdc::SigmaConstants)) {
        origin = offsetof(nrdc::SigmaConstants, gRectOrigin), offset = offsetof(nrdc::SigmaConstants, gRectOffset);
        return true;
    }
    return false;
}

// Resolves the resources of dispatch i and fills the launcher arguments (no launch). Returns nullptr or an error text.
static const char* PrepareDispatch(NrdHipExecutor* e, const nrd::DispatchDesc& d, PassArgs& args, std::string& err) {
    e->scratchPlanes.resize(d.resourcesNum);
    e->scratchBytesPerTexel.resize(d.resourcesNum);
    e->scratchFormats.resize(d.resourcesNum);
    for (uint32_t r = 0; r < d.resourcesNum; r++) {
        const nrd::ResourceDesc& res = d.resources[r];
        if (res.type == nrd::ResourceType::PERMANENT_POOL) {
            if (res.indexInPool >= e->permanent.size())
                return "permanent pool index out of range";
            e->scratchPlanes[r] = e->permanent[res.indexInPool];
            e->scratchBytesPerTexel[r] = (uint8_t)BytesPerTexel(e->permanentFormat[res.indexInPool]);
            e->scratchFormats[r] = (uint8_t)e->permanentFormat[res.indexInPool];
        } else if (res.type == nrd::ResourceType::TRANSIENT_POOL) {
            if (res.indexInPool >= e->transient.size())
                return "transient pool index out of range";
            // (the identity, except for an instance created under NRD_HIP_REFERENCE_QUIRKS: csrc/host/instance.h)
            const uint16_t index = nrd::TransientAliasOf(*e->instance, d.identifier, res.indexInPool);
            if (index >= e->transient.size())
                return "transient pool index out of range";
            e->scratchPlanes[r] = e->transient[index];
            e->scratchBytesPerTexel[r] = (uint8_t)BytesPerTexel(e->transientFormat[index]);
            e->scratchFormats[r] = (uint8_t)e->transientFormat[index];
        } else {
            uint32_t t = (uint32_t)res.type;
            if (t >= (uint32_t)nrd::ResourceType::MAX_NUM || !e->userBound[t]) {
                err = std::string("resource not bound: ") + (nrd::GetResourceTypeString(res.type) ? nrd::GetResourceTypeString(res.type) : "?");
                return err.c_str();
            }
            e->scratchPlanes[r] = (e->originX || e->originY) && IsGuideInput(res.type) && e->shifted[t].ptr ? e->shifted[t] : e->user[t];
            e->scratchBytesPerTexel[r] = (uint8_t)BytesPerTexel(ExpectedUserFormat(res.type, e->translucentShadow));
            e->scratchFormats[r] = (uint8_t)ExpectedUserFormat(res.type, e->translucentShadow);
        }
    }
    args.planes = e->scratchPlanes.data();
    args.planesNum = d.resourcesNum;
    args.bytesPerTexel = e->scratchBytesPerTexel.data();
    args.formats = e->scratchFormats.data();
    args.constants = d.constantBufferData;
    args.constantsSize = d.constantBufferDataSize;
    args.gridWidth = d.gridWidth;
    args.gridHeight = d.gridHeight;
    args.stream = e->stream;
    return nullptr;
}

// Graph mode: the recorded launches of a range as a linear chain of kernel nodes. One executable graph per topology (sequence of kernels);
// on a topology hit only the nodes whose parameters changed (constants, ping-pong planes, row ranges) are updated before the launch.
static uint32_t LaunchAsGraph(NrdHipExecutor* e, std::vector<LaunchRecord>& records) {
    if (records.empty())
        return (uint32_t)nrd::Result::SUCCESS;
    std::vector<const void*> funcs(records.size());
    for (size_t i = 0; i < records.size(); i++)
        funcs[i] = records[i].func;
    NrdHipExecutor::CachedGraph* hit = nullptr;
    for (auto& g : e->graphs)
        if (g.funcs == funcs)
            hit = &g;
    std::vector<void*> argPtrs;
    auto paramsOf = [&](LaunchRecord& r) {
        argPtrs.resize(r.offsets.size());
        for (size_t k = 0; k < r.offsets.size(); k++)
            argPtrs[k] = r.args.data() + r.offsets[k];
        hipKernelNodeParams p = {};
        p.func = (void*)r.func;
        p.gridDim = r.grid;
        p.blockDim = r.block;
        p.sharedMemBytes = 0;
        p.kernelParams = argPtrs.data();
        p.extra = nullptr;
        return p;
    };
    if (!hit) {
        if (e->graphs.size() >= 32) { // evict the least recently used topology (a sharded frame is launched as up to ~10 dispatch ranges, each its own topology)
            size_t lru = 0;
            for (size_t i = 1; i < e->graphs.size(); i++)
                if (e->graphs[i].lastUse < e->graphs[lru].lastUse)
                    lru = i;
            // its last launch may still be in flight on the stream: wait before the executable graph goes away (evictions are rare -- 32 topologies)
            (void)hipStreamSynchronize(e->stream);
            (void)hipGraphExecDestroy(e->graphs[lru].exec);
            (void)hipGraphDestroy(e->graphs[lru].graph);
            e->graphs.erase(e->graphs.begin() + (long)lru);
        }
        NrdHipExecutor::CachedGraph g;
        g.funcs = funcs;
        if (hipGraphCreate(&g.graph, 0) != hipSuccess)
            return e->Fail(nrd::Result::FAILURE, "hipGraphCreate failed");
        g.nodes.resize(records.size());
        for (size_t i = 0; i < records.size(); i++) {
            hipKernelNodeParams p = paramsOf(records[i]);
            hipError_t err = hipGraphAddKernelNode(&g.nodes[i], g.graph, i ? &g.nodes[i - 1] : nullptr, i ? 1 : 0, &p);
            if (err != hipSuccess) {
                (void)hipGraphDestroy(g.graph);
                return e->Fail(nrd::Result::FAILURE, std::string("hipGraphAddKernelNode failed: ") + hipGetErrorString(err));
            }
        }
        hipError_t err = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (err != hipSuccess) {
            (void)hipGraphDestroy(g.graph);
            return e->Fail(nrd::Result::FAILURE, std::string("hipGraphInstantiate failed: ") + hipGetErrorString(err));
        }
        g.records = records;
        e->graphs.push_back(std::move(g));
        hit = &e->graphs.back();
        e->graphBuilds++;
    } else {
        for (size_t i = 0; i < records.size(); i++) {
            LaunchRecord& have = hit->records[i];
            LaunchRecord& want = records[i];
            const bool same = have.args == want.args && have.grid.x == want.grid.x && have.grid.y == want.grid.y && have.grid.z == want.grid.z && have.block.x == want.block.x &&
                              have.block.y == want.block.y && have.block.z == want.block.z;
            if (same)
                continue;
            hipKernelNodeParams p = paramsOf(want);
            hipError_t err = hipGraphExecKernelNodeSetParams(hit->exec, hit->nodes[i], &p);
            if (err != hipSuccess)
                return e->Fail(nrd::Result::FAILURE, std::string("hipGraphExecKernelNodeSetParams failed: ") + hipGetErrorString(err));
            have = want;
            e->graphNodeUpdates++;
        }
    }
    hit->lastUse = ++e->graphClock;
    hipError_t err = hipGraphLaunch(hit->exec, e->stream);
    if (err != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, std::string("hipGraphLaunch failed: ") + hipGetErrorString(err));
    e->graphLaunches++;
    return (uint32_t)nrd::Result::SUCCESS;
}

static uint32_t ExecuteRange(NrdHipExecutor* e, const nrd::DispatchDesc* descs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count, const int32_t* rowBegin, const int32_t* rowEnd) {
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*e->instance);
    // ---- shifted rect: rect-at-origin copies of the guide inputs this list binds (kernels_common.hip "shifted rect")
    e->originX = e->originY = 0;
    for (uint32_t i = 0; i < dispatchDescsNum; i++) {
        size_t oo, of;
        if (descs[i].pipelineIndex < idesc.pipelinesNum && descs[i].constantBufferData &&
            RectOriginOffsets(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, descs[i].constantBufferDataSize, oo, of)) {
            const uint32_t* o = (const uint32_t*)((const uint8_t*)descs[i].constantBufferData + oo);
            e->originX = (int)o[0], e->originY = (int)o[1];
            break;
        }
    }
    const bool shiftedRect = e->originX != 0 || e->originY != 0;
    std::vector<uint32_t> shiftTypes; // guide slots of this list that get a rect-at-origin twin
    bool writesMv = false;
    if (shiftedRect) {
        for (uint32_t i = 0; i < dispatchDescsNum; i++)
            for (uint32_t r = 0; r < descs[i].resourcesNum; r++) {
                const nrd::ResourceDesc& res = descs[i].resources[r];
                const uint32_t t = (uint32_t)res.type;
                if (!IsGuideInput(res.type) || t >= (uint32_t)nrd::ResourceType::MAX_NUM || !e->userBound[t])
                    continue;
                writesMv = writesMv || (res.type == nrd::ResourceType::IN_MV && res.descriptorType == nrd::DescriptorType::STORAGE_TEXTURE);
                bool known = false;
                for (uint32_t k : shiftTypes)
                    known = known || k == t;
                if (known)
                    continue;
                if (e->originX >= e->user[t].w || e->originY >= e->user[t].h)
                    return e->Fail(nrd::Result::INVALID_ARGUMENT, "CommonSettings::rectOrigin lies outside the bound planes; nothing was launched");
                Plane& twin = e->shifted[t];
                const Plane& src = e->user[t];
                if (!twin.ptr || twin.w != src.w || twin.h != src.h || twin.pitch != src.pitch) {
                    if (twin.ptr)
                        (void)hipFree(twin.ptr);
                    twin = src;
                    twin.ptr = nullptr;
                    if (hipMalloc((void**)&twin.ptr, (size_t)twin.pitch * (size_t)twin.h) != hipSuccess)
                        return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate a shifted-rect guide plane");
                    // cleared at once (a pre-flight failure further down used to leave the new twin uninitialised for the next call); a memset of
                    // a private buffer enqueues no pass work, so "nothing is launched before the pre-flight has passed" still holds
                    (void)hipMemsetAsync(twin.ptr, 0, (size_t)twin.pitch * (size_t)twin.h, e->stream);
                    e->decodedFresh = false;
                }
                shiftTypes.push_back(t);
            }
    }
    auto guidePlane = [&](nrd::ResourceType t) -> const Plane& { return shiftedRect && e->shifted[(uint32_t)t].ptr ? e->shifted[(uint32_t)t] : e->user[(uint32_t)t]; };

    // Guide planes: if any dispatch reads IN_NORMAL_ROUGHNESS, the bound plane is decoded once for the whole list -- into the planes of the families the list holds (below).
    // `decoded` = their common geometry (float4 texels at the packed plane's size); its ptr -- the float4 (normal, roughness | material) cache -- is set for RELAX lists only,
    // the one family that reads it (REBLUR- and SIGMA-only executors used to hold a dead 16 B/px plane: 59 MB at 1440p)
    Plane decoded = {};
    bool decodeNow = false, usesNormalRoughness = false;
    {
        const uint32_t slot = (uint32_t)nrd::ResourceType::IN_NORMAL_ROUGHNESS;
        bool used = false;
        for (uint32_t i = 0; i < dispatchDescsNum && !used; i++)
            for (uint32_t r = 0; r < descs[i].resourcesNum && !used; r++)
                used = descs[i].resources[r].type == nrd::ResourceType::IN_NORMAL_ROUGHNESS && descs[i].resources[r].descriptorType == nrd::DescriptorType::TEXTURE;
        if (used && e->userBound[slot]) {
            const Plane& packed = e->user[slot];
            usesNormalRoughness = true;
            decoded.pitch = ((uint32_t)packed.w * 16u + 255u) & ~255u;
            decoded.w = packed.w;
            decoded.h = packed.h;
            // first == 0 starts a new list (= a new frame); a later range decodes only if nothing valid is there (rebound plane, new cache,
            // or a caller that skipped the first range)
            decodeNow = first == 0 || !e->decodedFresh;
        }
    }
    // View-position guide plane of the REBLUR lists (same geometry again): needs IN_VIEWZ and the frame's REBLUR constants
    Plane viewPos = {};
    const void* reblurConstants = nullptr;
    if (usesNormalRoughness) {
        for (uint32_t i = 0; i < dispatchDescsNum && !reblurConstants; i++)
            if (descs[i].pipelineIndex < idesc.pipelinesNum && !strncmp(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, "REBLUR_", 7) && descs[i].constantBufferData &&
                descs[i].constantBufferDataSize >= sizeof(nrdc::ReblurConstants))
                reblurConstants = descs[i].constantBufferData;
        const Plane& z = e->user[(uint32_t)nrd::ResourceType::IN_VIEWZ];
        if (reblurConstants) { // the REBLUR kernels read normal + roughness from this pair only (reblur_device.h NormalRoughnessGuide): it has to exist
            if (!e->userBound[(uint32_t)nrd::ResourceType::IN_VIEWZ])
                return e->Fail(nrd::Result::INVALID_ARGUMENT, "resource not bound: IN_VIEWZ; nothing was launched");
            if (z.w != decoded.w || z.h != decoded.h)
                return e->Fail(nrd::Result::INVALID_ARGUMENT, "IN_VIEWZ and IN_NORMAL_ROUGHNESS differ in size; nothing was launched");
            Plane& cache = e->viewPos;
            if (!cache.ptr || cache.w != decoded.w || cache.h != decoded.h) {
                if (cache.ptr)
                    (void)hipFree(cache.ptr);
                cache = decoded;
                cache.ptr = nullptr;
                if (hipMalloc((void**)&cache.ptr, (size_t)cache.pitch * (size_t)cache.h) != hipSuccess)
                    return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate the view-position guide plane");
                // its companion, a quarter of the size: the w word of the decoded normals alone (same texel grid, a quarter of the pitch)
                Plane& word = e->roughnessWord;
                if (word.ptr)
                    (void)hipFree(word.ptr);
                word = decoded;
                word.ptr = nullptr;
                word.pitch = decoded.pitch / 4u;
                if (hipMalloc((void**)&word.ptr, (size_t)word.pitch * (size_t)word.h) != hipSuccess) {
                    (void)hipFree(cache.ptr); // the two live and die together: a later call starts over
                    cache = Plane{};
                    word = Plane{};
                    return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate the roughness-word guide plane");
                }
                e->decodedFresh = false;
                decodeNow = true;
            }
            viewPos = cache;
        }
    }
    // World-position guide plane of the RELAX lists (same geometry): IN_VIEWZ and the frame's RELAX constants. Independent of the REBLUR plane: one
    // dispatch list may hold both families (e.g. REBLUR_DIFFUSE + RELAX_SPECULAR in one instance), and then both guide planes are written
    Plane worldPos = {};
    const void* relaxConstants = nullptr;
    if (usesNormalRoughness) {
        for (uint32_t i = 0; i < dispatchDescsNum && !relaxConstants; i++)
            if (descs[i].pipelineIndex < idesc.pipelinesNum && !strncmp(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, "RELAX_", 6) && descs[i].constantBufferData &&
                descs[i].constantBufferDataSize >= sizeof(nrdc::RelaxConstants))
                relaxConstants = descs[i].constantBufferData;
        if (relaxConstants) {
            if (!e->userBound[(uint32_t)nrd::ResourceType::IN_VIEWZ])
                return e->Fail(nrd::Result::INVALID_ARGUMENT, "resource not bound: IN_VIEWZ; nothing was launched");
            const Plane& z = e->user[(uint32_t)nrd::ResourceType::IN_VIEWZ];
            if (z.w != decoded.w || z.h != decoded.h)
                return e->Fail(nrd::Result::INVALID_ARGUMENT, "IN_VIEWZ and IN_NORMAL_ROUGHNESS differ in size; nothing was launched");
            Plane& nr = e->decodedNormalRoughness; // the float4 (normal, roughness | material) plane: RELAX lists only
            if (!nr.ptr || nr.w != decoded.w || nr.h != decoded.h) {
                if (nr.ptr)
                    (void)hipFree(nr.ptr);
                nr = decoded;
                nr.ptr = nullptr;
                if (hipMalloc((void**)&nr.ptr, (size_t)nr.pitch * (size_t)nr.h) != hipSuccess) {
                    nr = Plane{};
                    return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate the decoded normal/roughness cache");
                }
                e->decodedFresh = false;
                decodeNow = true;
            }
            decoded.ptr = nr.ptr;
            Plane& cache = e->worldPosViewZ;
            if (!cache.ptr || cache.w != decoded.w || cache.h != decoded.h) {
                if (cache.ptr)
                    (void)hipFree(cache.ptr);
                cache = decoded;
                cache.ptr = nullptr;
                if (hipMalloc((void**)&cache.ptr, (size_t)cache.pitch * (size_t)cache.h) != hipSuccess)
                    return e->Fail(nrd::Result::FAILURE, "nrdHipExecuteDispatches: cannot allocate the world-position guide plane");
                e->decodedFresh = false;
                decodeNow = true;
            }
            worldPos = cache;
        }
    }
    // once per list, in front of its first pass: the rect-at-origin twins of the guide inputs (shifted rect only), then the decoded guides
    const bool prepareNow = decodeNow || (shiftedRect && (first == 0 || !e->decodedFresh));
    auto shiftGuides = [&](LaunchRecorder* rec, bool back) {
        PassArgs args = {};
        args.stream = e->stream;
        args.recorder = rec;
        for (uint32_t t : shiftTypes)
            if (!back || t == (uint32_t)nrd::ResourceType::IN_MV)
                LaunchShiftPlane(args, e->user[t], e->shifted[t], e->originX, e->originY, BytesPerTexel(ExpectedUserFormat((nrd::ResourceType)t, e->translucentShadow)), back);
    };
    // multi-GPU: the guide planes are needed on the rows the passes of this rank read them at -- every dispatch's rows widened by its guide reach, rounded out to the
    // 16-row tile grid; the rest of the planes keeps whatever it held (nothing of this list reads it). Whole frame when any dispatch runs on the whole frame.
    int guideRow0 = 0, guideRow1 = INT_MAX;
    if (rowBegin && rowEnd && decodeNow) {
        int lo = INT_MAX, hi = 0;
        bool whole = dispatchDescsNum == 0;
        for (uint32_t i = 0; i < dispatchDescsNum && !whole; i++) {
            bool readsGuides = false; // the guide planes stand in for IN_NORMAL_ROUGHNESS (and IN_VIEWZ next to it): a pass that does not bind it (tile classification) reads none of them
            for (uint32_t r = 0; r < descs[i].resourcesNum && !readsGuides; r++)
                readsGuides = descs[i].resources[r].type == nrd::ResourceType::IN_NORMAL_ROUGHNESS;
            if (!readsGuides)
                continue;
            const int reach = descs[i].pipelineIndex < idesc.pipelinesNum ? GuideReachRows(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, descs[i].constantBufferData, descs[i].constantBufferDataSize) : -1;
            whole = rowBegin[i] < 0 || reach < 0;
            if (!whole) {
                lo = std::min(lo, (int)rowBegin[i] - reach);
                hi = std::max(hi, (int)rowEnd[i] + reach);
            }
        }
        if (!whole && hi > lo) {
            guideRow0 = std::max(lo, 0) & ~15;
            guideRow1 = (hi + 15) & ~15;
        }
        static const bool trace = getenv("NRD_HIP_TRACE_GUIDE_ROWS") != nullptr; // debugging aid of the sharding tests
        if (trace)
            fprintf(stderr, "[nrdhip] guide planes decoded on rows [%d, %d) of %d\n", guideRow0, guideRow1 == INT_MAX ? (int)e->height : std::min(guideRow1, (int)e->height), (int)e->height);
    }
    // Whole-frame decode of a single-family list that starts (behind its clears, if any) with that family's tile classification: the classification kernel writes the guide
    // planes too (kernels_common.hip DecodeGuidesClassifyKernel) and no decode kernel is launched here. Not with a shifted rect (the twins are prepared first), not
    // under row sharding (the strips decode only their rows), not with both families in one list. NRD_HIP_FUSE_CLASSIFY=0: the two separate kernels (A/B switch).
    uint32_t fuseDispatch = UINT32_MAX;
    static const bool fuseClassify = !(getenv("NRD_HIP_FUSE_CLASSIFY") && atoi(getenv("NRD_HIP_FUSE_CLASSIFY")) == 0);
    if (fuseClassify && decodeNow && !shiftedRect && !rowBegin && (viewPos.ptr != nullptr) != (worldPos.ptr != nullptr)) {
        const char* classify = viewPos.ptr ? "REBLUR_ClassifyTiles.cs" : "RELAX_ClassifyTiles.cs";
        for (uint32_t i = first; i < first + count; i++) {
            const char* shader = descs[i].pipelineIndex < idesc.pipelinesNum ? idesc.pipelines[descs[i].pipelineIndex].shaderFileName : "";
            if (!strncmp(shader, "Clear_", 6))
                continue;
            if (!strcmp(shader, classify) && descs[i].constantBufferData && descs[i].constantBufferDataSize >= (viewPos.ptr ? sizeof(nrdc::ReblurConstants) : sizeof(nrdc::RelaxConstants)))
                fuseDispatch = i;
            break;
        }
        static const bool trace = getenv("NRD_HIP_TRACE_GUIDE_ROWS") != nullptr;
        if (trace && fuseDispatch != UINT32_MAX)
            fprintf(stderr, "[nrdhip] guide planes written by the tile classification kernel (dispatch %u)\n", fuseDispatch);
    }
    auto decode = [&](LaunchRecorder* rec) {
        if (shiftedRect)
            shiftGuides(rec, false);
        if (!decodeNow || fuseDispatch != UINT32_MAX)
            return;
        PassArgs args = {};
        args.stream = e->stream;
        args.recorder = rec;
        args.rowBegin = guideRow0;
        args.rowEnd = guideRow1;
        // RELAX: float4 (normal, roughness | material) + float4 (world position, viewZ); REBLUR: float4 (normal, viewZ) + the roughness | material word. A list with
        // both families gets both sets; a list with neither (SIGMA, REFERENCE: they read the packed plane themselves) gets none
        if (worldPos.ptr)
            LaunchDecodeGuidesRelax(args, guidePlane(nrd::ResourceType::IN_NORMAL_ROUGHNESS), guidePlane(nrd::ResourceType::IN_VIEWZ), decoded, worldPos, relaxConstants);
        if (viewPos.ptr)
            LaunchDecodeGuides(args, guidePlane(nrd::ResourceType::IN_NORMAL_ROUGHNESS), guidePlane(nrd::ResourceType::IN_VIEWZ), viewPos, e->roughnessWord, reblurConstants);
    };
    // a pass of the list rewrites IN_MV (REBLUR specular MV modification): the twin goes back into the user's plane behind the last pass
    const bool shiftBackMv = shiftedRect && writesMv && first + count == dispatchDescsNum;

    auto passName = [&](const nrd::DispatchDesc& d) {
        return std::string("'") + (d.name ? d.name : "?") + "' (" + (d.pipelineIndex < idesc.pipelinesNum ? idesc.pipelines[d.pipelineIndex].shaderFileName : "?") + ")";
    };
    e->patchedConstants.assign(shiftedRect ? count : 0, std::vector<uint8_t>());
    auto fill = [&](uint32_t i, PassArgs& args, std::string& msg) -> const char* {
        const char* err = PrepareDispatch(e, descs[i], args, msg);
        size_t oo, of;
        if (shiftedRect && !err && descs[i].constantBufferData && RectOriginOffsets(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, descs[i].constantBufferDataSize, oo, of)) {
            // the passes run on rect-at-origin guides: they must see rectOrigin = rectOffset = 0
            std::vector<uint8_t>& copy = e->patchedConstants[i - first];
            copy.assign((const uint8_t*)descs[i].constantBufferData, (const uint8_t*)descs[i].constantBufferData + descs[i].constantBufferDataSize);
            memset(copy.data() + oo, 0, 8);
            memset(copy.data() + of, 0, 8);
            args.constants = copy.data();
        }
        args.rowBegin = 0;
        args.rowEnd = INT_MAX;
        args.decodedNormalRoughness = decoded;
        args.worldPosViewZ = worldPos;
        args.viewPos = viewPos;
        args.roughnessWord = viewPos.ptr ? e->roughnessWord : Plane{};
        args.tileFlags = e->tileFlags;
        args.historyReachWord = e->historyReachWord;
        args.windowRegion = e->windowRegion;
        if (i == fuseDispatch)
            args.fuseGuidesFrom = guidePlane(nrd::ResourceType::IN_NORMAL_ROUGHNESS);
        if (rowBegin && rowBegin[i] >= 0) {
            args.rowBegin = rowBegin[i];
            args.rowEnd = rowEnd[i];
        }
        return err;
    };

    // ---- pre-flight: every pass of the range must have a launcher, bound resources and pass its own support checks BEFORE anything is enqueued
    // (the reference integration's contract: a Denoise call either runs completely or not at all). The same walk records every launch (kernel, grid,
    // arguments); the records are then either turned into / matched against a graph or launched one by one -- the launchers run once per frame.
    const bool useGraph = e->graphMode && !e->profiling;
    LaunchRecorder recorder;
    recorder.keep = true;
    if (prepareNow)
        decode(&recorder);
    const uint32_t prepareRecords = (uint32_t)recorder.records.size(); // shift / decode kernels in front of the first pass
    std::vector<uint32_t> recordEnd(count); // records [recordEnd[k-1], recordEnd[k]) belong to pass first + k
    for (uint32_t i = first; i < first + count; i++) {
        const nrd::DispatchDesc& d = descs[i];
        if (d.pipelineIndex >= e->launchers.size())
            return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipExecuteDispatches: pipeline index out of range");
        PassLauncher launch = e->launchers[d.pipelineIndex];
        if (!launch)
            return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipExecuteDispatches: no HIP kernel for pass " + passName(d) + "; nothing was launched");
        if (d.constantBufferDataSize && !d.constantBufferData)
            return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipExecuteDispatches: pass " + passName(d) + " has no constant data (constant arena overflow?); nothing was launched");
        PassArgs args = {};
        std::string msg;
        if (const char* err = fill(i, args, msg))
            return e->Fail(nrd::Result::INVALID_ARGUMENT, std::string(err) + " in pass " + passName(d) + "; nothing was launched");
        args.recorder = &recorder;
        if (const char* err = launch(args))
            return e->Fail(nrd::Result::UNSUPPORTED, std::string(err) + " [pass " + passName(d) + "; nothing was launched]");
        recordEnd[i - first] = (uint32_t)recorder.records.size();
    }
    const uint32_t passRecordsEnd = (uint32_t)recorder.records.size();
    if (shiftBackMv)
        shiftGuides(&recorder, true);

    // ---- from here on work is enqueued
    if (useGraph) {
        uint32_t r = LaunchAsGraph(e, recorder.records);
        if (r != (uint32_t)nrd::Result::SUCCESS)
            return r;
    } else {
        auto enqueue = [&](uint32_t begin, uint32_t end) -> hipError_t {
            for (uint32_t k = begin; k < end; k++)
                recorder.records[k].launch(recorder.records[k], e->stream);
            return hipGetLastError(); // launch-configuration errors surface here (no synchronisation)
        };
        {   // outside the timing bracket of the first pass; profiled as a row of its own (pipeline index == number of pipelines: include/NRDHip.h nrdHipCollectPassTimings)
            NrdHipExecutor::Bracket bracket = {};
            const bool timed = e->profiling && prepareRecords > 0;
            if (timed) {
                bracket.start = AcquireEvent(e);
                bracket.stop = AcquireEvent(e);
                bracket.pipelineIndex = (uint32_t)e->launchers.size();
                (void)hipEventRecord(bracket.start, e->stream);
            }
            const hipError_t prepareError = enqueue(0, prepareRecords);
            if (timed) {
                (void)hipEventRecord(bracket.stop, e->stream);
                e->brackets.push_back(bracket);
            }
            if (prepareError != hipSuccess)
                return e->Fail(nrd::Result::FAILURE, "HIP launch failed while preparing the guide planes");
        }
        for (uint32_t i = first; i < first + count; i++) {
            const nrd::DispatchDesc& d = descs[i];
            const uint32_t from = i == first ? prepareRecords : recordEnd[i - first - 1];
            NrdHipExecutor::Bracket bracket = {};
            if (e->profiling) {
                bracket.start = AcquireEvent(e);
                bracket.stop = AcquireEvent(e);
                bracket.pipelineIndex = d.pipelineIndex;
                (void)hipEventRecord(bracket.start, e->stream);
            }
            hipError_t launchError = enqueue(from, recordEnd[i - first]);
            if (e->profiling) {
                (void)hipEventRecord(bracket.stop, e->stream);
                e->brackets.push_back(bracket);
            }
            if (launchError != hipSuccess)
                return e->Fail(nrd::Result::FAILURE, "HIP launch failed in pass " + passName(d) + ": " + hipGetErrorString(launchError));
        }
        if (enqueue(passRecordsEnd, (uint32_t)recorder.records.size()) != hipSuccess) // the IN_MV twin back into the user's plane
            return e->Fail(nrd::Result::FAILURE, "HIP launch failed while copying IN_MV back");
    }
    if (usesNormalRoughness || shiftedRect)
        e->decodedFresh = first + count < dispatchDescsNum; // the list is complete: the next call belongs to another frame

    hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, std::string("HIP launch failed: ") + hipGetErrorString(err));
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetTileFallbackStats(NrdHipExecutor* e, uint32_t* fallbackTiles, uint32_t* totalTiles) {
    if (!e || !e->tileFlags.ptr)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    std::vector<uint8_t> host((size_t)e->tileFlags.pitch * (size_t)e->tileFlags.h);
    if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(host.data(), e->tileFlags.ptr, host.size(), hipMemcpyDeviceToHost) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipGetTileFallbackStats: cannot read the tile flags back");
    // only the region the last window kernel covered holds flags of that frame: the rect's tile columns, this rank's tile rows
    const int cols = e->windowRegion[0] < e->tileFlags.w ? e->windowRegion[0] : e->tileFlags.w, rowBegin = e->windowRegion[1], rowEnd = e->windowRegion[2] < e->tileFlags.h ? e->windowRegion[2] : e->tileFlags.h;
    uint32_t n = 0, total = 0;
    for (int y = rowBegin; y < rowEnd; y++)
        for (int x = 0; x < cols; x++) {
            n += host[(size_t)y * e->tileFlags.pitch + (size_t)x] == 1 ? 1u : 0u;
            total++;
        }
    if (fallbackTiles)
        *fallbackTiles = n;
    if (totalTiles)
        *totalTiles = total;
    return (uint32_t)nrd::Result::SUCCESS;
}

// Multi-GPU: how far does THIS frame's surface-motion reprojection reach vertically, over the rows [rowBegin, rowEnd) of the rect? (include/NRDHip.h)
// the measurement enqueued on the executor's stream: deviceWord (4 bytes of device memory) receives the float's bits when the stream gets there; found = false: the list has no
// temporal denoiser and nothing was enqueued
static uint32_t EnqueueMotionRows(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd, uint32_t* deviceWord, bool& found);

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipMeasureMotionRows(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd,
    float* maxRows) {
    if (!e || !maxRows || (!dispatchDescs && dispatchDescsNum))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    *maxRows = 0.0f;
    if (!e->motionBits && hipMalloc((void**)&e->motionBits, sizeof(uint32_t)) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipMeasureMotionRows: cannot allocate the result word");
    bool found = false;
    const uint32_t r = EnqueueMotionRows(e, dispatchDescs, dispatchDescsNum, rowBegin, rowEnd, e->motionBits, found);
    if (r != (uint32_t)nrd::Result::SUCCESS || !found)
        return r;
    uint32_t bits = 0;
    if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&bits, e->motionBits, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipMeasureMotionRows: cannot read the result back");
    memcpy(maxRows, &bits, sizeof(bits));
    return (uint32_t)nrd::Result::SUCCESS;
}

// The same measurement WITHOUT the host round trip (round 6): the result lands in 4 bytes of the CALLER'S device memory, in stream order. A multi-GPU host
// hands that word straight to its MAX all-reduce (RCCL reads it on the device) and synchronises once, on the reduced value -- instead of stream-synchronise, read back, upload,
// reduce, read back. 0.0f is written when the list has no temporal denoiser.
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipMeasureMotionRowsAsync(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd,
    void* deviceMaxRows) {
    if (!e || !deviceMaxRows || (!dispatchDescs && dispatchDescsNum))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    bool found = false;
    const uint32_t r = EnqueueMotionRows(e, dispatchDescs, dispatchDescsNum, rowBegin, rowEnd, (uint32_t*)deviceMaxRows, found);
    if (r == (uint32_t)nrd::Result::SUCCESS && !found && hipMemsetAsync(deviceMaxRows, 0, sizeof(uint32_t), e->stream) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipMeasureMotionRowsAsync: hipMemsetAsync failed");
    return r;
}

static uint32_t EnqueueMotionRows(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd, uint32_t* deviceWord, bool& found) {
    found = false;
    const nrd::DispatchDesc* descs = (const nrd::DispatchDesc*)dispatchDescs;
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*e->instance);
    MotionParams p = {};
    int originX = 0, originY = 0;
    for (uint32_t i = 0; i < dispatchDescsNum && !found; i++) {
        const nrd::DispatchDesc& d = descs[i];
        if (d.pipelineIndex >= idesc.pipelinesNum || !d.constantBufferData)
            continue;
        const char* shader = idesc.pipelines[d.pipelineIndex].shaderFileName;
        auto common = [&](const auto& c) {
            memcpy(p.worldToClipPrev, c.gWorldToClipPrev, sizeof(p.worldToClipPrev));
            const float mvScale[4] = {c.gMvScale.x, c.gMvScale.y, c.gMvScale.z, c.gMvScale.w};
            memcpy(p.mvScale, mvScale, sizeof(mvScale));
            p.rectSizeInv[0] = c.gRectSizeInv.x, p.rectSizeInv[1] = c.gRectSizeInv.y;
            p.rectHeightPrev = c.gRectSizePrev.y;
            p.viewZScale = c.gViewZScale, p.denoisingRange = c.gDenoisingRange;
            p.rectW = (int)c.gRectSize.x, p.rectH = (int)c.gRectSize.y;
            originX = (int)c.gRectOrigin.x, originY = (int)c.gRectOrigin.y;
            found = true;
        };
        auto frustum = [&](const auto& c) {
            const float f[4] = {c.gFrustum.x, c.gFrustum.y, c.gFrustum.z, c.gFrustum.w};
            memcpy(p.frustum, f, sizeof(f));
        };
        if (!strncmp(shader, "REBLUR_", 7) && d.constantBufferDataSize >= sizeof(nrdc::ReblurConstants)) {
            nrdc::ReblurConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
            frustum(c);
            memcpy(p.viewToWorld, c.gViewToWorld, sizeof(p.viewToWorld));
        } else if (!strncmp(shader, "RELAX_", 6) && d.constantBufferDataSize >= sizeof(nrdc::RelaxConstants)) {
            nrdc::RelaxConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
            p.relaxForm = 1;
            const float r[4] = {c.gFrustumRight.x, c.gFrustumRight.y, c.gFrustumRight.z, 0.0f}, u[4] = {c.gFrustumUp.x, c.gFrustumUp.y, c.gFrustumUp.z, 0.0f},
                        f[4] = {c.gFrustumForward.x, c.gFrustumForward.y, c.gFrustumForward.z, 0.0f};
            memcpy(p.frustumRight, r, sizeof(r));
            memcpy(p.frustumUp, u, sizeof(u));
            memcpy(p.frustumForward, f, sizeof(f));
        } else if (!strncmp(shader, "SIGMA_", 6) && d.constantBufferDataSize >= sizeof(nrdc::SigmaConstants)) {
            nrdc::SigmaConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
            frustum(c);
            for (int r = 0; r < 3; r++) // view -> world = the transposed rotation of gWorldToView (column-major storage)
                for (int k = 0; k < 3; k++)
                    p.viewToWorld[k * 4 + r] = c.gWorldToView[r * 4 + k];
        }
    }
    if (!found)
        return (uint32_t)nrd::Result::SUCCESS; // no temporal denoiser in the list (REFERENCE, empty list): nothing reprojects
    const uint32_t tz = (uint32_t)nrd::ResourceType::IN_VIEWZ, tm = (uint32_t)nrd::ResourceType::IN_MV;
    if (!e->userBound[tz] || !e->userBound[tm])
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipMeasureMotionRows: IN_VIEWZ and IN_MV have to be bound");
    Plane z = e->user[tz], mv = e->user[tm];
    if (originX + p.rectW > z.w || originY + p.rectH > z.h || originX + p.rectW > mv.w || originY + p.rectH > mv.h)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipMeasureMotionRows: the rect leaves the bound IN_VIEWZ / IN_MV planes");
    z.ptr += (size_t)originY * z.pitch + (size_t)originX * 4;
    mv.ptr += (size_t)originY * mv.pitch + (size_t)originX * 8;
    const int r0 = (int)(rowBegin < (uint32_t)p.rectH ? rowBegin : (uint32_t)p.rectH), r1 = (int)(rowEnd < (uint32_t)p.rectH ? rowEnd : (uint32_t)p.rectH);
    if (hipMemsetAsync(deviceWord, 0, sizeof(uint32_t), e->stream) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipMeasureMotionRows: hipMemsetAsync failed");
    LaunchMotionRows(e->stream, z, mv, p, r0, r1, deviceWord);
    return (uint32_t)nrd::Result::SUCCESS;
}

// ---- nrdHipCheckInputs (include/NRDHip.h): the bound inputs of THIS frame's list against NRD's input rules, in one launch of kernels_check_inputs.hip -----------------------
static const char* const kInputRuleNames[NRD_HIP_INPUT_RULES_NUM] = {"VIEWZ_NOT_FINITE", "MV_NOT_FINITE", "DIFF_NOT_FINITE", "SPEC_NOT_FINITE", "DIFF_HITDIST_RANGE", "SPEC_HITDIST_RANGE",
    "PENUMBRA_INVALID", "SIGNAL_NOT_FINITE"};

extern "C" __attribute__((visibility("default"))) const char* nrdHipGetInputRuleString(uint32_t rule) { return rule < NRD_HIP_INPUT_RULES_NUM ? kInputRuleNames[rule] : nullptr; }

static bool IsFloatFormat(nrd::Format f) {
    using F = nrd::Format;
    return f == F::R16_SFLOAT || f == F::RG16_SFLOAT || f == F::RGBA16_SFLOAT || f == F::R32_SFLOAT || f == F::RG32_SFLOAT || f == F::RGB32_SFLOAT || f == F::RGBA32_SFLOAT;
}

// Validates everything, then (enqueue) clears deviceReport and launches the audit on the executor's stream. mask = the rules that apply, whether enqueued or not; launched = false:
// no rule applies and only the clearing was enqueued.
static uint32_t EnqueueCheckInputs(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t* deviceReport, uint32_t& mask) {
    using R = nrd::ResourceType;
    mask = 0;
    const nrd::DispatchDesc* descs = (const nrd::DispatchDesc*)dispatchDescs;
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*e->instance);
    CheckInputsParams p = {};
    p.viewZScale = 1.0f;
    p.diffCell = p.specCell = 2u;
    int originX = 0, originY = 0;
    bool haveConstants = false;
    bool named[(size_t)R::MAX_NUM] = {}, namedOutsideReblur[(size_t)R::MAX_NUM] = {};
    for (uint32_t i = 0; i < dispatchDescsNum; i++) {
        const nrd::DispatchDesc& d = descs[i];
        if (d.pipelineIndex >= idesc.pipelinesNum)
            continue;
        const char* shader = idesc.pipelines[d.pipelineIndex].shaderFileName;
        const bool reblur = !strncmp(shader, "REBLUR_", 7);
        for (uint32_t r = 0; r < d.resourcesNum; r++) {
            const uint32_t t = (uint32_t)d.resources[r].type;
            if (t < (uint32_t)R::MAX_NUM) {
                named[t] = true;
                namedOutsideReblur[t] = namedOutsideReblur[t] || !reblur;
            }
        }
        if (haveConstants || !d.constantBufferData)
            continue;
        // the frame's rect, range and checkerboard: the first constant block of a pass family (every block of a list carries the same CommonSettings)
        auto common = [&](const auto& c) {
            p.rectW = (int)c.gRectSize.x, p.rectH = (int)c.gRectSize.y;
            originX = (int)c.gRectOrigin.x, originY = (int)c.gRectOrigin.y;
            p.viewZScale = c.gViewZScale, p.denoisingRange = c.gDenoisingRange;
            p.frameIndex = c.gFrameIndex;
            haveConstants = true;
        };
        if (reblur && d.constantBufferDataSize >= sizeof(nrdc::ReblurConstants)) {
            nrdc::ReblurConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
            p.diffCell = c.gDiffCheckerboard, p.specCell = c.gSpecCheckerboard;
        } else if (!strncmp(shader, "RELAX_", 6) && d.constantBufferDataSize >= sizeof(nrdc::RelaxConstants)) {
            nrdc::RelaxConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
            p.viewZScale = 1.0f; // RELAX classifies its tiles by Abs( z ) > range (kernels_common.hip DecodeGuidesClassifyKernel)
            p.diffCell = c.gDiffCheckerboard, p.specCell = c.gSpecCheckerboard;
        } else if (!strncmp(shader, "SIGMA_", 6) && d.constantBufferDataSize >= sizeof(nrdc::SigmaConstants)) {
            nrdc::SigmaConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            common(c);
        } else if (!strcmp(shader, "REFERENCE_Copy.cs") && d.constantBufferDataSize >= sizeof(nrdc::ReferenceCopyConstants)) {
            // REFERENCE's blocks carry the rect as its inverse only: 1 / ( 1 / n ) rounds back to n for every 16-bit n. Its kernels address IN_SIGNAL at the pixel itself.
            nrdc::ReferenceCopyConstants c;
            memcpy(&c, d.constantBufferData, sizeof(c));
            p.rectW = (int)std::lround(1.0f / c.gRectSizeInv.x), p.rectH = (int)std::lround(1.0f / c.gRectSizeInv.y);
            haveConstants = true;
        }
    }
    auto applies = [&](R t) { return named[(size_t)t] && IsFloatFormat(ExpectedUserFormat(t, e->translucentShadow)); };
    const bool diffRadiance = applies(R::IN_DIFF_RADIANCE_HITDIST), diffSh = applies(R::IN_DIFF_SH0), specRadiance = applies(R::IN_SPEC_RADIANCE_HITDIST), specSh = applies(R::IN_SPEC_SH0);
    if (haveConstants) {
        mask |= applies(R::IN_VIEWZ) ? 1u << NRD_HIP_INPUT_RULE_VIEWZ_NOT_FINITE : 0u;
        mask |= applies(R::IN_MV) ? 1u << NRD_HIP_INPUT_RULE_MV_NOT_FINITE : 0u;
        mask |= (diffRadiance || diffSh || applies(R::IN_DIFF_SH1)) ? 1u << NRD_HIP_INPUT_RULE_DIFF_NOT_FINITE : 0u;
        mask |= (specRadiance || specSh || applies(R::IN_SPEC_SH1)) ? 1u << NRD_HIP_INPUT_RULE_SPEC_NOT_FINITE : 0u;
        mask |= (diffRadiance || diffSh) ? 1u << NRD_HIP_INPUT_RULE_DIFF_HITDIST_RANGE : 0u;
        mask |= (specRadiance || specSh) ? 1u << NRD_HIP_INPUT_RULE_SPEC_HITDIST_RANGE : 0u;
        mask |= applies(R::IN_PENUMBRA) ? 1u << NRD_HIP_INPUT_RULE_PENUMBRA_INVALID : 0u;
        mask |= applies(R::IN_SIGNAL) ? 1u << NRD_HIP_INPUT_RULE_SIGNAL_NOT_FINITE : 0u;
    }
    if ((diffRadiance && diffSh) || (specRadiance && specSh))
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipCheckInputs: the list reads a signal both as RADIANCE_HITDIST and as SH0 / SH1; check the denoisers one at a time");

    // the planes the kernel reads, each with the area it is addressed in: guides at rectOrigin + pixel, noisy planes at the pixel, a checkerboarded signal in the left half
    std::string problem;
    auto take = [&](Plane& dst, R t, bool needed, bool atOrigin, uint32_t cell) {
        if (!needed || !problem.empty())
            return;
        const char* name = nrd::GetResourceTypeString(t);
        if (!e->userBound[(size_t)t]) {
            problem = std::string("nrdHipCheckInputs: resource not bound: ") + (name ? name : "?");
            return;
        }
        dst = e->user[(size_t)t];
        const int ox = atOrigin ? originX : 0, oy = atOrigin ? originY : 0, w = cell != 2u ? (p.rectW + 1) / 2 : p.rectW;
        if (ox + w > dst.w || oy + p.rectH > dst.h) {
            problem = std::string("nrdHipCheckInputs: the rect leaves the bound plane ") + (name ? name : "?");
            return;
        }
        dst.ptr += (size_t)oy * dst.pitch + (size_t)ox * BytesPerTexel(ExpectedUserFormat(t, e->translucentShadow));
    };
    const uint32_t noisyRules = 1u << NRD_HIP_INPUT_RULE_DIFF_NOT_FINITE | 1u << NRD_HIP_INPUT_RULE_SPEC_NOT_FINITE | 1u << NRD_HIP_INPUT_RULE_DIFF_HITDIST_RANGE |
                                1u << NRD_HIP_INPUT_RULE_SPEC_HITDIST_RANGE | 1u << NRD_HIP_INPUT_RULE_PENUMBRA_INVALID;
    take(p.viewZ, R::IN_VIEWZ, (mask & (noisyRules | 1u << NRD_HIP_INPUT_RULE_VIEWZ_NOT_FINITE)) != 0u, true, 2u); // the range test of every noisy rule
    take(p.mv, R::IN_MV, (mask & 1u << NRD_HIP_INPUT_RULE_MV_NOT_FINITE) != 0u, true, 2u);
    take(p.diff0, diffSh ? R::IN_DIFF_SH0 : R::IN_DIFF_RADIANCE_HITDIST, diffRadiance || diffSh, false, p.diffCell);
    take(p.diff1, R::IN_DIFF_SH1, applies(R::IN_DIFF_SH1), false, p.diffCell);
    take(p.spec0, specSh ? R::IN_SPEC_SH0 : R::IN_SPEC_RADIANCE_HITDIST, specRadiance || specSh, false, p.specCell);
    take(p.spec1, R::IN_SPEC_SH1, applies(R::IN_SPEC_SH1), false, p.specCell);
    take(p.penumbra, R::IN_PENUMBRA, applies(R::IN_PENUMBRA), false, 2u);
    take(p.signal, R::IN_SIGNAL, applies(R::IN_SIGNAL), false, 2u);
    if (!problem.empty())
        return e->Fail(nrd::Result::INVALID_ARGUMENT, problem);
    if ((p.diff1.ptr && !p.diff0.ptr) || (p.spec1.ptr && !p.spec0.ptr))
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipCheckInputs: the list reads SH1 of a signal without its SH0");
    // the > 1 bound: a normalised hit distance, which is what a slot holds that only REBLUR passes read
    p.diffNormalized = !namedOutsideReblur[(size_t)(diffSh ? R::IN_DIFF_SH0 : R::IN_DIFF_RADIANCE_HITDIST)];
    p.specNormalized = !namedOutsideReblur[(size_t)(specSh ? R::IN_SPEC_SH0 : R::IN_SPEC_RADIANCE_HITDIST)];

    // { pixels 0, inRangePixels 0, count[] 0, first[] 0xFFFFFFFF }
    const size_t head = offsetof(NrdHipInputReport, first);
    if (hipMemsetAsync(deviceReport, 0, head, e->stream) != hipSuccess || hipMemsetAsync((uint8_t*)deviceReport + head, 0xFF, sizeof(NrdHipInputReport) - head, e->stream) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipCheckInputs: hipMemsetAsync failed");
    if (mask)
        LaunchCheckInputs(e->stream, p, deviceReport);
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCheckInputsAsync(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, void* deviceReport, uint32_t* rulesChecked) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (!deviceReport || !rulesChecked || (!dispatchDescs && dispatchDescsNum) || ((uintptr_t)deviceReport & 3u) != 0)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipCheckInputsAsync: a NULL or misaligned pointer");
    uint32_t mask = 0;
    const uint32_t r = EnqueueCheckInputs(e, dispatchDescs, dispatchDescsNum, (uint32_t*)deviceReport, mask);
    if (r == (uint32_t)nrd::Result::SUCCESS)
        *rulesChecked = mask;
    return r;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCheckInputs(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, NrdHipInputReport* report, uint32_t* rulesChecked) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (!report || !rulesChecked || (!dispatchDescs && dispatchDescsNum))
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipCheckInputs: a NULL pointer");
    if (!e->inputReport && hipMalloc((void**)&e->inputReport, sizeof(NrdHipInputReport)) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipCheckInputs: cannot allocate the device report");
    uint32_t mask = 0;
    const uint32_t r = EnqueueCheckInputs(e, dispatchDescs, dispatchDescsNum, e->inputReport, mask);
    if (r != (uint32_t)nrd::Result::SUCCESS)
        return r;
    NrdHipInputReport host;
    if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&host, e->inputReport, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess)
        return e->Fail(nrd::Result::FAILURE, "nrdHipCheckInputs: cannot read the report back");
    *report = host;
    *rulesChecked = mask;
    return (uint32_t)nrd::Result::SUCCESS;
}

// Multi-GPU: where the temporal passes report how far (rows) they read last frame's planes from a pixel's own row (include/NRDHip.h). The word belongs to the caller, who clears
// it (in stream order) before a frame and reads / all-reduces it after; nullptr switches the tracking off (the default: the kernels then skip it on a uniform branch).
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetHistoryReachWord(NrdHipExecutor* e, void* deviceWord) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->historyReachWord = (uint32_t*)deviceWord; // (graph mode: a kernel argument like any other -- the node parameters are updated when they change)
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipSetGraphMode(NrdHipExecutor* e, uint32_t enable) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    e->graphMode = enable != 0;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetGraphStats(const NrdHipExecutor* e, uint64_t* graphLaunches, uint64_t* graphBuilds, uint64_t* nodeUpdates) {
    if (!e)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (graphLaunches)
        *graphLaunches = e->graphLaunches;
    if (graphBuilds)
        *graphBuilds = e->graphBuilds;
    if (nodeUpdates)
        *nodeUpdates = e->graphNodeUpdates;
    return (uint32_t)nrd::Result::SUCCESS;
}

// always 0: the library has one arithmetic (DESIGN.md "Numerics"), bit-identical to the CPU oracle in device mode; kept for callers of the round-2 interface
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetNumericsMode(void) {
    return 0; // one library, one arithmetic (the value 1 named the "fast" build of round 2, which no longer exists)
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

namespace nrdhip {
void LaunchEvalNumerics(uint32_t op, const float* in1, const float* in2, float* out, uint32_t count, hipStream_t stream);
void LaunchCopyProbe(const void* src, void* dst, uint64_t bytes, hipStream_t stream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipMeasureCopyBandwidth(uint64_t bytes, uint32_t repetitions, void* hipStream, double* gigabytesPerSecond) {
    if (!gigabytesPerSecond || bytes < 16 || !repetitions)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)hipStream;
    bytes &= ~(uint64_t)15;
    void *src = nullptr, *dst = nullptr;
    if (hipMalloc(&src, bytes) != hipSuccess || hipMalloc(&dst, bytes) != hipSuccess) {
        (void)hipFree(src);
        return (uint32_t)nrd::Result::FAILURE;
    }
    (void)hipMemsetAsync(src, 1, bytes, stream);
    hipEvent_t t0, t1;
    (void)hipEventCreate(&t0);
    (void)hipEventCreate(&t1);
    for (int i = 0; i < 3; i++)
        nrdhip::LaunchCopyProbe(src, dst, bytes, stream);
    (void)hipEventRecord(t0, stream);
    for (uint32_t i = 0; i < repetitions; i++)
        nrdhip::LaunchCopyProbe(src, dst, bytes, stream);
    (void)hipEventRecord(t1, stream);
    const bool ok = hipStreamSynchronize(stream) == hipSuccess;
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, t0, t1);
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    (void)hipFree(src);
    (void)hipFree(dst);
    if (!ok || ms <= 0.0f)
        return (uint32_t)nrd::Result::FAILURE;
    *gigabytesPerSecond = 2.0 * (double)bytes * repetitions / ((double)ms * 1e-3) / 1e9;
    return (uint32_t)nrd::Result::SUCCESS;
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipEvalNumerics(uint32_t op, const float* in1, const float* in2, float* out, uint32_t count, void* hipStream) {
    if (!in1 || !out || op > 24)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (count)
        nrdhip::LaunchEvalNumerics(op, in1, in2, out, count, (hipStream_t)hipStream);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : (uint32_t)nrd::Result::FAILURE;
}
