// Internal to the HIP executor (executor.hip, executor_graph.hip, executor_queries.hip: DESIGN.md "Executor structure"): its state and the helpers its units share.
#pragma once

#include "NRD.h"
#include "NRDHip.h"

#include "passes.h"

#include "../host/dispatch_list.h"

#include <climits>
#include <string>
#include <vector>

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
    std::vector<nrdhip::Plane> permanent, transient;
    nrdhip::Plane decodedNormalRoughness = {}; // internal float4 cache of IN_NORMAL_ROUGHNESS (not an NRD pool plane; own allocation)
    nrdhip::Plane worldPosViewZ = {};          // internal float4 scratch of the RELAX a-trous chain (world position + viewZ per pixel)
    int windowRegion[3] = {0, 0, 0};   // {tile columns, first tile row, end tile row} of the last window-kernel launch (passes.h PassArgs::windowRegion)
    nrdhip::Plane tileFlags = {};              // one byte per 32x8-pixel workgroup tile: hand-over between the two kernels of a split pass (kernels_reblur_ta.hip "window")
    nrdhip::Plane viewPos = {};                // internal float4 guide plane of the REBLUR lists (decoded normal + viewZ per pixel)
    nrdhip::Plane roughnessWord = {};          // internal 4-B/px copy of the decoded normals' w word, written with viewPos (passes.h PassArgs::roughnessWord)
    uint32_t* historyReachWord = nullptr; // nrdHipSetHistoryReachWord: the CALLER'S device word the temporal passes report their history reach into (passes.h); null = not tracked
    uint32_t* motionBits = nullptr;    // nrdHipMeasureMotionRows: the reduction's result (float bits), own 4-byte allocation made on first use
    uint32_t* inputReport = nullptr;   // nrdHipCheckInputs: the device copy of the NrdHipInputReport, own allocation made on first use
    std::vector<nrd::Format> permanentFormat, transientFormat;
    // nrdHipCreateExecutorLayered: every pool plane exists layersNum times, layer l of plane i at permanent[i].ptr + l * permanentStride[i] (its 256-byte aligned size);
    // the per-layer user slots are stacks of planes userLayerBytes apart (nrdHipBindResourceLayers; 0 = a plain plane shared by all layers)
    uint32_t layersNum = 1;
    std::vector<uint64_t> permanentStride, transientStride;
    uint64_t userLayerBytes[nrdhip::kUserSlots] = {};
    std::vector<uint64_t> scratchLayerStrides;

    nrdhip::Plane user[nrdhip::kUserSlots] = {};
    bool userBound[nrdhip::kUserSlots] = {};
    // CommonSettings::rectOrigin != 0: rect-at-origin copies of the guide inputs (kernels_common.hip "shifted rect"); own allocations, made on demand
    nrdhip::Plane shifted[nrdhip::kUserSlots] = {};
    int originX = 0, originY = 0;   // origin of the list being executed
    std::vector<std::vector<uint8_t>> patchedConstants; // per dispatch of the range: the constant block with gRectOrigin / gRectOffset zeroed

    std::vector<nrdhip::PassLauncher> launchers; // per pipeline index (nullptr = pass not implemented in this build)
    std::vector<nrdhip::Plane> scratchPlanes;
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
        std::vector<nrdhip::LaunchRecord> records; // parameters the executable graph currently holds
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

namespace nrdhip {

uint32_t BytesPerTexel(nrd::Format f);
// Format each user slot must have in this build (MAX_NUM = slot not supported). translucentShadow: the instance holds SIGMA_SHADOW_TRANSLUCENCY, whose output is RGBA8
nrd::Format ExpectedUserFormat(nrd::ResourceType t, bool translucentShadow);

// The kernels address a plane with 32-bit byte offsets built by a 24-bit multiply (planes.h TexelOffset): row pitch < 2^24 bytes, pitch x rows < 2^32 bytes (strictly: the offset of the row one past the end must not wrap either). Every frame size a
// 16-bit resource size can name stays below that except the very largest with 16-byte texels (RGBA32F pool planes, the decoded-guide cache: 16384 x 16384 texels and more) -- refused
// at creation / binding instead of wrapping around.
inline bool PlaneAddressable(uint64_t pitchBytes, uint64_t rows) { return pitchBytes < (1ull << 24) && pitchBytes * rows < (1ull << 32); }

// Makes sure the executor's own `plane` exists with the size and pitch of `geometry` (whose ptr is ignored): PRESENT = it already did, REALLOCATED = a new, uninitialised allocation
// took its place (what it held is gone: the caller drops decodedFresh), FAILED = hipMalloc failed and the plane is empty.
enum class Ensured { PRESENT, REALLOCATED, FAILED };
Ensured EnsurePlane(Plane& plane, const Plane& geometry);

// executor_graph.hip: launches the records as one cached graph
uint32_t LaunchAsGraph(NrdHipExecutor* e, std::vector<LaunchRecord>& records);

} // namespace nrdhip
