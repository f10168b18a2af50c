// HIP execution back-end of the NRD pass chain for AMD Instinct MI355X (gfx950) -- thin C-ABI.
//
// The reference library only DESCRIBES dispatches; executing them is the job of its integration layer
// (reference Integration/NRDIntegration.h:83-165, NRDIntegration.hpp). This header is what replaces that layer:
//
//   reference nrd::Integration::Initialize   (NRDIntegration.hpp:93-139, :292-454: creates the pool textures)   -> nrdHipCreateExecutor
//   reference nrd::Integration::Destroy      (NRDIntegration.hpp:805-...)                                       -> nrdHipDestroyExecutor
//   reference UserPool / Integration_SetResource (NRDIntegration.h:37-60: app textures by ResourceType slot)     -> nrdHipBindResource
//   reference nrd::Integration::Denoise      (NRDIntegration.hpp:516-623: GetComputeDispatches + loop)           -> nrdHipDenoise
//   reference nrd::Integration::Dispatch     (NRDIntegration.hpp:625-803: bind + constants + CmdDispatch)        -> nrdHipExecuteDispatches
//   reference nrd::Integration::GetTotalMemoryUsageInMb (NRDIntegration.h:120-127)                               -> nrdHipGetPoolMemoryUsage
//
// Plain C types only: device pointers are void*, the stream is a hipStream_t passed as void*, formats and resource
// slots are the numeric values of nrd::Format / nrd::ResourceType (include/NRDDescs.h). Every function returns an
// nrd::Result value as uint32_t (0 = SUCCESS). Nothing here synchronises the device: launches are enqueued on the
// executor's stream in dispatch order.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct NrdHipExecutor NrdHipExecutor;

// A pitched 2D plane in device memory ("texture" of the reference). Texel (x, y) lives at
// data + y * rowPitchBytes + x * bytesPerTexel(format). rowPitchBytes must be a multiple of the texel size.
typedef struct NrdHipPlaneDesc {
    void* data;
    uint32_t rowPitchBytes;
    uint32_t format; // nrd::Format
    uint16_t width;
    uint16_t height;
} NrdHipPlaneDesc;

// Creates the executor for an nrd::Instance (include/NRD.h) and allocates its permanent + transient pool planes
// (one hipMalloc arena, 256-byte aligned rows) for textures of resourceWidth x resourceHeight.
// "instance" is an nrd::Instance*; "hipStream" is a hipStream_t (NULL = default stream).
// Size limit: planes are addressed with 32-bit byte offsets, so a plane of 16-byte texels must stay below 4 GiB -- every size up to 16384 x 16383 (or 65535 x 4095) is accepted,
// larger ones return UNSUPPORTED (as does a user plane whose row pitch reaches 16 MiB or whose pitch x height reaches 4 GiB, in nrdHipBindResource).
uint32_t nrdHipCreateExecutor(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, NrdHipExecutor** executor);
void nrdHipDestroyExecutor(NrdHipExecutor* executor);

// Same, but the pool arena is provided (and owned) by the caller, which is the reference's own model ("NRD allocates no GPU
// memory": reference Integration creates the pool textures from InstanceDesc). "arena" must be device memory of at least
// nrdHipGetArenaSize() bytes, 256-byte aligned; it is zero-filled on the stream. Lets a host that owns the memory (e.g. a
// tensor library) alias pool planes for collectives.
uint64_t nrdHipGetArenaSize(void* instance, uint16_t resourceWidth, uint16_t resourceHeight);
uint32_t nrdHipCreateExecutorWithArena(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, void* hipStream, void* arena, uint64_t arenaSize, NrdHipExecutor** executor);

// Binds an application plane to an IN_* / OUT_* slot. The bytes are not copied; the binding persists until rebound.
// Formats accepted in this build (anything else -> UNSUPPORTED):
//   IN_MV RGBA16_SFLOAT | IN_NORMAL_ROUGHNESS R10_G10_B10_A2_UNORM (the format of the library's normal encoding, nrd::GetLibraryDesc().normalEncoding: RGBA8_UNORM /
//   RGBA8_SNORM / R10_G10_B10_A2_UNORM / RGBA16_UNORM / RGBA16_SNORM for encodings 0..4 -- a build option as in the reference) | IN_VIEWZ R32_SFLOAT
//   IN/OUT_{DIFF,SPEC}_RADIANCE_HITDIST RGBA16_SFLOAT | IN/OUT_{DIFF,SPEC}_SH0, _SH1 RGBA16_SFLOAT (REBLUR / RELAX SH variants)
//   IN/OUT_{DIFF,SPEC}_HITDIST R16_UNORM (REBLUR occlusion family) | IN/OUT_DIFF_DIRECTION_HITDIST RGBA16_SNORM | IN_PENUMBRA R16_SFLOAT | IN_TRANSLUCENCY, IN_BASECOLOR_METALNESS RGBA8_UNORM
//   OUT_SHADOW_TRANSLUCENCY R8_UNORM (SIGMA_SHADOW) or RGBA8_UNORM (an instance holding SIGMA_SHADOW_TRANSLUCENCY)
//   IN_SIGNAL / OUT_SIGNAL RGBA32_SFLOAT | IN_{DIFF,SPEC}_CONFIDENCE, IN_DISOCCLUSION_THRESHOLD_MIX R8_UNORM | OUT_VALIDATION RGBA8_UNORM
// include/NRD.hip.h has the device functions that produce / consume these encodings (the NRD.hlsli front-end and back-end).
uint32_t nrdHipBindResource(NrdHipExecutor* executor, uint32_t resourceType, const NrdHipPlaneDesc* plane);

// Describes a pool plane (resourceType = TRANSIENT_POOL or PERMANENT_POOL, index into InstanceDesc::*Pool).
// For tooling and parity tests (history inspection); the memory stays owned by the executor.
uint32_t nrdHipGetPoolPlane(NrdHipExecutor* executor, uint32_t resourceType, uint32_t indexInPool, NrdHipPlaneDesc* plane);

// ---- Layered executor: SIGMA for many lights, N shadow layers in one pass chain ------------------------------------------------------------------------------
// One executor over ONE instance of SIGMA_SHADOW and / or SIGMA_SHADOW_TRANSLUCENCY denoises layersNum (1 .. NRD_HIP_MAX_SHADOW_LIGHTS) shadow layers -- one per light -- per
// nrdHipDenoise: every dispatch of the list is still ONE launch, whose grid's z extent is layersNum (Clear_* dispatches included). This is possible because the layers differ in
// nothing but the planes they touch: every constant of a SIGMA pass comes from CommonSettings and SigmaSettings, and the one per-light field, lightDirection
// (gLightDirectionView), is filled by the host and read by no pass in this version (the reference uses it only with SIGMA_USE_SCREEN_SPACE_SAMPLING == 0; its config sets 1).
// So there are no per-layer constants. layersNum == 1 is exactly nrdHipCreateExecutor: the same pool, the same kernels, the same bytes. With layersNum > 1 an instance that
// holds any pass other than SIGMA_* / Clear_* returns UNSUPPORTED (message on stderr); layersNum of 0 or above the maximum returns INVALID_ARGUMENT.
//   Pool: every permanent and transient pool plane exists once per layer, layer l starting l x (the plane's 256-byte aligned size) behind layer 0; the whole arena is zero-filled
// once; nrdHipGetPoolMemoryUsage reports the totals; nrdHipGetPoolPlane describes layer 0 and nrdHipGetPoolPlaneLayer any layer (layer >= layersNum: INVALID_ARGUMENT). A
// caller-provided arena (nrdHipCreateExecutorWithArena) stays unlayered.
//   Slots: IN_PENUMBRA, IN_TRANSLUCENCY and OUT_SHADOW_TRANSLUCENCY are per layer. On an executor with layersNum > 1 they are bound with nrdHipBindResourceLayers only (a plain
// nrdHipBindResource of one of them returns INVALID_ARGUMENT and names the slot): `plane` describes layer 0 under the formats and limits of nrdHipBindResource, layer l is
// data + l x layerBytes (64-bit: the stack may exceed 4 GiB, a layer may not), layerBytes >= rowPitchBytes x height and a multiple of 4 -- the light-layer rule of
// nrdHipPackShadowLights, whose stacks bind as they are. IN_VIEWZ, IN_NORMAL_ROUGHNESS and IN_MV are shared: bound with nrdHipBindResource, one plane read by all layers.
// nrdHipBindResourceLayers on a shared slot, on an executor without layers or with a bad stride returns INVALID_ARGUMENT. Nothing is bound or enqueued on any error.
//   Execution: nrdHipDenoise, nrdHipExecuteDispatches and nrdHipExecuteDispatchRange (NULL row arrays) work as on any executor -- all-or-nothing pre-flight, graph mode, profiling
// (one launch per pass), dynamic resolution (only the shared guide planes get rect-at-origin twins); the word of nrdHipSetHistoryReachWord receives the maximum over the layers.
// Refused with UNSUPPORTED + nrdHipGetLastError, nothing enqueued: a row restriction (nrdHipSetOwnedRows with less than the whole frame, non-NULL row arrays), nrdHipCheckInputs
// and nrdHipCheckInputsAsync (audit a layer through an unlayered executor), any pass in a list that is neither SIGMA_* nor Clear_*.
//   Contract: after any sequence of frames, layer l of OUT_SHADOW_TRANSLUCENCY and of every pool plane holds byte for byte what a separate unlayered executor over its own instance
// holds that was fed the same settings and shared guides with layer l's penumbra, translucency and output planes bound -- temporal stabilisation per light included, which the
// one-instance loop over the lights cannot have. Layers never read each other; the bytes between the layers of a user stack are never written.
uint32_t nrdHipCreateExecutorLayered(void* instance, uint16_t resourceWidth, uint16_t resourceHeight, uint32_t layersNum, void* hipStream, NrdHipExecutor** executor);
uint32_t nrdHipBindResourceLayers(NrdHipExecutor* executor, uint32_t resourceType, const NrdHipPlaneDesc* plane, uint64_t layerBytes);
uint32_t nrdHipGetPoolPlaneLayer(NrdHipExecutor* executor, uint32_t resourceType, uint32_t indexInPool, uint32_t layer, NrdHipPlaneDesc* plane);
uint32_t nrdHipGetLayersNum(const NrdHipExecutor* executor, uint32_t* layersNum);

// Executes a dispatch list obtained from nrd::GetComputeDispatches on the executor's stream, in order.
// "dispatchDescs" is a const nrd::DispatchDesc*. All-or-nothing: the whole list is checked first (a HIP kernel exists for every pass, all
// resources are bound, every pass accepts its constants) and an error (UNSUPPORTED / INVALID_ARGUMENT + nrdHipGetLastError) is returned
// BEFORE anything is enqueued.
uint32_t nrdHipExecuteDispatches(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum);

// nrd::GetComputeDispatches(identifiers) followed by nrdHipExecuteDispatches: one denoised frame.
// nrd::SetCommonSettings / SetDenoiserSettings must have been called for this frame.
uint32_t nrdHipDenoise(NrdHipExecutor* executor, const uint32_t* identifiers, uint32_t identifiersNum);

// Multi-GPU row-strip sharding: restricts this executor to PRODUCING rows [rowBegin, rowEnd) of the final outputs and of the
// permanent (history) planes. Planes stay full-size; every pass is launched on the strip extended by the cumulative reach of the
// passes that follow it in the dispatch list (nrdHipGetDispatchReach below: temporal stabilization 1 row, REBLUR's blur / post-blur
// the bound of their tap rings -- 39 / 79 rows at the default radius and 1440p --, history fix its base stride + 6, ...), so the owned rows are
// bit-identical to a single-GPU run provided the caller makes the other ranks' owned rows of the permanent planes available before
// the next frame (one in-place all-gather per plane: owned strips are contiguous row ranges). rowBegin = 0, rowEnd >= height
// restores whole-frame execution. REBLUR, RELAX and SIGMA lists are all bounded; a pass of unknown reach (a dynamic-resolution
// step, a blur ring as large as its distance from the camera) and every pass in front of it run on the whole frame, as does
// SIGMA's history Copy.
uint32_t nrdHipSetOwnedRows(NrdHipExecutor* executor, uint32_t rowBegin, uint32_t rowEnd);

// Finer-grained sharding control for a host that exchanges halos between passes (raytracingdenoiser_amd/sharding.py, HaloSharder):
//   nrdHipGetDispatchReach     reachRows[i] = how many rows above / below a pixel dispatch i reads from planes written earlier in the same
//                              frame (0 = own row only, -1 = unknown: the pass must run on the whole frame); "instance" is an nrd::Instance*
//                              (host-only: needs no device)
//   nrdHipExecuteDispatchRange executes dispatches [first, first + count) of the list; rowBegin[i] / rowEnd[i] (indexed by the absolute
//                              dispatch index; NULL or rowBegin[i] < 0 = whole frame) are the rows dispatch i has to produce. Ranges of one
//                              list must be executed in order starting at first = 0 (the per-frame caches are rebuilt there).
uint32_t nrdHipGetDispatchReach(void* instance, const void* dispatchDescs, uint32_t dispatchDescsNum, int32_t* reachRows);
uint32_t nrdHipExecuteDispatchRange(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t first, uint32_t count, const int32_t* rowBegin,
    const int32_t* rowEnd);

// The halo-exchange plan of one dispatch list for rank `rank` of `world` ranks owning the row strips [stripBounds[r], stripBounds[r + 1]) (host-only,
// no device needed). This is the planner: raytracingdenoiser_amd/sharding.py (HaloSharder), include/NRDShardedIntegrationHip.hpp and hosts that drive
// RCCL themselves all plan with it.
//   steps[s]   dispatches [firstDispatch, firstDispatch + dispatchCount) run between two exchanges; before them the rank sends / receives, for each of
//              items[firstItem .. firstItem + itemCount), `widthRows` rows on either side of its strip boundaries to / from ranks rank - 1 and rank + 1
//              (send its own top / bottom rows, receive into the rows just above / below its strip); the first `earlyCount` dispatches of the step touch
//              none of these planes and may run while the transfers are in flight
//   rowBegin / rowEnd (length dispatchDescsNum)   the rows every dispatch has to produce, ready for nrdHipExecuteDispatchRange (-1 = whole frame)
//   info->fallback = 1   the list cannot be sharded (unknown reach, halo wider than a strip): every rank runs the whole frame, after having received
//                        the other ranks' strips of the carried-over planes if the previous frame was sharded
// Returns INVALID_ARGUMENT with info->stepsNum / itemsNum set when the capacities are too small.
typedef struct NrdHipHaloItem {
    uint32_t resourceType; // nrd::ResourceType: TRANSIENT_POOL / PERMANENT_POOL (+ indexInPool) or an OUT_* slot doubling as history
    uint32_t indexInPool;
    uint32_t widthRows;
} NrdHipHaloItem;
typedef struct NrdHipHaloStep {
    uint32_t firstDispatch, dispatchCount, earlyCount, firstItem, itemCount;
} NrdHipHaloStep;
typedef struct NrdHipHaloPlanInfo {
    uint32_t fallback, stepsNum, itemsNum;
} NrdHipHaloPlanInfo;
uint32_t nrdHipPlanHaloExchange(void* instance, const void* dispatchDescs, uint32_t dispatchDescsNum, const uint32_t* stripBounds, uint32_t world, uint32_t rank, uint32_t height,
    uint32_t maxMotionRows, uint32_t exchangeThreshold, int32_t* rowBegin, int32_t* rowEnd, NrdHipHaloStep* steps, uint32_t stepsCapacity, NrdHipHaloItem* items, uint32_t itemsCapacity,
    NrdHipHaloPlanInfo* info);

// The motion side of the sharding contract, measured on the device: *maxRows = the largest vertical distance (in rows of the previous rect) over which the
// surface-motion reprojection of the temporal passes (reference REBLUR_TemporalAccumulation.hlsli:136-150, RELAX_TemporalAccumulation.hlsli:560-575,
// SIGMA_TemporalStabilization.hlsli) moves a denoised pixel of rows [rowBegin, rowEnd) of the rect -- from the bound IN_VIEWZ / IN_MV planes and the constants
// of the given dispatch list (the list of THIS frame, before it is executed). One streaming kernel over the strip (12 B per pixel), a 4-byte read-back and
// a stream synchronisation. A rank calls it on its own strip, takes the MAX over ranks, and runs the frame unsharded when the result + 2 rows (bicubic
// footprint) does not fit the history halo it planned with (maxMotionRows below). 0 for lists without a temporal denoiser; pixels whose previous position
// lies behind the previous camera (or whose motion vector is NaN) report a huge value on purpose. The value bounds the SURFACE motion only: hosts double it for the
// virtual motion of specular reflections, which is a heuristic (a curved reflector can exceed it), not a check.
uint32_t nrdHipMeasureMotionRows(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd, float* maxRows);
// The same measurement without the host round trip: enqueued on the executor's stream, the result (a float) lands in 4 bytes of the CALLER'S device memory in stream order -- the
// buffer a multi-GPU host hands to its MAX all-reduce (RCCL reads it on the device); the host then synchronises once, on the reduced value.
// What the measurement above cannot bound: the temporal passes of the SPECULAR denoisers also read last frame's planes at the virtual-motion position and at look-back taps behind
// it, whose distance depends on hit distances and surface curvature. So the kernels report it: with a device word registered here, every temporal pass (REBLUR / RELAX
// TemporalAccumulation, SIGMA TemporalStabilization) leaves in it -- atomicMax on the bits of a non-negative float -- the largest number of rows one of its pixels read away from its
// own row (sample positions only: add 3 rows for the bicubic footprint). The word belongs to the caller: clear it in stream order before a frame, read it (or MAX-all-reduce it over
// the ranks) after, hold it against the history halo that frame was run with, and size the next frame's decision with it. nullptr (the default) switches the tracking off.
uint32_t nrdHipSetHistoryReachWord(NrdHipExecutor* executor, void* deviceWord);
uint32_t nrdHipMeasureMotionRowsAsync(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd, void* deviceMaxRows);

// The input side of the contract, audited on the device: are the bound IN_* planes inside NRD's input rules (reference README "NOISY & NON-NOISY DATA REQUIREMENTS", "NOISY
// INPUTS") for the frame the given dispatch list describes (the list of THIS frame, before it is executed)? The denoisers promise nothing outside these rules and a broken one
// poisons the history planes silently; the pack calls below sanitise, a host that binds planes it encoded itself has this call. It only reports: nothing is fixed or written but
// the report. One streaming kernel over the rect, which tests exactly the texels the passes read, loads nothing outside the rect and touches only planes that can hold a non-finite value (UNORM / SNORM planes -- normals,
// confidences, IN_*_HITDIST, IN_DIFF_DIRECTION_HITDIST, translucency, base colour -- are never touched).
//   rule                    violated by a pixel of the rect when
#define NRD_HIP_INPUT_RULE_VIEWZ_NOT_FINITE 0u   // guide: IN_VIEWZ is NaN / INF
#define NRD_HIP_INPUT_RULE_MV_NOT_FINITE 1u      // guide: .x, .y or .z of IN_MV is NaN / INF
#define NRD_HIP_INPUT_RULE_DIFF_NOT_FINITE 2u    // noisy: any channel of IN_DIFF_RADIANCE_HITDIST, or of IN_DIFF_SH0 / IN_DIFF_SH1, is NaN / INF
#define NRD_HIP_INPUT_RULE_SPEC_NOT_FINITE 3u    // noisy: the same for IN_SPEC_RADIANCE_HITDIST, IN_SPEC_SH0 / IN_SPEC_SH1
#define NRD_HIP_INPUT_RULE_DIFF_HITDIST_RANGE 4u // noisy: .w of the radiance / SH0 plane is finite and < 0; for a slot read by REBLUR passes only (normalised hit distance), also > 1
#define NRD_HIP_INPUT_RULE_SPEC_HITDIST_RANGE 5u
#define NRD_HIP_INPUT_RULE_PENUMBRA_INVALID 6u   // noisy: IN_PENUMBRA is NaN / INF or < 0
#define NRD_HIP_INPUT_RULE_SIGNAL_NOT_FINITE 7u  // any channel of REFERENCE's IN_SIGNAL is NaN / INF
#define NRD_HIP_INPUT_RULES_NUM 8u
// Which rules: *rulesChecked (host side, written by both calls) has bit r set for every rule that applies -- a dispatch of the list names the rule's IN_* slot among its
// resources and the slot holds a float format in this build. A list to which no rule applies (the REBLUR occlusion family without its guides, an empty list) is SUCCESS with mask
// 0, pixels = inRangePixels = 0 and nothing but the clearing of the report enqueued. The > 1 bound of rules 4 / 5 applies when every dispatch naming the slot is a REBLUR pass.
// Which texels: rect, rectOrigin, denoisingRange, viewZScale, frameIndex and the checkerboard cells are those of the list's constants. Guides are read at rectOrigin + (x, y) for
// every pixel (x, y) of the rect, noisy planes at (x, y); a checkerboarded signal only where ( ( x ^ y ) ^ frameIndex ) & 1 equals the signal's cell, at column x >> 1. The noisy
// rules 2 .. 6 are tested only where the pixel is in range by the passes' own predicate, !( abs( viewZ * viewZScale ) > denoisingRange ) (RELAX: abs( viewZ )), and viewZ is
// finite: garbage beyond the range and outside the rect is allowed and not reported; a pixel whose viewZ is not finite counts under rule 0 only. Guides are tested on the sky too.
// IN_SIGNAL has no range test. -0.0 is not negative; a NaN or INF hit distance counts under the NOT_FINITE rule only.
typedef struct NrdHipInputReport {
    uint32_t pixels;                         // pixels of the rect
    uint32_t inRangePixels;                  // of which the passes denoise (not sky by the predicate above; all of them for a list that does not read IN_VIEWZ)
    uint32_t count[NRD_HIP_INPUT_RULES_NUM]; // pixels violating the rule (a pixel counts once per rule, however many channels or planes are bad)
    uint32_t first[NRD_HIP_INPUT_RULES_NUM]; // smallest y * rectWidth + x (rect coordinates) among them; 0xFFFFFFFF when count is 0
} NrdHipInputReport;
// INVALID_ARGUMENT + nrdHipGetLastError, with nothing enqueued and the report untouched: a NULL pointer (Async: or one that is not 4-byte aligned), a slot a checked rule needs
// that is not bound (IN_VIEWZ for every noisy rule), a rect that leaves a bound plane. UNSUPPORTED, likewise with nothing enqueued: a list that reads a signal both as
// *_RADIANCE_HITDIST and as *_SH0 / *_SH1 (two denoisers of one instance: check them one at a time), or *_SH1 without *_SH0. A list of several pass families (REBLUR + RELAX +
// SIGMA denoisers in one instance) is audited with the constants of the FIRST family block in it: its viewZScale and its form of the sky predicate hold for every pixel and plane. Both calls cover the whole rect whatever nrdHipSetOwnedRows says. The sync form keeps its device buffer in the executor (made on first
// use), synchronises the stream and copies the report back. The Async form zeroes and fills sizeof( NrdHipInputReport ) bytes of the CALLER'S device memory (4-byte aligned) in
// stream order: no allocation, no synchronisation, capturable into a graph. Counts are integers: the report does not depend on the order in which the waves arrive.
uint32_t nrdHipCheckInputs(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum, NrdHipInputReport* report, uint32_t* rulesChecked);
uint32_t nrdHipCheckInputsAsync(NrdHipExecutor* executor, const void* dispatchDescs, uint32_t dispatchDescsNum, void* deviceReport, uint32_t* rulesChecked);
const char* nrdHipGetInputRuleString(uint32_t rule); // "VIEWZ_NOT_FINITE", ...; NULL beyond the table

// Per-pass GPU timing. When enabled, every dispatch is bracketed by hipEvents on the executor's stream.
// nrdHipCollectPassTimings synchronises the stream, folds all brackets recorded since the last collect into per-pipeline
// totals and returns the number of pipelines written: pipelineIndices[i] (index into InstanceDesc::pipelines),
// milliseconds[i] (sum of durations) and launches[i] (count). One more row than there are pipelines: index == InstanceDesc::pipelinesNum is the per-frame guide
// preparation (the decode / rect-shift kernels in front of the first pass of a list; absent when the list's tile-classification kernel writes the guide planes itself --
// whole-frame decode of a REBLUR-only or RELAX-only list without a shifted rect: that time is then part of the *_ClassifyTiles.cs row). Pass capacity >= InstanceDesc::pipelinesNum + 1.
uint32_t nrdHipSetProfiling(NrdHipExecutor* executor, uint32_t enable);
uint32_t nrdHipCollectPassTimings(NrdHipExecutor* executor, uint32_t* pipelineIndices, double* milliseconds, uint32_t* launches, uint32_t capacity, uint32_t* written);

// Graph mode (the HIP-graph counterpart of the command list the reference integration records per Denoise call, reference
// Integration/NRDIntegration.hpp:516-623): with enable != 0 the kernel launches of a dispatch range are not enqueued one by one but as ONE
// hipGraph launch. The executable graph is built once per topology (the sequence of kernels of the range; ping-pong and per-frame constants do
// not change it) and on the following frames only the parameters of the nodes that changed are updated (hipGraphExecKernelNodeSetParams).
// Results are bit-identical to eager launches; per-pass profiling (nrdHipSetProfiling) falls back to eager launches while it is on.
// nrdHipGetGraphStats: graph launches, graphs built (topology misses) and node-parameter updates so far (any pointer may be NULL).
uint32_t nrdHipSetGraphMode(NrdHipExecutor* executor, uint32_t enable);
uint32_t nrdHipGetGraphStats(const NrdHipExecutor* executor, uint64_t* graphLaunches, uint64_t* graphBuilds, uint64_t* nodeUpdates);

// Diagnostics of the passes that run as a fast kernel plus a fallback kernel (REBLUR TemporalAccumulation: the surface-motion footprints of a 32x8-pixel tile come
// from one LDS-staged window of the previous frame; a tile whose window would be too large is left to the plain kernel -- DESIGN.md section 3). Reads the tile
// flags of the LAST frame back (synchronises the stream): tiles the fallback kernel processed and tiles in total. Results never depend on the split.
uint32_t nrdHipGetTileFallbackStats(NrdHipExecutor* executor, uint32_t* fallbackTiles, uint32_t* totalTiles);

// DEPRECATED (kept so that round-2 callers still link; do not use in new code). Always 0: there is one library and one arithmetic (DESIGN.md "Numerics": IEEE + - * and
// source-determined fused multiply-adds, division / sqrt / exp2 / log2 through v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 / v_exp_f32 / v_log_f32 -- bit-identical to the CPU oracle).
__attribute__((deprecated("one library, one arithmetic: the answer is always 0")))
uint32_t nrdHipGetNumericsMode(void);

// Bytes held by the pool arena (permanent, transient).
uint32_t nrdHipGetPoolMemoryUsage(const NrdHipExecutor* executor, uint64_t* permanentBytes, uint64_t* transientBytes);

// Diagnostics: evaluates one primitive of the device numerics contract (DESIGN.md "Numerics") elementwise on device
// arrays, so a harness can pin the GPU's codecs and transcendentals bit-for-bit against another implementation.
//   op: 0 exp2, 1 log2, 2 atan, 3 pow(x, y = in2), 4 fp32->fp16->fp32 round trip, 5 Div(x, in2) = x * v_rcp_f32(in2), 6 sqrt, 7 1/sqrt,
//       8..12 small-integer / {1023, 255, 63, 15, 3} (the codecs' 3-op exact division), 13 exp(-0.66 x^2), 14 small-integer / 65535, 15 int16 / 32767;
//       16 v_rcp_f32, 17 v_rsq_f32, 18 v_sqrt_f32 (the raw instructions), 19 v_cvt_pk_f16_f32(x, in2) (the packed word as float bits), 20 Rcp;
//       21 Exp2NonPos(x) = 2 * v_exp_f32(x - 1) for x <= 0, 22 SatExp2(x) = saturate(2^x), 23 ExpNegAbs(x) = e^-|x|, 24 Pow01(x, in2) = saturate(x)^in2 for in2 >= 0 (round 5)
// in2 may be NULL for unary ops. Launches on hipStream (a hipStream_t as void*, may be NULL).
uint32_t nrdHipEvalNumerics(uint32_t op, const float* in1, const float* in2, float* out, uint32_t count, void* hipStream);

// Diagnostics: the streaming bandwidth this GPU delivers to a plain 16-bytes-per-lane copy kernel (read + write, GB/s) -- the "measured copy
// bandwidth on the same device" the roofline fractions of bench.py are also quoted against. Allocates 2 * bytes of scratch
// device memory, runs `repetitions` timed copies after 3 warm-up copies (HIP events on hipStream) and frees the scratch again.
uint32_t nrdHipMeasureCopyBandwidth(uint64_t bytes, uint32_t repetitions, void* hipStream, double* gigabytesPerSecond);

// Last error text of this executor (never NULL).
const char* nrdHipGetLastError(const NrdHipExecutor* executor);

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Front end / back end on the device: what an application does with the reference's NRD.hlsli in its own shaders -- pack its fp32 G-buffer and noisy
// signals into the planes nrdHipBindResource accepts, and turn the denoised OUT_* planes back into linear radiance -- as two fused kernels of the
// library, for hosts that hold device buffers but write no HIP kernels (a tensor library). The arithmetic is include/NRD.hip.h, unfused IEEE with
// correctly rounded division and square root; the stores are the codecs of the passes (fp16 round-to-nearest-even, UNORM floor(x * max + 0.5), SNORM
// round half away from zero). Executor-free: no instance, no pool. One launch each, asynchronous on the given stream, no allocation and no
// synchronisation (usable inside a HIP graph capture). Everything is validated before the first HIP call and nothing is enqueued on an error:
//   a required plane (or one the chosen mode needs: direction, camera, albedo / Rf0, the matching output) with data == NULL     -> INVALID_ARGUMENT
//   a format other than the one listed for the plane                                                                           -> UNSUPPORTED
//   planes of different sizes, a row pitch below the row or not a multiple of the texel size, a misaligned pointer             -> INVALID_ARGUMENT
//   a row pitch >= 16 MiB or pitch x height >= 4 GiB (the limits of nrdHipBindResource), an orthographic camera                -> UNSUPPORTED
// nrdHipGetLastFrontEndError says which (per calling thread, never NULL). A plane with data == NULL is absent and costs nothing.
//
// Signal modes (which packer / unpacker of NRD.hip.h a signal goes through)
#define NRD_HIP_SIGNAL_NONE 0u
#define NRD_HIP_SIGNAL_REBLUR_RADIANCE 1u              // RADIANCE_HITDIST RGBA16_SFLOAT: YCoCg + normalised hit distance
#define NRD_HIP_SIGNAL_REBLUR_SH 2u                    // SH0 + SH1 RGBA16_SFLOAT
#define NRD_HIP_SIGNAL_REBLUR_OCCLUSION 3u             // HITDIST R16_UNORM: the normalised hit distance alone
#define NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION 4u // DIFF_DIRECTION_HITDIST RGBA16_SNORM
#define NRD_HIP_SIGNAL_RELAX_RADIANCE 5u               // RADIANCE_HITDIST RGBA16_SFLOAT: radiance + hit distance in world units
#define NRD_HIP_SIGNAL_RELAX_SH 6u                     // SH0 + SH1 RGBA16_SFLOAT
// How an SH pair (or a directional-occlusion texel) becomes a colour in the back end
#define NRD_HIP_RESOLVE_SG_EXTRACT_COLOR 0u // NRD_SG_ExtractColor: the denoised colour, no normal involved
#define NRD_HIP_RESOLVE_SH 1u               // NRD_SH_ResolveDiffuse / NRD_SH_ResolveSpecular
#define NRD_HIP_RESOLVE_SG 2u               // NRD_SG_ResolveDiffuse / NRD_SG_ResolveSpecular

typedef struct NrdHipFrontEndSignal {
    uint32_t mode;                   // NRD_HIP_SIGNAL_*
    NrdHipPlaneDesc radianceHitDist; // in,  RGBA32_SFLOAT: radiance.rgb, hit distance in world units (the occlusion modes read .w only)
    NrdHipPlaneDesc direction;       // in,  RGBA32_SFLOAT: direction.xyz of the ray (SH and directional-occlusion modes)
    NrdHipPlaneDesc out0;            // out, the format of the mode: IN_*_RADIANCE_HITDIST / IN_*_SH0 / IN_*_HITDIST / IN_DIFF_DIRECTION_HITDIST
    NrdHipPlaneDesc out1;            // out, IN_*_SH1 RGBA16_SFLOAT (SH modes)
} NrdHipFrontEndSignal;

// REBLUR modes normalise the hit distance with REBLUR_FrontEnd_GetNormHitDist( hitDist, viewZ * viewZScale, hitDistParams, roughness ), roughness = 1 for
// the diffuse signal and the pixel's linear roughness for the specular one; every packer runs with sanitize = true.
// Demodulation: with albedo AND rf0 given, the radiance of each signal is divided by its NRD_MaterialFactors factor (of the raw normal and roughness and
// the view vector below) before it is packed; commonSettings is needed for that alone.
typedef struct NrdHipFrontEndDesc {
    const void* commonSettings;         // const nrd::CommonSettings* of the frame (camera) or NULL
    float hitDistParams[4];             // ReblurSettings::hitDistanceParameters
    float viewZScale;                   // IN_VIEWZ = viewZ * viewZScale; 0 is read as 1
    float tanOfLightAngularRadius;      // SIGMA_FrontEnd_PackPenumbra (directional light)
    NrdHipPlaneDesc normalRoughness;    // in,  RGBA32_SFLOAT, required: world-space normal.xyz, linear roughness
    NrdHipPlaneDesc viewZ;              // in,  R32_SFLOAT, required
    NrdHipPlaneDesc materialID;         // in,  R32_SFLOAT: 0..3, kept by normal encoding 2 only
    NrdHipPlaneDesc motion;             // in,  RGBA32_SFLOAT or RG32_SFLOAT (.zw = 0), clamped to +-65504
    NrdHipPlaneDesc albedo, rf0;        // in,  RGBA32_SFLOAT (.rgb): demodulation
    NrdHipPlaneDesc distanceToOccluder; // in,  R32_SFLOAT: 0 where NoL <= 0, the hit distance of the shadow ray, >= 65504 on a miss (NRD.hip.h SIGMA_FrontEnd_PackPenumbra)
    NrdHipPlaneDesc translucency;       // in,  RGBA32_SFLOAT (.rgb)
    NrdHipFrontEndSignal diffuse, specular;
    NrdHipPlaneDesc outNormalRoughness; // out, IN_NORMAL_ROUGHNESS in the format of the library's normal encoding
    NrdHipPlaneDesc outViewZ;           // out, IN_VIEWZ R32_SFLOAT
    NrdHipPlaneDesc outMv;              // out, IN_MV RGBA16_SFLOAT (needs motion)
    NrdHipPlaneDesc outPenumbra;        // out, IN_PENUMBRA R16_SFLOAT (needs distanceToOccluder)
    NrdHipPlaneDesc outTranslucency;    // out, IN_TRANSLUCENCY RGBA8_UNORM (needs distanceToOccluder and translucency)
} NrdHipFrontEndDesc;

typedef struct NrdHipBackEndSignal {
    uint32_t mode;       // NRD_HIP_SIGNAL_*
    uint32_t resolve;    // NRD_HIP_RESOLVE_* (SH and directional-occlusion modes)
    NrdHipPlaneDesc in0; // in,  OUT_*_RADIANCE_HITDIST / OUT_*_SH0 (RGBA16_SFLOAT or RGBA32_SFLOAT), OUT_*_HITDIST R16_UNORM, OUT_DIFF_DIRECTION_HITDIST RGBA16_SNORM
    NrdHipPlaneDesc in1; // in,  OUT_*_SH1 (RGBA16_SFLOAT or RGBA32_SFLOAT; SH modes)
    NrdHipPlaneDesc out; // out, RGBA32_SFLOAT: linear rgb, hit distance (R32_SFLOAT for the occlusion mode)
} NrdHipBackEndSignal;

// REBLUR radiance goes through REBLUR_BackEnd_UnpackRadianceAndNormHitDist, RELAX radiance and REBLUR occlusion are widened as they are, an SH pair
// (REBLUR_BackEnd_UnpackSh / RELAX_BackEnd_UnpackSh) or a directional-occlusion texel (REBLUR_BackEnd_UnpackDirectionalOcclusion) is resolved as `resolve`
// says into .rgb with its hit distance in .w. denormalizeHitDist != 0 turns the hit distance of the REBLUR modes back into world units (REBLUR_GetHitDist;
// roughness 1 / the pixel's). N and the roughness are those of the bound IN_NORMAL_ROUGHNESS plane (NRD_LoadNormalRoughnessTexel +
// NRD_FrontEnd_UnpackNormalAndRoughness). remodulate != 0 multiplies each resolved colour by its NRD_MaterialFactors factor (needs albedo, rf0 and the camera).
// View vector, per pixel (x, y) of a w x h frame, in correctly rounded fp32 operations in exactly this order, nothing fused:
//   uv = ( ( x + 0.5 ) / w, ( y + 0.5 ) / h )      Xv = ( ( uv.x * frustum.z + frustum.x ) * viewZ, ( uv.y * frustum.w + frustum.y ) * viewZ, viewZ )
//   Xw.i = ( R[ i ][ 0 ] * Xv.x + R[ i ][ 1 ] * Xv.y ) + R[ i ][ 2 ] * Xv.z      V = -( Xw * ( 1 / sqrt( ( Xw.x * Xw.x + Xw.y * Xw.y ) + Xw.z * Xw.z ) ) )
// with frustum and R = the rotation of view-to-world as the denoisers' constants hold them (gFrustum, gViewToWorld) for the given nrd::CommonSettings, whose
// rectSize must be the size of the planes, and viewZ the value of the IN_VIEWZ plane. Perspective projections only.
typedef struct NrdHipBackEndDesc {
    const void* commonSettings;      // const nrd::CommonSettings* of the frame or NULL (needed wherever V is: specular SH / SG resolves, remodulation, factors, outViewVector)
    float hitDistParams[4];          // ReblurSettings::hitDistanceParameters
    uint32_t denormalizeHitDist;
    uint32_t remodulate;
    NrdHipPlaneDesc normalRoughness; // in,  IN_NORMAL_ROUGHNESS as bound (needed by SH / SG resolves, the specular hit distance, remodulation)
    NrdHipPlaneDesc viewZ;           // in,  IN_VIEWZ R32_SFLOAT (needed by V and by denormalizeHitDist)
    NrdHipPlaneDesc albedo, rf0;     // in,  RGBA32_SFLOAT (.rgb)
    NrdHipBackEndSignal diffuse, specular;
    NrdHipPlaneDesc shadow;          // in,  OUT_SHADOW_TRANSLUCENCY R8_UNORM or RGBA8_UNORM
    NrdHipPlaneDesc outShadow;       // out, R32_SFLOAT or RGBA32_SFLOAT: SIGMA_BackEnd_UnpackShadow
    NrdHipPlaneDesc outComposed;     // out, RGBA32_SFLOAT: diffuse.rgb + specular.rgb as written to their out planes, .w = 0
    NrdHipPlaneDesc outViewVector;   // out, RGBA32_SFLOAT: V, .w = 0
    NrdHipPlaneDesc outDiffFactor, outSpecFactor; // out, RGBA32_SFLOAT: the NRD_MaterialFactors factors, .w = 0
} NrdHipBackEndDesc;

uint32_t nrdHipPackInputs(const NrdHipFrontEndDesc* desc, void* hipStream);
uint32_t nrdHipResolveOutputs(const NrdHipBackEndDesc* desc, void* hipStream);
const char* nrdHipGetLastFrontEndError(void);

// The same two calls with an options struct next to the descriptor. options == NULL or an all-zero struct is exactly the call above: the same kernel, the same bytes.
// The contract is the one above: validated before the first HIP call, nothing enqueued on an error, no allocation, no synchronisation, capturable into a graph,
// errors through nrdHipGetLastFrontEndError. (In all four calls the camera of commonSettings is read when the call is made: a captured call replays with the camera it was captured with.)
//
// Checkerboarded noisy inputs (reference NRDSettings.h:35-44 "checkerboardMode"; every REBLUR / RELAX pass here implements it). All planes keep the full size. With
// BLACK the diffuse signal lives in cell 0 and the specular one in cell 1, with WHITE the opposite; pixel (x, y) carries a signal's data when
// ( ( x ^ y ) ^ frameIndex ) & 1 == cell (nrdmath.h CheckerBoard). Only those pixels of the signal's fp32 planes (radianceHitDist, direction) are read -- the others may
// hold anything, NaN included -- and the texel the plain call would write for that pixel (its own viewZ, roughness and material factor) goes to column x >> 1 of the same
// row of out0 / out1. No other byte of out0 / out1 is written: not the right half, and not the last column of the left half in the rows where, at an odd width, it has no
// source pixel. The G-buffer outputs are unaffected. checkerboardMode > 2, or a mode other than OFF without a diffuse or specular signal -> INVALID_ARGUMENT.
typedef struct NrdHipFrontEndOptions {
    uint32_t checkerboardMode; // nrd::CheckerboardMode: 0 OFF, 1 BLACK, 2 WHITE -- the orientation of the DIFFUSE signal, the specular one is the opposite (Reblur.cpp:318-330, Relax.cpp:88-97)
    uint32_t frameIndex;       // CommonSettings::frameIndex of the frame the planes are for
} NrdHipFrontEndOptions;
uint32_t nrdHipPackInputsEx(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, void* hipStream);

// Re-jittering: step two of the high-quality resolve of an SH denoiser (reference README "IMPROVING OUTPUT QUALITY": SG resolve, re-jitter, remodulation). With
// reJitter != 0 pixel (x, y) computes
//   scale = NRD_SG_ReJitter( diffSg, specSg, Rf0, V, roughness, Z, Ze, Zw, Zn, Zs, N, Ne, Nw, Nn, Ns )
// from the two unpacked SH pairs, Rf0 of the rf0 plane, V of the contract above, Z of IN_VIEWZ, N and the roughness of the IN_NORMAL_ROUGHNESS texel, and the Z and N of the
// neighbours e = ( x + 1, y ), w = ( x - 1, y ), n = ( x, y + 1 ), s = ( x, y - 1 ); a neighbour outside the plane has N = 0 and Z = 0, with which the function
// returns ( 1, 1 ): border pixels are exactly unscaled. The colour written is ( resolved.rgb * scale.x or .y ) * factor, in that order, the factor only with remodulate; .w and
// outComposed (the sum of the two colours as written) are as without it. Needs both signals in an SH mode with resolve SH or SG (else INVALID_ARGUMENT), and
// normalRoughness, viewZ, rf0 and commonSettings (INVALID_ARGUMENT naming the one that is missing); albedo only with remodulation or the factor outputs.
// outReJitterScale in another format -> UNSUPPORTED; outReJitterScale without reJitter -> INVALID_ARGUMENT.
typedef struct NrdHipBackEndOptions {
    uint32_t reJitter;                // != 0: multiply both resolved colours by NRD_SG_ReJitter
    NrdHipPlaneDesc outReJitterScale; // out, RG32_SFLOAT, optional: the two factors (x diffuse, y specular)
} NrdHipBackEndOptions;
uint32_t nrdHipResolveOutputsEx(const NrdHipBackEndDesc* desc, const NrdHipBackEndOptions* options, void* hipStream);

// Many paths per pixel (reference README "NOISY INPUTS": "In case of many paths per pixel hitT for specular must be 'averaged' by
// NRD_FrontEnd_SpecHitDistAveraging_* functions from NRD.hlsli"): the pack call over N sample layers per signal, reduced by the reference's rules and packed in the
// same launch. Sample layer s of a signal plane is the plane of the descriptor with its `data` advanced by s x layerBytes -- a [ N, H, W, 4 ] tensor; layer bases are
// 64-bit pointers, each layer obeys the per-plane limits above, the whole stack may exceed 4 GiB. samples == NULL, or a struct whose counts are 0 or 1 and whose
// threshold is 0, is exactly nrdHipPackInputsEx( desc, options, stream ): the same kernel, the same bytes, no extra loads. The contract is the one above: validated
// before the first HIP call, nothing enqueued on an error, no allocation, no synchronisation, capturable into a graph, errors through nrdHipGetLastFrontEndError.
// INVALID_ARGUMENT, naming the field: samplesNum > 64; a non-zero `reserved`; a negative or NaN hitDistTrimThreshold; and with samplesNum > 1: a layer stride
// (of a plane the mode reads) that is not a multiple of 16 or is below rowPitchBytes x height of that plane, or a signal whose mode is NONE.
//
// Per pixel and signal, in unfused fp32 with correctly rounded division, with r = 1 for the diffuse signal and the pixel's roughness for the specular one, and
// `factor` the signal's NRD_MaterialFactors factor when demodulating -- for s = 0 .. N - 1, in this order:
//   1. ( rad_s, h_s ) and, where the mode needs it, dir_s are read from layer s
//   2. if hitDistTrimThreshold > 0: h_s = NRD_FrontEnd_TrimHitDistance( h_s, hitDistTrimThreshold )
//   3. if demodulating: rad_s = rad_s / factor, component-wise, as the plain call does
//   4. P_s = what the mode's packer of NRD.hip.h returns for that one sample with sanitize = true: the fp32 out0 (and out1 for the SH modes), before any store codec.
//      Sanitising, clamping to NRD_FP16_MAX and the hit-distance normalisation ( REBLUR_FrontEnd_GetNormHitDist( h_s, viewZ, hitDistParams, r ) ) are per sample,
//      exactly as the plain call would do for a pixel holding that sample.
// Then
//   diffuse signal, every mode:            texel = ( ( ( P_0 + P_1 ) + P_2 ) + ... ) / float( N ), component-wise over all channels of out0 and out1
//   specular signal, colour channels:      the same mean over every channel except the one that carries the hit distance
//   specular signal, hit-distance channel: ( out0.w, or the only channel in the occlusion mode ) the packer's hit-distance output for the single value H, where
//                                          a = NRD_FrontEnd_SpecHitDistAveraging_Begin(); _Add( a, h_s ) for each s in order; _End( a ); H = a
//                                          -- normalised once for the REBLUR modes, clamped by RELAX's packer for the RELAX modes
// and the texel goes through the store codec of the plain call. This is the only place where the two signals differ: the reference prescribes the minimum of the
// non-zero samples (0 when all are 0) for the specular hitT only and nothing for the diffuse one, for which the mean of the normalised (RELAX: clamped) hit
// distances is used. Every packer is linear in ( radiance, direction x luminance ) once its per-sample clamp is applied, so the mean of the packed samples is the
// packed estimate of the mean signal for radiance, SH and directional occlusion alike; N = 1 degenerates to the plain call bit for bit ( P_0 / 1.0f ).
// Checkerboarding: pixel selection and the x >> 1 column are those of nrdHipPackInputsEx; only the selected pixels of any layer are read. The G-buffer and SIGMA
// outputs are unaffected.
typedef struct NrdHipSignalSamples {
    uint32_t samplesNum;                // 0 is read as 1; at most 64
    uint32_t reserved;                  // must be 0
    uint64_t radianceHitDistLayerBytes; // distance from sample layer s to layer s + 1 of NrdHipFrontEndSignal::radianceHitDist
    uint64_t directionLayerBytes;       // the same for ::direction (modes that read it)
} NrdHipSignalSamples;
typedef struct NrdHipFrontEndSamples {
    NrdHipSignalSamples diffuse, specular;
    float hitDistTrimThreshold;         // > 0: every sample's hit distance goes through NRD_FrontEnd_TrimHitDistance first; 0: off
    uint32_t reserved;                  // must be 0
} NrdHipFrontEndSamples;
uint32_t nrdHipPackInputsSamples(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, void* hipStream);

// Three-channel and split planes: the layout a tensor host holds -- normal [ H, W, 3 ] and roughness [ H, W ], radiance [ H, W, 3 ] and hit distance [ H, W ] -- read and
// written in place, with no widened RGBA32_SFLOAT copy. In the two calls below a plane documented as RGBA32_SFLOAT may be RGB32_SFLOAT instead (nrd::Format, 12-byte texels):
//   pack:     normalRoughness, motion, albedo, rf0, translucency, { diffuse, specular }.radianceHitDist and .direction
//   resolve:  the inputs albedo and rf0; the outputs diffuse.out, specular.out, outComposed, outViewVector, outDiffFactor, outSpecFactor
// (the fp32 in0 / in1 planes, outShadow and outReJitterScale keep their formats; the calls above still answer UNSUPPORTED to RGB32_SFLOAT). An RGB32_SFLOAT plane: pointer and
// row pitch multiples of 4 (not of 12, not of 16), row pitch >= 12 x width, the 32-bit limits as above. Where `.w` comes from:
//   normalRoughness RGB32_SFLOAT                       -> .w = split->roughness
//   { diffuse, specular }.radianceHitDist RGB32_SFLOAT -> .w = split->{ diffuse, specular }HitDist
//   a companion that is missing -> INVALID_ARGUMENT naming the field (no roughness or hit distance is ever taken as 0 silently); a companion given next to an RGBA32_SFLOAT
//   plane, or for a signal whose mode is NONE -> INVALID_ARGUMENT (.w would have two sources). .w of every other RGB32_SFLOAT input is not read; motion.w = 0, as .zw of RG32_SFLOAT.
//   REBLUR_OCCLUSION reads .w only: radianceHitDist.data may be NULL when the companion is given (4 bytes per pixel are read for that signal).
// Resolve: .rgb goes to the RGB32_SFLOAT plane, the hit distance to split->{ diffuse, specular }HitDist if given and nowhere otherwise; the output of REBLUR_OCCLUSION is
// R32_SFLOAT already, a companion for it -> INVALID_ARGUMENT. Sample layers (nrdHipPackInputsSamples rules): the layer stride of an RGB32_SFLOAT stack or of a companion is a
// multiple of 4 and >= rowPitchBytes x height; a companion has the layer count of its signal; the rule of RGBA32_SFLOAT stacks (a multiple of 16) is unchanged.
// Every output byte equals what the call above writes for RGBA32_SFLOAT planes holding the same .xyz and the companion's value in .w: the arithmetic is the same code, only loads
// and stores differ. split == NULL or zeroed with every plane RGBA32_SFLOAT is exactly nrdHipPackInputsSamples( desc, options, samples, stream ) / nrdHipResolveOutputsEx( desc,
// options, stream ): the same kernels, the same bytes. The contract is the one above: validated before the first HIP call, nothing enqueued on an error, no allocation, no
// synchronisation, capturable into a graph, errors through nrdHipGetLastFrontEndError.
typedef struct NrdHipFrontEndSplit {
    NrdHipPlaneDesc roughness;          // in, R32_SFLOAT: .w of normalRoughness when that plane is RGB32_SFLOAT
    NrdHipPlaneDesc diffuseHitDist;     // in, R32_SFLOAT: .w of diffuse.radianceHitDist when that plane is RGB32_SFLOAT (or absent: the occlusion mode)
    NrdHipPlaneDesc specularHitDist;    // in, R32_SFLOAT: the same for the specular signal
    uint64_t diffuseHitDistLayerBytes;  // distance from sample layer s to layer s + 1 of diffuseHitDist
    uint64_t specularHitDistLayerBytes; // the same for specularHitDist
} NrdHipFrontEndSplit;
uint32_t nrdHipPackInputsSplit(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, const NrdHipFrontEndSplit* split, void* hipStream);

typedef struct NrdHipBackEndSplit {
    NrdHipPlaneDesc diffuseHitDist, specularHitDist; // out, R32_SFLOAT, optional: .w of diffuse.out / specular.out when those are RGB32_SFLOAT
} NrdHipBackEndSplit;
uint32_t nrdHipResolveOutputsSplit(const NrdHipBackEndDesc* desc, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split, void* hipStream);

// Quarter-resolution tracing and denoising (reference README "RECOMMENDATIONS AND BEST PRACTICES: LESSER TIPS": "In case of quarter resolution tracing and denoising use
// pixelPos / 2 as texture coordinates ... 'Nearest Z' upsampling works best for upscaling of the denoised output"). The full size is W x H, the low size w = ( W + 1 ) >> 1,
// h = ( H + 1 ) >> 1; low pixel ( i, j ) stands for full pixel ( 2i, 2j ) -- not a rotated grid. The denoisers run at any size; the two calls below are the front end and
// the back end of such a frame: a decimated pack, the denoise at w x h, and a resolve that brings the low OUT_* planes back to the full-size frame, where albedo, Rf0 and the
// normals have their detail. Both follow the contract above: validated before the first HIP call, nothing enqueued on an error, no allocation, no synchronisation, capturable
// into a graph, errors through nrdHipGetLastFrontEndError, the 32-bit limits for each plane at its own size, RGB32_SFLOAT planes by the rules of the *Split calls.
// Out of scope: checkerboarding combined with decimation, re-jittering combined with upsampling, decimation inside nrdHipPackGuides (pack the guides at full size and hand
// them to the calls below), any filter other than nearest Z.
//
// nrdHipPackInputsDecimated. guideShift == 0 is exactly nrdHipPackInputsSplit( desc, options, samples, split, stream ): the same kernels, the same bytes. guideShift == 1:
//   full size (W x H), read at ( 2x, 2y ) for low pixel ( x, y ):  normalRoughness, viewZ, materialID, motion, albedo, rf0 and split->roughness -- the G-buffer
//   low size (w x h):  everything traced -- both signals' radianceHitDist / direction and their sample layers, split->{ diffuse, specular }HitDist, distanceToOccluder,
//                      translucency -- and every output
// Every output byte equals what nrdHipPackInputsSplit writes when it is fed contiguous copies of the G-buffer planes decimated [ ::2, ::2 ]: the arithmetic is the same code,
// only the load coordinate of the G-buffer planes differs. commonSettings (demodulation) is the struct of the LOW-size frame: rectSize = ( w, h ), and the view vector is that
// of pixel ( x, y ) of a w x h frame. guideShift > 1 -> INVALID_ARGUMENT. With guideShift 1: G-buffer planes that are not all one size W x H, low planes that are not all one
// size w x h, or sizes that break the relation above -> INVALID_ARGUMENT naming the plane; a checkerboardMode other than OFF -> UNSUPPORTED (out of scope).
uint32_t nrdHipPackInputsDecimated(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, const NrdHipFrontEndSplit* split,
                                   uint32_t guideShift, void* hipStream);

// One traced lobe per sample: the probabilistic diffuse / specular split (reference README "NOISY INPUTS": "Probabilistic split at primary hit": divide the radiance by the
// selection probability, do not divide the hit distance, set the hit distance of the signal that was not traced to exactly 0, turn hitDistanceReconstructionMode and the
// pre-pass on, and guarantee a valid sample in every 3x3 / 5x5 area). The application holds ONE traced plane -- what the one path of a pixel returned -- a byte per pixel
// saying which lobe that path took and, optionally, the probability with which the specular lobe is chosen there; the call builds both packed signals from them in one launch,
// each traced byte loaded once. lobes == NULL is exactly nrdHipPackInputsSplit( desc, options, NULL, split, stream ): the same kernels, the same bytes. The contract is the one
// above: validated before the first HIP call, nothing enqueued on an error, no allocation, no synchronisation, one launch, capturable into a graph, errors through
// nrdHipGetLastFrontEndError, the 32-bit limits for every plane and layer. Sample layer s of a plane of `lobes` is the plane with its `data` advanced by s x its layer stride
// (64-bit); with samplesNum > 1 a stride is a multiple of 16 for an RGBA32_SFLOAT stack and of 4 for RGB32_SFLOAT, R32_SFLOAT and R8_UINT stacks, and >= rowPitchBytes x height.
// With `lobes` given:
//   INVALID_ARGUMENT, naming the field: a non-NULL { diffuse, specular }.radianceHitDist or .direction of the descriptor, or split->{ diffuse, specular }HitDist (the traced
//       data would have two sources); a signal whose mode is NONE (both are produced); a missing lobe plane; a missing direction when a mode reads one; samplesNum > 64;
//       a non-zero reserved; a bad layer stride
//   UNSUPPORTED: a checkerboardMode other than OFF (checkerboarding is the other way to split); a format other than the one listed
// The G-buffer inputs and outputs, demodulation, split->roughness and the SIGMA outputs behave as in the plain call. Decimation is out of scope.
//
// Per pixel and signal X (0 diffuse, 1 specular), in unfused fp32 with correctly rounded division, for s = 0 .. N - 1 in this order:
//   1. ( rad, h ), dir where a mode of either signal reads a direction, the byte L and, when the probability plane is given, p are read from layer s, each once
//   2. q = L == NRD_HIP_LOBE_SPECULAR ? p : 1 - p;  q = 1 without the probability plane
//   3. the sample counts for X iff L == X and q > 0 (false for a NaN): then rad_s = rad / q component-wise, h_s = h, dir_s = dir;
//      else rad_s = ( 0, 0, 0 ), h_s = 0 and dir_s = ( 0, 0, 1 ) -- never the loaded values, which may be NaN where the other lobe was traced
//   4. steps 3 and 4 of nrdHipPackInputsSamples: demodulation, then P_s = the mode's packer with sanitize = true
// Then
//   both signals, every channel but the one carrying the hit distance:  ( ( ( P_0 + P_1 ) + P_2 ) + ... ) / float( N ) over ALL N samples -- the zeros of the samples that do
//                                                                       not count are what makes rad / q an unbiased estimate
//   specular hit distance:  NRD_FrontEnd_SpecHitDistAveraging_Begin / _Add( h_s ) / _End over all samples (zeros drop out by that rule; 0 if none), then the packer's
//                           hit-distance output for that value, as nrdHipPackInputsSamples does
//   diffuse hit distance:   the sum, in order, of the packer's hit-distance output over the n COUNTED samples only, divided by float( n ); 0 when n == 0. (A mean that took in
//                           the zeros of the other samples would pull the distance toward 0 and still mark the texel valid for the hit-distance reconstruction.)
// and the texel goes through the store codec of the plain call. With N = 1 every output byte equals nrdHipPackInputsEx fed two RGBA32_SFLOAT planes that hold ( rad / q, h )
// -- direction planes: dir -- where the sample counts and ( 0, 0, 0, 0 ) -- direction planes: ( 0, 0, 1 ) -- elsewhere.
#define NRD_HIP_LOBE_DIFFUSE 0u
#define NRD_HIP_LOBE_SPECULAR 1u // any other byte: nothing was traced for this sample
typedef struct NrdHipFrontEndLobes {
    NrdHipPlaneDesc radianceHitDist; // in, RGBA32_SFLOAT, or RGB32_SFLOAT with hitDist below: what the ONE traced path returned (may be absent when both modes read .w only and hitDist is given)
    NrdHipPlaneDesc hitDist;         // in, R32_SFLOAT: .w when radianceHitDist is RGB32_SFLOAT (rules of nrdHipPackInputsSplit)
    NrdHipPlaneDesc direction;       // in, RGBA32_SFLOAT / RGB32_SFLOAT: needed when either signal's mode reads a direction
    NrdHipPlaneDesc lobe;            // in, R8_UINT, required: NRD_HIP_LOBE_*
    NrdHipPlaneDesc probability;     // in, R32_SFLOAT, optional: probability with which the SPECULAR lobe is chosen at this pixel; absent = radiance is already divided (q = 1)
    uint32_t samplesNum;             // 0 is read as 1; at most 64
    uint32_t reserved;               // must be 0
    uint64_t radianceHitDistLayerBytes, hitDistLayerBytes, directionLayerBytes, lobeLayerBytes, probabilityLayerBytes;
} NrdHipFrontEndLobes;
uint32_t nrdHipPackInputsLobes(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSplit* split, const NrdHipFrontEndLobes* lobes,
                               void* hipStream);

// Combined denoising of direct and indirect lighting (reference README "GREATER TIPS: COMBINED DENOISING OF DIRECT AND INDIRECT LIGHTING"): a path tracer with next-event
// estimation or ReSTIR holds the two in separate planes and wants one REBLUR / RELAX instance to denoise their sum. The README's rule: the radiance is summed; the SPECULAR
// hit distance is the indirect one alone ("a light chosen for its diffuse contribution breaks specular reprojection"); the DIFFUSE hit distance is
// lerp( indirect, direct, min( Ldirect / ( Ldirect + Lindirect + EPS ), maxContribution ) ), which gives sharper contact shadows. nrdHipPackInputsDirect does it in the pack
// launch, each traced byte loaded once. direct == NULL, or a struct in which neither signal has a direct plane, is exactly nrdHipPackInputsDecimated( desc, options, samples,
// split, guideShift, stream ): the same kernels, the same bytes. The contract is the one above: validated before the first HIP call, nothing enqueued on an error, no
// allocation, no synchronisation, one launch, capturable into a graph, errors through nrdHipGetLastFrontEndError, the 32-bit limits for every plane and layer.
// The planes of the descriptor ( desc->diffuse / specular, split->*HitDist, samples ) are the INDIRECT ones under this call. The direct planes are traced data: low-size under
// guideShift == 1, and under checkerboarding read only at the pixels selected for their signal. A signal without a direct plane is packed as ever: no load is added to it.
//
// Per pixel and signal, in unfused fp32 with correctly rounded division. Sample s = 0 .. N - 1, N the signal's sample count; direct layer t = s when the direct stack has N layers:
//   1. ( rad_i, h_i ), dir_i from indirect layer s; ( rad_d, h_d ), dir_d from direct layer t. h_d is loaded ONLY for the diffuse signal with maxHitDistContribution > 0.
//   2. hitDistTrimThreshold > 0: h_i and h_d go through NRD_FrontEnd_TrimHitDistance.
//   3. Demodulating, both radiances are divided by the signal's factor, as the plain call does.
//   4. P_i, P_d = the mode's packer ( sanitize = true ) for ( rad_i, h_i, dir_i ) and ( rad_d, 0, dir_d ). Every channel that does not carry the hit distance:
//      C_s = clamp( P_i + P_d, -NRD_FP16_MAX, NRD_FP16_MAX ) -- a no-op below fp16 overflow: the store codec never rounds a sum of two clamped terms to infinity. The packers are
//      linear in ( radiance, direction x luminance ): this is the packed estimate of the summed signal, in the radiance and the SH modes alike.
//   5. Hit distance. SPECULAR: h_i, exactly as without `direct` (with samples: NRD_FrontEnd_SpecHitDistAveraging_* over the h_i). DIFFUSE: the packer's hit-distance output for
//      h = NRD_HIP_MixDiffuseHitDist( h_i, h_d, L_i, L_d, maxHitDistContribution ) (NRD.hip.h), L = _NRD_Luminance( san( rad ) ) of the demodulated radiance, san the packers'
//      own first line: _NRD_IsInvalid( r ) ? 0 : clamp( r, 0, NRD_FP16_MAX ). A direct term never makes an invalid hit distance valid: an h_i of 0 stays 0, so the texel stays
//      marked for HitDistanceReconstruction and nrdHipCheckHitDistCoverage. Where no light was sampled ( rad_d NaN or zero, h_d anything ) every channel is the indirect-only one.
//   6. Over the samples: colour channels ( ( C_0 + C_1 ) + ... ) / float( N ); the diffuse hit-distance channel is the mean of the packed per-sample values, as
//      nrdHipPackInputsSamples does; then the store codec of the plain call.
//   7. ONE direct layer under N > 1 (one NEE / ReSTIR sample per pixel under many indirect paths): the direct texel is loaded once; colour = clamp( mean_s( P_i,s ) + P_d );
//      the diffuse hit distance mixes every h_i,s with the same ( h_d, L_d ) and its own L_i,s, then takes the mean.
// INVALID_ARGUMENT, naming the field: a direct plane for a signal whose mode is NONE, REBLUR_OCCLUSION or REBLUR_DIRECTIONAL_OCCLUSION (no radiance to weigh by); a missing
// direction where the mode reads one, or a direction where it reads none; specular.hitDist given (the specular direct distance is never read: .w of an RGBA32_SFLOAT specular
// direct plane may hold anything); diffuse.hitDist missing when the plane is RGB32_SFLOAT and maxHitDistContribution > 0, given when the plane is RGBA32_SFLOAT or when
// maxHitDistContribution == 0; maxHitDistContribution NaN, negative or above 1; samplesNum neither 1 nor the signal's count; a non-zero reserved; layer strides that break the
// rules of nrdHipPackInputsSamples / Split; size, pitch or alignment mismatches as elsewhere. UNSUPPORTED: a format other than those listed.
// Out of scope: combining with nrdHipPackInputsLobes; the back end (a combined signal resolves like any other).
#define NRD_HIP_DIRECT_MAX_CONTRIBUTION_DEFAULT 0.5f // README: "0.65 works good as well"
typedef struct NrdHipDirectSignal {
    NrdHipPlaneDesc radianceHitDist; // in, RGBA32_SFLOAT, or RGB32_SFLOAT (+ hitDist below): direct radiance.rgb, distance to the sampled light / occluder in .w; data NULL = this signal has no direct term
    NrdHipPlaneDesc hitDist;         // in, R32_SFLOAT: .w when radianceHitDist is RGB32_SFLOAT -- DIFFUSE signal only
    NrdHipPlaneDesc direction;       // in, RGBA32_SFLOAT / RGB32_SFLOAT: direction to the light (SH modes)
    uint64_t radianceHitDistLayerBytes, hitDistLayerBytes, directionLayerBytes;
    uint32_t samplesNum;             // 0 is read as 1; must be 1 or the signal's own sample count
    uint32_t reserved;               // must be 0
} NrdHipDirectSignal;
typedef struct NrdHipFrontEndDirect {
    NrdHipDirectSignal diffuse, specular;
    float maxHitDistContribution;    // [0, 1]; 0 = the diffuse hit distance stays the indirect one and no direct hit distance is read
    uint32_t reserved;               // must be 0
} NrdHipFrontEndDirect;
uint32_t nrdHipPackInputsDirect(const NrdHipFrontEndDesc* desc, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, const NrdHipFrontEndSplit* split,
                                const NrdHipFrontEndDirect* direct, uint32_t guideShift, void* hipStream);

// Does every pixel have a valid hit distance in the area the hit-distance reconstruction searches? A probabilistic split (above) leaves the hit distance of the lobe that was not
// traced at 0, and REBLUR / RELAX_HitDistReconstruction look no further than 3x3 or 5x5 texels: a pixel whose area holds no valid sample keeps a hit distance of 0, silently, and
// the history keeps it. nrdHipCheckInputs cannot see that -- it is a property of a neighbourhood. This call audits the PACKED planes as they will be bound; it needs no executor.
//   in range:         viewZ is finite and !( abs( viewZ * viewZScale ) > denoisingRange ) -- the passes' own predicate, as in nrdHipCheckInputs
//   valid neighbour:  inside the plane, in range, and its stored hit distance != 0 as the passes test it on the decoded value ( .w of an RGBA16_SFLOAT / RGBA16_SNORM texel, the
//                     channel of an R16_UNORM one); a NaN counts as non-zero (whether values are finite is rules 2..5 of nrdHipCheckInputs)
//   empty[ s ]:       in-range pixels whose own stored hit distance is 0
//   holes[ s ]:       of those, the pixels with no valid neighbour in the ( 2 area + 1 )^2 texels around them: CERTAINLY unreconstructable. A necessary condition only: the passes
//                     also weight by geometry and normal, so a pixel that is not a hole can still end up with nothing.
// The report goes to 4-byte aligned CALLER device memory, zeroed and filled in stream order: no allocation, no synchronisation, capturable into a graph. Counts are integers and
// firstHole is a minimum: the report does not depend on the order of the waves. Everything is validated before the first HIP call and nothing is enqueued on an error
// (nrdHipGetLastFrontEndError): a missing viewZ or report, no signal at all, an area of 0 or above 2, a non-zero reserved, planes of different sizes -> INVALID_ARGUMENT; any
// other format -> UNSUPPORTED.
typedef struct NrdHipCoverageSignal {
    NrdHipPlaneDesc plane; // IN_*_RADIANCE_HITDIST / IN_*_SH0 RGBA16_SFLOAT (.w), IN_*_HITDIST R16_UNORM, IN_DIFF_DIRECTION_HITDIST RGBA16_SNORM (.w); data NULL = absent
} NrdHipCoverageSignal;
typedef struct NrdHipCoverageDesc {
    NrdHipPlaneDesc viewZ; // IN_VIEWZ R32_SFLOAT, required
    NrdHipCoverageSignal diffuse, specular;
    float viewZScale;      // 0 is read as 1
    float denoisingRange;
    uint32_t area;         // nrd::HitDistanceReconstructionMode: 1 = 3x3, 2 = 5x5
    uint32_t reserved;     // must be 0
} NrdHipCoverageDesc;
typedef struct NrdHipCoverageReport { // per signal s: 0 diffuse, 1 specular
    uint32_t inRangePixels;
    uint32_t empty[2];     // in-range pixels whose own stored hit distance is 0
    uint32_t holes[2];     // of those, pixels with no valid neighbour in the area
    uint32_t firstHole[2]; // smallest y * width + x; 0xFFFFFFFF when holes is 0
} NrdHipCoverageReport;
uint32_t nrdHipCheckHitDistCoverage(const NrdHipCoverageDesc* desc, void* deviceReport, void* hipStream);

// nrdHipResolveOutputsUpsampled. upsample == NULL is exactly nrdHipResolveOutputsSplit( desc, options, split, stream ). With upsample given:
//   low size:   diffuse.in0 / in1, specular.in0 / in1, shadow and upsample->lowViewZ -- the denoiser's OUT_* planes and its IN_VIEWZ
//   full size:  normalRoughness (the IN_NORMAL_ROUGHNESS format, packed at full size by a plain pack call), viewZ, albedo, rf0, every output of the descriptor, the split
//               hit-distance outputs and upsample->outSource
// commonSettings, viewZ and lowViewZ are required. commonSettings is the denoiser's own struct of the frame -- it supplies viewZScale, denoisingRange and the camera -- so its
// rectSize must be the LOW size; the view vector of the contract above is evaluated with w = W, h = H. One launch. Per full pixel ( X, Y ), in correctly rounded fp32:
//   s  = viewZScale          R = denoisingRange
//   Zf = abs( viewZ[ X, Y ] * s )
//   out of range      if Zf is NaN or Zf > R                                   -> source = none
//   candidate k = a + 2b, for a, b in { 0, 1 }:
//       texel ( i, j ) = ( ( X >> 1 ) + a, ( Y >> 1 ) + b )
//       exists         iff ( a == 0 or X is odd ) and ( b == 0 or Y is odd ) and i < w and j < h
//       Zk             = abs( lowViewZ[ i, j ] * s )
//       valid          iff Zk is not NaN and !( Zk > R )
//       dk             = abs( Zk - Zf )
//   source            = the valid candidate of smallest dk; a tie goes to the lowest k
//                       none if there is no valid candidate
//                       none if depthThreshold > 0 and dk > depthThreshold * Zf
// N, the roughness, V, the material factors, and the viewZ and roughness denormalizeHitDist uses are those of the FULL pixel, computed exactly as the plain call does. Only the
// signal texels -- in0, in1 and shadow -- are read at the source texel; they then go through the code of the plain call: unpack, SH / SG / extract resolve, remodulation, store.
// (A hit distance denormalised with the full pixel's depth and roughness is exact where those equal the source texel's and an approximation elsewhere.) Where the source is none,
// every signal output, its split hit-distance plane, outShadow and outComposed get zeros and outSource 255; outViewVector, outDiffFactor and outSpecFactor do not depend on the
// source and are written for every pixel, as the plain call does. No byte of a signal plane is loaded at a candidate that is not the chosen source: the denoisers leave texels
// beyond the denoising range unwritten, so those may hold anything, NaN included.
// UNSUPPORTED: options->reJitter != 0 together with upsample (it needs full-size SG neighbours: out of scope); an outSource in a format other than R8_UINT. INVALID_ARGUMENT,
// naming the field: a missing commonSettings, viewZ or lowViewZ; a non-zero reserved; a NaN, negative or infinite depthThreshold; a rectSize that is not the low size; low or
// full planes that differ in size within their class or break the size relation.
typedef struct NrdHipBackEndUpsample {
    NrdHipPlaneDesc lowViewZ;  // in,  R32_SFLOAT, low size: the IN_VIEWZ plane the denoiser ran with
    NrdHipPlaneDesc outSource; // out, R8_UINT, full size, optional: which low texel a pixel took (0..3), 255 = none
    float depthThreshold;      // 0 = off; > 0: reject a source whose depth differs by more than depthThreshold * depth
    uint32_t reserved;         // must be 0
} NrdHipBackEndUpsample;
uint32_t nrdHipResolveOutputsUpsampled(const NrdHipBackEndDesc* desc, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split, const NrdHipBackEndUpsample* upsample,
                                       void* hipStream);

// SIGMA shadows for local and many lights (reference README "RECOMMENDATIONS ... LESSER TIPS", [SIGMA]): the front end and the back end of up to NRD_HIP_MAX_SHADOW_LIGHTS lights
// per pixel, one launch each, every input byte read once. The contract is the one above: validated before the first HIP call, nothing enqueued on an error, no allocation, no
// synchronisation, capturable into a graph, errors through nrdHipGetLastFrontEndError, the 32-bit limits per plane. The arithmetic is NRD.hip.h in unfused fp32 with correctly
// rounded division; the stores are fp16 round-to-nearest-even (IN_PENUMBRA) and floor( x * 255 + 0.5 ) (RGBA8_UNORM).
// Lights: a host array of `lightsNum` entries, read when the call is made and handed to the kernel by value in its arguments -- no device table, no copy; a captured call replays
// with the lights it was captured with. Layers: light i of a plane stack is the descriptor's plane with `data` advanced by i x its ...LayerBytes ([ N, H, W(, C) ] tensors), by the
// rules of nrdHipPackInputsSamples: with lightsNum > 1 a layer stride is >= rowPitchBytes x height and a multiple of 16 for an RGBA32_SFLOAT stack, of 4 for every other one
// (R32_SFLOAT, RGB32_SFLOAT, R16_SFLOAT, RGBA8_UNORM, R8_UNORM); layer bases are 64-bit, the whole stack may exceed 4 GiB. Inputs must be finite (distanceToOccluder by the rule
// of NRD.hip.h: 0 where NoL <= 0, the hit distance of the shadow ray, >= 65504 on a miss); nothing is sanitised beyond what the three reference functions do.
#define NRD_HIP_MAX_SHADOW_LIGHTS 32u
#define NRD_HIP_LIGHT_DIRECTIONAL 0u // p = SIGMA_FrontEnd_PackPenumbra( distanceToOccluder, tanOfLightAngularRadius )
#define NRD_HIP_LIGHT_LOCAL 1u       // p = SIGMA_FrontEnd_PackPenumbra( distanceToOccluder, distanceToLight, lightSize ): point, spot and sphere lights
#define NRD_HIP_SHADOWS_PER_LIGHT 0u // SIGMA applied per light: one IN_PENUMBRA (and IN_TRANSLUCENCY) layer per light, one denoiser instance reused with SigmaSettings::maxStabilizedFrameNum = 0 (the README's "stabilizationStrength = 0")
#define NRD_HIP_SHADOWS_COMBINED 1u  // one SIGMA_SHADOW_TRANSLUCENCY pass for all lights: pseudo translucency and a weighted penumbra
typedef struct NrdHipShadowLight {
    uint32_t type;                 // NRD_HIP_LIGHT_*
    float tanOfLightAngularRadius; // DIRECTIONAL: finite and >= 0 (not looked at for a LOCAL light)
    float lightSize;               // LOCAL: finite and >= 0, in world units (not looked at for a DIRECTIONAL light)
    uint32_t reserved;             // must be 0
} NrdHipShadowLight;

// Pack. With d_i = distanceToOccluder of light i and p_i = its penumbra by the light's type (layer i of distanceToLight is read only if light i is LOCAL: the layer of a
// directional light may hold anything):
//   PER_LIGHT  layer i of outPenumbra = p_i; with outTranslucency (needs translucency), its layer i = SIGMA_FrontEnd_PackTranslucency( d_i, translucency_i ). One DIRECTIONAL
//              light writes exactly the bytes nrdHipPackInputs writes to outPenumbra / outTranslucency for the same planes. Layer i binds as IN_PENUMBRA / IN_TRANSLUCENCY.
//   COMBINED   (lighting = the unshadowed L_i.rgb, required, as are outTranslucency and outLightingSum) for i = 0 .. N - 1 in this order, all sums starting at 0, dMin at +INF:
//                Lsum  = Lsum + L_i ( component-wise );   lit = d_i >= NRD_FP16_MAX;   LSsum = LSsum + L_i * ( lit ? 1 : 0 )
//                w     = ( weight given ? weight_i : ( lit ? 0 : 1 ) ) * _NRD_Luminance( L_i )
//                Wsum  = Wsum + w;   Psum = Psum + p_i * w;   dMin = min( dMin, d_i )
//              outPenumbra     = dMin >= NRD_FP16_MAX ? NRD_FP16_MAX : Psum / max( Wsum, NRD_EPS )
//              outTranslucency = SIGMA_FrontEnd_PackTranslucency( dMin, LSsum / max( Lsum, NRD_EPS ) ): .x = 1 exactly where no light is occluded
//              outLightingSum  = Lsum, .w = 0
//              The default weight counts occluded lights only -- the README's "weight should be zero if a pixel is not in the penumbra" in the one form the call can know; a
//              caller's weight plane should be zero for such lights too (a lit light carries p_i = NRD_FP16_MAX). After SIGMA: sum( L_i * S_i ) = Lsum * OUT_SHADOW_TRANSLUCENCY.yzw.
//              The README's caveats hold: one penumbra stands for all lights, overlapping shadows of very different sizes blur towards their weighted mean.
// INVALID_ARGUMENT, naming the field: lightsNum of 0 or above the maximum, lights == NULL; an unknown type or mode; a non-zero reserved; a NaN, negative or infinite
// tanOfLightAngularRadius / lightSize of a light whose type uses it; a missing plane the mode needs (distanceToOccluder; distanceToLight with a LOCAL light; lighting,
// outTranslucency, outLightingSum in COMBINED; translucency with outTranslucency in PER_LIGHT; outPenumbra); a plane the mode does not take (weight, lighting, outLightingSum in
// PER_LIGHT, and translucency there without outTranslucency; translucency in COMBINED); a bad layer stride with lightsNum > 1; size, pitch and alignment mismatches as above. Another format than listed: UNSUPPORTED.
typedef struct NrdHipShadowLightsPackDesc {
    uint32_t mode;                       // NRD_HIP_SHADOWS_*
    uint32_t lightsNum;                  // 1 .. NRD_HIP_MAX_SHADOW_LIGHTS
    const NrdHipShadowLight* lights;     // host memory, lightsNum entries
    NrdHipPlaneDesc distanceToOccluder;  // in,  R32_SFLOAT stack, required
    NrdHipPlaneDesc distanceToLight;     // in,  R32_SFLOAT stack: needed when any light is LOCAL
    NrdHipPlaneDesc translucency;        // in,  RGBA32_SFLOAT or RGB32_SFLOAT stack (.rgb): PER_LIGHT with outTranslucency
    NrdHipPlaneDesc lighting;            // in,  RGBA32_SFLOAT or RGB32_SFLOAT stack (.rgb): COMBINED
    NrdHipPlaneDesc weight;              // in,  R32_SFLOAT stack: COMBINED, optional
    uint64_t distanceToOccluderLayerBytes, distanceToLightLayerBytes, translucencyLayerBytes, lightingLayerBytes, weightLayerBytes;
    NrdHipPlaneDesc outPenumbra;         // out, R16_SFLOAT, required: a stack (PER_LIGHT) or one plane (COMBINED)
    NrdHipPlaneDesc outTranslucency;     // out, RGBA8_UNORM: a stack (PER_LIGHT, optional) or one plane (COMBINED, required)
    NrdHipPlaneDesc outLightingSum;      // out, RGBA32_SFLOAT or RGB32_SFLOAT: COMBINED, required
    uint64_t outPenumbraLayerBytes, outTranslucencyLayerBytes; // PER_LIGHT
} NrdHipShadowLightsPackDesc;
uint32_t nrdHipPackShadowLights(const NrdHipShadowLightsPackDesc* desc, void* hipStream);

// Resolve, with s = SIGMA_BackEnd_UnpackShadow of the denoised OUT_SHADOW_TRANSLUCENCY:
//   COMBINED   shadow: one RGBA8_UNORM plane, lighting: one plane holding Lsum (outLightingSum of the pack call). out.rgb = Lsum.rgb * s.yzw, out.w = s.x
//   PER_LIGHT  shadow: a stack of R8_UNORM (scalar s_i) or RGBA8_UNORM (s_i = .yzw) planes, lighting: the stack of L_i. acc = 0; for i in order: acc = acc + L_i * s_i;
//              out.rgb = acc, out.w = 0
// lightsNum is held to 1 .. NRD_HIP_MAX_SHADOW_LIGHTS in both modes (COMBINED reads one plane of each whatever it says). All three planes are required.
typedef struct NrdHipShadowLightsResolveDesc {
    uint32_t mode;            // NRD_HIP_SHADOWS_*
    uint32_t lightsNum;
    NrdHipPlaneDesc shadow;   // in,  RGBA8_UNORM (either mode) or R8_UNORM (PER_LIGHT)
    NrdHipPlaneDesc lighting; // in,  RGBA32_SFLOAT or RGB32_SFLOAT (.rgb)
    uint64_t shadowLayerBytes, lightingLayerBytes; // PER_LIGHT
    NrdHipPlaneDesc out;      // out, RGBA32_SFLOAT or RGB32_SFLOAT (.w is dropped)
} NrdHipShadowLightsResolveDesc;
uint32_t nrdHipResolveShadowLights(const NrdHipShadowLightsResolveDesc* desc, void* hipStream);

// Guides from world positions (reference README "INPUTS": IN_VIEWZ, IN_MV and the "LESSER TIPS" on motion vectors): what a path tracer holds are world-space hit positions, what
// the denoisers take is linear view depth and motion vectors in exactly the convention the temporal passes undo (REBLUR_TemporalAccumulation.hlsli:131-150: old = new + MV, uv
// units after motionVectorScale, .z = viewZprev - viewZ for 2.5D). This call derives both from `position` (and, for moving geometry, `positionPrev`) and the matrices of
// nrd::CommonSettings, and encodes the four optional UNORM slots from fp32 planes with the passes' store codec -- so that every IN_* guide can be produced by the library. The
// contract is the one above: executor-free, one launch, asynchronous on the stream, validated before the first HIP call, nothing enqueued on an error, no allocation, no
// synchronisation, capturable into a graph (the camera is read when the call is made: a captured call replays with the camera it was captured with), errors through
// nrdHipGetLastFrontEndError, the 32-bit limits per plane, RGB32_SFLOAT planes by the rules of nrdHipPackInputsSplit. Every output is optional; a plane with data == NULL is absent.
//
// Arithmetic: correctly rounded fp32 + - * / in exactly this order, nothing fused; a sum of three products is ( a * x + b * y ) + c * z, of three products and a constant
// ( ( a * x + b * y ) + c * z ) + d. A float32 restatement reproduces every byte.
// Host, once per call, from the caller's matrices as given (column-major, M[ i ][ j ] = row i, column j; no handedness flip: the flip the denoisers apply cancels in
// viewToClip . worldToView, so uv is the same for a left-handed and a right-handed pair of matrices; outViewZ has the sign of the caller's convention, which IN_VIEWZ may have --
// the passes take abs( IN_VIEWZ * viewZScale ) and form viewZprev = viewZ + IN_MV.z * s.z from it, so mv.z is the difference of the ABSOLUTE depths, the same for either handedness):
//   R[ i ][ j ] = worldToViewMatrix[ i ][ j ], i, j < 3      c.i = -( ( R[ 0 ][ i ] * t.x + R[ 1 ][ i ] * t.y ) + R[ 2 ][ i ] * t.z ), t = column 3 of worldToViewMatrix (the camera position)
//   P = viewToClipMatrix      Rp, cp, Pp: the same of worldToViewMatrixPrev / viewToClipMatrixPrev      s = motionVectorScale      world = isMotionVectorInWorldSpace
// Device, per pixel, with X = position.xyz:
//   miss      any component of X is NaN / INF: outViewZ = missViewZ, outMv = ( 0, 0, 0, 0 )
//   current   D = X - c ( component-wise, the subtraction first: camera-relative as the passes are )      Xv.i = ( R[ i ][ 0 ] * D.x + R[ i ][ 1 ] * D.y ) + R[ i ][ 2 ] * D.z      viewZ = Xv.z
//             clip.k = ( ( P[ k ][ 0 ] * Xv.x + P[ k ][ 1 ] * Xv.y ) + P[ k ][ 2 ] * Xv.z ) + P[ k ][ 3 ], k = 0, 1, 3 ( x, y, w )
//             uv = ( clip.x / clip.w * 0.5 + 0.5, clip.y / clip.w * -0.5 + 0.5 ), replaced by ( 99999, 99999 ) if clip.w < 0 ( GetScreenUv )
//   previous  Xp = positionPrev.xyz if the plane is given and its three components are finite, else X ( a static point )
//             Xvp, viewZp, uvp: the same of Xp with Rp, cp, Pp
//   motion    screen space:  mv.x = ( uvp.x - uv.x ) / s.x      mv.y = ( uvp.y - uv.y ) / s.y      mv.z = s.z != 0 ? ( abs( viewZp ) - abs( viewZ ) ) / s.z : 0
//             world space:   mv.i = s.i != 0 ? ( Xp.i - X.i ) / s.i : 0 ( absolute coordinates, no camera term )
//   store     outMv = ( mv.xyz, 0 ): a NaN component becomes 0, then clamped to +-65504, fp16 round-to-nearest-even.      outViewZ = viewZ
//   UNORM     floor( saturate( x ) * 255 + 0.5 ), saturate( NaN ) = 0 ( the HLSL rule );  outBaseColorMetalness = ( baseColor.rgb, metalness )
// The projection difference is taken unscaled on purpose: a jittered sample position cancels out of uvp - uv, and for a sample at the pixel centre uv is the pixelUv the passes add
// the vector to. The matrices are the non-jittered ones CommonSettings asks for. outMv binds as IN_MV for THESE commonSettings (their motionVectorScale and mode).
// INVALID_ARGUMENT, naming the field: no output at all; outViewZ / outMv without position or commonSettings, a UNORM output without its input(s); an input without any output
// that reads it (position without outViewZ / outMv, positionPrev without outMv, ...); a non-zero reserved; commonSettings.rectSize that is not the size of the planes; with
// outViewZ a missViewZ that is NaN / INF or for which !( abs( missViewZ * commonSettings.viewZScale ) > denoisingRange ) (it must satisfy the passes' own sky predicate); with
// outMv in screen-space mode s.x == 0 or s.y == 0; size, pitch and alignment mismatches as above. UNSUPPORTED: an orthographic projection (as everywhere else in this build);
// another format than listed.
typedef struct NrdHipGuidesDesc {
    const void* commonSettings;      // const nrd::CommonSettings* of the frame: required with outViewZ or outMv
    float missViewZ;                 // written to outViewZ where `position` is not finite (sky)
    uint32_t reserved;               // must be 0
    NrdHipPlaneDesc position;        // in,  RGBA32_SFLOAT or RGB32_SFLOAT (.xyz): world-space position of the primary hit (or of the PSR's virtual position)
    NrdHipPlaneDesc positionPrev;    // in,  same formats, optional: where that surface point was in the previous frame, previous world space; absent = static scene
    NrdHipPlaneDesc baseColor;       // in,  RGBA32_SFLOAT or RGB32_SFLOAT (.rgb)
    NrdHipPlaneDesc metalness;       // in,  R32_SFLOAT
    NrdHipPlaneDesc diffConfidence, specConfidence, disocclusionThresholdMix; // in, R32_SFLOAT
    NrdHipPlaneDesc outViewZ;        // out, R32_SFLOAT: unscaled view depth = `viewZ` of nrdHipPackInputs; binds as IN_VIEWZ when viewZScale is 1
    NrdHipPlaneDesc outMv;           // out, RGBA16_SFLOAT: binds as IN_MV for THESE commonSettings
    NrdHipPlaneDesc outBaseColorMetalness;                                     // out, RGBA8_UNORM (needs baseColor and metalness)
    NrdHipPlaneDesc outDiffConfidence, outSpecConfidence, outDisocclusionThresholdMix; // out, R8_UNORM (each needs its input)
} NrdHipGuidesDesc;
uint32_t nrdHipPackGuides(const NrdHipGuidesDesc* desc, void* hipStream);

#ifdef __cplusplus
static_assert(sizeof(NrdHipGuidesDesc) == 328, "mirrored by raytracingdenoiser_amd/api.py"); // 16 + 13 planes of 24 bytes
static_assert(sizeof(NrdHipShadowLight) == 16 && sizeof(NrdHipShadowLightsPackDesc) == 264 && sizeof(NrdHipShadowLightsResolveDesc) == 96, "mirrored by raytracingdenoiser_amd/api.py");
static_assert(sizeof(NrdHipFrontEndSplit) == 88 && sizeof(NrdHipBackEndSplit) == 48, "mirrored by raytracingdenoiser_amd/api.py");
static_assert(sizeof(NrdHipInputReport) == 72, "mirrored by raytracingdenoiser_amd/api.py");
static_assert(sizeof(NrdHipBackEndUpsample) == 56, "mirrored by raytracingdenoiser_amd/api.py"); // 2 planes of 24 bytes + 8
static_assert(sizeof(NrdHipFrontEndLobes) == 168, "mirrored by raytracingdenoiser_amd/api.py"); // 5 planes of 24 bytes + 8 + 5 strides
static_assert(sizeof(NrdHipDirectSignal) == 104 && sizeof(NrdHipFrontEndDirect) == 216, "mirrored by raytracingdenoiser_amd/api.py"); // 3 planes of 24 bytes + 3 strides + 8; two of them + 8
static_assert(sizeof(NrdHipCoverageDesc) == 88 && sizeof(NrdHipCoverageReport) == 28, "mirrored by raytracingdenoiser_amd/api.py");
#endif

#ifdef __cplusplus
}
#endif
