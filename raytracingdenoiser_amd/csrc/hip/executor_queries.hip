// HIP executor, the entry points that inspect rather than denoise (include/NRDHip.h): the frame's motion reach, the input audit, pass timings, tile statistics, device probes.
#include "executor.h"

#include <cstring>

using namespace nrdhip;

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetLayersNum(const NrdHipExecutor* e, uint32_t* layersNum) {
    if (!e || !layersNum)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    *layersNum = e->layersNum;
    return (uint32_t)nrd::Result::SUCCESS;
}

// nrdHipGetPoolPlane describes layer 0; layer l of the same plane lies l x (its 256-byte aligned size) behind it
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetPoolPlaneLayer(NrdHipExecutor* e, uint32_t resourceType, uint32_t indexInPool, uint32_t layer, NrdHipPlaneDesc* plane) {
    if (!e || !plane)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    if (layer >= e->layersNum)
        return e->Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipGetPoolPlaneLayer: the executor has " + std::to_string(e->layersNum) + " layer(s)");
    const uint32_t r = nrdHipGetPoolPlane(e, resourceType, indexInPool, plane);
    if (r == (uint32_t)nrd::Result::SUCCESS)
        plane->data = (uint8_t*)plane->data + (uint64_t)layer * (resourceType == (uint32_t)nrd::ResourceType::PERMANENT_POOL ? e->permanentStride : e->transientStride)[indexInPool];
    return r;
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
static uint32_t EnqueueMotionRows(NrdHipExecutor* e, const void* dispatchDescs, uint32_t dispatchDescsNum, uint32_t rowBegin, uint32_t rowEnd, uint32_t* deviceWord, bool& found) {
    const ListScan s = ScanDispatchList(nrd::GetInstanceDesc(*e->instance), (const nrd::DispatchDesc*)dispatchDescs, dispatchDescsNum);
    MotionParams p = {};
    auto common = [&](const auto& c) {
        memcpy(p.worldToClipPrev, c.gWorldToClipPrev, sizeof(p.worldToClipPrev));
        const float mvScale[4] = {c.gMvScale.x, c.gMvScale.y, c.gMvScale.z, c.gMvScale.w};
        memcpy(p.mvScale, mvScale, sizeof(mvScale));
        p.rectSizeInv[0] = c.gRectSizeInv.x, p.rectSizeInv[1] = c.gRectSizeInv.y;
        p.rectHeightPrev = c.gRectSizePrev.y;
        p.viewZScale = c.gViewZScale, p.denoisingRange = c.gDenoisingRange;
        p.rectW = (int)c.gRectSize.x, p.rectH = (int)c.gRectSize.y;
    };
    auto frustum = [&](const auto& c) {
        const float f[4] = {c.gFrustum.x, c.gFrustum.y, c.gFrustum.z, c.gFrustum.w};
        memcpy(p.frustum, f, sizeof(f));
    };
    found = s.firstWithOrigin != Family::NONE;
    if (s.firstWithOrigin == Family::REBLUR) {
        common(*s.reblur);
        frustum(*s.reblur);
        memcpy(p.viewToWorld, s.reblur->gViewToWorld, sizeof(p.viewToWorld));
    } else if (s.firstWithOrigin == Family::RELAX) { // RELAX's block has no gFrustum / gViewToWorld: it rebuilds positions from three frustum vectors (passes.h MotionParams "RELAX form")
        const nrdc::RelaxConstants& c = *s.relax;
        common(c);
        p.relaxForm = 1;
        auto set = [](float* dst, const auto& v) { dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = 0.0f; };
        set(p.frustumRight, c.gFrustumRight);
        set(p.frustumUp, c.gFrustumUp);
        set(p.frustumForward, c.gFrustumForward);
    } else if (s.firstWithOrigin == Family::SIGMA) {
        common(*s.sigma);
        frustum(*s.sigma);
        for (int r = 0; r < 3; r++) // SIGMA's block has no gViewToWorld: view -> world = the transposed rotation of gWorldToView (column-major storage)
            for (int k = 0; k < 3; k++)
                p.viewToWorld[k * 4 + r] = s.sigma->gWorldToView[r * 4 + k];
    } else
        return (uint32_t)nrd::Result::SUCCESS; // no temporal denoiser in the list (REFERENCE, empty list): nothing reprojects
    const int originX = s.originX, originY = s.originY; // (of the block the parameters came from)
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
    if (e->layersNum > 1) // (the audit kernel reads one plane per slot: audit a layer through an unlayered executor with that layer's planes bound)
        return e->Fail(nrd::Result::UNSUPPORTED, "nrdHipCheckInputs: not on a layered executor; audit one layer through an unlayered executor");
    // the frame's rect, range and checkerboard: the first constant block of a pass family (every block of a list carries the same CommonSettings)
    const ListScan s = ScanDispatchList(nrd::GetInstanceDesc(*e->instance), (const nrd::DispatchDesc*)dispatchDescs, dispatchDescsNum);
    CheckInputsParams p = {};
    p.rectW = s.rectW, p.rectH = s.rectH;
    p.viewZScale = s.first == Family::RELAX ? 1.0f : s.viewZScale; // RELAX classifies its tiles by Abs( z ) > range (kernels_common.hip DecodeGuidesClassifyKernel)
    p.denoisingRange = s.denoisingRange, p.frameIndex = s.frameIndex;
    p.diffCell = s.diffCell, p.specCell = s.specCell;
    // the origin the guides are audited at comes from the same first block; REFERENCE's carries none (a later family's origin does not count)
    const int originX = s.first == s.firstWithOrigin ? s.originX : 0, originY = s.first == s.firstWithOrigin ? s.originY : 0;
    auto applies = [&](R t) { return s.named[(size_t)t] && IsFloatFormat(ExpectedUserFormat(t, e->translucentShadow)); };
    const bool diffRadiance = applies(R::IN_DIFF_RADIANCE_HITDIST), diffSh = applies(R::IN_DIFF_SH0), specRadiance = applies(R::IN_SPEC_RADIANCE_HITDIST), specSh = applies(R::IN_SPEC_SH0);
    if (s.first != Family::NONE) {
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
    p.diffNormalized = !s.namedOutsideReblur[(size_t)(diffSh ? R::IN_DIFF_SH0 : R::IN_DIFF_RADIANCE_HITDIST)];
    p.specNormalized = !s.namedOutsideReblur[(size_t)(specSh ? R::IN_SPEC_SH0 : R::IN_SPEC_RADIANCE_HITDIST)];

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

// always 0: the library has one arithmetic (DESIGN.md "Numerics"), bit-identical to the CPU oracle in device mode; kept for callers of the round-2 interface
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetNumericsMode(void) {
    return 0; // (the value 1 named the "fast" build of round 2, which no longer exists)
}

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
