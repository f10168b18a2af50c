// nrd::IntegrationHip -- header-only C++ convenience layer over the HIP back-end's C-ABI (include/NRDHip.h), shaped like the
// reference integration class so that an application written against it changes types, not structure:
//
//   reference Integration/NRDIntegration.h:37-48   UserPool + Integration_SetResource        -> nrd::UserPoolHip + IntegrationHip_SetResource
//   reference Integration/NRDIntegration.h:50-81   IntegrationCreationDesc                    -> nrd::IntegrationHipCreationDesc
//   reference Integration/NRDIntegration.h:83-127  Integration::{Initialize, NewFrame, SetCommonSettings, SetDenoiserSettings,
//                                                  Denoise, Destroy, Get*MemoryUsageInMb}     -> same member names
//
// What differs, and why: textures are pitched device-memory planes (NrdHipPlaneDesc) instead of nri::TextureBarrierDesc, the
// "command buffer" is the hipStream_t given at Initialize (launches are asynchronous on it, in order), there are no barriers,
// descriptor pools or buffered-frame constants to manage (constants travel as kernel arguments), and pipelines need no creation step.
// Include after NRD.h and NRDHip.h. No HIP headers are needed: the stream is passed as void*.
#pragma once

#include <array>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#define NRD_INTEGRATION_HIP_MAJOR 1
#define NRD_INTEGRATION_HIP_MINOR 0

#ifndef NRD_INTEGRATION_ASSERT
#    include <assert.h>
#    define NRD_INTEGRATION_ASSERT(expr, msg) assert(msg && expr)
#endif

namespace nrd {

// One entry per ResourceType slot (the two pool pseudo-slots excluded, as in the reference). Zero-initialise; fill the slots the
// requested denoisers need (NRDDescs.h lists them per denoiser).
// With an executor of several layers (IntegrationHipCreationDesc::layersNum > 1) a per-layer slot -- IN_PENUMBRA, IN_TRANSLUCENCY, OUT_SHADOW_TRANSLUCENCY -- holds a stack of
// planes: its entry describes layer 0 and layerBytes[ slot ] is the distance in bytes from one layer to the next (NRDHip.h nrdHipBindResourceLayers); 0 = a plain plane.
struct UserPoolHip : std::array<NrdHipPlaneDesc, (size_t)ResourceType::MAX_NUM - 2> {
    std::array<uint64_t, (size_t)ResourceType::MAX_NUM - 2> layerBytes = {};
};

inline void IntegrationHip_SetResource(UserPoolHip& pool, ResourceType slot, const NrdHipPlaneDesc& plane) {
    NRD_INTEGRATION_ASSERT(plane.data != nullptr, "Invalid plane!");
    pool[(size_t)slot] = plane;
    pool.layerBytes[(size_t)slot] = 0;
}

inline void IntegrationHip_SetResourceLayers(UserPoolHip& pool, ResourceType slot, const NrdHipPlaneDesc& layer0, uint64_t layerBytes) {
    NRD_INTEGRATION_ASSERT(layer0.data != nullptr && layerBytes != 0, "Invalid stack of planes!");
    pool[(size_t)slot] = layer0;
    pool.layerBytes[(size_t)slot] = layerBytes;
}

struct IntegrationHipCreationDesc {
    const char* name = "";
    uint16_t resourceWidth = 0;
    uint16_t resourceHeight = 0;
    void* hipStream = nullptr; // hipStream_t; nullptr = the default stream
    // Optional caller-owned pool memory ("NRD allocates no GPU memory"): at least nrdHipGetArenaSize() bytes, 256-byte aligned.
    void* arena = nullptr;
    uint64_t arenaSize = 0;
    // SIGMA for many lights (NRDHip.h "layered executor"): > 1 = that many shadow layers, one per light, denoised by one pass chain of an instance of SIGMA denoisers only.
    // The pool then belongs to the library (not with "arena"), and the per-layer slots of the user pool are stacks (IntegrationHip_SetResourceLayers).
    uint32_t layersNum = 1;
};

class IntegrationHip {
public:
    inline IntegrationHip() {}
    inline ~IntegrationHip() { NRD_INTEGRATION_ASSERT(m_Executor == nullptr, "Destroy() must be called before the destructor!"); }

    // There is no "Resize": recreate (Destroy + Initialize), exactly as with the reference integration.
    inline bool Initialize(const IntegrationHipCreationDesc& desc, const InstanceCreationDesc& instanceCreationDesc) {
        NRD_INTEGRATION_ASSERT(m_Instance == nullptr, "Already initialized! Did you forget to call 'Destroy'?");
        if (CreateInstance(instanceCreationDesc, m_Instance) != Result::SUCCESS)
            return false;
        uint32_t r = desc.arena && desc.layersNum != 1 ? (uint32_t)Result::UNSUPPORTED // (a caller-provided arena stays unlayered)
                     : desc.arena ? nrdHipCreateExecutorWithArena(m_Instance, desc.resourceWidth, desc.resourceHeight, desc.hipStream, desc.arena, desc.arenaSize, &m_Executor)
                                  : nrdHipCreateExecutorLayered(m_Instance, desc.resourceWidth, desc.resourceHeight, desc.layersNum, desc.hipStream, &m_Executor);
        if (r != (uint32_t)Result::SUCCESS) {
            DestroyInstance(*m_Instance);
            m_Instance = nullptr;
            m_Executor = nullptr;
            return false;
        }
        m_Name = desc.name;
        m_Stream = desc.hipStream;
        m_FrameIndex = 0;
        nrdHipGetPoolMemoryUsage(m_Executor, &m_PermanentPoolSize, &m_TransientPoolSize);
        return true;
    }

    // Must be called once on a frame start (kept for call-order compatibility; nothing is buffered per frame here)
    inline void NewFrame() {
        NRD_INTEGRATION_ASSERT(m_Instance != nullptr, "Uninitialized! Did you forget to call 'Initialize'?");
        m_FrameIndex++;
        m_CheckedDispatches = nullptr; // a list "CheckInputs" fetched for a frame that was never denoised is stale
    }

    // Explicitly call the eponymous NRD API functions
    inline bool SetCommonSettings(const CommonSettings& commonSettings) {
        NRD_INTEGRATION_ASSERT(m_Instance != nullptr, "Uninitialized! Did you forget to call 'Initialize'?");
        m_CheckedDispatches = nullptr; // new settings: a list fetched before them no longer describes the frame
        return nrd::SetCommonSettings(*m_Instance, commonSettings) == Result::SUCCESS;
    }
    inline bool SetDenoiserSettings(Identifier denoiser, const void* denoiserSettings) {
        NRD_INTEGRATION_ASSERT(m_Instance != nullptr, "Uninitialized! Did you forget to call 'Initialize'?");
        m_CheckedDispatches = nullptr;
        return nrd::SetDenoiserSettings(*m_Instance, denoiser, denoiserSettings) == Result::SUCCESS;
    }

    // Enqueues the denoising passes of the given denoisers on the stream. Every non-null entry of "userPool" is (re)bound first;
    // entries with data == nullptr are left as they are. Returns false (and GetLastError() says why) if a permutation is not
    // supported by this build or a required slot is not bound -- nothing is launched in that case.
    inline bool Denoise(const Identifier* denoisers, uint32_t denoisersNum, const UserPoolHip& userPool) {
        NRD_INTEGRATION_ASSERT(m_Executor != nullptr, "Uninitialized! Did you forget to call 'Initialize'?");
        if (!BindPool(userPool))
            return false;
        if (m_CheckedDispatches && m_CheckedIdentifiers == std::vector<Identifier>(denoisers, denoisers + denoisersNum)) {
            // CheckInputs fetched this frame's list already (GetComputeDispatches advances the instance's ping-pong state: once per frame): execute that very list
            const DispatchDesc* descs = m_CheckedDispatches;
            m_CheckedDispatches = nullptr;
            return nrdHipExecuteDispatches(m_Executor, descs, m_CheckedDispatchesNum) == (uint32_t)Result::SUCCESS;
        }
        m_CheckedDispatches = nullptr;
        return nrdHipDenoise(m_Executor, denoisers, denoisersNum) == (uint32_t)Result::SUCCESS;
    }

    // Audits the inputs of the frame against NRD's input rules BEFORE it is denoised (NRDHip.h nrdHipCheckInputs: one launch, a stream synchronisation and a 72-byte
    // read-back): call after SetCommonSettings / SetDenoiserSettings, with the pool "Denoise" will get. report.count[ rule ] / report.first[ rule ] say which rule of
    // NRD_HIP_INPUT_RULE_* fails and where; *rulesChecked (optional) which rules applied. Returns false (GetLastError() says why) on an argument error only -- a violation
    // is a report, not a failure; "IsClean" below folds it into a bool. The frame's dispatch list is fetched here, and the "Denoise" of the same denoisers that follows executes
    // it -- unless "SetCommonSettings", "SetDenoiserSettings" or "NewFrame" came in between: they drop it, and "Denoise" fetches the list of the frame it is called for. A fetched
    // list is meant to be executed: a frame that is checked and then dropped has still advanced the ping-pong planes (as any unexecuted GetComputeDispatches does), so restart
    // the accumulation (AccumulationMode::RESTART) on the next one. A host that calls nrd::GetComputeDispatches on GetInstance() itself between the two calls overwrites the list.
    inline bool CheckInputs(const Identifier* denoisers, uint32_t denoisersNum, const UserPoolHip& userPool, NrdHipInputReport& report, uint32_t* rulesChecked = nullptr) {
        uint32_t mask = 0;
        if (!FetchForCheck(denoisers, denoisersNum, userPool))
            return false;
        const bool ok = nrdHipCheckInputs(m_Executor, m_CheckedDispatches, m_CheckedDispatchesNum, &report, &mask) == (uint32_t)Result::SUCCESS;
        if (ok && rulesChecked)
            *rulesChecked = mask;
        return ok;
    }
    // The same audit without the host round trip (nrdHipCheckInputsAsync): sizeof( NrdHipInputReport ) bytes of the caller's device memory are filled in stream order
    inline bool CheckInputsAsync(const Identifier* denoisers, uint32_t denoisersNum, const UserPoolHip& userPool, void* deviceReport, uint32_t* rulesChecked = nullptr) {
        uint32_t mask = 0;
        if (!FetchForCheck(denoisers, denoisersNum, userPool))
            return false;
        const bool ok = nrdHipCheckInputsAsync(m_Executor, m_CheckedDispatches, m_CheckedDispatchesNum, deviceReport, &mask) == (uint32_t)Result::SUCCESS;
        if (ok && rulesChecked)
            *rulesChecked = mask;
        return ok;
    }
    static inline bool IsClean(const NrdHipInputReport& report) {
        uint32_t n = 0;
        for (uint32_t r = 0; r < NRD_HIP_INPUT_RULES_NUM; r++)
            n += report.count[r];
        return n == 0;
    }

    // Front end / back end on the device (NRDHip.h nrdHipPackInputs / nrdHipResolveOutputs) on this integration's stream: pack the application's fp32 buffers
    // into the planes "Denoise" consumes, resolve its outputs into linear radiance. Asynchronous; false + GetLastFrontEndError() on an invalid descriptor.
    inline bool PackInputs(const NrdHipFrontEndDesc& desc) { return nrdHipPackInputs(&desc, m_Stream) == (uint32_t)Result::SUCCESS; }
    inline bool ResolveOutputs(const NrdHipBackEndDesc& desc) { return nrdHipResolveOutputs(&desc, m_Stream) == (uint32_t)Result::SUCCESS; }
    // with options (nrdHipPackInputsEx / nrdHipResolveOutputsEx): checkerboarded noisy inputs, NRD_SG_ReJitter between the resolve and the remodulation
    inline bool PackInputs(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndOptions& options) { return nrdHipPackInputsEx(&desc, &options, m_Stream) == (uint32_t)Result::SUCCESS; }
    // many paths per pixel (nrdHipPackInputsSamples): N sample layers per signal, reduced by the reference's rules (specular hitT: NRD_FrontEnd_SpecHitDistAveraging_*) and packed in one launch
    inline bool PackInputs(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndOptions& options, const NrdHipFrontEndSamples& samples) {
        return nrdHipPackInputsSamples(&desc, &options, &samples, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    inline bool ResolveOutputs(const NrdHipBackEndDesc& desc, const NrdHipBackEndOptions& options) { return nrdHipResolveOutputsEx(&desc, &options, m_Stream) == (uint32_t)Result::SUCCESS; }
    // three-channel and split planes in place (nrdHipPackInputsSplit / nrdHipResolveOutputsSplit): RGB32_SFLOAT planes, .w (roughness, hit distance) in R32_SFLOAT planes of their own
    inline bool PackInputs(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndOptions& options, const NrdHipFrontEndSamples& samples, const NrdHipFrontEndSplit& split) {
        return nrdHipPackInputsSplit(&desc, &options, &samples, &split, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    inline bool ResolveOutputs(const NrdHipBackEndDesc& desc, const NrdHipBackEndOptions& options, const NrdHipBackEndSplit& split) {
        return nrdHipResolveOutputsSplit(&desc, &options, &split, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    // SIGMA for point, spot, sphere and directional lights, up to NRD_HIP_MAX_SHADOW_LIGHTS per pixel (nrdHipPackShadowLights / nrdHipResolveShadowLights): IN_PENUMBRA /
    // IN_TRANSLUCENCY per light, or combined for one SIGMA_SHADOW_TRANSLUCENCY pass; then the shadowed radiance of all lights from the denoised OUT_SHADOW_TRANSLUCENCY
    inline bool PackShadowLights(const NrdHipShadowLightsPackDesc& desc) { return nrdHipPackShadowLights(&desc, m_Stream) == (uint32_t)Result::SUCCESS; }
    inline bool ResolveShadowLights(const NrdHipShadowLightsResolveDesc& desc) { return nrdHipResolveShadowLights(&desc, m_Stream) == (uint32_t)Result::SUCCESS; }
    // IN_VIEWZ and IN_MV from world-space hit positions and the matrices of the frame's CommonSettings, and the optional UNORM guide slots from fp32 planes (nrdHipPackGuides)
    inline bool PackGuides(const NrdHipGuidesDesc& desc) { return nrdHipPackGuides(&desc, m_Stream) == (uint32_t)Result::SUCCESS; }
    // Quarter-resolution tracing and denoising (nrdHipPackInputsDecimated / nrdHipResolveOutputsUpsampled): the G-buffer planes of the pack are full-size and read at every second
    // texel, everything traced and every packed plane has the low size ( ( W + 1 ) >> 1 ) x ( ( H + 1 ) >> 1 ), for an instance recreated at that size; the resolve brings the low
    // OUT_* planes back to the full-size frame by nearest-Z upsampling. options / samples / split may be NULL
    inline bool PackInputsDecimated(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndOptions* options = nullptr, const NrdHipFrontEndSamples* samples = nullptr,
        const NrdHipFrontEndSplit* split = nullptr, uint32_t guideShift = 1) {
        return nrdHipPackInputsDecimated(&desc, options, samples, split, guideShift, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    inline bool ResolveOutputsUpsampled(const NrdHipBackEndDesc& desc, const NrdHipBackEndUpsample& upsample, const NrdHipBackEndOptions* options = nullptr, const NrdHipBackEndSplit* split = nullptr) {
        return nrdHipResolveOutputsUpsampled(&desc, options, split, &upsample, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    // One traced lobe per pixel, the probabilistic diffuse / specular split of the README's "NOISY INPUTS" (nrdHipPackInputsLobes): both signals from ONE traced plane set, a lobe
    // byte and a probability. options / split may be NULL. Set "hitDistanceReconstructionMode" and the pre-pass radii of the denoiser: the signal that was not traced has hit distance 0
    inline bool PackInputsLobes(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndLobes& lobes, const NrdHipFrontEndOptions* options = nullptr, const NrdHipFrontEndSplit* split = nullptr) {
        return nrdHipPackInputsLobes(&desc, options, split, &lobes, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    // Combined denoising of direct and indirect lighting, the README's "GREATER TIPS" rule (nrdHipPackInputsDirect): the descriptor's signal planes are the INDIRECT ones, "direct"
    // holds the direct ones; the radiance is summed, the specular hit distance stays the indirect one, the diffuse one is mixed by the direct share of the luminance, capped by
    // direct.maxHitDistContribution (NRD_HIP_DIRECT_MAX_CONTRIBUTION_DEFAULT). options / samples / split may be NULL; guideShift as in "PackInputsDecimated", default 0
    inline bool PackInputsDirect(const NrdHipFrontEndDesc& desc, const NrdHipFrontEndDirect& direct, const NrdHipFrontEndOptions* options = nullptr, const NrdHipFrontEndSamples* samples = nullptr,
        const NrdHipFrontEndSplit* split = nullptr, uint32_t guideShift = 0) {
        return nrdHipPackInputsDirect(&desc, options, samples, split, &direct, guideShift, m_Stream) == (uint32_t)Result::SUCCESS;
    }
    // ... and the audit of the dithering that chose the lobes (nrdHipCheckHitDistCoverage): sizeof( NrdHipCoverageReport ) bytes of the caller's device memory are filled in stream
    // order; holes[ s ] != 0 = pixels of signal s with no valid hit distance in the area the reconstruction searches
    inline bool CheckHitDistCoverage(const NrdHipCoverageDesc& desc, void* deviceReport) { return nrdHipCheckHitDistCoverage(&desc, deviceReport, m_Stream) == (uint32_t)Result::SUCCESS; }
    inline const char* GetLastFrontEndError() const { return nrdHipGetLastFrontEndError(); }

    // Assumes that no work of this integration is in flight on the stream
    inline void Destroy() {
        if (m_Executor)
            nrdHipDestroyExecutor(m_Executor);
        if (m_Instance)
            DestroyInstance(*m_Instance);
        m_Executor = nullptr;
        m_Instance = nullptr;
        m_PermanentPoolSize = m_TransientPoolSize = 0;
    }

    // Helpers
    inline double GetTotalMemoryUsageInMb() const { return double(m_PermanentPoolSize + m_TransientPoolSize) / (1024.0 * 1024.0); }
    inline double GetPersistentMemoryUsageInMb() const { return double(m_PermanentPoolSize) / (1024.0 * 1024.0); }
    inline double GetAliasableMemoryUsageInMb() const { return double(m_TransientPoolSize) / (1024.0 * 1024.0); }
    inline const char* GetLastError() const { return m_Executor ? nrdHipGetLastError(m_Executor) : "not initialized"; }
    inline Instance* GetInstance() const { return m_Instance; }
    inline NrdHipExecutor* GetExecutor() const { return m_Executor; }

private:
    IntegrationHip(const IntegrationHip&) = delete;

    // every non-null entry of the pool: a stack of per-layer planes where the pool gives a layer stride, a plain plane otherwise
    inline bool BindPool(const UserPoolHip& userPool) {
        for (size_t slot = 0; slot < userPool.size(); slot++) {
            if (!userPool[slot].data)
                continue;
            const uint32_t r = userPool.layerBytes[slot] ? nrdHipBindResourceLayers(m_Executor, (uint32_t)slot, &userPool[slot], userPool.layerBytes[slot])
                                                         : nrdHipBindResource(m_Executor, (uint32_t)slot, &userPool[slot]);
            if (r != (uint32_t)Result::SUCCESS)
                return false;
        }
        return true;
    }

    inline bool FetchForCheck(const Identifier* denoisers, uint32_t denoisersNum, const UserPoolHip& userPool) {
        NRD_INTEGRATION_ASSERT(m_Executor != nullptr, "Uninitialized! Did you forget to call 'Initialize'?");
        m_CheckedDispatches = nullptr;
        if (!BindPool(userPool))
            return false;
        const DispatchDesc* descs = nullptr;
        if (GetComputeDispatches(*m_Instance, denoisers, denoisersNum, descs, m_CheckedDispatchesNum) != Result::SUCCESS)
            return false;
        m_CheckedIdentifiers.assign(denoisers, denoisers + denoisersNum);
        m_CheckedDispatches = descs;
        return true;
    }

    const DispatchDesc* m_CheckedDispatches = nullptr; // the list "CheckInputs" fetched for the frame that "Denoise" has not executed yet
    uint32_t m_CheckedDispatchesNum = 0;
    std::vector<Identifier> m_CheckedIdentifiers;

    Instance* m_Instance = nullptr;
    NrdHipExecutor* m_Executor = nullptr;
    const char* m_Name = "";
    void* m_Stream = nullptr;
    uint64_t m_PermanentPoolSize = 0, m_TransientPoolSize = 0;
    uint32_t m_FrameIndex = 0;
};

} // namespace nrd
