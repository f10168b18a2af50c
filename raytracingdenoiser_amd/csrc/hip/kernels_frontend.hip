// Front end / back end on the device (include/NRDHip.h nrdHipPackInputs / nrdHipResolveOutputs): the application side of the reference's NRD.hlsli as two
// fused streaming kernels -- one launch packs a frame's fp32 G-buffer and noisy signals into the planes nrdHipBindResource accepts, one launch turns the
// denoised OUT_* planes into linear fp32 radiance. One thread per pixel, 64 x 4 workgroups: a wave covers 64 consecutive pixels of one row, so every load
// and store of a wave is one contiguous segment (16 B per lane for the RGBA32_SFLOAT inputs: global_load_dwordx4). The calls with options (nrdHipPackInputsEx /
// nrdHipResolveOutputsEx) launch these very kernels when the options are absent or zero, else one of two more: the checkerboard twin of the pack kernel and the re-jitter kernel.
// nrdHipPackInputsSplit / nrdHipResolveOutputsSplit launch the kernels of those calls when every plane is RGBA32_SFLOAT, else the split twin of the kernel the call would have
// taken: the same body instantiated with SPLIT = true, in which a colour / vector plane may hold 12-byte RGB32_SFLOAT texels (global_load_dwordx3 / global_store_dwordx3,
// never a 16-byte access) and `.w` lives in an R32_SFLOAT plane of its own.
// nrdHipPackInputsDecimated / nrdHipResolveOutputsUpsampled (quarter-resolution tracing) launch the kernels of the split calls when nothing is decimated / upsampled, else a
// DECIMATED instantiation of the pack body (the G-buffer planes read at every second texel) and the two upsampling resolve kernels (nearest Z among the low texels around a pixel).
// nrdHipPackInputsLobes (one traced lobe per sample: the probabilistic diffuse / specular split) launches the kernels of the split call when `lobes` is NULL, else the LOBES
// instantiation of the pack body: both signals built from one traced plane set, each traced byte loaded once. (Its audit, nrdHipCheckHitDistCoverage: kernels_coverage.hip.)
// nrdHipPackInputsDirect (combined direct and indirect lighting) launches the kernels of the decimated call when no signal has a direct plane, else a DIRECT instantiation of the
// pack body in its samples + split form: a signal with a direct plane adds the packed direct term to its packed indirect samples and mixes the diffuse hit distance.
//
// Arithmetic: include/NRD.hip.h and nothing else -- its contract, and the reference text it is pinned to, is unfused IEEE fp32 with correctly rounded
// division and square root. The product builds its device sources with -ffp-contract=on, hence the pragma below, in front of every include: no statement
// of this translation unit is contracted. No v_rcp / v_rsq / v_exp / v_log forms, no nrdmath.h, no fast-math. The stores are the codecs of the passes (planes.h).
#pragma clang fp contract(off)

#include "NRD.h"
#include "NRDHip.h"

#include "NRD.hip.h"

#include "planes.h"
#include "frontend_host.h"

#include "../host/hostmath.h"

#include <cstdio>
#include <string>

using namespace nrdhip;

namespace {

// camera of the view vector (NRDHip.h): frustum and the rotation rows of view-to-world, as the denoisers' constants hold them
struct FeCamera {
    float4 frustum;
    float4 row0, row1, row2;
};

struct PackArgs {
    FePlane normalRoughness, viewZ, materialID, motion, albedo, rf0, occluder, translucency;
    FePlane diffIn, diffDir, diffOut0, diffOut1, specIn, specDir, specOut0, specOut1;
    FePlane outNormalRoughness, outViewZ, outMv, outPenumbra, outTranslucency;
    FeCamera camera;
    float4 hitDistParams;
    float viewZScale, tanOfLightAngularRadius;
    int32_t w, h;
    uint32_t diffMode, specMode, motionIsRG, demodulate;
};

// nrdHipPackInputsSamples: sample layer s of a signal's fp32 planes starts s x layer bytes behind the plane of PackArgs (64-bit: a stack of layers may exceed 4 GiB)
struct SampleArgs {
    uint64_t diffInLayer, diffDirLayer, specInLayer, specDirLayer;
    uint32_t diffNum, specNum; // >= 1
    float trim;                // > 0: NRD_FrontEnd_TrimHitDistance on every sample's hit distance
};

// nrdHipPackInputsSplit: which fp32 planes of PackArgs hold 12-byte RGB32_SFLOAT texels (a bit each), and the R32_SFLOAT planes `.w` comes from instead. A signal whose
// kSplit*In bit is set takes its hit distance from its companion (its own plane is RGB32_SFLOAT, or absent in the occlusion mode); all of it is uniform: scalar branches
enum : uint32_t {
    kSplitNormalRoughness = 1u << 0, kSplitMotion = 1u << 1, kSplitAlbedo = 1u << 2, kSplitRf0 = 1u << 3, kSplitTranslucency = 1u << 4,
    kSplitDiffIn = 1u << 5, kSplitDiffDir = 1u << 6, kSplitSpecIn = 1u << 7, kSplitSpecDir = 1u << 8,
    // nrdHipResolveOutputsSplit: the outputs (kSplitAlbedo / kSplitRf0 are its inputs)
    kSplitDiffOut = 1u << 9, kSplitSpecOut = 1u << 10, kSplitComposed = 1u << 11, kSplitViewVector = 1u << 12, kSplitDiffFactor = 1u << 13, kSplitSpecFactor = 1u << 14,
    // nrdHipPackInputsLobes: the traced planes of NrdHipFrontEndLobes (host side only: the kernel gets their texel sizes in LobeArgs)
    kSplitLobeIn = 1u << 15, kSplitLobeDir = 1u << 16,
    // nrdHipPackInputsDirect: the direct planes of NrdHipFrontEndDirect (host side only: the kernel gets their texel sizes in DirectSignal)
    kSplitDirectDiffIn = 1u << 17, kSplitDirectDiffDir = 1u << 18, kSplitDirectSpecIn = 1u << 19, kSplitDirectSpecDir = 1u << 20
};
struct SplitArgs {
    FePlane roughness, diffHitDist, specHitDist;
    uint64_t diffHitDistLayer, specHitDistLayer; // sample layers of the two companions (SampleArgs rules)
    uint32_t rgb;                                // kSplit* bits
};
// nrdHipPackInputsLobes: the ONE traced plane set both signals are built from (their own planes of PackArgs are absent), and where sample layer s of each plane starts
struct LobeArgs {
    FePlane in, hitDist, dir, lobe, prob; // in: absent when both modes read .w only; hitDist: `.w` of an RGB32_SFLOAT `in`; dir: absent unless a mode reads it; prob: optional
    uint64_t inLayer, hitDistLayer, dirLayer, lobeLayer, probLayer;
    uint32_t num;               // >= 1
    uint32_t inBytes, dirBytes; // 12 or 16
};

// nrdHipPackInputsDirect: the direct planes of one signal (in absent: the signal has no direct term and is packed by the code of the other kernels) and their layers
struct DirectSignal {
    FePlane in, hitDist, dir; // hitDist: `.w` of an RGB32_SFLOAT `in`, diffuse signal with maxContribution > 0 only; dir: the SH modes
    uint64_t inLayer, hitDistLayer, dirLayer;
    uint32_t num;               // 1 (one direct texel under every sample) or the signal's own sample count
    uint32_t inBytes, dirBytes; // 12 or 16
};
struct DirectArgs {
    DirectSignal diff, spec;
    float maxContribution;  // 0: the diffuse hit distance stays the indirect one, no direct hit distance is consumed
    uint32_t multiSample;   // the call without `direct` would take the samples kernels (else: the plain ones, whose specular hit distance is not run through the averaging rule)
};

struct ResolveSplitArgs {
    FePlane diffHitDist, specHitDist; // optional: `.w` of an RGB32_SFLOAT diffOut / specOut
    uint32_t rgb;
};

struct ResolveArgs {
    FePlane normalRoughness, viewZ, albedo, rf0;
    FePlane diffIn0, diffIn1, diffOut, specIn0, specIn1, specOut;
    FePlane shadow, outShadow, outComposed, outViewVector, outDiffFactor, outSpecFactor;
    FeCamera camera;
    float4 hitDistParams;
    int32_t w, h;
    uint32_t diffMode, specMode, diffResolve, specResolve, diffWide, specWide; // wide: the in planes are RGBA32_SFLOAT
    uint32_t denormalize, remodulate, needV, needFactors, shadowIsRGBA;
};

__device__ __forceinline__ Plane AsPlane(const FePlane& p, int w, int h) { return Plane{p.ptr, p.pitch, w, h}; }
__device__ __forceinline__ float3 Xyz(float4 v) { return make_float3(v.x, v.y, v.z); }

// ---- the loads and stores of the split twins (nrdHipPackInputsSplit / nrdHipResolveOutputsSplit); with SPLIT = false each of them is the access the plain kernels make
__device__ __forceinline__ uint32_t SplitTexelBytes(uint32_t rgb, uint32_t bit) { return (rgb & bit) ? 12u : 16u; }
// a plane of which .xyz alone is consumed (albedo, rf0, translucency, direction): 12 bytes per lane whatever the texel size
template <bool SPLIT>
__device__ __forceinline__ float3 LoadColour(const FePlane& p, uint32_t rgb, uint32_t bit, int x, int y, int w, int h) {
    return SPLIT ? LoadXyz32F(AsPlane(p, w, h), x, y, SplitTexelBytes(rgb, bit)) : Xyz(LoadRGBA32F(AsPlane(p, w, h), x, y));
}
// a plane consumed whole: one 16-byte load, or 12 bytes + the companion's dword. needXyz = false (a mode that reads .w only): the split form reads the companion alone
template <bool SPLIT>
__device__ __forceinline__ float4 LoadTexel(const FePlane& p, const FePlane& companion, uint32_t rgb, uint32_t bit, bool needXyz, int x, int y, int w, int h) {
    if (SPLIT && (rgb & bit)) {
        const float3 c = needXyz ? LoadRGB32F(AsPlane(p, w, h), x, y) : make_float3(0.0f, 0.0f, 0.0f);
        return make_float4(c.x, c.y, c.z, LoadR32F(AsPlane(companion, w, h), x, y));
    }
    return LoadRGBA32F(AsPlane(p, w, h), x, y);
}
// an fp32 colour output: 16 bytes, or 12 bytes + .w to the companion where one is given (dropped otherwise)
template <bool SPLIT>
__device__ __forceinline__ void StoreTexel(const FePlane& p, const FePlane& companion, uint32_t rgb, uint32_t bit, int x, int y, int w, int h, float4 c) {
    if (SPLIT && (rgb & bit)) {
        StoreRGB32F(AsPlane(p, w, h), x, y, Xyz(c));
        if (companion.ptr)
            StoreR32F(AsPlane(companion, w, h), x, y, c.w);
    } else
        StoreRGBA32F(AsPlane(p, w, h), x, y, c);
}

// V of NRDHip.h: only correctly rounded + - * / sqrt in a fixed order (a float32 numpy restatement is bit-exact)
__device__ __forceinline__ float3 ViewVector(const FeCamera& c, int x, int y, int w, int h, float viewZ) {
    const float u = (float(x) + 0.5f) / float(w);
    const float v = (float(y) + 0.5f) / float(h);
    const float xv = (u * c.frustum.z + c.frustum.x) * viewZ;
    const float yv = (v * c.frustum.w + c.frustum.y) * viewZ;
    const float3 Xw = make_float3((c.row0.x * xv + c.row0.y * yv) + c.row0.z * viewZ, (c.row1.x * xv + c.row1.y * yv) + c.row1.z * viewZ, (c.row2.x * xv + c.row2.y * yv) + c.row2.z * viewZ);
    const float3 n = nrd_hip_detail::normalize(Xw);
    return make_float3(-n.x, -n.y, -n.z);
}

// (x, y): the pixel whose data is packed; the texels go to column xo of its row (xo = x, or x >> 1 of a checkerboarded frame)
template <bool SPEC, bool SPLIT>
__device__ __forceinline__ void PackSignal(uint32_t mode, const FePlane& in, const FePlane& dirPlane, const FePlane& out0, const FePlane& out1, const FePlane& hitDistPlane, uint32_t rgb,
    int x, int xo, int y, int w, int h, float viewZ, float roughness, float4 hitDistParams, bool demodulate, float3 factor) {
    const float4 s = LoadTexel<SPLIT>(in, hitDistPlane, rgb, SPEC ? kSplitSpecIn : kSplitDiffIn, mode != NRD_HIP_SIGNAL_REBLUR_OCCLUSION && mode != NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION,
        x, y, w, h);
    float3 radiance = Xyz(s);
    if (demodulate)
        radiance = make_float3(radiance.x / factor.x, radiance.y / factor.y, radiance.z / factor.z);
    const float hitDist = s.w;
    const float r = SPEC ? roughness : 1.0f;
    const bool needsDirection = mode == NRD_HIP_SIGNAL_REBLUR_SH || mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION || mode == NRD_HIP_SIGNAL_RELAX_SH;
    float3 direction = make_float3(0.0f, 0.0f, 0.0f);
    if (needsDirection)
        direction = LoadColour<SPLIT>(dirPlane, rgb, SPEC ? kSplitSpecDir : kSplitDiffDir, x, y, w, h);
    const Plane o0 = AsPlane(out0, w, h), o1 = AsPlane(out1, w, h);
    float4 p1;
    switch (mode) { // wave-uniform: a kernel argument
        case NRD_HIP_SIGNAL_REBLUR_RADIANCE:
            StoreRGBA16F(o0, xo, y, REBLUR_FrontEnd_PackRadianceAndNormHitDist(radiance, REBLUR_FrontEnd_GetNormHitDist(hitDist, viewZ, hitDistParams, r), true));
            break;
        case NRD_HIP_SIGNAL_REBLUR_SH:
            StoreRGBA16F(o0, xo, y, REBLUR_FrontEnd_PackSh(radiance, REBLUR_FrontEnd_GetNormHitDist(hitDist, viewZ, hitDistParams, r), direction, p1, true));
            StoreRGBA16F(o1, xo, y, p1);
            break;
        case NRD_HIP_SIGNAL_REBLUR_OCCLUSION: // the hit distance channel of the radiance packer, sanitised by it (NaN / inf -> 0)
            StoreR16Unorm(o0, xo, y, REBLUR_FrontEnd_PackRadianceAndNormHitDist(make_float3(0.0f, 0.0f, 0.0f), REBLUR_FrontEnd_GetNormHitDist(hitDist, viewZ, hitDistParams, r), true).w);
            break;
        case NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION:
            StoreRGBA16Snorm(o0, xo, y, REBLUR_FrontEnd_PackDirectionalOcclusion(direction, REBLUR_FrontEnd_GetNormHitDist(hitDist, viewZ, hitDistParams, r), true));
            break;
        case NRD_HIP_SIGNAL_RELAX_RADIANCE:
            StoreRGBA16F(o0, xo, y, RELAX_FrontEnd_PackRadianceAndHitDist(radiance, hitDist, true));
            break;
        case NRD_HIP_SIGNAL_RELAX_SH:
            StoreRGBA16F(o0, xo, y, RELAX_FrontEnd_PackSh(radiance, hitDist, direction, p1, true));
            StoreRGBA16F(o1, xo, y, p1);
            break;
        default:
            break;
    }
}

// ---- many paths per pixel (nrdHipPackInputsSamples; the per-pixel rules are spelled out in NRDHip.h) ---------------------------------------------------
// P_s of one sample: the fp32 texels the mode's packer returns, before the store codec. The specular signal takes its hit-distance channel from PackedHitDist
// of the reduced value instead, so its samples are packed with a hit distance of 0 and that channel of the sum is never read.
template <bool SPEC, uint32_t MODE>
__device__ __forceinline__ float4 PackSample(float3 radiance, float hitDist, float3 direction, float viewZ, float r, float4 hitDistParams, float4& p1) {
    constexpr bool kReblur = MODE != NRD_HIP_SIGNAL_RELAX_RADIANCE && MODE != NRD_HIP_SIGNAL_RELAX_SH;
    const float hd = SPEC ? 0.0f : kReblur ? REBLUR_FrontEnd_GetNormHitDist(hitDist, viewZ, hitDistParams, r) : hitDist;
    if (MODE == NRD_HIP_SIGNAL_REBLUR_RADIANCE)
        return REBLUR_FrontEnd_PackRadianceAndNormHitDist(radiance, hd, true);
    if (MODE == NRD_HIP_SIGNAL_REBLUR_SH)
        return REBLUR_FrontEnd_PackSh(radiance, hd, direction, p1, true);
    if (MODE == NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        return REBLUR_FrontEnd_PackRadianceAndNormHitDist(make_float3(0.0f, 0.0f, 0.0f), hd, true);
    if (MODE == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        return REBLUR_FrontEnd_PackDirectionalOcclusion(direction, hd, true);
    if (MODE == NRD_HIP_SIGNAL_RELAX_RADIANCE)
        return RELAX_FrontEnd_PackRadianceAndHitDist(radiance, hd, true);
    return RELAX_FrontEnd_PackSh(radiance, hd, direction, p1, true);
}

// the hit-distance channel the mode's packer writes for the single hit distance H (specular signal): normalised once (REBLUR) or clamped by RELAX's packer
template <uint32_t MODE>
__device__ __forceinline__ float PackedHitDist(float H, float viewZ, float r, float4 hitDistParams) {
    float4 unused;
    const float3 zero = make_float3(0.0f, 0.0f, 0.0f);
    if (MODE == NRD_HIP_SIGNAL_RELAX_RADIANCE)
        return RELAX_FrontEnd_PackRadianceAndHitDist(zero, H, true).w;
    if (MODE == NRD_HIP_SIGNAL_RELAX_SH)
        return RELAX_FrontEnd_PackSh(zero, H, zero, unused, true).w;
    const float normHitDist = REBLUR_FrontEnd_GetNormHitDist(H, viewZ, hitDistParams, r);
    if (MODE == NRD_HIP_SIGNAL_REBLUR_SH)
        return REBLUR_FrontEnd_PackSh(zero, normHitDist, zero, unused, true).w;
    return REBLUR_FrontEnd_PackRadianceAndNormHitDist(zero, normHitDist, true).w;
}

struct SampleSums {
    float4 p0, p1;
    float specHitDist; // the accumulator of NRD_FrontEnd_SpecHitDistAveraging_*
};

template <bool SPEC, uint32_t MODE>
__device__ __forceinline__ void AddSample(SampleSums& sums, float4 s, float4 d, float trim, float viewZ, float r, float4 hitDistParams, bool demodulate, float3 factor) {
    float3 radiance = Xyz(s);
    float hitDist = s.w;
    if (trim > 0.0f)
        hitDist = NRD_FrontEnd_TrimHitDistance(hitDist, trim);
    if (demodulate)
        radiance = make_float3(radiance.x / factor.x, radiance.y / factor.y, radiance.z / factor.z);
    if (SPEC)
        NRD_FrontEnd_SpecHitDistAveraging_Add(sums.specHitDist, hitDist);
    float4 p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 p0 = PackSample<SPEC, MODE>(radiance, hitDist, Xyz(d), viewZ, r, hitDistParams, p1);
    sums.p0 = make_float4(sums.p0.x + p0.x, sums.p0.y + p0.y, sums.p0.z + p0.z, sums.p0.w + p0.w);
    sums.p1 = make_float4(sums.p1.x + p1.x, sums.p1.y + p1.y, sums.p1.z + p1.z, sums.p1.w + p1.w);
}

// ---- combined direct and indirect lighting (nrdHipPackInputsDirect; the per-pixel rules are spelled out in NRDHip.h) ---------------------------------------------------
// the packers' own first line
__device__ __forceinline__ float3 SanitizedRadiance(float3 r) { return _NRD_IsInvalid(r) ? make_float3(0.0f, 0.0f, 0.0f) : nrd_hip_detail::clamp(r, 0.0f, NRD_FP16_MAX); }
__device__ __forceinline__ float ClampToHalfRange(float v) { return fminf(fmaxf(v, -NRD_FP16_MAX), NRD_FP16_MAX); }
// C = clamp( P_i + P_d ): the store codec never rounds a sum of two clamped terms to infinity. keepW: .w carries the hit distance and is not a sum
__device__ __forceinline__ float4 AddClamped(float4 a, float4 b, bool keepW) {
    return make_float4(ClampToHalfRange(a.x + b.x), ClampToHalfRange(a.y + b.y), ClampToHalfRange(a.z + b.z), keepW ? a.w : ClampToHalfRange(a.w + b.w));
}

// what one direct texel contributes: P_d, and ( h_d, L_d ) for the diffuse hit distance
struct DirectTerm {
    float4 p0, p1;
    float hitDist, lum;
};
// t: the direct texel ( .w consumed only with needHitDist: it may hold anything otherwise ), d: its direction
template <bool SPEC, uint32_t MODE>
__device__ __forceinline__ DirectTerm PackDirectTerm(float4 t, float4 d, bool needHitDist, float trim, float viewZ, float r, float4 hitDistParams, bool demodulate, float3 factor) {
    float3 radiance = Xyz(t);
    float hitDist = needHitDist ? t.w : 0.0f;
    if (trim > 0.0f)
        hitDist = NRD_FrontEnd_TrimHitDistance(hitDist, trim);
    if (demodulate)
        radiance = make_float3(radiance.x / factor.x, radiance.y / factor.y, radiance.z / factor.z);
    DirectTerm term;
    term.p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    term.p0 = PackSample<SPEC, MODE>(radiance, 0.0f, Xyz(d), viewZ, r, hitDistParams, term.p1);
    term.hitDist = hitDist;
    term.lum = _NRD_Luminance(SanitizedRadiance(radiance));
    return term;
}

// AddSample of a signal with a direct term. perSample: the term is this sample's own and is added here (else it is added once, to the mean: ReduceSignal); mix: the diffuse
// hit distance takes the direct one in; averaging: the specular hit distance goes through NRD_FrontEnd_SpecHitDistAveraging_* (else there is one sample and it is kept as it is)
template <bool SPEC, uint32_t MODE>
__device__ __forceinline__ void AddSampleDirect(SampleSums& sums, float4 s, float4 d, const DirectTerm& term, bool perSample, bool mix, bool averaging, float maxContribution, float trim, float viewZ,
    float r, float4 hitDistParams, bool demodulate, float3 factor) {
    float3 radiance = Xyz(s);
    float hitDist = s.w;
    if (trim > 0.0f)
        hitDist = NRD_FrontEnd_TrimHitDistance(hitDist, trim);
    if (demodulate)
        radiance = make_float3(radiance.x / factor.x, radiance.y / factor.y, radiance.z / factor.z);
    if (SPEC) {
        if (averaging)
            NRD_FrontEnd_SpecHitDistAveraging_Add(sums.specHitDist, hitDist);
        else
            sums.specHitDist = hitDist;
    } else if (mix)
        hitDist = NRD_HIP_MixDiffuseHitDist(hitDist, term.hitDist, _NRD_Luminance(SanitizedRadiance(radiance)), term.lum, maxContribution);
    float4 p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 p0 = PackSample<SPEC, MODE>(radiance, hitDist, Xyz(d), viewZ, r, hitDistParams, p1);
    if (perSample) {
        p0 = AddClamped(p0, term.p0, true);
        p1 = AddClamped(p1, term.p1, false);
    }
    sums.p0 = make_float4(sums.p0.x + p0.x, sums.p0.y + p0.y, sums.p0.z + p0.z, sums.p0.w + p0.w);
    sums.p1 = make_float4(sums.p1.x + p1.x, sums.p1.y + p1.y, sums.p1.z + p1.z, sums.p1.w + p1.w);
}

// a sample texel, read whole: one global_load_dwordx4 per lane in every mode (a mode that consumes .w or .xyz alone would else get a narrower load of the same sectors,
// and a 16-byte lane stride with it: the wave still touches the whole 1 KiB segment)
__device__ __forceinline__ float4 LoadSampleTexel(const Plane& layer, int x, int y) {
    float4 v = LoadRGBA32F(layer, x, y);
    NRD_LDS_WHOLE_TEXEL(v);
    return v;
}

// One signal of one pixel over `num` sample layers, the mode a template argument: the wave-uniform switch sits outside the sample loop (PackSignalSamples).
// Layer bases advance by scalar 64-bit additions; a lane's byte offset inside a layer is computed once. The loads of four layers are issued before the first of
// them is consumed (a wave reads one contiguous 1 KiB segment per layer and plane), the remaining num & 3 layers one by one.
// SPLIT (nrdHipPackInputsSplit): a sample costs two loads per plane instead of one, in the same loop -- 12 bytes of .xyz at a lane stride of 12 or 16, and the dword of .w, which is
// the companion's (its own pitch and layer stride) or the fourth of the 16-byte texel itself. Which is decided once, in front of the loop, by selecting base, offset and stride.
struct SplitSignal {
    FePlane hitDist;       // the companion
    uint64_t hitDistLayer;
    uint32_t inBytes, dirBytes; // 12 or 16
    bool wFromCompanion;
};

// DIRECT (nrdHipPackInputsDirect, a signal that has a direct plane): each sample's packed texel takes in the packed direct term of layer s of `ds` -- loaded with the indirect
// loads of its batch, a 16-byte texel whole -- or, when `ds` holds one layer, the mean takes in the one term, loaded once in front of the loop.
template <bool SPEC, uint32_t MODE, bool SPLIT, bool DIRECT = false>
__device__ __forceinline__ void ReduceSignal(const FePlane& in, const FePlane& dirPlane, const FePlane& out0, const FePlane& out1, uint64_t inLayer, uint64_t dirLayer, const SplitSignal& sp, uint32_t num,
    float trim, int x, int xo, int y, int w, int h, float viewZ, float roughness, float4 hitDistParams, bool demodulate, float3 factor, const DirectSignal& ds = DirectSignal{},
    float maxContribution = 0.0f, bool averaging = true) {
    static_assert(!DIRECT || SPLIT, "the direct call takes the split form of the body");
    constexpr bool kRadiance = MODE != NRD_HIP_SIGNAL_REBLUR_OCCLUSION && MODE != NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION; // (else .xyz is not consumed: not loaded by the split form)
    constexpr bool kDirection = MODE == NRD_HIP_SIGNAL_REBLUR_SH || MODE == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION || MODE == NRD_HIP_SIGNAL_RELAX_SH;
    constexpr bool kSh = MODE == NRD_HIP_SIGNAL_REBLUR_SH || MODE == NRD_HIP_SIGNAL_RELAX_SH;
    constexpr uint32_t kBatch = 4;
    const float r = SPEC ? roughness : 1.0f;
    // -0 is the identity of the addition ( -0 + p == p bit for bit, also for p = -0 and p = +0 ): the sums below are ( ( P_0 + P_1 ) + P_2 ) + ...
    SampleSums sums = {make_float4(-0.0f, -0.0f, -0.0f, -0.0f), make_float4(-0.0f, -0.0f, -0.0f, -0.0f), NRD_FrontEnd_SpecHitDistAveraging_Begin()};
    Plane layer = AsPlane(in, w, h), dirLayerPlane = AsPlane(kDirection ? dirPlane : in, w, h);
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // SPLIT: where this lane's .w lives in a layer, and how far the next layer is
    const Plane wPlane = AsPlane(SPLIT && sp.wFromCompanion ? sp.hitDist : in, w, h);
    const uint8_t* wPtr = !SPLIT ? nullptr : wPlane.ptr + (sp.wFromCompanion ? TexelOffset(wPlane, x, y, 4u, true) : TexelOffset(wPlane, x, y, 16u, true) + 12u);
    const uint64_t wLayer = SPLIT && sp.wFromCompanion ? sp.hitDistLayer : inLayer;
    auto loadSample = [&]() {
        if (!SPLIT)
            return LoadSampleTexel(layer, x, y);
        const float3 c = kRadiance ? LoadXyz32F(layer, x, y, sp.inBytes) : make_float3(0.0f, 0.0f, 0.0f);
        const float4 t = make_float4(c.x, c.y, c.z, *(const float*)wPtr);
        wPtr += wLayer;
        return t;
    };
    auto loadDirection = [&]() {
        if (!SPLIT)
            return LoadSampleTexel(dirLayerPlane, x, y);
        const float3 c = LoadXyz32F(dirLayerPlane, x, y, sp.dirBytes);
        return make_float4(c.x, c.y, c.z, 0.0f);
    };
    // DIRECT: where this lane's direct texel, its .w (an RGB32_SFLOAT plane's companion) and its direction live in a layer
    const bool mix = DIRECT && !SPEC && maxContribution > 0.0f, perSample = DIRECT && ds.num > 1u;
    Plane directLayer = AsPlane(DIRECT ? ds.in : in, w, h), directDirLayer = AsPlane(DIRECT && kDirection ? ds.dir : in, w, h);
    const uint8_t* directWPtr = DIRECT && mix && ds.hitDist.ptr ? ds.hitDist.ptr + TexelOffset(AsPlane(ds.hitDist, w, h), x, y, 4u, true) : nullptr;
    auto loadDirect = [&]() {
        float4 t;
        if (ds.inBytes == 16u)
            t = LoadSampleTexel(directLayer, x, y);
        else {
            const float3 c = LoadXyz32F(directLayer, x, y, 12u);
            t = make_float4(c.x, c.y, c.z, 0.0f);
            if (directWPtr) {
                t.w = *(const float*)directWPtr;
                directWPtr += ds.hitDistLayer;
            }
        }
        directLayer.ptr += ds.inLayer;
        return t;
    };
    auto loadDirectDirection = [&]() {
        const float3 c = LoadXyz32F(directDirLayer, x, y, ds.dirBytes);
        directDirLayer.ptr += ds.dirLayer;
        return make_float4(c.x, c.y, c.z, 0.0f);
    };
    float4 directTexel = zero, directDirection = zero; // one direct layer: loaded here, packed behind the first indirect loads
    if (DIRECT && !perSample) {
        directTexel = loadDirect();
        if (kDirection)
            directDirection = loadDirectDirection();
    }
    DirectTerm term = {zero, zero, 0.0f, 0.0f};
    uint32_t s = 0;
    for (; s + kBatch <= num; s += kBatch) {
        float4 t[kBatch], d[kBatch], td[kBatch], dd[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++) {
            t[k] = loadSample();
            d[k] = kDirection ? loadDirection() : zero;
            layer.ptr += inLayer;
            dirLayerPlane.ptr += dirLayer;
            if (DIRECT && perSample) {
                td[k] = loadDirect();
                dd[k] = kDirection ? loadDirectDirection() : zero;
            }
        }
        if (DIRECT && !perSample && s == 0u)
            term = PackDirectTerm<SPEC, MODE>(directTexel, directDirection, mix, trim, viewZ, r, hitDistParams, demodulate, factor);
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++) {
            if (DIRECT) {
                if (perSample)
                    term = PackDirectTerm<SPEC, MODE>(td[k], dd[k], mix, trim, viewZ, r, hitDistParams, demodulate, factor);
                AddSampleDirect<SPEC, MODE>(sums, t[k], d[k], term, perSample, mix, averaging, maxContribution, trim, viewZ, r, hitDistParams, demodulate, factor);
            } else
                AddSample<SPEC, MODE>(sums, t[k], d[k], trim, viewZ, r, hitDistParams, demodulate, factor);
        }
    }
    for (; s < num; s++) {
        const float4 t = loadSample();
        const float4 d = kDirection ? loadDirection() : zero;
        layer.ptr += inLayer;
        dirLayerPlane.ptr += dirLayer;
        if (DIRECT) {
            if (perSample) {
                const float4 td = loadDirect();
                const float4 dd = kDirection ? loadDirectDirection() : zero;
                term = PackDirectTerm<SPEC, MODE>(td, dd, mix, trim, viewZ, r, hitDistParams, demodulate, factor);
            } else if (s == 0u)
                term = PackDirectTerm<SPEC, MODE>(directTexel, directDirection, mix, trim, viewZ, r, hitDistParams, demodulate, factor);
            AddSampleDirect<SPEC, MODE>(sums, t, d, term, perSample, mix, averaging, maxContribution, trim, viewZ, r, hitDistParams, demodulate, factor);
        } else
            AddSample<SPEC, MODE>(sums, t, d, trim, viewZ, r, hitDistParams, demodulate, factor);
    }
    const float n = float(num);
    float4 p0 = make_float4(sums.p0.x / n, sums.p0.y / n, sums.p0.z / n, sums.p0.w / n);
    if (DIRECT && !perSample) // one direct layer: clamp( mean_s( P_i,s ) + P_d )
        p0 = AddClamped(p0, term.p0, true);
    if (SPEC) {
        if (!DIRECT || averaging)
            NRD_FrontEnd_SpecHitDistAveraging_End(sums.specHitDist);
        p0.w = PackedHitDist<MODE>(sums.specHitDist, viewZ, r, hitDistParams);
    }
    const Plane o0 = AsPlane(out0, w, h);
    if (MODE == NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        StoreR16Unorm(o0, xo, y, p0.w);
    else if (MODE == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        StoreRGBA16Snorm(o0, xo, y, p0);
    else
        StoreRGBA16F(o0, xo, y, p0);
    if (kSh && DIRECT) {
        const float4 p1 = make_float4(sums.p1.x / n, sums.p1.y / n, sums.p1.z / n, sums.p1.w / n);
        StoreRGBA16F(AsPlane(out1, w, h), xo, y, perSample ? p1 : AddClamped(p1, term.p1, false));
    } else if (kSh)
        StoreRGBA16F(AsPlane(out1, w, h), xo, y, make_float4(sums.p1.x / n, sums.p1.y / n, sums.p1.z / n, sums.p1.w / n));
}

#define NRD_REDUCE_SIGNAL(MODE) \
    case MODE: \
        ReduceSignal<SPEC, MODE, SPLIT>(in, dirPlane, out0, out1, inLayer, dirLayer, sp, num, trim, x, xo, y, w, h, viewZ, roughness, hitDistParams, demodulate, factor); \
        break;
template <bool SPEC, bool SPLIT>
__device__ __forceinline__ void PackSignalSamples(uint32_t mode, const FePlane& in, const FePlane& dirPlane, const FePlane& out0, const FePlane& out1, uint64_t inLayer, uint64_t dirLayer,
    const SplitSignal& sp, uint32_t num, float trim, int x, int xo, int y, int w, int h, float viewZ, float roughness, float4 hitDistParams, bool demodulate, float3 factor) {
    switch (mode) { // wave-uniform: a kernel argument
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_RADIANCE)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_SH)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_RELAX_RADIANCE)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_RELAX_SH)
        default:
            break;
    }
}
#undef NRD_REDUCE_SIGNAL

// a signal with a direct plane (nrdHipPackInputsDirect): the radiance and SH modes alone -- the host refuses a direct plane for the others
#define NRD_REDUCE_SIGNAL(MODE) \
    case MODE: \
        ReduceSignal<SPEC, MODE, true, true>(in, dirPlane, out0, out1, inLayer, dirLayer, sp, num, trim, x, xo, y, w, h, viewZ, roughness, hitDistParams, demodulate, factor, ds, maxContribution, averaging); \
        break;
template <bool SPEC>
__device__ __forceinline__ void PackSignalDirect(uint32_t mode, const FePlane& in, const FePlane& dirPlane, const FePlane& out0, const FePlane& out1, uint64_t inLayer, uint64_t dirLayer,
    const SplitSignal& sp, uint32_t num, float trim, int x, int xo, int y, int w, int h, float viewZ, float roughness, float4 hitDistParams, bool demodulate, float3 factor, const DirectSignal& ds,
    float maxContribution, bool averaging) {
    switch (mode) { // wave-uniform: a kernel argument
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_RADIANCE)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_REBLUR_SH)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_RELAX_RADIANCE)
        NRD_REDUCE_SIGNAL(NRD_HIP_SIGNAL_RELAX_SH)
        default:
            break;
    }
}
#undef NRD_REDUCE_SIGNAL

// ---- one traced lobe per sample (nrdHipPackInputsLobes; the per-pixel rules are spelled out in NRDHip.h) ------------------------------------------------------
// Both signals are built from ONE traced texel per sample: it is loaded once, outside the signals, and each signal then keeps it or replaces it by zeros. The signal's mode is
// a wave-uniform switch per sample here (a scalar branch), not a template argument: the loads are shared by two signals, whose modes would make 30 instantiations of the loop.
#define NRD_LOBE_MODES(CASE)                                                                                                                                        \
    CASE(NRD_HIP_SIGNAL_REBLUR_RADIANCE) CASE(NRD_HIP_SIGNAL_REBLUR_SH) CASE(NRD_HIP_SIGNAL_REBLUR_OCCLUSION) CASE(NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION) \
    CASE(NRD_HIP_SIGNAL_RELAX_RADIANCE) CASE(NRD_HIP_SIGNAL_RELAX_SH)
template <bool SPEC>
__device__ __forceinline__ float4 PackSampleOfMode(uint32_t mode, float3 radiance, float hitDist, float3 direction, float viewZ, float r, float4 hitDistParams, float4& p1) {
    switch (mode) {
#define NRD_LOBE_CASE(MODE) \
    case MODE:              \
        return PackSample<SPEC, MODE>(radiance, hitDist, direction, viewZ, r, hitDistParams, p1);
        NRD_LOBE_MODES(NRD_LOBE_CASE)
#undef NRD_LOBE_CASE
        default:
            return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}
__device__ __forceinline__ float PackedHitDistOfMode(uint32_t mode, float H, float viewZ, float r, float4 hitDistParams) {
    switch (mode) {
#define NRD_LOBE_CASE(MODE) \
    case MODE:              \
        return PackedHitDist<MODE>(H, viewZ, r, hitDistParams);
        NRD_LOBE_MODES(NRD_LOBE_CASE)
#undef NRD_LOBE_CASE
        default:
            return 0.0f;
    }
}
#undef NRD_LOBE_MODES

struct LobeSums {
    float4 p0, p1;
    float specHitDist;  // specular: the accumulator of NRD_FrontEnd_SpecHitDistAveraging_*
    float diffHitDist;  // diffuse: the packer's hit-distance output summed over the samples that count
    uint32_t countedNum;
};

// one sample for one signal: kept where it counts for the signal, else zeros with the direction ( 0, 0, 1 ) -- the loaded values may be NaN where the other lobe was traced.
// t: ( rad / q, h ) -- a sample counts for one signal at most, so the division is made once, in front of the two calls
template <bool SPEC>
__device__ __forceinline__ void AddLobeSample(uint32_t mode, LobeSums& sums, float4 t, float3 d, bool counted, float viewZ, float r, float4 hitDistParams, bool demodulate, float3 factor) {
    float3 radiance = counted ? Xyz(t) : make_float3(0.0f, 0.0f, 0.0f);
    const float hitDist = counted ? t.w : 0.0f;
    const float3 direction = counted ? d : make_float3(0.0f, 0.0f, 1.0f);
    if (demodulate)
        radiance = make_float3(radiance.x / factor.x, radiance.y / factor.y, radiance.z / factor.z);
    if (SPEC)
        NRD_FrontEnd_SpecHitDistAveraging_Add(sums.specHitDist, hitDist);
    float4 p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 p0 = PackSampleOfMode<SPEC>(mode, radiance, hitDist, direction, viewZ, r, hitDistParams, p1);
    sums.p0 = make_float4(sums.p0.x + p0.x, sums.p0.y + p0.y, sums.p0.z + p0.z, sums.p0.w + p0.w);
    sums.p1 = make_float4(sums.p1.x + p1.x, sums.p1.y + p1.y, sums.p1.z + p1.z, sums.p1.w + p1.w);
    if (!SPEC && counted) {
        sums.diffHitDist += p0.w;
        sums.countedNum++;
    }
}

template <bool SPEC>
__device__ __forceinline__ void StoreLobeSignal(uint32_t mode, const LobeSums& sums, uint32_t num, const FePlane& out0, const FePlane& out1, int x, int y, int w, int h, float viewZ, float r,
    float4 hitDistParams) {
    // one sample per pixel (uniform): x / 1.0f is x bit for bit, so none of the divisions of the means is made
    const float n = float(num);
    float4 p0 = sums.p0, p1 = sums.p1;
    if (num > 1u) {
        p0 = make_float4(sums.p0.x / n, sums.p0.y / n, sums.p0.z / n, 0.0f);
        p1 = make_float4(sums.p1.x / n, sums.p1.y / n, sums.p1.z / n, sums.p1.w / n);
    }
    p0.w = 0.0f;
    if (SPEC) {
        float H = sums.specHitDist;
        NRD_FrontEnd_SpecHitDistAveraging_End(H);
        p0.w = PackedHitDistOfMode(mode, H, viewZ, r, hitDistParams);
    } else if (sums.countedNum)
        p0.w = num > 1u ? sums.diffHitDist / float(sums.countedNum) : sums.diffHitDist;
    const Plane o0 = AsPlane(out0, w, h);
    if (mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        StoreR16Unorm(o0, x, y, p0.w);
    else if (mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        StoreRGBA16Snorm(o0, x, y, p0);
    else
        StoreRGBA16F(o0, x, y, p0);
    if (mode == NRD_HIP_SIGNAL_REBLUR_SH || mode == NRD_HIP_SIGNAL_RELAX_SH)
        StoreRGBA16F(AsPlane(out1, w, h), x, y, p1);
}

// Both signals of one pixel over lo.num sample layers. A lane's byte offset inside a layer is computed once per plane; layer bases advance by 64-bit additions. Per sample and
// lane: 16 bytes of the traced texel (or 12 + 4 of an RGB32_SFLOAT plane and its companion; 4 alone when no mode reads .xyz), 12 of the direction where a mode reads one, the
// lobe byte and the probability's dword -- each loaded once, whichever signal ends up using it.
__device__ __forceinline__ void PackLobes(const PackArgs& a, const LobeArgs& lo, int x, int y, int w, int h, float viewZ, float roughness, float3 diffFactor, float3 specFactor) {
    const bool wholeTexel = lo.in.ptr && !lo.hitDist.ptr; // RGBA32_SFLOAT: one global_load_dwordx4
    const uint8_t* inPtr = lo.in.ptr ? lo.in.ptr + TexelOffset(AsPlane(lo.in, w, h), x, y, lo.inBytes, true) : nullptr;
    const uint8_t* wPtr = lo.hitDist.ptr ? lo.hitDist.ptr + TexelOffset(AsPlane(lo.hitDist, w, h), x, y, 4u, true) : nullptr;
    const uint8_t* dirPtr = lo.dir.ptr ? lo.dir.ptr + TexelOffset(AsPlane(lo.dir, w, h), x, y, lo.dirBytes, true) : nullptr;
    const uint8_t* lobePtr = lo.lobe.ptr + TexelOffset(AsPlane(lo.lobe, w, h), x, y, 1u, true);
    const uint8_t* const probPtr0 = lo.prob.ptr; // (the plane's presence: uniform)
    const uint8_t* probPtr = lo.prob.ptr ? lo.prob.ptr + TexelOffset(AsPlane(lo.prob, w, h), x, y, 4u, true) : nullptr;
    // -0 is the identity of the addition (ReduceSignal): the sums are ( ( P_0 + P_1 ) + P_2 ) + ...
    const float4 minusZero = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
    LobeSums diff = {minusZero, minusZero, 0.0f, -0.0f, 0u}, spec = {minusZero, minusZero, NRD_FrontEnd_SpecHitDistAveraging_Begin(), 0.0f, 0u};
    for (uint32_t s = 0; s < lo.num; s++) {
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (wholeTexel)
            t = *(const float4*)inPtr;
        else {
            if (inPtr) {
                const Rgb32Texel c = *(const Rgb32Texel*)inPtr;
                t = make_float4(c.x, c.y, c.z, 0.0f);
            }
            t.w = *(const float*)wPtr;
        }
        float3 d = make_float3(0.0f, 0.0f, 1.0f);
        if (dirPtr) {
            const Rgb32Texel c = *(const Rgb32Texel*)dirPtr;
            d = make_float3(c.x, c.y, c.z);
            dirPtr += lo.dirLayer;
        }
        const uint32_t lobe = *lobePtr;
        const float p = probPtr ? *(const float*)probPtr : 0.0f;
        if (inPtr)
            inPtr += lo.inLayer;
        if (wPtr)
            wPtr += lo.hitDistLayer;
        lobePtr += lo.lobeLayer;
        if (probPtr)
            probPtr += lo.probLayer;
        float q = 1.0f;
        if (probPtr0) { // uniform. (Without the plane q is 1 and rad / 1 is rad: no division)
            q = lobe == NRD_HIP_LOBE_SPECULAR ? p : 1.0f - p;
            t = make_float4(t.x / q, t.y / q, t.z / q, t.w);
        }
        const bool traced = q > 0.0f; // (false for a NaN)
        AddLobeSample<false>(a.diffMode, diff, t, d, traced && lobe == NRD_HIP_LOBE_DIFFUSE, viewZ, 1.0f, a.hitDistParams, a.demodulate != 0u, diffFactor);
        AddLobeSample<true>(a.specMode, spec, t, d, traced && lobe == NRD_HIP_LOBE_SPECULAR, viewZ, roughness, a.hitDistParams, a.demodulate != 0u, specFactor);
    }
    StoreLobeSignal<false>(a.diffMode, diff, lo.num, a.diffOut0, a.diffOut1, x, y, w, h, viewZ, 1.0f, a.hitDistParams);
    StoreLobeSignal<true>(a.specMode, spec, lo.num, a.specOut0, a.specOut1, x, y, w, h, viewZ, roughness, a.hitDistParams);
}

// motion is clamped to +-FP16_MAX as raytracingdenoiser_amd/synth.py clamps it: infinities land on the bounds, a NaN stays a NaN (fminf / fmaxf alone would turn it into a bound)
__device__ __forceinline__ float ClampToHalf(float v) { return isnan(v) ? v : fminf(fmaxf(v, -NRD_FP16_MAX), NRD_FP16_MAX); }

// One pixel of the front end. CHECKERBOARD (nrdHipPackInputsEx, NRDSettings.h:35-44): a pixel carries the data of ONE signal -- the diffuse one where
// ( ( x ^ y ) ^ frameIndex ) & 1 == diffCell (nrdmath.h CheckerBoard), the specular one elsewhere -- and its texel goes to column x >> 1: the left half of the plane.
// Only those pixels of a signal's fp32 planes are read and no other texel of its packed planes is written.
// SAMPLES (nrdHipPackInputsSamples): each signal is reduced over its sample layers (PackSignalSamples); the other kernels never look at `sa`.
// SPLIT (nrdHipPackInputsSplit): the fp32 colour / vector planes may hold 12-byte RGB32_SFLOAT texels, `.w` in a plane of its own (`sp`, which the other kernels never look at).
// The same body: only the loads differ.
// DECIMATED (nrdHipPackInputsDecimated with guideShift = 1, quarter-resolution tracing): w x h is the LOW size, that of everything traced and of every output; the G-buffer planes
// (normalRoughness and its roughness companion, viewZ, materialID, motion, albedo, rf0) are full-size planes of which pixel ( x, y ) reads texel ( gx, gy ) = ( 2x, 2y ) -- inside
// them because w = ( W + 1 ) >> 1, h = ( H + 1 ) >> 1 (held by the host). Only that load coordinate differs: the view vector of the demodulation is that of ( x, y ) in w x h.
// LOBES (nrdHipPackInputsLobes): both signals come from one traced plane set (`lo`, which the other kernels never look at) through PackLobes; everything else is the plain body.
// DIRECT (nrdHipPackInputsDirect, the samples + split form of the body): a signal that has a direct plane in `di` (which the other kernels never look at) goes through
// PackSignalDirect; one that has none takes the very code it takes without `direct` -- that of the samples kernels, or of the plain ones where di.multiSample is 0 -- and no load more.
template <bool CHECKERBOARD, bool SAMPLES, bool SPLIT, bool DECIMATED = false, bool LOBES = false, bool DIRECT = false>
__device__ __forceinline__ void PackPixel(const PackArgs& a, const SampleArgs& sa, const SplitArgs& sp, uint32_t diffCell, uint32_t frameIndex, const LobeArgs& lo = LobeArgs{},
    const DirectArgs& di = DirectArgs{}) {
    static_assert(!DIRECT || (SAMPLES && SPLIT && !LOBES), "the direct call takes the samples + split form of the body");
    static_assert(!(DECIMATED && CHECKERBOARD), "checkerboarding and decimation are not combined");
    static_assert(!LOBES || (!CHECKERBOARD && !SAMPLES && !DECIMATED), "the lobes call has sample layers of its own and is neither checkerboarded nor decimated");
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = a.w, h = a.h;
    if (x >= w || y >= h)
        return;
    const int gx = DECIMATED ? x << 1 : x, gy = DECIMATED ? y << 1 : y;
    const float4 nr = LoadTexel<SPLIT>(a.normalRoughness, sp.roughness, sp.rgb, kSplitNormalRoughness, true, gx, gy, w, h);
    const float viewZ = LoadR32F(AsPlane(a.viewZ, w, h), gx, gy) * a.viewZScale;
    const float3 N = Xyz(nr);
    const float roughness = nr.w;

    if (a.outNormalRoughness.ptr) {
        const float materialID = a.materialID.ptr ? LoadR32F(AsPlane(a.materialID, w, h), gx, gy) : 0.0f;
        *TexelPtr<NRD_NormalRoughnessTexel>(AsPlane(a.outNormalRoughness, w, h), x, y) = NRD_StoreNormalRoughnessTexel(NRD_FrontEnd_PackNormalAndRoughness(N, roughness, materialID));
    }
    if (a.outViewZ.ptr)
        StoreR32F(AsPlane(a.outViewZ, w, h), x, y, viewZ);
    if (a.outMv.ptr) {
        float4 mv;
        if (a.motionIsRG) {
            const float2 m = *TexelPtr<const float2>(AsPlane(a.motion, w, h), gx, gy);
            mv = make_float4(m.x, m.y, 0.0f, 0.0f);
        } else if (SPLIT && (sp.rgb & kSplitMotion)) {
            const float3 m = LoadRGB32F(AsPlane(a.motion, w, h), gx, gy);
            mv = make_float4(m.x, m.y, m.z, 0.0f);
        } else
            mv = LoadRGBA32F(AsPlane(a.motion, w, h), gx, gy);
        StoreRGBA16F(AsPlane(a.outMv, w, h), x, y, make_float4(ClampToHalf(mv.x), ClampToHalf(mv.y), ClampToHalf(mv.z), ClampToHalf(mv.w)));
    }

    float3 diffFactor = make_float3(1.0f, 1.0f, 1.0f), specFactor = diffFactor;
    if (a.demodulate) {
        const float3 V = ViewVector(a.camera, x, y, w, h, viewZ);
        NRD_MaterialFactors(N, V, LoadColour<SPLIT>(a.albedo, sp.rgb, kSplitAlbedo, gx, gy, w, h), LoadColour<SPLIT>(a.rf0, sp.rgb, kSplitRf0, gx, gy, w, h), roughness, diffFactor, specFactor);
    }
    const bool diffHere = !CHECKERBOARD || ((((uint32_t)x ^ (uint32_t)y) ^ frameIndex) & 1u) == diffCell;
    const int xo = CHECKERBOARD ? x >> 1 : x;
    if (LOBES)
        PackLobes(a, lo, x, y, w, h, viewZ, roughness, diffFactor, specFactor);
    else if (SAMPLES) {
        const SplitSignal diffSplit = {sp.diffHitDist, sp.diffHitDistLayer, SplitTexelBytes(sp.rgb, kSplitDiffIn), SplitTexelBytes(sp.rgb, kSplitDiffDir), (sp.rgb & kSplitDiffIn) != 0u};
        const SplitSignal specSplit = {sp.specHitDist, sp.specHitDistLayer, SplitTexelBytes(sp.rgb, kSplitSpecIn), SplitTexelBytes(sp.rgb, kSplitSpecDir), (sp.rgb & kSplitSpecIn) != 0u};
        if (a.diffMode && diffHere) {
            if (DIRECT && di.diff.in.ptr)
                PackSignalDirect<false>(a.diffMode, a.diffIn, a.diffDir, a.diffOut0, a.diffOut1, sa.diffInLayer, sa.diffDirLayer, diffSplit, sa.diffNum, sa.trim, x, xo, y, w, h, viewZ, roughness,
                    a.hitDistParams, a.demodulate != 0u, diffFactor, di.diff, di.maxContribution, di.multiSample != 0u);
            else if (DIRECT && !di.multiSample)
                PackSignal<false, SPLIT>(a.diffMode, a.diffIn, a.diffDir, a.diffOut0, a.diffOut1, sp.diffHitDist, sp.rgb, x, xo, y, w, h, viewZ, roughness, a.hitDistParams, a.demodulate != 0u, diffFactor);
            else
                PackSignalSamples<false, SPLIT>(a.diffMode, a.diffIn, a.diffDir, a.diffOut0, a.diffOut1, sa.diffInLayer, sa.diffDirLayer, diffSplit, sa.diffNum, sa.trim, x, xo, y, w, h, viewZ, roughness,
                    a.hitDistParams, a.demodulate != 0u, diffFactor);
        }
        if (a.specMode && (!CHECKERBOARD || !diffHere)) {
            if (DIRECT && di.spec.in.ptr)
                PackSignalDirect<true>(a.specMode, a.specIn, a.specDir, a.specOut0, a.specOut1, sa.specInLayer, sa.specDirLayer, specSplit, sa.specNum, sa.trim, x, xo, y, w, h, viewZ, roughness,
                    a.hitDistParams, a.demodulate != 0u, specFactor, di.spec, 0.0f, di.multiSample != 0u);
            else if (DIRECT && !di.multiSample)
                PackSignal<true, SPLIT>(a.specMode, a.specIn, a.specDir, a.specOut0, a.specOut1, sp.specHitDist, sp.rgb, x, xo, y, w, h, viewZ, roughness, a.hitDistParams, a.demodulate != 0u, specFactor);
            else
                PackSignalSamples<true, SPLIT>(a.specMode, a.specIn, a.specDir, a.specOut0, a.specOut1, sa.specInLayer, sa.specDirLayer, specSplit, sa.specNum, sa.trim, x, xo, y, w, h, viewZ, roughness,
                    a.hitDistParams, a.demodulate != 0u, specFactor);
        }
    } else {
        if (a.diffMode && diffHere)
            PackSignal<false, SPLIT>(a.diffMode, a.diffIn, a.diffDir, a.diffOut0, a.diffOut1, sp.diffHitDist, sp.rgb, x, xo, y, w, h, viewZ, roughness, a.hitDistParams, a.demodulate != 0u, diffFactor);
        if (a.specMode && (!CHECKERBOARD || !diffHere))
            PackSignal<true, SPLIT>(a.specMode, a.specIn, a.specDir, a.specOut0, a.specOut1, sp.specHitDist, sp.rgb, x, xo, y, w, h, viewZ, roughness, a.hitDistParams, a.demodulate != 0u, specFactor);
    }

    if (a.outPenumbra.ptr || a.outTranslucency.ptr) {
        const float distanceToOccluder = LoadR32F(AsPlane(a.occluder, w, h), x, y);
        if (a.outPenumbra.ptr)
            StoreR16F(AsPlane(a.outPenumbra, w, h), x, y, SIGMA_FrontEnd_PackPenumbra(distanceToOccluder, a.tanOfLightAngularRadius));
        if (a.outTranslucency.ptr)
            StoreRGBA8Unorm(AsPlane(a.outTranslucency, w, h), x, y, SIGMA_FrontEnd_PackTranslucency(distanceToOccluder, LoadColour<SPLIT>(a.translucency, sp.rgb, kSplitTranslucency, x, y, w, h)));
    }
}

__global__ void __launch_bounds__(256) PackInputsKernel(const PackArgs a) { PackPixel<false, false, false>(a, SampleArgs{}, SplitArgs{}, 0u, 0u); }

__global__ void __launch_bounds__(256) PackCheckerboardKernel(const PackArgs a, const uint32_t diffCell, const uint32_t frameIndex) {
    PackPixel<true, false, false>(a, SampleArgs{}, SplitArgs{}, diffCell, frameIndex);
}

// the multi-sample twin of the two (nrdHipPackInputsSamples with more than one sample layer or a trim threshold), templated on checkerboard like them
template <bool CHECKERBOARD>
__global__ void __launch_bounds__(256) PackSamplesKernel(const PackArgs a, const SampleArgs sa, const uint32_t diffCell, const uint32_t frameIndex) {
    PackPixel<CHECKERBOARD, true, false>(a, sa, SplitArgs{}, diffCell, frameIndex);
}

// the split twins of the four (nrdHipPackInputsSplit with an RGB32_SFLOAT plane or a companion): further instantiations of the same body, their kernel arguments those of
// their siblings plus SplitArgs
__global__ void __launch_bounds__(256) PackInputsSplitKernel(const PackArgs a, const SplitArgs sp) { PackPixel<false, false, true>(a, SampleArgs{}, sp, 0u, 0u); }

__global__ void __launch_bounds__(256) PackCheckerboardSplitKernel(const PackArgs a, const SplitArgs sp, const uint32_t diffCell, const uint32_t frameIndex) {
    PackPixel<true, false, true>(a, SampleArgs{}, sp, diffCell, frameIndex);
}

template <bool CHECKERBOARD>
__global__ void __launch_bounds__(256) PackSamplesSplitKernel(const PackArgs a, const SampleArgs sa, const SplitArgs sp, const uint32_t diffCell, const uint32_t frameIndex) {
    PackPixel<CHECKERBOARD, true, true>(a, sa, sp, diffCell, frameIndex);
}

// the decimated twins of the four kernels without checkerboarding (nrdHipPackInputsDecimated with guideShift = 1): the same body once more, the G-buffer planes read at ( 2x, 2y )
__global__ void __launch_bounds__(256) PackDecimatedKernel(const PackArgs a) { PackPixel<false, false, false, true>(a, SampleArgs{}, SplitArgs{}, 0u, 0u); }

__global__ void __launch_bounds__(256) PackDecimatedSamplesKernel(const PackArgs a, const SampleArgs sa) { PackPixel<false, true, false, true>(a, sa, SplitArgs{}, 0u, 0u); }

__global__ void __launch_bounds__(256) PackDecimatedSplitKernel(const PackArgs a, const SplitArgs sp) { PackPixel<false, false, true, true>(a, SampleArgs{}, sp, 0u, 0u); }

__global__ void __launch_bounds__(256) PackDecimatedSamplesSplitKernel(const PackArgs a, const SampleArgs sa, const SplitArgs sp) { PackPixel<false, true, true, true>(a, sa, sp, 0u, 0u); }

// nrdHipPackInputsLobes: the split form of the body (an RGB32_SFLOAT G-buffer plane is a uniform branch on a bit of sp.rgb), the two signals from the traced planes of `lo`
__global__ void __launch_bounds__(256) PackLobesKernel(const PackArgs a, const SplitArgs sp, const LobeArgs lo) { PackPixel<false, false, true, false, true>(a, SampleArgs{}, sp, 0u, 0u, lo); }

// nrdHipPackInputsDirect with a direct plane: the samples + split form of the body (one sample layer and four-channel planes are uniform branches of it), plain, checkerboarded
// and decimated
__global__ void __launch_bounds__(256) PackDirectKernel(const PackArgs a, const SampleArgs sa, const SplitArgs sp, const DirectArgs di) {
    PackPixel<false, true, true, false, false, true>(a, sa, sp, 0u, 0u, LobeArgs{}, di);
}

__global__ void __launch_bounds__(256) PackDirectCheckerboardKernel(const PackArgs a, const SampleArgs sa, const SplitArgs sp, const DirectArgs di, const uint32_t diffCell, const uint32_t frameIndex) {
    PackPixel<true, true, true, false, false, true>(a, sa, sp, diffCell, frameIndex, LobeArgs{}, di);
}

__global__ void __launch_bounds__(256) PackDirectDecimatedKernel(const PackArgs a, const SampleArgs sa, const SplitArgs sp, const DirectArgs di) {
    PackPixel<false, true, true, true, false, true>(a, sa, sp, 0u, 0u, LobeArgs{}, di);
}

__device__ __forceinline__ float4 LoadSignalTexel(const FePlane& p, bool wide, int x, int y, int w, int h) {
    return wide ? LoadRGBA32F(AsPlane(p, w, h), x, y) : LoadRGBA16F(AsPlane(p, w, h), x, y);
}

// one signal of the back end: returns the colour written to `out` (for the composition). ( sx, sy ) in sw x sh: the texel of in0 / in1 the pixel takes its signal from -- the
// pixel itself in the plain kernels, the nearest-Z texel of the low-size planes in the upsampling ones; everything else (viewZ, N, V, roughness, factor, the store) is the pixel's
template <bool SPEC, bool SPLIT>
__device__ __forceinline__ float3 ResolveSignal(uint32_t mode, uint32_t resolve, bool wide, const FePlane& in0, const FePlane& in1, const FePlane& out, const FePlane& outHitDist, uint32_t splitBits,
    int x, int y, int w, int h, int sx, int sy, int sw, int sh, float viewZ, float3 N, float3 V, float roughness, float4 hitDistParams, bool denormalize, bool remodulate, float3 factor) {
    const float r = SPEC ? roughness : 1.0f;
    const Plane o = AsPlane(out, w, h);
    if (mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION) {
        float normHitDist = LoadR16Unorm(AsPlane(in0, sw, sh), sx, sy);
        if (denormalize)
            normHitDist = REBLUR_GetHitDist(normHitDist, viewZ, hitDistParams, r);
        StoreR32F(o, x, y, normHitDist);
        return make_float3(0.0f, 0.0f, 0.0f);
    }
    float4 c;
    const bool reblur = mode != NRD_HIP_SIGNAL_RELAX_RADIANCE && mode != NRD_HIP_SIGNAL_RELAX_SH;
    if (mode == NRD_HIP_SIGNAL_REBLUR_RADIANCE)
        c = REBLUR_BackEnd_UnpackRadianceAndNormHitDist(LoadSignalTexel(in0, wide, sx, sy, sw, sh));
    else if (mode == NRD_HIP_SIGNAL_RELAX_RADIANCE)
        c = RELAX_BackEnd_UnpackRadiance(LoadSignalTexel(in0, wide, sx, sy, sw, sh));
    else {
        NRD_SG sg;
        if (mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
            sg = REBLUR_BackEnd_UnpackDirectionalOcclusion(LoadRGBA16Snorm(AsPlane(in0, sw, sh), sx, sy));
        else if (mode == NRD_HIP_SIGNAL_REBLUR_SH)
            sg = REBLUR_BackEnd_UnpackSh(LoadSignalTexel(in0, wide, sx, sy, sw, sh), LoadSignalTexel(in1, wide, sx, sy, sw, sh));
        else
            sg = RELAX_BackEnd_UnpackSh(LoadSignalTexel(in0, wide, sx, sy, sw, sh), LoadSignalTexel(in1, wide, sx, sy, sw, sh));
        float3 rgb;
        if (resolve == NRD_HIP_RESOLVE_SH)
            rgb = SPEC ? NRD_SH_ResolveSpecular(sg, N, V, roughness) : NRD_SH_ResolveDiffuse(sg, N);
        else if (resolve == NRD_HIP_RESOLVE_SG)
            rgb = SPEC ? NRD_SG_ResolveSpecular(sg, N, V, roughness) : NRD_SG_ResolveDiffuse(sg, N);
        else
            rgb = NRD_SG_ExtractColor(sg);
        c = make_float4(rgb.x, rgb.y, rgb.z, sg.normHitDist);
    }
    if (denormalize && reblur)
        c.w = REBLUR_GetHitDist(c.w, viewZ, hitDistParams, r);
    if (remodulate)
        c = make_float4(c.x * factor.x, c.y * factor.y, c.z * factor.z, c.w);
    StoreTexel<SPLIT>(out, outHitDist, splitBits, SPEC ? kSplitSpecOut : kSplitDiffOut, x, y, w, h, c);
    return Xyz(c);
}

// one pixel of the back end. SPLIT (nrdHipResolveOutputsSplit): albedo / rf0 and the colour outputs may hold 12-byte RGB32_SFLOAT texels, the hit distance of a signal then goes
// to a plane of its own or nowhere (`sp`, which the plain kernel never looks at). The same body: only the loads of albedo / rf0 and the stores differ.
template <bool SPLIT>
__device__ __forceinline__ void ResolvePixel(const ResolveArgs& a, const ResolveSplitArgs& sp) {
    const FePlane none = {nullptr, 0};
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = a.w, h = a.h;
    if (x >= w || y >= h)
        return;
    const float viewZ = a.viewZ.ptr ? LoadR32F(AsPlane(a.viewZ, w, h), x, y) : 0.0f;
    float3 N = make_float3(0.0f, 0.0f, 1.0f);
    float roughness = 1.0f;
    if (a.normalRoughness.ptr) {
        const float4 nr = NRD_FrontEnd_UnpackNormalAndRoughness(NRD_LoadNormalRoughnessTexel(*TexelPtr<const NRD_NormalRoughnessTexel>(AsPlane(a.normalRoughness, w, h), x, y)));
        N = Xyz(nr);
        roughness = nr.w;
    }
    float3 V = make_float3(0.0f, 0.0f, 0.0f);
    if (a.needV) {
        V = ViewVector(a.camera, x, y, w, h, viewZ);
        if (a.outViewVector.ptr)
            StoreTexel<SPLIT>(a.outViewVector, none, sp.rgb, kSplitViewVector, x, y, w, h, make_float4(V.x, V.y, V.z, 0.0f));
    }
    float3 diffFactor = make_float3(1.0f, 1.0f, 1.0f), specFactor = diffFactor;
    if (a.needFactors) {
        NRD_MaterialFactors(N, V, LoadColour<SPLIT>(a.albedo, sp.rgb, kSplitAlbedo, x, y, w, h), LoadColour<SPLIT>(a.rf0, sp.rgb, kSplitRf0, x, y, w, h), roughness, diffFactor, specFactor);
        if (a.outDiffFactor.ptr)
            StoreTexel<SPLIT>(a.outDiffFactor, none, sp.rgb, kSplitDiffFactor, x, y, w, h, make_float4(diffFactor.x, diffFactor.y, diffFactor.z, 0.0f));
        if (a.outSpecFactor.ptr)
            StoreTexel<SPLIT>(a.outSpecFactor, none, sp.rgb, kSplitSpecFactor, x, y, w, h, make_float4(specFactor.x, specFactor.y, specFactor.z, 0.0f));
    }
    float3 diff = make_float3(0.0f, 0.0f, 0.0f), spec = diff;
    if (a.diffMode)
        diff = ResolveSignal<false, SPLIT>(a.diffMode, a.diffResolve, a.diffWide != 0u, a.diffIn0, a.diffIn1, a.diffOut, sp.diffHitDist, sp.rgb, x, y, w, h, x, y, w, h, viewZ, N, V, roughness, a.hitDistParams, a.denormalize != 0u,
            a.remodulate != 0u, diffFactor);
    if (a.specMode)
        spec = ResolveSignal<true, SPLIT>(a.specMode, a.specResolve, a.specWide != 0u, a.specIn0, a.specIn1, a.specOut, sp.specHitDist, sp.rgb, x, y, w, h, x, y, w, h, viewZ, N, V, roughness, a.hitDistParams, a.denormalize != 0u,
            a.remodulate != 0u, specFactor);
    if (a.outComposed.ptr)
        StoreTexel<SPLIT>(a.outComposed, none, sp.rgb, kSplitComposed, x, y, w, h, make_float4(diff.x + spec.x, diff.y + spec.y, diff.z + spec.z, 0.0f));
    if (a.outShadow.ptr) {
        if (a.shadowIsRGBA)
            StoreRGBA32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadRGBA8Unorm(AsPlane(a.shadow, w, h), x, y)));
        else
            StoreR32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadR8Unorm(AsPlane(a.shadow, w, h), x, y)));
    }
}

__global__ void __launch_bounds__(256) ResolveOutputsKernel(const ResolveArgs a) { ResolvePixel<false>(a, ResolveSplitArgs{}); }

__global__ void __launch_bounds__(256) ResolveOutputsSplitKernel(const ResolveArgs a, const ResolveSplitArgs sp) { ResolvePixel<true>(a, sp); }

// ---- quarter-resolution denoising: the resolve of low-size OUT_* planes into the full-size frame (nrdHipResolveOutputsUpsampled; the rule is spelled out in NRDHip.h) -------
// ResolveArgs::w x h is the FULL size: normalRoughness, viewZ, albedo, rf0 and every output are full-size planes and everything per pixel -- N, roughness, V, the material
// factors, the depth and roughness of denormalizeHitDist -- is computed as ResolvePixel computes it. The signal planes (in0 / in1, shadow) and lowViewZ are lw x lh: low texel
// ( i, j ) stands for full pixel ( 2i, 2j ). A pixel looks at the up to four low texels around it, takes the one nearest in depth ("nearest Z") and reads its signals there.
// A 64-lane row touches 33 consecutive low texels of one or two rows; the row pair above / below re-reads them from the cache: no LDS.
struct UpsampleArgs {
    FePlane lowViewZ, outSource;
    float viewZScale, denoisingRange, depthThreshold;
    int32_t lw, lh;
};

constexpr uint32_t kNoSource = 255u;

// zeros where a pixel has no source: the signal's output and its split hit-distance plane
template <bool SPEC, bool SPLIT>
__device__ __forceinline__ void StoreNoSignal(uint32_t mode, const FePlane& out, const FePlane& outHitDist, uint32_t splitBits, int x, int y, int w, int h) {
    if (mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        StoreR32F(AsPlane(out, w, h), x, y, 0.0f);
    else
        StoreTexel<SPLIT>(out, outHitDist, splitBits, SPEC ? kSplitSpecOut : kSplitDiffOut, x, y, w, h, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
}

template <bool SPLIT>
__device__ __forceinline__ void ResolveUpsampledPixel(const ResolveArgs& a, const ResolveSplitArgs& sp, const UpsampleArgs& u) {
    const FePlane none = {nullptr, 0};
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = a.w, h = a.h, lw = u.lw, lh = u.lh;
    if (x >= w || y >= h)
        return;
    const float viewZ = LoadR32F(AsPlane(a.viewZ, w, h), x, y);
    float3 N = make_float3(0.0f, 0.0f, 1.0f);
    float roughness = 1.0f;
    if (a.normalRoughness.ptr) {
        const float4 nr = NRD_FrontEnd_UnpackNormalAndRoughness(NRD_LoadNormalRoughnessTexel(*TexelPtr<const NRD_NormalRoughnessTexel>(AsPlane(a.normalRoughness, w, h), x, y)));
        N = Xyz(nr);
        roughness = nr.w;
    }
    float3 V = make_float3(0.0f, 0.0f, 0.0f);
    if (a.needV) {
        V = ViewVector(a.camera, x, y, w, h, viewZ);
        if (a.outViewVector.ptr)
            StoreTexel<SPLIT>(a.outViewVector, none, sp.rgb, kSplitViewVector, x, y, w, h, make_float4(V.x, V.y, V.z, 0.0f));
    }
    float3 diffFactor = make_float3(1.0f, 1.0f, 1.0f), specFactor = diffFactor;
    if (a.needFactors) {
        NRD_MaterialFactors(N, V, LoadColour<SPLIT>(a.albedo, sp.rgb, kSplitAlbedo, x, y, w, h), LoadColour<SPLIT>(a.rf0, sp.rgb, kSplitRf0, x, y, w, h), roughness, diffFactor, specFactor);
        if (a.outDiffFactor.ptr)
            StoreTexel<SPLIT>(a.outDiffFactor, none, sp.rgb, kSplitDiffFactor, x, y, w, h, make_float4(diffFactor.x, diffFactor.y, diffFactor.z, 0.0f));
        if (a.outSpecFactor.ptr)
            StoreTexel<SPLIT>(a.outSpecFactor, none, sp.rgb, kSplitSpecFactor, x, y, w, h, make_float4(specFactor.x, specFactor.y, specFactor.z, 0.0f));
    }

    // nearest Z: candidate k = a + 2b is low texel ( ( x >> 1 ) + a, ( y >> 1 ) + b ); an even coordinate has the one texel that stands for it, an odd one the two around it
    const float Zf = fabsf(viewZ * u.viewZScale);
    uint32_t source = kNoSource;
    float best = 0.0f;
    if (!(isnan(Zf) || Zf > u.denoisingRange)) {
        const Plane lz = AsPlane(u.lowViewZ, lw, lh);
        const int i0 = x >> 1, j0 = y >> 1;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const int ca = (int)(k & 1u), cb = (int)(k >> 1);
            const bool exists = (ca == 0 || (x & 1)) && (cb == 0 || (y & 1)) && i0 + ca < lw && j0 + cb < lh;
            if (!exists)
                continue;
            const float Zk = fabsf(LoadR32F(lz, i0 + ca, j0 + cb) * u.viewZScale);
            if (isnan(Zk) || Zk > u.denoisingRange)
                continue;
            const float dk = fabsf(Zk - Zf);
            if (source == kNoSource || dk < best) { // (a tie stays with the lowest k)
                source = k;
                best = dk;
            }
        }
        if (source != kNoSource && u.depthThreshold > 0.0f && best > u.depthThreshold * Zf)
            source = kNoSource;
    }
    if (u.outSource.ptr)
        StoreR8U(AsPlane(u.outSource, w, h), x, y, source);

    if (source == kNoSource) { // sky at full size, or nothing denoised nearby: zeros, and no signal texel is loaded
        if (a.diffMode)
            StoreNoSignal<false, SPLIT>(a.diffMode, a.diffOut, sp.diffHitDist, sp.rgb, x, y, w, h);
        if (a.specMode)
            StoreNoSignal<true, SPLIT>(a.specMode, a.specOut, sp.specHitDist, sp.rgb, x, y, w, h);
        if (a.outComposed.ptr)
            StoreTexel<SPLIT>(a.outComposed, none, sp.rgb, kSplitComposed, x, y, w, h, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        if (a.outShadow.ptr) {
            if (a.shadowIsRGBA)
                StoreRGBA32F(AsPlane(a.outShadow, w, h), x, y, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            else
                StoreR32F(AsPlane(a.outShadow, w, h), x, y, 0.0f);
        }
        return;
    }
    const int sx = (x >> 1) + (int)(source & 1u), sy = (y >> 1) + (int)(source >> 1);
    float3 diff = make_float3(0.0f, 0.0f, 0.0f), spec = diff;
    if (a.diffMode)
        diff = ResolveSignal<false, SPLIT>(a.diffMode, a.diffResolve, a.diffWide != 0u, a.diffIn0, a.diffIn1, a.diffOut, sp.diffHitDist, sp.rgb, x, y, w, h, sx, sy, lw, lh, viewZ, N, V, roughness, a.hitDistParams,
            a.denormalize != 0u, a.remodulate != 0u, diffFactor);
    if (a.specMode)
        spec = ResolveSignal<true, SPLIT>(a.specMode, a.specResolve, a.specWide != 0u, a.specIn0, a.specIn1, a.specOut, sp.specHitDist, sp.rgb, x, y, w, h, sx, sy, lw, lh, viewZ, N, V, roughness, a.hitDistParams,
            a.denormalize != 0u, a.remodulate != 0u, specFactor);
    if (a.outComposed.ptr)
        StoreTexel<SPLIT>(a.outComposed, none, sp.rgb, kSplitComposed, x, y, w, h, make_float4(diff.x + spec.x, diff.y + spec.y, diff.z + spec.z, 0.0f));
    if (a.outShadow.ptr) {
        if (a.shadowIsRGBA)
            StoreRGBA32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadRGBA8Unorm(AsPlane(a.shadow, lw, lh), sx, sy)));
        else
            StoreR32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadR8Unorm(AsPlane(a.shadow, lw, lh), sx, sy)));
    }
}

__global__ void __launch_bounds__(256) ResolveUpsampledKernel(const ResolveArgs a, const UpsampleArgs u) { ResolveUpsampledPixel<false>(a, ResolveSplitArgs{}, u); }

__global__ void __launch_bounds__(256) ResolveUpsampledSplitKernel(const ResolveArgs a, const ResolveSplitArgs sp, const UpsampleArgs u) { ResolveUpsampledPixel<true>(a, sp, u); }

// ---- the high-quality resolve of an SH denoiser (nrdHipResolveOutputsEx with reJitter): SG / SH resolve, NRD_SG_ReJitter, remodulation ---------------
// NRD_SG_ReJitter is the one stencil of the back end: it wants viewZ and the decoded normal of the four edge neighbours. NRD_REJITTER_TILE = 1 (shipped; DESIGN.md
// section 3.4 has the A/B): a workgroup stages the decoded N.xyz and Z of its 64 x 4 pixels plus a one-texel halo in LDS -- every lane decodes its own texel, the
// first 140 lanes one halo texel more: 396 / 256 = 1.55 decodes per pixel -- and reads its neighbours from there. Rows of 66 float4: the 64 lanes of a wave (one row of
// the tile) read 64 consecutive 16-byte texels, at any of the three column offsets and three rows -- a conflict-free ds_read_b128. NRD_REJITTER_TILE = 0 (A/B builds): every lane loads
// and decodes its four neighbour texels itself, 5 decodes per pixel. Same decoded values, same function: the two forms give the same bits.
// Texels outside the plane read as zeros (N = 0, Z = 0), with which NRD_SG_ReJitter returns (1, 1): border pixels are exactly unscaled.
#ifndef NRD_REJITTER_TILE
#define NRD_REJITTER_TILE 1
#endif
constexpr int kReJitterTileW = 64, kReJitterTileH = 4; // = the workgroup

struct ReJitterArgs {
    ResolveArgs r;
    FePlane outScale;
};

// decoded N.xyz and Z (.w) of texel (x, y), zeros outside the plane; roughness: that of the texel
__device__ __forceinline__ float4 LoadNormalAndViewZ(const ResolveArgs& a, int x, int y, float& roughness) {
    roughness = 0.0f;
    if ((unsigned)x >= (unsigned)a.w || (unsigned)y >= (unsigned)a.h)
        return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 nr = NRD_FrontEnd_UnpackNormalAndRoughness(NRD_LoadNormalRoughnessTexel(*TexelPtr<const NRD_NormalRoughnessTexel>(AsPlane(a.normalRoughness, a.w, a.h), x, y)));
    roughness = nr.w;
    return make_float4(nr.x, nr.y, nr.z, LoadR32F(AsPlane(a.viewZ, a.w, a.h), x, y));
}

template <bool SPEC>
__device__ __forceinline__ NRD_SG LoadSg(uint32_t mode, bool wide, const FePlane& in0, const FePlane& in1, int x, int y, int w, int h) {
    const float4 sh0 = LoadSignalTexel(in0, wide, x, y, w, h), sh1 = LoadSignalTexel(in1, wide, x, y, w, h);
    return mode == NRD_HIP_SIGNAL_REBLUR_SH ? REBLUR_BackEnd_UnpackSh(sh0, sh1) : RELAX_BackEnd_UnpackSh(sh0, sh1);
}

// ( resolved.rgb * scale ) * factor, in that order; .w as ResolveSignal writes it
template <bool SPEC, bool SPLIT>
__device__ __forceinline__ float3 StoreReJittered(const ResolveArgs& a, uint32_t mode, uint32_t resolve, const FePlane& out, const FePlane& outHitDist, uint32_t splitBits, NRD_SG sg, int x, int y, float viewZ,
    float3 N, float3 V, float roughness, float scale, float3 factor) {
    float3 rgb;
    if (resolve == NRD_HIP_RESOLVE_SH)
        rgb = SPEC ? NRD_SH_ResolveSpecular(sg, N, V, roughness) : NRD_SH_ResolveDiffuse(sg, N);
    else
        rgb = SPEC ? NRD_SG_ResolveSpecular(sg, N, V, roughness) : NRD_SG_ResolveDiffuse(sg, N);
    float4 c = make_float4(rgb.x * scale, rgb.y * scale, rgb.z * scale, sg.normHitDist);
    if (a.denormalize && mode == NRD_HIP_SIGNAL_REBLUR_SH)
        c.w = REBLUR_GetHitDist(c.w, viewZ, a.hitDistParams, SPEC ? roughness : 1.0f);
    if (a.remodulate)
        c = make_float4(c.x * factor.x, c.y * factor.y, c.z * factor.z, c.w);
    StoreTexel<SPLIT>(out, outHitDist, splitBits, SPEC ? kSplitSpecOut : kSplitDiffOut, x, y, a.w, a.h, c);
    return Xyz(c);
}

// SPLIT (nrdHipResolveOutputsSplit with reJitter): the LDS tile is the same; only the loads of rf0 / albedo and the stores differ
template <bool SPLIT>
__device__ __forceinline__ void ReJitterPixel(const ReJitterArgs& args, const ResolveSplitArgs& sp) {
    const FePlane none = {nullptr, 0};
    const ResolveArgs& a = args.r;
    const int x = (int)(blockIdx.x * (uint32_t)kReJitterTileW + threadIdx.x), y = (int)(blockIdx.y * (uint32_t)kReJitterTileH + threadIdx.y);
    const int w = a.w, h = a.h;
    float roughness, unused;
    const float4 c = LoadNormalAndViewZ(a, x, y, roughness);
#if NRD_REJITTER_TILE
    __shared__ float4 s_Tile[kReJitterTileH + 2][kReJitterTileW + 2];
    const int tx = (int)threadIdx.x + 1, ty = (int)threadIdx.y + 1;
    s_Tile[ty][tx] = c;
    // the halo: the row above, the row below (66 texels each), then the columns left and right (4 each)
    constexpr int kRow = kReJitterTileW + 2, kHalo = 2 * kRow + 2 * kReJitterTileH;
    const int j = (int)(threadIdx.y * (uint32_t)kReJitterTileW + threadIdx.x);
    if (j < kHalo) {
        const int k = j - 2 * kRow;
        const int hx = j < kRow ? j : j < 2 * kRow ? j - kRow : k < kReJitterTileH ? 0 : kRow - 1;
        const int hy = j < kRow ? 0 : j < 2 * kRow ? kReJitterTileH + 1 : (k < kReJitterTileH ? k : k - kReJitterTileH) + 1;
        s_Tile[hy][hx] = LoadNormalAndViewZ(a, (int)(blockIdx.x * (uint32_t)kReJitterTileW) + hx - 1, (int)(blockIdx.y * (uint32_t)kReJitterTileH) + hy - 1, unused);
    }
    __syncthreads();
    if (x >= w || y >= h)
        return;
    const float4 e = LdsFloat4(&s_Tile[ty][tx + 1]), wn = LdsFloat4(&s_Tile[ty][tx - 1]), n = LdsFloat4(&s_Tile[ty + 1][tx]), s = LdsFloat4(&s_Tile[ty - 1][tx]);
#else
    if (x >= w || y >= h)
        return;
    const float4 e = LoadNormalAndViewZ(a, x + 1, y, unused), wn = LoadNormalAndViewZ(a, x - 1, y, unused), n = LoadNormalAndViewZ(a, x, y + 1, unused), s = LoadNormalAndViewZ(a, x, y - 1, unused);
#endif
    const float viewZ = c.w;
    const float3 N = Xyz(c);
    const float3 V = ViewVector(a.camera, x, y, w, h, viewZ);
    if (a.outViewVector.ptr)
        StoreTexel<SPLIT>(a.outViewVector, none, sp.rgb, kSplitViewVector, x, y, w, h, make_float4(V.x, V.y, V.z, 0.0f));
    const float3 Rf0 = LoadColour<SPLIT>(a.rf0, sp.rgb, kSplitRf0, x, y, w, h);
    float3 diffFactor = make_float3(1.0f, 1.0f, 1.0f), specFactor = diffFactor;
    if (a.needFactors) {
        NRD_MaterialFactors(N, V, LoadColour<SPLIT>(a.albedo, sp.rgb, kSplitAlbedo, x, y, w, h), Rf0, roughness, diffFactor, specFactor);
        if (a.outDiffFactor.ptr)
            StoreTexel<SPLIT>(a.outDiffFactor, none, sp.rgb, kSplitDiffFactor, x, y, w, h, make_float4(diffFactor.x, diffFactor.y, diffFactor.z, 0.0f));
        if (a.outSpecFactor.ptr)
            StoreTexel<SPLIT>(a.outSpecFactor, none, sp.rgb, kSplitSpecFactor, x, y, w, h, make_float4(specFactor.x, specFactor.y, specFactor.z, 0.0f));
    }
    const NRD_SG diffSg = LoadSg<false>(a.diffMode, a.diffWide != 0u, a.diffIn0, a.diffIn1, x, y, w, h), specSg = LoadSg<true>(a.specMode, a.specWide != 0u, a.specIn0, a.specIn1, x, y, w, h);
    const float2 scale = NRD_SG_ReJitter(diffSg, specSg, Rf0, V, roughness, viewZ, e.w, wn.w, n.w, s.w, N, Xyz(e), Xyz(wn), Xyz(n), Xyz(s));
    if (args.outScale.ptr)
        *TexelPtr<float2>(AsPlane(args.outScale, w, h), x, y) = scale;
    const float3 diff = StoreReJittered<false, SPLIT>(a, a.diffMode, a.diffResolve, a.diffOut, sp.diffHitDist, sp.rgb, diffSg, x, y, viewZ, N, V, roughness, scale.x, diffFactor);
    const float3 spec = StoreReJittered<true, SPLIT>(a, a.specMode, a.specResolve, a.specOut, sp.specHitDist, sp.rgb, specSg, x, y, viewZ, N, V, roughness, scale.y, specFactor);
    if (a.outComposed.ptr)
        StoreTexel<SPLIT>(a.outComposed, none, sp.rgb, kSplitComposed, x, y, w, h, make_float4(diff.x + spec.x, diff.y + spec.y, diff.z + spec.z, 0.0f));
    if (a.outShadow.ptr) {
        if (a.shadowIsRGBA)
            StoreRGBA32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadRGBA8Unorm(AsPlane(a.shadow, w, h), x, y)));
        else
            StoreR32F(AsPlane(a.outShadow, w, h), x, y, SIGMA_BackEnd_UnpackShadow(LoadR8Unorm(AsPlane(a.shadow, w, h), x, y)));
    }
}

__global__ void __launch_bounds__(256) ReJitterKernel(const ReJitterArgs args) { ReJitterPixel<false>(args, ResolveSplitArgs{}); }

__global__ void __launch_bounds__(256) ReJitterSplitKernel(const ReJitterArgs args, const ResolveSplitArgs sp) { ReJitterPixel<true>(args, sp); }

// ---- host side: validation (all of it in front of the first HIP call) and the launch ---------------------------------------------------------------
constexpr nrd::Format kNormalRoughnessFormat = NRD_NORMAL_ENCODING == 0 ? nrd::Format::RGBA8_UNORM : NRD_NORMAL_ENCODING == 1 ? nrd::Format::RGBA8_SNORM : NRD_NORMAL_ENCODING == 2 ? nrd::Format::R10_G10_B10_A2_UNORM
    : NRD_NORMAL_ENCODING == 3 ? nrd::Format::RGBA16_UNORM : nrd::Format::RGBA16_SNORM;

// frustum and view-to-world rotation of a frame: the steps of nrd::SetCommonSettings (csrc/host/instance.cpp) with the same functions
bool Camera(Checker& c, const void* commonSettings, const char* why, FeCamera& out) {
    using namespace nrdhost;
    if (c.Failed())
        return false;
    if (!commonSettings) {
        c.Error(nrd::Result::INVALID_ARGUMENT, "commonSettings", why);
        return false;
    }
    const nrd::CommonSettings& cs = *(const nrd::CommonSettings*)commonSettings;
    Mat4 viewToClip = Mat4::FromColumnMajor(cs.viewToClipMatrix), worldToView = Mat4::FromColumnMajor(cs.worldToViewMatrix);
    ProjectionInfo info = DecomposeProjection(viewToClip);
    if (info.isOrtho) {
        c.Error(nrd::Result::UNSUPPORTED, "commonSettings", "orthographic projections are not supported");
        return false;
    }
    if (cs.rectSize[0] != c.w || cs.rectSize[1] != c.h) {
        c.Error(nrd::Result::INVALID_ARGUMENT, "commonSettings", "rectSize is not the size of the planes");
        return false;
    }
    if (!info.isLeftHanded) { // everything downstream is left-handed
        for (int i = 0; i < 4; i++)
            viewToClip.c[2].v[i] = -viewToClip.c[2].v[i];
        for (int j = 0; j < 4; j++)
            worldToView.at(2, j) = -worldToView.at(2, j);
    }
    const Mat4 viewToWorld = InvertRigid(worldToView);
    info = DecomposeProjection(viewToClip);
    out.frustum = make_float4(info.frustum[0], info.frustum[1], info.frustum[2], info.frustum[3]);
    out.row0 = make_float4(viewToWorld.at(0, 0), viewToWorld.at(0, 1), viewToWorld.at(0, 2), 0.0f);
    out.row1 = make_float4(viewToWorld.at(1, 0), viewToWorld.at(1, 1), viewToWorld.at(1, 2), 0.0f);
    out.row2 = make_float4(viewToWorld.at(2, 0), viewToWorld.at(2, 1), viewToWorld.at(2, 2), 0.0f);
    return true;
}

bool IsSh(uint32_t mode) { return mode == NRD_HIP_SIGNAL_REBLUR_SH || mode == NRD_HIP_SIGNAL_RELAX_SH; }

// hitDistDesc: the signal's companion of NrdHipFrontEndSplit (an absent plane for the old calls); inBit / dirBit: the kSplit* bits of its two fp32 planes
void FrontEndSignal(Checker& c, const NrdHipFrontEndSignal& s, const char* name, const NrdHipPlaneDesc& hitDistDesc, uint32_t inBit, uint32_t dirBit, FePlane& in, FePlane& dir, FePlane& out0,
    FePlane& out1, FePlane& hitDist, bool lobes = false) {
    using F = nrd::Format;
    const std::string n(name), companion = "split: " + n + "HitDist";
    if (lobes) { // nrdHipPackInputsLobes: the traced data comes from the planes of NrdHipFrontEndLobes and from nowhere else; both signals are produced
        if (s.mode == NRD_HIP_SIGNAL_NONE)
            c.Error(nrd::Result::INVALID_ARGUMENT, (n + ".mode").c_str(), "NONE: the lobes call produces both signals");
        Refuse(c, s.radianceHitDist, (n + ".radianceHitDist").c_str(), "given next to lobes: the traced data would have two sources");
        Refuse(c, s.direction, (n + ".direction").c_str(), "given next to lobes: the traced data would have two sources");
        Refuse(c, hitDistDesc, companion.c_str(), "given next to lobes: the hit distance would have two sources");
    } else if (s.mode == NRD_HIP_SIGNAL_NONE) {
        if (hitDistDesc.data)
            c.Error(nrd::Result::INVALID_ARGUMENT, companion.c_str(), "given for a signal whose mode is NONE");
        return;
    } else if (c.split && s.mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION && !s.radianceHitDist.data && hitDistDesc.data) { // the mode reads .w only: the companion alone will do
        hitDist = c.Check(hitDistDesc, companion.c_str(), nullptr, F::R32_SFLOAT);
        if (hitDist.ptr)
            c.rgb |= inBit;
    } else {
        in = c.CheckColour(s.radianceHitDist, (n + ".radianceHitDist").c_str(), "the signal's mode needs it", inBit);
        hitDist = c.CheckCompanion(hitDistDesc, companion.c_str(), (c.rgb & inBit) != 0u, "radianceHitDist is RGB32_SFLOAT: the hit distance comes from this plane", (n + ".radianceHitDist").c_str());
    }
    if (!lobes && (IsSh(s.mode) || s.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION))
        dir = c.CheckColour(s.direction, (n + ".direction").c_str(), "the signal's mode needs a direction plane", dirBit);
    const F outFormat = s.mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION ? F::R16_UNORM : s.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION ? F::RGBA16_SNORM : F::RGBA16_SFLOAT;
    out0 = c.Check(s.out0, (n + ".out0").c_str(), "the signal's mode needs it", outFormat);
    if (IsSh(s.mode))
        out1 = c.Check(s.out1, (n + ".out1").c_str(), "the SH modes write SH1 there", F::RGBA16_SFLOAT);
}

// hitDistDesc: the signal's companion of NrdHipBackEndSplit (an absent plane for the old calls); outBit: the kSplit* bit of its output
// upsampled: nrdHipResolveOutputsUpsampled -- in0 / in1 are low-size planes, the output and its companion full-size ones
void BackEndSignal(Checker& c, const NrdHipBackEndSignal& s, const char* name, const NrdHipPlaneDesc& hitDistDesc, uint32_t outBit, FePlane& in0, FePlane& in1, FePlane& out, FePlane& outHitDist,
    uint32_t& wide, bool upsampled = false) {
    using F = nrd::Format;
    const std::string n(name), companion = "split: " + n + "HitDist";
    if (s.mode == NRD_HIP_SIGNAL_NONE) {
        if (hitDistDesc.data)
            c.Error(nrd::Result::INVALID_ARGUMENT, companion.c_str(), "given for a signal whose mode is NONE");
        return;
    }
    if (s.mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION)
        in0 = c.Check(s.in0, (n + ".in0").c_str(), "the signal's mode needs it", F::R16_UNORM);
    else if (s.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        in0 = c.Check(s.in0, (n + ".in0").c_str(), "the signal's mode needs it", F::RGBA16_SNORM);
    else
        in0 = c.Check(s.in0, (n + ".in0").c_str(), "the signal's mode needs it", F::RGBA16_SFLOAT, F::RGBA32_SFLOAT);
    wide = s.in0.format == (uint32_t)F::RGBA32_SFLOAT;
    if (IsSh(s.mode)) {
        in1 = c.Check(s.in1, (n + ".in1").c_str(), "the SH modes read SH1 there", F::RGBA16_SFLOAT, F::RGBA32_SFLOAT);
        if (!c.Failed() && s.in1.format != s.in0.format)
            c.Error(nrd::Result::INVALID_ARGUMENT, (n + ".in1").c_str(), "SH0 and SH1 must have the same format");
    }
    FullSize outputs(c, upsampled);
    if (s.mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION) {
        out = c.Check(s.out, (n + ".out").c_str(), "the signal's mode needs it", F::R32_SFLOAT);
        if (hitDistDesc.data)
            c.Error(nrd::Result::INVALID_ARGUMENT, companion.c_str(), "the occlusion mode's output is the hit distance already (R32_SFLOAT): nothing to split");
        return;
    }
    out = c.CheckColour(s.out, (n + ".out").c_str(), "the signal's mode needs it", outBit);
    outHitDist = c.CheckCompanion(hitDistDesc, companion.c_str(), (c.rgb & outBit) != 0u, nullptr, (n + ".out").c_str()); // optional: the hit distance is dropped without it
}

} // namespace

extern "C" __attribute__((visibility("default"))) const char* nrdHipGetLastFrontEndError(void) { return t_LastError.c_str(); }

namespace {

// the rules of NrdHipFrontEndSamples that need no plane; num: the signal's sample count, 0 read as 1
uint32_t CheckSamples(const NrdHipSignalSamples& s, uint32_t mode, const char* name, uint32_t& num) {
    const std::string n = std::string("nrdHipPackInputsSamples: samples: ") + name;
    num = s.samplesNum ? s.samplesNum : 1u;
    if (s.samplesNum > 64u)
        return Fail(nrd::Result::INVALID_ARGUMENT, n + ".samplesNum: more than 64 sample layers");
    if (s.reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, n + ".reserved: must be 0");
    if (num > 1u && mode == NRD_HIP_SIGNAL_NONE)
        return Fail(nrd::Result::INVALID_ARGUMENT, n + ".samplesNum: sample layers given for a signal whose mode is NONE");
    return (uint32_t)nrd::Result::SUCCESS;
}

// the rules of one signal of NrdHipFrontEndDirect; num: the signal's own sample count. Returns whether the signal has a direct term
bool DirectSignalPlanes(Checker& c, const NrdHipDirectSignal& s, const char* name, uint32_t mode, uint32_t num, bool spec, float maxContribution, uint32_t inBit, uint32_t dirBit, DirectSignal& out) {
    const std::string n = std::string("direct: ") + name;
    if (s.reserved)
        c.Error(nrd::Result::INVALID_ARGUMENT, (n + ".reserved").c_str(), "must be 0");
    if (!s.radianceHitDist.data) { // no direct term: nothing else of the signal may be given
        Refuse(c, s.hitDist, (n + ".hitDist").c_str(), "given without radianceHitDist");
        Refuse(c, s.direction, (n + ".direction").c_str(), "given without radianceHitDist");
        return false;
    }
    if (mode == NRD_HIP_SIGNAL_NONE || mode == NRD_HIP_SIGNAL_REBLUR_OCCLUSION || mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        c.Error(nrd::Result::INVALID_ARGUMENT, (n + ".radianceHitDist").c_str(), "given for a signal whose mode is NONE or an occlusion mode: there is no radiance to weigh the direct term by");
    out.num = s.samplesNum ? s.samplesNum : 1u;
    if (out.num != 1u && out.num != num)
        c.Error(nrd::Result::INVALID_ARGUMENT, (n + ".samplesNum").c_str(), "neither 1 nor the signal's own sample count");
    out.in = c.CheckColour(s.radianceHitDist, (n + ".radianceHitDist").c_str(), nullptr, inBit);
    const bool rgb = (c.rgb & inBit) != 0u;
    if (spec)
        Refuse(c, s.hitDist, (n + ".hitDist").c_str(), "given: the specular hit distance is the indirect one alone, a direct distance is never read");
    else if (!(maxContribution > 0.0f))
        Refuse(c, s.hitDist, (n + ".hitDist").c_str(), "given with maxHitDistContribution == 0: no direct hit distance is read");
    else
        out.hitDist = c.CheckCompanion(s.hitDist, (n + ".hitDist").c_str(), rgb, "radianceHitDist is RGB32_SFLOAT: the direct hit distance comes from this plane", (n + ".radianceHitDist").c_str());
    if (IsSh(mode))
        out.dir = c.CheckColour(s.direction, (n + ".direction").c_str(), "the signal's mode needs a direction plane", dirBit);
    else
        Refuse(c, s.direction, (n + ".direction").c_str(), "given for a mode that reads no direction");
    out.inBytes = rgb ? 12u : 16u;
    out.dirBytes = (c.rgb & dirBit) ? 12u : 16u;
    CheckLayerBytes(c, out.inLayer = s.radianceHitDistLayerBytes, out.in, out.num, (n + ".radianceHitDistLayerBytes").c_str(), rgb);
    CheckLayerBytes(c, out.hitDistLayer = s.hitDistLayerBytes, out.hitDist, out.num, (n + ".hitDistLayerBytes").c_str(), true);
    CheckLayerBytes(c, out.dirLayer = s.directionLayerBytes, out.dir, out.num, (n + ".directionLayerBytes").c_str(), (c.rgb & dirBit) != 0u);
    return true;
}

// split != nullptr or splitEntry: nrdHipPackInputsSplit -- RGB32_SFLOAT planes and their companions are accepted
// decimated: nrdHipPackInputsDecimated with guideShift = 1 -- the G-buffer planes form the full-size class of the checker, everything else the low-size one
// lobes != nullptr: nrdHipPackInputsLobes -- both signals come from the traced planes of `lobes` (samples == nullptr: the sample layers are those of `lobes`)
// direct != nullptr: nrdHipPackInputsDirect -- the signals' own planes are the indirect ones, `direct` holds the direct ones
uint32_t PackInputs(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, const NrdHipFrontEndSplit* split, bool splitEntry, void* hipStream,
    bool decimated = false, const NrdHipFrontEndLobes* lobes = nullptr, const NrdHipFrontEndDirect* direct = nullptr) {
    using F = nrd::Format;
    static const NrdHipFrontEndSplit noSplit = {};
    const NrdHipFrontEndSplit& sd = split ? *split : noSplit;
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputs: null descriptor");
    if (d->diffuse.mode > NRD_HIP_SIGNAL_RELAX_SH || d->specular.mode > NRD_HIP_SIGNAL_RELAX_SH || d->specular.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputs: unknown signal mode (directional occlusion is a diffuse mode)");
    const uint32_t checkerboardMode = options ? options->checkerboardMode : 0u;
    if (checkerboardMode > (uint32_t)nrd::CheckerboardMode::WHITE)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsEx: options: unknown checkerboardMode");
    if (decimated && checkerboardMode)
        return Fail(nrd::Result::UNSUPPORTED, "nrdHipPackInputsDecimated: options: checkerboardMode: checkerboarding combined with decimation (guideShift = 1) is out of scope");
    if (checkerboardMode && d->diffuse.mode == NRD_HIP_SIGNAL_NONE && d->specular.mode == NRD_HIP_SIGNAL_NONE)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsEx: options: checkerboardMode without a diffuse or a specular signal to checkerboard");
    if (lobes && checkerboardMode)
        return Fail(nrd::Result::UNSUPPORTED, "nrdHipPackInputsLobes: options: checkerboardMode: checkerboarding is the other way to split a frame between the signals; combined with lobes it is out of scope");
    if (lobes && lobes->samplesNum > 64u)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsLobes: lobes: samplesNum: more than 64 sample layers");
    if (lobes && lobes->reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsLobes: lobes: reserved: must be 0");
    if (direct && direct->reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsDirect: direct: reserved: must be 0");
    if (direct && !(direct->maxHitDistContribution >= 0.0f && direct->maxHitDistContribution <= 1.0f)) // (a NaN fails every comparison)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsDirect: direct: maxHitDistContribution: NaN or outside [0, 1]");
    SampleArgs sa = {};
    sa.diffNum = sa.specNum = 1u;
    if (samples) {
        if (uint32_t r = CheckSamples(samples->diffuse, d->diffuse.mode, "diffuse", sa.diffNum))
            return r;
        if (uint32_t r = CheckSamples(samples->specular, d->specular.mode, "specular", sa.specNum))
            return r;
        if (samples->reserved)
            return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsSamples: samples: reserved: must be 0");
        if (!(samples->hitDistTrimThreshold >= 0.0f)) // (a NaN fails every comparison)
            return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsSamples: samples: hitDistTrimThreshold: negative or NaN");
        sa.trim = samples->hitDistTrimThreshold;
    }
    const bool multiSample = sa.diffNum > 1u || sa.specNum > 1u || sa.trim > 0.0f; // else: the kernels of nrdHipPackInputsEx, the same bytes, no extra loads
    const char* entry = direct ? "nrdHipPackInputsDirect" : lobes ? "nrdHipPackInputsLobes" : decimated ? "nrdHipPackInputsDecimated" : splitEntry ? "nrdHipPackInputsSplit" : "nrdHipPackInputs";
    Checker c{entry};
    c.split = splitEntry;
    PackArgs a = {};
    SplitArgs sp = {};
    {
        FullSize guides(c, decimated);
        a.normalRoughness = c.CheckColour(d->normalRoughness, "normalRoughness", "required", kSplitNormalRoughness);
        sp.roughness = c.CheckCompanion(sd.roughness, "split: roughness", (c.rgb & kSplitNormalRoughness) != 0u, "normalRoughness is RGB32_SFLOAT: the roughness comes from this plane", "normalRoughness");
        a.viewZ = c.Check(d->viewZ, "viewZ", "required", F::R32_SFLOAT);
        a.materialID = c.Check(d->materialID, "materialID", nullptr, F::R32_SFLOAT);
    }
    a.outNormalRoughness = c.Check(d->outNormalRoughness, "outNormalRoughness", nullptr, kNormalRoughnessFormat);
    a.outViewZ = c.Check(d->outViewZ, "outViewZ", nullptr, F::R32_SFLOAT);
    a.outMv = c.Check(d->outMv, "outMv", nullptr, F::RGBA16_SFLOAT);
    {
        FullSize guides(c, decimated);
        a.motion = c.CheckColour(d->motion, "motion", a.outMv.ptr ? "outMv needs it" : nullptr, kSplitMotion, F::RG32_SFLOAT);
    }
    a.motionIsRG = d->motion.format == (uint32_t)F::RG32_SFLOAT;
    a.outPenumbra = c.Check(d->outPenumbra, "outPenumbra", nullptr, F::R16_SFLOAT);
    a.outTranslucency = c.Check(d->outTranslucency, "outTranslucency", nullptr, F::RGBA8_UNORM);
    a.occluder = c.Check(d->distanceToOccluder, "distanceToOccluder", a.outPenumbra.ptr || a.outTranslucency.ptr ? "outPenumbra / outTranslucency need it" : nullptr, F::R32_SFLOAT);
    a.translucency = c.CheckColour(d->translucency, "translucency", a.outTranslucency.ptr ? "outTranslucency needs it" : nullptr, kSplitTranslucency);
    const bool demodulate = d->albedo.data || d->rf0.data;
    {
        FullSize guides(c, decimated);
        a.albedo = c.CheckColour(d->albedo, "albedo", demodulate ? "demodulation needs albedo and rf0" : nullptr, kSplitAlbedo);
        a.rf0 = c.CheckColour(d->rf0, "rf0", demodulate ? "demodulation needs albedo and rf0" : nullptr, kSplitRf0);
    }
    FrontEndSignal(c, d->diffuse, "diffuse", sd.diffuseHitDist, kSplitDiffIn, kSplitDiffDir, a.diffIn, a.diffDir, a.diffOut0, a.diffOut1, sp.diffHitDist, lobes != nullptr);
    FrontEndSignal(c, d->specular, "specular", sd.specularHitDist, kSplitSpecIn, kSplitSpecDir, a.specIn, a.specDir, a.specOut0, a.specOut1, sp.specHitDist, lobes != nullptr);
    LobeArgs lo = {};
    if (lobes) {
        auto readsXyz = [](uint32_t mode) { return mode != NRD_HIP_SIGNAL_REBLUR_OCCLUSION && mode != NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION; };
        auto readsDirection = [](uint32_t mode) { return IsSh(mode) || mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION; };
        if (!lobes->radianceHitDist.data && lobes->hitDist.data && !readsXyz(d->diffuse.mode) && !readsXyz(d->specular.mode)) // both modes read .w only: the companion alone will do
            lo.hitDist = c.Check(lobes->hitDist, "lobes: hitDist", nullptr, F::R32_SFLOAT);
        else {
            lo.in = c.CheckColour(lobes->radianceHitDist, "lobes: radianceHitDist", "required: what the traced path of each sample returned", kSplitLobeIn);
            lo.hitDist = c.CheckCompanion(lobes->hitDist, "lobes: hitDist", (c.rgb & kSplitLobeIn) != 0u, "radianceHitDist is RGB32_SFLOAT: the hit distance comes from this plane", "lobes: radianceHitDist");
        }
        if (readsDirection(d->diffuse.mode) || readsDirection(d->specular.mode)) // (else it is not read)
            lo.dir = c.CheckColour(lobes->direction, "lobes: direction", "a signal's mode needs a direction plane", kSplitLobeDir);
        lo.lobe = c.Check(lobes->lobe, "lobes: lobe", "required: the lobe each sample traced", F::R8_UINT);
        lo.prob = c.Check(lobes->probability, "lobes: probability", nullptr, F::R32_SFLOAT);
        lo.num = lobes->samplesNum ? lobes->samplesNum : 1u;
        lo.inBytes = (c.rgb & kSplitLobeIn) ? 12u : 16u;
        lo.dirBytes = (c.rgb & kSplitLobeDir) ? 12u : 16u;
        CheckLayerBytes(c, lo.inLayer = lobes->radianceHitDistLayerBytes, lo.in, lo.num, "lobes: radianceHitDistLayerBytes", (c.rgb & kSplitLobeIn) != 0u);
        CheckLayerBytes(c, lo.hitDistLayer = lobes->hitDistLayerBytes, lo.hitDist, lo.num, "lobes: hitDistLayerBytes", true);
        CheckLayerBytes(c, lo.dirLayer = lobes->directionLayerBytes, lo.dir, lo.num, "lobes: directionLayerBytes", (c.rgb & kSplitLobeDir) != 0u);
        CheckLayerBytes(c, lo.lobeLayer = lobes->lobeLayerBytes, lo.lobe, lo.num, "lobes: lobeLayerBytes", true);
        CheckLayerBytes(c, lo.probLayer = lobes->probabilityLayerBytes, lo.prob, lo.num, "lobes: probabilityLayerBytes", true);
    }
    DirectArgs di = {};
    bool hasDirect = false;
    if (direct) {
        di.maxContribution = direct->maxHitDistContribution;
        di.multiSample = multiSample ? 1u : 0u;
        hasDirect |= DirectSignalPlanes(c, direct->diffuse, "diffuse", d->diffuse.mode, sa.diffNum, false, di.maxContribution, kSplitDirectDiffIn, kSplitDirectDiffDir, di.diff);
        hasDirect |= DirectSignalPlanes(c, direct->specular, "specular", d->specular.mode, sa.specNum, true, di.maxContribution, kSplitDirectSpecIn, kSplitDirectSpecDir, di.spec);
    }
    if (multiSample && samples && splitEntry) { // the same rules, in dwords where the stack holds RGB32_SFLOAT texels, and for the companions
        CheckLayerBytes(c, sa.diffInLayer = samples->diffuse.radianceHitDistLayerBytes, a.diffIn, sa.diffNum, "samples: diffuse.radianceHitDistLayerBytes", (c.rgb & kSplitDiffIn) != 0u);
        CheckLayerBytes(c, sa.diffDirLayer = samples->diffuse.directionLayerBytes, a.diffDir, sa.diffNum, "samples: diffuse.directionLayerBytes", (c.rgb & kSplitDiffDir) != 0u);
        CheckLayerBytes(c, sa.specInLayer = samples->specular.radianceHitDistLayerBytes, a.specIn, sa.specNum, "samples: specular.radianceHitDistLayerBytes", (c.rgb & kSplitSpecIn) != 0u);
        CheckLayerBytes(c, sa.specDirLayer = samples->specular.directionLayerBytes, a.specDir, sa.specNum, "samples: specular.directionLayerBytes", (c.rgb & kSplitSpecDir) != 0u);
        CheckLayerBytes(c, sp.diffHitDistLayer = sd.diffuseHitDistLayerBytes, sp.diffHitDist, sa.diffNum, "split: diffuseHitDistLayerBytes", true);
        CheckLayerBytes(c, sp.specHitDistLayer = sd.specularHitDistLayerBytes, sp.specHitDist, sa.specNum, "split: specularHitDistLayerBytes", true);
        if (!a.diffIn.ptr) // (the occlusion mode on its companion alone: no plane to step through)
            sa.diffInLayer = 0;
        if (!a.specIn.ptr)
            sa.specInLayer = 0;
    } else if (multiSample && samples) {
        c.entry = "nrdHipPackInputsSamples";
        CheckLayerBytes(c, sa.diffInLayer = samples->diffuse.radianceHitDistLayerBytes, a.diffIn, sa.diffNum, "samples: diffuse.radianceHitDistLayerBytes");
        CheckLayerBytes(c, sa.diffDirLayer = samples->diffuse.directionLayerBytes, a.diffDir, sa.diffNum, "samples: diffuse.directionLayerBytes");
        CheckLayerBytes(c, sa.specInLayer = samples->specular.radianceHitDistLayerBytes, a.specIn, sa.specNum, "samples: specular.radianceHitDistLayerBytes");
        CheckLayerBytes(c, sa.specDirLayer = samples->specular.directionLayerBytes, a.specDir, sa.specNum, "samples: specular.directionLayerBytes");
        c.entry = entry;
    }
    if (decimated && !c.Failed() && !c.w) // (every plane given is a G-buffer plane: nothing has the low size)
        c.Error(nrd::Result::INVALID_ARGUMENT, "descriptor", "no low-size plane: no output and no signal");
    if (demodulate)
        Camera(c, d->commonSettings, "demodulation needs the frame's camera", a.camera);
    if (c.Failed())
        return c.result;
    a.demodulate = demodulate ? 1u : 0u;
    a.diffMode = d->diffuse.mode;
    a.specMode = d->specular.mode;
    a.hitDistParams = make_float4(d->hitDistParams[0], d->hitDistParams[1], d->hitDistParams[2], d->hitDistParams[3]);
    a.viewZScale = d->viewZScale == 0.0f ? 1.0f : d->viewZScale;
    a.tanOfLightAngularRadius = d->tanOfLightAngularRadius;
    a.w = c.w;
    a.h = c.h;
    t_LastError.clear();
    const dim3 grid((c.w + 63u) / 64u, (c.h + 3u) / 4u), block(64, 4);
    if (lobes) {
        sp.rgb = c.rgb;
        hipLaunchKernelGGL(PackLobesKernel, grid, block, 0, (hipStream_t)hipStream, a, sp, lo);
    } else if (hasDirect) { // (without a direct plane: the kernels of the call without `direct` below, the same bytes)
        sp.rgb = c.rgb;
        if (decimated)
            hipLaunchKernelGGL(PackDirectDecimatedKernel, grid, block, 0, (hipStream_t)hipStream, a, sa, sp, di);
        else if (checkerboardMode)
            hipLaunchKernelGGL(PackDirectCheckerboardKernel, grid, block, 0, (hipStream_t)hipStream, a, sa, sp, di,
                checkerboardMode == (uint32_t)nrd::CheckerboardMode::BLACK ? 0u : 1u, options ? options->frameIndex & 1u : 0u);
        else
            hipLaunchKernelGGL(PackDirectKernel, grid, block, 0, (hipStream_t)hipStream, a, sa, sp, di);
    } else if (decimated) { // the decimated twins: plain, samples and their split forms (checkerboarding was refused above)
        sp.rgb = c.rgb;
        if (c.rgb && multiSample)
            hipLaunchKernelGGL(PackDecimatedSamplesSplitKernel, grid, block, 0, (hipStream_t)hipStream, a, sa, sp);
        else if (c.rgb)
            hipLaunchKernelGGL(PackDecimatedSplitKernel, grid, block, 0, (hipStream_t)hipStream, a, sp);
        else if (multiSample)
            hipLaunchKernelGGL(PackDecimatedSamplesKernel, grid, block, 0, (hipStream_t)hipStream, a, sa);
        else
            hipLaunchKernelGGL(PackDecimatedKernel, grid, block, 0, (hipStream_t)hipStream, a);
    } else if (c.rgb) { // something to split: the twins. (Else the kernels of the old calls: the same code, the same bytes.)
        sp.rgb = c.rgb;
        const uint32_t diffCell = checkerboardMode == (uint32_t)nrd::CheckerboardMode::BLACK ? 0u : 1u, frameIndex = options ? options->frameIndex & 1u : 0u;
        if (multiSample && checkerboardMode)
            hipLaunchKernelGGL(PackSamplesSplitKernel<true>, grid, block, 0, (hipStream_t)hipStream, a, sa, sp, diffCell, frameIndex);
        else if (multiSample)
            hipLaunchKernelGGL(PackSamplesSplitKernel<false>, grid, block, 0, (hipStream_t)hipStream, a, sa, sp, 0u, 0u);
        else if (checkerboardMode)
            hipLaunchKernelGGL(PackCheckerboardSplitKernel, grid, block, 0, (hipStream_t)hipStream, a, sp, diffCell, frameIndex);
        else
            hipLaunchKernelGGL(PackInputsSplitKernel, grid, block, 0, (hipStream_t)hipStream, a, sp);
    } else if (multiSample) {
        const uint32_t diffCell = checkerboardMode == (uint32_t)nrd::CheckerboardMode::BLACK ? 0u : 1u, frameIndex = options ? options->frameIndex & 1u : 0u;
        if (checkerboardMode)
            hipLaunchKernelGGL(PackSamplesKernel<true>, grid, block, 0, (hipStream_t)hipStream, a, sa, diffCell, frameIndex);
        else
            hipLaunchKernelGGL(PackSamplesKernel<false>, grid, block, 0, (hipStream_t)hipStream, a, sa, 0u, 0u);
    } else if (checkerboardMode) // BLACK: the diffuse signal lives in cell 0, the specular one in cell 1 (reference Reblur.cpp:318-330, Relax.cpp:88-97); WHITE: the opposite
        hipLaunchKernelGGL(PackCheckerboardKernel, dim3((c.w + 63u) / 64u, (c.h + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)hipStream, a,
            checkerboardMode == (uint32_t)nrd::CheckerboardMode::BLACK ? 0u : 1u, options->frameIndex & 1u);
    else
        hipLaunchKernelGGL(PackInputsKernel, dim3((c.w + 63u) / 64u, (c.h + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)hipStream, a);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipPackInputs: the kernel launch failed");
}

} // namespace

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsEx(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, void* hipStream) {
    return PackInputs(d, options, nullptr, nullptr, false, hipStream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsSamples(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples, void* hipStream) {
    return PackInputs(d, options, samples, nullptr, false, hipStream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsSplit(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples,
    const NrdHipFrontEndSplit* split, void* hipStream) {
    return PackInputs(d, options, samples, split, true, hipStream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputs(const NrdHipFrontEndDesc* d, void* hipStream) { return nrdHipPackInputsEx(d, nullptr, hipStream); }

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsLobes(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSplit* split,
    const NrdHipFrontEndLobes* lobes, void* hipStream) {
    return PackInputs(d, options, nullptr, split, true, hipStream, false, lobes);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsDecimated(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples,
    const NrdHipFrontEndSplit* split, uint32_t guideShift, void* hipStream) {
    if (guideShift > 1u)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsDecimated: guideShift: 0 (the call is nrdHipPackInputsSplit) or 1 (G-buffer planes of twice the size, read at every second texel)");
    return PackInputs(d, options, samples, split, true, hipStream, guideShift == 1u);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackInputsDirect(const NrdHipFrontEndDesc* d, const NrdHipFrontEndOptions* options, const NrdHipFrontEndSamples* samples,
    const NrdHipFrontEndSplit* split, const NrdHipFrontEndDirect* direct, uint32_t guideShift, void* hipStream) {
    if (guideShift > 1u)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackInputsDirect: guideShift: 0 or 1 (G-buffer planes of twice the size, read at every second texel)");
    return PackInputs(d, options, samples, split, true, hipStream, guideShift == 1u, nullptr, direct);
}

namespace {

// splitEntry: nrdHipResolveOutputsSplit -- RGB32_SFLOAT planes and the hit-distance companions are accepted
// up: nrdHipResolveOutputsUpsampled -- the signal planes, the shadow and up->lowViewZ form the low-size class of the checker, everything else the full-size one
uint32_t ResolveOutputs(const NrdHipBackEndDesc* d, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split, bool splitEntry, void* hipStream, const NrdHipBackEndUpsample* up = nullptr) {
    using F = nrd::Format;
    static const NrdHipBackEndSplit noSplit = {};
    const NrdHipBackEndSplit& sd = split ? *split : noSplit;
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputs: null descriptor");
    const bool reJitter = options && options->reJitter;
    const NrdHipBackEndSignal &ds = d->diffuse, &ss = d->specular;
    if (ds.mode > NRD_HIP_SIGNAL_RELAX_SH || ss.mode > NRD_HIP_SIGNAL_RELAX_SH || ss.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION || ds.resolve > NRD_HIP_RESOLVE_SG ||
        ss.resolve > NRD_HIP_RESOLVE_SG)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputs: unknown signal mode or resolve (directional occlusion is a diffuse mode)");
    if (reJitter && !(IsSh(ds.mode) && IsSh(ss.mode)))
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputsEx: options: reJitter needs a diffuse and a specular signal in an SH mode (NRD_SG_ReJitter takes both SGs)");
    if (reJitter && (ds.resolve == NRD_HIP_RESOLVE_SG_EXTRACT_COLOR || ss.resolve == NRD_HIP_RESOLVE_SG_EXTRACT_COLOR))
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputsEx: options: reJitter scales a resolved colour: the resolve of both signals must be SH or SG, not SG_EXTRACT_COLOR");
    if (!reJitter && options && options->outReJitterScale.data)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputsEx: options: outReJitterScale: given without reJitter");
    const bool upsampled = up != nullptr;
    if (upsampled && reJitter)
        return Fail(nrd::Result::UNSUPPORTED, "nrdHipResolveOutputsUpsampled: options: reJitter: re-jittering needs full-size SG neighbours; combined with upsampling it is out of scope");
    if (upsampled && up->reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputsUpsampled: upsample: reserved: must be 0");
    if (upsampled && !(up->depthThreshold >= 0.0f && up->depthThreshold <= 3.402823466e+38f)) // (a NaN fails every comparison)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveOutputsUpsampled: upsample: depthThreshold: NaN, negative or infinite");
    Checker c{upsampled ? "nrdHipResolveOutputsUpsampled" : splitEntry ? "nrdHipResolveOutputsSplit" : "nrdHipResolveOutputs"};
    c.split = splitEntry;
    ReJitterArgs ra = {};
    ResolveArgs& a = ra.r;
    ResolveSplitArgs sp = {};
    BackEndSignal(c, ds, "diffuse", sd.diffuseHitDist, kSplitDiffOut, a.diffIn0, a.diffIn1, a.diffOut, sp.diffHitDist, a.diffWide, upsampled);
    BackEndSignal(c, ss, "specular", sd.specularHitDist, kSplitSpecOut, a.specIn0, a.specIn1, a.specOut, sp.specHitDist, a.specWide, upsampled);
    a.shadow = c.Check(d->shadow, "shadow", d->outShadow.data ? "outShadow needs it" : nullptr, F::R8_UNORM, F::RGBA8_UNORM);
    a.shadowIsRGBA = d->shadow.format == (uint32_t)F::RGBA8_UNORM;
    UpsampleArgs ua = {};
    if (upsampled)
        ua.lowViewZ = c.Check(up->lowViewZ, "upsample: lowViewZ", "required: the IN_VIEWZ plane the denoiser ran with", F::R32_SFLOAT);
    FullSize outputsAndGuides(c, upsampled); // from here on every plane is a full-size one
    if (upsampled)
        ua.outSource = c.Check(up->outSource, "upsample: outSource", nullptr, F::R8_UINT);
    a.outShadow = c.Check(d->outShadow, "outShadow", nullptr, a.shadowIsRGBA ? F::RGBA32_SFLOAT : F::R32_SFLOAT);
    a.outComposed = c.CheckColour(d->outComposed, "outComposed", nullptr, kSplitComposed);
    a.outViewVector = c.CheckColour(d->outViewVector, "outViewVector", nullptr, kSplitViewVector);
    a.outDiffFactor = c.CheckColour(d->outDiffFactor, "outDiffFactor", nullptr, kSplitDiffFactor);
    a.outSpecFactor = c.CheckColour(d->outSpecFactor, "outSpecFactor", nullptr, kSplitSpecFactor);
    auto resolved = [](const NrdHipBackEndSignal& s) { return IsSh(s.mode) || s.mode == NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION; };
    auto carriesColour = [](const NrdHipBackEndSignal& s) { return s.mode != NRD_HIP_SIGNAL_NONE && s.mode != NRD_HIP_SIGNAL_REBLUR_OCCLUSION; };
    const bool reblurSpec = ss.mode >= NRD_HIP_SIGNAL_REBLUR_RADIANCE && ss.mode <= NRD_HIP_SIGNAL_REBLUR_OCCLUSION;
    const bool anyReblur = reblurSpec || (ds.mode >= NRD_HIP_SIGNAL_REBLUR_RADIANCE && ds.mode <= NRD_HIP_SIGNAL_REBLUR_DIRECTIONAL_OCCLUSION);
    const bool needFactors = d->remodulate || a.outDiffFactor.ptr || a.outSpecFactor.ptr;
    const bool needV = reJitter || needFactors || a.outViewVector.ptr || (resolved(ss) && ss.resolve != NRD_HIP_RESOLVE_SG_EXTRACT_COLOR);
    const bool needN = reJitter || needFactors || (resolved(ds) && ds.resolve != NRD_HIP_RESOLVE_SG_EXTRACT_COLOR) || (resolved(ss) && ss.resolve != NRD_HIP_RESOLVE_SG_EXTRACT_COLOR) ||
        (d->denormalizeHitDist && reblurSpec);
    if (a.outComposed.ptr && !(carriesColour(ds) && carriesColour(ss)) && !c.Failed())
        c.Error(nrd::Result::INVALID_ARGUMENT, "outComposed", "needs a diffuse and a specular signal that carry a colour");
    a.normalRoughness = c.Check(d->normalRoughness, "normalRoughness", needN ? "the chosen resolves / remodulation / specular hit distance need N and the roughness" : nullptr, kNormalRoughnessFormat);
    a.viewZ = c.Check(d->viewZ, "viewZ", upsampled ? "required: nearest-Z upsampling compares it with lowViewZ" : needV || (d->denormalizeHitDist && anyReblur) ? "the view vector / denormalizeHitDist need it" : nullptr,
        F::R32_SFLOAT);
    a.albedo = c.CheckColour(d->albedo, "albedo", needFactors ? "remodulation needs albedo and rf0" : nullptr, kSplitAlbedo);
    a.rf0 = c.CheckColour(d->rf0, "rf0", needFactors ? "remodulation needs albedo and rf0" : reJitter ? "reJitter needs Rf0" : nullptr, kSplitRf0);
    if (reJitter)
        ra.outScale = c.Check(options->outReJitterScale, "outReJitterScale", nullptr, F::RG32_SFLOAT);
    c.full = false; // (Camera holds rectSize against w x h: the low size of an upsampled call)
    if (!c.Failed() && !c.w)
        c.Error(nrd::Result::INVALID_ARGUMENT, "descriptor", "nothing to do: no signal, no shadow, no output plane");
    if (needV || upsampled)
        Camera(c, d->commonSettings, upsampled ? "required: viewZScale, denoisingRange and the camera of the frame the denoiser ran with" : "the chosen resolves / remodulation / outViewVector need the frame's camera",
            a.camera);
    if (c.Failed())
        return c.result;
    a.diffMode = ds.mode;
    a.specMode = ss.mode;
    a.diffResolve = ds.resolve;
    a.specResolve = ss.resolve;
    a.denormalize = d->denormalizeHitDist ? 1u : 0u;
    a.remodulate = d->remodulate ? 1u : 0u;
    a.needV = needV ? 1u : 0u;
    a.needFactors = needFactors ? 1u : 0u;
    a.hitDistParams = make_float4(d->hitDistParams[0], d->hitDistParams[1], d->hitDistParams[2], d->hitDistParams[3]);
    a.w = c.w;
    a.h = c.h;
    t_LastError.clear();
    sp.rgb = c.rgb;
    if (upsampled) { // one thread per FULL pixel
        const nrd::CommonSettings& cs = *(const nrd::CommonSettings*)d->commonSettings;
        ua.viewZScale = cs.viewZScale;
        ua.denoisingRange = cs.denoisingRange;
        ua.depthThreshold = up->depthThreshold;
        ua.lw = c.w;
        ua.lh = c.h;
        a.w = c.fw;
        a.h = c.fh;
        const dim3 grid((c.fw + 63u) / 64u, (c.fh + 3u) / 4u), block(64, 4);
        if (c.rgb)
            hipLaunchKernelGGL(ResolveUpsampledSplitKernel, grid, block, 0, (hipStream_t)hipStream, a, sp, ua);
        else
            hipLaunchKernelGGL(ResolveUpsampledKernel, grid, block, 0, (hipStream_t)hipStream, a, ua);
        return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipResolveOutputsUpsampled: the kernel launch failed");
    }
    const dim3 reJitterGrid((c.w + (uint32_t)kReJitterTileW - 1u) / (uint32_t)kReJitterTileW, (c.h + (uint32_t)kReJitterTileH - 1u) / (uint32_t)kReJitterTileH);
    if (c.rgb && reJitter) // something to split: the twins. (Else the kernels of the old calls: the same code, the same bytes.)
        hipLaunchKernelGGL(ReJitterSplitKernel, reJitterGrid, dim3(kReJitterTileW, kReJitterTileH), 0, (hipStream_t)hipStream, ra, sp);
    else if (c.rgb)
        hipLaunchKernelGGL(ResolveOutputsSplitKernel, dim3((c.w + 63u) / 64u, (c.h + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)hipStream, a, sp);
    else if (reJitter)
        hipLaunchKernelGGL(ReJitterKernel, dim3((c.w + (uint32_t)kReJitterTileW - 1u) / (uint32_t)kReJitterTileW, (c.h + (uint32_t)kReJitterTileH - 1u) / (uint32_t)kReJitterTileH),
            dim3(kReJitterTileW, kReJitterTileH), 0, (hipStream_t)hipStream, ra);
    else
        hipLaunchKernelGGL(ResolveOutputsKernel, dim3((c.w + 63u) / 64u, (c.h + 3u) / 4u), dim3(64, 4), 0, (hipStream_t)hipStream, a);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipResolveOutputs: the kernel launch failed");
}

} // namespace

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipResolveOutputsEx(const NrdHipBackEndDesc* d, const NrdHipBackEndOptions* options, void* hipStream) {
    return ResolveOutputs(d, options, nullptr, false, hipStream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipResolveOutputsSplit(const NrdHipBackEndDesc* d, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split, void* hipStream) {
    return ResolveOutputs(d, options, split, true, hipStream);
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipResolveOutputs(const NrdHipBackEndDesc* d, void* hipStream) { return nrdHipResolveOutputsEx(d, nullptr, hipStream); }

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipResolveOutputsUpsampled(const NrdHipBackEndDesc* d, const NrdHipBackEndOptions* options, const NrdHipBackEndSplit* split,
    const NrdHipBackEndUpsample* upsample, void* hipStream) {
    return ResolveOutputs(d, options, split, true, hipStream, upsample);
}
