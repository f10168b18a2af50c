// Guides from world positions on the device (include/NRDHip.h nrdHipPackGuides): IN_VIEWZ and IN_MV derived from a path tracer's world-space hit positions and the matrices of
// nrd::CommonSettings, and the four optional UNORM slots (IN_BASECOLOR_METALNESS, IN_DIFF_CONFIDENCE, IN_SPEC_CONFIDENCE, IN_DISOCCLUSION_THRESHOLD_MIX) encoded from fp32
// planes -- one streaming kernel, one launch. One thread per pixel, 64 x 4 workgroups, as in kernels_frontend.hip: a wave covers 64 consecutive pixels of one row, so every load
// and store of a wave is one contiguous segment per plane (16 B per lane for an RGBA32_SFLOAT plane, 12 B for an RGB32_SFLOAT one, never a 16-byte access to a 12-byte texel).
// Every input texel is read once, nothing goes through LDS or scratch. The two cameras, the motion-vector scale and the miss depth travel in the kernel arguments: they are
// wave-uniform, so they sit in scalar registers. The kernel is instantiated per texel size of `position` (none / 12 / 16) and of `positionPrev` (none / 12 / 16); which outputs
// exist and the motion-vector mode are uniforms of the launch: scalar branches.
//
// Arithmetic: the text of NRDHip.h and nothing else, unfused (the pragma below, in front of every include) with correctly rounded division. The stores are the codecs of planes.h.
#pragma clang fp contract(off)

#include "NRD.h"
#include "NRDHip.h"

#include "planes.h"
#include "frontend_host.h"

#include "../host/hostmath.h"

#include <cmath>
#include <string>

using namespace nrdhip;

namespace {

// one frame's camera: rows of the rotation of world-to-view with the camera position in .w (row i: R[ i ][ 0..2 ], c[ i ]); rows 0, 1 and 3 of view-to-clip
struct GuideCamera {
    float4 r0, r1, r2;
    float4 p0, p1, p3;
};

struct GuidesArgs {
    FePlane position, positionPrev, baseColor, metalness, diffConfidence, specConfidence, mix;
    FePlane outViewZ, outMv, outBaseColorMetalness, outDiffConfidence, outSpecConfidence, outMix;
    GuideCamera cur, prev;
    float4 mvScale; // motionVectorScale, .w unused
    float missViewZ;
    int32_t w, h;
    uint32_t world, baseColorBytes;
};

__device__ __forceinline__ Plane AsPlane(const FePlane& p, int w, int h) { return Plane{p.ptr, p.pitch, w, h}; }

__device__ __forceinline__ bool IsFinite(float v) { return fabsf(v) <= 3.402823466e+38f; } // (a NaN fails every comparison)
__device__ __forceinline__ bool IsFinite(float3 v) { return IsFinite(v.x) && IsFinite(v.y) && IsFinite(v.z); }

// `.xyz` of a position or colour texel: BYTES = 16 reads the whole texel with one 16-byte load (.w is carried and never looked at), BYTES = 12 the three packed dwords
template <uint32_t BYTES>
__device__ __forceinline__ float3 LoadXyz(const FePlane& p, int x, int y, int w, int h) {
    if constexpr (BYTES == 16u) {
        float4 v = LoadRGBA32F(AsPlane(p, w, h), x, y);
        NRD_LDS_WHOLE_TEXEL(v); // keeps the four components together: global_load_dwordx4
        return make_float3(v.x, v.y, v.z);
    } else
        return LoadRGB32F(AsPlane(p, w, h), x, y);
}

// Xv = R . ( X - c ): the subtraction first, sums as ( a * x + b * y ) + c * z
__device__ __forceinline__ float3 ToView(const GuideCamera& c, float3 X) {
    const float dx = X.x - c.r0.w, dy = X.y - c.r1.w, dz = X.z - c.r2.w;
    return make_float3((c.r0.x * dx + c.r0.y * dy) + c.r0.z * dz, (c.r1.x * dx + c.r1.y * dy) + c.r1.z * dz, (c.r2.x * dx + c.r2.y * dy) + c.r2.z * dz);
}

__device__ __forceinline__ float ClipRow(float4 row, float3 Xv) { return ((row.x * Xv.x + row.y * Xv.y) + row.z * Xv.z) + row.w; }

// GetScreenUv (nrdmath.h) of a view-space position
__device__ __forceinline__ float2 ScreenUv(const GuideCamera& c, float3 Xv) {
    const float cx = ClipRow(c.p0, Xv), cy = ClipRow(c.p1, Xv), cw = ClipRow(c.p3, Xv);
    const float u = cx / cw * 0.5f + 0.5f, v = cy / cw * -0.5f + 0.5f;
    return cw < 0.0f ? make_float2(99999.0f, 99999.0f) : make_float2(u, v);
}

__device__ __forceinline__ float DivOrZero(float a, float s) { return s != 0.0f ? a / s : 0.0f; }
__device__ __forceinline__ float ToHalfRange(float v) { return v != v ? 0.0f : fminf(fmaxf(v, -65504.0f), 65504.0f); }

template <uint32_t POS_BYTES, uint32_t PREV_BYTES>
__global__ void __launch_bounds__(256) PackGuidesKernel(const GuidesArgs a) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = a.w, h = a.h;
    if (x >= w || y >= h)
        return;
    // every load of the pixel first
    float3 X = make_float3(0.0f, 0.0f, 0.0f), Xp = X, baseColor = X;
    float metalness = 0.0f, diffConfidence = 0.0f, specConfidence = 0.0f, mix = 0.0f;
    if constexpr (POS_BYTES != 0u)
        X = LoadXyz<POS_BYTES>(a.position, x, y, w, h);
    if constexpr (PREV_BYTES != 0u)
        Xp = LoadXyz<PREV_BYTES>(a.positionPrev, x, y, w, h);
    if (a.outBaseColorMetalness.ptr) {
        baseColor = a.baseColorBytes == 16u ? LoadXyz<16u>(a.baseColor, x, y, w, h) : LoadXyz<12u>(a.baseColor, x, y, w, h); // (a uniform: a scalar branch)
        metalness = LoadR32F(AsPlane(a.metalness, w, h), x, y);
    }
    if (a.outDiffConfidence.ptr)
        diffConfidence = LoadR32F(AsPlane(a.diffConfidence, w, h), x, y);
    if (a.outSpecConfidence.ptr)
        specConfidence = LoadR32F(AsPlane(a.specConfidence, w, h), x, y);
    if (a.outMix.ptr)
        mix = LoadR32F(AsPlane(a.mix, w, h), x, y);

    if constexpr (POS_BYTES != 0u) {
        const bool hit = IsFinite(X);
        const float3 Xv = ToView(a.cur, X);
        if (a.outViewZ.ptr)
            StoreR32F(AsPlane(a.outViewZ, w, h), x, y, hit ? Xv.z : a.missViewZ);
        if (a.outMv.ptr) {
            if (PREV_BYTES == 0u || !IsFinite(Xp))
                Xp = X;
            float3 mv;
            if (a.world) {
                mv = make_float3(DivOrZero(Xp.x - X.x, a.mvScale.x), DivOrZero(Xp.y - X.y, a.mvScale.y), DivOrZero(Xp.z - X.z, a.mvScale.z));
            } else {
                const float3 Xvp = ToView(a.prev, Xp);
                const float2 uv = ScreenUv(a.cur, Xv), uvp = ScreenUv(a.prev, Xvp);
                mv = make_float3((uvp.x - uv.x) / a.mvScale.x, (uvp.y - uv.y) / a.mvScale.y, DivOrZero(fabsf(Xvp.z) - fabsf(Xv.z), a.mvScale.z)); // the passes take abs( IN_VIEWZ )
            }
            const float4 stored = hit ? make_float4(ToHalfRange(mv.x), ToHalfRange(mv.y), ToHalfRange(mv.z), 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            StoreRGBA16F(AsPlane(a.outMv, w, h), x, y, stored);
        }
    }
    if (a.outBaseColorMetalness.ptr)
        StoreRGBA8Unorm(AsPlane(a.outBaseColorMetalness, w, h), x, y, make_float4(baseColor.x, baseColor.y, baseColor.z, metalness));
    if (a.outDiffConfidence.ptr)
        StoreR8Unorm(AsPlane(a.outDiffConfidence, w, h), x, y, diffConfidence);
    if (a.outSpecConfidence.ptr)
        StoreR8Unorm(AsPlane(a.outSpecConfidence, w, h), x, y, specConfidence);
    if (a.outMix.ptr)
        StoreR8Unorm(AsPlane(a.outMix, w, h), x, y, mix);
}

// ---- host side: validation (all of it in front of the first HIP call) and the launch ---------------------------------------------------------------
// rotation rows and camera position of a world-to-view matrix (the camera position is the translation of its rigid inverse, as csrc/host/instance.cpp takes it), rows 0, 1, 3 of
// view-to-clip: the caller's matrices as given
GuideCamera MakeCamera(const float* worldToViewMatrix, const float* viewToClipMatrix) {
    using namespace nrdhost;
    const Mat4 worldToView = Mat4::FromColumnMajor(worldToViewMatrix), viewToClip = Mat4::FromColumnMajor(viewToClipMatrix);
    const Mat4 viewToWorld = InvertRigid(worldToView);
    GuideCamera c;
    c.r0 = make_float4(worldToView.at(0, 0), worldToView.at(0, 1), worldToView.at(0, 2), viewToWorld.at(0, 3));
    c.r1 = make_float4(worldToView.at(1, 0), worldToView.at(1, 1), worldToView.at(1, 2), viewToWorld.at(1, 3));
    c.r2 = make_float4(worldToView.at(2, 0), worldToView.at(2, 1), worldToView.at(2, 2), viewToWorld.at(2, 3));
    c.p0 = make_float4(viewToClip.at(0, 0), viewToClip.at(0, 1), viewToClip.at(0, 2), viewToClip.at(0, 3));
    c.p1 = make_float4(viewToClip.at(1, 0), viewToClip.at(1, 1), viewToClip.at(1, 2), viewToClip.at(1, 3));
    c.p3 = make_float4(viewToClip.at(3, 0), viewToClip.at(3, 1), viewToClip.at(3, 2), viewToClip.at(3, 3));
    return c;
}

bool IsOrtho(const float* viewToClipMatrix) { return nrdhost::DecomposeProjection(nrdhost::Mat4::FromColumnMajor(viewToClipMatrix)).isOrtho; }

typedef void (*GuidesKernel)(const GuidesArgs);

GuidesKernel PickKernel(uint32_t posBytes, uint32_t prevBytes) {
    if (posBytes == 0u)
        return PackGuidesKernel<0u, 0u>;
    if (posBytes == 12u)
        return prevBytes == 0u ? PackGuidesKernel<12u, 0u> : prevBytes == 12u ? PackGuidesKernel<12u, 12u> : PackGuidesKernel<12u, 16u>;
    return prevBytes == 0u ? PackGuidesKernel<16u, 0u> : prevBytes == 12u ? PackGuidesKernel<16u, 12u> : PackGuidesKernel<16u, 16u>;
}

} // namespace

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackGuides(const NrdHipGuidesDesc* d, void* hipStream) {
    using F = nrd::Format;
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackGuides: null descriptor");
    if (d->reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackGuides: reserved: must be 0");
    const bool wantViewZ = d->outViewZ.data != nullptr, wantMv = d->outMv.data != nullptr, wantCamera = wantViewZ || wantMv;
    const bool wantBcm = d->outBaseColorMetalness.data != nullptr;
    if (!wantCamera && !wantBcm && !d->outDiffConfidence.data && !d->outSpecConfidence.data && !d->outDisocclusionThresholdMix.data)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackGuides: no output: every out* plane is absent");
    Checker c{"nrdHipPackGuides"};
    GuidesArgs a = {};
    if (!wantCamera)
        Refuse(c, d->position, "position", "given without outViewZ or outMv: nothing would consume it");
    if (!wantMv)
        Refuse(c, d->positionPrev, "positionPrev", "given without outMv: nothing would consume it");
    if (!wantBcm) {
        Refuse(c, d->baseColor, "baseColor", "given without outBaseColorMetalness: nothing would consume it");
        Refuse(c, d->metalness, "metalness", "given without outBaseColorMetalness: nothing would consume it");
    }
    if (!d->outDiffConfidence.data)
        Refuse(c, d->diffConfidence, "diffConfidence", "given without outDiffConfidence: nothing would consume it");
    if (!d->outSpecConfidence.data)
        Refuse(c, d->specConfidence, "specConfidence", "given without outSpecConfidence: nothing would consume it");
    if (!d->outDisocclusionThresholdMix.data)
        Refuse(c, d->disocclusionThresholdMix, "disocclusionThresholdMix", "given without outDisocclusionThresholdMix: nothing would consume it");
    a.position = c.Check(d->position, "position", wantCamera ? "outViewZ / outMv are derived from it" : nullptr, F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    a.positionPrev = c.Check(d->positionPrev, "positionPrev", nullptr, F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    a.baseColor = c.Check(d->baseColor, "baseColor", wantBcm ? "outBaseColorMetalness needs it" : nullptr, F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    a.metalness = c.Check(d->metalness, "metalness", wantBcm ? "outBaseColorMetalness needs it" : nullptr, F::R32_SFLOAT);
    a.diffConfidence = c.Check(d->diffConfidence, "diffConfidence", d->outDiffConfidence.data ? "outDiffConfidence needs it" : nullptr, F::R32_SFLOAT);
    a.specConfidence = c.Check(d->specConfidence, "specConfidence", d->outSpecConfidence.data ? "outSpecConfidence needs it" : nullptr, F::R32_SFLOAT);
    a.mix = c.Check(d->disocclusionThresholdMix, "disocclusionThresholdMix", d->outDisocclusionThresholdMix.data ? "outDisocclusionThresholdMix needs it" : nullptr, F::R32_SFLOAT);
    a.outViewZ = c.Check(d->outViewZ, "outViewZ", nullptr, F::R32_SFLOAT);
    a.outMv = c.Check(d->outMv, "outMv", nullptr, F::RGBA16_SFLOAT);
    a.outBaseColorMetalness = c.Check(d->outBaseColorMetalness, "outBaseColorMetalness", nullptr, F::RGBA8_UNORM);
    a.outDiffConfidence = c.Check(d->outDiffConfidence, "outDiffConfidence", nullptr, F::R8_UNORM);
    a.outSpecConfidence = c.Check(d->outSpecConfidence, "outSpecConfidence", nullptr, F::R8_UNORM);
    a.outMix = c.Check(d->outDisocclusionThresholdMix, "outDisocclusionThresholdMix", nullptr, F::R8_UNORM);
    if (wantCamera && !c.Failed()) {
        if (!d->commonSettings)
            c.Error(nrd::Result::INVALID_ARGUMENT, "commonSettings", "NULL: outViewZ / outMv are derived with the matrices of the frame");
        else {
            const nrd::CommonSettings& cs = *(const nrd::CommonSettings*)d->commonSettings;
            const float* s = cs.motionVectorScale;
            a.world = cs.isMotionVectorInWorldSpace ? 1u : 0u;
            if (IsOrtho(cs.viewToClipMatrix) || (wantMv && !a.world && IsOrtho(cs.viewToClipMatrixPrev)))
                c.Error(nrd::Result::UNSUPPORTED, "commonSettings", "orthographic projections are not supported");
            else if (cs.rectSize[0] != c.w || cs.rectSize[1] != c.h)
                c.Error(nrd::Result::INVALID_ARGUMENT, "commonSettings", "rectSize is not the size of the planes");
            else if (wantViewZ && !(std::fabs(d->missViewZ) <= 3.402823466e+38f))
                c.Error(nrd::Result::INVALID_ARGUMENT, "missViewZ", "NaN or infinite");
            else if (wantViewZ && !(std::fabs(d->missViewZ * cs.viewZScale) > cs.denoisingRange))
                c.Error(nrd::Result::INVALID_ARGUMENT, "missViewZ", "abs( missViewZ * commonSettings.viewZScale ) is not above denoisingRange: the passes would not take the pixel for sky");
            else if (wantMv && !a.world && (s[0] == 0.0f || s[1] == 0.0f))
                c.Error(nrd::Result::INVALID_ARGUMENT, "commonSettings", "motionVectorScale .x or .y is 0 in screen-space mode: no vector stored could give the motion back");
            else {
                a.cur = MakeCamera(cs.worldToViewMatrix, cs.viewToClipMatrix);
                a.prev = MakeCamera(cs.worldToViewMatrixPrev, cs.viewToClipMatrixPrev);
                a.mvScale = make_float4(s[0], s[1], s[2], 0.0f);
            }
        }
    }
    if (c.Failed())
        return c.result;
    a.missViewZ = d->missViewZ;
    a.baseColorBytes = IsRgb(d->baseColor) ? 12u : 16u;
    a.w = c.w;
    a.h = c.h;
    const uint32_t posBytes = a.position.ptr ? (IsRgb(d->position) ? 12u : 16u) : 0u;
    const uint32_t prevBytes = a.positionPrev.ptr ? (IsRgb(d->positionPrev) ? 12u : 16u) : 0u;
    t_LastError.clear();
    const dim3 grid((c.w + 63u) / 64u, (c.h + 3u) / 4u), block(64, 4);
    const GuidesKernel kernel = PickKernel(posBytes, prevBytes);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)hipStream, a);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipPackGuides: the kernel launch failed");
}
