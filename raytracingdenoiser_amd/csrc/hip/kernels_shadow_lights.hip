// SIGMA shadows for local and many lights on the device (include/NRDHip.h nrdHipPackShadowLights / nrdHipResolveShadowLights): the two recipes of the reference README for several
// lights -- SIGMA applied per light, and the single pass through SIGMA_SHADOW_TRANSLUCENCY -- as streaming kernels over N light layers. One thread per pixel, 64 x 4 workgroups,
// as in kernels_frontend.hip: a wave covers 64 consecutive pixels of one row, so every load and store of a wave is one contiguous segment per layer and plane. The lights come by
// value in the kernel arguments (512 bytes): the light index is wave-uniform, so a light's parameters are scalar loads and the branch on its type is a scalar branch. Layer bases
// advance by scalar 64-bit additions; the loads of four lights are issued before the first of them is consumed. Only the loads the formulas need are made: layer i of
// distanceToLight is read if light i is LOCAL, the colour / weight stacks if the mode takes them.
//
// Arithmetic: include/NRD.hip.h and nothing else, unfused (the pragma below, in front of every include) with correctly rounded division. The stores are the codecs of planes.h.
#pragma clang fp contract(off)

#include "NRD.h"
#include "NRDHip.h"

#include "NRD.hip.h"

#include "planes.h"
#include "frontend_host.h"

#include <cmath>
#include <string>

using namespace nrdhip;

namespace {

struct LightTable {
    NrdHipShadowLight light[NRD_HIP_MAX_SHADOW_LIGHTS];
};

// colour: translucency (PER_LIGHT) or lighting (COMBINED), 12- or 16-byte texels of which .xyz is read
struct PackLightsArgs {
    FePlane occluder, lightDist, colour, weight, outPenumbra, outTranslucency, outLightingSum;
    uint64_t occluderLayer, lightDistLayer, colourLayer, weightLayer, outPenumbraLayer, outTranslucencyLayer;
    int32_t w, h;
    uint32_t num, colourBytes, outSumBytes;
};

struct ResolveLightsArgs {
    FePlane shadow, lighting, out;
    uint64_t shadowLayer, lightingLayer;
    int32_t w, h;
    uint32_t num, shadowIsRGBA, lightingBytes, outBytes;
};

constexpr uint32_t kBatch = 4;

__device__ __forceinline__ Plane AsPlane(const FePlane& p, int w, int h) { return Plane{p.ptr, p.pitch, w, h}; }

// what one light contributes to one pixel, as loaded (a plane that is not read gives zeros)
struct LightTexel {
    float d, dl, weight;
    float3 colour;
};

// the current layer of every input stack
struct LightLayers {
    Plane occluder, lightDist, colour, weight;
};

__device__ __forceinline__ LightLayers FirstLayers(const PackLightsArgs& a) {
    return LightLayers{AsPlane(a.occluder, a.w, a.h), AsPlane(a.lightDist, a.w, a.h), AsPlane(a.colour, a.w, a.h), AsPlane(a.weight, a.w, a.h)};
}

// loads light `type`'s texel of the current layers and steps to the next layer; everything but (x, y) is wave-uniform
__device__ __forceinline__ LightTexel LoadLight(LightLayers& l, const PackLightsArgs& a, uint32_t type, int x, int y) {
    LightTexel t = {0.0f, 0.0f, 0.0f, make_float3(0.0f, 0.0f, 0.0f)};
    t.d = LoadR32F(l.occluder, x, y);
    if (type == NRD_HIP_LIGHT_LOCAL)
        t.dl = LoadR32F(l.lightDist, x, y);
    if (a.colour.ptr)
        t.colour = LoadXyz32F(l.colour, x, y, a.colourBytes);
    if (a.weight.ptr)
        t.weight = LoadR32F(l.weight, x, y);
    l.occluder.ptr += a.occluderLayer;
    l.lightDist.ptr += a.lightDistLayer;
    l.colour.ptr += a.colourLayer;
    l.weight.ptr += a.weightLayer;
    return t;
}

__device__ __forceinline__ float Penumbra(const NrdHipShadowLight& light, const LightTexel& t) {
    return light.type == NRD_HIP_LIGHT_LOCAL ? SIGMA_FrontEnd_PackPenumbra(t.d, t.dl, light.lightSize) : SIGMA_FrontEnd_PackPenumbra(t.d, light.tanOfLightAngularRadius);
}

// ---- PER_LIGHT: layer i of the outputs is what the plain pack kernel writes for light i
__device__ __forceinline__ void StoreLight(Plane& outPenumbra, Plane& outTranslucency, const PackLightsArgs& a, const NrdHipShadowLight& light, const LightTexel& t, int x, int y) {
    StoreR16F(outPenumbra, x, y, Penumbra(light, t));
    outPenumbra.ptr += a.outPenumbraLayer;
    if (a.outTranslucency.ptr) {
        StoreRGBA8Unorm(outTranslucency, x, y, SIGMA_FrontEnd_PackTranslucency(t.d, t.colour));
        outTranslucency.ptr += a.outTranslucencyLayer;
    }
}

__global__ void __launch_bounds__(256) PackLightsPerLightKernel(const PackLightsArgs a, const LightTable lights) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.w || y >= a.h)
        return;
    LightLayers layers = FirstLayers(a);
    Plane outPenumbra = AsPlane(a.outPenumbra, a.w, a.h), outTranslucency = AsPlane(a.outTranslucency, a.w, a.h);
    uint32_t i = 0;
    for (; i + kBatch <= a.num; i += kBatch) {
        LightTexel t[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            t[k] = LoadLight(layers, a, lights.light[i + k].type, x, y);
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            StoreLight(outPenumbra, outTranslucency, a, lights.light[i + k], t[k], x, y);
    }
    for (; i < a.num; i++) {
        const LightTexel t = LoadLight(layers, a, lights.light[i].type, x, y);
        StoreLight(outPenumbra, outTranslucency, a, lights.light[i], t, x, y);
    }
}

// ---- COMBINED: the sums of NRDHip.h, light by light in index order
struct LightSums {
    float3 L, LS;
    float W, P, dMin;
};

__device__ __forceinline__ void AddLight(LightSums& s, const PackLightsArgs& a, const NrdHipShadowLight& light, const LightTexel& t) {
    const float3 L = t.colour;
    s.L = make_float3(s.L.x + L.x, s.L.y + L.y, s.L.z + L.z);
    const bool lit = t.d >= NRD_FP16_MAX;
    const float shadow = lit ? 1.0f : 0.0f;
    s.LS = make_float3(s.LS.x + L.x * shadow, s.LS.y + L.y * shadow, s.LS.z + L.z * shadow);
    const float w = (a.weight.ptr ? t.weight : (lit ? 0.0f : 1.0f)) * _NRD_Luminance(L);
    s.W = s.W + w;
    s.P = s.P + Penumbra(light, t) * w;
    s.dMin = fminf(s.dMin, t.d);
}

__global__ void __launch_bounds__(256) PackLightsCombinedKernel(const PackLightsArgs a, const LightTable lights) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    const int w = a.w, h = a.h;
    if (x >= w || y >= h)
        return;
    LightLayers layers = FirstLayers(a);
    LightSums s = {make_float3(0.0f, 0.0f, 0.0f), make_float3(0.0f, 0.0f, 0.0f), 0.0f, 0.0f, INFINITY};
    uint32_t i = 0;
    for (; i + kBatch <= a.num; i += kBatch) {
        LightTexel t[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            t[k] = LoadLight(layers, a, lights.light[i + k].type, x, y);
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            AddLight(s, a, lights.light[i + k], t[k]);
    }
    for (; i < a.num; i++) {
        const LightTexel t = LoadLight(layers, a, lights.light[i].type, x, y);
        AddLight(s, a, lights.light[i], t);
    }
    const float3 translucency = make_float3(s.LS.x / fmaxf(s.L.x, NRD_EPS), s.LS.y / fmaxf(s.L.y, NRD_EPS), s.LS.z / fmaxf(s.L.z, NRD_EPS));
    const float penumbra = s.dMin >= NRD_FP16_MAX ? NRD_FP16_MAX : s.P / fmaxf(s.W, NRD_EPS);
    StoreR16F(AsPlane(a.outPenumbra, w, h), x, y, penumbra);
    StoreRGBA8Unorm(AsPlane(a.outTranslucency, w, h), x, y, SIGMA_FrontEnd_PackTranslucency(s.dMin, translucency));
    if (a.outSumBytes == 12u)
        StoreRGB32F(AsPlane(a.outLightingSum, w, h), x, y, s.L);
    else
        StoreRGBA32F(AsPlane(a.outLightingSum, w, h), x, y, make_float4(s.L.x, s.L.y, s.L.z, 0.0f));
}

// ---- resolve
__device__ __forceinline__ void StoreResolved(const ResolveLightsArgs& a, int x, int y, float4 c) {
    if (a.outBytes == 12u)
        StoreRGB32F(AsPlane(a.out, a.w, a.h), x, y, make_float3(c.x, c.y, c.z));
    else
        StoreRGBA32F(AsPlane(a.out, a.w, a.h), x, y, c);
}

__global__ void __launch_bounds__(256) ResolveLightsCombinedKernel(const ResolveLightsArgs a) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.w || y >= a.h)
        return;
    const float4 s = SIGMA_BackEnd_UnpackShadow(LoadRGBA8Unorm(AsPlane(a.shadow, a.w, a.h), x, y));
    const float3 L = LoadXyz32F(AsPlane(a.lighting, a.w, a.h), x, y, a.lightingBytes);
    StoreResolved(a, x, y, make_float4(L.x * s.y, L.y * s.z, L.z * s.w, s.x));
}

struct ShadowedLight {
    float3 L, s;
};

__device__ __forceinline__ ShadowedLight LoadShadowedLight(Plane& shadow, Plane& lighting, const ResolveLightsArgs& a, int x, int y) {
    ShadowedLight t;
    if (a.shadowIsRGBA) {
        const float4 s = SIGMA_BackEnd_UnpackShadow(LoadRGBA8Unorm(shadow, x, y));
        t.s = make_float3(s.y, s.z, s.w);
    } else {
        const float s = SIGMA_BackEnd_UnpackShadow(LoadR8Unorm(shadow, x, y));
        t.s = make_float3(s, s, s);
    }
    t.L = LoadXyz32F(lighting, x, y, a.lightingBytes);
    shadow.ptr += a.shadowLayer;
    lighting.ptr += a.lightingLayer;
    return t;
}

__device__ __forceinline__ float3 AddShadowed(float3 acc, const ShadowedLight& t) { return make_float3(acc.x + t.L.x * t.s.x, acc.y + t.L.y * t.s.y, acc.z + t.L.z * t.s.z); }

__global__ void __launch_bounds__(256) ResolveLightsPerLightKernel(const ResolveLightsArgs a) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.w || y >= a.h)
        return;
    Plane shadow = AsPlane(a.shadow, a.w, a.h), lighting = AsPlane(a.lighting, a.w, a.h);
    float3 acc = make_float3(0.0f, 0.0f, 0.0f);
    uint32_t i = 0;
    for (; i + kBatch <= a.num; i += kBatch) {
        ShadowedLight t[kBatch];
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            t[k] = LoadShadowedLight(shadow, lighting, a, x, y);
#pragma unroll
        for (uint32_t k = 0; k < kBatch; k++)
            acc = AddShadowed(acc, t[k]);
    }
    for (; i < a.num; i++)
        acc = AddShadowed(acc, LoadShadowedLight(shadow, lighting, a, x, y));
    StoreResolved(a, x, y, make_float4(acc.x, acc.y, acc.z, 0.0f));
}

// ---- host side: validation (all of it in front of the first HIP call) and the launch ---------------------------------------------------------------
uint32_t CheckCount(const char* entry, uint32_t mode, uint32_t lightsNum) {
    if (mode > NRD_HIP_SHADOWS_COMBINED)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": mode: unknown (NRD_HIP_SHADOWS_PER_LIGHT or NRD_HIP_SHADOWS_COMBINED)");
    if (!lightsNum || lightsNum > NRD_HIP_MAX_SHADOW_LIGHTS)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": lightsNum: 0 or more than " + std::to_string(NRD_HIP_MAX_SHADOW_LIGHTS) + " lights");
    return (uint32_t)nrd::Result::SUCCESS;
}

} // namespace

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPackShadowLights(const NrdHipShadowLightsPackDesc* d, void* hipStream) {
    using F = nrd::Format;
    const char* entry = "nrdHipPackShadowLights";
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackShadowLights: null descriptor");
    if (uint32_t r = CheckCount(entry, d->mode, d->lightsNum))
        return r;
    if (!d->lights)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipPackShadowLights: lights: NULL");
    const bool combined = d->mode == NRD_HIP_SHADOWS_COMBINED;
    const uint32_t num = d->lightsNum;
    LightTable table = {};
    bool anyLocal = false;
    for (uint32_t i = 0; i < num; i++) {
        const NrdHipShadowLight& l = d->lights[i];
        const std::string field = std::string(entry) + ": lights[" + std::to_string(i) + "].";
        if (l.type > NRD_HIP_LIGHT_LOCAL)
            return Fail(nrd::Result::INVALID_ARGUMENT, field + "type: unknown (NRD_HIP_LIGHT_DIRECTIONAL or NRD_HIP_LIGHT_LOCAL)");
        if (l.reserved)
            return Fail(nrd::Result::INVALID_ARGUMENT, field + "reserved: must be 0");
        const bool local = l.type == NRD_HIP_LIGHT_LOCAL;
        const float v = local ? l.lightSize : l.tanOfLightAngularRadius;
        if (!(v >= 0.0f && v < INFINITY)) // (a NaN fails every comparison)
            return Fail(nrd::Result::INVALID_ARGUMENT, field + (local ? "lightSize" : "tanOfLightAngularRadius") + ": NaN, negative or infinite");
        anyLocal |= local;
        table.light[i] = l;
    }
    Checker c{entry};
    PackLightsArgs a = {};
    a.occluder = c.Check(d->distanceToOccluder, "distanceToOccluder", "required", F::R32_SFLOAT);
    a.lightDist = c.Check(d->distanceToLight, "distanceToLight", anyLocal ? "a LOCAL light needs it" : nullptr, F::R32_SFLOAT);
    a.outPenumbra = c.Check(d->outPenumbra, "outPenumbra", "required", F::R16_SFLOAT);
    a.outTranslucency = c.Check(d->outTranslucency, "outTranslucency", combined ? "the COMBINED mode writes the pseudo translucency there" : nullptr, F::RGBA8_UNORM);
    if (combined) {
        Refuse(c, d->translucency, "translucency", "not taken in the COMBINED mode (the translucency it packs is that of the lights' sum)");
        a.colour = c.Check(d->lighting, "lighting", "the COMBINED mode needs the unshadowed lighting of every light", F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
        a.weight = c.Check(d->weight, "weight", nullptr, F::R32_SFLOAT);
        a.outLightingSum = c.Check(d->outLightingSum, "outLightingSum", "the COMBINED mode writes the lights' sum there", F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    } else {
        Refuse(c, d->weight, "weight", "not taken in the PER_LIGHT mode");
        Refuse(c, d->lighting, "lighting", "not taken by the PER_LIGHT pack (nrdHipResolveShadowLights reads it)");
        Refuse(c, d->outLightingSum, "outLightingSum", "not taken in the PER_LIGHT mode");
        if (!d->outTranslucency.data)
            Refuse(c, d->translucency, "translucency", "given without outTranslucency: nothing would consume it");
        a.colour = c.Check(d->translucency, "translucency", a.outTranslucency.ptr ? "outTranslucency needs it" : nullptr, F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    }
    const NrdHipPlaneDesc& colourDesc = combined ? d->lighting : d->translucency;
    CheckLayerBytes(c, a.occluderLayer = d->distanceToOccluderLayerBytes, a.occluder, num, "distanceToOccluderLayerBytes", true);
    CheckLayerBytes(c, a.lightDistLayer = d->distanceToLightLayerBytes, anyLocal ? a.lightDist : FePlane{nullptr, 0}, num, "distanceToLightLayerBytes", true);
    CheckLayerBytes(c, a.colourLayer = combined ? d->lightingLayerBytes : d->translucencyLayerBytes, a.colour, num, combined ? "lightingLayerBytes" : "translucencyLayerBytes", IsRgb(colourDesc));
    CheckLayerBytes(c, a.weightLayer = d->weightLayerBytes, a.weight, num, "weightLayerBytes", true);
    if (!combined) {
        CheckLayerBytes(c, a.outPenumbraLayer = d->outPenumbraLayerBytes, a.outPenumbra, num, "outPenumbraLayerBytes", true);
        CheckLayerBytes(c, a.outTranslucencyLayer = d->outTranslucencyLayerBytes, a.outTranslucency, num, "outTranslucencyLayerBytes", true);
    }
    if (c.Failed())
        return c.result;
    if (!anyLocal)
        a.lightDist = FePlane{nullptr, 0};
    a.colourBytes = IsRgb(colourDesc) ? 12u : 16u;
    a.outSumBytes = IsRgb(d->outLightingSum) ? 12u : 16u;
    a.w = c.w;
    a.h = c.h;
    a.num = num;
    t_LastError.clear();
    const dim3 grid((c.w + 63u) / 64u, (c.h + 3u) / 4u), block(64, 4);
    if (combined)
        hipLaunchKernelGGL(PackLightsCombinedKernel, grid, block, 0, (hipStream_t)hipStream, a, table);
    else
        hipLaunchKernelGGL(PackLightsPerLightKernel, grid, block, 0, (hipStream_t)hipStream, a, table);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipPackShadowLights: the kernel launch failed");
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipResolveShadowLights(const NrdHipShadowLightsResolveDesc* d, void* hipStream) {
    using F = nrd::Format;
    const char* entry = "nrdHipResolveShadowLights";
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, "nrdHipResolveShadowLights: null descriptor");
    if (uint32_t r = CheckCount(entry, d->mode, d->lightsNum))
        return r;
    const bool combined = d->mode == NRD_HIP_SHADOWS_COMBINED;
    const uint32_t num = combined ? 1u : d->lightsNum;
    Checker c{entry};
    ResolveLightsArgs a = {};
    if (combined)
        a.shadow = c.Check(d->shadow, "shadow", "required", F::RGBA8_UNORM);
    else
        a.shadow = c.Check(d->shadow, "shadow", "required", F::R8_UNORM, F::RGBA8_UNORM);
    a.lighting = c.Check(d->lighting, "lighting", "required", F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    a.out = c.Check(d->out, "out", "required", F::RGBA32_SFLOAT, F::RGB32_SFLOAT);
    CheckLayerBytes(c, a.shadowLayer = d->shadowLayerBytes, a.shadow, num, "shadowLayerBytes", true);
    CheckLayerBytes(c, a.lightingLayer = d->lightingLayerBytes, a.lighting, num, "lightingLayerBytes", IsRgb(d->lighting));
    if (c.Failed())
        return c.result;
    a.shadowIsRGBA = d->shadow.format == (uint32_t)F::RGBA8_UNORM;
    a.lightingBytes = IsRgb(d->lighting) ? 12u : 16u;
    a.outBytes = IsRgb(d->out) ? 12u : 16u;
    a.w = c.w;
    a.h = c.h;
    a.num = num;
    t_LastError.clear();
    const dim3 grid((c.w + 63u) / 64u, (c.h + 3u) / 4u), block(64, 4);
    if (combined)
        hipLaunchKernelGGL(ResolveLightsCombinedKernel, grid, block, 0, (hipStream_t)hipStream, a);
    else
        hipLaunchKernelGGL(ResolveLightsPerLightKernel, grid, block, 0, (hipStream_t)hipStream, a);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, "nrdHipResolveShadowLights: the kernel launch failed");
}
