// IntegrationHip::PackShadowLights / ResolveShadowLights (nrdHipPackShadowLights / nrdHipResolveShadowLights) used the way an application would: include/NRD.h +
// include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against libNRD_hip.so.
//   host part: the two methods forward to the library -- invalid descriptors are refused with a text that names the field, nothing is enqueued (no device is touched)
//   GPU part:  a 70 x 6 frame, two LOCAL lights whose values are exact in every format: the per-light penumbra layers, the combined planes and both resolves
// usage: shadow_lights_integration [--no-gpu]
#include "NRD.h"
#include "NRDHip.h"
#include "NRDIntegrationHip.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x)                                            \
    do {                                                    \
        if (!(x)) {                                         \
            printf("FAILED: %s (line %d)\n", #x, __LINE__); \
            return 1;                                       \
        }                                                   \
    } while (0)

int main(int argc, char** argv) {
    const bool noGpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
    const uint16_t W = 70, H = 6;
    const size_t px = (size_t)W * H;
    nrd::IntegrationHip nrdi; // the two calls need no instance: they run on the integration's stream (the default one here)

    NrdHipShadowLight lights[2] = {{NRD_HIP_LIGHT_LOCAL, 0.0f, 4.0f, 0}, {NRD_HIP_LIGHT_LOCAL, 0.0f, 1.0f, 0}};
    NrdHipShadowLightsPackDesc pack = {};
    CHECK(!nrdi.PackShadowLights(pack));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "lightsNum"));
    pack.lightsNum = 2;
    pack.lights = lights;
    lights[1].lightSize = -1.0f;
    CHECK(!nrdi.PackShadowLights(pack));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "lights[1].lightSize"));
    lights[1].lightSize = 1.0f;
    lights[0].type = 2;
    CHECK(!nrdi.PackShadowLights(pack));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "lights[0].type"));
    lights[0].type = NRD_HIP_LIGHT_LOCAL;
    CHECK(!nrdi.PackShadowLights(pack));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "distanceToOccluder"));
    NrdHipShadowLightsResolveDesc resolve = {};
    resolve.mode = 5;
    CHECK(!nrdi.ResolveShadowLights(resolve));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "mode"));
    resolve.mode = NRD_HIP_SHADOWS_COMBINED;
    resolve.lightsNum = 2;
    CHECK(!nrdi.ResolveShadowLights(resolve));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "shadow"));
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // light 0: occluder at 2, light at 6, size 4 -> penumbra size 4 * 2 / 4 = 2, radius 1; light 1: a miss. L_0 = (1, 2, 3), L_1 = (0.5, 0.25, 4)
    std::vector<float> d(2 * px), dl(2 * px, 6.0f), L(2 * px * 4);
    for (size_t i = 0; i < px; i++) {
        d[i] = 2.0f;
        d[px + i] = 1e5f;
        const float l0[4] = {1.0f, 2.0f, 3.0f, 0.0f}, l1[4] = {0.5f, 0.25f, 4.0f, 0.0f};
        memcpy(&L[4 * i], l0, 16);
        memcpy(&L[4 * (px + i)], l1, 16);
    }
    float *dD, *dDl, *dL, *dSum, *dOut;
    uint16_t* dPen; // two per-light layers, then the combined plane
    uint32_t* dTr;
    uint8_t* dShadow;
    CHECK(hipMalloc(&dD, 2 * px * 4) == hipSuccess && hipMalloc(&dDl, 2 * px * 4) == hipSuccess && hipMalloc(&dL, 2 * px * 16) == hipSuccess && hipMalloc(&dSum, px * 16) == hipSuccess);
    CHECK(hipMalloc(&dOut, px * 16) == hipSuccess && hipMalloc(&dPen, 3 * px * 2) == hipSuccess && hipMalloc(&dTr, px * 4) == hipSuccess && hipMalloc(&dShadow, 4 * px) == hipSuccess);
    CHECK(hipMemcpy(dD, d.data(), 2 * px * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dDl, dl.data(), 2 * px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dL, L.data(), 2 * px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dPen, 0x5A, 3 * px * 2) == hipSuccess && hipMemset(dShadow, 0xFF, 4 * px) == hipSuccess);
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    pack.mode = NRD_HIP_SHADOWS_PER_LIGHT;
    pack.distanceToOccluder = plane(dD, 4, nrd::Format::R32_SFLOAT);
    pack.distanceToLight = plane(dDl, 4, nrd::Format::R32_SFLOAT);
    pack.distanceToOccluderLayerBytes = pack.distanceToLightLayerBytes = px * 4;
    pack.outPenumbra = plane(dPen, 2, nrd::Format::R16_SFLOAT);
    pack.outPenumbraLayerBytes = px * 2;
    if (!nrdi.PackShadowLights(pack)) {
        printf("PackShadowLights (PER_LIGHT) failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    pack.mode = NRD_HIP_SHADOWS_COMBINED;
    pack.lighting = plane(dL, 16, nrd::Format::RGBA32_SFLOAT);
    pack.lightingLayerBytes = px * 16;
    pack.outPenumbra = plane(dPen + 2 * px, 2, nrd::Format::R16_SFLOAT);
    pack.outTranslucency = plane(dTr, 4, nrd::Format::RGBA8_UNORM);
    pack.outLightingSum = plane(dSum, 16, nrd::Format::RGBA32_SFLOAT);
    if (!nrdi.PackShadowLights(pack)) {
        printf("PackShadowLights (COMBINED) failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    std::vector<uint16_t> pen(3 * px);
    std::vector<uint32_t> tr(px);
    std::vector<float> sum(px * 4), out(px * 4);
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(pen.data(), dPen, 3 * px * 2, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(tr.data(), dTr, px * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(sum.data(), dSum, px * 16, hipMemcpyDeviceToHost) == hipSuccess);
    // per light: 1.0 and 65504 as fp16. Combined: only light 0 is occluded, so the penumbra is its own ( 1 * w / w ); the translucency is LSsum / Lsum = L_1 / ( L_0 + L_1 ):
    // ( 0.5 / 1.5, 0.25 / 2.25, 4 / 7 ) -> floor( x * 255 + 0.5 ) = ( 85, 28, 146 ), .x = 0 (a light is occluded)
    size_t wrong = 0;
    for (size_t i = 0; i < px; i++) {
        wrong += pen[i] != 0x3C00 || pen[px + i] != 0x7BFF || pen[2 * px + i] != 0x3C00;
        wrong += tr[i] != (0u | 85u << 8 | 28u << 16 | 146u << 24);
        wrong += sum[4 * i] != 1.5f || sum[4 * i + 1] != 2.25f || sum[4 * i + 2] != 7.0f || sum[4 * i + 3] != 0.0f;
    }
    printf("packed penumbra, translucency and lighting sum: %zu wrong pixels\n", wrong);
    CHECK(wrong == 0);

    // resolves with fully lit shadows ( 255 -> 1 ): PER_LIGHT gives L_0 + L_1 with .w = 0, COMBINED gives Lsum with .w = the shadow
    resolve.mode = NRD_HIP_SHADOWS_PER_LIGHT;
    resolve.shadow = plane(dShadow, 1, nrd::Format::R8_UNORM);
    resolve.shadowLayerBytes = px;
    resolve.lighting = plane(dL, 16, nrd::Format::RGBA32_SFLOAT);
    resolve.lightingLayerBytes = px * 16;
    resolve.out = plane(dOut, 16, nrd::Format::RGBA32_SFLOAT);
    for (int combined = 0; combined < 2; combined++) {
        if (combined) {
            resolve.mode = NRD_HIP_SHADOWS_COMBINED;
            resolve.shadow = plane(dShadow, 4, nrd::Format::RGBA8_UNORM);
            resolve.lighting = plane(dSum, 16, nrd::Format::RGBA32_SFLOAT);
        }
        if (!nrdi.ResolveShadowLights(resolve)) {
            printf("ResolveShadowLights failed: %s\n", nrdi.GetLastFrontEndError());
            return 1;
        }
        CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(out.data(), dOut, px * 16, hipMemcpyDeviceToHost) == hipSuccess);
        wrong = 0;
        for (size_t i = 0; i < px; i++)
            wrong += out[4 * i] != 1.5f || out[4 * i + 1] != 2.25f || out[4 * i + 2] != 7.0f || out[4 * i + 3] != (combined ? 1.0f : 0.0f);
        printf("%s resolve: %zu wrong pixels\n", combined ? "COMBINED" : "PER_LIGHT", wrong);
        CHECK(wrong == 0);
    }
    hipFree(dD), hipFree(dDl), hipFree(dL), hipFree(dSum), hipFree(dOut), hipFree(dPen), hipFree(dTr), hipFree(dShadow);
    printf("shadow lights integration OK\n");
    return 0;
}
