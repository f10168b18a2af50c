// SIGMA for many lights through the C++ integration layer: an IntegrationHip with layersNum = 2 denoises two shadow layers (one per light) in one pass chain; layer 1 must
// hold byte for byte what an unlayered IntegrationHip holds that ran the same frame on layer 1's planes (include/NRDHip.h "layered executor"). 64 x 32, one frame.
// usage: sigma_layers_integration [--no-gpu]   (--no-gpu: stop after the host-only part: the user pool with its layer strides)
#include "NRD.h"
#include "NRDHip.h"
#include "NRDIntegrationHip.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAILED: %s (line %d)\n", #x, __LINE__);       \
            return 1;                                             \
        }                                                         \
    } while (0)

static uint16_t Half(float f) { // fp32 -> fp16 of the few values used here (normal range, no rounding needed beyond truncation of zero bits)
    uint32_t u;
    memcpy(&u, &f, 4);
    if (f == 0.0f)
        return 0;
    const uint32_t e = ((u >> 23) & 0xFFu) - 127u + 15u;
    return (uint16_t)(((u >> 16) & 0x8000u) | (e << 10) | ((u >> 13) & 0x3FFu));
}

int main(int argc, char** argv) {
    const bool noGpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
    const uint16_t W = 64, H = 32;
    const uint32_t layers = 2;
    const size_t texels = (size_t)W * H;

    // ---- host only: the pool entry of a stack carries its layer stride, a plain entry none
    nrd::UserPoolHip probe = {};
    CHECK(probe.size() == (size_t)nrd::ResourceType::MAX_NUM - 2 && probe.layerBytes[(size_t)nrd::ResourceType::IN_PENUMBRA] == 0);
    nrd::IntegrationHip_SetResourceLayers(probe, nrd::ResourceType::IN_PENUMBRA, NrdHipPlaneDesc{&probe, (uint32_t)W * 2, (uint32_t)nrd::Format::R16_SFLOAT, W, H}, texels * 2);
    CHECK(probe.layerBytes[(size_t)nrd::ResourceType::IN_PENUMBRA] == texels * 2 && probe[(size_t)nrd::ResourceType::IN_PENUMBRA].data == &probe);
    nrd::IntegrationHip_SetResource(probe, nrd::ResourceType::IN_PENUMBRA, NrdHipPlaneDesc{&probe, (uint32_t)W * 2, (uint32_t)nrd::Format::R16_SFLOAT, W, H});
    CHECK(probe.layerBytes[(size_t)nrd::ResourceType::IN_PENUMBRA] == 0);
    CHECK(nrd::IntegrationHipCreationDesc().layersNum == 1);
    if (noGpu) {
        printf("host-only OK\n");
        return 0;
    }

    // ---- the frame: a tilted floor seen by a perspective camera, two lights with different penumbrae
    std::vector<float> viewZ(texels);
    std::vector<uint32_t> normalRoughness(texels);
    std::vector<uint16_t> mv(texels * 4, 0), penumbra(texels * layers);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            viewZ[i] = 4.0f + 0.05f * float(x) + 0.1f * float(y);
            normalRoughness[i] = 511u | (511u << 10) | (0u << 20) | (1u << 30); // R10_G10_B10_A2_UNORM: normal (0, 0, -1)
            // light 0: a soft shadow edge that runs down the frame; light 1: lit on the left, hard shadow in a block, a penumbra elsewhere
            const float p0 = x < 20 ? 65504.0f : (x < 44 ? 0.25f + 0.125f * float((x + y) & 7) : 0.0f);
            const float p1 = x < 8 ? 65504.0f : ((x >= 40 && y >= 8 && y < 24) ? 0.0f : 0.5f + 0.0625f * float((3 * x + 5 * y) & 15));
            penumbra[i] = p0 == 65504.0f ? 0x7BFFu : Half(p0);
            penumbra[texels + i] = p1 == 65504.0f ? 0x7BFFu : Half(p1);
        }

    void *dViewZ = nullptr, *dNormal = nullptr, *dMv = nullptr, *dPenumbra = nullptr, *dOut = nullptr, *dOutSingle = nullptr;
    CHECK(hipMalloc(&dViewZ, texels * 4) == hipSuccess && hipMalloc(&dNormal, texels * 4) == hipSuccess && hipMalloc(&dMv, texels * 8) == hipSuccess);
    CHECK(hipMalloc(&dPenumbra, texels * 2 * layers) == hipSuccess && hipMalloc(&dOut, texels * layers) == hipSuccess && hipMalloc(&dOutSingle, texels) == hipSuccess);
    CHECK(hipMemcpy(dViewZ, viewZ.data(), texels * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dNormal, normalRoughness.data(), texels * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dMv, mv.data(), texels * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dPenumbra, penumbra.data(), texels * 2 * layers, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemset(dOut, 0, texels * layers) == hipSuccess && hipMemset(dOutSingle, 0, texels) == hipSuccess);

    nrd::CommonSettings cs = {};
    const float zn = 0.1f, zf = 1000.0f, sx = 0.5f, sy = 1.0f; // 90 degrees vertically, aspect 2; column-major, vectors are columns
    const float proj[16] = {sx, 0, 0, 0, 0, sy, 0, 0, 0, 0, zf / (zf - zn), 1.0f, 0, 0, -zn * zf / (zf - zn), 0};
    memcpy(cs.viewToClipMatrix, proj, sizeof(proj));
    memcpy(cs.viewToClipMatrixPrev, proj, sizeof(proj));
    cs.resourceSize[0] = cs.resourceSizePrev[0] = cs.rectSize[0] = cs.rectSizePrev[0] = W;
    cs.resourceSize[1] = cs.resourceSizePrev[1] = cs.rectSize[1] = cs.rectSizePrev[1] = H;
    cs.motionVectorScale[0] = cs.motionVectorScale[1] = cs.motionVectorScale[2] = 0.0f;
    cs.isMotionVectorInWorldSpace = true;
    nrd::SigmaSettings ss = {};

    nrd::DenoiserDesc denoisers[] = {{0, nrd::Denoiser::SIGMA_SHADOW}};
    nrd::InstanceCreationDesc icd = {};
    icd.denoisers = denoisers;
    icd.denoisersNum = 1;
    const nrd::Identifier id = 0;
    auto guides = [&](nrd::UserPoolHip& pool) {
        nrd::IntegrationHip_SetResource(pool, nrd::ResourceType::IN_VIEWZ, NrdHipPlaneDesc{dViewZ, (uint32_t)W * 4, (uint32_t)nrd::Format::R32_SFLOAT, W, H});
        nrd::IntegrationHip_SetResource(pool, nrd::ResourceType::IN_NORMAL_ROUGHNESS, NrdHipPlaneDesc{dNormal, (uint32_t)W * 4, (uint32_t)nrd::Format::R10_G10_B10_A2_UNORM, W, H});
        nrd::IntegrationHip_SetResource(pool, nrd::ResourceType::IN_MV, NrdHipPlaneDesc{dMv, (uint32_t)W * 8, (uint32_t)nrd::Format::RGBA16_SFLOAT, W, H});
    };

    // ---- both layers through one layered integration
    nrd::IntegrationHipCreationDesc desc = {};
    desc.name = "layered";
    desc.resourceWidth = W;
    desc.resourceHeight = H;
    desc.layersNum = layers;
    nrd::IntegrationHip layered;
    CHECK(layered.Initialize(desc, icd));
    uint32_t reported = 0;
    CHECK(nrdHipGetLayersNum(layered.GetExecutor(), &reported) == (uint32_t)nrd::Result::SUCCESS && reported == layers);
    nrd::UserPoolHip pool = {};
    guides(pool);
    nrd::IntegrationHip_SetResourceLayers(pool, nrd::ResourceType::IN_PENUMBRA, NrdHipPlaneDesc{dPenumbra, (uint32_t)W * 2, (uint32_t)nrd::Format::R16_SFLOAT, W, H}, texels * 2);
    nrd::IntegrationHip_SetResourceLayers(pool, nrd::ResourceType::OUT_SHADOW_TRANSLUCENCY, NrdHipPlaneDesc{dOut, (uint32_t)W, (uint32_t)nrd::Format::R8_UNORM, W, H}, texels);
    layered.NewFrame();
    CHECK(layered.SetCommonSettings(cs) && layered.SetDenoiserSettings(id, &ss));
    if (!layered.Denoise(&id, 1, pool)) {
        printf("layered Denoise failed: %s\n", layered.GetLastError());
        return 1;
    }
    CHECK(hipDeviceSynchronize() == hipSuccess);

    // ---- layer 1 alone through an unlayered one
    desc.name = "single";
    desc.layersNum = 1;
    nrd::IntegrationHip single;
    CHECK(single.Initialize(desc, icd));
    nrd::UserPoolHip poolSingle = {};
    guides(poolSingle);
    nrd::IntegrationHip_SetResource(poolSingle, nrd::ResourceType::IN_PENUMBRA, NrdHipPlaneDesc{(uint8_t*)dPenumbra + texels * 2, (uint32_t)W * 2, (uint32_t)nrd::Format::R16_SFLOAT, W, H});
    nrd::IntegrationHip_SetResource(poolSingle, nrd::ResourceType::OUT_SHADOW_TRANSLUCENCY, NrdHipPlaneDesc{dOutSingle, (uint32_t)W, (uint32_t)nrd::Format::R8_UNORM, W, H});
    single.NewFrame();
    CHECK(single.SetCommonSettings(cs) && single.SetDenoiserSettings(id, &ss));
    if (!single.Denoise(&id, 1, poolSingle)) {
        printf("single Denoise failed: %s\n", single.GetLastError());
        return 1;
    }
    CHECK(hipDeviceSynchronize() == hipSuccess);

    std::vector<uint8_t> out(texels * layers), outSingle(texels);
    CHECK(hipMemcpy(out.data(), dOut, out.size(), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(outSingle.data(), dOutSingle, outSingle.size(), hipMemcpyDeviceToHost) == hipSuccess);
    size_t mismatches = 0, distinct = 0, differing = 0;
    bool seen[256] = {};
    for (size_t i = 0; i < texels; i++) {
        mismatches += out[texels + i] != outSingle[i];
        differing += out[texels + i] != out[i];
        if (!seen[out[texels + i]])
            seen[out[texels + i]] = true, distinct++;
    }
    printf("SIGMA_SHADOW %ux%u, %u layers: layer 1 has %zu mismatching bytes, %zu distinct values, differs from layer 0 in %zu texels\n", W, H, layers, mismatches, distinct, differing);

    layered.Destroy();
    single.Destroy();
    for (void* p : {dViewZ, dNormal, dMv, dPenumbra, dOut, dOutSingle})
        (void)hipFree(p);
    if (mismatches || distinct < 3 || !differing)
        return 1;
    printf("sigma layers integration OK\n");
    return 0;
}
