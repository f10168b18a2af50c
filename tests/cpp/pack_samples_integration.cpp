// The third IntegrationHip::PackInputs overload (desc, options, samples -> nrdHipPackInputsSamples) used the way an application would: include/NRD.h +
// include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against libNRD_hip.so.
//   host part: the overload forwards to the library -- an invalid sample count is refused with a text that names the field, nothing is enqueued (no device is touched)
//   GPU part:  a 70 x 6 frame, RELAX_RADIANCE on both signals, two EQUAL sample layers per signal: ( P + P ) / 2 is exact, so every byte of the two packed planes
//              must be the byte PackInputs( desc ) writes for one layer; then two different layers, diffuse .w = the mean, specular .w = the smaller non-zero one
// usage: pack_samples_integration [--no-gpu]
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
    nrd::IntegrationHip nrdi; // PackInputs needs no instance: it runs on the integration's stream (the default one here)

    NrdHipFrontEndDesc desc = {};
    NrdHipFrontEndOptions options = {};
    NrdHipFrontEndSamples samples = {};
    samples.diffuse.samplesNum = 65;
    CHECK(!nrdi.PackInputs(desc, options, samples));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "diffuse.samplesNum"));
    samples.diffuse.samplesNum = 0;
    samples.hitDistTrimThreshold = -1.0f;
    CHECK(!nrdi.PackInputs(desc, options, samples));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "hitDistTrimThreshold"));
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // two layers of ( radiance.rgb, hit distance ) per signal, layer 1 first equal to layer 0
    std::vector<float> nr(px * 4), z(px, 10.0f), rad(2 * px * 4);
    for (size_t i = 0; i < px; i++) {
        nr[4 * i + 2] = 1.0f;
        nr[4 * i + 3] = 0.5f;
        for (int c = 0; c < 3; c++)
            rad[4 * i + c] = 0.25f * float((i * 7 + c * 3) % 19);
        rad[4 * i + 3] = 1.0f + float(i % 13);
    }
    memcpy(&rad[px * 4], &rad[0], px * 16);
    float *dNr, *dZ, *dRad;
    uint16_t* dOut; // four RGBA16_SFLOAT planes: diffuse / specular of the plain call, diffuse / specular of the call with samples
    CHECK(hipMalloc(&dNr, px * 16) == hipSuccess && hipMalloc(&dZ, px * 4) == hipSuccess && hipMalloc(&dRad, 2 * px * 16) == hipSuccess && hipMalloc(&dOut, 4 * px * 8) == hipSuccess);
    CHECK(hipMemcpy(dNr, nr.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dZ, z.data(), px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dRad, rad.data(), 2 * px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dOut, 0x5A, 4 * px * 8) == hipSuccess);
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    desc.normalRoughness = plane(dNr, 16, nrd::Format::RGBA32_SFLOAT);
    desc.viewZ = plane(dZ, 4, nrd::Format::R32_SFLOAT);
    desc.diffuse.mode = desc.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.diffuse.radianceHitDist = desc.specular.radianceHitDist = plane(dRad, 16, nrd::Format::RGBA32_SFLOAT);
    desc.diffuse.out0 = plane(dOut, 8, nrd::Format::RGBA16_SFLOAT);
    desc.specular.out0 = plane(dOut + px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    if (!nrdi.PackInputs(desc)) {
        printf("PackInputs failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    desc.diffuse.out0 = plane(dOut + 2 * px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    desc.specular.out0 = plane(dOut + 3 * px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    samples = {};
    samples.diffuse.samplesNum = samples.specular.samplesNum = 2;
    samples.diffuse.radianceHitDistLayerBytes = samples.specular.radianceHitDistLayerBytes = px * 16;
    if (!nrdi.PackInputs(desc, options, samples)) {
        printf("PackInputs with samples failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    std::vector<uint16_t> out(4 * px * 4);
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(out.data(), dOut, out.size() * 2, hipMemcpyDeviceToHost) == hipSuccess);
    size_t mismatches = 0;
    for (size_t i = 0; i < 2 * px * 4; i++)
        mismatches += out[i] != out[2 * px * 4 + i];
    printf("two equal layers vs one: %zu mismatching values\n", mismatches);
    CHECK(mismatches == 0);

    // layer 1: the hit distance of layer 0 plus 2 (exact in fp16 for these small integers): diffuse .w = h + 1, specular .w = h
    for (size_t i = 0; i < px; i++)
        rad[px * 4 + 4 * i + 3] = rad[4 * i + 3] + 2.0f;
    CHECK(hipMemcpy(dRad, rad.data(), 2 * px * 16, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(nrdi.PackInputs(desc, options, samples));
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(out.data(), dOut, out.size() * 2, hipMemcpyDeviceToHost) == hipSuccess);
    auto half = [](float v) { // small non-negative integers only
        uint32_t u;
        memcpy(&u, &v, 4);
        return (uint16_t)(((u >> 23) - 112u) << 10 | ((u >> 13) & 0x3FFu));
    };
    size_t wrong = 0;
    for (size_t i = 0; i < px; i++) {
        wrong += out[(2 * px + i) * 4 + 3] != half(rad[4 * i + 3] + 1.0f);
        wrong += out[(3 * px + i) * 4 + 3] != half(rad[4 * i + 3]);
    }
    printf("mean (diffuse) and smallest non-zero (specular) hit distance: %zu wrong values\n", wrong);
    CHECK(wrong == 0);
    hipFree(dNr), hipFree(dZ), hipFree(dRad), hipFree(dOut);
    printf("pack samples integration OK\n");
    return 0;
}
