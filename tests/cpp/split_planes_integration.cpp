// The split overloads of IntegrationHip (PackInputs( desc, options, samples, split ) -> nrdHipPackInputsSplit, ResolveOutputs( desc, options, split ) ->
// nrdHipResolveOutputsSplit) used the way an application would: include/NRD.h + include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against libNRD_hip.so.
//   host part: RGB32_SFLOAT without its companion is refused with a text that names the field; the old overload answers UNSUPPORTED to RGB32_SFLOAT (no device is touched)
//   GPU part:  a 70 x 6 frame, RELAX_RADIANCE on both signals: normal [ H, W, 3 ] + roughness [ H, W ] and radiance [ H, W, 3 ] + hit distance [ H, W ] packed in place
//              give the bytes PackInputs( desc ) writes for the RGBA32_SFLOAT planes of the same values; the packed planes resolved into RGB32_SFLOAT + hit-distance
//              planes equal .rgb and .w of the RGBA32_SFLOAT resolve, and the floats behind the last RGB32_SFLOAT texel keep their stamp
// usage: split_planes_integration [--no-gpu]
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
    nrd::IntegrationHip nrdi;
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };

    // ---- host part: host memory stands in for the planes, nothing is launched
    std::vector<float> nr3(px * 3), rough(px, 0.5f), z(px, 10.0f), rad3(px * 3), hit(px);
    std::vector<uint16_t> packedHost(px * 4);
    std::vector<uint32_t> wordHost(px);
    NrdHipFrontEndDesc desc = {};
    NrdHipFrontEndOptions options = {};
    NrdHipFrontEndSamples samples = {};
    NrdHipFrontEndSplit split = {};
    desc.normalRoughness = plane(nr3.data(), 12, nrd::Format::RGB32_SFLOAT);
    desc.viewZ = plane(z.data(), 4, nrd::Format::R32_SFLOAT);
    desc.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.specular.radianceHitDist = plane(rad3.data(), 12, nrd::Format::RGB32_SFLOAT);
    desc.specular.out0 = plane(packedHost.data(), 8, nrd::Format::RGBA16_SFLOAT);
    CHECK(!nrdi.PackInputs(desc, options, samples, split));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "split: roughness"));
    split.roughness = plane(rough.data(), 4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.PackInputs(desc, options, samples, split));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "split: specularHitDist"));
    CHECK(nrdHipPackInputsSamples(&desc, &options, &samples, nullptr) == (uint32_t)nrd::Result::UNSUPPORTED); // the old entry point
    NrdHipBackEndDesc back = {};
    NrdHipBackEndOptions backOptions = {};
    NrdHipBackEndSplit backSplit = {};
    back.specular.mode = NRD_HIP_SIGNAL_REBLUR_OCCLUSION;
    back.specular.in0 = plane(packedHost.data(), 2, nrd::Format::R16_UNORM);
    back.specular.out = plane(hit.data(), 4, nrd::Format::R32_SFLOAT);
    backSplit.specularHitDist = plane(z.data(), 4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.ResolveOutputs(back, backOptions, backSplit));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "split: specularHitDist"));
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // ---- GPU part
    std::vector<float> nr4(px * 4), rad4(px * 4);
    for (size_t i = 0; i < px; i++) {
        nr3[3 * i + 2] = 1.0f;
        rough[i] = 0.125f * float(1 + i % 7);
        hit[i] = 1.0f + float(i % 13);
        for (int c = 0; c < 3; c++) {
            rad3[3 * i + c] = 0.25f * float((i * 7 + c * 3) % 19);
            nr4[4 * i + c] = nr3[3 * i + c];
            rad4[4 * i + c] = rad3[3 * i + c];
        }
        nr4[4 * i + 3] = rough[i];
        rad4[4 * i + 3] = hit[i];
    }
    // one arena of floats: [ nr3 | rough | z | rad3 | hit | nr4 | rad4 | resolved rgb (diffuse, specular) + 4 stamped floats each | hit distances | resolved rgba x 2 ]
    const size_t oNr3 = 0, oRough = oNr3 + px * 3, oZ = oRough + px, oRad3 = oZ + px, oHit = oRad3 + px * 3, oNr4 = oHit + px, oRad4 = oNr4 + px * 4, oRgbD = oRad4 + px * 4,
                 oRgbS = oRgbD + px * 3 + 4, oHdD = oRgbS + px * 3 + 4, oHdS = oHdD + px, oRgbaD = oHdS + px, oRgbaS = oRgbaD + px * 4, floats = oRgbaS + px * 4;
    float* dF;
    uint16_t* dPacked; // four RGBA16_SFLOAT planes: diffuse / specular of the RGBA32 call, diffuse / specular of the split call
    uint32_t* dWord;   // IN_NORMAL_ROUGHNESS of the two calls
    float* dZOut;
    CHECK(hipMalloc(&dF, floats * 4) == hipSuccess && hipMalloc(&dPacked, 4 * px * 8) == hipSuccess && hipMalloc(&dWord, 2 * px * 8) == hipSuccess && hipMalloc(&dZOut, px * 4) == hipSuccess);
    CHECK(hipMemset(dF, 0x5A, floats * 4) == hipSuccess && hipMemset(dPacked, 0x5A, 4 * px * 8) == hipSuccess && hipMemset(dWord, 0x5A, 2 * px * 8) == hipSuccess);
    auto up = [&](size_t off, const std::vector<float>& v) { return hipMemcpy(dF + off, v.data(), v.size() * 4, hipMemcpyHostToDevice) == hipSuccess; };
    CHECK(up(oNr3, nr3) && up(oRough, rough) && up(oZ, z) && up(oRad3, rad3) && up(oHit, hit) && up(oNr4, nr4) && up(oRad4, rad4));
    const nrd::NormalEncoding enc = nrd::GetLibraryDesc().normalEncoding;
    const nrd::Format nrFormat = enc == nrd::NormalEncoding::RGBA8_UNORM ? nrd::Format::RGBA8_UNORM : enc == nrd::NormalEncoding::RGBA8_SNORM ? nrd::Format::RGBA8_SNORM
        : enc == nrd::NormalEncoding::R10_G10_B10_A2_UNORM ? nrd::Format::R10_G10_B10_A2_UNORM : enc == nrd::NormalEncoding::RGBA16_UNORM ? nrd::Format::RGBA16_UNORM : nrd::Format::RGBA16_SNORM;
    const uint32_t nrBytes = nrFormat == nrd::Format::RGBA16_UNORM || nrFormat == nrd::Format::RGBA16_SNORM ? 8 : 4;
    desc = {};
    desc.normalRoughness = plane(dF + oNr4, 16, nrd::Format::RGBA32_SFLOAT);
    desc.viewZ = plane(dF + oZ, 4, nrd::Format::R32_SFLOAT);
    desc.outNormalRoughness = plane(dWord, nrBytes, nrFormat);
    desc.outViewZ = plane(dZOut, 4, nrd::Format::R32_SFLOAT);
    desc.diffuse.mode = desc.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.diffuse.radianceHitDist = desc.specular.radianceHitDist = plane(dF + oRad4, 16, nrd::Format::RGBA32_SFLOAT);
    desc.diffuse.out0 = plane(dPacked, 8, nrd::Format::RGBA16_SFLOAT);
    desc.specular.out0 = plane(dPacked + px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    if (!nrdi.PackInputs(desc)) {
        printf("PackInputs failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    desc.normalRoughness = plane(dF + oNr3, 12, nrd::Format::RGB32_SFLOAT);
    desc.diffuse.radianceHitDist = desc.specular.radianceHitDist = plane(dF + oRad3, 12, nrd::Format::RGB32_SFLOAT);
    desc.outNormalRoughness = plane((uint8_t*)dWord + px * nrBytes, nrBytes, nrFormat);
    desc.diffuse.out0 = plane(dPacked + 2 * px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    desc.specular.out0 = plane(dPacked + 3 * px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    split = {};
    split.roughness = plane(dF + oRough, 4, nrd::Format::R32_SFLOAT);
    split.diffuseHitDist = split.specularHitDist = plane(dF + oHit, 4, nrd::Format::R32_SFLOAT);
    if (!nrdi.PackInputs(desc, options, samples, split)) {
        printf("PackInputs with split planes failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    std::vector<uint16_t> packed(4 * px * 4);
    std::vector<uint8_t> word(2 * px * nrBytes);
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(packed.data(), dPacked, packed.size() * 2, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(word.data(), dWord, word.size(), hipMemcpyDeviceToHost) == hipSuccess);
    size_t mismatches = 0;
    for (size_t i = 0; i < 2 * px * 4; i++)
        mismatches += packed[i] != packed[2 * px * 4 + i];
    for (size_t i = 0; i < px * nrBytes; i++)
        mismatches += word[i] != word[px * nrBytes + i];
    printf("split pack vs RGBA32 pack: %zu mismatching values\n", mismatches);
    CHECK(mismatches == 0);

    // resolve the packed planes: RGBA32_SFLOAT outputs, then RGB32_SFLOAT + hit-distance planes
    back = {};
    back.diffuse.mode = back.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    back.diffuse.in0 = plane(dPacked, 8, nrd::Format::RGBA16_SFLOAT);
    back.specular.in0 = plane(dPacked + px * 4, 8, nrd::Format::RGBA16_SFLOAT);
    back.diffuse.out = plane(dF + oRgbaD, 16, nrd::Format::RGBA32_SFLOAT);
    back.specular.out = plane(dF + oRgbaS, 16, nrd::Format::RGBA32_SFLOAT);
    CHECK(nrdi.ResolveOutputs(back));
    back.diffuse.out = plane(dF + oRgbD, 12, nrd::Format::RGB32_SFLOAT);
    back.specular.out = plane(dF + oRgbS, 12, nrd::Format::RGB32_SFLOAT);
    backSplit = {};
    backSplit.diffuseHitDist = plane(dF + oHdD, 4, nrd::Format::R32_SFLOAT);
    backSplit.specularHitDist = plane(dF + oHdS, 4, nrd::Format::R32_SFLOAT);
    if (!nrdi.ResolveOutputs(back, backOptions, backSplit)) {
        printf("ResolveOutputs with split planes failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    std::vector<uint32_t> f(floats);
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(f.data(), dF, floats * 4, hipMemcpyDeviceToHost) == hipSuccess);
    size_t wrong = 0;
    for (size_t i = 0; i < px; i++) {
        for (int c = 0; c < 3; c++) {
            wrong += f[oRgbD + 3 * i + c] != f[oRgbaD + 4 * i + c];
            wrong += f[oRgbS + 3 * i + c] != f[oRgbaS + 4 * i + c];
        }
        wrong += f[oHdD + i] != f[oRgbaD + 4 * i + 3];
        wrong += f[oHdS + i] != f[oRgbaS + 4 * i + 3];
    }
    for (int k = 0; k < 4; k++) // the floats behind the last 12-byte texel: a 16-byte store would have reached the first of them
        wrong += (f[oRgbD + px * 3 + k] != 0x5A5A5A5Au) + (f[oRgbS + px * 3 + k] != 0x5A5A5A5Au);
    printf("split resolve vs RGBA32 resolve: %zu wrong values\n", wrong);
    CHECK(wrong == 0);
    hipFree(dF), hipFree(dPacked), hipFree(dWord), hipFree(dZOut);
    printf("split planes integration OK\n");
    return 0;
}
