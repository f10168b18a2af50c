// nrdHipPackInputsDirect used the way an application would: include/NRD.h + include/NRDHip.h + include/NRDIntegrationHip.hpp (+ include/NRD.hip.h for the mixing function),
// linked against libNRD_hip.so.
//   --mix IN OUT: NRD_HIP_MixDiffuseHitDist evaluated on the HOST over the rows ( h_i, h_d, L_i, L_d, maxContribution ) of the float32 file IN; one float32 per row goes to OUT
//                 (tests/test_pack_direct_cpp.py holds them against tests/direct_model.py bit for bit)
//   host part:    the struct sizes; invalid descriptors are refused with a text that names the field, nothing is enqueued (no device is touched)
//   GPU part:     a 67 x 23 frame, RELAX_RADIANCE on both signals, the indirect planes ( 1, 1, 1, 2 ), the direct ones ( 1, 1, 1, 4 ), maxHitDistContribution 0.5:
//                 IntegrationHip::PackInputsDirect writes the bytes nrdHipPackInputsDirect writes -- radiance 2, the specular hit distance 2, the diffuse one
//                 2 + ( 4 - 2 ) * ( 1 / ( 2 + 1e-6 ) ), which is 3 in fp16
// usage: pack_direct_integration [--no-gpu | --mix IN OUT]
#include "NRD.h"
#include "NRDHip.h"
#include "NRDIntegrationHip.hpp"

#include "NRD.hip.h"

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

static int Mix(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    CHECK(f);
    std::vector<float> rows;
    float row[5];
    while (fread(row, sizeof(float), 5, f) == 5)
        rows.insert(rows.end(), row, row + 5);
    fclose(f);
    std::vector<float> result(rows.size() / 5);
    for (size_t i = 0; i < result.size(); i++)
        result[i] = NRD_HIP_MixDiffuseHitDist(rows[5 * i], rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4]);
    f = fopen(out, "wb");
    CHECK(f && fwrite(result.data(), sizeof(float), result.size(), f) == result.size());
    fclose(f);
    printf("mixed %zu rows\n", result.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--mix"))
        return Mix(argv[2], argv[3]);
    const bool noGpu = argc > 1 && !strcmp(argv[1], "--no-gpu");
    const uint16_t W = 67, H = 23;
    const size_t px = (size_t)W * H;
    static_assert(sizeof(NrdHipDirectSignal) == 104 && sizeof(NrdHipFrontEndDirect) == 216, "the structs of the call");
    static_assert(NRD_HIP_DIRECT_MAX_CONTRIBUTION_DEFAULT == 0.5f, "the README's default");
    nrd::IntegrationHip nrdi; // the call needs no instance: it runs on the integration's stream (the default one here)

    // ---- host part: every plane points at host memory, which no call below may touch
    std::vector<float> host(px * 4);
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    NrdHipFrontEndDesc desc = {};
    desc.normalRoughness = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    desc.viewZ = plane(host.data(), 4, nrd::Format::R32_SFLOAT);
    desc.diffuse.mode = desc.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.diffuse.radianceHitDist = desc.specular.radianceHitDist = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    desc.diffuse.out0 = desc.specular.out0 = plane(host.data(), 8, nrd::Format::RGBA16_SFLOAT);
    NrdHipFrontEndDirect direct = {};
    direct.maxHitDistContribution = NRD_HIP_DIRECT_MAX_CONTRIBUTION_DEFAULT;
    direct.diffuse.radianceHitDist = direct.specular.radianceHitDist = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    direct.maxHitDistContribution = 1.5f;
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "nrdHipPackInputsDirect") && strstr(nrdi.GetLastFrontEndError(), "maxHitDistContribution"));
    direct.maxHitDistContribution = 0.5f;
    direct.specular.hitDist = plane(host.data(), 4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "direct: specular.hitDist"));
    direct.specular.hitDist = NrdHipPlaneDesc{};
    direct.diffuse.direction = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "direct: diffuse.direction"));
    direct.diffuse.direction = NrdHipPlaneDesc{};
    direct.diffuse.samplesNum = 3;
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "direct: diffuse.samplesNum"));
    direct.diffuse.samplesNum = 0;
    direct.reserved = 1;
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "reserved"));
    direct.reserved = 0;
    desc.diffuse.mode = NRD_HIP_SIGNAL_REBLUR_OCCLUSION;
    desc.diffuse.out0.format = (uint32_t)nrd::Format::R16_UNORM;
    desc.diffuse.out0.rowPitchBytes = (uint32_t)W * 2;
    CHECK(!nrdi.PackInputsDirect(desc, direct));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "direct: diffuse.radianceHitDist"));
    desc.diffuse.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.diffuse.out0 = desc.specular.out0;
    CHECK(!nrdi.PackInputsDirect(desc, direct, nullptr, nullptr, nullptr, 2));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "guideShift"));
    for (float v : host)
        CHECK(v == 0.0f);
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // ---- GPU part
    std::vector<float> nr(px * 4), z(px, 10.0f), indirect(px * 4), lit(px * 4);
    for (size_t i = 0; i < px; i++) {
        nr[4 * i + 2] = 1.0f;
        nr[4 * i + 3] = 0.5f;
        indirect[4 * i] = indirect[4 * i + 1] = indirect[4 * i + 2] = lit[4 * i] = lit[4 * i + 1] = lit[4 * i + 2] = 1.0f;
        indirect[4 * i + 3] = 2.0f;
        lit[4 * i + 3] = 4.0f;
    }
    float *dNr, *dZ, *dIndirect, *dLit;
    uint16_t* dOut; // four RGBA16_SFLOAT planes: two per call
    CHECK(hipMalloc(&dNr, px * 16) == hipSuccess && hipMalloc(&dZ, px * 4) == hipSuccess && hipMalloc(&dIndirect, px * 16) == hipSuccess && hipMalloc(&dLit, px * 16) == hipSuccess);
    CHECK(hipMalloc(&dOut, 4 * px * 8) == hipSuccess && hipMemset(dOut, 0x5A, 4 * px * 8) == hipSuccess);
    CHECK(hipMemcpy(dNr, nr.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dZ, z.data(), px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dIndirect, indirect.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dLit, lit.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess);
    desc.normalRoughness.data = dNr;
    desc.viewZ.data = dZ;
    desc.diffuse.radianceHitDist.data = desc.specular.radianceHitDist.data = dIndirect;
    direct.diffuse.radianceHitDist.data = direct.specular.radianceHitDist.data = dLit;
    desc.diffuse.out0.data = dOut;
    desc.specular.out0.data = dOut + px * 4;
    CHECK(nrdi.PackInputsDirect(desc, direct));
    desc.diffuse.out0.data = dOut + 2 * px * 4;
    desc.specular.out0.data = dOut + 3 * px * 4;
    CHECK(nrdHipPackInputsDirect(&desc, nullptr, nullptr, nullptr, &direct, 0, nullptr) == (uint32_t)nrd::Result::SUCCESS);
    CHECK(hipDeviceSynchronize() == hipSuccess);
    std::vector<uint16_t> out(4 * px * 4);
    CHECK(hipMemcpy(out.data(), dOut, 4 * px * 8, hipMemcpyDeviceToHost) == hipSuccess);
    size_t mismatches = 0, differing = 0;
    for (size_t i = 0; i < px; i++)
        for (int signal = 0; signal < 2; signal++)
            for (int c = 0; c < 4; c++) { // fp16 2.0 = 0x4000, 3.0 = 0x4200
                const uint16_t want = c < 3 ? 0x4000 : signal == 0 ? 0x4200 : 0x4000;
                mismatches += out[(signal * px + i) * 4 + c] != want;
                differing += out[(signal * px + i) * 4 + c] != out[((signal + 2) * px + i) * 4 + c];
            }
    printf("packed texels: %zu mismatching values, %zu differing from the C-ABI call's\n", mismatches, differing);
    CHECK(mismatches == 0 && differing == 0);
    for (void* p : {(void*)dNr, (void*)dZ, (void*)dIndirect, (void*)dLit, (void*)dOut})
        (void)hipFree(p);
    printf("pack direct integration OK\n");
    return 0;
}
