// nrdHipPackInputsLobes / nrdHipCheckHitDistCoverage used the way an application would: include/NRD.h + include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against
// libNRD_hip.so.
//   host part: invalid descriptors are refused with a text that names the field, nothing is enqueued (no device is touched)
//   GPU part:  a 67 x 21 frame, RELAX_RADIANCE on both signals, one traced plane holding ( 1, 1, 1, 2 ) everywhere, the lobes a checkerboard with one 3x3 all-specular block,
//              the probability 0.5: a counted sample packs to ( 2, 2, 2, 2 ) -- rad / q, h -- the other signal's texel to zeros; then the audit of the two packed planes finds
//              the one diffuse hole of the block's centre for 3x3 and none for 5x5
// usage: pack_lobes_integration [--no-gpu]
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
    const uint16_t W = 67, H = 21;
    const size_t px = (size_t)W * H;
    static_assert(sizeof(NrdHipFrontEndLobes) == 168 && sizeof(NrdHipCoverageDesc) == 88 && sizeof(NrdHipCoverageReport) == 28, "the structs of the two calls");
    nrd::IntegrationHip nrdi; // the calls need no instance: they run on the integration's stream (the default one here)

    // ---- host part: every plane points at host memory, which no call below may touch
    std::vector<float> host(px * 4);
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    NrdHipFrontEndDesc desc = {};
    desc.normalRoughness = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    desc.viewZ = plane(host.data(), 4, nrd::Format::R32_SFLOAT);
    desc.diffuse.mode = desc.specular.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    desc.diffuse.out0 = desc.specular.out0 = plane(host.data(), 8, nrd::Format::RGBA16_SFLOAT);
    NrdHipFrontEndLobes lobes = {};
    lobes.radianceHitDist = plane(host.data(), 16, nrd::Format::RGBA32_SFLOAT);
    CHECK(!nrdi.PackInputsLobes(desc, lobes));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "nrdHipPackInputsLobes") && strstr(nrdi.GetLastFrontEndError(), "lobes: lobe"));
    lobes.lobe = plane(host.data(), 1, nrd::Format::R8_UINT);
    lobes.samplesNum = 65;
    CHECK(!nrdi.PackInputsLobes(desc, lobes));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "samplesNum"));
    lobes.samplesNum = 1;
    desc.specular.radianceHitDist = lobes.radianceHitDist;
    CHECK(!nrdi.PackInputsLobes(desc, lobes));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "specular.radianceHitDist"));
    desc.specular.radianceHitDist = NrdHipPlaneDesc{};
    desc.diffuse.mode = NRD_HIP_SIGNAL_NONE;
    CHECK(!nrdi.PackInputsLobes(desc, lobes));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "diffuse.mode"));
    desc.diffuse.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    NrdHipFrontEndOptions checkerboard = {1, 0};
    CHECK(!nrdi.PackInputsLobes(desc, lobes, &checkerboard));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "checkerboardMode"));
    NrdHipCoverageDesc coverage = {};
    coverage.area = 1;
    coverage.diffuse.plane = plane(host.data(), 8, nrd::Format::RGBA16_SFLOAT);
    CHECK(!nrdi.CheckHitDistCoverage(coverage, host.data()));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "nrdHipCheckHitDistCoverage") && strstr(nrdi.GetLastFrontEndError(), "viewZ"));
    coverage.viewZ = plane(host.data(), 4, nrd::Format::R32_SFLOAT);
    coverage.area = 3;
    CHECK(!nrdi.CheckHitDistCoverage(coverage, host.data()));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "area"));
    coverage.area = 1;
    CHECK(!nrdi.CheckHitDistCoverage(coverage, nullptr));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "deviceReport"));
    coverage.diffuse.plane.format = (uint32_t)nrd::Format::RGBA32_SFLOAT;
    CHECK(!nrdi.CheckHitDistCoverage(coverage, host.data()));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "diffuse.plane"));
    for (float v : host)
        CHECK(v == 0.0f);
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // ---- GPU part
    std::vector<float> nr(px * 4), z(px, 10.0f), traced(px * 4), prob(px, 0.5f);
    std::vector<uint8_t> lobe(px);
    const int bx = 10, by = 12; // the centre of the all-specular block
    size_t specularNum = 0;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            nr[4 * i + 2] = 1.0f;
            nr[4 * i + 3] = 0.5f;
            traced[4 * i] = traced[4 * i + 1] = traced[4 * i + 2] = 1.0f;
            traced[4 * i + 3] = 2.0f;
            const bool inBlock = x >= bx - 1 && x <= bx + 1 && y >= by - 1 && y <= by + 1;
            lobe[i] = inBlock || ((x ^ y) & 1) ? NRD_HIP_LOBE_SPECULAR : NRD_HIP_LOBE_DIFFUSE;
            specularNum += lobe[i];
        }
    float *dNr, *dZ, *dTraced, *dProb;
    uint8_t* dLobe;
    uint16_t* dOut; // two RGBA16_SFLOAT planes
    uint32_t* dReport;
    CHECK(hipMalloc(&dNr, px * 16) == hipSuccess && hipMalloc(&dZ, px * 4) == hipSuccess && hipMalloc(&dTraced, px * 16) == hipSuccess && hipMalloc(&dProb, px * 4) == hipSuccess);
    CHECK(hipMalloc(&dLobe, px) == hipSuccess && hipMalloc(&dOut, 2 * px * 8) == hipSuccess && hipMalloc(&dReport, 2 * sizeof(NrdHipCoverageReport)) == hipSuccess);
    CHECK(hipMemcpy(dNr, nr.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dZ, z.data(), px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dTraced, traced.data(), px * 16, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dProb, prob.data(), px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemcpy(dLobe, lobe.data(), px, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dOut, 0x5A, 2 * px * 8) == hipSuccess);
    desc.normalRoughness.data = dNr;
    desc.viewZ.data = dZ;
    desc.diffuse.out0.data = dOut;
    desc.specular.out0.data = dOut + px * 4;
    lobes.radianceHitDist.data = dTraced;
    lobes.lobe.data = dLobe;
    lobes.probability = plane(dProb, 4, nrd::Format::R32_SFLOAT);
    CHECK(nrdi.PackInputsLobes(desc, lobes));
    coverage.viewZ.data = dZ;
    coverage.diffuse.plane = desc.diffuse.out0;
    coverage.specular.plane = desc.specular.out0;
    coverage.denoisingRange = 500000.0f;
    CHECK(nrdi.CheckHitDistCoverage(coverage, dReport));
    coverage.area = 2;
    CHECK(nrdi.CheckHitDistCoverage(coverage, dReport + 7));
    CHECK(hipDeviceSynchronize() == hipSuccess);
    std::vector<uint16_t> out(2 * px * 4);
    NrdHipCoverageReport report[2];
    CHECK(hipMemcpy(out.data(), dOut, 2 * px * 8, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(report, dReport, sizeof(report), hipMemcpyDeviceToHost) == hipSuccess);
    size_t mismatches = 0;
    for (size_t i = 0; i < px; i++)
        for (int signal = 0; signal < 2; signal++)
            for (int c = 0; c < 4; c++) // fp16 2.0 = 0x4000: radiance 1 / 0.5, hit distance 2 (not divided)
                mismatches += out[(signal * px + i) * 4 + c] != (lobe[i] == signal ? 0x4000 : 0);
    printf("packed texels: %zu mismatching values\n", mismatches);
    CHECK(mismatches == 0);
    CHECK(report[0].inRangePixels == px && report[0].empty[0] == specularNum && report[0].empty[1] == px - specularNum);
    CHECK(report[0].holes[0] == 1 && report[0].firstHole[0] == (uint32_t)by * W + bx && report[0].holes[1] == 0 && report[0].firstHole[1] == 0xFFFFFFFFu);
    CHECK(report[1].holes[0] == 0 && report[1].holes[1] == 0 && report[1].firstHole[0] == 0xFFFFFFFFu && report[1].empty[0] == specularNum);
    printf("3x3: %u diffuse hole(s), the first at (%u, %u); 5x5: %u\n", report[0].holes[0], report[0].firstHole[0] % W, report[0].firstHole[0] / W, report[1].holes[0]);
    for (void* p : {(void*)dNr, (void*)dZ, (void*)dTraced, (void*)dProb, (void*)dLobe, (void*)dOut, (void*)dReport})
        (void)hipFree(p);
    printf("pack lobes integration OK\n");
    return 0;
}
