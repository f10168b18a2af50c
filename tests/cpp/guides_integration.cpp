// IntegrationHip::PackGuides (nrdHipPackGuides) used the way an application would: include/NRD.h + include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against
// libNRD_hip.so.
//   host part: the method forwards to the library -- invalid descriptors are refused with a text that names the field, nothing is enqueued (no device is touched)
//   GPU part:  a 70 x 6 frame, one world position seen by a camera that moved, with values that are exact in every format: IN_VIEWZ, IN_MV (2.5D), a sky row, a confidence plane
// usage: guides_integration [--no-gpu]
#include "NRD.h"
#include "NRDHip.h"
#include "NRDIntegrationHip.hpp"

#include <hip/hip_runtime_api.h>

#include <cmath>
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
    nrd::IntegrationHip nrdi; // the call needs no instance: it runs on the integration's stream (the default one here)

    // column-major: a left-handed projection with clip.xy = view.xy, clip.w = view.z; the camera at the origin now, at ( 1, 0, -4 ) one frame ago
    nrd::CommonSettings cs = {};
    cs.viewToClipMatrix[0] = cs.viewToClipMatrix[5] = cs.viewToClipMatrix[10] = cs.viewToClipMatrix[11] = 1.0f;
    cs.viewToClipMatrix[14] = -0.1f;
    memcpy(cs.viewToClipMatrixPrev, cs.viewToClipMatrix, sizeof(cs.viewToClipMatrix));
    cs.worldToViewMatrix[0] = cs.worldToViewMatrix[5] = cs.worldToViewMatrix[10] = cs.worldToViewMatrix[15] = 1.0f;
    memcpy(cs.worldToViewMatrixPrev, cs.worldToViewMatrix, sizeof(cs.worldToViewMatrix));
    cs.worldToViewMatrixPrev[12] = -1.0f;
    cs.worldToViewMatrixPrev[14] = 4.0f;
    cs.motionVectorScale[0] = 0.125f, cs.motionVectorScale[1] = 0.5f, cs.motionVectorScale[2] = 1.0f;
    cs.isMotionVectorInWorldSpace = false;
    cs.rectSize[0] = cs.resourceSize[0] = W;
    cs.rectSize[1] = cs.resourceSize[1] = H;

    std::vector<float> hostPlane(px * 4);
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    NrdHipGuidesDesc desc = {};
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "no output"));
    desc.outViewZ = plane(hostPlane.data(), 4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "position"));
    desc.position = plane(hostPlane.data(), 16, nrd::Format::RGBA32_SFLOAT);
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "commonSettings"));
    desc.commonSettings = &cs;
    desc.missViewZ = 100.0f; // below the denoising range: not sky to the passes
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "missViewZ"));
    desc.missViewZ = 1e6f;
    desc.reserved = 1;
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "reserved"));
    desc.reserved = 0;
    desc.diffConfidence = plane(hostPlane.data(), 4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.PackGuides(desc));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "diffConfidence"));
    printf("host-only OK\n");
    if (noGpu)
        return 0;

    // X = ( 1, 2, 4 ): viewZ = 4, uv = ( 0.625, 0.25 ); one frame ago Xv = ( 0, 2, 8 ): uv = ( 0.5, 0.375 ). mv = ( -0.125 / 0.125, 0.125 / 0.5, 8 - 4 ) = ( -1, 0.25, 4 ).
    // The last row is sky ( NaN ): missViewZ and a zero vector. Confidence 0.5 -> floor( 127.5 + 0.5 ) = 128
    std::vector<float> X(px * 3), conf(px, 0.5f);
    for (size_t i = 0; i < px; i++) {
        const bool sky = i >= (size_t)W * (H - 1);
        X[3 * i] = sky ? NAN : 1.0f, X[3 * i + 1] = 2.0f, X[3 * i + 2] = 4.0f;
    }
    float *dX, *dConf, *dZ;
    uint16_t* dMv;
    uint8_t* dC8;
    CHECK(hipMalloc(&dX, px * 12) == hipSuccess && hipMalloc(&dConf, px * 4) == hipSuccess && hipMalloc(&dZ, px * 4) == hipSuccess && hipMalloc(&dMv, px * 8) == hipSuccess);
    CHECK(hipMalloc(&dC8, px) == hipSuccess);
    CHECK(hipMemcpy(dX, X.data(), px * 12, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dConf, conf.data(), px * 4, hipMemcpyHostToDevice) == hipSuccess);
    CHECK(hipMemset(dZ, 0x5A, px * 4) == hipSuccess && hipMemset(dMv, 0x5A, px * 8) == hipSuccess && hipMemset(dC8, 0x5A, px) == hipSuccess);
    desc.position = plane(dX, 12, nrd::Format::RGB32_SFLOAT);
    desc.diffConfidence = plane(dConf, 4, nrd::Format::R32_SFLOAT);
    desc.outViewZ = plane(dZ, 4, nrd::Format::R32_SFLOAT);
    desc.outMv = plane(dMv, 8, nrd::Format::RGBA16_SFLOAT);
    desc.outDiffConfidence = plane(dC8, 1, nrd::Format::R8_UNORM);
    if (!nrdi.PackGuides(desc)) {
        printf("PackGuides failed: %s\n", nrdi.GetLastFrontEndError());
        return 1;
    }
    std::vector<float> z(px);
    std::vector<uint16_t> mv(px * 4);
    std::vector<uint8_t> c8(px);
    CHECK(hipDeviceSynchronize() == hipSuccess && hipMemcpy(z.data(), dZ, px * 4, hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(mv.data(), dMv, px * 8, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(c8.data(), dC8, px, hipMemcpyDeviceToHost) == hipSuccess);
    size_t wrong = 0;
    for (size_t i = 0; i < px; i++) {
        const bool sky = i >= (size_t)W * (H - 1);
        const uint16_t want[4] = {(uint16_t)(sky ? 0 : 0xBC00), (uint16_t)(sky ? 0 : 0x3400), (uint16_t)(sky ? 0 : 0x4400), 0};
        wrong += z[i] != (sky ? 1e6f : 4.0f) || memcmp(&mv[4 * i], want, 8) != 0 || c8[i] != 128;
    }
    printf("view depth, motion vectors and confidence: %zu wrong pixels\n", wrong);
    CHECK(wrong == 0);
    hipFree(dX), hipFree(dConf), hipFree(dZ), hipFree(dMv), hipFree(dC8);
    printf("guides integration OK\n");
    return 0;
}
