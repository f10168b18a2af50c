// IntegrationHip::PackInputsDecimated / ResolveOutputsUpsampled (nrdHipPackInputsDecimated / nrdHipResolveOutputsUpsampled) used the way an application would: include/NRD.h +
// include/NRDHip.h + include/NRDIntegrationHip.hpp, linked against libNRD_hip.so. Host only: the methods forward to the library, invalid descriptors are refused with a text
// that names the field and nothing is enqueued (no device is touched).
#include "NRD.h"
#include "NRDHip.h"
#include "NRDIntegrationHip.hpp"

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

int main() {
    const uint16_t W = 70, H = 7, w = 35, h = 4;
    static_assert(sizeof(NrdHipBackEndUpsample) == 56, "two planes, a threshold, a reserved word");
    nrd::IntegrationHip nrdi; // the calls need no instance: they run on the integration's stream (the default one here)
    std::vector<float> host((size_t)W * H * 4);
    auto full = [&](uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{host.data(), (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    auto low = [&](uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{host.data(), (uint32_t)w * bytes, (uint32_t)f, w, h}; };

    // ---- the decimated pack
    NrdHipFrontEndDesc front = {};
    front.normalRoughness = full(16, nrd::Format::RGBA32_SFLOAT);
    front.viewZ = full(4, nrd::Format::R32_SFLOAT);
    front.outViewZ = low(4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.PackInputsDecimated(front, nullptr, nullptr, nullptr, 2));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "guideShift"));
    NrdHipFrontEndOptions options = {1, 0};
    CHECK(!nrdi.PackInputsDecimated(front, &options));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "checkerboardMode") && strstr(nrdi.GetLastFrontEndError(), "out of scope"));
    front.outViewZ = full(4, nrd::Format::R32_SFLOAT); // an output with the full size
    CHECK(!nrdi.PackInputsDecimated(front));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "outViewZ") && strstr(nrdi.GetLastFrontEndError(), ">> 1"));
    front.outViewZ = low(4, nrd::Format::R32_SFLOAT);
    front.viewZ = low(4, nrd::Format::R32_SFLOAT); // a G-buffer plane with the low size
    CHECK(!nrdi.PackInputsDecimated(front));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "viewZ") && strstr(nrdi.GetLastFrontEndError(), "size"));

    // ---- the upsampled resolve
    nrd::CommonSettings cs = {};
    cs.viewToClipMatrix[0] = cs.viewToClipMatrix[5] = cs.viewToClipMatrix[10] = cs.viewToClipMatrix[11] = 1.0f;
    cs.viewToClipMatrix[14] = -0.1f;
    cs.worldToViewMatrix[0] = cs.worldToViewMatrix[5] = cs.worldToViewMatrix[10] = cs.worldToViewMatrix[15] = 1.0f;
    cs.rectSize[0] = cs.resourceSize[0] = W; // the full size: not the denoiser's rect
    cs.rectSize[1] = cs.resourceSize[1] = H;
    NrdHipBackEndDesc back = {};
    back.diffuse.mode = NRD_HIP_SIGNAL_RELAX_RADIANCE;
    back.diffuse.in0 = low(8, nrd::Format::RGBA16_SFLOAT);
    back.diffuse.out = full(16, nrd::Format::RGBA32_SFLOAT);
    NrdHipBackEndUpsample upsample = {};
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "lowViewZ"));
    upsample.lowViewZ = low(4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "viewZ"));
    back.viewZ = full(4, nrd::Format::R32_SFLOAT);
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "commonSettings"));
    back.commonSettings = &cs;
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "rectSize"));
    cs.rectSize[0] = w, cs.rectSize[1] = h;
    upsample.depthThreshold = NAN;
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "depthThreshold"));
    upsample.depthThreshold = 0.1f;
    upsample.reserved = 7;
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "reserved"));
    upsample.reserved = 0;
    upsample.outSource = full(1, nrd::Format::R8_UNORM);
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "outSource"));
    upsample.outSource = full(1, nrd::Format::R8_UINT);
    NrdHipBackEndOptions reJitter = {};
    reJitter.reJitter = 1;
    back.diffuse.mode = back.specular.mode = NRD_HIP_SIGNAL_REBLUR_SH;
    back.diffuse.resolve = back.specular.resolve = NRD_HIP_RESOLVE_SG;
    CHECK(!nrdi.ResolveOutputsUpsampled(back, upsample, &reJitter));
    CHECK(strstr(nrdi.GetLastFrontEndError(), "reJitter") && strstr(nrdi.GetLastFrontEndError(), "out of scope"));
    printf("host-only OK\n");
    return 0;
}
