// CPU only: the split twins of the front-end / back-end kernels (nrdHipPackInputsSplit / nrdHipResolveOutputsSplit) on the emulation library of tests/emu -- the device
// source compiled for the host -- with every RGB32_SFLOAT plane and every R32_SFLOAT companion placed so that its last byte is the last byte of a mapped page followed by an
// inaccessible one (mmap + mprotect). A 16-byte access on the last 12-byte texel, or a companion read past its end, ends this program with SIGSEGV; it prints a line and
// exits 0 otherwise. Runs pack (the full G-buffer), samples (N = 5), resolve and re-jitter at 67 x 23 and at 1024 x 4 (rows of exactly three pages).
// Linked against tests/emu/libNRD_emu.so (tests/emu/build_emu.py). usage: split_planes_bounds
#include "NRD.h"
#include "NRDHip.h"

#include <sys/mman.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                                  \
    do {                                                                                          \
        if (!(x)) {                                                                               \
            printf("FAILED: %s (line %d): %s\n", #x, __LINE__, nrdHipGetLastFrontEndError());     \
            return 1;                                                                             \
        }                                                                                         \
    } while (0)

// `bytes` of memory whose last byte is the last byte of a page in front of a PROT_NONE page, filled with floats `fill`
static uint8_t* Guarded(size_t bytes, float fill) {
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), mapped = (bytes + page - 1) / page * page;
    uint8_t* base = (uint8_t*)mmap(nullptr, mapped + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (base == (uint8_t*)MAP_FAILED || mprotect(base + mapped, page, PROT_NONE) != 0) {
        printf("mmap / mprotect failed\n");
        _exit(2);
    }
    uint8_t* p = base + mapped - bytes; // (bytes is a multiple of 4: p is dword-aligned)
    for (size_t i = 0; i < bytes / 4; i++)
        memcpy(p + 4 * i, &fill, 4);
    return p;
}

static int Run(uint16_t W, uint16_t H) {
    const size_t px = (size_t)W * H;
    const uint32_t N = 5;
    auto plane = [&](void* p, uint32_t bytes, nrd::Format f) { return NrdHipPlaneDesc{p, (uint32_t)W * bytes, (uint32_t)f, W, H}; };
    auto rgb = [&](size_t layers, float fill) { return plane(Guarded(layers * px * 12, fill), 12, nrd::Format::RGB32_SFLOAT); };
    auto r32 = [&](size_t layers, float fill) { return plane(Guarded(layers * px * 4, fill), 4, nrd::Format::R32_SFLOAT); };
    std::vector<uint8_t> packed(16 * px * 8); // the packed planes: ordinary memory
    auto out = [&](int k, uint32_t bytes, nrd::Format f) { return plane(packed.data() + (size_t)k * px * 8, bytes, f); };

    nrd::CommonSettings cs = {};
    const float fx = 1.2f, fy = 2.0f, zn = 0.1f, zf = 1000.0f;
    const float proj[16] = {fx, 0, 0, 0, 0, fy, 0, 0, 0, 0, zf / (zf - zn), 1.0f, 0, 0, -zn * zf / (zf - zn), 0};
    memcpy(cs.viewToClipMatrix, proj, sizeof(proj));
    for (int k = 0; k < 4; k++)
        cs.worldToViewMatrix[k * 5] = 1.0f;
    cs.rectSize[0] = cs.resourceSize[0] = W;
    cs.rectSize[1] = cs.resourceSize[1] = H;

    // ---- pack: every plane that takes RGB32_SFLOAT, every companion; then the same signals as stacks of N layers
    NrdHipFrontEndDesc d = {};
    NrdHipFrontEndSplit split = {};
    NrdHipFrontEndOptions options = {};
    NrdHipFrontEndSamples samples = {};
    d.hitDistParams[0] = 3.0f, d.hitDistParams[1] = 0.1f, d.hitDistParams[2] = 20.0f, d.hitDistParams[3] = -25.0f;
    d.tanOfLightAngularRadius = 0.02f;
    d.commonSettings = &cs;
    d.normalRoughness = rgb(1, 0.57735f);
    split.roughness = r32(1, 0.5f);
    d.viewZ = r32(1, 10.0f);
    d.motion = rgb(1, 0.25f);
    d.albedo = rgb(1, 0.5f);
    d.rf0 = rgb(1, 0.04f);
    d.distanceToOccluder = r32(1, 2.0f);
    d.translucency = rgb(1, 0.75f);
    const nrd::NormalEncoding enc = nrd::GetLibraryDesc().normalEncoding;
    const bool wideNormals = enc == nrd::NormalEncoding::RGBA16_UNORM || enc == nrd::NormalEncoding::RGBA16_SNORM;
    const nrd::Format nrFormat = enc == nrd::NormalEncoding::RGBA8_UNORM ? nrd::Format::RGBA8_UNORM : enc == nrd::NormalEncoding::RGBA8_SNORM ? nrd::Format::RGBA8_SNORM
        : enc == nrd::NormalEncoding::R10_G10_B10_A2_UNORM ? nrd::Format::R10_G10_B10_A2_UNORM : enc == nrd::NormalEncoding::RGBA16_UNORM ? nrd::Format::RGBA16_UNORM : nrd::Format::RGBA16_SNORM;
    d.outNormalRoughness = out(0, wideNormals ? 8 : 4, nrFormat);
    d.outViewZ = out(1, 4, nrd::Format::R32_SFLOAT);
    d.outMv = out(2, 8, nrd::Format::RGBA16_SFLOAT);
    d.outPenumbra = out(3, 2, nrd::Format::R16_SFLOAT);
    d.outTranslucency = out(4, 4, nrd::Format::RGBA8_UNORM);
    d.diffuse.mode = d.specular.mode = NRD_HIP_SIGNAL_REBLUR_SH;
    d.diffuse.radianceHitDist = rgb(N, 1.5f);
    d.specular.radianceHitDist = rgb(N, 2.5f);
    d.diffuse.direction = rgb(N, 0.57735f);
    d.specular.direction = rgb(N, 0.57735f);
    split.diffuseHitDist = r32(N, 3.0f);
    split.specularHitDist = r32(N, 4.0f);
    d.diffuse.out0 = out(5, 8, nrd::Format::RGBA16_SFLOAT);
    d.diffuse.out1 = out(6, 8, nrd::Format::RGBA16_SFLOAT);
    d.specular.out0 = out(7, 8, nrd::Format::RGBA16_SFLOAT);
    d.specular.out1 = out(8, 8, nrd::Format::RGBA16_SFLOAT);
    // one layer: the LAST one of each stack, which ends at the page edge
    NrdHipFrontEndDesc one = d;
    NrdHipFrontEndSplit oneSplit = split;
    for (NrdHipPlaneDesc* p : {&one.diffuse.radianceHitDist, &one.specular.radianceHitDist, &one.diffuse.direction, &one.specular.direction})
        p->data = (uint8_t*)p->data + (N - 1) * px * 12;
    for (NrdHipPlaneDesc* p : {&oneSplit.diffuseHitDist, &oneSplit.specularHitDist})
        p->data = (uint8_t*)p->data + (N - 1) * px * 4;
    CHECK(nrdHipPackInputsSplit(&one, nullptr, nullptr, &oneSplit, nullptr) == 0);
    options.checkerboardMode = 1;
    CHECK(nrdHipPackInputsSplit(&one, &options, nullptr, &oneSplit, nullptr) == 0);
    // the occlusion mode on its companion alone
    NrdHipFrontEndDesc occ = one;
    occ.diffuse.mode = occ.specular.mode = NRD_HIP_SIGNAL_REBLUR_OCCLUSION;
    occ.diffuse.radianceHitDist = occ.specular.radianceHitDist = NrdHipPlaneDesc{};
    occ.diffuse.out0 = out(9, 2, nrd::Format::R16_UNORM);
    occ.specular.out0 = out(10, 2, nrd::Format::R16_UNORM);
    CHECK(nrdHipPackInputsSplit(&occ, nullptr, nullptr, &oneSplit, nullptr) == 0);
    // N layers, plain and checkerboarded
    samples.diffuse.samplesNum = samples.specular.samplesNum = N;
    samples.diffuse.radianceHitDistLayerBytes = samples.specular.radianceHitDistLayerBytes = samples.diffuse.directionLayerBytes = samples.specular.directionLayerBytes = px * 12;
    split.diffuseHitDistLayerBytes = split.specularHitDistLayerBytes = px * 4;
    samples.hitDistTrimThreshold = 0.5f;
    CHECK(nrdHipPackInputsSplit(&d, nullptr, &samples, &split, nullptr) == 0);
    CHECK(nrdHipPackInputsSplit(&d, &options, &samples, &split, nullptr) == 0);

    // ---- resolve and re-jitter: the SH planes packed above, every colour output and both companions guarded
    NrdHipBackEndDesc b = {};
    NrdHipBackEndSplit backSplit = {};
    NrdHipBackEndOptions backOptions = {};
    memcpy(b.hitDistParams, d.hitDistParams, sizeof(b.hitDistParams));
    b.commonSettings = &cs;
    b.remodulate = 1;
    b.denormalizeHitDist = 1;
    b.normalRoughness = d.outNormalRoughness;
    b.viewZ = d.outViewZ;
    b.albedo = d.albedo;
    b.rf0 = d.rf0;
    b.diffuse.mode = b.specular.mode = NRD_HIP_SIGNAL_REBLUR_SH;
    b.diffuse.resolve = b.specular.resolve = NRD_HIP_RESOLVE_SG;
    b.diffuse.in0 = d.diffuse.out0, b.diffuse.in1 = d.diffuse.out1, b.specular.in0 = d.specular.out0, b.specular.in1 = d.specular.out1;
    b.diffuse.out = rgb(1, 0.0f);
    b.specular.out = rgb(1, 0.0f);
    b.outComposed = rgb(1, 0.0f);
    b.outViewVector = rgb(1, 0.0f);
    b.outDiffFactor = rgb(1, 0.0f);
    b.outSpecFactor = rgb(1, 0.0f);
    backSplit.diffuseHitDist = r32(1, 0.0f);
    backSplit.specularHitDist = r32(1, 0.0f);
    CHECK(nrdHipResolveOutputsSplit(&b, nullptr, &backSplit, nullptr) == 0);
    CHECK(nrdHipResolveOutputsSplit(&b, nullptr, nullptr, nullptr) == 0); // the hit distances dropped
    backOptions.reJitter = 1;
    CHECK(nrdHipResolveOutputsSplit(&b, &backOptions, &backSplit, nullptr) == 0);
    const float* rgbOut = (const float*)b.diffuse.out.data;
    CHECK(rgbOut[3 * (px - 1)] == rgbOut[3 * (px - 1)]); // (the last texel was written with a number)
    return 0;
}

int main() {
    if (Run(67, 23) || Run(1024, 4))
        return 1;
    printf("split planes bounds OK\n");
    return 0;
}
