// nrdHipCheckInputs (include/NRDHip.h): one streaming audit of the bound IN_* planes against NRD's input rules. It only reads the planes and writes nothing but the report.
//
// Shape: that of the front-end kernels -- a wave covers 64 consecutive pixels of one row, so every load is one contiguous wave-wide segment (viewZ 256 B, the fp16 planes 512 B).
// No LDS, no scratch. REBLUR_DIFFUSE_SPECULAR reads 28 B per pixel (viewZ 4, IN_MV 8, two signals 8 + 8); the noisy rules are tested only where the pixel is in range.
//
// Reduction: violations are rare, so the clean path must not pay for them. A wave keeps its counters in uniform registers (wave-wide ballot + population count; within a row a
// wave's lanes are in raster order, so the first set bit of a ballot is the raster-first pixel) and loops over many row segments: the grid is a few workgroups per CU, not one per
// tile. At its exit a wave issues one atomicAdd for inRangePixels, and one atomicAdd + one atomicMin per rule that fired -- none on a clean frame. 4 096 waves at most: a few
// thousand atomics on one word per launch, spread over the kernel's run, where one wave per 64 x 4 tile would be 57 600 at 1440p (one contended word takes about 88 returning
// atomics per microsecond). Counts and minima are integers: the report does not depend on the order in which the waves arrive.
#include "nrdmath.h"
#include "passes.h"

#include "NRDHip.h"

namespace nrdhip {

namespace {

#ifdef NRD_EMU
// The CPU emulation (tests/emu) has __any / __all / __shfl_xor and atomicMax only: the ballot is an OR-butterfly over the lanes (all 64 lanes of a wave stay in the loop below),
// the two atomics go through the compiler's builtins as the shim's atomicMax does.
struct WaveMask {
    uint32_t lo, hi;
};
inline WaveMask Ballot(bool p) {
    const uint32_t lane = threadIdx.x & 63u;
    WaveMask m = {p && lane < 32u ? 1u << lane : 0u, p && lane >= 32u ? 1u << (lane - 32u) : 0u};
    for (int o = 1; o < 64; o <<= 1) {
        m.lo |= __shfl_xor(m.lo, o);
        m.hi |= __shfl_xor(m.hi, o);
    }
    return m;
}
inline bool None(WaveMask m) { return (m.lo | m.hi) == 0u; }
inline uint32_t Count(WaveMask m) { return (uint32_t)(__builtin_popcount(m.lo) + __builtin_popcount(m.hi)); }
inline uint32_t FirstLane(WaveMask m) { return m.lo ? (uint32_t)__builtin_ctz(m.lo) : 32u + (uint32_t)__builtin_ctz(m.hi); }
inline int WaveUniform(int x) { return x; }
inline void atomicAdd(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline void atomicMin(uint32_t* p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}
#else
typedef unsigned long long WaveMask;
NRD_D WaveMask Ballot(bool p) { return __ballot(p ? 1 : 0); }
NRD_D bool None(WaveMask m) { return m == 0ull; }
NRD_D uint32_t Count(WaveMask m) { return (uint32_t)__popcll(m); }
NRD_D uint32_t FirstLane(WaveMask m) { return (uint32_t)__builtin_ctzll(m); }
NRD_D int WaveUniform(int x) { return __builtin_amdgcn_readfirstlane(x); } // the same in every lane, and provably so: segment arithmetic and totals stay on the scalar unit
#endif

// Non-finite = all exponent bits set, tested on the raw word: no conversion, and no compiler folding of a float comparison with itself
NRD_D bool HalfNotFinite(uint32_t h) { return (h & 0x7C00u) == 0x7C00u; }
NRD_D bool FloatNotFinite(uint32_t f) { return (f & 0x7F800000u) == 0x7F800000u; }
NRD_D bool HalfNegative(uint32_t h) { return (h & 0x8000u) != 0u && (h & 0x7FFFu) != 0u; } // -0.0 is not negative (callers exclude NaN / INF)
// any of the four (or, xyzOnly, the first three) halves of an RGBA16_SFLOAT texel
NRD_D bool TexelNotFinite(uint2 raw, bool xyzOnly = false) {
    return HalfNotFinite(raw.x) || HalfNotFinite(raw.x >> 16) || HalfNotFinite(raw.y) || (!xyzOnly && HalfNotFinite(raw.y >> 16));
}

constexpr uint32_t IN_RANGE_BIT = 1u << NRD_HIP_INPUT_RULES_NUM; // bit r < 8: the pixel violates rule r

// Which planes a launch reads is a compile-time mask for the plane sets of the denoisers (bit i = plane i of CheckInputsParams in declaration order), so that the loads of a
// trip are straight-line code: no branch on a plane's presence, none on a lane's position (coordinates are clamped into the rect instead, where every texel is addressable, and
// the lane's result is dropped afterwards), hence nothing the compiler has to wait for between two loads. What bounds a streaming kernel with 4- and 8-byte loads is the number
// of bytes a wave has in flight: nothing here waits for viewZ before it asks for the noisy texels -- the range test masks them afterwards. PLANES = 0: any other plane set,
// presence tested at run time (uniform branches).
enum : uint32_t { HAS_VIEWZ = 1, HAS_MV = 2, HAS_DIFF0 = 4, HAS_DIFF1 = 8, HAS_SPEC0 = 16, HAS_SPEC1 = 32, HAS_PENUMBRA = 64, HAS_SIGNAL = 128 };
template <uint32_t PLANES>
NRD_D bool Has(uint32_t plane, const Plane& p) {
    return PLANES ? (PLANES & plane) != 0u : p.ptr != nullptr;
}

struct PixelTexels {
    uint32_t viewZ;
    uint2 mv, diff0, diff1, spec0, spec1;
    uint32_t penumbra;
    uint4 signal;
};

// (x, y): a pixel inside the rect. A checkerboarded signal lives in the left half of its plane, at column x >> 1 (kernels_reblur_ta.hip "Checkerboard"); the pixel of a pair
// that has no data this frame loads the pair's texel too and ignores it (ClassifyPixel).
template <uint32_t PLANES>
NRD_D PixelTexels LoadPixel(const CheckInputsParams& p, int x, int y) {
    PixelTexels t = {};
    if (Has<PLANES>(HAS_VIEWZ, p.viewZ))
        t.viewZ = LoadR32U(p.viewZ, x, y);
    if (Has<PLANES>(HAS_MV, p.mv))
        t.mv = *TexelPtr<const uint2>(p.mv, x, y);
    const int dx = p.diffCell != 2u ? x >> 1 : x, sx = p.specCell != 2u ? x >> 1 : x;
    if (Has<PLANES>(HAS_DIFF0, p.diff0))
        t.diff0 = *TexelPtr<const uint2>(p.diff0, dx, y);
    if (Has<PLANES>(HAS_DIFF1, p.diff1))
        t.diff1 = *TexelPtr<const uint2>(p.diff1, dx, y);
    if (Has<PLANES>(HAS_SPEC0, p.spec0))
        t.spec0 = *TexelPtr<const uint2>(p.spec0, sx, y);
    if (Has<PLANES>(HAS_SPEC1, p.spec1))
        t.spec1 = *TexelPtr<const uint2>(p.spec1, sx, y);
    if (Has<PLANES>(HAS_PENUMBRA, p.penumbra))
        t.penumbra = LoadR16U(p.penumbra, x, y);
    if (Has<PLANES>(HAS_SIGNAL, p.signal))
        t.signal = *TexelPtr<const uint4>(p.signal, x, y);
    return t;
}

// bits { NOT_FINITE, HITDIST_RANGE } of one noisy signal
NRD_D uint32_t ClassifySignal(uint2 t0, uint2 t1, uint32_t normalized, uint32_t notFiniteRule, uint32_t rangeRule) {
    const bool notFinite = TexelNotFinite(t0) || TexelNotFinite(t1);
    const uint32_t hitDist = t0.y >> 16;
    const bool outOfRange = !HalfNotFinite(hitDist) && (HalfNegative(hitDist) || (normalized != 0u && (hitDist & 0x8000u) == 0u && hitDist > 0x3C00u)); // 0x3C00 = 1.0
    return (notFinite ? 1u << notFiniteRule : 0u) | (outOfRange ? 1u << rangeRule : 0u);
}

// rule bits + IN_RANGE_BIT of pixel (x, y) of the rect from its texels; 0 for a lane outside (whose texels are those of a clamped position)
template <uint32_t PLANES>
NRD_D uint32_t ClassifyPixel(const CheckInputsParams& p, const PixelTexels& t, int x, int y, bool inside) {
    uint32_t bits = IN_RANGE_BIT;
    bool inRange = true; // a list that does not read IN_VIEWZ (REFERENCE) has no sky: every pixel of the rect is processed
    if (Has<PLANES>(HAS_VIEWZ, p.viewZ)) {
        const bool zNotFinite = FloatNotFinite(t.viewZ);
        const bool denoised = !(Abs(__uint_as_float(t.viewZ) * p.viewZScale) > p.denoisingRange); // the tile classification's predicate (kernels_common.hip DecodeGuidesClassifyKernel), not the README's >=
        bits = (zNotFinite ? 1u << NRD_HIP_INPUT_RULE_VIEWZ_NOT_FINITE : 0u) | (denoised ? IN_RANGE_BIT : 0u);
        inRange = denoised && !zNotFinite; // a pixel whose viewZ is not finite counts under rule 0 only
    }
    if (TexelNotFinite(t.mv, true))
        bits |= 1u << NRD_HIP_INPUT_RULE_MV_NOT_FINITE;
    // the noisy rules: garbage beyond the denoising range is allowed, and a checkerboarded signal is read only where the pixel's colour is the signal's cell. Masks, not
    // branches: a test behind a branch invites the compiler to move the texel's load there too, where it would be waited for on its own
    const uint32_t colour = CheckerBoard((uint32_t)x, (uint32_t)y, p.frameIndex);
    const uint32_t diffMask = inRange && (p.diffCell == 2u || colour == p.diffCell) ? ~0u : 0u, specMask = inRange && (p.specCell == 2u || colour == p.specCell) ? ~0u : 0u;
    bits |= ClassifySignal(t.diff0, t.diff1, p.diffNormalized, NRD_HIP_INPUT_RULE_DIFF_NOT_FINITE, NRD_HIP_INPUT_RULE_DIFF_HITDIST_RANGE) & diffMask;
    bits |= ClassifySignal(t.spec0, t.spec1, p.specNormalized, NRD_HIP_INPUT_RULE_SPEC_NOT_FINITE, NRD_HIP_INPUT_RULE_SPEC_HITDIST_RANGE) & specMask;
    bits |= (HalfNotFinite(t.penumbra) || HalfNegative(t.penumbra)) && inRange ? 1u << NRD_HIP_INPUT_RULE_PENUMBRA_INVALID : 0u;
    if (FloatNotFinite(t.signal.x) || FloatNotFinite(t.signal.y) || FloatNotFinite(t.signal.z) || FloatNotFinite(t.signal.w))
        bits |= 1u << NRD_HIP_INPUT_RULE_SIGNAL_NOT_FINITE;
    return inside ? bits : 0u;
}

struct WaveTotals {
    uint32_t inRange;
    uint32_t count[NRD_HIP_INPUT_RULES_NUM], first[NRD_HIP_INPUT_RULES_NUM];
};

// folds the 64 pixels of one row segment (first pixel = rect index `base`) into the wave's uniform totals
NRD_D void Accumulate(WaveTotals& t, uint32_t bits, uint32_t base) {
    t.inRange += Count(Ballot((bits & IN_RANGE_BIT) != 0u));
    if (!__any((bits & (IN_RANGE_BIT - 1u)) != 0u))
        return; // the clean path: one ballot, one vote
#pragma unroll
    for (uint32_t r = 0; r < NRD_HIP_INPUT_RULES_NUM; r++) {
        const WaveMask m = Ballot((bits >> r & 1u) != 0u);
        if (None(m))
            continue;
        t.count[r] += Count(m);
        t.first[r] = min(t.first[r], base + FirstLane(m));
    }
}

constexpr int CHECK_WAVES_PER_BLOCK = 4;
constexpr int CHECK_MAX_BLOCKS = 1024; // 4 workgroups of 4 waves per CU of an MI355X
constexpr int CHECK_SEGMENTS_PER_TRIP = 4; // x 64 pixels x 28 B: 7 KiB of loads in flight per wave on REBLUR_DIFFUSE_SPECULAR

template <uint32_t PLANES>
__global__ __launch_bounds__(64 * CHECK_WAVES_PER_BLOCK) void CheckInputsKernel(CheckInputsParams p, int segmentsPerRow, int segments, uint32_t* report) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * CHECK_WAVES_PER_BLOCK + WaveUniform((int)(threadIdx.x >> 6)), waves = gridDim.x * CHECK_WAVES_PER_BLOCK;
    WaveTotals t;
    t.inRange = 0u;
#pragma unroll
    for (uint32_t r = 0; r < NRD_HIP_INPUT_RULES_NUM; r++)
        t.count[r] = 0u, t.first[r] = 0xFFFFFFFFu;
    // the waves of a workgroup take neighbouring segments, CHECK_SEGMENTS_PER_TRIP of them per trip with all their loads issued first. Every lane of a wave runs every trip
    // (a lane outside the rect and a segment past the end load a clamped position and classify to 0): the votes are wave-wide
    for (int s0 = wave; s0 < segments; s0 += CHECK_SEGMENTS_PER_TRIP * waves) {
        PixelTexels texels[CHECK_SEGMENTS_PER_TRIP];
        int x0[CHECK_SEGMENTS_PER_TRIP], y[CHECK_SEGMENTS_PER_TRIP];
#pragma unroll
        for (int k = 0; k < CHECK_SEGMENTS_PER_TRIP; k++) {
            const int s = min(s0 + k * waves, segments - 1);
            y[k] = s / segmentsPerRow;
            x0[k] = (s - y[k] * segmentsPerRow) * 64;
            texels[k] = LoadPixel<PLANES>(p, min(x0[k] + lane, p.rectW - 1), y[k]);
        }
#pragma unroll
        for (int k = 0; k < CHECK_SEGMENTS_PER_TRIP; k++) {
            const int x = x0[k] + lane;
            const uint32_t bits = ClassifyPixel<PLANES>(p, texels[k], x, y[k], s0 + k * waves < segments && x < p.rectW);
            Accumulate(t, bits, (uint32_t)y[k] * (uint32_t)p.rectW + (uint32_t)x0[k]);
        }
    }
    if (lane != 0)
        return;
    if (wave == 0)
        report[0] = (uint32_t)p.rectW * (uint32_t)p.rectH; // NrdHipInputReport::pixels (16-bit sizes: below 2^32)
    if (t.inRange)
        atomicAdd(report + 1, t.inRange);
#pragma unroll
    for (uint32_t r = 0; r < NRD_HIP_INPUT_RULES_NUM; r++)
        if (t.count[r]) {
            atomicAdd(report + 2 + r, t.count[r]);
            atomicMin(report + 2 + NRD_HIP_INPUT_RULES_NUM + r, t.first[r]);
        }
}

} // namespace

void LaunchCheckInputs(hipStream_t stream, const CheckInputsParams& p, uint32_t* report) {
    static_assert(sizeof(NrdHipInputReport) == 4 * (2 + 2 * NRD_HIP_INPUT_RULES_NUM), "the kernel addresses the report as words: pixels, inRangePixels, count[], first[]");
    if (p.rectW <= 0 || p.rectH <= 0)
        return;
    const int segmentsPerRow = (p.rectW + 63) / 64, segments = segmentsPerRow * p.rectH; // < 2^26 for 16-bit frame sizes
    const int blocks = (segments + CHECK_WAVES_PER_BLOCK - 1) / CHECK_WAVES_PER_BLOCK;
    const dim3 grid((unsigned)(blocks < CHECK_MAX_BLOCKS ? blocks : CHECK_MAX_BLOCKS)), block(64 * CHECK_WAVES_PER_BLOCK);
    const Plane* planes[] = {&p.viewZ, &p.mv, &p.diff0, &p.diff1, &p.spec0, &p.spec1, &p.penumbra, &p.signal};
    uint32_t have = 0;
    for (int i = 0; i < 8; i++)
        have |= planes[i]->ptr ? 1u << i : 0u;
    constexpr uint32_t GUIDES = HAS_VIEWZ | HAS_MV;
#define NRD_CHECK_INPUTS_CASE(MASK)                                                                               \
    case MASK:                                                                                                    \
        hipLaunchKernelGGL(CheckInputsKernel<MASK>, grid, block, 0, stream, p, segmentsPerRow, segments, report); \
        break
    switch (have) {
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_DIFF0 | HAS_SPEC0);                         // REBLUR / RELAX _DIFFUSE_SPECULAR
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_DIFF0);                                     // _DIFFUSE
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_SPEC0);                                     // _SPECULAR
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_DIFF0 | HAS_DIFF1 | HAS_SPEC0 | HAS_SPEC1); // _DIFFUSE_SPECULAR_SH
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_DIFF0 | HAS_DIFF1);                         // _DIFFUSE_SH
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_SPEC0 | HAS_SPEC1);                         // _SPECULAR_SH
        NRD_CHECK_INPUTS_CASE(GUIDES | HAS_PENUMBRA);                                  // SIGMA
        NRD_CHECK_INPUTS_CASE(GUIDES);                                                 // the REBLUR occlusion families
        NRD_CHECK_INPUTS_CASE(HAS_SIGNAL);                                             // REFERENCE
        default: // several denoisers in one list
            hipLaunchKernelGGL(CheckInputsKernel<0u>, grid, block, 0, stream, p, segmentsPerRow, segments, report);
            break;
    }
#undef NRD_CHECK_INPUTS_CASE
}

} // namespace nrdhip
