// nrdHipCheckHitDistCoverage (include/NRDHip.h): does every in-range pixel have a valid hit distance within the 3x3 / 5x5 texels the hit-distance reconstruction searches? The
// audit of a probabilistic diffuse / specular split (nrdHipPackInputsLobes), whose dithering is the application's. It only reads the packed planes and writes nothing but the report.
//
// Shape: that of the stencil passes -- 256 threads own a 32 x 8 pixel tile and stage the tile plus a 2-texel border (36 x 12 texels) in LDS; a workgroup is four such groups. A texel's viewZ and the 16 bits that
// carry each signal's hit distance are loaded once, by predicated loads (a texel outside the plane is not read and is invalid), and reduced at once to ONE byte: bit s = "a valid
// neighbour for signal s" (inside, in range, hit distance != 0), bit 2 = in range. 432 bytes of LDS per tile, twice: the loads of a trip's next tile are in flight while the 9 or
// 25 taps of the current one read bytes from LDS, and one barrier per trip separates the two buffers.
// The hit distance != 0 test is the passes' test on the decoded value, made on the stored bits: an fp16 is zero iff its low 15 bits are (a NaN is not), an UNORM16 / SNORM16
// iff all 16 are (-32768 decodes to -1).
//
// Reduction: as in nrdHipCheckInputs (kernels_check_inputs.hip) -- a wave keeps its five counters and two minima in uniform registers (ballot + population count; a wave is two
// tile rows in raster order, so the first set bit of a ballot is its raster-first pixel) while the workgroup loops over tiles. In a split frame every wave has pixels to count in
// three of the counters, and the seven words of the report share one cache line, which takes some 90 atomics per microsecond: one atomic per wave and counter from 1 024
// workgroups of 4 waves measured 0.172 ms at 2560 x 1440, all of it the atomics. So the 16 waves of a workgroup fold into LDS first and the workgroup issues one global atomic per
// counter that is not zero: at most 256 workgroups, under a thousand atomics per launch however large the frame. Counts and minima are integers: the report does not depend on
// the order in which the waves arrive.
#include "NRD.h"
#include "NRDHip.h"

#include "planes.h"
#include "frontend_host.h"

#include <cstddef>
#include <string>

using namespace nrdhip;

namespace {

// (the votes of kernels_check_inputs.hip, which keeps them private: the CPU emulation of tests/emu has __any / __shfl_xor only, hence the butterfly)
#ifdef NRD_EMU
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
#endif

constexpr int kTileW = 32, kTileH = 8, kBorder = 2;
constexpr int kStageW = kTileW + 2 * kBorder, kStageH = kTileH + 2 * kBorder, kStageTexels = kStageW * kStageH; // 36 x 12 = 432
constexpr int kGroups = 4;      // tiles a workgroup of 1 024 threads works on at a time
constexpr int kMaxBlocks = 512; // two workgroups of 16 waves per CU of an MI355X: every wave slot
constexpr uint32_t kInRange = 4u; // bit s < 2: a valid neighbour for signal s

// how a signal's plane carries its hit distance: 16 bits at `channelOffset` of a `texelBytes` texel; zeroMask selects the bits that are all clear iff the decoded value is 0
struct CoverageSignal {
    FePlane plane; // ptr == nullptr: absent
    uint32_t texelBytes, channelOffset, zeroMask;
};

struct CoverageArgs {
    FePlane viewZ;
    CoverageSignal signal[2];
    float viewZScale, denoisingRange;
    int32_t w, h, tilesX, tiles;
};

// the validity byte of texel ( x, y ); 0 outside the plane, where nothing is read
NRD_D uint32_t ClassifyTexel(const CoverageArgs& a, int x, int y) {
    if ((unsigned)x >= (unsigned)a.w || (unsigned)y >= (unsigned)a.h)
        return 0u;
    const uint32_t zBits = *(const uint32_t*)(a.viewZ.ptr + __umul24((uint32_t)y, a.viewZ.pitch) + (uint32_t)x * 4u);
    uint32_t stored[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < 2; s++)
        if (a.signal[s].plane.ptr) // uniform
            stored[s] = *(const uint16_t*)(a.signal[s].plane.ptr + __umul24((uint32_t)y, a.signal[s].plane.pitch) + (uint32_t)x * a.signal[s].texelBytes + a.signal[s].channelOffset);
    const bool finite = (zBits & 0x7F800000u) != 0x7F800000u;
    const bool inRange = finite && !(fabsf(__uint_as_float(zBits) * a.viewZScale) > a.denoisingRange);
    if (!inRange)
        return 0u;
    return kInRange | ((stored[0] & a.signal[0].zeroMask) ? 1u : 0u) | ((stored[1] & a.signal[1].zeroMask) ? 2u : 0u);
}

// { inRangePixels 0, empty[] 0, holes[] 0, firstHole[] 0xFFFFFFFF }, in stream order in front of the audit. A kernel, not two hipMemsetAsync: like every other call that is
// captured into a graph here, the call then consists of kernel nodes alone
__global__ void __launch_bounds__(64) ResetCoverageReportKernel(uint32_t* report) {
    if (threadIdx.x < 7u)
        report[threadIdx.x] = threadIdx.x < 5u ? 0u : 0xFFFFFFFFu;
}

// RADIUS: nrd::HitDistanceReconstructionMode -- 1 = 3x3, 2 = 5x5. A workgroup is kGroups groups of 256 threads, each with a tile of its own per trip
template <int RADIUS>
__global__ void __launch_bounds__(256 * kGroups) HitDistCoverageKernel(const CoverageArgs a, uint32_t* report) {
    __shared__ uint8_t s_Valid[2][kGroups][kStageH][kStageW]; // double-buffered: the bytes of the next trip's tiles are written while this trip's are read
    __shared__ uint32_t s_Totals[7];
    const int group = (int)(threadIdx.x >> 8), tid = (int)(threadIdx.x & 255u), px = tid & (kTileW - 1), py = tid >> 5;
    const uint32_t lane = threadIdx.x & 63u;
    if (threadIdx.x < 7u)
        s_Totals[threadIdx.x] = threadIdx.x < 5u ? 0u : 0xFFFFFFFFu;
    uint32_t inRangeNum = 0u, emptyNum[2] = {0u, 0u}, holesNum[2] = {0u, 0u}, firstHole[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    // this thread's one or two texels of its group's 36 x 12 stage; a tile index past the end has its origin outside the plane: every texel classifies to 0, nothing is read
    const int i0 = tid, i1 = tid + 256;
    const int sy0 = i0 / kStageW, sx0 = i0 - sy0 * kStageW, sy1 = i1 / kStageW, sx1 = i1 - sy1 * kStageW;
    auto origin = [&](int tile, int& x0, int& y0) {
        const int tileY = tile / a.tilesX;
        x0 = tile < a.tiles ? (tile - tileY * a.tilesX) * kTileW : a.w + kBorder;
        y0 = tileY * kTileH;
    };
    const int stride = (int)gridDim.x * kGroups;
    int tile = (int)blockIdx.x * kGroups + group, x0, y0;
    origin(tile, x0, y0);
    s_Valid[0][group][sy0][sx0] = (uint8_t)ClassifyTexel(a, x0 + sx0 - kBorder, y0 + sy0 - kBorder);
    if (i1 < kStageTexels)
        s_Valid[0][group][sy1][sx1] = (uint8_t)ClassifyTexel(a, x0 + sx1 - kBorder, y0 + sy1 - kBorder);
    __syncthreads();
    // every thread of the workgroup makes the same number of trips (the first group's tile decides: the others' indices are larger): the barrier is met by all
    for (int first = (int)blockIdx.x * kGroups, buffer = 0; first < a.tiles; first += stride, tile += stride, buffer ^= 1) {
        // the loads of the next trip are issued in front of this trip's taps and waited for behind them
        int nx0, ny0;
        origin(tile + stride, nx0, ny0);
        const uint32_t next0 = ClassifyTexel(a, nx0 + sx0 - kBorder, ny0 + sy0 - kBorder);
        const uint32_t next1 = i1 < kStageTexels ? ClassifyTexel(a, nx0 + sx1 - kBorder, ny0 + sy1 - kBorder) : 0u;
        const uint32_t own = s_Valid[buffer][group][py + kBorder][px + kBorder]; // 0 for a pixel outside the plane
        uint32_t around = 0u;
#pragma unroll
        for (int dy = -RADIUS; dy <= RADIUS; dy++)
#pragma unroll
            for (int dx = -RADIUS; dx <= RADIUS; dx++)
                around |= s_Valid[buffer][group][py + kBorder + dy][px + kBorder + dx];
        const bool inRange = (own & kInRange) != 0u;
        inRangeNum += Count(Ballot(inRange));
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (!a.signal[s].plane.ptr) // uniform
                continue;
            const bool empty = inRange && !(own & (1u << s)); // in range, inside: the bit is clear iff the pixel's own hit distance is 0
            const WaveMask e = Ballot(empty);
            if (None(e))
                continue;
            emptyNum[s] += Count(e);
            const bool hole = empty && !(around & (1u << s));
            const WaveMask m = Ballot(hole);
            if (None(m))
                continue;
            holesNum[s] += Count(m);
            // the raster-first hole of the wave is the pixel of its first set lane: lane l of wave v of a group is pixel ( l & 31, 2 v + ( l >> 5 ) ) of the group's tile
            const uint32_t l = FirstLane(m);
            const uint32_t x = (uint32_t)x0 + (l & 31u), y = (uint32_t)y0 + 2u * ((uint32_t)tid >> 6) + (l >> 5);
            firstHole[s] = min(firstHole[s], y * (uint32_t)a.w + x);
        }
        s_Valid[buffer ^ 1][group][sy0][sx0] = (uint8_t)next0;
        if (i1 < kStageTexels)
            s_Valid[buffer ^ 1][group][sy1][sx1] = (uint8_t)next1;
        x0 = nx0;
        y0 = ny0;
        __syncthreads(); // one barrier per trip: the buffer written above was last read in front of the previous trip's barrier
    }
    // the waves of a workgroup fold into LDS, the workgroup issues one global atomic per counter that is not zero: one contended word takes few atomics per microsecond
    if (lane == 0u) {
        if (inRangeNum)
            atomicAdd(&s_Totals[0], inRangeNum);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            if (emptyNum[s])
                atomicAdd(&s_Totals[1 + s], emptyNum[s]);
            if (holesNum[s]) {
                atomicAdd(&s_Totals[3 + s], holesNum[s]);
                atomicMin(&s_Totals[5 + s], firstHole[s]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 5u && s_Totals[threadIdx.x])
        atomicAdd(report + threadIdx.x, s_Totals[threadIdx.x]);
    else if (threadIdx.x >= 5u && threadIdx.x < 7u && s_Totals[threadIdx.x] != 0xFFFFFFFFu)
        atomicMin(report + threadIdx.x, s_Totals[threadIdx.x]);
}

CoverageSignal Signal(Checker& c, const NrdHipCoverageSignal& s, const char* name) {
    using F = nrd::Format;
    CoverageSignal out = {};
    if (!s.plane.data || c.Failed())
        return out;
    const F f = (F)s.plane.format;
    if (f != F::RGBA16_SFLOAT && f != F::R16_UNORM && f != F::RGBA16_SNORM) {
        c.Error(nrd::Result::UNSUPPORTED, name, "unexpected format: RGBA16_SFLOAT (IN_*_RADIANCE_HITDIST, IN_*_SH0), R16_UNORM (IN_*_HITDIST) or RGBA16_SNORM (IN_DIFF_DIRECTION_HITDIST)");
        return out;
    }
    out.plane = c.Check(s.plane, name, nullptr, f);
    out.texelBytes = f == F::R16_UNORM ? 2u : 8u;
    out.channelOffset = f == F::R16_UNORM ? 0u : 6u; // .w
    out.zeroMask = f == F::RGBA16_SFLOAT ? 0x7FFFu : 0xFFFFu;
    return out;
}

} // namespace

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipCheckHitDistCoverage(const NrdHipCoverageDesc* d, void* deviceReport, void* hipStream) {
    static_assert(sizeof(NrdHipCoverageReport) == 4 * 7, "the kernel addresses the report as words: inRangePixels, empty[ 2 ], holes[ 2 ], firstHole[ 2 ]");
    const char* entry = "nrdHipCheckHitDistCoverage";
    if (!d)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": null descriptor");
    if (!deviceReport || ((uintptr_t)deviceReport % 4u) != 0)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": deviceReport: null or not 4-byte aligned");
    if (d->area < 1u || d->area > 2u)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": area: 1 (3x3) or 2 (5x5), the areas of nrd::HitDistanceReconstructionMode");
    if (d->reserved)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": reserved: must be 0");
    if (!d->diffuse.plane.data && !d->specular.plane.data)
        return Fail(nrd::Result::INVALID_ARGUMENT, std::string(entry) + ": diffuse / specular: no signal plane to audit");
    Checker c{entry};
    CoverageArgs a = {};
    a.viewZ = c.Check(d->viewZ, "viewZ", "required: IN_VIEWZ decides which pixels are in range", nrd::Format::R32_SFLOAT);
    a.signal[0] = Signal(c, d->diffuse, "diffuse.plane");
    a.signal[1] = Signal(c, d->specular, "specular.plane");
    if (c.Failed())
        return c.result;
    a.viewZScale = d->viewZScale == 0.0f ? 1.0f : d->viewZScale;
    a.denoisingRange = d->denoisingRange;
    a.w = c.w;
    a.h = c.h;
    a.tilesX = (c.w + kTileW - 1) / kTileW;
    a.tiles = a.tilesX * ((c.h + kTileH - 1) / kTileH); // < 2^24 for 16-bit frame sizes
    t_LastError.clear();
    static_assert(offsetof(NrdHipCoverageReport, firstHole) == 4 * 5, "ResetCoverageReportKernel: five counters, then the two minima");
    hipLaunchKernelGGL(ResetCoverageReportKernel, dim3(1), dim3(64), 0, (hipStream_t)hipStream, (uint32_t*)deviceReport);
    const int blocks = (a.tiles + kGroups - 1) / kGroups;
    const dim3 grid((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), block(256 * kGroups);
    if (d->area == 1u)
        hipLaunchKernelGGL(HitDistCoverageKernel<1>, grid, block, 0, (hipStream_t)hipStream, a, (uint32_t*)deviceReport);
    else
        hipLaunchKernelGGL(HitDistCoverageKernel<2>, grid, block, 0, (hipStream_t)hipStream, a, (uint32_t*)deviceReport);
    return hipGetLastError() == hipSuccess ? (uint32_t)nrd::Result::SUCCESS : Fail(nrd::Result::FAILURE, std::string(entry) + ": the kernel launch failed");
}
