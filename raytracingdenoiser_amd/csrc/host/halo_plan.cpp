// The host-only planning of multi-GPU row-strip sharding (include/NRDHip.h): how many rows each pass reads around a pixel (the reach model), which rows each pass of a
// rank has to produce, and which bands of which planes the ranks exchange in front of which pass. Plain C++ over the dispatch list: no device, no HIP header -- so the
// file also builds into a stand-alone host program (tests/cpp/halo_plan_host.cpp runs it under the sanitizers).
#include "halo_plan.h"

#include "NRDHip.h"

#include "dispatch_list.h" // FamilyOf, ConstantsAs: the family tests and the typed views of the constant blocks

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

using nrdhip::ConstantsAs;
using nrdhip::Family;
using nrdhip::ShaderOf;

// Rows a tap of REBLUR's Blur / PostBlur can lie from its pixel (kernels_reblur_spatial.hip; reference REBLUR_Common_SpatialFilter.hlsli):
//   diffuse taps: screen space, |offset| <= blurRadius * skew with skew <= 1 and blurRadius = max( scale * maxBlurRadius * sqrt( areaFactor <= 1 ), minBlurRadius );
//   specular taps: a ring in WORLD space with the half-axes worldRadius * skewFactor and worldRadius / skewFactor, worldRadius = blurRadius * unproject * viewZ (the ring's size
//     in pixels at the pixel's own depth), skewFactor >= 0.25 + 0.75 * roughness, and blurRadius <= scale * maxBlurRadius * sqrt( roughness ) unless the minimum radius wins:
//       scale * maxBlurRadius * sqrt( r ) / ( 0.25 + 0.75 r ) <= 1.1547 * scale * maxBlurRadius (at r = 1 / 3),   minBlurRadius / ( 0.25 + 0.75 r ) <= 4 * minBlurRadius (r = 0);
//     projected, a world offset L at depth z lands L / ( unproject * z_tap ) pixels away with z_tap >= z - L: a factor 1 / ( 1 - t ), t = L / z = ringPixels * unproject, the tangent
//     of the ring's angular radius. A ring half as large as its distance (tiny frames with huge radii) has no useful bound: -1 = whole frame.
// + 2: the bilinear footprint of a tap and the rounding of its position. (Rounds 2-5 declared 2 x max( scale * maxBlurRadius, minBlurRadius ) + 2: 62 / 122 rows at the default
// radius of 30 where the bound is 39 / 79 -- most of the redundant rows of the 8-rank plan, VERDICT r05 item 5a -- and too FEW rows where the minimum radius dominates: 4 x, not 2 x.)
// NRD_HIP_SPECULAR_REACH_SLACK scales the bound (experiments; tests/test_sharding.py under-declares with it to show that its poisoned-halo check fires).
static int ReblurBlurReachRows(float scaledMaxRadius, float minRadius, float unproject) {
    static const float kScale = getenv("NRD_HIP_SPECULAR_REACH_SLACK") ? std::fmax(0.05f, (float)atof(getenv("NRD_HIP_SPECULAR_REACH_SLACK"))) : 1.0f;
    const float diffuse = std::fmax(scaledMaxRadius, minRadius);
    const float ring = std::fmax(1.1547006f * scaledMaxRadius, 4.0f * minRadius);
    const float t = ring * unproject;
    if (!(t < 0.5f))
        return -1;
    return (int)std::ceil(kScale * std::fmax(diffuse, ring / (1.0f - t))) + 2;
}

// Rows of its INPUT planes (produced earlier in the same frame) a pass reads around an output row. -1 = unknown pass: it and
// everything before it run on the whole frame.
static int PassReachRows(const char* shader, const void* constants, uint32_t constantsSize) {
    if (!strncmp(shader, "Clear_", 6))
        return 0; // the clears of a restart frame: texel-local (the launch covers the whole plane on every rank, which is what a single GPU's plane holds afterwards)
    if (const nrdc::RelaxConstants* relax = ConstantsAs<nrdc::RelaxConstants>(Family::RELAX, shader, constants, constantsSize)) {
        const nrdc::RelaxConstants& c = *relax;
        if (c.gRectSizePrev.x != float(c.gRectSize.x) || c.gRectSizePrev.y != float(c.gRectSize.y))
            return -1; // dynamic resolution step: history rows map to different rows of this frame, no bounded halo -> whole frame
        if (strstr(shader, "_AtrousSmem") || strstr(shader, "_HistoryClamping"))
            return 2; // 5x5 windows
        if (strstr(shader, "_Atrous")) {
            const nrdc::RelaxAtrousConstants* atrous = ConstantsAs<nrdc::RelaxAtrousConstants>(Family::RELAX, shader, constants, constantsSize);
            if (!atrous)
                return -1;
            const uint32_t step = atrous->gStepSize;
            return (int)(step + (step > 4 ? (step + 3) / 4 : 0)); // +-step taps, shifted by up to step / 4 at the large steps
        }
        if (strstr(shader, "_HistoryFix"))
            return 2 * (int)std::floor(c.gHistoryFixBasePixelStride / 2.0f + 0.5f); // 5x5 taps at stride <= base / (1 + 1)
        if (strstr(shader, "_TemporalAccumulation") || strstr(shader, "_AntiFirefly"))
            return 1;
        if (strstr(shader, "_PrePass") || strstr(shader, "_SplitScreen") || strstr(shader, "ClassifyTiles") || strstr(shader, "_HitDistReconstruction") || strstr(shader, "_Copy"))
            return 0; // read user inputs only (the pre-pass behind a reconstruction pass: DispatchReachRows) / copy texel to texel (the copy's launch covers the whole plane: a superset)
        return -1;
    }
    if (const nrdc::SigmaConstants* sigma = ConstantsAs<nrdc::SigmaConstants>(Family::SIGMA, shader, constants, constantsSize)) {
        // round 6. Blur / PostBlur: screen-space taps at <= SIGMA_MAX_PIXEL_RADIUS = 32 pixels (skew <= 1; reference SIGMA_Common.hlsli:21-33, SIGMA_Config.hlsli:34),
        // snapped to a texel centre (+ 1), around the 5x5 radius-estimation window (2); TemporalStabilization: 5x5 moments. The tile passes write down-sampled planes (every rank
        // runs them on the whole frame: nrdHipPlanHaloExchange); Copy and SplitScreen work texel to texel.
        const nrdc::SigmaConstants& c = *sigma;
        if (c.gRectSizePrev.x != c.gRectSize.x || c.gRectSizePrev.y != c.gRectSize.y)
            return -1;
        if (strstr(shader, "_PostBlur") || strstr(shader, "_Blur"))
            return 32 + 1 + 2;
        if (strstr(shader, "_TemporalStabilization"))
            return 2;
        if (strstr(shader, "ClassifyTiles") || strstr(shader, "SmoothTiles") || strstr(shader, "_Copy") || strstr(shader, "_SplitScreen"))
            return 0;
        return -1;
    }
    const nrdc::ReblurConstants* reblur = ConstantsAs<nrdc::ReblurConstants>(Family::REBLUR, shader, constants, constantsSize);
    if (!reblur)
        return -1;
    const nrdc::ReblurConstants& c = *reblur;
    if (c.gRectSizePrev.x != c.gRectSize.x || c.gRectSizePrev.y != c.gRectSize.y)
        return -1; // dynamic resolution step: history rows map to different rows of this frame, no bounded halo -> whole frame
    if (strstr(shader, "_TemporalStabilization"))
        return 1;
    if (strstr(shader, "_PostBlur"))
        return ReblurBlurReachRows(2.0f * c.gMaxBlurRadius, c.gMinBlurRadius, c.gUnproject); // REBLUR_POST_BLUR_RADIUS_SCALE = 2
    if (strstr(shader, "_Blur"))
        return ReblurBlurReachRows(c.gMaxBlurRadius, c.gMinBlurRadius, c.gUnproject);
    if (strstr(shader, "_HistoryFix"))
        return 2 * (int)std::floor(c.gHistoryFixBasePixelStride / 2.0f) + 4 + 2;
    if (strstr(shader, "_TemporalAccumulation"))
        return 1;
    if (strstr(shader, "_PrePass") || strstr(shader, "_SplitScreen") || strstr(shader, "ClassifyTiles") || strstr(shader, "_HitDistReconstruction"))
        return 0; // read user inputs only (the pre-pass behind a reconstruction pass: DispatchReachRows)
    return -1;
}

// Rows above / below a produced pixel at which dispatch i reads the per-frame GUIDE planes (decoded normals, view / world positions): PassReachRows, except for the
// pre-passes, whose taps read nothing written earlier in the frame (reach 0 for the halo plan) but do read the guides at blur-radius distance. -1 = unknown.
static int PrePassTapRows(const char* shader, const void* constants, uint32_t constantsSize);
int nrdhip::GuideReachRows(const char* shader, const void* constants, uint32_t constantsSize) {
    const int reach = PassReachRows(shader, constants, constantsSize);
    // TemporalAccumulation with a specular signal (REBLUR and RELAX): the curvature estimate's high-parallax tap reads the decoded normals smbParallaxInPixelsMin * (1 + gFramerateScale *
    // Bayer) pixels away along the motion direction (reference REBLUR_TemporalAccumulation.hlsli:398-420) -- many ROWS under vertical camera translation, and bounded by neither the
    // halo reach (1) nor the measured surface motion (a rotation can cancel the translation's parallax on screen). Unknown reach: the guide planes are decoded on the whole frame
    // (18 us more per 1440p frame at 8 ranks; ADVICE r04 -- the rows happened to be covered by the pre-pass's guide reach at the default radii, and by nothing without a pre-pass:
    // tests/test_sharding.py, the "_camera_rise" cases)
    if (reach >= 0 && strstr(shader, "_TemporalAccumulation") && strstr(shader, "Specular"))
        return -1;
    if (reach < 0 || !strstr(shader, "_PrePass"))
        return reach;
    return PrePassTapRows(shader, constants, constantsSize);
}

// Rows a tap of a pre-pass (REBLUR or RELAX) can lie from its pixel. Where they land on planes written earlier in the frame -- the output of a hit-distance reconstruction pass --
// this is the pass's reach for the halo plan (DispatchReachRows); it always is its reach on the per-frame guide planes (GuideReachRows).
static int PrePassTapRows(const char* shader, const void* constants, uint32_t constantsSize) {
    // the pre-pass taps of both families are SCREEN-space (REBLUR: skew 1 for diffuse, REBLUR_USE_SCREEN_SPACE_SAMPLING_FOR_SPECULAR in the pre-pass; RELAX: pixelUv + rotator *
    // blurRadius): the radius itself bounds them (rounds 2-5 doubled it)
    float radius;
    if (const nrdc::RelaxConstants* c = ConstantsAs<nrdc::RelaxConstants>(Family::RELAX, shader, constants, constantsSize))
        radius = std::fmax(c->gDiffBlurRadius, c->gSpecBlurRadius);
    else if (const nrdc::ReblurConstants* c = ConstantsAs<nrdc::ReblurConstants>(Family::REBLUR, shader, constants, constantsSize))
        radius = std::fmax(std::fmax(c->gDiffPrepassBlurRadius, c->gSpecPrepassBlurRadius), c->gMinBlurRadius);
    else
        return -1; // (not reached: both callers come here with a reach PassReachRows took from the same block)
    return (int)std::ceil(std::fmax(radius, 1.0f)) + 2; // (RELAX: a zero hit distance widens the radius to at least one pixel)
}

// PassReachRows of dispatch i in the context of its list: a pre-pass reads user inputs only (reach 0) UNLESS a hit-distance reconstruction pass ran in front of it -- then its taps
// gather from that pass's output, a full-resolution plane written earlier in the frame, at blur-radius distance (rounds 2-5 ran such frames unsharded).
static int DispatchReachRows(const nrd::InstanceDesc& idesc, const nrd::DispatchDesc* descs, uint32_t i) {
    const nrd::DispatchDesc& d = descs[i];
    const char* shader = ShaderOf(idesc, d);
    if (!*shader)
        return -1; // a pipeline the instance does not have
    const int reach = PassReachRows(shader, d.constantBufferData, d.constantBufferDataSize);
    if (reach != 0 || !strstr(shader, "_PrePass"))
        return reach;
    for (uint32_t r = 0; r < d.resourcesNum; r++) {
        const nrd::ResourceDesc& in = d.resources[r];
        if (in.descriptorType != nrd::DescriptorType::TEXTURE || (uint32_t)in.type < (uint32_t)nrd::ResourceType::OUT_DIFF_RADIANCE_HITDIST)
            continue; // a user input: complete on every rank
        for (uint32_t j = 0; j < i; j++)
            for (uint32_t w = 0; w < descs[j].resourcesNum; w++) {
                const nrd::ResourceDesc& out = descs[j].resources[w];
                if (out.descriptorType == nrd::DescriptorType::STORAGE_TEXTURE && out.type == in.type && out.indexInPool == in.indexInPool && strstr(ShaderOf(idesc, descs[j]), "_HitDistReconstruction"))
                    return PrePassTapRows(shader, d.constantBufferData, d.constantBufferDataSize);
            }
    }
    return reach;
}

// nrdHipSetOwnedRows: walk the list backwards accumulating the reach of the later passes
void nrdhip::OwnedRowRanges(const nrd::Instance& instance, const nrd::DispatchDesc* descs, uint32_t num, int ownedRowBegin, int ownedRowEnd, int32_t* rowBegin, int32_t* rowEnd) {
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(instance);
    int margin = 0;
    for (int i = (int)num - 1; i >= 0; i--) {
        rowBegin[i] = -1;
        rowEnd[i] = INT_MAX;
        const nrd::DispatchDesc& d = descs[i];
        int reach = DispatchReachRows(idesc, descs, i);
        if (reach < 0 || margin < 0) {
            margin = -1; // whole frame from here backwards
            continue;
        }
        if (!strncmp(ShaderOf(idesc, d), "SIGMA_Copy", 10))
            continue; // its output is last frame's history, which TemporalStabilization samples at the REPROJECTED position: the texel-to-texel copy (10 B/px) covers the whole frame, the margin walks on
        rowBegin[i] = std::max(ownedRowBegin - margin, 0);
        rowEnd[i] = ownedRowEnd == INT_MAX ? INT_MAX : ownedRowEnd + margin;
        margin += reach;
    }
}

extern "C" __attribute__((visibility("default"))) uint32_t nrdHipGetDispatchReach(void* instance, const void* dispatchDescs, uint32_t dispatchDescsNum, int32_t* reachRows) {
    if (!instance || (!dispatchDescs && dispatchDescsNum) || !reachRows)
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const nrd::DispatchDesc* descs = (const nrd::DispatchDesc*)dispatchDescs;
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*(nrd::Instance*)instance);
    for (uint32_t i = 0; i < dispatchDescsNum; i++) {
        reachRows[i] = DispatchReachRows(idesc, descs, i);
    }
    return (uint32_t)nrd::Result::SUCCESS;
}

// Halo-exchange plan of one dispatch list for one rank (include/NRDHip.h) -- THE planner: raytracingdenoiser_amd/sharding.py plan_halo_exchange and
// include/NRDShardedIntegrationHip.hpp both call it (tests/golden/halo_plans.json pins its plans). Segments start in front of every pass whose reach
// exceeds the threshold; margins accumulate backwards from 0 at each segment end; a plane read from an earlier segment (or carried over from the
// previous frame: widened by the motion bound) is exchanged in front of the reader's segment.
extern "C" __attribute__((visibility("default"))) uint32_t nrdHipPlanHaloExchange(void* instance, const void* dispatchDescs, uint32_t num, const uint32_t* stripBounds, uint32_t world, uint32_t rank,
    uint32_t height, uint32_t maxMotionRows, uint32_t exchangeThreshold, int32_t* rowBegin, int32_t* rowEnd, NrdHipHaloStep* steps, uint32_t stepsCapacity, NrdHipHaloItem* items,
    uint32_t itemsCapacity, NrdHipHaloPlanInfo* info) {
    if (!instance || (!dispatchDescs && num) || !info || !stripBounds || world == 0 || rank >= world || (num && (!rowBegin || !rowEnd)))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT;
    const nrd::DispatchDesc* descs = (const nrd::DispatchDesc*)dispatchDescs;
    const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*(nrd::Instance*)instance);
    *info = NrdHipHaloPlanInfo{};
    auto fallback = [&]() {
        info->fallback = 1;
        info->stepsNum = info->itemsNum = 0;
        for (uint32_t i = 0; i < num; i++) {
            rowBegin[i] = -1;
            rowEnd[i] = (int32_t)height;
        }
        return (uint32_t)nrd::Result::SUCCESS;
    };
    std::vector<int> reach(num);
    bool known = num != 0 && world > 1;
    for (uint32_t i = 0; i < num; i++) {
        reach[i] = DispatchReachRows(idesc, descs, i);
        known = known && reach[i] >= 0;
    }
    if (!known)
        return fallback();
    const int rb = (int)stripBounds[rank], re = (int)stripBounds[rank + 1];
    int per = INT_MAX; // a halo must fit into the neighbouring strips
    for (uint32_t r = 0; r < world; r++)
        per = std::min(per, (int)stripBounds[r + 1] - (int)stripBounds[r]);

    std::vector<uint32_t> starts(1, 0);
    for (uint32_t i = 1; i < num; i++)
        if (reach[i] > (int)exchangeThreshold)
            starts.push_back(i);
    std::vector<uint32_t> bounds(starts);
    bounds.push_back(num);
    std::vector<int> segOf(num), margins(num);
    for (size_t s = 0; s < starts.size(); s++) {
        int m = 0;
        for (int i = (int)bounds[s + 1] - 1; i >= (int)bounds[s]; i--) {
            segOf[i] = (int)s;
            margins[i] = m;
            m += reach[i];
        }
    }
    typedef std::pair<uint32_t, uint32_t> Key; // (resource type, index in pool)
    auto isUserInput = [](nrd::ResourceType t) { return (uint32_t)t < (uint32_t)nrd::ResourceType::OUT_DIFF_RADIANCE_HITDIST; };
    auto isSmall = [&](const Key& k) { // down-sampled pool planes (tile maps): complete on every rank, never exchanged
        if (k.first == (uint32_t)nrd::ResourceType::TRANSIENT_POOL)
            return k.second < idesc.transientPoolSize && idesc.transientPool[k.second].downsampleFactor != 1;
        if (k.first == (uint32_t)nrd::ResourceType::PERMANENT_POOL)
            return k.second < idesc.permanentPoolSize && idesc.permanentPool[k.second].downsampleFactor != 1;
        return false;
    };
    std::map<Key, int> lastWrite;
    std::set<Key> cleared; // planes a Clear_ pass of this list wrote (every texel, on every rank)
    std::map<std::pair<Key, int>, int> need; // (plane, writer index or -1) -> halo rows
    std::vector<char> wholeFrame(num, 0);
    for (uint32_t i = 0; i < num; i++) {
        const nrd::DispatchDesc& d = descs[i];
        std::vector<Key> reads, writes;
        bool writesSmall = false, writesLarge = false;
        for (uint32_t r = 0; r < d.resourcesNum; r++) {
            const nrd::ResourceDesc& res = d.resources[r];
            if (isUserInput(res.type))
                continue;
            const Key key((uint32_t)res.type, res.indexInPool);
            if (res.descriptorType == nrd::DescriptorType::TEXTURE) {
                if (!isSmall(key))
                    reads.push_back(key);
            } else {
                writes.push_back(key);
                (isSmall(key) ? writesSmall : writesLarge) = true;
            }
        }
        if (writesSmall) {
            wholeFrame[i] = 1;
            if (writesLarge || !reads.empty())
                return fallback(); // a tile-map pass that also touches full-resolution planes: not expected, stay safe
            continue;
        }
        for (const Key& key : reads) {
            auto it = lastWrite.find(key);
            const int w = it == lastWrite.end() ? -1 : it->second;
            // a plane written by SIGMA's Copy IS last frame's history (SIGMA_Copy.hlsli: previous output -> HISTORY, texel to texel): TemporalStabilization samples it at
            // the reprojected position, so its readers need the motion bound like readers of a carried-over plane
            const bool historyCopy = w >= 0 && !strncmp(ShaderOf(idesc, descs[w]), "SIGMA_Copy", 10);
            if (historyCopy && segOf[w] == segOf[i])
                return fallback(); // (never with the default threshold: Blur's reach starts a segment between the two)
            if (w >= 0 && segOf[w] == segOf[i]) {
                // produced in this segment with a sufficient margin -- where it was WRITTEN: every pass skips the sky, and a reader with a neighbourhood also reads the texels next
                // to the geometry that the writer left alone (they hold what the plane held at the end of the last frame -- on a rank only inside its strip). The rows of the
                // reader's neighbourhood outside the strip are therefore fetched from their owner at the frame start, before the writer runs (RELAX TemporalAccumulation takes the
                // specular hit distance of its 3x3 from the pre-pass output, sky or not: reference RELAX_TemporalAccumulation.hlsli:363, 433-450)
                if (reach[i] > 0 && !cleared.count(key)) { // (a plane cleared earlier in this frame holds zeros wherever nothing was written since: the same on every rank)
                    int& slot = need[std::make_pair(key, -1)];
                    slot = std::max(slot, margins[i] + reach[i]);
                }
                continue;
            }
            const int h = margins[i] + reach[i] + ((w < 0 || historyCopy) ? (int)maxMotionRows : 0);
            if (h > 0) {
                int& slot = need[std::make_pair(key, w)];
                slot = std::max(slot, h);
            }
        }
        const bool isClear = !strncmp(ShaderOf(idesc, d), "Clear_", 6);
        for (const Key& key : writes) {
            lastWrite[key] = (int)i;
            if (isClear)
                cleared.insert(key);
        }
    }
    for (const auto& kv : need)
        if (kv.second > per)
            return fallback(); // a halo would reach past the neighbouring strip

    std::vector<std::vector<NrdHipHaloItem>> exchanges(starts.size());
    for (const auto& kv : need) {
        const int w = kv.first.second;
        exchanges[w < 0 ? 0 : segOf[w] + 1].push_back(NrdHipHaloItem{kv.first.first.first, kv.first.first.second, (uint32_t)kv.second});
    }
    uint32_t itemsNum = 0;
    for (const auto& e : exchanges)
        itemsNum += (uint32_t)e.size();
    info->stepsNum = (uint32_t)starts.size();
    info->itemsNum = itemsNum;
    if (info->stepsNum > stepsCapacity || itemsNum > itemsCapacity || (info->stepsNum && !steps) || (itemsNum && !items))
        return (uint32_t)nrd::Result::INVALID_ARGUMENT; // info tells the capacities needed
    uint32_t cursor = 0;
    for (size_t s = 0; s < starts.size(); s++) {
        NrdHipHaloStep& st = steps[s];
        st.firstDispatch = bounds[s];
        st.dispatchCount = bounds[s + 1] - bounds[s];
        st.firstItem = cursor;
        st.itemCount = (uint32_t)exchanges[s].size();
        for (const NrdHipHaloItem& it : exchanges[s])
            items[cursor++] = it;
        // leading dispatches that touch none of the exchanged planes: they can run while the transfers are in flight
        st.earlyCount = 0;
        if (st.itemCount)
            for (uint32_t i = bounds[s]; i < bounds[s + 1]; i++) {
                bool touches = false;
                for (uint32_t r = 0; r < descs[i].resourcesNum && !touches; r++)
                    for (const NrdHipHaloItem& it : exchanges[s])
                        touches = touches || (it.resourceType == (uint32_t)descs[i].resources[r].type && it.indexInPool == descs[i].resources[r].indexInPool);
                if (touches)
                    break;
                st.earlyCount++;
            }
    }
    for (uint32_t i = 0; i < num; i++) {
        rowBegin[i] = wholeFrame[i] ? -1 : std::max(rb - margins[i], 0);
        rowEnd[i] = wholeFrame[i] ? (int32_t)height : std::min(re + margins[i], (int)height);
    }
    return (uint32_t)nrd::Result::SUCCESS;
}
