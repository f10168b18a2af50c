// TEST INFRASTRUCTURE -- the host-only sharding planner (csrc/host/halo_plan.cpp) as a stand-alone program: tests/test_halo_plan_host.py links it from csrc/host/*.cpp alone
// (no HIP runtime: the link is the proof that planning needs no device) under AddressSanitizer + UndefinedBehaviorSanitizer and holds what it prints against
// tests/golden/halo_plans.json.
//
// usage: halo_plan_host <cases file>, a token stream:
//   case <nrd::Denoiser> <height> <maxMotionRows> <exchangeThreshold> <frames> <world> <world + 1 strip bounds>
//   followed per frame by: <nrd::CommonSettings bytes, hex> <denoiser settings bytes, hex>
// Prints one JSON document: per case, per frame the reach list and per rank the plan, as in the golden file. Every rank is planned twice: with no room for steps and items
// (INVALID_ARGUMENT + the sizes needed), then with arrays of exactly those sizes; rank 0 once more with arrays one element short; and every frame once with world = 1.
#include "NRD.h"
#include "NRDHip.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

static std::vector<uint8_t> FromHex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++)
        out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}

#define CHECK(cond) \
    do { \
        if (!(cond)) { \
            fprintf(stderr, "halo_plan_host.cpp:%d: %s\n", __LINE__, #cond); \
            return 1; \
        } \
    } while (0)

template <typename T> static void PrintList(const std::vector<T>& v) {
    printf("[");
    for (size_t i = 0; i < v.size(); i++)
        printf("%s%d", i ? "," : "", (int)v[i]);
    printf("]");
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream in(argv[1]);
    CHECK(in.good());
    const uint32_t kSuccess = (uint32_t)nrd::Result::SUCCESS, kInvalid = (uint32_t)nrd::Result::INVALID_ARGUMENT;
    std::string word;
    bool firstCase = true;
    printf("[");
    while (in >> word) {
        CHECK(word == "case");
        uint32_t denoiser, height, maxMotionRows, exchangeThreshold, frames, world;
        CHECK(in >> denoiser >> height >> maxMotionRows >> exchangeThreshold >> frames >> world);
        std::vector<uint32_t> bounds(world + 1);
        for (uint32_t& b : bounds)
            CHECK(in >> b);

        const nrd::DenoiserDesc denoiserDesc = {0, (nrd::Denoiser)denoiser};
        nrd::InstanceCreationDesc creation = {};
        creation.denoisers = &denoiserDesc;
        creation.denoisersNum = 1;
        nrd::Instance* instance = nullptr;
        CHECK(nrd::CreateInstance(creation, instance) == nrd::Result::SUCCESS && instance);

        printf("%s[", firstCase ? "" : ",\n");
        firstCase = false;
        for (uint32_t f = 0; f < frames; f++) {
            std::string commonHex, settingsHex;
            CHECK(in >> commonHex >> settingsHex);
            const std::vector<uint8_t> commonBytes = FromHex(commonHex), settingsBytes = FromHex(settingsHex);
            nrd::CommonSettings common;
            CHECK(commonBytes.size() == sizeof(common));
            memcpy(&common, commonBytes.data(), sizeof(common));
            CHECK(nrd::SetDenoiserSettings(*instance, 0, settingsBytes.data()) == nrd::Result::SUCCESS);
            CHECK(nrd::SetCommonSettings(*instance, common) == nrd::Result::SUCCESS);
            const nrd::Identifier identifier = 0;
            const nrd::DispatchDesc* descs = nullptr;
            uint32_t num = 0;
            CHECK(nrd::GetComputeDispatches(*instance, &identifier, 1, descs, num) == nrd::Result::SUCCESS && num);

            std::vector<int32_t> reach(num);
            CHECK(nrdHipGetDispatchReach(instance, descs, num, reach.data()) == kSuccess);
            CHECK(nrdHipGetDispatchReach(instance, descs, num, nullptr) == kInvalid);
            printf("%s{\"reach\":", f ? "," : "");
            PrintList(reach);

            // one rank: nothing to exchange, the whole frame
            {
                const uint32_t whole[2] = {0, height};
                std::vector<int32_t> rowBegin(num), rowEnd(num);
                NrdHipHaloPlanInfo info = {};
                CHECK(nrdHipPlanHaloExchange(instance, descs, num, whole, 1, 0, height, maxMotionRows, exchangeThreshold, rowBegin.data(), rowEnd.data(), nullptr, 0, nullptr, 0, &info) == kSuccess);
                CHECK(info.fallback == 1 && info.stepsNum == 0 && info.itemsNum == 0);
                for (uint32_t i = 0; i < num; i++)
                    CHECK(rowBegin[i] == -1 && rowEnd[i] == (int32_t)height);
                CHECK(nrdHipPlanHaloExchange(instance, descs, num, whole, 1, 1, height, maxMotionRows, exchangeThreshold, rowBegin.data(), rowEnd.data(), nullptr, 0, nullptr, 0, &info) == kInvalid); // rank >= world
            }

            printf(",\"ranks\":[");
            for (uint32_t rank = 0; rank < world; rank++) {
                std::vector<int32_t> rowBegin(num), rowEnd(num);
                NrdHipHaloPlanInfo info = {};
                uint32_t r = nrdHipPlanHaloExchange(instance, descs, num, bounds.data(), world, rank, height, maxMotionRows, exchangeThreshold, rowBegin.data(), rowEnd.data(), nullptr, 0, nullptr, 0,
                    &info);
                CHECK(r == (info.fallback ? kSuccess : kInvalid)); // a sharded plan has at least one step: no room for it
                CHECK(info.fallback || info.stepsNum);
                std::vector<NrdHipHaloStep> steps(info.stepsNum);
                std::vector<NrdHipHaloItem> items(info.itemsNum);
                if (rank == 0 && !info.fallback) { // one element short
                    std::vector<NrdHipHaloStep> fewer(info.stepsNum - 1);
                    NrdHipHaloPlanInfo again = {};
                    CHECK(nrdHipPlanHaloExchange(instance, descs, num, bounds.data(), world, rank, height, maxMotionRows, exchangeThreshold, rowBegin.data(), rowEnd.data(), fewer.data(),
                              (uint32_t)fewer.size(), items.data(), (uint32_t)items.size(), &again) == kInvalid);
                    CHECK(again.stepsNum == info.stepsNum && again.itemsNum == info.itemsNum);
                }
                NrdHipHaloPlanInfo exact = {};
                CHECK(nrdHipPlanHaloExchange(instance, descs, num, bounds.data(), world, rank, height, maxMotionRows, exchangeThreshold, rowBegin.data(), rowEnd.data(), steps.data(),
                          (uint32_t)steps.size(), items.data(), (uint32_t)items.size(), &exact) == kSuccess);
                CHECK(exact.fallback == info.fallback && exact.stepsNum == info.stepsNum && exact.itemsNum == info.itemsNum);

                printf("%s{\"fallback\":%s,\"steps\":[", rank ? "," : "", exact.fallback ? "true" : "false");
                std::vector<uint32_t> early;
                for (size_t s = 0; s < steps.size(); s++) {
                    const NrdHipHaloStep& st = steps[s];
                    CHECK(st.firstItem + st.itemCount <= items.size());
                    printf("%s[[", s ? "," : "");
                    for (uint32_t k = st.firstItem; k < st.firstItem + st.itemCount; k++)
                        printf("%s[[%u,%u],%u]", k > st.firstItem ? "," : "", items[k].resourceType, items[k].indexInPool, items[k].widthRows);
                    printf("],%u,%u]", st.firstDispatch, st.dispatchCount);
                    early.push_back(st.earlyCount);
                }
                printf("],\"early\":");
                PrintList(early);
                printf(",\"row_begin\":");
                PrintList(rowBegin);
                printf(",\"row_end\":");
                PrintList(rowEnd);
                printf("}");
            }
            printf("]}");
        }
        printf("]");
        nrd::DestroyInstance(*instance);
    }
    printf("]\n");
    return 0;
}
