// TEST INFRASTRUCTURE -- the one reader of a dispatch list (csrc/host/dispatch_list.cpp) as a stand-alone program: tests/test_dispatch_list_host.py links it from csrc/host/*.cpp
// alone (no HIP runtime) under AddressSanitizer + UndefinedBehaviorSanitizer and holds what it prints against values computed from the settings it wrote.
//
// usage: dispatch_list_host <cases file>, a token stream:
//   case <mutation> <n> <n nrd::Denoiser values>      mutation: 0 none, 1 empty list, 2 first family block nulled, 3 first family block one byte short
//   followed by: <nrd::CommonSettings bytes, hex> <n denoiser settings, bytes, hex>
// Prints one JSON document: per case the scan of the instance's dispatch list. A shortened block lives in a heap allocation of exactly its stated size, so a read past it is
// a sanitizer report.
#include "NRD.h"

#include "../../raytracingdenoiser_amd/csrc/host/dispatch_list.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace nrdhip;

static std::vector<uint8_t> FromHex(const std::string& s) {
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); i++)
        out[i] = (uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return out;
}

#define CHECK(cond) \
    do { \
        if (!(cond)) { \
            fprintf(stderr, "dispatch_list_host.cpp:%d: %s\n", __LINE__, #cond); \
            return 1; \
        } \
    } while (0)

static void PrintSlots(const char* key, const bool* flags) {
    printf(",\"%s\":[", key);
    bool any = false;
    for (size_t t = 0; t < kUserSlots; t++)
        if (flags[t]) {
            printf("%s%d", any ? "," : "", (int)t);
            any = true;
        }
    printf("]");
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    std::ifstream in(argv[1]);
    CHECK(in.good());
    std::string word;
    bool firstCase = true;
    printf("[");
    while (in >> word) {
        CHECK(word == "case");
        uint32_t mutation, n;
        CHECK(in >> mutation >> n);
        std::vector<nrd::DenoiserDesc> denoisers(n);
        for (uint32_t k = 0; k < n; k++) {
            uint32_t denoiser;
            CHECK(in >> denoiser);
            denoisers[k] = {k, (nrd::Denoiser)denoiser};
        }
        nrd::InstanceCreationDesc creation = {};
        creation.denoisers = denoisers.data();
        creation.denoisersNum = n;
        nrd::Instance* instance = nullptr;
        CHECK(nrd::CreateInstance(creation, instance) == nrd::Result::SUCCESS && instance);

        std::string commonHex;
        CHECK(in >> commonHex);
        const std::vector<uint8_t> commonBytes = FromHex(commonHex);
        nrd::CommonSettings common;
        CHECK(commonBytes.size() == sizeof(common));
        memcpy(&common, commonBytes.data(), sizeof(common));
        std::vector<nrd::Identifier> identifiers(n);
        for (uint32_t k = 0; k < n; k++) {
            std::string settingsHex;
            CHECK(in >> settingsHex);
            CHECK(nrd::SetDenoiserSettings(*instance, k, FromHex(settingsHex).data()) == nrd::Result::SUCCESS);
            identifiers[k] = k;
        }
        const nrd::DispatchDesc* list = nullptr;
        uint32_t num = 0;
        for (int frame = 0; frame < 2; frame++) { // (the first list of an instance also holds the Clear_ passes of a history restart; the second is a frame like any other)
            CHECK(nrd::SetCommonSettings(*instance, common) == nrd::Result::SUCCESS);
            CHECK(nrd::GetComputeDispatches(*instance, identifiers.data(), n, list, num) == nrd::Result::SUCCESS && num);
        }
        const nrd::InstanceDesc& idesc = nrd::GetInstanceDesc(*instance);

        std::vector<nrd::DispatchDesc> descs(list, list + num);
        std::vector<uint8_t> shortBlock;
        int mutated = -1;
        if (mutation == 1)
            descs.clear();
        // (the mutations are applied to REBLUR lists; the pass is found by its name here, not by the code under test)
        for (uint32_t i = 0; i < (uint32_t)descs.size() && mutation >= 2 && mutated < 0; i++)
            if (!strncmp(idesc.pipelines[descs[i].pipelineIndex].shaderFileName, "REBLUR_", 7) && descs[i].constantBufferData) {
                mutated = (int)i;
                if (mutation == 2)
                    descs[i].constantBufferData = nullptr;
                else {
                    const size_t need = sizeof(nrdc::ReblurConstants); // one byte short of the family's shared block
                    CHECK(descs[i].constantBufferDataSize >= need);
                    shortBlock.assign((const uint8_t*)descs[i].constantBufferData, (const uint8_t*)descs[i].constantBufferData + need - 1);
                    shortBlock.shrink_to_fit();
                    descs[i].constantBufferData = shortBlock.data();
                    descs[i].constantBufferDataSize = (uint32_t)shortBlock.size();
                }
            }
        CHECK(mutation < 2 || mutated >= 0);

        std::vector<uint8_t> binds(descs.size());
        const ListScan s = ScanDispatchList(idesc, descs.data(), (uint32_t)descs.size(), binds.data());
        const ListScan again = ScanDispatchList(idesc, descs.data(), (uint32_t)descs.size()); // without the per-dispatch array
        CHECK(again.bindsNormalRoughness == nullptr && again.first == s.first && again.slotsNum == s.slotsNum && again.reblur == s.reblur && again.relax == s.relax);

        // the dispatch whose block the scan took first (REFERENCE: the scan keeps the rect only; its first copy pass)
        const void* firstBlock = s.first == Family::REBLUR ? (const void*)s.reblur : s.first == Family::RELAX ? (const void*)s.relax : (const void*)s.sigma;
        int firstBlockDispatch = -1;
        for (uint32_t i = 0; i < (uint32_t)descs.size() && firstBlockDispatch < 0; i++)
            if (s.first == Family::REFERENCE ? !strcmp(ShaderOf(idesc, descs[i]), "REFERENCE_Copy.cs") : (firstBlock && descs[i].constantBufferData == firstBlock))
                firstBlockDispatch = (int)i;
        // the typed view and the rect offsets agree with the scan on every dispatch
        for (const nrd::DispatchDesc& d : descs) {
            size_t oo = 0, of = 0;
            const Family f = FamilyOf(ShaderOf(idesc, d));
            const char* shader = ShaderOf(idesc, d);
            const bool typed = ConstantsAs<nrdc::ReblurConstants>(Family::REBLUR, shader, d.constantBufferData, d.constantBufferDataSize) ||
                               ConstantsAs<nrdc::RelaxConstants>(Family::RELAX, shader, d.constantBufferData, d.constantBufferDataSize) ||
                               ConstantsAs<nrdc::SigmaConstants>(Family::SIGMA, shader, d.constantBufferData, d.constantBufferDataSize);
            CHECK(!typed || (f != Family::NONE && f != Family::REFERENCE));
            CHECK(!typed || RectOriginOffsets(shader, d.constantBufferDataSize, oo, of));
            CHECK(!ConstantsAs<nrdc::ReblurConstants>(Family::RELAX, shader, d.constantBufferData, d.constantBufferDataSize) || f == Family::RELAX); // the family asked for decides
        }

        printf("%s{\"num\":%u,\"first\":%d,\"first_with_origin\":%d,\"has\":[%d,%d,%d,%d]", firstCase ? "" : ",\n", (uint32_t)descs.size(), (int)s.first, (int)s.firstWithOrigin, s.reblur != nullptr,
            s.relax != nullptr, s.sigma != nullptr, s.first == Family::REFERENCE);
        firstCase = false;
        printf(",\"rect\":[%d,%d],\"origin\":[%d,%d]", s.rectW, s.rectH, s.originX, s.originY);
        printf(",\"view_z_scale\":%.9g,\"denoising_range\":%.9g,\"frame_index\":%u,\"cells\":[%u,%u]", s.viewZScale, s.denoisingRange, s.frameIndex, s.diffCell, s.specCell);
        PrintSlots("named", s.named);
        PrintSlots("read", s.read);
        PrintSlots("written", s.written);
        PrintSlots("outside_reblur", s.namedOutsideReblur);
        printf(",\"slots\":[");
        for (uint32_t k = 0; k < s.slotsNum; k++)
            printf("%s%d", k ? "," : "", (int)s.slots[k]);
        printf("],\"binds_normal_roughness\":[");
        for (size_t i = 0; i < binds.size(); i++)
            printf("%s%d", i ? "," : "", (int)binds[i]);
        printf("],\"families\":[");
        for (size_t i = 0; i < descs.size(); i++)
            printf("%s%d", i ? "," : "", (int)FamilyOf(ShaderOf(idesc, descs[i])));
        printf("],\"shaders\":[");
        for (size_t i = 0; i < descs.size(); i++)
            printf("%s\"%s\"", i ? "," : "", ShaderOf(idesc, descs[i]));
        printf("],\"first_block_dispatch\":%d,\"mutated_dispatch\":%d}", firstBlockDispatch, mutated);
        nrd::DestroyInstance(*instance);
    }
    printf("]\n");
    return 0;
}
