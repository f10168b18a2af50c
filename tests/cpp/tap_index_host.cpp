// TEST PROGRAM (tests/test_tap_index_host.py) -- host only, no HIP: csrc/host/tap_index.h TapIndexAddressesAllPlanes on the cases of the file given as argv[1], one case
// per line: "w h n pitch0 bytes0 pitch1 bytes1 ...". Prints one 0 / 1 per case. For every case it accepts, the program also forms the index the way the kernel does
// (kernels_reblur_spatial.hip FetchTapGuidesFullRect, FR == 3: one fp32 fma of the integer-valued coordinates, one conversion) at the corners and along the last row and
// column of the plane and holds index * bytesPerTexel against y * pitch + x * bytesPerTexel in every plane: "bad_offsets" counts the disagreements.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../raytracingdenoiser_amd/csrc/host/tap_index.h"

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    FILE* fp = fopen(argv[1], "r");
    if (!fp)
        return 2;
    std::vector<int> verdicts;
    uint64_t checked = 0, bad = 0;
    int w, h, n;
    while (fscanf(fp, "%d %d %d", &w, &h, &n) == 3) {
        std::vector<uint32_t> pitch(n), bytes(n);
        for (int i = 0; i < n; i++)
            if (fscanf(fp, "%u %u", &pitch[i], &bytes[i]) != 2)
                return 3;
        const bool ok = nrdhip::TapIndexAddressesAllPlanes(w, h, pitch.data(), bytes.data(), (uint32_t)n);
        verdicts.push_back(ok ? 1 : 0);
        if (!ok)
            continue;
        const float pitchInTexels = float(pitch[0] / bytes[0]);
        auto check = [&](int x, int y) {
            const uint32_t index = (uint32_t)std::fmaf(float(y), pitchInTexels, float(x));
            for (int i = 0; i < n; i++, checked++)
                bad += (uint64_t)index * bytes[i] != (uint64_t)y * pitch[i] + (uint64_t)x * bytes[i];
        };
        for (int x = 0; x < w; x++)
            check(x, 0), check(x, h - 1), check(x, h / 2);
        for (int y = 0; y < h; y++)
            check(0, y), check(w - 1, y), check(w / 2, y);
    }
    fclose(fp);
    printf("{\"tap_index\": [");
    for (size_t i = 0; i < verdicts.size(); i++)
        printf("%s%d", i ? ", " : "", verdicts[i]);
    printf("], \"offsets_checked\": %llu, \"bad_offsets\": %llu}\n", (unsigned long long)checked, (unsigned long long)bad);
    return 0;
}
