// Test infrastructure: NRD_FrontEnd_PackNormalAndRoughness + NRD_StoreNormalRoughnessTexel of include/NRD.hip.h on the HOST, in the G-buffer encoding this file is compiled for
// (-DNRD_NORMAL_ENCODING / -DNRD_ROUGHNESS_ENCODING), over samples read from a file: the whole texel, all 32 or 64 bits, which tests/cpp/frontend_check's dump holds only half of.
// usage: pack_texels IN OUT   IN: float32 rows (N.x, N.y, N.z, roughness, materialID); OUT: one uint64 per row (a 32-bit texel zero-extended)
#include "NRD.hip.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3)
        return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out)
        return 3;
    float row[5];
    size_t n = 0;
    while (fread(row, sizeof(float), 5, in) == 5) {
        const uint64_t texel = (uint64_t)NRD_StoreNormalRoughnessTexel(NRD_FrontEnd_PackNormalAndRoughness(make_float3(row[0], row[1], row[2]), row[3], row[4]));
        fwrite(&texel, sizeof(texel), 1, out);
        n++;
    }
    fclose(in);
    fclose(out);
    printf("packed %zu texels of %zu bits\n", n, sizeof(NRD_NormalRoughnessTexel) * 8);
    return 0;
}
