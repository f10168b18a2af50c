// Test infrastructure: NRD_SG_ReJitter of include/NRD.hip.h over stencil rows that the TEST assembled from its planes (tests/test_rejitter_checkerboard.py), on the host
// (--host) or on the device, one thread per row (--device) -- the expectation of the re-jitter kernel that does not come from the library. N and the roughness of a texel
// are the header's own unpack of its packed word, in the G-buffer encoding this file is compiled for (-DNRD_NORMAL_ENCODING / -DNRD_ROUGHNESS_ENCODING).
// usage: rejitter_rows --host|--device IN OUT
//   IN : rows of 38 32-bit words: diffuse SH0, SH1, specular SH0, SH1 (4 floats each), Rf0 (3), V (3), Z, Ze, Zw, Zn, Zs, one word of padding, then the IN_NORMAL_ROUGHNESS
//        texels of the pixel and of its e, w, n, s neighbours as five uint64 (a 32-bit texel zero-extended); a neighbour outside the plane is an all-zero texel with Z = 0
//   OUT: two floats per row: the diffuse and the specular scale
#include <hip/hip_runtime.h>

#include "NRD.hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

constexpr int kWords = 38;

__host__ __device__ inline float2 EvalRow(const uint32_t* row) {
    const float* f = (const float*)row;
    const NRD_SG diffSg = REBLUR_BackEnd_UnpackSh(make_float4(f[0], f[1], f[2], f[3]), make_float4(f[4], f[5], f[6], f[7]));
    const NRD_SG specSg = REBLUR_BackEnd_UnpackSh(make_float4(f[8], f[9], f[10], f[11]), make_float4(f[12], f[13], f[14], f[15]));
    float4 nr[5];
    for (int k = 0; k < 5; k++) {
        const uint64_t texel = (uint64_t)row[28 + 2 * k] | ((uint64_t)row[29 + 2 * k] << 32);
        nr[k] = NRD_FrontEnd_UnpackNormalAndRoughness(NRD_LoadNormalRoughnessTexel((NRD_NormalRoughnessTexel)texel));
    }
    auto n3 = [&](int k) { return make_float3(nr[k].x, nr[k].y, nr[k].z); };
    return NRD_SG_ReJitter(diffSg, specSg, make_float3(f[16], f[17], f[18]), make_float3(f[19], f[20], f[21]), nr[0].w, f[22], f[23], f[24], f[25], f[26], n3(0), n3(1), n3(2), n3(3), n3(4));
}

__global__ void EvalRows(const uint32_t* rows, float2* out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count)
        out[i] = EvalRow(rows + (size_t)i * kWords);
}

#define HIP_OK(x)                                                              \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess) {                                                \
            printf("%s failed: %s\n", #x, hipGetErrorString(e_));              \
            return 4;                                                          \
        }                                                                      \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "--host") && strcmp(argv[1], "--device")))
        return 2;
    const bool device = !strcmp(argv[1], "--device");
    FILE* in = fopen(argv[2], "rb");
    if (!in)
        return 3;
    std::vector<uint32_t> rows;
    uint32_t row[kWords];
    while (fread(row, 4, kWords, in) == (size_t)kWords)
        rows.insert(rows.end(), row, row + kWords);
    fclose(in);
    const size_t count = rows.size() / kWords;
    std::vector<float2> host(count), result(count);
    for (size_t i = 0; i < count; i++)
        host[i] = EvalRow(rows.data() + i * kWords);
    result = host;
    if (device && count) {
        uint32_t* dRows = nullptr;
        float2* dOut = nullptr;
        HIP_OK(hipMalloc((void**)&dRows, rows.size() * 4));
        HIP_OK(hipMalloc((void**)&dOut, count * sizeof(float2)));
        HIP_OK(hipMemcpy(dRows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(EvalRows, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, dRows, dOut, (uint32_t)count);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(result.data(), dOut, count * sizeof(float2), hipMemcpyDeviceToHost));
        HIP_OK(hipFree(dRows));
        HIP_OK(hipFree(dOut));
        double worst = 0.0;
        for (size_t i = 0; i < count; i++)
            worst = fmax(worst, fmax(fabs((double)result[i].x - host[i].x), fabs((double)result[i].y - host[i].y)));
        printf("host vs device maximum difference %g\n", worst);
    }
    FILE* out = fopen(argv[3], "wb");
    if (!out)
        return 3;
    fwrite(result.data(), sizeof(float2), count, out);
    fclose(out);
    printf("rejitter rows %zu (%s)\n", count, device ? "device" : "host");
    return 0;
}
