// fp64 matrix-core issue ceiling on this box (the yardstick of csrc/grf_expm.hip):
// back-to-back v_mfma_f64_16x16x4_f64 on 8 independent accumulators, one workgroup of 256 * wps lanes per CU, i.e.
// wps waves on every SIMD.  Every wave stamps the shader clock around its loop; cycles per MFMA per SIMD = the
// median workgroup's longest stamp / (MFMAs per wave * wps).  One MFMA is 16 * 16 * 4 * 2 = 2048 flops, so the
// chip's rate is 2048 / cycles * 4 SIMDs * CUs * clock, taken from the wall time of the same launch.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/mfma_f64_ceiling tools/mfma_f64_ceiling.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));

__global__ void mfma_kernel(unsigned long long *stamps, double *out, int iters, double seed) {
    f64x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double a = seed * (threadIdx.x & 15), b = seed * (threadIdx.x >> 4);
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if ((threadIdx.x & 63) == 0) stamps[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
        fprintf(stderr, "mfma_f64_ceiling: no GPU\n");
        return 1;
    }
    const int cus = prop.multiProcessorCount, iters = 4000;
    double *out;
    unsigned long long *stamps;
    hipMalloc(&out, (size_t)cus * 1024 * sizeof(double));
    hipMalloc(&stamps, (size_t)cus * 16 * sizeof(unsigned long long));
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    std::vector<unsigned long long> h((size_t)cus * 16);
    printf("v_mfma_f64_16x16x4_f64, %d CUs\n", cus);
    printf("wps  cycles_per_mfma_per_SIMD(median WG)  wall_ms  TFLOPs(wall)\n");
    for (int wps = 1; wps <= 2; ++wps) {
        const int threads = 256 * wps;
        for (int rep = 0; rep < 3; ++rep) {
            hipEventRecord(e0);
            mfma_kernel<<<cus, threads>>>(stamps, out, iters, 1e-3);
            hipEventRecord(e1);
            hipEventSynchronize(e1);
            if (rep == 0) continue;
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            hipMemcpy(h.data(), stamps, (size_t)cus * 4 * wps * sizeof(unsigned long long), hipMemcpyDeviceToHost);
            std::vector<double> per_wg(cus);
            for (int g = 0; g < cus; ++g) {
                unsigned long long mx = 0;
                for (int w = 0; w < 4 * wps; ++w) mx = std::max(mx, h[(size_t)g * 4 * wps + w]);
                per_wg[g] = (double)mx;
            }
            std::sort(per_wg.begin(), per_wg.end());
            const double mfmas = (double)iters * 32.0;
            const double flops = mfmas * 2048.0 * 4.0 * wps * cus;
            printf("%d  %8.3f  %8.3f  %8.2f\n", wps, per_wg[cus / 2] / (mfmas * wps), ms, flops / (ms * 1e-3) / 1e12);
        }
    }
    hipFree(out);
    hipFree(stamps);
    return 0;
}
