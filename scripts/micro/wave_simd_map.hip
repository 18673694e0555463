// wave_simd_map.hip -- which SIMD does each wave of a 1024-thread workgroup run on?
//
// The stagger of the 16-row scan roles (sfsn_scan3j_dev.h, SFSN_S3J_STAGGER) splits a SIMD's four waves by the slot wave >> 2, which
// assumes that waves w, w + 4, w + 8, w + 12 share SIMD w & 3.  Every wave of a few workgroups that fill a CU the way the scan does
// (1024 threads, 128 registers asked for through the LDS size instead: one workgroup per CU) writes HW_REG_HW_ID; the host prints, per
// workgroup, the SIMD of every wave (bits 5:4) and says whether the assumption holds.
//
// Build and run:  hipcc --offload-arch=gfx950 -O3 -o wave_simd_map.bin wave_simd_map.hip && ./wave_simd_map.bin
#include <hip/hip_runtime.h>
#include <cstdio>

constexpr int WGS = 8, WAVES = 16;

__global__ __launch_bounds__(1024) void wave_simd_kernel(unsigned* out) {
    extern __shared__ char lds[];  // (nearly all of a CU's LDS: one workgroup per CU, as in the scan launches)
    unsigned hw = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    if ((threadIdx.x & 63) == 0) out[blockIdx.x * WAVES + (threadIdx.x >> 6)] = hw;
}

int main() {
    unsigned* d = nullptr;
    unsigned h[WGS * WAVES];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 1;
    if (hipFuncSetAttribute((const void*)wave_simd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024) != hipSuccess) return 1;
    hipLaunchKernelGGL(wave_simd_kernel, dim3(WGS), dim3(1024), 140 * 1024, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    bool holds = true;
    for (int g = 0; g < WGS; ++g) {
        printf("workgroup %d (CU %u): SIMD of waves 0..15:", g, (h[g * WAVES] >> 8) & 15u);
        for (int w = 0; w < WAVES; ++w) {
            const unsigned simd = (h[g * WAVES + w] >> 4) & 3u;
            printf(" %u", simd);
            holds = holds && simd == ((h[g * WAVES + (w & 3)] >> 4) & 3u);  // the SIMD of wave w is that of wave w & 3 ...
        }
        for (int w = 1; w < 4; ++w)  // ... and waves 0 .. 3 sit on four different SIMDs
            for (int v = 0; v < w; ++v) holds = holds && ((h[g * WAVES + w] >> 4) & 3u) != ((h[g * WAVES + v] >> 4) & 3u);
        printf("\n");
    }
    printf("waves w, w + 4, w + 8, w + 12 share a SIMD and waves 0 .. 3 sit on four SIMDs: %s\n", holds ? "yes" : "NO");
    (void)hipFree(d);
    return 0;
}
