// Micro-benchmark, the sibling of mfma32_shadow.hip: does the vector work of prune_bound_mm32_kernel ride in the shadow
// of v_mfma_f32_32x32x16_bf16 on gfx950?  The guide's figures say the instruction takes 32 cycles per SIMD and holds the
// vector issue for 8 of them.  One "tile" is a 32 x 32 block of exponents.
//   MODE 0  the bf16 form: four CHAINED v_mfma_f32_32x32x16_bf16 into one accumulator tile (the first from C = 0), and
//           behind each of them 4 v_exp_f32 + 8 v_fma_f32 on the PREVIOUS tile's accumulators (sched_barrier pins the
//           order): 16 exponentials and 32 fmas per tile
//   MODE 1  the four chained bf16 MFMAs alone
//   MODE 2  the fillers alone
//   MODE 3  today's shape, four tiles in one piece: 20 v_mfma_f32_32x32x2_f32, then 64 v_exp_f32 + 128 v_fma_f32
// at one, two and three wavefronts per SIMD; 96 KB of dynamic LDS keeps one workgroup per CU.  Reported: cycles
// (s_memtime) of the slowest wavefront of workgroup 0 per tile it formed, and the same per SIMD (divided by the
// wavefronts that share it).  Three runs per variant: their spread is the probe's own noise.
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

template <int MODE>
__global__ __launch_bounds__(768) void k(float* out, unsigned long long* cyc, int iters, float seed) {
    extern __shared__ float lds[];
    // b is tiny: the accumulators stay near their start values, the exponentials stay finite
    const float a = seed + threadIdx.x * 1e-6f, b = (1.0f - seed) * 1e-7f;
    bf16x8 pa[4], qb[4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 8; ++j) { pa[i][j] = (__bf16)(a + 0.01f * (i + j)); qb[i][j] = (__bf16)(b * (1 + i + j)); }
    f32x16 c[4];
    for (int g = 0; g < 4; ++g)
        for (int r = 0; r < 16; ++r) c[g][r] = -seed * r;
    float al[16], ps = 0.0f, pS = 0.0f;
    for (int r = 0; r < 16; ++r) al[r] = seed - 0.1f * r;
    // four exponentials of accumulator tile g (values r0 ..) and two fmas per exponential, as in the kernel; ONE block of
    // instructions, for the reasons mfma32_shadow.hip gives
    auto fill = [&](int g, int r0) {
#define X(j) "v"(c[g][(r0 + j) & 15])
#define W(j) "v"(al[(r0 + j) & 15])
#define FM(k, w) "v_fmac_f32 %0, " k ", " w "\n v_fma_f32 %1, " k ", |" w "|, %1\n"
        float k0, k1, k2, k3;
        asm volatile("v_exp_f32 %2, %6\n v_exp_f32 %3, %7\n v_exp_f32 %4, %8\n v_exp_f32 %5, %9\n"
                     FM("%2", "%10") FM("%3", "%11") FM("%4", "%12") FM("%5", "%13")
                     : "+v"(ps), "+v"(pS), "=&v"(k0), "=&v"(k1), "=&v"(k2), "=&v"(k3)
                     : X(0), X(1), X(2), X(3), W(0), W(1), W(2), W(3));
#undef X
#undef W
#undef FM
    };
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if (MODE == 3) {
#pragma unroll
            for (int i = 0; i < 20; ++i) c[i & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c[i & 3], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) fill(i >> 2, 4 * i);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            // four tiles per iteration, tile t into c[t & 1] while the fillers read c[(t + 1) & 1]
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (MODE != 2) c[t & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[i], qb[(i + t) & 3], i ? c[t & 1] : zero, 0, 0, 0);
                    else asm volatile("" : "+v"(c[(t + 1) & 1]));      // no MFMA: opaque, or the fillers leave the loop
                    if (MODE != 1) fill((t + 1) & 1, 4 * i);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = ps + pS;
    for (int g = 0; g < 4; ++g)
        for (int r = 0; r < 16; ++r) s += c[g][r];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) cyc[threadIdx.x >> 6] = t1 - t0;
}

template <int MODE>
void run(const char* name) {
    float* out; unsigned long long* cyc;
    const int nblk = 256, iters = 2000, lds = 96 * 1024;
    (void)hipMalloc(&out, sizeof(float) * nblk * 768); (void)hipMalloc(&cyc, 8 * 12);
    (void)hipFuncSetAttribute((const void*)k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    for (int wps = 1; wps <= 3; ++wps) {
        const int nw = 4 * wps;
        printf("%-52s %d wave/SIMD:", name, wps);
        for (int rep = 0; rep < 3; ++rep) {
            hipLaunchKernelGGL((k<MODE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, 50, 0.5f);
            (void)hipDeviceSynchronize();
            hipLaunchKernelGGL((k<MODE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, iters, 0.5f);
            if (hipDeviceSynchronize() != hipSuccess) { printf(" launch failed\n"); return; }
            unsigned long long c[12], mx = 0;
            (void)hipMemcpy(c, cyc, 8 * nw, hipMemcpyDeviceToHost);
            for (int i = 0; i < nw; ++i) mx = c[i] > mx ? c[i] : mx;
            const double per = (double)mx / iters / 4;
            printf("  %7.1f /wave %7.1f /SIMD", per, per / wps);
        }
        printf("  cycles per tile\n");
    }
    (void)hipFree(out); (void)hipFree(cyc);
}

int main() {
    run<0>("4 chained bf16 mfma, 4 exp + 8 fma behind each");
    run<1>("4 chained bf16 mfma alone");
    run<2>("16 exp + 32 fma per tile, no mfma");
    run<3>("today: 20 fp32 mfma, then 64 exp + 128 fma (4 tiles)");
    return 0;
}
