// Micro-benchmark: what rides in the shadow of v_mfma_f32_32x32x2_f32 on gfx950?  The fp32 matrix rate equals the fp32
// vector rate, so the question is whether the two share the vector lanes (as the fp64 MFMA shares the DP pipe) or
// whether v_exp_f32 / v_fma_f32 of the SAME wavefront issue for free while an MFMA's 64 cycles run.
// Variants, each 20 MFMAs per iteration (one 32-row tile of prune_bound_mm32_kernel<8>: 4 groups x 5 steps):
//   MODE 0  MFMAs alone
//   MODE 1  each MFMA followed by NE v_exp_f32 + 2 NE v_fma_f32 (sched_barrier pins the order)
//   MODE 2  the same fillers with no MFMA
//   MODE 3  the burst shape: 20 MFMAs, then 64 v_exp_f32 + 128 v_fma_f32
// at one wavefront per SIMD (256 threads) and at three (768 threads); 96 KB of dynamic LDS keeps one workgroup per CU.
// Reported: cycles of the slowest wavefront of workgroup 0 per MFMA it issued (per slot for MODE 2), and the same per
// SIMD (divided by the wavefronts that share it).  Three runs per variant: their spread is the probe's own noise.
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define NM 20

template <int MODE, int NE>
__global__ __launch_bounds__(768) void k(float* out, unsigned long long* cyc, int iters, float seed) {
    extern __shared__ float lds[];
    // b is tiny: the accumulators stay near their start values, the exponentials stay finite
    const float a = seed + threadIdx.x * 1e-6f, b = (1.0f - seed) * 1e-7f;
    f32x16 c[4];
    for (int g = 0; g < 4; ++g)
        for (int r = 0; r < 16; ++r) c[g][r] = -seed * r;
    float al[16], ps = 0.0f, pS = 0.0f;
    for (int r = 0; r < 16; ++r) al[r] = seed - 0.1f * r;
    // ne (3 or 4) exponentials of accumulator tile g (values r0 ..) and two fmas per exponential, as in the kernel.
    // Written as ONE block of instructions: left to itself hipcc pairs the two sums into v_pk_fma_f32 (which the kernel
    // does not get) and gathers them across the MFMAs before the scheduler, and its barriers, ever see them; and it
    // puts an s_nop in front of every asm statement, so there is one statement per slot.  Every exponential stands at
    // least two instructions before its first use.
    auto fill = [&](int g, int r0, int ne) {
#define X(j) "v"(c[g][(r0 + j) & 15])
#define W(j) "v"(al[(r0 + j) & 15])
#define FM(k, w) "v_fmac_f32 %0, " k ", " w "\n v_fma_f32 %1, " k ", |" w "|, %1\n"
        float k0, k1, k2, k3;
        if (ne == 3)
            asm volatile("v_exp_f32 %2, %5\n v_exp_f32 %3, %6\n v_exp_f32 %4, %7\n" FM("%2", "%8") FM("%3", "%9") FM("%4", "%10")
                         : "+v"(ps), "+v"(pS), "=&v"(k0), "=&v"(k1), "=&v"(k2) : X(0), X(1), X(2), W(0), W(1), W(2));
        if (ne == 4)
            asm volatile("v_exp_f32 %2, %6\n v_exp_f32 %3, %7\n v_exp_f32 %4, %8\n v_exp_f32 %5, %9\n"
                         FM("%2", "%10") FM("%3", "%11") FM("%4", "%12") FM("%5", "%13")
                         : "+v"(ps), "+v"(pS), "=&v"(k0), "=&v"(k1), "=&v"(k2), "=&v"(k3)
                         : X(0), X(1), X(2), X(3), W(0), W(1), W(2), W(3));
#undef X
#undef W
#undef FM
    };
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if (MODE == 3) {
#pragma unroll
            for (int i = 0; i < NM; ++i) c[i & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c[i & 3], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 16; ++i) fill(i >> 2, 4 * i, 4);
            __builtin_amdgcn_sched_barrier(0);
        } else {
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                // the fillers read the tile written two MFMAs ago: its result is in, as in a software pipeline
                if (MODE != 2) c[i & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c[i & 3], 0, 0, 0);
                else asm volatile("" : "+v"(c[(i + 2) & 3]));      // no MFMA: opaque, or the fillers leave the loop
                fill((i + 2) & 3, NE * i, NE);
                __builtin_amdgcn_sched_barrier(0);
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

template <int MODE, int NE>
void run(const char* name) {
    float* out; unsigned long long* cyc;
    const int nblk = 256, iters = 2000, lds = 96 * 1024;
    (void)hipMalloc(&out, sizeof(float) * nblk * 768); (void)hipMalloc(&cyc, 8 * 12);
    (void)hipFuncSetAttribute((const void*)k<MODE, NE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    for (int wps = 1; wps <= 3; wps += 2) {
        const int nw = 4 * wps;
        printf("%-44s %d wave/SIMD:", name, wps);
        for (int rep = 0; rep < 3; ++rep) {
            hipLaunchKernelGGL((k<MODE, NE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, 50, 0.5f);
            (void)hipDeviceSynchronize();
            hipLaunchKernelGGL((k<MODE, NE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, iters, 0.5f);
            if (hipDeviceSynchronize() != hipSuccess) { printf(" launch failed\n"); return; }
            unsigned long long c[12], mx = 0;
            (void)hipMemcpy(c, cyc, 8 * nw, hipMemcpyDeviceToHost);
            for (int i = 0; i < nw; ++i) mx = c[i] > mx ? c[i] : mx;
            const double per = (double)mx / iters / NM;
            printf("  %7.2f /wave %7.2f /SIMD", per, per / wps);
        }
        printf("  cycles per MFMA\n");
    }
    (void)hipFree(out); (void)hipFree(cyc);
}

int main() {
    run<0, 0>("mfma alone");
    run<1, 3>("mfma + 3 exp + 6 fma each");
    run<1, 4>("mfma + 4 exp + 8 fma each");
    run<2, 3>("3 exp + 6 fma per slot, no mfma");
    run<2, 4>("4 exp + 8 fma per slot, no mfma");
    run<3, 4>("20 mfma, then 64 exp + 128 fma");
    return 0;
}
