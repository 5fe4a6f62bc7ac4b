// Micro-benchmark, the sibling of mfma_bf16_shadow.hip: the instruction mix of prune_bound_mm32_kernel<8, true, true> per
// 32-row matrix tile and wavefront -- 16 v_mfma_f32_32x32x16_bf16 in four chains of four (one chain per 32-candidate
// group, the first from C = 0), 8 ds_read_b128 (4 fragments + 16 alphas), 64 v_exp_f32, 64 v_fmac_f32, 8 v_cvt_f64_f32 +
// 8 v_add_f64 -- in two orders:
//   MODE 0  the order hipcc emits for the kernel (docs/experiments.md, round 30): the reads and their wait open the
//           iteration, the 16 MFMAs follow in one burst (t-major, four accumulator tiles live), the vector work of all
//           four groups stands behind them
//   MODE 1  the pipelined order: the NEXT matrix tile's reads are issued before the vector work into a second register
//           set; the four chained MFMAs of group g + 1 are issued one at a time, each in front of 4 v_exp_f32 +
//           4 v_fmac_f32 of group g; group 0 of the next matrix tile runs under group 3 of this one; two accumulator
//           tiles live
// sched_barrier(0) pins the order and the fillers are written as instructions, as in mfma_bf16_shadow.hip.  One and two
// wavefronts per SIMD in ONE workgroup (96 KB of dynamic LDS keeps one workgroup per CU).  Reported: cycles (s_memtime)
// of the slowest wavefront of workgroup 0 per 32 x 32 tile of exponents (a quarter of a matrix tile), and the same per
// SIMD (divided by the wavefronts that share it).  Three runs per variant: their spread is the probe's own noise.
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

#define PITCH 72            // bf16 values per LDS row, the kernel's at Dpad = 8
#define NT 4                // 32-row matrix tiles in LDS (a staged tile of the kernel)

template <int MODE>
__global__ __launch_bounds__(512) void k(float* out, unsigned long long* cyc, int iters, float seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __bf16* xt = (__bf16*)lds;
    float* at = (float*)(lds + NT * 32 * PITCH * 2);
    for (int i = threadIdx.x; i < NT * 32 * PITCH; i += blockDim.x) xt[i] = (__bf16)(seed + 0.01f * (i % 7));
    for (int i = threadIdx.x; i < NT * 32; i += blockDim.x) at[i] = seed - 0.01f * (i % 16);
    __syncthreads();
    const int lane = threadIdx.x & 63, h = lane >> 5, l32 = lane & 31;
    // b is tiny: the exponents stay near 0, the exponentials near 1
    const float b = (1.0f - seed) * 1e-7f;
    bf16x8 qb[4][4];
    for (int g = 0; g < 4; ++g)
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 8; ++j) qb[g][i][j] = (__bf16)(b * (1 + g + i + j));
    double accm[4] = {0.0, 0.0, 0.0, 0.0}, accs[4] = {0.0, 0.0, 0.0, 0.0};
    // a matrix tile's fragments and alphas, as the kernel reads them
    auto rd = [&](int t, bf16x8 (&p)[4], f32x4 (&al)[4]) {
        const __bf16* xr = xt + (t * 32 + l32) * PITCH + 8 * h;
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = *(const bf16x8*)(xr + 16 * i);
#pragma unroll
        for (int q = 0; q < 4; ++q) al[q] = *(const f32x4*)(at + t * 32 + 8 * q + 4 * h);
    };
    // four exponentials of an accumulator tile (values 4 i ..) and one fma per exponential; ONE block of instructions
    auto fill = [&](const f32x16& c, int i, const f32x4& al, float& ps) {
        float k0, k1, k2, k3;
        asm volatile("v_exp_f32 %1, %5\n v_exp_f32 %2, %6\n v_exp_f32 %3, %7\n v_exp_f32 %4, %8\n"
                     "v_fmac_f32 %0, %1, %9\n v_fmac_f32 %0, %2, %10\n v_fmac_f32 %0, %3, %11\n v_fmac_f32 %0, %4, %12\n"
                     : "+v"(ps), "=&v"(k0), "=&v"(k1), "=&v"(k2), "=&v"(k3)
                     : "v"(c[4 * i]), "v"(c[4 * i + 1]), "v"(c[4 * i + 2]), "v"(c[4 * i + 3]),
                       "v"(al[0]), "v"(al[1]), "v"(al[2]), "v"(al[3]));
    };
    auto sums = [&](int g, float& ps) {
        accm[g] += (double)ps;
        accs[g] += (double)fabsf(ps);
        ps = 0.0f;
    };
    const f32x16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bf16x8 p0[4], p1[4];
    f32x4 a0[4], a1[4];
    f32x16 c[4];
    float ps[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (MODE == 0) {
#pragma unroll 1
        for (int it = 0; it < iters; ++it) {
            rd(it & (NT - 1), p0, a0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    c[g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0[i], qb[g][i], i ? c[g] : zero, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int i = 0; i < 4; ++i) fill(c[g], i, a0[i], ps[g]);
                sums(g, ps[g]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // one matrix tile: its rows in (p, al), the next one's read into (pn, aln); c[0] holds group 0 on entry and on exit
        auto body = [&](int t, bf16x8 (&p)[4], f32x4 (&al)[4], bf16x8 (&pn)[4], f32x4 (&aln)[4]) {
            rd((t + 1) & (NT - 1), pn, aln);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    c[(g + 1) & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g < 3 ? p[i] : pn[i], qb[(g + 1) & 3][i],
                                                                            i ? c[(g + 1) & 1] : zero, 0, 0, 0);
                    fill(c[g & 1], i, al[i], ps[0]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                sums(g, ps[0]);
            }
        };
        rd(0, p0, a0);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(p0[i], qb[0][i], i ? c[0] : zero, 0, 0, 0);
#pragma unroll 1
        for (int it = 0; it < iters; it += 2) {
            body(it, p0, a0, p1, a1);
            body(it + 1, p1, a1, p0, a0);
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    double s = 0.0;
    for (int g = 0; g < 4; ++g) s += accm[g] + accs[g];
    for (int r = 0; r < 16; ++r) s += c[0][r];
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = (float)s;
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) cyc[threadIdx.x >> 6] = t1 - t0;
}

template <int MODE>
void run(const char* name) {
    float* out; unsigned long long* cyc;
    const int nblk = 256, iters = 2000, lds = 96 * 1024;
    (void)hipMalloc(&out, sizeof(float) * nblk * 512); (void)hipMalloc(&cyc, 8 * 8);
    (void)hipFuncSetAttribute((const void*)k<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    for (int wps = 1; wps <= 2; ++wps) {
        const int nw = 4 * wps;
        printf("%-58s %d wave/SIMD:", name, wps);
        for (int rep = 0; rep < 3; ++rep) {
            hipLaunchKernelGGL((k<MODE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, 50, 0.5f);
            (void)hipDeviceSynchronize();
            hipLaunchKernelGGL((k<MODE>), dim3(nblk), dim3(64 * nw), lds, 0, out, cyc, iters, 0.5f);
            if (hipDeviceSynchronize() != hipSuccess) { printf(" launch failed\n"); return; }
            unsigned long long c[8], mx = 0;
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
    run<0>("(a) reads + wait, 16 mfma in a burst, the vector work behind");
    run<1>("(b) next tile prefetched, 1 mfma per 4 exp + 4 fma");
    return 0;
}
