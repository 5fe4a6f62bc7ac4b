// What does v_mfma_f32_32x32x16_bf16 do with its 16 products and C on gfx950?  One wavefront forms D = A B + C for a
// 32 x 16 A, a 16 x 32 B (bf16) and a 32 x 32 C (fp32) per case; the host holds the exact value of every entry (products of
// two bf16 numbers are exact in fp64; the 17 addends are summed in long double, inside whose 64 bits every case here
// stays) and the value under a family of models, and counts the entries of D whose BITS differ from each model:
//   exact groups  "g<G> exact rne|rz": the products are taken G at a time in k order (G = 1, 2, 4, 8, 16), each group summed
//                 exactly onto the accumulator (which starts at C), one rounding per group;
//   cut groups    "g<G> W<w> fl|tz [un] [all] [ac]": as above, but the products of a group are first aligned to the group's
//                 largest exponent and cut to w bits below its 24-bit significand (struct Model).
// and the largest error against an envelope that needs no bit-exact model (report()).
// Cases: random operands (narrow and wide exponent range); one large addend with fifteen small ones of one sign (each
// 1/8 ulp of the large one: per-addend rounding loses them all, one rounding of the exact sum sees 15/8 ulp, negative
// ones tell truncation from rounding); full cancellation with a small residue; C large against the products and the
// reverse; the same products in permuted k slots (bits against the identity order); slots 10 .. 15 zero; operands and
// results near 2^-126 (bf16 subnormal inputs, fp32 subnormal products and sums, subnormal C).
// Also printed per case: the largest |D - exact| in units of u (|C| + sum |a_k b_k|), u = 2^-24.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// A: [32][16] bf16 bits, B: [16][32], C and D: [32][32]; lane maps as in DESIGN.md section 2
__global__ __launch_bounds__(64) void k(const uint16_t* A, const uint16_t* B, const float* C, float* D) {
    const int l = threadIdx.x, r = l & 31, h = l >> 5;
    union { bf16x8 v; uint16_t s[8]; } a, b;
    for (int j = 0; j < 8; ++j) { a.s[j] = A[r * 16 + 8 * h + j]; b.s[j] = B[(8 * h + j) * 32 + r]; }
    f32x16 c;
    for (int i = 0; i < 16; ++i) c[i] = C[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r];
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, c, 0, 0, 0);
    for (int i = 0; i < 16; ++i) D[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = c[i];
}

static uint64_t rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 16); }
static float bf2f(uint16_t s) { uint32_t u = (uint32_t)s << 16; float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
// random bf16 with exponent in [e0, e1], random sign unless sgn != 0
static uint16_t rbf(int e0, int e1, int sgn = 0) {
    const int e = e0 + (int)(rnd() % (uint32_t)(e1 - e0 + 1));
    const uint16_t s = sgn ? (sgn < 0 ? 0x8000 : 0) : (rnd() & 1 ? 0x8000 : 0);
    return (uint16_t)(s | ((e + 127) << 7) | (rnd() & 0x7f));
}
static float rz32(long double x) { float f = (float)x; if (fabsl((long double)f) > fabsl(x)) f = nextafterf(f, 0.0f); return f; }
static float rnd32(long double x, bool rz) { return rz ? rz32(x) : (float)x; }

struct Case { uint16_t A[32 * 16], B[16 * 32]; float C[32 * 32], D[32 * 32]; };

// One model: the products G at a time in k order; per group a reference exponent (of the largest product, taken from the
// normalised product or, "un", from the sum of the operands' exponents; "all": the accumulator counts too), the products
// (and with "ac" the accumulator) cut toward -inf ("fl") or toward zero to W bits below the reference's 24-bit significand
// (W < 0: no cut; "acfl": the accumulator toward -inf whatever the products), everything summed exactly, one rounding (to nearest, or "rz") per group.
struct Model { int G, W; bool fl, un, all; int ac; bool rz; };     // ac: 0 the accumulator is not cut, 1 cut as the products, 2 toward -inf
static float model(const Case& c, int i, int j, const Model& m) {
    float acc = c.C[i * 32 + j];
    for (int k0 = 0; k0 < 16; k0 += m.G) {
        long double t[17];
        int eref = -100000, e;
        for (int k = 0; k < m.G; ++k) {
            const float a = bf2f(c.A[i * 16 + k0 + k]), b = bf2f(c.B[(k0 + k) * 32 + j]);
            t[k] = (long double)a * (long double)b;
            if (t[k] == 0.0L) continue;
            if (m.un) { int ea, eb; frexpf(a, &ea); frexpf(b, &eb); e = ea + eb; } else frexpl(t[k], &e);
            eref = e > eref ? e : eref;
        }
        if (m.all && acc != 0.0f) { frexpf(acc, &e); eref = e > eref ? e : eref; }
        long double s = 0.0L, av = acc;
        if (m.W >= 0 && eref != -100000) {
            const long double q = ldexpl(1.0L, eref - 24 - m.W);
            for (int k = 0; k < m.G; ++k) s += (m.fl ? floorl(t[k] / q) : truncl(t[k] / q)) * q;
            if (m.ac) av = (m.fl || m.ac == 2 ? floorl(av / q) : truncl(av / q)) * q;
        } else
            for (int k = 0; k < m.G; ++k) s += t[k];
        acc = rnd32(s + av, m.rz);
    }
    return acc;
}
static std::vector<Model> models() {
    std::vector<Model> v;
    const int Gs[5] = {1, 2, 4, 8, 16};
    for (int g = 0; g < 5; ++g)
        for (int z = 0; z < 2; ++z) v.push_back(Model{Gs[g], -1, false, false, false, 0, z != 0});
    for (int g = 2; g < 5; ++g)
        for (int w = 0; w <= 4; ++w)
            for (int f = 0; f < 2; ++f)
                for (int un = 0; un < 2; ++un)
                    for (int aa = 0; aa < 6; ++aa) {
                        if (f && aa >= 4) continue;          // (fl with ac 2 is fl with ac 1)
                        v.push_back(Model{Gs[g], w, f != 0, un != 0, (aa & 1) != 0, aa >> 1, false});
                    }
    return v;
}
static void name_of(const Model& m, char* buf) {
    if (m.W < 0) sprintf(buf, "g%d exact %s", m.G, m.rz ? "rz" : "rne");
    else sprintf(buf, "g%d W%d %s%s%s%s", m.G, m.W, m.fl ? "fl" : "tz", m.un ? " un" : "", m.all ? " all" : "", m.ac == 2 ? " acfl" : m.ac ? " ac" : "");
}
static long double exact(const Case& c, int i, int j, long double* mag) {
    long double s = c.C[i * 32 + j], m = fabsl(s);
    for (int k = 0; k < 16; ++k) {
        const long double p = (long double)bf2f(c.A[i * 16 + k]) * (long double)bf2f(c.B[k * 32 + j]);
        s += p; m += fabsl(p);
    }
    *mag = m;
    return s;
}

static uint16_t *dA, *dB; static float *dC, *dD;
static void run(Case& c) {
    (void)hipMemcpy(dA, c.A, sizeof c.A, hipMemcpyHostToDevice);
    (void)hipMemcpy(dB, c.B, sizeof c.B, hipMemcpyHostToDevice);
    (void)hipMemcpy(dC, c.C, sizeof c.C, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); exit(1); }
    (void)hipMemcpy(c.D, dD, sizeof c.D, hipMemcpyDeviceToHost);
}

static std::vector<long> total_mis;
static void report(const char* name, std::vector<Case>& cs) {
    static const std::vector<Model> ms = models();
    if (total_mis.empty()) total_mis.assign(ms.size(), 0);
    std::vector<long> mis(ms.size(), 0);
    long tot = 0, nz_zero = 0;
    double worst = 0.0, env[4] = {0.0, 0.0, 0.0, 0.0};
    for (Case& c : cs) {
        run(c);
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                const float d = c.D[i * 32 + j];
                ++tot;
                for (size_t q = 0; q < ms.size(); ++q) mis[q] += bits(model(c, i, j, ms[q])) != bits(d);
                long double mag;
                const long double ex = exact(c, i, j, &mag);
                const long double err = fabsl((long double)d - ex);
                if (mag > 0.0L) { const double e = (double)(err / (mag * 0x1p-24L)); worst = e > worst ? e : worst; }
                if (ex != 0.0L && d == 0.0f) ++nz_zero;
                // the envelope: per half (slots 0 .. 7, 8 .. 15) every non-zero product loses less than 2^-W ulp of the
                // half's largest product (ulp(p) <= 2 u |p|), and each half ends in one rounding to nearest of a partial
                // sum that is at most |C| + sum |ab|
                long double cut = 0.0L;
                for (int h = 0; h < 2; ++h) {
                    long double pm = 0.0L; int nn = 0;
                    for (int k = 8 * h; k < 8 * h + 8; ++k) {
                        const long double p = fabsl((long double)bf2f(c.A[i * 16 + k]) * (long double)bf2f(c.B[k * 32 + j]));
                        pm = p > pm ? p : pm; nn += p != 0.0L;
                    }
                    cut += nn * 0x1p-23L * pm;
                }
                for (int w = 0; w < 4; ++w) {
                    const long double bound = ldexpl(cut, -w) + 2.0L * 0x1p-24L * mag + 0x1p-149L;
                    const double r = (double)(err / bound);
                    env[w] = r > env[w] ? r : env[w];
                }
            }
    }
    printf("== %s: %ld entries, worst |D - exact| = %.4f u (|C| + sum|ab|), exact != 0 but D == 0: %ld\n", name, tot, worst, nz_zero);
    printf("   largest |D - exact| / envelope(W):  W0 %.3f  W1 %.3f  W2 %.3f  W3 %.3f\n", env[0], env[1], env[2], env[3]);
    printf("   entries whose bits differ from a model, the eight closest models:");
    std::vector<bool> done(ms.size(), false);
    for (int b = 0; b < 8; ++b) {
        size_t best = 0; long bv = -1;
        for (size_t q = 0; q < ms.size(); ++q)
            if (!done[q] && (bv < 0 || mis[q] < bv)) { bv = mis[q]; best = q; }
        done[best] = true;
        char buf[64];
        name_of(ms[best], buf);
        printf("%s [%s] %ld", b ? "," : "", buf, bv);
    }
    printf("\n");
    for (size_t q = 0; q < ms.size(); ++q) total_mis[q] += mis[q];
}
static void report_total() {
    const std::vector<Model> ms = models();
    printf("== all cases together, the twelve closest models:\n");
    std::vector<bool> done(ms.size(), false);
    for (int b = 0; b < 12; ++b) {
        size_t best = 0; long bv = -1;
        for (size_t q = 0; q < ms.size(); ++q)
            if (!done[q] && (bv < 0 || total_mis[q] < bv)) { bv = total_mis[q]; best = q; }
        done[best] = true;
        char buf[64];
        name_of(ms[best], buf);
        printf("   [%s] %ld\n", buf, bv);
    }
}

static void fill_random(Case& c, int e0, int e1, int ce0, int ce1) {
    for (int i = 0; i < 32 * 16; ++i) { c.A[i] = rbf(e0, e1); c.B[i] = rbf(e0, e1); }
    for (int i = 0; i < 32 * 32; ++i) {
        const uint32_t u = ((rnd() & 1u) << 31) | ((uint32_t)(ce0 + (int)(rnd() % (uint32_t)(ce1 - ce0 + 1)) + 127) << 23) | (rnd() & 0x7fffff);
        memcpy(&c.C[i], &u, 4);
    }
}

int main() {
    (void)hipMalloc(&dA, 1024); (void)hipMalloc(&dB, 1024); (void)hipMalloc(&dC, 4096); (void)hipMalloc(&dD, 4096);
    const int T = 8;
    std::vector<Case> cs(T);
    for (Case& c : cs) fill_random(c, -2, 2, -2, 2);
    report("random, exponents within 2^+-2", cs);
    for (Case& c : cs) fill_random(c, -10, 10, -20, 20);
    report("random, operand exponents within 2^+-10, C within 2^+-20", cs);
    // one large addend (slot ks, magnitude in [1, 4)) and fifteen of 2^-26 .. 2^-25 relative to 1: 1/8 .. 1/4 ulp of the
    // large one each; the small ones positive in even rows, negative in odd rows; C = 0
    for (int t = 0; t < T; ++t) {
        Case& c = cs[t];
        const int ks = (5 * t + 3) & 15;
        for (int i = 0; i < 32; ++i)
            for (int kk = 0; kk < 16; ++kk) c.A[i * 16 + kk] = kk == ks ? rbf(0, 0, 1) : rbf(-13, -13, (i & 1) ? -1 : 1);
        for (int kk = 0; kk < 16; ++kk)
            for (int j = 0; j < 32; ++j) c.B[kk * 32 + j] = kk == ks ? rbf(0, 0, 1) : rbf(-13, -13, 1);
        memset(c.C, 0, sizeof c.C);
    }
    report("one large addend, fifteen small ones of one sign, C = 0", cs);
    // the same with the large addend in C
    for (int t = 0; t < T; ++t) {
        Case& c = cs[t];
        for (int i = 0; i < 32; ++i)
            for (int kk = 0; kk < 16; ++kk) c.A[i * 16 + kk] = rbf(-13, -13, (i & 1) ? -1 : 1);
        for (int i = 0; i < 16 * 32; ++i) c.B[i] = rbf(-13, -13, 1);
        for (int i = 0; i < 32 * 32; ++i) c.C[i] = 1.0f + (float)(rnd() & 0x7fffff) * 0x1p-23f;
    }
    report("C large, sixteen small products of one sign", cs);
    // full cancellation: slots 2 q and 2 q + 1 cancel exactly for q < 7, slots 14, 15 hold a residue 2^-20 of them; C = 0
    for (Case& c : cs) {
        fill_random(c, -2, 2, 0, 0);
        for (int i = 0; i < 32; ++i)
            for (int q = 0; q < 7; ++q) c.A[i * 16 + 2 * q + 1] = c.A[i * 16 + 2 * q] ^ 0x8000;
        for (int j = 0; j < 32; ++j)
            for (int q = 0; q < 7; ++q) c.B[(2 * q + 1) * 32 + j] = c.B[(2 * q) * 32 + j];
        for (int i = 0; i < 32; ++i) { c.A[i * 16 + 14] = rbf(-21, -19); c.A[i * 16 + 15] = rbf(-21, -19); }
        memset(c.C, 0, sizeof c.C);
    }
    report("seven cancelling pairs and a residue of 2^-20, C = 0", cs);
    for (Case& c : cs) fill_random(c, -2, 2, 18, 22);
    report("C 2^20 times the products", cs);
    for (Case& c : cs) fill_random(c, -2, 2, -24, -20);
    report("C 2^-20 times the products", cs);
    // against the cut: per half one product of 1 .. 4 and seven of 2^-24 .. 2^-22 of one sign per row, around the grid of
    // the large one; C = 0 in the first half of the cases, of the large products' size in the others
    for (int t = 0; t < T; ++t) {
        Case& c = cs[t];
        for (int i = 0; i < 32; ++i)
            for (int kk = 0; kk < 16; ++kk) c.A[i * 16 + kk] = (kk & 7) == (t & 7) ? rbf(0, 0, 1) : rbf(-12, -12, (i & 1) ? -1 : 1);
        for (int kk = 0; kk < 16; ++kk)
            for (int j = 0; j < 32; ++j) c.B[kk * 32 + j] = (kk & 7) == (t & 7) ? rbf(0, 0, 1) : rbf(-12, -12, 1);
        for (int i = 0; i < 32 * 32; ++i) c.C[i] = t < T / 2 ? 0.0f : 1.0f + (float)(rnd() & 0x7fffff) * 0x1p-23f;
    }
    report("per half one large product and seven around its grid", cs);
    // the same products in permuted k slots: bits against the identity order
    {
        long diff = 0, tot = 0;
        for (int t = 0; t < T; ++t) {
            Case c0;
            fill_random(c0, -10, 10, -20, 20);
            run(c0);
            for (int p = 0; p < 4; ++p) {
                int perm[16];
                for (int i = 0; i < 16; ++i) perm[i] = i;
                for (int i = 15; i > 0; --i) { const int j = (int)(rnd() % (uint32_t)(i + 1)), x = perm[i]; perm[i] = perm[j]; perm[j] = x; }
                Case c1 = c0;
                for (int i = 0; i < 32; ++i)
                    for (int kk = 0; kk < 16; ++kk) c1.A[i * 16 + kk] = c0.A[i * 16 + perm[kk]];
                for (int kk = 0; kk < 16; ++kk)
                    for (int j = 0; j < 32; ++j) c1.B[kk * 32 + j] = c0.B[perm[kk] * 32 + j];
                run(c1);
                for (int i = 0; i < 1024; ++i) { ++tot; diff += bits(c0.D[i]) != bits(c1.D[i]); }
            }
        }
        printf("== permuted k slots (wide exponents): %ld of %ld entries differ in bits from the identity order\n", diff, tot);
    }
    for (Case& c : cs) {
        fill_random(c, -10, 10, -20, 20);
        for (int i = 0; i < 32; ++i)
            for (int kk = 10; kk < 16; ++kk) c.A[i * 16 + kk] = 0;
        for (int kk = 10; kk < 16; ++kk)
            for (int j = 0; j < 32; ++j) c.B[kk * 32 + j] = (kk & 1) ? 0 : c.B[kk * 32 + j];      // 0 x 0 and 0 x finite
    }
    report("slots 10 .. 15 zero (wide exponents)", cs);
    // near 2^-126
    for (Case& c : cs) {
        fill_random(c, -64, -62, -128, -124);          // products 2^-128 .. 2^-124, C in the same range
        for (int i = 0; i < 1024; ++i) if (i & 1) c.C[i] = 0.0f;
    }
    report("products and C around 2^-126 (normal bf16 operands)", cs);
    for (Case& c : cs) {
        for (int i = 0; i < 32 * 16; ++i) {
            c.A[i] = (uint16_t)((rnd() & 1 ? 0x8000 : 0) | (1 + rnd() % 0x7f));        // bf16 subnormal: exponent field 0
            c.B[i] = rbf(100, 104);
        }
        memset(c.C, 0, sizeof c.C);
    }
    report("bf16 subnormal A times 2^100 .. 2^104, C = 0", cs);
    for (Case& c : cs) {
        fill_random(c, -2, 2, 0, 0);
        for (int i = 0; i < 1024; ++i) { const uint32_t u = ((rnd() & 1u) << 31) | (1 + (rnd() & 0x7ffffe)); memcpy(&c.C[i], &u, 4); }
        for (int i = 0; i < 32 * 16; ++i) c.A[i] = 0;
    }
    report("A = 0, C subnormal", cs);
    report_total();
    return 0;
}
