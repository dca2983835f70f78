// fiveeq_math.hpp — the shared model, the lane value types and the hand-written math of the step.
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Shared model in kernel precision, passed BY VALUE as the FIRST kernel argument (496 B): it
// lands at offset 0 of the kernarg segment, from where each workgroup stages it into LDS once
// (stage_model below); lanes then read it with broadcast ds_reads.  No HBM traffic per member.
// ---------------------------------------------------------------------------------
template <typename T>
struct KGas {
    T ndt_over_tau[MAX_POOLS];  // -dt / tau_i
    T atc[MAX_POOLS];           // a_i * tau_i * c      (so x_eq_i = atc_i * E * alpha)
    T g0, inv_g1, ra, inv_c, C0, inv_C0, sqrtC0, f1, f2, f3;
};
template <typename T>
struct KModel {
    KGas<T> gas[MAX_GAS];
    T em1_d[2];                 // expm1(-dt/d_j), computed on the host in fp64
    T iirf_max;
    T dt;
};

__device__ __forceinline__ double fe_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fe_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---------------------------------------------------------------------------------
// Lane value types.  A lane carries ONE member (V = double or float) or, in the packed fp32 kernels, TWO CONSECUTIVE
// members (V = float2v: lane l of a wave owns members 2l and 2l + 1 of the wave's 128).  Packed lanes load and store
// 8 bytes per row (512 B per wave-instruction, the fp64 kernels' access shape) and their multiplies, adds and FMAs issue
// as v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 — one instruction for both members (5.0-5.2 cycles per wave-instruction
// against 2 x 2.9-3.6 for the scalar forms, profiles/r03/valu_rates_microbench.txt); what the ISA has no packed form
// for (v_rcp_f32, v_sqrt_f32, v_rndne_f32, v_ldexp_f32, v_frexp_*, min/max, compares and selects) runs per component.
// Packed arithmetic is IEEE per component and every routine below mirrors its scalar twin operation by operation, so a
// member's result does not depend on which kernel shape computed it (tested bit for bit).
// ---------------------------------------------------------------------------------
typedef float float2v __attribute__((ext_vector_type(2)));

template <typename V> struct Lane { using S = V; static constexpr int W = 1; };
template <> struct Lane<float2v> { using S = float; static constexpr int W = 2; };

__device__ __forceinline__ float2v fe_fma(float2v a, float2v b, float2v c) { return __builtin_elementwise_fma(a, b, c); }
// fma with any mix of lane values and shared scalars (constants are splat into both components)
template <typename V, typename A, typename B, typename C>
__device__ __forceinline__ V fma3(A a, B b, C c) { return fe_fma((V)a, (V)b, (V)c); }

// per-lane predicates and selects
struct Mask2 { bool x, y; };
template <typename V> struct MaskOf { using type = bool; };
template <> struct MaskOf<float2v> { using type = Mask2; };
__device__ __forceinline__ bool fe_gt0(double v) { return v > 0.0; }
__device__ __forceinline__ bool fe_gt0(float v) { return v > 0.0f; }
__device__ __forceinline__ Mask2 fe_gt0(float2v v) { return Mask2{v.x > 0.0f, v.y > 0.0f}; }
__device__ __forceinline__ double fe_sel(bool m, double a, double b) { return m ? a : b; }
__device__ __forceinline__ float fe_sel(bool m, float a, float b) { return m ? a : b; }
__device__ __forceinline__ float2v fe_sel(Mask2 m, float2v a, float2v b) { return float2v{m.x ? a.x : b.x, m.y ? a.y : b.y}; }

template <int P0, int P1, int P2>
struct Layout {
    static constexpr int G = (P0 > 0) + (P1 > 0) + (P2 > 0);
    static constexpr int SP = P0 + P1 + P2;
    __host__ __device__ static constexpr int pools(int g) { return g == 0 ? P0 : (g == 1 ? P1 : P2); }
    __host__ __device__ static constexpr int off(int g) { return g == 0 ? 0 : (g == 1 ? P0 : P0 + P1); }
};

// ---------------------------------------------------------------------------------
// Math.  Every transcendental of the step is written for the argument range the model can
// produce (each pinned to <= 2 ulp against a CPU libm through fiveeq_math_probe_*).  expm1 is the
// hot one (one per pool per member-step), always with an argument <= 0:
//   x = k ln2 + r, |r| <= ln2/2 ;  expm1(x) = 2^k (expm1 r) + (2^k - 1)
// with expm1(r) = r + r^2 Q(r), Q a degree-10 near-minimax polynomial (8.5e-19 relative).  For
// k = 0 the result is expm1(r) itself, so small arguments (the tau ~ 1e6 yr pool: x ~ -1e-6)
// keep full RELATIVE accuracy.  A NaN argument: fmax / fmin return their other operand, so expm1 and exp (both precisions)
// evaluate at a clamp (expm1: -1, exp: exp of the lower clamp); log, sqrt and rcp return NaN.
// ---------------------------------------------------------------------------------
// expm1(r) on |r| <= ln2/2 as r + r^2 Q(r): shared by fe_expm1_neg and fe_exp.  Q is the degree-10
// interpolant of (expm1(r) - r)/r^2 at the Chebyshev nodes of the interval (computed in 60-digit
// decimal arithmetic, coefficients rounded to double): approximation error 8.5e-19 relative, where
// the Taylor polynomial needs degree 12 for 1.2e-17.  Two fewer FMAs on each of the nine exp-type
// calls of a three-gas member-step.
__device__ __forceinline__ double fe_expm1_reduced(double r) {
    double q = 0x1.1f72fc730b4ffp-29;
    q = __builtin_fma(q, r, 0x1.af4ddd84882fep-26);
    q = __builtin_fma(q, r, 0x1.27e4db67b4303p-22);
    q = __builtin_fma(q, r, 0x1.71de02375656cp-19);
    q = __builtin_fma(q, r, 0x1.a01a01a6d7808p-16);
    q = __builtin_fma(q, r, 0x1.a01a01abe62ddp-13);
    q = __builtin_fma(q, r, 0x1.6c16c16c162d6p-10);
    q = __builtin_fma(q, r, 0x1.11111111100dfp-7);
    q = __builtin_fma(q, r, 0x1.5555555555556p-5);
    q = __builtin_fma(q, r, 0x1.5555555555557p-3);
    q = __builtin_fma(q, r, 0x1.0000000000000p-1);
    return __builtin_fma(r * r, q, r);
}
// x = k ln2 + r with |r| <= ln2/2 (two-step Cody-Waite; ln2 hi has 32 zero low bits)
__device__ __forceinline__ double fe_reduce_ln2(double x, double& k) {
    k = __builtin_rint(x * 1.4426950408889634);              // v_rndne_f64
    const double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);
    return __builtin_fma(-k, 1.90821492927058770002e-10, r);
}

__device__ __forceinline__ double fe_expm1_neg(double x) {
    x = fmax(x, -800.0);                                     // exp(-800) == 0: result -1
    double k;
    const double p = fe_expm1_reduced(fe_reduce_ln2(x, k));
    const double s = __builtin_ldexp(1.0, (int)k);           // 2^k, k <= 0
    return __builtin_fma(s, p, s - 1.0);                     // k = 0: exactly p
}
// fp32 routines.  Same scheme, re-cut for what the fp32 VALU is good at (round 3; each step measured on the fused
// config-5 shard, profiles/r03/ab_variants.txt):
//   * expm1(r) = r + r^2 Q(r) with Q the DEGREE-4 interpolant of (expm1(r) - r)/r^2 at the Chebyshev nodes of
//     |r| <= ln2/2 (2.3e-8 relative — the degree-5 Taylor polynomial it replaces had 1.8e-8 — one FMA fewer per call);
//   * the reduction x = k ln2 + r takes k from the magic-number add u = fma(x, log2 e, 1.5 * 2^23) (round to nearest even
//     in the add itself), k = u - magic, and builds 2^k from u's low mantissa bits with one integer shift-add — no
//     v_rndne / v_cvt / v_ldexp; the argument is clamped at -87 so that 2^k stays a normal float (expm1 is -1 below -17);
//   * exp (the alpha closure) uses the hardware 2^t (v_exp_f32, 1 ulp) on t = x log2(e) with the product's rounding
//     error and the low part of log2(e) folded back in: exp(x) = 2^t (1 + lo ln2), six instructions instead of fourteen.
// All within 2 ulp(float) of the exact value over the model's ranges (tests/test_engine_gpu.py on random draws and
// tests/test_math_edges_gpu.py at every reduction tie, split, clamp and range end, through fiveeq_math_probe_f32).
__device__ __forceinline__ float fe_expm1_reduced(float r) {
    float q = 0x1.6d10fcp-10f;
    q = __builtin_fmaf(q, r, 0x1.120b62p-7f);
    q = __builtin_fmaf(q, r, 0x1.55551ap-5f);
    q = __builtin_fmaf(q, r, 0x1.5554dep-3f);
    q = __builtin_fmaf(q, r, 0.5f);
    return __builtin_fmaf(r * r, q, r);
}
constexpr float F32_LOG2E = 1.44269504088896341f;
constexpr float F32_LN2 = 0.693147182f;
constexpr float F32_RINT_MAGIC = 12582912.0f;                // 1.5 * 2^23
// 2^k for the integer k held in the low mantissa bits of u = 1.5 * 2^23 + k, -126 <= k <= 0: (bits(u) << 23) + bits(1.0f),
// one v_lshl_add_u32.  Written as inline asm: as plain C++ the packed form below was MISCOMPILED by hipcc 7.2 (the shift-add
// of the second component was dropped and the first component's 2^k used for both members; found by the packed-vs-scalar
// probe test).  Not volatile: the scheduler may still move it.
__device__ __forceinline__ float fe_exp2_from_magic(float u) {
    float s;
    asm("v_lshl_add_u32 %0, %1, 23, 1.0" : "=v"(s) : "v"(u));
    return s;
}
__device__ __forceinline__ float fe_expm1_neg(float x) {
    x = fmaxf(x, -87.0f);                                    // k >= -126
    const float u = __builtin_fmaf(x, F32_LOG2E, F32_RINT_MAGIC);      // magic + rint(x log2 e)
    const float k = u - F32_RINT_MAGIC;
    // ONE fma for the reduction: ln2's own rounding error enters the result as 2^k |k| 2^-26 <= 1e-8 absolute on a result of
    // magnitude >= 0.29 whenever k != 0 (and not at all for k = 0): 0.3 ulp at worst, where exp() proper would need the
    // two-step Cody-Waite form.  Same 1.01 ulp maximum over the probe ranges; one instruction fewer on each of six calls.
    const float r = __builtin_fmaf(-k, F32_LN2, x);
    const float p = fe_expm1_reduced(r);
    const float s = fe_exp2_from_magic(u);
    return __builtin_fmaf(s, p, s - 1.0f);                   // k = 0: exactly p
}

// exp(x) for the alpha closure.  The argument is clamped to +-700 so that alpha is always a
// finite normal number (e^+-700 ~ 1e+-304) and the Newton reciprocal below is always valid.
__device__ __forceinline__ double fe_exp(double x) {
    x = fmin(fmax(x, -700.0), 700.0);
    double k;
    const double p = fe_expm1_reduced(fe_reduce_ln2(x, k));
    return __builtin_ldexp(1.0 + p, (int)k);
}
constexpr float F32_LOG2E_HI = 0x1.715476p+0f;               // log2(e) rounded to float, and what it leaves
constexpr float F32_LOG2E_LO = 0x1.4ae0cp-26f;
__device__ __forceinline__ float fe_exp(float x) {
    x = fminf(fmaxf(x, -80.0f), 80.0f);                      // alpha stays a finite normal float
    const float t = x * F32_LOG2E_HI;
    float lo = __builtin_fmaf(x, F32_LOG2E_HI, -t);          // the product's rounding error, exactly
    lo = __builtin_fmaf(x, F32_LOG2E_LO, lo);
    const float e = __builtin_amdgcn_exp2f(t);               // v_exp_f32
    return __builtin_fmaf(e, lo * F32_LN2, e);
}

// 1/a for finite normal a > 0 (alpha): v_rcp_f64 seed + two Newton steps (<= 1 ulp), without the
// scale / fixup sequence a full IEEE division needs for subnormal and infinite operands.
__device__ __forceinline__ double fe_rcp(double a) {
    double y = __builtin_amdgcn_rcp(a);
    double e = __builtin_fma(-a, y, 1.0);
    y = __builtin_fma(y, e, y);
    e = __builtin_fma(-a, y, 1.0);
    return __builtin_fma(y, e, y);
}
__device__ __forceinline__ float fe_rcp(float a) {
    return __builtin_amdgcn_rcpf(a);                         // v_rcp_f32: 1 ulp.  (A Newton step on top, <= 0.5 ulp, was 2 % of the
}                                                            // fused fp32 kernel and moved no fp32-vs-fp64 figure: r03/ab_variants.txt)

// ln(x) for finite normal x > 0 (a concentration ratio).  The classic fdlibm scheme:
// x = 2^k (1+f) with sqrt(1/2) <= 1+f < sqrt(2);  s = f/(2+f);  ln(1+f) = f - f^2/2 + s (f^2/2 + R(s^2))
// with R the degree-7 minimax polynomial in s^2 (Lg1..Lg7, |error| < 2^-58.45), and k ln2 added in
// hi/lo parts.  The quotient uses the Newton reciprocal (2+f is in [1.7, 2.42]).  ~35 VALU ops against
// ~95 for the general device-library routine, which carries double-double arithmetic and
// special-case selects this argument range never needs.
__device__ __forceinline__ double fe_log(double x) {
    double m = __builtin_amdgcn_frexp_mant(x);                   // [0.5, 1)
    int k = __builtin_amdgcn_frexp_exp(x);
    const bool low = m < 0.70710678118654752440;
    m = low ? m + m : m;                                         // [sqrt(1/2), sqrt(2))
    k = low ? k - 1 : k;
    const double dk = (double)k;
    const double f = m - 1.0;
    const double s = f * fe_rcp(2.0 + f);
    const double z = s * s;
    const double w = z * z;
    double t1 = __builtin_fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01);   // Lg6, Lg4
    t1 = __builtin_fma(w, t1, 3.999999999940941908e-01);                                 // Lg2
    t1 = w * t1;
    double t2 = __builtin_fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01);   // Lg7, Lg5
    t2 = __builtin_fma(w, t2, 2.857142874366239149e-01);                                 // Lg3
    t2 = __builtin_fma(w, t2, 6.666666666666735130e-01);                                 // Lg1
    const double R = __builtin_fma(z, t2, t1);
    const double hfsq = 0.5 * f * f;
    const double tail = __builtin_fma(dk, 1.90821492927058770002e-10, s * (hfsq + R));  // + k ln2_lo
    return __builtin_fma(dk, 6.93147180369123816490e-01, -((hfsq - tail) - f));          // k ln2_hi - ...
}
// fp32 log: ln(x) = ln2 * log2(x) with the hardware log2 (v_log_f32).  Measured on gfx950 (tools/microbench/hw_log_accuracy.hip,
// profiles/r03/hw_log_accuracy.txt): v_log_f32 is within 1 ulp of log2(x) over [0.5, 16] AND right next to 1 (x in
// [1, 1 + 1e-5]: 0.92 ulp of a result of ~1e-6 — no loss of relative accuracy where ln x -> 0, which is where the CO2 forcing
// starts), and it returns exactly 0 at x = 1.  The product with ln2 = hi + lo carries the rounding error of t * hi along:
// <= 2.1 ulp of ln(x), mean 0.55.  Five instructions per member where the frexp + division + polynomial form above took
// twenty (fdlibm's, < 1 ulp): the forcing's log was 9 % of the fused fp32 kernel (r03/ab_variants.txt section 16).
constexpr float F32_LN2_H = 0x1.62e430p-1f;                  // ln2 rounded to float, and what it leaves
constexpr float F32_LN2_L = -0x1.05c610p-29f;
__device__ __forceinline__ float fe_log(float x) {
    const float t = __builtin_amdgcn_logf(x);
    const float p = t * F32_LN2_H;
    const float e = __builtin_fmaf(t, F32_LN2_H, -p);
    return p + __builtin_fmaf(t, F32_LN2_L, e);
}

// sqrt(x) for finite normal x > 0 (a concentration): v_rsq_f64 seed, one Goldschmidt step and a
// final residual correction (<= 1 ulp; a second Goldschmidt step was redundant), without the rescaling a
// full sqrt needs near the ends of the exponent range.  (Also tried in round 2 and not kept: magic-number
// rint + integer-built 2^k in the exp core — 6 fewer VALU per step but +4 VGPRs: 7 -> 6 waves/SIMD in the
// per-step kernel.)
__device__ __forceinline__ double fe_sqrt(double x) {
    const double y = __builtin_amdgcn_rsq(x);                // >= 23 good bits
    double g = x * y;
    double h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);              // one Goldschmidt step: ~2^-45
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-g, g, x);                // residual (Newton) correction: quadratic again
    return __builtin_fma(d, h, g);
}
__device__ __forceinline__ float fe_sqrt(float x) {
    return __builtin_amdgcn_sqrtf(x);                        // v_sqrt_f32: 1 ulp for normal x > 0
}
__device__ __forceinline__ double fe_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float fe_min(float a, float b) { return fminf(a, b); }

// ---- packed fp32 twins (two members per lane): the same operations in the same order as the float routines above ----
__device__ __forceinline__ float2v fe_min(float2v a, float b) { return float2v{fminf(a.x, b), fminf(a.y, b)}; }
__device__ __forceinline__ float2v fe_expm1_reduced(float2v r) {
    float2v q = (float2v)0x1.6d10fcp-10f;
    q = fe_fma(q, r, (float2v)0x1.120b62p-7f);
    q = fe_fma(q, r, (float2v)0x1.55551ap-5f);
    q = fe_fma(q, r, (float2v)0x1.5554dep-3f);
    q = fe_fma(q, r, (float2v)0.5f);
    return fe_fma(r * r, q, r);
}
__device__ __forceinline__ float2v fe_expm1_neg(float2v x) {
    x = float2v{fmaxf(x.x, -87.0f), fmaxf(x.y, -87.0f)};
    const float2v u = fe_fma(x, (float2v)F32_LOG2E, (float2v)F32_RINT_MAGIC);
    const float2v k = u - F32_RINT_MAGIC;
    const float2v r = fe_fma(-k, (float2v)F32_LN2, x);
    const float2v p = fe_expm1_reduced(r);
    const float2v s = float2v{fe_exp2_from_magic(u.x), fe_exp2_from_magic(u.y)};
    return fe_fma(s, p, s - 1.0f);
}
__device__ __forceinline__ float2v fe_exp(float2v x) {
    x = float2v{fminf(fmaxf(x.x, -80.0f), 80.0f), fminf(fmaxf(x.y, -80.0f), 80.0f)};
    const float2v t = x * F32_LOG2E_HI;
    float2v lo = fe_fma(x, (float2v)F32_LOG2E_HI, -t);
    lo = fe_fma(x, (float2v)F32_LOG2E_LO, lo);
    const float2v e = float2v{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    return fe_fma(e, lo * F32_LN2, e);
}
__device__ __forceinline__ float2v fe_rcp(float2v a) {
    return float2v{__builtin_amdgcn_rcpf(a.x), __builtin_amdgcn_rcpf(a.y)};
}
__device__ __forceinline__ float2v fe_log(float2v x) {
    const float2v t = float2v{__builtin_amdgcn_logf(x.x), __builtin_amdgcn_logf(x.y)};
    const float2v p = t * F32_LN2_H;
    const float2v e = fe_fma(t, (float2v)F32_LN2_H, -p);
    return p + fe_fma(t, (float2v)F32_LN2_L, e);
}
__device__ __forceinline__ float2v fe_sqrt(float2v x) {
    return float2v{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)};
}

}  // namespace fiveeq
