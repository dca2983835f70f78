// fiveeq_member.hpp — one member, one step: member_step(), the misfit update, and what the stepping kernels share around them.
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// One member, one step.  All state lives in registers; the caller moves it.
//   drv : this step's drive record (LDS): [0..2] E_g, [3..5] cumE_g, [6] F_ext
//   rr  : per-member r0,rC,rT per gas ;  qq: per-member q_1,q_2
//   R,S : in/out ;  C[g], Tnew: outputs
// Every loop has compile-time bounds and is fully unrolled: arrays stay in VGPRs.
//
// INV = true is the concentration-driven (inverse) form: drv[g] holds the TARGET concentration
// at the end of the step, the member's cumulative emissions cum[g] are per-member state, and
// the emission rate that reaches the target is diagnosed from the same pool equations
//     C* - C0 = sum_i R_i (1 + em1_i) - E alpha sum_i (a_i tau_i c) em1_i
// and returned in out[g]; the pools are then advanced with that E.
// ---------------------------------------------------------------------------------
// V is the lane value type (double, float, or float2v = two members per lane); S its scalar type: the shared model and
// the drive record are S, everything per member is V.
//
// COMP = true is the COMPENSATED fp32 form (round 6; opt-in, register-resident kernels only — fiveeq_run_fused_comp_f32):
//   * every POOL carries a second word (Rlo): the rounding error of its own update, fed back into the next one —
//     y = fma(em1, x, lo); t = R + y; lo = y - (t - R); R = t (Kahan's summation with the product fused into the first add);
//     three more instructions per pool and step, no HBM bytes (the words live and die in registers).  The thermal boxes are NOT
//     compensated: with the forcing below their rounding is 4e-7 of T, and their six instructions were 2.5 % of the kernel;
//   * the forcing is computed from the EXCESS sumN = C - C0 instead of from the rounded C: ln(C/C0) = log1p(x), x = sumN / C0, as
//     ln(u) + (x - (u - 1)) with u = fl(1 + x) (the correction's own 1/u is dropped: it matters only where u ~ 1, where it is 1),
//     and sqrt C - sqrt C0 = sumN / (sqrt C + sqrt C0).  In fp32 the default form loses the small excess of the first decades to
//     the rounding of C itself (ulp(278 ppm) = 3e-5 ppm against an excess of 1e-2 ppm: a forcing good to 1e-3 relative) — that,
//     not the state, is what bounds T in fp32.
// Against 50-digit arithmetic over the 24 golden members: C 2.9e-6 -> 1.4e-7, T 1.7e-5 -> 7e-7 (profiles/r06/fp32_compensated.txt).
// It is its own arithmetic: NOT bit-identical to the default forms, and the per-step kernels (state in HBM) do not have it.
// THE FORCING OF ONE GAS from its concentration (step_forc): f2 (C - C0), then the f1 log and the f3 sqrt term, each behind a
// wave-uniform test of its coefficient (terms whose coefficient is zero are skipped) and the C > 0 guard — for C <= 0 and NaN the
// log term is dropped and sqrt C reads 0.  Written ONCE: gas_step() below calls it for every non-compensated form, and the
// forcing-rows pass (fiveeq_forcrows.hpp) recomputes a run's forcing from its stored C rows with it, so the two cannot drift
// apart.  Scalar lanes and packed lanes spell the selects differently and give the same bits per member.
template <typename V>
__device__ __forceinline__ V gas_forcing(const KGas<typename Lane<V>::S>& kg, const V Cg) {
    using S = typename Lane<V>::S;
    const auto pos = fe_gt0(Cg);
    V Fg = kg.f2 * (Cg - kg.C0);
    if constexpr (Lane<V>::W == 1) {
        if (kg.f1 != S(0)) Fg = pos ? fe_fma(kg.f1, fe_log(pos ? Cg * kg.inv_C0 : S(1)), Fg) : Fg;
        if (kg.f3 != S(0)) Fg = fe_fma(kg.f3, (pos ? fe_sqrt(pos ? Cg : S(1)) : S(0)) - kg.sqrtC0, Fg);
    } else {
        if (kg.f1 != S(0)) Fg = fe_sel(pos, fma3<V>(kg.f1, fe_log(fe_sel(pos, Cg * kg.inv_C0, (V)S(1))), Fg), Fg);
        if (kg.f3 != S(0)) Fg = fma3<V>(kg.f3, fe_sel(pos, fe_sqrt(fe_sel(pos, Cg, (V)S(1))), (V)S(0)) - kg.sqrtC0, Fg);
    }
    return Fg;
}

template <typename V, typename L, int g, bool INV, bool COMP = false, int OWN = 0>
__device__ __forceinline__ V gas_step(const KModel<typename Lane<V>::S>& km, const KGas<typename Lane<V>::S>& kg,
                                      const typename Lane<V>::S* __restrict__ drv, const V (&rr)[3 * L::G], const V T_old,
                                      V (&R)[L::SP], V (&out)[L::G], V (&cum)[L::G], V (&Rlo)[L::SP]) {
    using S = typename Lane<V>::S;
    static_assert(!INV || Lane<V>::W == 1, "the concentration-driven form has no packed instantiation");
    static_assert(!COMP || (!INV && sizeof(S) == 4), "the compensated form is an fp32 form of the emission-driven step");
    constexpr int P = L::pools(g);
    constexpr int o = L::off(g);
    // --- alpha_val -----------------------------------------------------------------
    V sumR = R[o];
#pragma unroll
    for (int i = 1; i < P; ++i) sumR += R[o + i];
    const V G_a = sumR * kg.inv_c;
    V G_u;
    if constexpr (INV) G_u = cum[g] - G_a;
    else G_u = drv[3 + g] - G_a;
    // (skipping the ra and f2 terms behind wave-uniform tests of those coefficients — zero in most default gases — was
    // tried: 8 fewer instructions per member-step and +2.5 % fused fp32 / +3 % fused fp64; the branches cost more than
    // they save, r03/ab_variants.txt)
    V iirf = fma3<V>(kg.ra, G_a, fma3<V>(rr[3 * g + 2], T_old, fma3<V>(rr[3 * g + 1], G_u, rr[3 * g])));
    iirf = fe_min(iirf, km.iirf_max);
    const V alpha = kg.g0 * fe_exp(iirf * kg.inv_g1);
    const V inv_alpha = fe_rcp(alpha);
    // --- step_conc -----------------------------------------------------------------
    V em1[P];
#pragma unroll
    for (int i = 0; i < P; ++i) em1[i] = fe_expm1_neg(kg.ndt_over_tau[i] * inv_alpha);
    V E;
    if constexpr (INV) {
        V num = V(0), den = V(0);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            num += fe_fma(R[o + i], em1[i], R[o + i]);
            den = fe_fma(kg.atc[i], em1[i], den);
        }
        E = (num - (drv[g] - kg.C0)) / (alpha * den);
        cum[g] = fe_fma(E, km.dt, cum[g]);
        out[g] = E;
    } else {
        E = (V)drv[g];
    }
    const V Ea = E * alpha;
    V sumN = (V)S(0);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const V Ri = R[o + i];
        V Rn;
        if constexpr (COMP) {
            const V y = fe_fma(em1[i], fma3<V>(-kg.atc[i], Ea, Ri), Rlo[o + i]);     // the increment plus what earlier sums dropped
            Rn = Ri + y;
            Rlo[o + i] = y - (Rn - Ri);                                            // what THIS sum dropped
        } else {
            Rn = fe_fma(em1[i], fma3<V>(-kg.atc[i], Ea, Ri), Ri);         // R + em1 (R - a tau c E alpha)
        }
        R[o + i] = Rn;
        sumN += Rn;
    }
    const V Cg = kg.C0 + sumN;
    if constexpr (!INV) out[g] = Cg;
    // --- step_forc: gas_forcing() above; the compensated form takes it from the excess sumN instead ---
    if constexpr (COMP) {
        const auto pos = fe_gt0(Cg);
        V Fg = kg.f2 * sumN;
        if (kg.f1 != S(0)) {
            const V x = sumN * kg.inv_C0;                                          // C / C0 - 1, to the precision of the excess
            const V u = fe_sel(pos, (V)S(1) + x, (V)S(1));
            const V lg = fe_log(u) + (x - (u - (V)S(1)));                          // log1p(x)
            Fg = fe_sel(pos, fma3<V>(kg.f1, lg, Fg), Fg);
        }
        if (kg.f3 != S(0)) {
            const V den = fe_sqrt(fe_sel(pos, Cg, (V)S(1))) + kg.sqrtC0;
            Fg = fma3<V>(kg.f3, fe_sel(pos, sumN * fe_rcp(den), (V)(-kg.sqrtC0)), Fg);
        }
        return Fg;
    } else {
        return gas_forcing<V>(kg, Cg);
    }
}

// FORC = true (round 8) is the form with PER-MEMBER FORCING SCALES: the member carries G + K factors, sg_g per gas and sx_k per
// external forcing category (0 <= K <= MAX_FEXT), and the run a shared table X [n_steps][MAX_FEXT] of category forcings:
//     F = F_ext(t);   F = fma(sx_k, X[t][k], F), k = 0 .. K-1;   F = fma(sg_g, F_g, F), g = 0 .. G-1
// with F_g exactly what gas_step() returns.  fma(1, F_g, F) is F + F_g with the same single rounding, so unit scales with
// K = 0 (or an all-zero table) give the bits of the plain step.  Scale j of the lane is fs[j * fs_stride] (gas rows first:
// registers with stride 1, or a lane-private LDS slot), xr the step's table record (wave-uniform), n_fext = K is
// wave-uniform: the category loop is scalar branches.  Nothing else of the step differs; FORC = false is the code as it was.
// With INV (the concentration-driven form) the gas step is the inverse one as it stands — gas_step() does not know FORC — and F
// is accumulated in exactly this way from the forcing of the concentrations the diagnosed emissions reach.
// OWN (gas_step() too) changes no code: it is a tag that gives the INV forms with FORC or MISFIT instantiations of the two step
// functions that no other kernel shares.  Sharing gas_step<.., INV = true> with the plain INV kernel of the same layout moved
// that kernel's instruction schedule (the same instructions in another order); with the tag every kernel that existed keeps
// its machine code (profiles/r24/inverse_forcing_isa.txt).
// AFTER-GAS HOOK (round 18): after_gas(GasTag<g>{}) is called once gas g's pools R[off(g) ..], its out[g] and its share of F
// are final and before the next gas's arithmetic starts — the per-step kernels store that gas's rows there (step_body).  The
// hook touches no value of the step: the arithmetic, its order and its roundings are those of the unhooked call, and the
// default NoGasHook compiles to nothing (every kernel that does not pass one keeps its machine code).
constexpr int MAX_FEXT = 4;
template <int g>
struct GasTag {
    static constexpr int value = g;
};
struct NoGasHook {
    template <int g>
    __device__ __forceinline__ void operator()(GasTag<g>) const {}
};
// MFORC = true (with FORC): the member also carries its OWN forcing series, one value per step (member_forcing rows, mf): the
// step opens F = drive[t][6] + mf — one add — and goes on with the category and gas fmas exactly as FORC does.  A zero mf gives
// the FORC step bit for bit (x + 0 = x for every x but -0).  MFORC = false is the code as it was.
// CM is the PER-GAS DRIVE MASK: bit g set = gas g is concentration-driven (gas_step<.., g, INV = true>: its target is drv[g], its
// cumulative emissions cum[g] the member's own, out[g] = E), bit g clear = emission-driven (the forward gas step: drv[g] = E_g,
// drv[3 + g] the shared cumulative emissions before the step, cum[g] neither read nor written, out[g] = C_g).  The default is what
// INV alone meant — every gas or none — so every call that does not name it instantiates the step functions it did; a proper
// mask (the mixed drive, fused_mixed_kernel) comes with an OWN value of its own, so that it shares no instantiation of the two
// step functions with a kernel that existed (see OWN above).  F, the forcing fmas and the thermal step do not know the mask.
template <typename V, typename L, bool INV, bool COMP, bool FORC = false, typename Hook = NoGasHook, int OWN = 0, bool MFORC = false,
          int CM = (INV ? (1 << L::G) - 1 : 0)>
__device__ __forceinline__ void member_step(const KModel<typename Lane<V>::S>& km, const typename Lane<V>::S* __restrict__ drv,
                                            const V (&rr)[3 * L::G], const V (&qq)[2],
                                            V (&R)[L::SP], V (&S)[2], V (&out)[L::G], V& Tnew, V (&cum)[L::G],
                                            V (&Rlo)[L::SP], const V* fs = nullptr, const int fs_stride = 1,
                                            const typename Lane<V>::S* xr = nullptr, const int n_fext = 0,
                                            const Hook after_gas = Hook{}, const V mf = V()) {
    static_assert(!FORC || !COMP, "the forcing scales are not carried by the compensated form");
    static_assert(!MFORC || (FORC && !INV), "the per-member forcing row is carried by the forward forcing-scale forms only");
    static_assert(CM >= 0 && CM < (1 << L::G) && (INV || CM == 0), "a drive mask names gases of the layout, and a forward step none");
    const V T_old = S[0] + S[1];
    V F = (V)drv[6];
    if constexpr (MFORC) F = F + mf;
    if constexpr (FORC) {
#pragma unroll
        for (int k = 0; k < MAX_FEXT; ++k)
            if (k < n_fext) F = fma3<V>(fs[(L::G + k) * fs_stride], xr[k], F);
    }
    // compiler-only barriers: keep each gas's LDS constant reads inside that gas's code instead of all
    // ~45 being hoisted to the kernel top (VGPR pressure) or out of the fused time loop.  (Issuing gas
    // g+1's reads before gas g's arithmetic was tried: +-1 %, 133 VGPRs; not kept.)
    asm volatile("" ::: "memory");
    const V F0 = gas_step<V, L, 0, bool(CM >> 0 & 1), COMP, OWN>(km, km.gas[0], drv, rr, T_old, R, out, cum, Rlo);
    if constexpr (FORC) F = fe_fma(fs[0 * fs_stride], F0, F);
    else F += F0;
    after_gas(GasTag<0>{});
    if constexpr (L::G > 1) {
        asm volatile("" ::: "memory");
        const V F1 = gas_step<V, L, 1, bool(CM >> 1 & 1), COMP, OWN>(km, km.gas[1], drv, rr, T_old, R, out, cum, Rlo);
        if constexpr (FORC) F = fe_fma(fs[1 * fs_stride], F1, F);
        else F += F1;
        after_gas(GasTag<1>{});
    }
    if constexpr (L::G > 2) {
        asm volatile("" ::: "memory");
        const V F2 = gas_step<V, L, 2, bool(CM >> 2 & 1), COMP, OWN>(km, km.gas[2], drv, rr, T_old, R, out, cum, Rlo);
        if constexpr (FORC) F = fe_fma(fs[2 * fs_stride], F2, F);
        else F += F2;
        after_gas(GasTag<2>{});
    }
    // --- step_temp: S + em1_d (S - q F) ------------------------------------------------
#pragma unroll
    for (int j = 0; j < 2; ++j) S[j] = fma3<V>(km.em1_d[j], fe_fma(-qq[j], F, S[j]), S[j]);
    Tnew = S[0] + S[1];
}
template <typename V, typename L, bool INV = false>
__device__ __forceinline__ void member_step(const KModel<typename Lane<V>::S>& km, const typename Lane<V>::S* __restrict__ drv,
                                            const V (&rr)[3 * L::G], const V (&qq)[2],
                                            V (&R)[L::SP], V (&S)[2], V (&out)[L::G], V& Tnew, V (&cum)[L::G]) {
    V no_Rlo[L::SP];                                     // never touched: COMP = false
    member_step<V, L, INV, false>(km, drv, rr, qq, R, S, out, Tnew, cum, no_Rlo);
}
template <typename V, typename L>
__device__ __forceinline__ void member_step(const KModel<typename Lane<V>::S>& km, const typename Lane<V>::S* __restrict__ drv,
                                            const V (&rr)[3 * L::G], const V (&qq)[2],
                                            V (&R)[L::SP], V (&S)[2], V (&C)[L::G], V& Tnew) {
    V unused[L::G];
    member_step<V, L, false>(km, drv, rr, qq, R, S, C, Tnew, unused);
}

// ---------------------------------------------------------------------------------
// THE MISFIT UPDATE (round 7, ABI v12): one member's running misfit against an observed series, three fp64 accumulators
// A, U, V per member.  obs [n_steps][4] fp64 holds per step (o_t, p_t = 1/sigma_t^2 or 0, b_t = 1/n_ref inside the
// reference period or 0, 0); Tw is the member's T after the step, widened exactly.  Every operation is rounded on its
// own (contraction is off in this file, no fma is written): every kernel that carries the accumulators calls this one
// function, so every form gives the same bits.  A step with p_t == 0 && b_t == 0 is skipped by the caller (the rows are
// not touched), in every form alike.  The host then scores chi2 = V - 2 A U + A^2 P, P = sum_t p_t.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ void misfit_update(const double o, const double p, const double b, const double Tw, double& A,
                                              double& U, double& Vq) {
    A = A + b * Tw;
    const double d = Tw - o;
    const double pd = p * d;
    U = U + pd;
    Vq = Vq + pd * d;
}
// the lane's members: one (scalar lanes) or two (packed lanes); Tw of member j of the lane
__device__ __forceinline__ double lane_member(const double v, int) { return v; }
__device__ __forceinline__ double lane_member(const float v, int) { return (double)v; }
__device__ __forceinline__ double lane_member(const float2v v, int j) { return (double)(j == 0 ? v.x : v.y); }

// The shared model is the FIRST kernel argument (by value): its bytes sit at offset 0 of the
// kernarg segment.  With ~45 fp64 constants per 3-gas layout plus the polynomial literals it does
// not fit the 102-SGPR budget (118 SGPR spills -> v_readlane/v_writelane in the VALU stream), so
// each workgroup copies it once into LDS and the lanes read it back with broadcast ds_reads,
// which issue beside the VALU instead of in it.
template <typename T>
__device__ __forceinline__ void stage_model(KModel<T>* dst) {
    constexpr int NW = sizeof(KModel<T>) / sizeof(T);
    const T* src = (const T*)__builtin_amdgcn_kernarg_segment_ptr();
    for (int i = threadIdx.x; i < NW; i += FIVEEQ_BLOCK) reinterpret_cast<T*>(dst)[i] = src[i];
}

// Row access of a lane: one element (scalar lanes) or two consecutive elements as ONE 8-byte access (packed lanes; the
// host guarantees even row strides and 8-byte aligned rows before it picks a packed kernel).  `full` = both members of
// a packed lane exist; the last lane of an odd ensemble stores its first member only.
template <typename V>
__device__ __forceinline__ V load_lane(const typename Lane<V>::S* p) { return *reinterpret_cast<const V*>(p); }
__device__ __forceinline__ void store_lane(double* p, double v, bool) { *p = v; }
__device__ __forceinline__ void store_lane(float* p, float v, bool) { *p = v; }
__device__ __forceinline__ void store_lane(float* p, float2v v, bool full) {
    if (full) *reinterpret_cast<float2v*>(p) = v;
    else *p = v.x;
}
// The same with the NON-TEMPORAL policy (NT = true): rows that are read or written once per pass over an ensemble far larger
// than the Infinity Cache, where keeping them resident cannot pay (step_kernel's STREAM form).
template <typename V, bool NT>
__device__ __forceinline__ V load_row(const typename Lane<V>::S* p) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
    else return load_lane<V>(p);
}
template <bool NT, typename S, typename V>
__device__ __forceinline__ void store_row(S* p, V v, bool full) {
    if constexpr (!NT) store_lane(p, v, full);
    else if constexpr (sizeof(V) == sizeof(S)) __builtin_nontemporal_store(v, p);
    else {
        if (full) __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
        else __builtin_nontemporal_store(v.x, p);
    }
}

// One misfit step of the lane's member(s) (misfit_update()).  ob is the step's obs record: wave-uniform, read with scalar
// loads, so the window test is a scalar branch; on a step outside the window (p_t == 0 && b_t == 0) the accumulators are
// neither read nor written.  Word k of member j of the lane is acc[j * mem_stride + k * word_stride]: misfit [3][ld] in HBM
// (strides 1, ld) or the fused kernel's lane-private LDS slots [3 W][FIVEEQ_BLOCK] (strides 3 FIVEEQ_BLOCK, FIVEEQ_BLOCK).
// full = false skips a packed lane's missing second member; the LDS carrier passes true (there the missing member shadows
// the first one and is never stored).
template <typename V>
__device__ __forceinline__ void misfit_step(const double* ob, const V Tn, double* acc, const int64_t mem_stride,
                                            const int64_t word_stride, const bool full) {
    const double o_t = ob[0], p_t = ob[1], b_t = ob[2];
    if (p_t != 0.0 || b_t != 0.0) {
#pragma unroll
        for (int j = 0; j < Lane<V>::W; ++j) {
            if (j == 0 || full) {
                double* a = acc + j * mem_stride;
                double A = a[0], U = a[word_stride], Vq = a[2 * word_stride];
                misfit_update(o_t, p_t, b_t, lane_member(Tn, j), A, U, Vq);
                a[0] = A;
                a[word_stride] = U;
                a[2 * word_stride] = Vq;
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// THE LANE'S MEMBER SPAN, written here once for step_kernel, step_scen_kernel, fused_kernel and small_multi_kernel
// (force-inlined: every kernel's code is what it was when each of them spelt it out, profiles/r10/refactor_digest.txt).
// m is the lane's first member (W consecutive members per lane); active, that member exists; full, every member of the lane
// exists; mm, the member an idle tail lane loads instead — it stores nothing.  The one-wave step kernels park idle lanes on
// the ensemble's last (aligned) lane, PARK_LAST; the register-resident kernels on member 0, PARK_FIRST.
enum Park { PARK_FIRST, PARK_LAST };
struct LaneSpan {
    int64_t m;
    bool active, full;
    int64_t mm;
};
template <int W, int BLOCK, Park PARK>
__device__ __forceinline__ LaneSpan lane_span(const int64_t n) {
    const int64_t m = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * W;
    const bool active = m < n;
    const bool full = m + (W - 1) < n;
    const int64_t mm = active ? m : (PARK == PARK_LAST ? ((n - 1) & ~(int64_t)(W - 1)) : 0);
    return LaneSpan{m, active, full, mm};
}

}  // namespace fiveeq
