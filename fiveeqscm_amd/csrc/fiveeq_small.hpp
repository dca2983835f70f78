// fiveeq_small.hpp — kernels 2c and 2d: small ensembles (small_kernel, small_multi_kernel, small_octet_kernel).
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 2c — SMALL ENSEMBLES: the time-fused step with ONE MEMBER SPREAD OVER A QUAD OF LANES (round 5).
//
// A 10k-member ensemble (BASELINE configs[1]) is 157 waves for 1024 SIMDs: every wave is alone on its SIMD, and a lone
// wave issues one vector instruction per ~3.7-4.2 ns whatever the instruction and however independent its neighbours are
// (tools/microbench/valu_rates.hip, "waves/SIMD 1": 9-10 nominal cycles for v_fma_f64 and for v_mov_b32 alike).  What such
// a run costs is therefore the NUMBER OF INSTRUCTIONS ONE WAVE ISSUES PER STEP — not bytes, not FLOPs, not occupancy — and
// the way to shorten it is to hand parts of a member's step to lanes that would otherwise not exist:
//   * LPM = 4 (layouts with a 4-pool gas and nothing else: CO2-only): lane 4m + i carries POOL i of member m.  Its expm1,
//     its pool update and its slice of the state are the lane's own (one expm1 chain per wave-step instead of four); the
//     alpha closure, the forcing and the thermal boxes are computed by all four lanes alike (redundant lanes are free:
//     the instruction is issued once per wave either way).  The two sums over pools are folded with quad_perm DPP moves
//     in the per-step kernel's order ((R0 + R1) + R2) + R3, every lane of the quad computing the same sum from the same
//     four values: the bits do not change.  4x the waves of the one-member-per-lane form, 16 members per wave;
//   * the shared model is read from the KERNEL ARGUMENT (scalar loads, hoisted out of the time loop) instead of being
//     re-read from LDS every step: with one wave per SIMD the registers are there (512 VGPRs), and an LDS round trip that
//     nothing hides is ~100 cycles of the wave's time;
//   * the step's drive record is read one step AHEAD (LDS, broadcast), so that its latency lies under the previous step.
// LPM = 1 is the same kernel without the spreading (any single-gas layout): what the register-resident constants buy alone.
// Per-wave statistics as in the fused kernel (the same records, bit for bit); no histogram ring: those runs take the fused
// kernel.  Same arithmetic, operation for operation, as member_step(): bit-identical results (tested against the per-step path).
// ---------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ double quad_bcast(const double v) {           // lane 4q + K of every quad, to the whole quad
    // (mov_dpp, not update_dpp: every lane has a source, so there is no "old" value to initialise — 16 v_mov less per step)
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), K * 0x55, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), K * 0x55, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int K>
__device__ __forceinline__ float quad_bcast(const float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), K * 0x55, 0xf, 0xf, true));
}

template <typename T, int P0, int LPM, bool STATS>
__global__ __launch_bounds__(FIVEEQ_SMALL_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2))) void small_kernel(
    const KModel<T> km, const T* __restrict__ drive, const int n_steps, const int t_begin, const int t_end,
    const int64_t n, const int64_t ld, const T* __restrict__ r, const T* __restrict__ q, T* __restrict__ R,
    T* __restrict__ S, T* __restrict__ C_traj /* [n_rows][1][ld] or nullptr */, T* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */) {
    static_assert(LPM == 1 || (LPM == 4 && P0 == 4), "a quad of lanes carries the four pools of one gas");
    static_assert(LPM == 1 || FIVEEQ_SMALL_BLOCK == 256, "quad form: one workgroup = 64 members = one statistics record");
    constexpr int MPB = FIVEEQ_SMALL_BLOCK / LPM;                        // members per workgroup
    __shared__ T drv[FIVEEQ_FUSED_CHUNK * DRIVE_STRIDE];
    __shared__ int row_s[FIVEEQ_FUSED_CHUNK];                            // the steps' output rows, converted once per chunk
    // per-64-member statistics records, batched over STAT_STEPS steps and folded by wave_stats_flush() exactly like the fused
    // kernel's (same tile layout, same order: the same record bits).  One lane per member: a tile per wave.  A quad per member:
    // the workgroup's four waves hold 16 members each = ONE record; they share a tile and wave 0 folds it between two barriers.
    // A compile-time variant (STATS): as a run-time test in the time loop it cost the statistics-free run 10 % (0.415 -> 0.456 us
    // per step at 10k members).
    __shared__ T stat_tile[!STATS ? 1 : (LPM == 1 ? FIVEEQ_SMALL_BLOCK / 64 : 1)][!STATS ? 1 : STAT_STEPS * STAT_ROW];
    const int64_t rec = LPM == 1 ? (int64_t)blockIdx.x * (FIVEEQ_SMALL_BLOCK / 64) + (threadIdx.x >> 6) : (int64_t)blockIdx.x;
    const bool rec_live = STATS && rec < ((n + 63) >> 6);                 // uniform over the wave (LPM = 1) / the workgroup (LPM = 4)
    const int n_valid = (int)min((int64_t)64, n - rec * 64);
    T* const tile = STATS ? stat_tile[LPM == 1 ? threadIdx.x >> 6 : 0] : nullptr;
    int ks = 0;
    const int lane = threadIdx.x;
    const int sub = lane % LPM;                                          // the pool this lane carries (LPM = 4)
    const int64_t m = (int64_t)blockIdx.x * MPB + lane / LPM;
    const bool active = m < n;
    const int64_t mm = active ? m : 0;                                   // idle tail lanes shadow member 0 and store nothing
    const KGas<T>& kg = km.gas[0];                                       // kernel argument: scalar loads, loop-invariant

    T rr[3], qq[2], Sv[2], Rv[LPM == 1 ? P0 : 1];
    T ndt[LPM == 1 ? P0 : 1], natc[LPM == 1 ? P0 : 1];                  // -dt / tau_i and -(a_i tau_i c) of this lane's pool(s)
    if constexpr (LPM == 1) {
#pragma unroll
        for (int i = 0; i < P0; ++i) Rv[i] = R[i * ld + mm], ndt[i] = kg.ndt_over_tau[i], natc[i] = -kg.atc[i];
    } else {
        Rv[0] = R[sub * ld + mm];
        ndt[0] = sub == 0 ? kg.ndt_over_tau[0] : (sub == 1 ? kg.ndt_over_tau[1] : (sub == 2 ? kg.ndt_over_tau[2] : kg.ndt_over_tau[3]));
        natc[0] = -(sub == 0 ? kg.atc[0] : (sub == 1 ? kg.atc[1] : (sub == 2 ? kg.atc[2] : kg.atc[3])));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = S[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 3; ++k) rr[k] = r[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = q[k * ld + mm];
    // LPM = 4: ONE store per step and lane — lane 0 of the quad writes C, lane 1 writes T (its own base pointer; null = this
    // lane stores nothing)
    T* const out_q = !active ? nullptr : (sub == 0 ? (C_traj ? C_traj + m : nullptr) : (sub == 1 ? (T_traj ? T_traj + m : nullptr) : nullptr));

    // the sum over pools of the CURRENT state, in the per-step kernel's order ((R0 + R1) + R2) + R3.  Computed here once; each
    // step's own sum over the NEW pools, (((0 + R0') + R1') + R2') + R3', is then the next step's: the same additions on the
    // same values (0 + x = x), except that a zero may come out with the other sign, which alpha = g0 exp(iIRF / g1) — the
    // sum's only consumer — cannot see.
    T sumR;
    if constexpr (LPM == 1) {
        sumR = Rv[0];
#pragma unroll
        for (int i = 1; i < P0; ++i) sumR += Rv[i];
    } else {
        sumR = quad_bcast<0>(Rv[0]);
        sumR += quad_bcast<1>(Rv[0]);
        sumR += quad_bcast<2>(Rv[0]);
        sumR += quad_bcast<3>(Rv[0]);
    }

    for (int tc = t_begin; tc < t_end; tc += FIVEEQ_FUSED_CHUNK) {
        const int nt = min(FIVEEQ_FUSED_CHUNK, t_end - tc);
        __syncthreads();                                                 // (one wave: the previous chunk is consumed)
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_SMALL_BLOCK) {
            const T v = drive[(int64_t)tc * DRIVE_STRIDE + i];
            drv[i] = v;
            if ((i & (DRIVE_STRIDE - 1)) == 7) row_s[i >> 3] = (int)v;
        }
        __syncthreads();
        T E = drv[0], cumE = drv[3], Fx = drv[6];                        // step tc
        int rowv = row_s[0];
        for (int k = 0; k < nt; ++k) {
            const int kn = k + 1 < nt ? k + 1 : k;                       // the NEXT step's record, asked for now
            const T En = drv[kn * DRIVE_STRIDE], cumEn = drv[kn * DRIVE_STRIDE + 3], Fxn = drv[kn * DRIVE_STRIDE + 6];
            const int rowvn = row_s[kn];
            // ---- member_step(), operation for operation (gas_step<.., g = 0, INV = false>) ----
            const T T_old = Sv[0] + Sv[1];
            const T G_a = sumR * kg.inv_c;
            const T G_u = cumE - G_a;
            T iirf = fe_fma(kg.ra, G_a, fe_fma(rr[2], T_old, fe_fma(rr[1], G_u, rr[0])));
            iirf = fe_min(iirf, km.iirf_max);
            const T alpha = kg.g0 * fe_exp(iirf * kg.inv_g1);
            const T inv_alpha = fe_rcp(alpha);
            const T Ea = E * alpha;
            T sumN = T(0);
            if constexpr (LPM == 1) {
                T em1[P0];
#pragma unroll
                for (int i = 0; i < P0; ++i) em1[i] = fe_expm1_neg(ndt[i] * inv_alpha);
#pragma unroll
                for (int i = 0; i < P0; ++i) {
                    const T Rn = fe_fma(em1[i], fe_fma(natc[i], Ea, Rv[i]), Rv[i]);
                    Rv[i] = Rn;
                    sumN += Rn;
                }
            } else {
                const T em1 = fe_expm1_neg(ndt[0] * inv_alpha);
                const T Rn = fe_fma(em1, fe_fma(natc[0], Ea, Rv[0]), Rv[0]);
                Rv[0] = Rn;
                sumN += quad_bcast<0>(Rn);
                sumN += quad_bcast<1>(Rn);
                sumN += quad_bcast<2>(Rn);
                sumN += quad_bcast<3>(Rn);
            }
            sumR = sumN;
            const T Cg = kg.C0 + sumN;
            const bool pos = Cg > T(0);
            T Fg = kg.f2 * (Cg - kg.C0);
            if (kg.f1 != T(0)) {                                         // gas_step()'s values, selected instead of branched around:
                const T lg = fe_log(pos ? Cg * kg.inv_C0 : T(1));        // straight-line code schedules better in a lone wave (-1...-3 %)
                const T with_log = fe_fma(kg.f1, lg, Fg);
                Fg = pos ? with_log : Fg;
            }
            if (kg.f3 != T(0)) {
                const T sq = fe_sqrt(pos ? Cg : T(1));
                Fg = fe_fma(kg.f3, (pos ? sq : T(0)) - kg.sqrtC0, Fg);
            }
            T F = Fx;
            F += Fg;
#pragma unroll
            for (int j = 0; j < 2; ++j) Sv[j] = fe_fma(km.em1_d[j], fe_fma(-qq[j], F, Sv[j]), Sv[j]);
            const T Tn = Sv[0] + Sv[1];
            // ---- the step's stored rows ----
            const int row = __builtin_amdgcn_readfirstlane(rowv);
            if (row >= 0 && row < n_rows) {
                if constexpr (LPM == 1) {
                    if (active) {
                        if (C_traj != nullptr) C_traj[(int64_t)row * ld + m] = Cg;
                        if (T_traj != nullptr) T_traj[(int64_t)row * ld + m] = Tn;
                    }
                } else {
                    if (out_q != nullptr) out_q[(int64_t)row * ld] = sub == 0 ? Cg : Tn;
                }
            }
            if constexpr (STATS) if (rec_live) {
                if (LPM == 1 || sub == 0) tile[ks * STAT_ROW + (LPM == 1 ? (threadIdx.x & 63) : (threadIdx.x >> 2))] = Tn;
                if (++ks == STAT_STEPS || tc + k + 1 == t_end) {
                    double* const out = stats + (rec * n_steps + (tc + k + 1 - ks)) * 4;
                    if constexpr (LPM == 1) {
                        wave_stats_flush(tile, ks, n_valid, out, 4);
                    } else {
                        __syncthreads();
                        if (threadIdx.x < 64) wave_stats_flush(tile, ks, n_valid, out, 4);
                        __syncthreads();
                    }
                    ks = 0;
                }
            }
            E = En, cumE = cumEn, Fx = Fxn, rowv = rowvn;
        }
    }
    if (active) {
        if constexpr (LPM == 1) {
#pragma unroll
            for (int i = 0; i < P0; ++i) R[i * ld + m] = Rv[i];
#pragma unroll
            for (int k = 0; k < 2; ++k) S[k * ld + m] = Sv[k];
        } else {
            R[sub * ld + m] = Rv[0];
            if (sub < 2) S[sub * ld + m] = sub == 0 ? Sv[0] : Sv[1];
        }
    }
}

// The same for layouts with SEVERAL gases, one member per lane: member_step() itself on a model that lives in registers
// (scalar loads of the kernel argument, hoisted out of the time loop: with at most two waves per SIMD the ~45 constants of
// three gases fit beside the state) and on a drive record held in registers and read one step ahead.  What a launch-bound
// multi-gas ensemble gains over the fused kernel is the LDS round trips per step that nothing hides when a wave is alone on
// its SIMD.  (A quad per gas would carry 4 members per wave: worth it below ~4k members only; not built.)
// COMP = true (fp32 only): the compensated form of gas_step (a compensation word per pool in registers, the forcing from the excess
// C - C0) on this kernel — what a launch-bound fp32 ensemble takes under EnsembleEngine(compensated=True); every layout, the
// single-gas ones included (fiveeq_run_small_comp_f32).
template <typename T, int P0, int P1, int P2, bool STATS, bool COMP = false>
__global__ __launch_bounds__(FIVEEQ_SMALL_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2))) void small_multi_kernel(
    const KModel<T> km, const T* __restrict__ drive, const int n_steps, const int t_begin, const int t_end,
    const int64_t n, const int64_t ld, const T* __restrict__ r, const T* __restrict__ q, T* __restrict__ R,
    T* __restrict__ S, T* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */, T* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */) {
    using L = Layout<P0, P1, P2>;
    __shared__ T drv[FIVEEQ_FUSED_CHUNK * DRIVE_STRIDE];
    __shared__ int row_s[FIVEEQ_FUSED_CHUNK];
    __shared__ T stat_tile[!STATS ? 1 : FIVEEQ_SMALL_BLOCK / 64][!STATS ? 1 : STAT_STEPS * STAT_ROW];     // as in small_kernel, one lane per member
    const int64_t rec = (int64_t)blockIdx.x * (FIVEEQ_SMALL_BLOCK / 64) + (threadIdx.x >> 6);
    const bool rec_live = STATS && rec < ((n + 63) >> 6);
    const int n_valid = (int)min((int64_t)64, n - rec * 64);
    T* const tile = STATS ? stat_tile[threadIdx.x >> 6] : nullptr;
    int ks = 0;
    // fp64: the model, word by word, into VECTOR registers.  Left to itself the compiler keeps the ~45 constants of three
    // gases in scalar registers, runs out of them (two each) and spills — 83 v_readlane per step, 1.25 us per step instead of
    // 0.94 at 10k members (r05/ab_variants.txt section 4).  fp32 constants fit the scalar file and stay there (0.51 against 0.61).
    KModel<T> kl;
    {
        constexpr int NW = sizeof(KModel<T>) / sizeof(T);
        const T* src = reinterpret_cast<const T*>(&km);
        T* dst = reinterpret_cast<T*>(&kl);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            T v = src[i];
            if constexpr (sizeof(T) == 8) asm("" : "+v"(v));             // (not volatile: words of absent gases are dropped)
            dst[i] = v;
        }
    }
    const auto [m, active, full, mm] = lane_span<1, FIVEEQ_SMALL_BLOCK, PARK_FIRST>(n);     // (full == active: one member per lane)
    T rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Cv[L::G], Tn;
    T Rlo[L::SP], no_cum[L::G];                                          // COMP: the compensation words (zero at launch)
    if constexpr (COMP) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) Rlo[k] = T(0);
    }
#pragma unroll
    for (int k = 0; k < L::SP; ++k) Rv[k] = R[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = S[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 3 * L::G; ++k) rr[k] = r[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = q[k * ld + mm];
    for (int tc = t_begin; tc < t_end; tc += FIVEEQ_FUSED_CHUNK) {
        const int nt = min(FIVEEQ_FUSED_CHUNK, t_end - tc);
        __syncthreads();
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_SMALL_BLOCK) {
            const T v = drive[(int64_t)tc * DRIVE_STRIDE + i];
            drv[i] = v;
            if ((i & (DRIVE_STRIDE - 1)) == 7) row_s[i >> 3] = (int)v;
        }
        __syncthreads();
        T cur[DRIVE_STRIDE - 1];
#pragma unroll
        for (int j = 0; j < DRIVE_STRIDE - 1; ++j) cur[j] = drv[j];
        int rowv = row_s[0];
        for (int k = 0; k < nt; ++k) {
            const int kn = k + 1 < nt ? k + 1 : k;                       // the NEXT step's record, asked for now
            T nxt[DRIVE_STRIDE - 1];
#pragma unroll
            for (int j = 0; j < DRIVE_STRIDE - 1; ++j) nxt[j] = drv[kn * DRIVE_STRIDE + j];
            const int rowvn = row_s[kn];
            member_step<T, L, false, COMP>(kl, cur, rr, qq, Rv, Sv, Cv, Tn, no_cum, Rlo);
            const int row = __builtin_amdgcn_readfirstlane(rowv);
            if (row >= 0 && row < n_rows && active) {
                if (C_traj != nullptr) {
                    T* c = C_traj + (int64_t)row * L::G * ld + m;
#pragma unroll
                    for (int g = 0; g < L::G; ++g) c[g * ld] = Cv[g];
                }
                if (T_traj != nullptr) T_traj[(int64_t)row * ld + m] = Tn;
            }
            if constexpr (STATS) if (rec_live) {
                tile[ks * STAT_ROW + (threadIdx.x & 63)] = Tn;
                if (++ks == STAT_STEPS || tc + k + 1 == t_end) {
                    wave_stats_flush(tile, ks, n_valid, stats + (rec * n_steps + (tc + k + 1 - ks)) * 4, 4);
                    ks = 0;
                }
            }
#pragma unroll
            for (int j = 0; j < DRIVE_STRIDE - 1; ++j) cur[j] = nxt[j];
            rowv = rowvn;
        }
    }
    if (active) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) R[k * ld + m] = Rv[k];
#pragma unroll
        for (int k = 0; k < 2; ++k) S[k * ld + m] = Sv[k];
    }
}

// ---------------------------------------------------------------------------------
// Kernel 2d — SMALL MULTI-GAS ENSEMBLES: one member per OCTET of lanes (round 6; layout 4 + 1 + 1, the default three-gas set).
//
// The quad idea of small_kernel carried to three gases: lanes 0-3 of an octet hold the four pools of gas 0, lane 4 the pool of
// gas 1, lane 5 the pool of gas 2 (lanes 6, 7 shadow lane 5 and store nothing).  Every lane runs ONE alpha closure, ONE expm1
// chain, ONE pool update and ONE forcing — its own gas's, with that gas's constants selected into registers once — where the
// one-member-per-lane form (small_multi_kernel) runs three closures, six expm1 chains and three forcings per wave-step: a third
// of the instructions per wave, on 8x the waves.  What crosses lanes, all of it DPP moves inside a row of 16 lanes:
//   * gas 0's sum over pools, folded inside its quad in member_step()'s order (((0 + R0) + R1) + R2) + R3; a single-pool gas's
//     sum is 0 + R, lane-local; one select between the two;
//   * the three forcings: quad_perm broadcasts lane 0 / lane 1 of every quad (quad 0: F_0, F_0; quad 1: F_1, F_2), row_shr:4 /
//     row_shl:4 under a bank mask carry them into the other quad, and every lane adds F_ext + F_0 + F_1 + F_2 in that order.
// The thermal boxes are computed by all eight lanes alike.  Same operations on the same values in the same order as
// member_step(): bit-identical results (tested against the per-step path, fp64 and fp32).  No per-wave statistics (a record
// is 64 members = eight of these waves; runs with collect_stats take the one-lane form).
// ---------------------------------------------------------------------------------
template <int CTRL, int BANKS>
__device__ __forceinline__ double dpp_merge(const double old, const double src) {       // lanes of the banks in BANKS: src moved by CTRL; others: old
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xf, BANKS, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xf, BANKS, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int BANKS>
__device__ __forceinline__ float dpp_merge(const float old, const float src) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), CTRL, 0xf, BANKS, false));
}
constexpr int DPP_ROW_SHL4 = 0x104, DPP_ROW_SHR4 = 0x114;          // lane i reads lane i + 4 / lane i - 4 of its row of 16

template <typename T>
__global__ __launch_bounds__(FIVEEQ_SMALL_BLOCK) __attribute__((amdgpu_waves_per_eu(1, 2))) void small_octet_kernel(
    const KModel<T> km, const T* __restrict__ drive, const int n_steps, const int t_begin, const int t_end,
    const int64_t n, const int64_t ld, const T* __restrict__ r, const T* __restrict__ q, T* __restrict__ R,
    T* __restrict__ S, T* __restrict__ C_traj /* [n_rows][3][ld] or nullptr */, T* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows) {
    constexpr int MPB = FIVEEQ_SMALL_BLOCK / 8;                          // members per workgroup
    __shared__ T drv[FIVEEQ_FUSED_CHUNK * DRIVE_STRIDE];
    __shared__ int row_s[FIVEEQ_FUSED_CHUNK];
    const int lane = threadIdx.x;
    const int o = lane & 7;                                              // position in the octet
    const int g = o < 4 ? 0 : (o == 4 ? 1 : 2);                          // this lane's gas
    const int prow = o < 4 ? o : (o == 4 ? 4 : 5);                       // ... and its pool's row of R
    const bool co2 = o < 4;
    const int64_t m = (int64_t)blockIdx.x * MPB + lane / 8;
    const bool active = m < n;
    const int64_t mm = active ? m : 0;                                   // idle tail lanes shadow member 0 and store nothing
    // this lane's gas, selected once from the kernel argument (scalar loads) into vector registers
#define FIVEEQ_PICK(field) (g == 0 ? km.gas[0].field : (g == 1 ? km.gas[1].field : km.gas[2].field))
    const T ndt = co2 ? (o == 0 ? km.gas[0].ndt_over_tau[0] : (o == 1 ? km.gas[0].ndt_over_tau[1] : (o == 2 ? km.gas[0].ndt_over_tau[2] : km.gas[0].ndt_over_tau[3])))
                      : (g == 1 ? km.gas[1].ndt_over_tau[0] : km.gas[2].ndt_over_tau[0]);
    const T natc = -(co2 ? (o == 0 ? km.gas[0].atc[0] : (o == 1 ? km.gas[0].atc[1] : (o == 2 ? km.gas[0].atc[2] : km.gas[0].atc[3])))
                         : (g == 1 ? km.gas[1].atc[0] : km.gas[2].atc[0]));
    const T g0 = FIVEEQ_PICK(g0), inv_g1 = FIVEEQ_PICK(inv_g1), ra = FIVEEQ_PICK(ra), inv_c = FIVEEQ_PICK(inv_c);
    const T C0 = FIVEEQ_PICK(C0), inv_C0 = FIVEEQ_PICK(inv_C0), sqrtC0 = FIVEEQ_PICK(sqrtC0);
    const T f1 = FIVEEQ_PICK(f1), f2 = FIVEEQ_PICK(f2), f3 = FIVEEQ_PICK(f3);
#undef FIVEEQ_PICK
    const bool has_log = f1 != T(0), has_sqrt = f3 != T(0);
    T rr[3], qq[2], Sv[2];
    T Rv = R[prow * ld + mm];
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = S[k * ld + mm];
#pragma unroll
    for (int k = 0; k < 3; ++k) rr[k] = r[(3 * g + k) * ld + mm];
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = q[k * ld + mm];
    // ONE store per step and lane: lanes 0 / 4 / 5 write their gas's C, lane 1 writes T (null = this lane stores nothing)
    T* out_p = nullptr;
    int64_t out_stride = 0;
    if (active) {
        if (o == 1) out_p = T_traj ? T_traj + m : nullptr, out_stride = ld;
        else if (o == 0 || o == 4 || o == 5) out_p = C_traj ? C_traj + g * ld + m : nullptr, out_stride = 3 * ld;
    }
    // the sum over this lane's gas's pools of the CURRENT state, as small_kernel keeps it (a step's own sum is the next step's)
    T sumR;
    {
        T s4 = quad_bcast<0>(Rv);
        s4 += quad_bcast<1>(Rv);
        s4 += quad_bcast<2>(Rv);
        s4 += quad_bcast<3>(Rv);
        sumR = co2 ? s4 : Rv;
    }
    for (int tc = t_begin; tc < t_end; tc += FIVEEQ_FUSED_CHUNK) {
        const int nt = min(FIVEEQ_FUSED_CHUNK, t_end - tc);
        __syncthreads();
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_SMALL_BLOCK) {
            const T v = drive[(int64_t)tc * DRIVE_STRIDE + i];
            drv[i] = v;
            if ((i & (DRIVE_STRIDE - 1)) == 7) row_s[i >> 3] = (int)v;
        }
        __syncthreads();
        T E = drv[g], cumE = drv[3 + g], Fx = drv[6];                    // step tc: this lane's gas's emission and cumulative emission
        int rowv = row_s[0];
        for (int k = 0; k < nt; ++k) {
            const int kn = k + 1 < nt ? k + 1 : k;                       // the NEXT step's record, asked for now
            const T En = drv[kn * DRIVE_STRIDE + g], cumEn = drv[kn * DRIVE_STRIDE + 3 + g], Fxn = drv[kn * DRIVE_STRIDE + 6];
            const int rowvn = row_s[kn];
            // ---- gas_step<.., g, INV = false>, operation for operation, for THIS lane's gas and pool ----
            const T T_old = Sv[0] + Sv[1];
            const T G_a = sumR * inv_c;
            const T G_u = cumE - G_a;
            T iirf = fe_fma(ra, G_a, fe_fma(rr[2], T_old, fe_fma(rr[1], G_u, rr[0])));
            iirf = fe_min(iirf, km.iirf_max);
            const T alpha = g0 * fe_exp(iirf * inv_g1);
            const T inv_alpha = fe_rcp(alpha);
            const T Ea = E * alpha;
            const T em1 = fe_expm1_neg(ndt * inv_alpha);
            const T Rn = fe_fma(em1, fe_fma(natc, Ea, Rv), Rv);
            Rv = Rn;
            T s4 = T(0);
            s4 += quad_bcast<0>(Rn);
            s4 += quad_bcast<1>(Rn);
            s4 += quad_bcast<2>(Rn);
            s4 += quad_bcast<3>(Rn);
            const T s1 = T(0) + Rn;
            const T sumN = co2 ? s4 : s1;
            sumR = sumN;
            const T Cg = C0 + sumN;
            const bool pos = Cg > T(0);
            T Fg = f2 * (Cg - C0);
            {
                const T lg = fe_log(pos ? Cg * inv_C0 : T(1));
                const T with_log = fe_fma(f1, lg, Fg);
                Fg = (has_log && pos) ? with_log : Fg;
                const T sq = fe_sqrt(pos ? Cg : T(1));
                const T with_sqrt = fe_fma(f3, (pos ? sq : T(0)) - sqrtC0, Fg);
                Fg = has_sqrt ? with_sqrt : Fg;
            }
            // ---- the three gases' forcings to every lane of the octet ----
            const T a0 = quad_bcast<0>(Fg);                              // quad 0: F_0 (lane 0's); quad 1: F_1 (lane 4's)
            const T a1 = quad_bcast<1>(Fg);                              // quad 0: F_0 (lane 1's); quad 1: F_2 (lane 5's)
            const T F0 = dpp_merge<DPP_ROW_SHR4, 0xA>(a0, a0);           // quads 1, 3 of the row take their left neighbour's
            const T F1 = dpp_merge<DPP_ROW_SHL4, 0x5>(a0, a0);           // quads 0, 2 take their right neighbour's
            const T F2 = dpp_merge<DPP_ROW_SHL4, 0x5>(a1, a1);
            T F = Fx;
            F += F0;
            F += F1;
            F += F2;
#pragma unroll
            for (int j = 0; j < 2; ++j) Sv[j] = fe_fma(km.em1_d[j], fe_fma(-qq[j], F, Sv[j]), Sv[j]);
            const T Tn = Sv[0] + Sv[1];
            const int row = __builtin_amdgcn_readfirstlane(rowv);
            if (row >= 0 && row < n_rows) {
                if (out_p != nullptr) out_p[(int64_t)row * out_stride] = o == 1 ? Tn : Cg;
            }
            E = En, cumE = cumEn, Fx = Fxn, rowv = rowvn;
        }
    }
    if (active) {
        if (o < 6) R[prow * ld + m] = Rv;
        if (o < 2) S[o * ld + m] = o == 0 ? Sv[0] : Sv[1];
    }
}

}  // namespace fiveeq
