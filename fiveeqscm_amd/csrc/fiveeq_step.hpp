// fiveeq_step.hpp — kernels 1 and 1s: one timestep per launch (step_kernel, step_scen_kernel).
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 1 — ONE TIMESTEP PER LAUNCH (the north-star form).
// Per member-step HBM traffic (elements): read SP + 2 (state) + 3G + 2 (params),
// write SP + 2 (state) + G + 1 (C, T rows)  ->  A = w (2 SP + 4 G + 7) bytes
// (152 B CO2-only fp64, 248 B for pools 4+1+1 fp64).
// The step's drive record — emissions, cumulative emissions, F_ext and the OUTPUT ROW this step
// is stored at (drive[t][7]; negative = not stored) — is staged through LDS once per workgroup,
// next to the shared model.  One member per lane; a workgroup is ONE wave of 64 members (finer
// dispatch granularity and a trivial barrier: -2 % at 1M members, -3 % at 8M, -7 % at 100k against
// 256-thread workgroups with identical buffers, profiles/r01/ab_variants.txt) and owns the same
// members in every launch.
// CACHE POLICY OF THE ROWS (round 5, profiles/r05/step_row_policy_ab.txt, hbm_rates.txt):
//   * the stored C / T rows are written with the NON-TEMPORAL policy in every form: written once, never read by a stepping
//     kernel, they only displace state and parameter rows from the 256 MiB Infinity Cache that the next step would have hit
//     (-1.4 % per step at 1M fp64 members, -1 % at the 1.25M shard, -3...-8 % on chunk-major runs of 8-25M members);
//   * NT = true (the STREAMED form): state and parameter rows too.  For a launch whose rows cannot survive until the next
//     step anyway — far more members than the cache holds, not scheduled chunk-major — the default policy only adds
//     allocate-and-evict work to every access: -4.5 % per step at 8M fp64 members (0.676 -> 0.707 of 8 TB/s), -9 % at 4M;
//     on a cache-resident ensemble it is the WRONG form (+11...13 % at 1-2M members).  The host picks per call
//     (fiveeq_capi.hip, rows_streamed()).  Same arithmetic: the same bits.
// ---------------------------------------------------------------------------------
// BINS = true: the streamed-histogram form.  Besides everything above, the kernel writes the histogram BIN INDEX of T of every
// step (fiveeq_hist_rows' bin rule, bit for bit; 0xFFFF for a NaN) as one uint16 per member into a ring
// bin_ring[ring_rows][ld] at row t mod ring_rows — 2 bytes per member-step where a ring of T rows takes w — for the
// histogram pass (hist_bins_kernel) to count.  The pass no longer sees T, so the moments stay in the kernel (stats).

#ifdef FIVEEQ_STEP_WAVES
#define FIVEEQ_STEP_ATTR __attribute__((amdgpu_waves_per_eu(FIVEEQ_STEP_WAVES, FIVEEQ_STEP_WAVES)))
#else
#define FIVEEQ_STEP_ATTR
#endif
// MISFIT = true (round 7): the step also carries the member's misfit accumulators misfit [3][ld] fp64 (misfit_update()).  The
// step's obs record is wave-uniform and read with scalar loads; on a step outside the window (p_t == 0 && b_t == 0) the
// rows are neither read nor written, so such a step moves the bytes of the plain kernel.  Inside it: 24 B read + 24 B
// written per member-step.  Instantiated for the {4} and 4 + 1 + 1 layouts, default row policy only.
// FORC = true (round 8): the step with per-member forcing scales (member_step<.., FORC>).  The lane also loads its G + n_fext
// scale rows fscale [G + n_fext][ld] (gas rows first) — issued with the other row loads, before the staging barrier — and
// the step's record fext [t][0 .. MAX_FEXT) is wave-uniform and read with scalar loads, like the obs record.  w (G + K) bytes
// more per member-step; combines with MISFIT, not with BINS; default row policy; the {4} and 4 + 1 + 1 layouts.
// UNI = true: the single-valued parameter rows (step_uniform_kernel below).  Row k of r (k < 3G) with bit k of uni.mask set,
// row j of q with bit 3G + j set, is NOT loaded: the lane takes uni.val[k] — wave-uniform, from the kernel arguments (scalar
// registers), splat into both members of a packed lane — behind one scalar branch per row.  The loads that remain are still
// all issued before the staging barrier; everything after them is the same member_step() and the same stores: the same bits.
template <typename T>
struct UniformRows {
    uint32_t mask;
    T val[3 * MAX_GAS + 2];
};
// The body of step_kernel and step_uniform_kernel (force-inlined: step_kernel's code is what it was when it spelt this out,
// profiles/r16/uniform_rows_isa.txt).
// MFORC = true (with FORC; step_mforc_kernel below): the lane also loads its element of THIS step's member_forcing row
// mforc [n_steps][ld] — one more coalesced row load, issued with the lane's other rows (where F opens: beside the category
// scales), w bytes more per member-step; a packed fp32 lane loads its two members as one 8-byte access.
template <typename V, int P0, int P1, int P2, bool BINS, bool NT, bool MISFIT, bool FORC, bool UNI, bool MFORC = false>
__device__ __forceinline__ void step_body(
    const typename Lane<V>::S* __restrict__ drive, const int n_steps, const int t,
    const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj, typename Lane<V>::S* __restrict__ T_traj,
    const int n_rows, double* __restrict__ stats,
    unsigned short* __restrict__ bin_ring, const int ring_rows,
    const double hist_lo, const double hist_inv_w, const int n_bins,
    const double* __restrict__ obs, double* __restrict__ misfit,
    const typename Lane<V>::S* __restrict__ fscale,
    const typename Lane<V>::S* __restrict__ fext, const int n_fext,
    const UniformRows<typename Lane<V>::S>& uni, const typename Lane<V>::S* __restrict__ mforc = nullptr) {
    using L = Layout<P0, P1, P2>;
    using T = typename Lane<V>::S;
    constexpr int W = Lane<V>::W;                 // members per lane
    constexpr bool NTT = true;                    // the stored C / T rows: written once, never read by a stepping kernel
    // SPREAD (round 18): the fp64 kernels load their rows in order of use and store each row as soon as its value is final
    // (below).  The fp32 kernels keep the block schedule — all loads, all arithmetic, all stores: with the spread one they
    // measured 7.1 % SLOWER per step at 1M members (profiles/r18/step_schedule_ab.txt, section B).
    constexpr bool SPREAD = sizeof(T) == 8;
    static_assert(!FORC || (!BINS && !NT), "the forcing scales: no histogram ring, default row policy");
    static_assert(!UNI || (!BINS && !MISFIT && !FORC), "the single-valued rows: the plain forward form only");
    static_assert(!MFORC || FORC, "the per-member forcing row: a form of the forcing-scale family");
    __shared__ T drv[DRIVE_STRIDE];
    // idle tail lanes load a valid (aligned) member and store nothing
    const LaneSpan span = lane_span<W, FIVEEQ_STEP_BLOCK, PARK_LAST>(n);
    const int64_t m = span.m, mm = span.mm;       // (plain locals: the row lambdas below capture them)
    const bool active = span.active, full = span.full;
    // Issue order matters for the workgroup's critical path: first the (tiny) shared loads, then
    // all row loads, and only then the LDS writes + barrier, so the staging round trip is
    // overlapped with the row round trip instead of preceding it (+1.3 % at 1M members, neutral
    // elsewhere: profiles/r01/ab_variants.txt).
    __shared__ KModel<T> km_s;
    constexpr int NW = sizeof(KModel<T>) / sizeof(T);
    static_assert(NW <= FIVEEQ_STEP_BLOCK, "model must stage in one pass");
    const T* kargs = (const T*)__builtin_amdgcn_kernarg_segment_ptr();
    T stage_v = T(0), drv_v = T(0);
    if (threadIdx.x < NW) stage_v = kargs[threadIdx.x];
    if (threadIdx.x < DRIVE_STRIDE) drv_v = drive[(int64_t)t * DRIVE_STRIDE + threadIdx.x];
    const KModel<T>& kmr = km_s;

    V rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Cv[L::G];
    V fs[FORC ? L::G + MAX_FEXT : 1];             // FORC: the lane's scales, gas rows first (rows past n_fext are never read)
    V mf = V();                                   // MFORC: the lane's element of this step's member_forcing row
    // one parameter row: the load, or (UNI, bit set) the single value from the kernel arguments
    const auto par_row = [&](const T* __restrict__ rows, const int k, const int bit) -> V {
        if constexpr (UNI) {
            if (uni.mask & (1u << bit)) return (V)uni.val[bit];
        }
        return load_row<V, NT>(rows + k * ld + mm);
    };
    if constexpr (SPREAD) {
        // In order of use: S (T_old), [FORC: the category scales, which open F], per gas its pools, its r0 / rC / rT and [FORC] its
        // scale, q last — so that gas 0 can start when ITS rows have landed, behind a partial vmcnt wait, with the later rows in flight.
#pragma unroll
        for (int k = 0; k < 2; ++k) Sv[k] = load_row<V, NT>(S + k * ld + mm);
        if constexpr (MFORC) mf = load_row<V, NT>(mforc + (int64_t)t * ld + mm);
        if constexpr (FORC) {
#pragma unroll
            for (int k = L::G; k < L::G + MAX_FEXT; ++k) fs[k] = k < L::G + n_fext ? load_row<V, NT>(fscale + k * ld + mm) : (V)T(0);
        }
#pragma unroll
        for (int g = 0; g < L::G; ++g) {
#pragma unroll
            for (int i = 0; i < L::pools(g); ++i) Rv[L::off(g) + i] = load_row<V, NT>(R + (L::off(g) + i) * ld + mm);
#pragma unroll
            for (int k = 3 * g; k < 3 * g + 3; ++k) rr[k] = par_row(r, k, k);
            if constexpr (FORC) fs[g] = load_row<V, NT>(fscale + g * ld + mm);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) qq[k] = par_row(q, k, 3 * L::G + k);
    } else {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) Rv[k] = load_row<V, NT>(R + k * ld + mm);
#pragma unroll
        for (int k = 0; k < 2; ++k) Sv[k] = load_row<V, NT>(S + k * ld + mm);
#pragma unroll
        for (int k = 0; k < 3 * L::G; ++k) rr[k] = par_row(r, k, k);
#pragma unroll
        for (int k = 0; k < 2; ++k) qq[k] = par_row(q, k, 3 * L::G + k);
        if constexpr (FORC) {
#pragma unroll
            for (int k = 0; k < L::G + MAX_FEXT; ++k) fs[k] = k < L::G + n_fext ? load_row<V, NT>(fscale + k * ld + mm) : (V)T(0);
        }
        if constexpr (MFORC) mf = load_row<V, NT>(mforc + (int64_t)t * ld + mm);
    }

    if (threadIdx.x < NW) reinterpret_cast<T*>(&km_s)[threadIdx.x] = stage_v;
    if (threadIdx.x < DRIVE_STRIDE) drv[threadIdx.x] = drv_v;
    __syncthreads();

    const int row = __builtin_amdgcn_readfirstlane((int)drv[7]);         // wave-uniform: scalar test + offsets
    const bool stored = row >= 0 && row < n_rows;
    // A row is stored AS SOON AS ITS VALUE IS FINAL: gas g's pools and, on a stored step, its C row right after gas g
    // (member_step's after-gas hook), before the next gas's arithmetic — the wave's writes are spread over its lifetime and
    // the registers die early (fp64 4 + 1 + 1: 72 -> 68 VGPRs).  With the loads in order of use: ratio 0.9869 (-1.3 %) per step
    // at 1M fp64 members, ranges disjoint; either half alone (0.994, 1.002) does not separate from the run-to-run spread
    // (profiles/r18/step_schedule_ab.txt, sections A and C).
    const auto store_gas = [&](auto gas) {
        constexpr int g = decltype(gas)::value;
        if (active) {
#pragma unroll
            for (int i = 0; i < L::pools(g); ++i) store_row<NT>(R + (L::off(g) + i) * ld + m, Rv[L::off(g) + i], full);
            if (stored && C_traj != nullptr) store_row<NTT>(C_traj + ((int64_t)row * L::G + g) * ld + m, Cv[g], full);
        }
    };
    V Tn = (V)T(0);
    V no_cum[L::G], no_Rlo[L::SP];                // never touched: INV = COMP = false
    if constexpr (MFORC && SPREAD)
        member_step<V, L, false, false, true, decltype(store_gas), 0, true>(kmr, drv, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, 1,
                                                                            fext + (int64_t)t * MAX_FEXT, n_fext, store_gas, mf);
    else if constexpr (MFORC)
        member_step<V, L, false, false, true, NoGasHook, 0, true>(kmr, drv, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, 1,
                                                                  fext + (int64_t)t * MAX_FEXT, n_fext, NoGasHook{}, mf);
    else if constexpr (SPREAD)
        member_step<V, L, false, false, FORC>(kmr, drv, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, 1,
                                              FORC ? fext + (int64_t)t * MAX_FEXT : nullptr, n_fext, store_gas);
    else
        member_step<V, L, false, false, FORC>(kmr, drv, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, 1,
                                              FORC ? fext + (int64_t)t * MAX_FEXT : nullptr, n_fext);
    if (active) {
        if constexpr (!SPREAD) {
#pragma unroll
            for (int k = 0; k < L::SP; ++k) store_row<NT>(R + k * ld + m, Rv[k], full);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) store_row<NT>(S + k * ld + m, Sv[k], full);
        if (stored) {
            if (!SPREAD && C_traj != nullptr) {
                T* c = C_traj + (int64_t)row * L::G * ld + m;
#pragma unroll
                for (int g = 0; g < L::G; ++g) store_row<NTT>(c + g * ld, Cv[g], full);
            }
            if (T_traj != nullptr) store_row<NTT>(T_traj + (int64_t)row * ld + m, Tn, full);
        }
        if constexpr (MISFIT) misfit_step(obs + (int64_t)t * 4, Tn, misfit + m, 1, ld, full);
        if constexpr (BINS)
            store_bin(bin_ring + (int64_t)(t % ring_rows) * ld + m, make_rule(T(0), hist_lo, hist_inv_w, n_bins), Tn, full);
    }
    if (stats != nullptr) {
        const int64_t n_rec = (n + 63) >> 6;                             // one record per 64 members
        const int64_t wave = (int64_t)blockIdx.x * (FIVEEQ_STEP_BLOCK / 64) + (threadIdx.x >> 6);
        if constexpr (W == 1) {
            if (wave < n_rec) wave_stats(active, Tn, stats + (wave * n_steps + t) * 4);
        } else {
            if (2 * wave < n_rec)
                wave_stats(active, full, Tn, stats + (2 * wave * n_steps + t) * 4,
                           2 * wave + 1 < n_rec ? stats + ((2 * wave + 1) * n_steps + t) * 4 : nullptr);
        }
    }
}

template <typename V, int P0, int P1, int P2, bool BINS = false, bool NT = false, bool MISFIT = false, bool FORC = false>
__global__ __launch_bounds__(FIVEEQ_STEP_BLOCK) FIVEEQ_STEP_ATTR void step_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps, const int t,
    const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */,
    typename Lane<V>::S* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */,
    unsigned short* __restrict__ bin_ring /* BINS: [ring_rows][ld], row t mod ring_rows */, const int ring_rows,
    const double hist_lo, const double hist_inv_w, const int n_bins,
    const double* __restrict__ obs /* MISFIT: [n_steps][4] */, double* __restrict__ misfit /* MISFIT: [3][ld] */,
    const typename Lane<V>::S* __restrict__ fscale /* FORC: [G + n_fext][ld] */,
    const typename Lane<V>::S* __restrict__ fext /* FORC: [n_steps][MAX_FEXT] */, const int n_fext) {
    step_body<V, P0, P1, P2, BINS, NT, MISFIT, FORC, false>(drive, n_steps, t, n, ld, r, q, R, S, C_traj, T_traj, n_rows, stats,
                                                            bin_ring, ring_rows, hist_lo, hist_inv_w, n_bins, obs, misfit, fscale,
                                                            fext, n_fext, UniformRows<typename Lane<V>::S>{});
}

// Kernel 1m — step_kernel<V, P0, P1, P2, false, false, MISFIT, true> WITH a per-member forcing row per step (MFORC above;
// fiveeq_run_mforc_*, include/fiveeq.h "MEMBER FORCING").  A kernel of its own name: every instantiation of step_kernel keeps
// its symbol and its machine code.  The {4} and 4 + 1 + 1 layouts, with and without the misfit, default row policy.
template <typename V, int P0, int P1, int P2, bool MISFIT = false>
__global__ __launch_bounds__(FIVEEQ_STEP_BLOCK) FIVEEQ_STEP_ATTR void step_mforc_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps, const int t,
    const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */,
    typename Lane<V>::S* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */,
    const double* __restrict__ obs /* MISFIT: [n_steps][4] */, double* __restrict__ misfit /* MISFIT: [3][ld] */,
    const typename Lane<V>::S* __restrict__ fscale /* [G + n_fext][ld] */,
    const typename Lane<V>::S* __restrict__ fext /* [n_steps][MAX_FEXT] */, const int n_fext,
    const typename Lane<V>::S* __restrict__ mforc /* [n_steps][ld] */) {
    step_body<V, P0, P1, P2, false, false, MISFIT, true, false, true>(drive, n_steps, t, n, ld, r, q, R, S, C_traj, T_traj, n_rows,
                                                                      stats, nullptr, 0, 0.0, 0.0, 0, obs, misfit, fscale, fext,
                                                                      n_fext, UniformRows<typename Lane<V>::S>{}, mforc);
}

// Kernel 1u — step_kernel<V, P0, P1, P2, false, NT> WITHOUT the loads of the parameter rows the caller declared single-valued
// (UNI above; fiveeq_run_uniform_*, include/fiveeq.h "SINGLE-VALUED PARAMETER ROWS").  w bytes less per member-step and masked
// row.  The {4} and 4 + 1 + 1 layouts, both row policies, the plain forward form.
template <typename V, int P0, int P1, int P2, bool NT = false>
__global__ __launch_bounds__(FIVEEQ_STEP_BLOCK) FIVEEQ_STEP_ATTR void step_uniform_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps, const int t,
    const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */,
    typename Lane<V>::S* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */,
    const UniformRows<typename Lane<V>::S> uni) {
    step_body<V, P0, P1, P2, false, NT, false, false, true>(drive, n_steps, t, n, ld, r, q, R, S, C_traj, T_traj, n_rows, stats,
                                                            nullptr, 0, 0.0, 0.0, 0, nullptr, nullptr, nullptr, nullptr, 0, uni);
}

// The scan behind fiveeq_uniform_rows_*: row k of rows_r [n_r][ld] (k < n_r), row j of rows_q [2][ld] as row n_r + j.  A row
// is single-valued iff every one of its n members has the BITS of its first (+0.0 and -0.0 differ; one NaN pattern is one
// value); ld padding is not read.  blockIdx.y is the row, the workgroups of a row stride over its members; a wave that saw
// another bit pattern ORs the row's bit into *differs (zeroed by the host), and the row's first workgroup stores the first
// member's bits into first[row].
template <typename U>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void uniform_rows_kernel(const int64_t n, const int64_t ld, const int n_r,
                                                                    const U* __restrict__ rows_r, const U* __restrict__ rows_q,
                                                                    unsigned int* __restrict__ differs, U* __restrict__ first) {
    const int row = blockIdx.y;
    const U* p = row < n_r ? rows_r + (int64_t)row * ld : rows_q + (int64_t)(row - n_r) * ld;
    const U v0 = p[0];
    U diff = 0;
    for (int64_t i = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * FIVEEQ_BLOCK)
        diff |= p[i] ^ v0;
    if (__ballot(diff != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(differs, 1u << row);
    if (blockIdx.x == 0 && threadIdx.x == 0) first[row] = v0;
}

// ---------------------------------------------------------------------------------
// Kernel 1s — SCENARIOS (ABI v13): one step of every parameter member under each of n_scen emission scenarios.  Same
// block shape, lane packing and row policy (NT) as step_kernel; the lane loads its member's 3G + 2 parameter rows ONCE
// and then, scenario by scenario, loads that scenario's R and S, calls the same member_step() with that scenario's drive
// record, and stores R, S, the stored rows and the wave's statistics record: member-scenario (m, s) is bit for bit member
// m of step_kernel run on scenario s's drive table.  Per member-scenario-step: w (2 SP + 4 + (G + 1) stored) + w (3G + 2) / S.
// The drive records are wave-uniform (a workgroup is one wave) and are read with scalar loads straight from
// drive [n_scen][n_steps][8] — no LDS staging and no barrier per scenario.  Every scenario stride derives from ld:
//   R [n_scen][SP][ld], S [n_scen][2][ld], C_traj [n_scen][n_rows][G][ld], T_traj [n_scen][n_rows][ld],
//   stats [n_scen][ceil(ld/64)][n_steps][4]
// so a member sub-range [m0, m0 + n) is a plain pointer offset, as for step_kernel.
//
// FORC = true (round 9): the scenarios with per-member forcing scales (member_step<.., FORC>).  The lane loads its G + n_fext
// scale rows fscale [G + n_fext][ld] ONCE, beside the parameter rows, for all scenarios — w (G + K) / S bytes per
// member-scenario-step — and scenario sc's table record fext [sc][t][0 .. MAX_FEXT) is wave-uniform and read with scalar
// loads, like its drive record (n_fext == 0: no record is read).  Member-scenario (m, s) is bit for bit member m of
// step_kernel<.., FORC> on scenario s's drive table and category table.  Default row policy; the {4} and 4 + 1 + 1 layouts.
// Where the scales live across the scenario loop is ScenForc::FS_LDS.
// ---------------------------------------------------------------------------------
// The plain fp64 4 + 1 + 1 scenario kernel sits at 120 VGPRs, 4 waves per SIMD: seven fp64 scales live across the scenario
// loop would take it past 128 and cost a wave.  Such an instantiation parks the scales in a lane-private LDS slot
// fs_s[G + MAX_FEXT][FIVEEQ_STEP_BLOCK] like fused_kernel's FS_LDS form (consecutive lanes, consecutive words: no bank
// conflicts; a lane reads only what it wrote, and a wave's LDS operations complete in program order: no barrier beyond the
// model's staging barrier), read back with one ds_read per fma.  Everything else keeps them in registers.
// profiles/r09/scenario_forcing_isa.txt has the counts both ways.
template <typename V, typename L>
struct ScenForc {
    static constexpr bool FS_LDS = false;
};
template <>
struct ScenForc<double, Layout<4, 1, 1>> {
    static constexpr bool FS_LDS = true;
};
template <typename V, int P0, int P1, int P2, bool NT = false, bool FORC = false>
__global__ __launch_bounds__(FIVEEQ_STEP_BLOCK) FIVEEQ_STEP_ATTR void step_scen_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps, const int t,
    const int64_t n, const int64_t ld, const int n_scen,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj, typename Lane<V>::S* __restrict__ T_traj,
    const int n_rows, double* __restrict__ stats,
    const typename Lane<V>::S* __restrict__ fscale /* FORC: [G + n_fext][ld] */,
    const typename Lane<V>::S* __restrict__ fext /* FORC: [n_scen][n_steps][MAX_FEXT] */, const int n_fext) {
    using L = Layout<P0, P1, P2>;
    using T = typename Lane<V>::S;
    constexpr int W = Lane<V>::W;                 // members per lane
    constexpr bool NTT = true;                    // the stored C / T rows: written once, never read by a stepping kernel
    static_assert(!FORC || !NT, "the forcing scales: default row policy");
    constexpr bool FS_LDS = FORC && ScenForc<V, L>::FS_LDS;           // FORC: the scales in a lane-private LDS slot
    const auto [m, active, full, mm] = lane_span<W, FIVEEQ_STEP_BLOCK, PARK_LAST>(n);
    __shared__ KModel<T> km_s;
    constexpr int NW = sizeof(KModel<T>) / sizeof(T);
    static_assert(NW <= FIVEEQ_STEP_BLOCK, "model must stage in one pass");
    const T* kargs = (const T*)__builtin_amdgcn_kernarg_segment_ptr();
    T stage_v = T(0);
    if (threadIdx.x < NW) stage_v = kargs[threadIdx.x];
    const KModel<T>& kmr = km_s;

    V rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Cv[L::G];
#pragma unroll
    for (int k = 0; k < 3 * L::G; ++k) rr[k] = load_row<V, NT>(r + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = load_row<V, NT>(q + k * ld + mm);
    // FORC: the lane's scales, gas rows first (rows past n_fext are never read): scale j at fs[j * FS_STRIDE]
    __shared__ V fs_s[FS_LDS ? (L::G + MAX_FEXT) * FIVEEQ_STEP_BLOCK : 1];
    V fs_r[FORC && !FS_LDS ? L::G + MAX_FEXT : 1];
    V* const fs = FS_LDS ? &fs_s[threadIdx.x] : fs_r;
    constexpr int FS_STRIDE = FS_LDS ? FIVEEQ_STEP_BLOCK : 1;
    if constexpr (FORC) {
#pragma unroll
        for (int k = 0; k < L::G + MAX_FEXT; ++k)
            fs[k * FS_STRIDE] = k < L::G + n_fext ? load_row<V, NT>(fscale + k * ld + mm) : (V)T(0);
    }
    if (threadIdx.x < NW) reinterpret_cast<T*>(&km_s)[threadIdx.x] = stage_v;
    __syncthreads();

    const int64_t n_rec = (n + 63) >> 6;
    const int64_t wave = (int64_t)blockIdx.x * (FIVEEQ_STEP_BLOCK / 64) + (threadIdx.x >> 6);
    const int64_t rec_stride = ((ld + 63) >> 6) * n_steps * 4;       // one scenario's statistics records
    // one 64-bit lane base per array, advanced by a scenario stride; the row offsets inside a scenario are wave-uniform (an
    // active lane stores where it loaded: m == mm) — per-row lane addresses kept live across the loop cost 50 VGPRs
    T* Rl = R + mm;
    T* Sl = S + mm;
#pragma unroll 1
    for (int sc = 0; sc < n_scen; ++sc, Rl += (int64_t)L::SP * ld, Sl += 2 * ld) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) Rv[k] = load_row<V, NT>(Rl + k * ld);
#pragma unroll
        for (int k = 0; k < 2; ++k) Sv[k] = load_row<V, NT>(Sl + k * ld);
        const T* d = drive + ((int64_t)sc * n_steps + t) * DRIVE_STRIDE;    // wave-uniform: scalar loads
        V Tn = (V)T(0);
        if constexpr (FORC) {
            V no_cum[L::G], no_Rlo[L::SP];        // never touched: INV = COMP = false
            member_step<V, L, false, false, true>(kmr, d, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, FS_STRIDE,
                                                  fext + ((int64_t)sc * n_steps + t) * MAX_FEXT, n_fext);
        } else {
            member_step<V, L>(kmr, d, rr, qq, Rv, Sv, Cv, Tn);
        }
        if (active) {
#pragma unroll
            for (int k = 0; k < L::SP; ++k) store_row<NT>(Rl + k * ld, Rv[k], full);
#pragma unroll
            for (int k = 0; k < 2; ++k) store_row<NT>(Sl + k * ld, Sv[k], full);
            const int row = __builtin_amdgcn_readfirstlane((int)d[7]);
            if (row >= 0 && row < n_rows) {
                if (C_traj != nullptr) {
                    T* c = C_traj + ((int64_t)sc * n_rows + row) * L::G * ld + m;
#pragma unroll
                    for (int g = 0; g < L::G; ++g) store_row<NTT>(c + g * ld, Cv[g], full);
                }
                if (T_traj != nullptr) store_row<NTT>(T_traj + ((int64_t)sc * n_rows + row) * ld + m, Tn, full);
            }
        }
        if (stats != nullptr) {
            double* const st = stats + sc * rec_stride;
            if constexpr (W == 1) {
                if (wave < n_rec) wave_stats(active, Tn, st + (wave * n_steps + t) * 4);
            } else {
                if (2 * wave < n_rec)
                    wave_stats(active, full, Tn, st + (2 * wave * n_steps + t) * 4,
                               2 * wave + 1 < n_rec ? st + ((2 * wave + 1) * n_steps + t) * 4 : nullptr);
            }
        }
    }
}

}  // namespace fiveeq
