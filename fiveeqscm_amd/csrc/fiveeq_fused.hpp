// fiveeq_fused.hpp — kernel 2: the time-fused step (fused_kernel).
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// Where the fused kernel keeps a lane's G + MAX_FEXT forcing scales (FORC), and how many steps it stages per refill.
// Registers by default.  The fp64 4 + 1 + 1 form is the exception: its plain kernel sits at 117 VGPRs, 4 waves per SIMD, and
// seven fp64 scales in registers took it to 129 (135 with the misfit): 3 waves.  There the scales live in a lane-private LDS
// slot fs_s[G + MAX_FEXT][FIVEEQ_BLOCK], like the misfit accumulators (consecutive lanes, consecutive words: no bank
// conflicts, no barrier), read back with one ds_read per fma; and so that four workgroups still fit a CU's 160 KB beside the
// misfit slot (14 + 6 KB of slots on 17 KB of statistics tile and model), it stages 25 steps per refill instead of 125
// (2.4 KB of drive and table records instead of 12): 39984 B per workgroup with the misfit, under the 40960 a static_assert in
// the kernel holds it to.  profiles/r08/forcing_isa.txt has the counts.
// With SCEN (round 9) the fp32 {4} form takes the slot too: its plain scenario kernel sits at 65 VGPRs, 7 waves per SIMD, and five
// fp32 scales in registers took it to 74: 6 waves; with the slot it is at 66 and keeps 7 (seven workgroups of 14.5 KB fit a CU).
// The fp64 {4} and the packed fp32 {4} scenario forms lose a wave either way (slot: 103 and 85 VGPRs where 96 and 80 would be
// needed, and six packed workgroups of 27.6 KB would not fit a CU), exactly as their single-scenario forms do: they keep
// the registers.  profiles/r09/scenario_forcing_isa.txt.  WGS: the workgroups per CU the slot has to leave room for.
template <typename V, typename L, bool MISFIT, bool FORC, bool SCEN = false>
struct FusedForc {
    static constexpr bool FS_LDS = false;
    static constexpr int CHUNK = FIVEEQ_FUSED_CHUNK;
    static constexpr int WGS = 4;
};
template <bool MISFIT, bool SCEN>
struct FusedForc<double, Layout<4, 1, 1>, MISFIT, true, SCEN> {
    static constexpr bool FS_LDS = true;
    static constexpr int CHUNK = FIVEEQ_FUSED_CHUNK < 25 ? FIVEEQ_FUSED_CHUNK : 25;
    static constexpr int WGS = 4;
};
template <>
struct FusedForc<float, Layout<4, 0, 0>, false, true, true> {
    static constexpr bool FS_LDS = true;
    static constexpr int CHUNK = FIVEEQ_FUSED_CHUNK < 25 ? FIVEEQ_FUSED_CHUNK : 25;
    static constexpr int WGS = 7;
};
constexpr int LDS_PER_CU = 160 * 1024;            // MI355X

// ---------------------------------------------------------------------------------
// Kernel 2 — TIME-FUSED: one launch advances [t_begin, t_end); a member's state and
// parameters stay in registers for the whole span, the drive table is staged into LDS
// FIVEEQ_FUSED_CHUNK steps at a time, and only the C/T rows of stored steps go to HBM.
// Per member-step traffic: w (G + 1) + w (2 SP + 3 G + 6) / n_steps.
// Same member_step() as kernel 1: results are bit-identical.
// ---------------------------------------------------------------------------------
//
// INV = true: concentration-driven form.  drive[t][0..2] are target concentrations, cumE [G][ld] is
// per-member cumulative-emission state (in/out), and C_traj receives the DIAGNOSED EMISSIONS.
// (112 VGPRs at fp64 4+1+1 = 4 waves/SIMD; launch-bounds hints for 5 or 6 waves spill: -3 % / -16 %.)
//
// MISFIT = true (round 7; BINS and COMP false; with INV see below): the member's misfit accumulators (misfit_update()) are loaded from
// misfit [3][ld] fp64 once at launch start, carried on chip and stored once at the end — 48 B per member and launch.
// THE CARRIER IS LDS, NOT REGISTERS: three fp64 per member are 6 VGPRs (12 on a packed lane), and in registers they cost the
// fp64 {4} form a wave per SIMD (93 -> 105 VGPRs: 5 -> 4 waves) and the fp32 {4} form one too (66 -> 74: 7 -> 6).  Each lane
// keeps its own words in a lane-private LDS slot (acc_s[3 W][FIVEEQ_BLOCK]: consecutive lanes, consecutive 8-byte words,
// no bank conflicts, no barrier — a wave's LDS operations complete in program order); a window step adds 3 ds_read_b64 +
// 3 ds_write_b64 per member beside the step's VALU.  The step's obs record is wave-uniform and read with SCALAR loads
// straight from obs [n_steps][4] (no LDS staging: the 3 KB a chunk of records would take is what keeps the fp64 {4} form at
// five workgroups per CU, 5 x 31 KB of 160 KB), so the window test is a scalar branch.  Every MISFIT instantiation keeps
// its plain counterpart's waves per SIMD with no scratch (tools/kernel_isa_stats.py); the packed fp32 form is instantiated
// for 4 + 1 + 1 only (fiveeq_capi.hip, misfit_packed_fused).
//
// SCEN = true (ABI v13; INV, BINS, COMP and MISFIT false): the grid's y dimension is the emission scenario.  A workgroup is
// scenario-uniform: it stages its own scenario's drive chunk and offsets the state, row and statistics pointers by the
// scenario strides of kernel 1s (all derived from ld, n_steps and n_rows, so no argument is added).  With SCEN false not
// one instruction of the kernel changes.
//
// FORC = true (round 8; BINS and COMP false, with or without MISFIT; with INV see below): per-member forcing scales
// (member_step<.., FORC>).  The G + n_fext scales are loaded once at launch start and stay on chip for the span; the table chunk
// fext [tc .. tc + nt)[MAX_FEXT] is staged into LDS beside the drive chunk.  Where the scales live is FS_LDS, below.
// With SCEN (round 9; MISFIT false) the table is fext [n_scen][n_steps][MAX_FEXT], one per scenario: the workgroup offsets it
// by its scenario like the drive table; the scale rows are shared by the scenarios.
//
// INV WITH FORC AND / OR MISFIT (scalar lanes, layouts {4} and 4 + 1 + 1): the concentration-driven form with the forcing scales
// and the in-loop misfit, fiveeq_run_inverse_forc_*.  The scales, the table chunk and the accumulators sit where the forward
// forms put them (FusedForc: the fp64 4 + 1 + 1 form keeps its scales in the LDS slot and stages 25 steps per refill); nothing
// of the plain INV kernels changes.  The fp64 4 + 1 + 1 forms run at 3 waves per SIMD (129 to 133 VGPRs; plain INV: 127, 4
// waves); no form uses scratch: profiles/r24/NOTES.md.
template <typename V, int P0, int P1, int P2, bool INV, bool BINS = false, bool COMP = false, bool MISFIT = false,
          bool SCEN = false, bool FORC = false>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void fused_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps,
    const int t_begin, const int t_end, const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ cumE /* [G][ld], INV only */,
    typename Lane<V>::S* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */,
    typename Lane<V>::S* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */,
    unsigned short* __restrict__ bin_ring /* BINS: [ring_rows][ld] */, const int ring_rows, const double hist_lo,
    const double hist_inv_w, const int n_bins,
    const double* __restrict__ obs /* MISFIT: [n_steps][4] */, double* __restrict__ misfit /* MISFIT: [3][ld] */,
    const typename Lane<V>::S* __restrict__ fscale /* FORC: [G + n_fext][ld] */,
    const typename Lane<V>::S* __restrict__ fext /* FORC: [n_steps][MAX_FEXT] */, const int n_fext) {
    using L = Layout<P0, P1, P2>;
    using T = typename Lane<V>::S;
    constexpr int W = Lane<V>::W;                 // members per lane
    static_assert(!(INV && BINS), "no streamed histograms in the concentration-driven form");
    static_assert(!FORC || (!BINS && !COMP), "the forcing scales are carried by the plain forward and inverse forms only");
    constexpr int OWN = INV && (MISFIT || FORC) ? 1 : 0;                    // see member_step(): the step functions of their own
    constexpr int CHUNK = FusedForc<V, L, MISFIT, FORC, SCEN>::CHUNK;       // steps staged per refill
    constexpr bool FS_LDS = FusedForc<V, L, MISFIT, FORC, SCEN>::FS_LDS;    // FORC: the scales in a lane-private LDS slot
    static_assert(!MISFIT || (!BINS && !COMP), "the misfit is carried by the plain forward and inverse forms only");
    static_assert(!INV || !(MISFIT || FORC) || W == 1, "the concentration-driven form has no packed instantiation");
    static_assert(!SCEN || (!INV && !BINS && !COMP && !MISFIT), "the scenario axis is carried by the plain forward form only");
    if constexpr (SCEN) {
        const int64_t sc = blockIdx.y;
        drive += sc * n_steps * DRIVE_STRIDE;
        R += sc * L::SP * ld;
        S += sc * 2 * ld;
        if (C_traj != nullptr) C_traj += sc * n_rows * L::G * ld;
        if (T_traj != nullptr) T_traj += sc * n_rows * ld;
        if (stats != nullptr) stats += sc * ((ld + 63) >> 6) * n_steps * 4;
        if constexpr (FORC) fext += sc * n_steps * MAX_FEXT;         // a table per scenario; fscale is shared: not offset
    }
    __shared__ T drv[CHUNK * DRIVE_STRIDE];
    __shared__ T xs[FORC ? CHUNK * MAX_FEXT : 1];                     // FORC: the table chunk
    __shared__ V fs_s[FS_LDS ? (L::G + MAX_FEXT) * FIVEEQ_BLOCK : 1];  // FS_LDS: [G + MAX_FEXT][FIVEEQ_BLOCK], lane-private
    __shared__ double acc_s[MISFIT ? 3 * W * FIVEEQ_BLOCK : 1];       // MISFIT: [3 W][FIVEEQ_BLOCK], lane-private
    __shared__ V stat_tile[FIVEEQ_BLOCK / 64][STAT_STEPS * STAT_ROW];
    __shared__ KModel<T> km_s;
    // the LDS slot exists to keep WGS workgroups (four: 4 waves per SIMD) on a CU: a change that outgrows the budget must not pass
    static_assert(!FS_LDS || sizeof(drv) + sizeof(xs) + sizeof(fs_s) + sizeof(acc_s) + sizeof(stat_tile) + sizeof(km_s) <=
                                 LDS_PER_CU / FusedForc<V, L, MISFIT, FORC, SCEN>::WGS,
                  "FS_LDS form: the workgroups it is there to keep no longer fit a CU's LDS");
    stage_model(&km_s);
    const KModel<T>& kmr = km_s;

    const auto [m, active, full, mm] = lane_span<W, FIVEEQ_BLOCK, PARK_FIRST>(n);    // idle tail lanes shadow member 0 and store nothing
    const int64_t n_rec = (n + 63) >> 6;                                             // statistics records: one per 64 members
    const int64_t wave = (int64_t)blockIdx.x * (FIVEEQ_BLOCK / 64) + (threadIdx.x >> 6);
    const bool wave_live = stats != nullptr && wave * W < n_rec;
    V* const tile = stat_tile[threadIdx.x >> 6];
    const int n_valid = (int)min((int64_t)64 * W, n - wave * 64 * W);               // members of this wave (<= 0: none)
    int ks = 0;                                                                      // steps parked in the tile
    const HistRule<T> rule = make_rule(T(0), hist_lo, hist_inv_w, n_bins);           // (BINS only)

    V rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Cv[L::G], Tn, cum[L::G];
    V Rlo[L::SP];                                         // COMP: the compensation words (zero at launch: they do not cross HBM)
    if constexpr (COMP) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) Rlo[k] = (V)T(0);
    }
    if constexpr (INV) {
#pragma unroll
        for (int g = 0; g < L::G; ++g) cum[g] = cumE[g * ld + mm];
    }
#pragma unroll
    for (int k = 0; k < L::SP; ++k) Rv[k] = load_lane<V>(R + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = load_lane<V>(S + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 3 * L::G; ++k) rr[k] = load_lane<V>(r + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = load_lane<V>(q + k * ld + mm);
    V fs_r[FORC && !FS_LDS ? L::G + MAX_FEXT : 1];
    V* const fs = FS_LDS ? &fs_s[threadIdx.x] : fs_r;    // FORC: scale j of this lane at fs[j * FS_STRIDE]
    constexpr int FS_STRIDE = FS_LDS ? FIVEEQ_BLOCK : 1;
    if constexpr (FORC) {
#pragma unroll
        for (int k = 0; k < L::G + MAX_FEXT; ++k)
            fs[k * FS_STRIDE] = k < L::G + n_fext ? load_lane<V>(fscale + k * ld + mm) : (V)T(0);
    }
    double* const acc = &acc_s[threadIdx.x];             // MISFIT: word k of member j of this lane at acc[(3 j + k) * FIVEEQ_BLOCK]
    if constexpr (MISFIT) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t mj = (j == 0 || full) ? mm + j : mm;    // a packed lane's missing second member shadows the first
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[(3 * j + k) * FIVEEQ_BLOCK] = misfit[k * ld + mj];
        }
    }

    for (int tc = t_begin; tc < t_end; tc += CHUNK) {
        const int nt = min(CHUNK, t_end - tc);
        __syncthreads();                                  // previous chunk fully consumed
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_BLOCK)
            drv[i] = drive[(int64_t)tc * DRIVE_STRIDE + i];
        if constexpr (FORC) {
            // n_fext == 0: member_step reads no record and fext may be NULL — nothing is staged (a wave-uniform test)
            if (n_fext > 0)
                for (int i = threadIdx.x; i < nt * MAX_FEXT; i += FIVEEQ_BLOCK) xs[i] = fext[(int64_t)tc * MAX_FEXT + i];
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const T* d = &drv[k * DRIVE_STRIDE];
            if constexpr (FORC)
                member_step<V, L, INV, false, true, NoGasHook, OWN>(kmr, d, rr, qq, Rv, Sv, Cv, Tn, cum, Rlo, fs, FS_STRIDE,
                                                                    &xs[k * MAX_FEXT], n_fext);
            else
                member_step<V, L, INV, COMP, false, NoGasHook, OWN>(kmr, d, rr, qq, Rv, Sv, Cv, Tn, cum, Rlo);
            if constexpr (MISFIT) misfit_step(obs + (int64_t)(tc + k) * 4, Tn, acc, 3 * FIVEEQ_BLOCK, FIVEEQ_BLOCK, true);
            // the output row is wave-uniform: read it once into an SGPR so that the row test is a
            // scalar branch and the row offsets are scalar arithmetic, not 64-bit VALU per lane
            const int row = __builtin_amdgcn_readfirstlane((int)d[7]);
            if (row >= 0 && row < n_rows) {
                if (active) {
                    if (C_traj != nullptr) {
                        T* c = C_traj + (int64_t)row * L::G * ld + m;
#pragma unroll
                        for (int g = 0; g < L::G; ++g) store_lane(c + g * ld, Cv[g], full);
                    }
                    if (T_traj != nullptr) store_lane(T_traj + (int64_t)row * ld + m, Tn, full);
                }
            }
            if constexpr (BINS) {
                if (active) store_bin(bin_ring + (int64_t)((tc + k) % ring_rows) * ld + m, rule, Tn, full);
            }
            if (wave_live) {
                tile[ks * STAT_ROW + (threadIdx.x & 63)] = Tn;
                if (++ks == STAT_STEPS || tc + k + 1 == t_end) {
                    const int64_t t_first = (int64_t)(tc + k + 1 - ks);
                    if constexpr (W == 1) {
                        wave_stats_flush(tile, ks, n_valid, stats + (wave * n_steps + t_first) * 4, 4);
                    } else {
                        wave_stats_flush(tile, ks, n_valid, stats + (2 * wave * n_steps + t_first) * 4,
                                         2 * wave + 1 < n_rec ? stats + ((2 * wave + 1) * n_steps + t_first) * 4 : nullptr, 4);
                    }
                    ks = 0;
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) store_lane(R + k * ld + m, Rv[k], full);
#pragma unroll
        for (int k = 0; k < 2; ++k) store_lane(S + k * ld + m, Sv[k], full);
        if constexpr (INV) {
#pragma unroll
            for (int g = 0; g < L::G; ++g) cumE[g * ld + m] = cum[g];
        }
        if constexpr (MISFIT) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (j == 0 || full) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) misfit[k * ld + m + j] = acc[(3 * j + k) * FIVEEQ_BLOCK];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Kernel 2m — fused_kernel<V, P0, P1, P2, false, false, false, MISFIT, false, true> WITH A PER-MEMBER FORCING ROW PER STEP
// (member_step<.., MFORC>; fiveeq_run_mforc_*, include/fiveeq.h "MEMBER FORCING"): mforc [n_steps][ld].  The row is STREAMED,
// not resident: the lane loads its element of row t + 1 while it computes step t (one step ahead, as the small kernels read the
// drive record ahead) — w bytes per member-step in this form too; a packed fp32 lane loads its two members as one 8-byte
// access.  Everything else — the scales and where they live (FusedForc), the staged drive and table chunks, the misfit slot,
// the statistics tile, the stores — is fused_kernel's forward FORC form, statement for statement.
// A KERNEL OF ITS OWN, not one more flag of fused_kernel and not a body the two share: a template parameter would rename
// every fused_kernel symbol, and moving fused_kernel's text into a shared force-inlined body reordered the instructions of
// all 199 of its instantiations (profiles/r25/member_forcing_isa.txt).  This way every kernel that existed keeps its symbol
// and its machine code.  The {4} and 4 + 1 + 1 layouts, with and without the misfit.
// ---------------------------------------------------------------------------------
template <typename V, int P0, int P1, int P2, bool MISFIT = false>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void fused_mforc_kernel(
    const KModel<typename Lane<V>::S> km, const typename Lane<V>::S* __restrict__ drive, const int n_steps,
    const int t_begin, const int t_end, const int64_t n, const int64_t ld,
    const typename Lane<V>::S* __restrict__ r, const typename Lane<V>::S* __restrict__ q,
    typename Lane<V>::S* __restrict__ R, typename Lane<V>::S* __restrict__ S,
    typename Lane<V>::S* __restrict__ C_traj /* [n_rows][G][ld] or nullptr */,
    typename Lane<V>::S* __restrict__ T_traj /* [n_rows][ld] or nullptr */,
    const int n_rows, double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */,
    const double* __restrict__ obs /* MISFIT: [n_steps][4] */, double* __restrict__ misfit /* MISFIT: [3][ld] */,
    const typename Lane<V>::S* __restrict__ fscale /* [G + n_fext][ld] */,
    const typename Lane<V>::S* __restrict__ fext /* [n_steps][MAX_FEXT] */, const int n_fext,
    const typename Lane<V>::S* __restrict__ mforc /* [n_steps][ld] */) {
    using L = Layout<P0, P1, P2>;
    using T = typename Lane<V>::S;
    constexpr int W = Lane<V>::W;                 // members per lane
    constexpr int CHUNK = FusedForc<V, L, MISFIT, true>::CHUNK;       // steps staged per refill
    constexpr bool FS_LDS = FusedForc<V, L, MISFIT, true>::FS_LDS;    // the scales in a lane-private LDS slot
    __shared__ T drv[CHUNK * DRIVE_STRIDE];
    __shared__ T xs[CHUNK * MAX_FEXT];                                // the table chunk
    __shared__ V fs_s[FS_LDS ? (L::G + MAX_FEXT) * FIVEEQ_BLOCK : 1];  // FS_LDS: [G + MAX_FEXT][FIVEEQ_BLOCK], lane-private
    __shared__ double acc_s[MISFIT ? 3 * W * FIVEEQ_BLOCK : 1];       // MISFIT: [3 W][FIVEEQ_BLOCK], lane-private
    __shared__ V stat_tile[FIVEEQ_BLOCK / 64][STAT_STEPS * STAT_ROW];
    __shared__ KModel<T> km_s;
    static_assert(!FS_LDS || sizeof(drv) + sizeof(xs) + sizeof(fs_s) + sizeof(acc_s) + sizeof(stat_tile) + sizeof(km_s) <=
                                 LDS_PER_CU / FusedForc<V, L, MISFIT, true>::WGS,
                  "FS_LDS form: the workgroups it is there to keep no longer fit a CU's LDS");
    stage_model(&km_s);
    const KModel<T>& kmr = km_s;

    const auto [m, active, full, mm] = lane_span<W, FIVEEQ_BLOCK, PARK_FIRST>(n);    // idle tail lanes shadow member 0 and store nothing
    const int64_t n_rec = (n + 63) >> 6;                                             // statistics records: one per 64 members
    const int64_t wave = (int64_t)blockIdx.x * (FIVEEQ_BLOCK / 64) + (threadIdx.x >> 6);
    const bool wave_live = stats != nullptr && wave * W < n_rec;
    V* const tile = stat_tile[threadIdx.x >> 6];
    const int n_valid = (int)min((int64_t)64 * W, n - wave * 64 * W);               // members of this wave (<= 0: none)
    int ks = 0;                                                                      // steps parked in the tile

    V rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Cv[L::G], Tn;
    V no_cum[L::G], no_Rlo[L::SP];                       // never touched: INV = COMP = false
#pragma unroll
    for (int k = 0; k < L::SP; ++k) Rv[k] = load_lane<V>(R + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = load_lane<V>(S + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 3 * L::G; ++k) rr[k] = load_lane<V>(r + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = load_lane<V>(q + k * ld + mm);
    V fs_r[!FS_LDS ? L::G + MAX_FEXT : 1];
    V* const fs = FS_LDS ? &fs_s[threadIdx.x] : fs_r;    // scale j of this lane at fs[j * FS_STRIDE]
    constexpr int FS_STRIDE = FS_LDS ? FIVEEQ_BLOCK : 1;
#pragma unroll
    for (int k = 0; k < L::G + MAX_FEXT; ++k)
        fs[k * FS_STRIDE] = k < L::G + n_fext ? load_lane<V>(fscale + k * ld + mm) : (V)T(0);
    double* const acc = &acc_s[threadIdx.x];             // MISFIT: word k of member j of this lane at acc[(3 j + k) * FIVEEQ_BLOCK]
    if constexpr (MISFIT) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int64_t mj = (j == 0 || full) ? mm + j : mm;    // a packed lane's missing second member shadows the first
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[(3 * j + k) * FIVEEQ_BLOCK] = misfit[k * ld + mj];
        }
    }
    // the lane's element of the NEXT step's row, loaded a step ahead (an idle lane reads member 0's: mm; t < t_end <= n_mforc_rows)
    V mf_next = V();
    if (t_begin < t_end) mf_next = load_lane<V>(mforc + (int64_t)t_begin * ld + mm);

    for (int tc = t_begin; tc < t_end; tc += CHUNK) {
        const int nt = min(CHUNK, t_end - tc);
        __syncthreads();                                  // previous chunk fully consumed
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_BLOCK)
            drv[i] = drive[(int64_t)tc * DRIVE_STRIDE + i];
        // n_fext == 0: member_step reads no record and fext is not a table — nothing is staged (a wave-uniform test)
        if (n_fext > 0)
            for (int i = threadIdx.x; i < nt * MAX_FEXT; i += FIVEEQ_BLOCK) xs[i] = fext[(int64_t)tc * MAX_FEXT + i];
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const T* d = &drv[k * DRIVE_STRIDE];
            const V mf = mf_next;
            if (tc + k + 1 < t_end) mf_next = load_lane<V>(mforc + (int64_t)(tc + k + 1) * ld + mm);
            member_step<V, L, false, false, true, NoGasHook, 0, true>(kmr, d, rr, qq, Rv, Sv, Cv, Tn, no_cum, no_Rlo, fs, FS_STRIDE,
                                                                      &xs[k * MAX_FEXT], n_fext, NoGasHook{}, mf);
            if constexpr (MISFIT) misfit_step(obs + (int64_t)(tc + k) * 4, Tn, acc, 3 * FIVEEQ_BLOCK, FIVEEQ_BLOCK, true);
            const int row = __builtin_amdgcn_readfirstlane((int)d[7]);      // wave-uniform: a scalar branch, scalar row offsets
            if (row >= 0 && row < n_rows) {
                if (active) {
                    if (C_traj != nullptr) {
                        T* c = C_traj + (int64_t)row * L::G * ld + m;
#pragma unroll
                        for (int g = 0; g < L::G; ++g) store_lane(c + g * ld, Cv[g], full);
                    }
                    if (T_traj != nullptr) store_lane(T_traj + (int64_t)row * ld + m, Tn, full);
                }
            }
            if (wave_live) {
                tile[ks * STAT_ROW + (threadIdx.x & 63)] = Tn;
                if (++ks == STAT_STEPS || tc + k + 1 == t_end) {
                    const int64_t t_first = (int64_t)(tc + k + 1 - ks);
                    if constexpr (W == 1) {
                        wave_stats_flush(tile, ks, n_valid, stats + (wave * n_steps + t_first) * 4, 4);
                    } else {
                        wave_stats_flush(tile, ks, n_valid, stats + (2 * wave * n_steps + t_first) * 4,
                                         2 * wave + 1 < n_rec ? stats + ((2 * wave + 1) * n_steps + t_first) * 4 : nullptr, 4);
                    }
                    ks = 0;
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) store_lane(R + k * ld + m, Rv[k], full);
#pragma unroll
        for (int k = 0; k < 2; ++k) store_lane(S + k * ld + m, Sv[k], full);
        if constexpr (MISFIT) {
#pragma unroll
            for (int j = 0; j < W; ++j) {
                if (j == 0 || full) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) misfit[k * ld + m + j] = acc[(3 * j + k) * FIVEEQ_BLOCK];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------
// Kernel 2x — THE MIXED DRIVE (fiveeq_run_mixed_*, include/fiveeq.h "MIXED DRIVE"): fused_kernel's concentration-driven form
// with a PER-GAS drive mask CM (member_step<.., CM>): bit g set, gas g follows the target concentrations in drive[t][g], its
// cumulative emissions cumE[g] are the member's own and row g of X_traj receives the diagnosed E; bit g clear, gas g takes the
// emissions drive[t][g] and the shared cumulative emissions drive[t][3 + g] like a forward run and row g receives C.
// cumE [G][ld]: only the rows of concentration-driven gases are loaded and stored — the row of an emission-driven gas is never
// read and never written.  CM is a PROPER mask (neither 0 nor all gases: those two are the forward and the inverse kernel, which
// the host dispatches to); scalar lanes, one launch per span; MISFIT and FORC are the carriers of the inverse forms, in the
// places FusedForc gives them (the fp64 4 + 1 + 1 FORC forms keep the scales in the LDS slot and stage 25 steps per refill).
// A KERNEL OF ITS OWN, for fused_mforc_kernel's reason: one more template parameter would rename every fused_kernel symbol.  Its
// step functions are instantiated with OWN = 2, which no other kernel uses, so no kernel that existed shares one with it
// (member_step(): sharing moved the plain inverse kernel's schedule once).  profiles/r26/NOTES.md has the register counts.
// ---------------------------------------------------------------------------------
template <typename V, int P0, int P1, int P2, int CM, bool MISFIT = false, bool FORC = false>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void fused_mixed_kernel(
    const KModel<V> km, const V* __restrict__ drive, const int n_steps, const int t_begin, const int t_end, const int64_t n,
    const int64_t ld, const V* __restrict__ r, const V* __restrict__ q, V* __restrict__ R, V* __restrict__ S,
    V* __restrict__ cumE /* [G][ld]: rows of the gases in CM only */, V* __restrict__ X_traj /* [n_rows][G][ld] or nullptr */,
    V* __restrict__ T_traj /* [n_rows][ld] or nullptr */, const int n_rows,
    double* __restrict__ stats /* [ceil(n/64)][n_steps][4] or nullptr */, const double* __restrict__ obs /* MISFIT: [n_steps][4] */,
    double* __restrict__ misfit /* MISFIT: [3][ld] */, const V* __restrict__ fscale /* FORC: [G + n_fext][ld] */,
    const V* __restrict__ fext /* FORC: [n_steps][MAX_FEXT] */, const int n_fext) {
    using L = Layout<P0, P1, P2>;
    using T = V;
    static_assert(Lane<V>::W == 1, "the mixed drive has no packed instantiation");
    static_assert(CM > 0 && CM < (1 << L::G) - 1, "a proper mask: some gas concentration-driven, some gas emission-driven");
    constexpr int OWN = 2;                                                  // see member_step(): step functions of its own
    constexpr int CHUNK = FusedForc<V, L, MISFIT, FORC>::CHUNK;             // steps staged per refill
    constexpr bool FS_LDS = FusedForc<V, L, MISFIT, FORC>::FS_LDS;          // FORC: the scales in a lane-private LDS slot
    __shared__ T drv[CHUNK * DRIVE_STRIDE];
    __shared__ T xs[FORC ? CHUNK * MAX_FEXT : 1];                     // FORC: the table chunk
    __shared__ V fs_s[FS_LDS ? (L::G + MAX_FEXT) * FIVEEQ_BLOCK : 1];  // FS_LDS: [G + MAX_FEXT][FIVEEQ_BLOCK], lane-private
    __shared__ double acc_s[MISFIT ? 3 * FIVEEQ_BLOCK : 1];           // MISFIT: [3][FIVEEQ_BLOCK], lane-private
    __shared__ V stat_tile[FIVEEQ_BLOCK / 64][STAT_STEPS * STAT_ROW];
    __shared__ KModel<T> km_s;
    static_assert(!FS_LDS || sizeof(drv) + sizeof(xs) + sizeof(fs_s) + sizeof(acc_s) + sizeof(stat_tile) + sizeof(km_s) <=
                                 LDS_PER_CU / FusedForc<V, L, MISFIT, FORC>::WGS,
                  "FS_LDS form: the workgroups it is there to keep no longer fit a CU's LDS");
    stage_model(&km_s);
    const KModel<T>& kmr = km_s;

    const auto [m, active, full, mm] = lane_span<1, FIVEEQ_BLOCK, PARK_FIRST>(n);    // idle tail lanes shadow member 0 and store nothing
    const int64_t n_rec = (n + 63) >> 6;                                             // statistics records: one per 64 members
    const int64_t wave = (int64_t)blockIdx.x * (FIVEEQ_BLOCK / 64) + (threadIdx.x >> 6);
    const bool wave_live = stats != nullptr && wave < n_rec;
    V* const tile = stat_tile[threadIdx.x >> 6];
    const int n_valid = (int)min((int64_t)64, n - wave * 64);                        // members of this wave (<= 0: none)
    int ks = 0;                                                                      // steps parked in the tile

    V rr[3 * L::G], qq[2], Rv[L::SP], Sv[2], Xv[L::G], Tn, cum[L::G];
    V no_Rlo[L::SP];                                      // never touched: COMP = false
#pragma unroll
    for (int g = 0; g < L::G; ++g) {
        if (CM >> g & 1) cum[g] = cumE[g * ld + mm];      // an emission-driven gas: its row is not read, cum[g] is not used
    }
#pragma unroll
    for (int k = 0; k < L::SP; ++k) Rv[k] = load_lane<V>(R + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) Sv[k] = load_lane<V>(S + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 3 * L::G; ++k) rr[k] = load_lane<V>(r + k * ld + mm);
#pragma unroll
    for (int k = 0; k < 2; ++k) qq[k] = load_lane<V>(q + k * ld + mm);
    V fs_r[FORC && !FS_LDS ? L::G + MAX_FEXT : 1];
    V* const fs = FS_LDS ? &fs_s[threadIdx.x] : fs_r;    // FORC: scale j of this lane at fs[j * FS_STRIDE]
    constexpr int FS_STRIDE = FS_LDS ? FIVEEQ_BLOCK : 1;
    if constexpr (FORC) {
#pragma unroll
        for (int k = 0; k < L::G + MAX_FEXT; ++k)
            fs[k * FS_STRIDE] = k < L::G + n_fext ? load_lane<V>(fscale + k * ld + mm) : (V)T(0);
    }
    double* const acc = &acc_s[threadIdx.x];             // MISFIT: word k of this lane's member at acc[k * FIVEEQ_BLOCK]
    if constexpr (MISFIT) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k * FIVEEQ_BLOCK] = misfit[k * ld + mm];
    }

    for (int tc = t_begin; tc < t_end; tc += CHUNK) {
        const int nt = min(CHUNK, t_end - tc);
        __syncthreads();                                  // previous chunk fully consumed
        for (int i = threadIdx.x; i < nt * DRIVE_STRIDE; i += FIVEEQ_BLOCK)
            drv[i] = drive[(int64_t)tc * DRIVE_STRIDE + i];
        if constexpr (FORC) {
            // n_fext == 0: member_step reads no record and fext is not a table — nothing is staged (a wave-uniform test)
            if (n_fext > 0)
                for (int i = threadIdx.x; i < nt * MAX_FEXT; i += FIVEEQ_BLOCK) xs[i] = fext[(int64_t)tc * MAX_FEXT + i];
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k) {
            const T* d = &drv[k * DRIVE_STRIDE];
            if constexpr (FORC)
                member_step<V, L, true, false, true, NoGasHook, OWN, false, CM>(kmr, d, rr, qq, Rv, Sv, Xv, Tn, cum, no_Rlo, fs,
                                                                                FS_STRIDE, &xs[k * MAX_FEXT], n_fext);
            else
                member_step<V, L, true, false, false, NoGasHook, OWN, false, CM>(kmr, d, rr, qq, Rv, Sv, Xv, Tn, cum, no_Rlo);
            if constexpr (MISFIT) misfit_step(obs + (int64_t)(tc + k) * 4, Tn, acc, 3 * FIVEEQ_BLOCK, FIVEEQ_BLOCK, true);
            const int row = __builtin_amdgcn_readfirstlane((int)d[7]);      // wave-uniform: a scalar branch, scalar row offsets
            if (row >= 0 && row < n_rows) {
                if (active) {
                    if (X_traj != nullptr) {
                        T* c = X_traj + (int64_t)row * L::G * ld + m;
#pragma unroll
                        for (int g = 0; g < L::G; ++g) store_lane(c + g * ld, Xv[g], full);
                    }
                    if (T_traj != nullptr) store_lane(T_traj + (int64_t)row * ld + m, Tn, full);
                }
            }
            if (wave_live) {
                tile[ks * STAT_ROW + (threadIdx.x & 63)] = Tn;
                if (++ks == STAT_STEPS || tc + k + 1 == t_end) {
                    const int64_t t_first = (int64_t)(tc + k + 1 - ks);
                    wave_stats_flush(tile, ks, n_valid, stats + (wave * n_steps + t_first) * 4, 4);
                    ks = 0;
                }
            }
        }
    }
    if (active) {
#pragma unroll
        for (int k = 0; k < L::SP; ++k) store_lane(R + k * ld + m, Rv[k], full);
#pragma unroll
        for (int k = 0; k < 2; ++k) store_lane(S + k * ld + m, Sv[k], full);
#pragma unroll
        for (int g = 0; g < L::G; ++g) {
            if (CM >> g & 1) cumE[g * ld + m] = cum[g];   // an emission-driven gas: its row is not written
        }
        if constexpr (MISFIT) {
#pragma unroll
            for (int k = 0; k < 3; ++k) misfit[k * ld + m] = acc[k * FIVEEQ_BLOCK];
        }
    }
}

}  // namespace fiveeq
