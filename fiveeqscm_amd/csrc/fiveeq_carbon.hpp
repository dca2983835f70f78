// fiveeq_carbon.hpp — kernel 16: CARBON ROWS, the airborne emissions, the cumulative emissions and uptake, the airborne
// fraction, the iIRF100, the lifetime scaling alpha and the sink flux of a run diagnosed from its STORED rows
// (include/fiveeq.h, "CARBON ROWS").
// Part of fiveeq_device.hpp, which includes it after fiveeq_noise.hpp: include that header, not this one.
//
// gas_step() forms G_a, G_u, the iIRF and alpha in registers and drops them.  They are functions of what a run stores (C, or
// for a concentration-driven gas the diagnosed emissions E, and T), of the member's r0, rC, rT and of the shared drive table, so
// one streaming pass recomputes them afterwards.  Per row k holding step t = steps[k], gas g, member m, every operation rounded
// on its own in the rows' precision unless an fma is written:
//     emission-driven gas (conc_mask bit clear):  C_g = the stored row,  E = drive[t][g],  cumE = cum_end[t][g]  (shared: the
//                                                 cumulative emissions at the END of step t, formed by the host in fp64)
//     concentration-driven gas (bit set):         C_g = drive[t][g],  E = the stored row,  cum = fma(E, dt, cum)  (THE statement
//                                                 of gas_step<INV>),  cumE = cum                                  (SEQ only)
//     G_a   = (C_g - C0) * inv_c                  airborne emissions
//     G_u   = cumE - G_a                          cumulative uptake
//     AF    = G_a / cumE                          airborne fraction, IEEE division (0/0 and x/0 as IEEE gives them)
//     iirf  = fe_min(fma3(ra, G_a, fma3(rT, T, fma3(rC, G_u, r0))), iirf_max)     the statements of gas_step(); T the row's stored
//     alpha = g0 * fe_exp(iirf * inv_g1)          T, so these are the values the NEXT step uses
//     sink  = E - (G_a - G_a_prev) / dt           IEEE division; G_a_prev carried through the rows             (SEQ only)
//   16  carbon_rows_kernel<T, VEC, SEQ>    VEC: 16-byte row accesses (every lane has all its members), else element accesses —
//                                          the ragged tail, unaligned rows;  SEQ: a lane carries cum and G_a_prev of its members
//                                          through all rows (grid.y = 1); else the rows are independent and blocks of
//                                          CARBON_YROWS rows are spread over grid.y
// A lane owns METRICS_LANE<T> consecutive members (16 bytes of a row).  Only the gases of gas_mask are read and written; output
// (k, slot, m) of a selected gas is out[(k n_sel + slot) ld_out + m], slot counting the selected gases below it.  Per member the
// lane loads once the three r rows of each selected gas (only when iirf or alpha is asked for) and the carried state; per row it
// reads the selected gases' stored rows, the T row only when iirf or alpha is asked for, and writes only the outputs asked for —
// rows read and written with the non-temporal policy.  What the members share per row — drive[t][g] and cum_end[t][g] — is
// staged into LDS by one thread per row, FIVEEQ_BLOCK rows a time, and read back by broadcast ds_reads; the model's constants
// come from the kernel arguments (scalar loads).  No floating-point atomics, no scratch; no output bit depends on the launch
// shape, on a stride or on how the rows and members are split over calls.
// fe_min is IEEE minNum, here as in gas_step(): a NaN iIRF reads iirf_max, so a NaN stored value makes the row's airborne,
// uptake, fraction and sink NaN and its iirf / alpha those of iirf_max — what the stepping kernel would have used.
// COPIES OF THIS HEADER'S OWN.  The iirf and alpha statements are carbon_alpha() below, not a function shared with gas_step():
// factoring them out of gas_step() changed the machine code of two fused_kernel instantiations that existed
// (profiles/r28/NOTES.md), so gas_step() stays as it was.  The row loads go through CarbonLoad (the text of MetricsLoad):
// sharing MetricsLoad's element-load instantiations with the kernels that existed moved their machine code in r27
// (profiles/r27/NOTES.md).
#pragma once

namespace fiveeq {

// rows whose loads are issued before the first is used: 16-byte loads / the element-access path, halved where a lane also
// carries its members' state through the rows (SEQ: registers)
template <bool VEC, bool SEQ> constexpr int CARBON_UNROLL = (VEC ? 4 : 2) / (SEQ ? 2 : 1);
constexpr int CARBON_YROWS = 16;                               // rows per workgroup of the row-parallel form (SEQ = false)
template <typename T> constexpr int CARBON_TILE = METRICS_LANE<T> * FIVEEQ_BLOCK;   // members per workgroup
enum CarbonOut { CARBON_AIRBORNE, CARBON_CUME, CARBON_UPTAKE, CARBON_FRACTION, CARBON_IIRF, CARBON_ALPHA, CARBON_SINK, CARBON_N_OUT };

// the arguments of one launch besides the model: n members from column 0 of every row (the host offsets the pointers for the
// ragged tail's launch).  A NULL pointer is an input not read or an output not written; Trows and r are NULL unless iirf or
// alpha is asked for (the host sees to it).
template <typename T>
struct CarbonArgs {
    int n_gas, n_rows, n, n_steps, conc_mask, gas_mask, n_sel;
    const T* rows;                                             // element (k, g, m) at rows[k c_row + g c_gas + m]: C, or E (driven gas)
    int64_t c_row, c_gas;
    const T* Trows;                                            // element (k, m) at Trows[k t_row + m]
    int64_t t_row;
    const int* steps;                                          // [n_rows]
    const T* drive;                                            // [n_steps][DRIVE_STRIDE]: E_g, or the target C_g, at [g]
    const T* cum_end;                                          // [n_steps][MAX_GAS]: cumulative emissions at the end of the step
    const T* r;                                                // [3 G][ld]: r0, rC, rT of gas 0, then of gas 1, ...
    int64_t ld;
    T* out[CARBON_N_OUT];                                      // each [n_rows][n_sel][ld_out]
    int64_t ld_out;
    T* cum_io;                                                 // [G][ld]: cum of the concentration-driven gases
    T* ga_io;                                                  // [G][ld]: G_a before the first row / after the last
};

template <typename T, bool VEC>
struct CarbonLoad {
    using V = typename MetricsVec<T>::V;
    static constexpr int M = METRICS_LANE<T>;
    V v;
    __device__ __forceinline__ void load(const T* p, const int live) {
        if constexpr (VEC) v = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
        else {
#pragma unroll
            for (int j = 0; j < M; ++j) v[j] = __builtin_nontemporal_load(p + (j < live ? j : live - 1));
        }
    }
};

// M members of a lane to one row: VEC, one 16-byte non-temporal store; else the members that exist, one element each.
template <typename T, int M, bool VEC>
__device__ __forceinline__ void carbon_store(T* p, const T (&v)[M], const int live) {
    if constexpr (VEC) {
        using V = typename MetricsVec<T>::V;
        V vv;
#pragma unroll
        for (int j = 0; j < M; ++j) vv[j] = v[j];
        __builtin_nontemporal_store(vv, reinterpret_cast<V*>(p));
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (j < live) __builtin_nontemporal_store(v[j], p + j);
    }
}

// THE LIFETIME SCALING OF ONE GAS: the iirf and alpha statements of gas_step() (fiveeq_member.hpp, "alpha_val"), operation for
// operation — a copy of this header's own, see the header comment.  A change of either is a change of both: the GPU tests hold
// the pass to the stepping kernels' cumE in bits and to the oracle's alpha (tests/test_carbon_rows_gpu.py).
template <typename T>
__device__ __forceinline__ T carbon_alpha(const KGas<T>& kg, const T iirf_max, const T r0, const T rC, const T rT, const T T_old,
                                          const T G_a, const T G_u, T& iirf) {
    iirf = fma3<T>(kg.ra, G_a, fma3<T>(rT, T_old, fma3<T>(rC, G_u, r0)));
    iirf = fe_min(iirf, iirf_max);
    return kg.g0 * fe_exp(iirf * kg.inv_g1);
}

// what a lane keeps per member: the r rows loaded once and, SEQ, the carried state
template <typename T>
struct CarbonLane {
    static constexpr int M = METRICS_LANE<T>;
    T rr[MAX_GAS][3][M];                                       // r0, rC, rT
    T cum[MAX_GAS][M];                                         // cumulative emissions of a concentration-driven gas
    T ga[MAX_GAS][M];                                          // G_a of the row before
};

// ONE ROW of the lane: row k of the call, its shared record (dr = drive[t][0..G), ce = cum_end[t][0..G): LDS), its loaded
// stored rows and T row.
template <typename T, bool VEC, bool SEQ>
__device__ __forceinline__ void carbon_row(const KModel<T>& km, const CarbonArgs<T>& a, const int k, const int64_t m, const int live,
                                           const T* dr, const T* ce, const CarbonLoad<T, VEC> (&x)[MAX_GAS],
                                           const CarbonLoad<T, VEC>& tr, CarbonLane<T>& s) {
    constexpr int M = METRICS_LANE<T>;
    const bool want_alpha = a.out[CARBON_IIRF] || a.out[CARBON_ALPHA];
    int slot = 0;
#pragma unroll
    for (int g = 0; g < MAX_GAS; ++g) {
        if (g < a.n_gas && (a.gas_mask >> g & 1)) {
            const KGas<T>& kg = km.gas[g];
            const bool conc = a.conc_mask >> g & 1;
            const T shared = dr[g], shared_cum = ce[g];
            const int64_t at = ((int64_t)k * a.n_sel + slot) * a.ld_out + m;
            T E[M], Ga[M], cE[M], Gu[M];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                const T xv = x[g].v[j];
                const T Cg = conc ? shared : xv;
                E[j] = conc ? xv : shared;
                if constexpr (SEQ) {
                    if (conc) s.cum[g][j] = fe_fma(xv, km.dt, s.cum[g][j]);
                }
                cE[j] = conc ? s.cum[g][j] : shared_cum;
                Ga[j] = (Cg - kg.C0) * kg.inv_c;
                Gu[j] = cE[j] - Ga[j];
            }
            if (a.out[CARBON_AIRBORNE]) carbon_store<T, M, VEC>(a.out[CARBON_AIRBORNE] + at, Ga, live);
            if (a.out[CARBON_CUME]) carbon_store<T, M, VEC>(a.out[CARBON_CUME] + at, cE, live);
            if (a.out[CARBON_UPTAKE]) carbon_store<T, M, VEC>(a.out[CARBON_UPTAKE] + at, Gu, live);
            if (a.out[CARBON_FRACTION]) {
                T AF[M];
#pragma unroll
                for (int j = 0; j < M; ++j) AF[j] = Ga[j] / cE[j];
                carbon_store<T, M, VEC>(a.out[CARBON_FRACTION] + at, AF, live);
            }
            if (want_alpha) {
                T ii[M], al[M];
#pragma unroll
                for (int j = 0; j < M; ++j)
                    al[j] = carbon_alpha<T>(kg, km.iirf_max, s.rr[g][0][j], s.rr[g][1][j], s.rr[g][2][j], tr.v[j], Ga[j], Gu[j], ii[j]);
                if (a.out[CARBON_IIRF]) carbon_store<T, M, VEC>(a.out[CARBON_IIRF] + at, ii, live);
                if (a.out[CARBON_ALPHA]) carbon_store<T, M, VEC>(a.out[CARBON_ALPHA] + at, al, live);
            }
            if constexpr (SEQ) {
                if (a.ga_io) {
                    T sk[M];
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        sk[j] = E[j] - (Ga[j] - s.ga[g][j]) / km.dt;
                        s.ga[g][j] = Ga[j];
                    }
                    if (a.out[CARBON_SINK]) carbon_store<T, M, VEC>(a.out[CARBON_SINK] + at, sk, live);
                }
            }
            ++slot;
        }
    }
}

// 16.  The arguments as in CarbonArgs.  VEC: every row pointer and stride allows 16-byte accesses and n is a multiple of the
// lane's members (the host has checked, and hands the ragged tail to a second launch without VEC).  A step outside [0, n_steps)
// is clamped into it: the kernel never reads outside the tables (the caller owes valid steps).  Columns [n, ..) of the outputs
// and of the carried state are never written.
template <typename T, bool VEC, bool SEQ>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void carbon_rows_kernel(const KModel<T> km, const CarbonArgs<T> a) {
    constexpr int M = METRICS_LANE<T>, UN = CARBON_UNROLL<VEC, SEQ>;
    __shared__ T s_drive[FIVEEQ_BLOCK][MAX_GAS];
    __shared__ T s_cum[FIVEEQ_BLOCK][MAX_GAS];
    const int tid = threadIdx.x;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + tid) * M;              // the lane's first member
    const bool active = m < a.n;                                                  // (no early return: the lane takes part in the barriers)
    const int live = !active ? 0 : a.n - m < M ? (int)(a.n - m) : M;              // members of this lane that exist
    const int k_begin = SEQ ? 0 : (int)blockIdx.y * CARBON_YROWS;
    const int k_end = SEQ ? a.n_rows : (k_begin + CARBON_YROWS < a.n_rows ? k_begin + CARBON_YROWS : a.n_rows);

    // per member, once: the r rows and the carried state; member j read at column min(j, live - 1) like the rows: what a
    // missing member holds is never stored
    CarbonLane<T> s;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int64_t col = m + (j < live ? j : live - 1);
#pragma unroll
        for (int g = 0; g < MAX_GAS; ++g) {
            const bool sel = active && g < a.n_gas && (a.gas_mask >> g & 1);
#pragma unroll
            for (int i = 0; i < 3; ++i) s.rr[g][i][j] = sel && a.r ? a.r[(3 * g + i) * a.ld + col] : T(0);
            s.cum[g][j] = SEQ && sel && a.cum_io && (a.conc_mask >> g & 1) ? a.cum_io[g * a.ld + col] : T(0);
            s.ga[g][j] = SEQ && sel && a.ga_io ? a.ga_io[g * a.ld + col] : T(0);
        }
    }

    for (int kc = k_begin; kc < k_end; kc += FIVEEQ_BLOCK) {
        // ---- the shared records of rows [kc, kc + FIVEEQ_BLOCK): one thread per row ----------------------------------------
        __syncthreads();                                       // the last chunk's records are read to their end
        if (kc + tid < k_end) {
            int t = a.steps[kc + tid];
            t = t < 0 ? 0 : t >= a.n_steps ? a.n_steps - 1 : t;
#pragma unroll
            for (int g = 0; g < MAX_GAS; ++g) {
                s_drive[tid][g] = g < a.n_gas ? a.drive[(int64_t)t * DRIVE_STRIDE + g] : T(0);
                s_cum[tid][g] = a.cum_end && g < a.n_gas ? a.cum_end[(int64_t)t * MAX_GAS + g] : T(0);
            }
        }
        __syncthreads();
        if (!active) continue;
        const int nr = k_end - kc < FIVEEQ_BLOCK ? k_end - kc : FIVEEQ_BLOCK;
        // ---- the row loop: the loads of UN rows in flight before the first is used -----------------------------------------
        const T* px = a.rows + m;
        const T* pt = a.Trows + m;
        int i = 0;
        for (; i + UN <= nr; i += UN) {
            CarbonLoad<T, VEC> x[UN][MAX_GAS], tr[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
#pragma unroll
                for (int g = 0; g < MAX_GAS; ++g)
                    if (g < a.n_gas && (a.gas_mask >> g & 1)) x[u][g].load(px + (int64_t)(kc + i + u) * a.c_row + g * a.c_gas, live);
                if (a.Trows) tr[u].load(pt + (int64_t)(kc + i + u) * a.t_row, live);
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) carbon_row<T, VEC, SEQ>(km, a, kc + i + u, m, live, s_drive[i + u], s_cum[i + u], x[u], tr[u], s);
        }
        for (; i < nr; ++i) {
            CarbonLoad<T, VEC> x[MAX_GAS], tr;
#pragma unroll
            for (int g = 0; g < MAX_GAS; ++g)
                if (g < a.n_gas && (a.gas_mask >> g & 1)) x[g].load(px + (int64_t)(kc + i) * a.c_row + g * a.c_gas, live);
            if (a.Trows) tr.load(pt + (int64_t)(kc + i) * a.t_row, live);
            carbon_row<T, VEC, SEQ>(km, a, kc + i, m, live, s_drive[i], s_cum[i], x, tr, s);
        }
    }

    if constexpr (SEQ) {
        if (active) {
#pragma unroll
            for (int g = 0; g < MAX_GAS; ++g) {
                if (g < a.n_gas && (a.gas_mask >> g & 1)) {
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        if (j < live) {
                            if (a.cum_io && (a.conc_mask >> g & 1)) a.cum_io[g * a.ld + m + j] = s.cum[g][j];
                            if (a.ga_io) a.ga_io[g * a.ld + m + j] = s.ga[g][j];
                        }
                    }
                }
            }
        }
    }
}

}  // namespace fiveeq
