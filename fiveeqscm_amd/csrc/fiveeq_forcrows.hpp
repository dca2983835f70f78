// fiveeq_forcrows.hpp — kernel 12: FORCING ROWS, the effective radiative forcing, the energy imbalance and the heat uptake of a
// run diagnosed from its STORED rows (include/fiveeq.h, "FORCING ROWS").
// Part of fiveeq_device.hpp, which includes it after fiveeq_score.hpp: include that header, not this one.
//
// member_step() forms the forcing F in registers, spends it on the two thermal boxes and drops it.  F is a pure function of
// what a run stores — the step's concentrations C_g, the member's forcing scales, the step's shared F_ext and category record —
// so one streaming pass recomputes it afterwards, for rows of every mode, with the arithmetic the stepping kernels used:
//     F_g = gas_forcing(C_g)                        (fiveeq_member.hpp: THE function gas_step() calls; it exists once)
//     F   = F_ext[t];  F = fma(sx_k, X[t][k], F);  F = fma(sg_g, F_g, F) with forcing scales,  F += F_g without
//     N   = F - T / (q0 + q1)                       each operation rounded on its own, IEEE division, in the rows' precision
//     H  += dt * (double)N                          one fp64 accumulator per member, rows in ascending order
//     S_j = fma(em1_d[j], fma(-q_j, F, S_j), S_j);  T' = S_0 + S_1      (THE REPLAY: member_step()'s step_temp on the diagnosed F;
//                                                                      T' is compared in bits with the stored T, NaN equal to NaN)
//   12  forcing_rows_kernel<T, VEC, SEQ>   VEC: 16-byte row accesses (every lane has all its members), else element accesses —
//                                          the ragged tail, unaligned rows;  SEQ: H or the replay is asked for, so a lane carries
//                                          its members through all rows (grid.y = 1); else the rows are independent and blocks
//                                          of FORCROWS_YROWS rows are spread over grid.y
// A lane owns METRICS_LANE<T> consecutive members (16 bytes of a row).  Per member it loads once q[2] (when T rows are read) and
// the G + K scales; per row it reads the G concentration rows, the T row only when N, H or the replay is asked for, and writes
// only the outputs asked for — rows read and written with the non-temporal policy.  What the members share per row — F_ext[t]
// and X[t][0..K) of the row's step t = steps[k] — is staged into LDS by one thread per row, FIVEEQ_BLOCK rows a time, and read
// back by broadcast ds_reads; the model's constants come from the kernel arguments (scalar loads).  No floating-point atomics,
// no scratch; no output bit depends on the launch shape, on a stride or on how the rows are split over calls.  The replay's
// mismatch count is the one integer result: lanes that found any add theirs with a 64-bit integer atomic.
#pragma once

namespace fiveeq {

// rows whose loads are issued before the first is used: 16-byte loads / the element-access path, halved where a lane also
// carries its members' state through the rows (SEQ: registers)
template <bool VEC, bool SEQ> constexpr int FORCROWS_UNROLL = (VEC ? 4 : 2) / (SEQ ? 2 : 1);
constexpr int FORCROWS_YROWS = 16;                             // rows per workgroup of the row-parallel form (SEQ = false)
template <typename T> constexpr int FORCROWS_TILE = METRICS_LANE<T> * FIVEEQ_BLOCK;  // members per workgroup

// the arguments of one launch besides the model: n members from column 0 of every row (the host offsets the pointers for the
// ragged tail's launch).  A NULL pointer is an input not read or an output not written; Trows is NULL unless N, H, H_io or S_io
// is there (the host sees to it).
template <typename T>
struct ForcRowsArgs {
    int n_gas, n_rows, n, n_steps, n_fext;
    const T* C;                                                // element (k, g, m) at C[k c_row + g c_gas + m]
    int64_t c_row, c_gas;
    const T* Trows;                                            // element (k, m) at Trows[k t_row + m]
    int64_t t_row;
    const int* steps;                                          // [n_rows]
    const T* drive;                                            // [n_steps][DRIVE_STRIDE], F_ext at [6]
    const T* q;                                                // [2][ld]
    const T* fs;                                               // [G + K][ld], gas rows first; NULL: the plain sum F += F_g
    const T* X;                                                // [n_steps][MAX_FEXT]
    int64_t ld;
    T* F;                                                      // [n_rows][ld_out]
    T* Fg;                                                     // [n_rows][G][ld_out]
    T* N;                                                      // [n_rows][ld_out]
    double* H;                                                 // [n_rows][ld_out]
    int64_t ld_out;
    double* H_io;                                              // [ld]
    T* S_io;                                                   // [2][ld]
    unsigned long long* n_mismatch;
    double dt;
};

__device__ __forceinline__ long long forcrows_bits(const double v) { return __double_as_longlong(v); }
__device__ __forceinline__ int forcrows_bits(const float v) { return __float_as_int(v); }

// M members of a lane to one row: VEC, 16-byte non-temporal stores (one for elements of the rows' type, two for the fp64 H of
// fp32 rows); else the members that exist, one element each.
template <typename TO, int M, bool VEC>
__device__ __forceinline__ void forcrows_store(TO* p, const TO (&v)[M], const int live) {
    if constexpr (VEC) {
        using V = typename MetricsVec<TO>::V;
        constexpr int PER = 16 / (int)sizeof(TO);
#pragma unroll
        for (int c = 0; c < M; c += PER) {
            V vv;
#pragma unroll
            for (int j = 0; j < PER; ++j) vv[j] = v[c + j];
            __builtin_nontemporal_store(vv, reinterpret_cast<V*>(p + c));
        }
    } else {
#pragma unroll
        for (int j = 0; j < M; ++j)
            if (j < live) __builtin_nontemporal_store(v[j], p + j);
    }
}

// what a lane keeps per member: the constants loaded once and, SEQ, the carried state
template <typename T>
struct ForcRowsLane {
    static constexpr int M = METRICS_LANE<T>;
    T q0[M], q1[M], qs[M];                                     // q_1, q_2 and q_1 + q_2 (1 / feedback parameter)
    T sg[MAX_GAS][M], sx[MAX_FEXT][M];                         // the forcing scales
    double H[M];
    T S0[M], S1[M];
    int mismatches;
};

// THE FORCING OF ONE ROW of a lane's M members from the row's shared record (fext, xr) and its loaded C rows: F_ext, then the
// categories by fma, then the gases through gas_forcing() — fma with the scales (scaled), the plain sum without.  Written
// ONCE: forcrows_row() below and the pulse-response pass (fiveeq_pulse.hpp) call it, so the two cannot drift apart.
// fg_out(g, Fg) is handed every gas's forcing as it is formed (kernel 12 stores it when F_gas is asked for).
template <typename T, bool VEC, typename FgOut>
__device__ __forceinline__ void forcrows_F(const KModel<T>& km, const int n_gas, const int n_fext, const bool scaled, const T fext,
                                           const T* xr, const MetricsLoad<T, VEC> (&c)[MAX_GAS],
                                           const T (&sg)[MAX_GAS][METRICS_LANE<T>], const T (&sx)[MAX_FEXT][METRICS_LANE<T>],
                                           T (&F)[METRICS_LANE<T>], FgOut&& fg_out) {
    constexpr int M = METRICS_LANE<T>;
#pragma unroll
    for (int j = 0; j < M; ++j) F[j] = fext;
    if (scaled) {
#pragma unroll
        for (int x = 0; x < MAX_FEXT; ++x) {
            if (x < n_fext) {
                const T xv = xr[x];
#pragma unroll
                for (int j = 0; j < M; ++j) F[j] = fe_fma(sx[x][j], xv, F[j]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < MAX_GAS; ++g) {
        if (g < n_gas) {
            T Fg[M];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                Fg[j] = gas_forcing<T>(km.gas[g], c[g].v[j]);
                F[j] = scaled ? fe_fma(sg[g][j], Fg[j], F[j]) : F[j] + Fg[j];
            }
            fg_out(g, Fg);
        }
    }
}

// ONE ROW of the lane: row k of the call, its shared record (fext, xr: LDS), its loaded C rows and T row.
template <typename T, bool VEC, bool SEQ>
__device__ __forceinline__ void forcrows_row(const KModel<T>& km, const ForcRowsArgs<T>& a, const int k, const int64_t m, const int live,
                                             const T fext, const T* xr, const MetricsLoad<T, VEC> (&c)[MAX_GAS],
                                             const MetricsLoad<T, VEC>& tr, ForcRowsLane<T>& s) {
    constexpr int M = METRICS_LANE<T>;
    T F[M];
    forcrows_F<T, VEC>(km, a.n_gas, a.n_fext, a.fs != nullptr, fext, xr, c, s.sg, s.sx, F, [&](const int g, const T (&Fg)[M]) {
        if (a.Fg) forcrows_store<T, M, VEC>(a.Fg + ((int64_t)k * a.n_gas + g) * a.ld_out + m, Fg, live);
    });
    if (a.F) forcrows_store<T, M, VEC>(a.F + (int64_t)k * a.ld_out + m, F, live);
    if (a.Trows) {
        T Nn[M];
#pragma unroll
        for (int j = 0; j < M; ++j) Nn[j] = F[j] - tr.v[j] / s.qs[j];
        if (a.N) forcrows_store<T, M, VEC>(a.N + (int64_t)k * a.ld_out + m, Nn, live);
        if constexpr (SEQ) {
            if (a.H || a.H_io) {
#pragma unroll
                for (int j = 0; j < M; ++j) s.H[j] = s.H[j] + a.dt * (double)Nn[j];
                if (a.H) forcrows_store<double, M, VEC>(a.H + (int64_t)k * a.ld_out + m, s.H, live);
            }
            if (a.S_io) {
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    s.S0[j] = fe_fma(km.em1_d[0], fe_fma(-s.q0[j], F[j], s.S0[j]), s.S0[j]);
                    s.S1[j] = fe_fma(km.em1_d[1], fe_fma(-s.q1[j], F[j], s.S1[j]), s.S1[j]);
                    const T Tp = s.S0[j] + s.S1[j], Ts = tr.v[j];
                    const bool same = forcrows_bits(Tp) == forcrows_bits(Ts) || (Tp != Tp && Ts != Ts);
                    s.mismatches += !same && j < live ? 1 : 0;
                }
            }
        }
    }
}

// 12.  The arguments as in ForcRowsArgs.  VEC: every row pointer and stride allows 16-byte accesses and n is a multiple of the
// lane's members (the host has checked, and hands the ragged tail to a second launch without VEC).  A step outside [0, n_steps)
// is clamped into it: the kernel never reads outside the tables (the caller owes valid steps).  Columns [n, ..) of the outputs
// and of the carried state are never written.
template <typename T, bool VEC, bool SEQ>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void forcing_rows_kernel(const KModel<T> km, const ForcRowsArgs<T> a) {
    constexpr int M = METRICS_LANE<T>, UN = FORCROWS_UNROLL<VEC, SEQ>;
    __shared__ T s_fext[FIVEEQ_BLOCK];
    __shared__ T s_x[FIVEEQ_BLOCK][MAX_FEXT];
    const int tid = threadIdx.x;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + tid) * M;              // the lane's first member
    const bool active = m < a.n;                                                  // (no early return: the lane takes part in the barriers)
    const int live = !active ? 0 : a.n - m < M ? (int)(a.n - m) : M;              // members of this lane that exist
    const int k_begin = SEQ ? 0 : (int)blockIdx.y * FORCROWS_YROWS;
    const int k_end = SEQ ? a.n_rows : (k_begin + FORCROWS_YROWS < a.n_rows ? k_begin + FORCROWS_YROWS : a.n_rows);

    // per member, once: q, the scales and the carried state; member j read at column min(j, live - 1) like the rows: what a
    // missing member holds is never stored
    ForcRowsLane<T> s;
    s.mismatches = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int64_t col = m + (j < live ? j : live - 1);
        const bool rq = active && a.Trows;
        s.q0[j] = rq ? a.q[col] : T(1);
        s.q1[j] = rq ? a.q[a.ld + col] : T(1);
        s.qs[j] = s.q0[j] + s.q1[j];
#pragma unroll
        for (int g = 0; g < MAX_GAS; ++g) s.sg[g][j] = active && a.fs && g < a.n_gas ? a.fs[g * a.ld + col] : T(1);
#pragma unroll
        for (int x = 0; x < MAX_FEXT; ++x) s.sx[x][j] = active && a.fs && x < a.n_fext ? a.fs[(a.n_gas + x) * a.ld + col] : T(0);
        s.H[j] = SEQ && active && a.H_io ? a.H_io[col] : 0.0;
        s.S0[j] = SEQ && active && a.S_io ? a.S_io[col] : T(0);
        s.S1[j] = SEQ && active && a.S_io ? a.S_io[a.ld + col] : T(0);
    }

    for (int kc = k_begin; kc < k_end; kc += FIVEEQ_BLOCK) {
        // ---- the shared records of rows [kc, kc + FIVEEQ_BLOCK): one thread per row ----------------------------------------
        __syncthreads();                                       // the last chunk's records are read to their end
        if (kc + tid < k_end) {
            int t = a.steps[kc + tid];
            t = t < 0 ? 0 : t >= a.n_steps ? a.n_steps - 1 : t;
            s_fext[tid] = a.drive[(int64_t)t * DRIVE_STRIDE + 6];
#pragma unroll
            for (int x = 0; x < MAX_FEXT; ++x) s_x[tid][x] = a.X && x < a.n_fext ? a.X[(int64_t)t * MAX_FEXT + x] : T(0);
        }
        __syncthreads();
        if (!active) continue;
        const int nr = k_end - kc < FIVEEQ_BLOCK ? k_end - kc : FIVEEQ_BLOCK;
        // ---- the row loop: the loads of UN rows in flight before the first is used -----------------------------------------
        const T* pc = a.C + m;
        const T* pt = a.Trows + m;
        int i = 0;
        for (; i + UN <= nr; i += UN) {
            MetricsLoad<T, VEC> c[UN][MAX_GAS], tr[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
#pragma unroll
                for (int g = 0; g < MAX_GAS; ++g)
                    if (g < a.n_gas) c[u][g].load(pc + (int64_t)(kc + i + u) * a.c_row + g * a.c_gas, live);
                if (a.Trows) tr[u].load(pt + (int64_t)(kc + i + u) * a.t_row, live);
            }
#pragma unroll
            for (int u = 0; u < UN; ++u)
                forcrows_row<T, VEC, SEQ>(km, a, kc + i + u, m, live, s_fext[i + u], s_x[i + u], c[u], tr[u], s);
        }
        for (; i < nr; ++i) {
            MetricsLoad<T, VEC> c[MAX_GAS], tr;
#pragma unroll
            for (int g = 0; g < MAX_GAS; ++g)
                if (g < a.n_gas) c[g].load(pc + (int64_t)(kc + i) * a.c_row + g * a.c_gas, live);
            if (a.Trows) tr.load(pt + (int64_t)(kc + i) * a.t_row, live);
            forcrows_row<T, VEC, SEQ>(km, a, kc + i, m, live, s_fext[i], s_x[i], c, tr, s);
        }
    }

    if constexpr (SEQ) {
        if (active) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                if (j < live) {
                    if (a.H_io) a.H_io[m + j] = s.H[j];
                    if (a.S_io) {
                        a.S_io[m + j] = s.S0[j];
                        a.S_io[a.ld + m + j] = s.S1[j];
                    }
                }
            }
            if (s.mismatches) atomicAdd(a.n_mismatch, (unsigned long long)s.mismatches);
        }
    }
}

}  // namespace fiveeq
