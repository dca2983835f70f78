// fiveeq_pulse.hpp — kernel 13: PULSE RESPONSE, the per-member response of forcing, warming and concentration to emission pulses,
// from the STORED rows of a scenario engine that ran "baseline" and "baseline + pulse of gas g" side by side (include/fiveeq.h,
// "PULSE RESPONSE").  Part of fiveeq_device.hpp, which includes it after fiveeq_forcrows.hpp: include that
// header, not this one.
//
// Per row k (model step t = steps[k]) and member, with b the base scenario and (s_p, g_p) pulse p, every operation rounded on
// its own:
//     F_b  = forcrows_F(row k of scenario b)          THE function kernel 12 forms F with (fiveeq_forcrows.hpp): the run's own bits
//     F_p  = forcrows_F(row k of scenario s_p)
//     dF_p = (double)F_p - (double)F_b                widened exactly, subtracted in fp64
//     dT_p = (double)T[s_p] - (double)T[b];   dC_p = (double)C[s_p][g_p] - (double)C[b][g_p]
//     I_F_p += dF_p;  I_T_p += dT_p;  I_C_p += dC_p   three fp64 running sums per pulse, rows in ascending order
// and when the row's index, counted from the first row of the experiment (row0 + k), is n_h - 1 for a horizon n_h, the lane
// writes I_F, I_T, I_C, dT, dC of every pulse to out [5][P][H][ld_out].  The sums before the first row and after the last are
// the carried state io [3][P][ld]: rows split over calls give the bits of one call.
//   13  pulse_response_kernel<T, VEC, NP>   VEC: 16-byte row accesses (every lane has all its members), else element accesses —
//                                           the ragged tail, unaligned rows;  NP: the number of pulses — a kernel per count, so
//                                           that a call pays registers and loads for the pulses it asked for
// The shape of forcing_rows_kernel<T, VEC, /*SEQ=*/true>: a lane owns METRICS_LANE<T> consecutive members (16 bytes of a row)
// and walks all rows in ascending order, its sums in registers; rows are read with the non-temporal policy.  The base
// scenario's G + 1 rows are loaded once per row step and shared by the NP pulses: (1 + NP)(G + 1) elements per member and
// row.  ONE row step's loads are in flight per lane — up to 16 loads of 16 bytes, twice what kernel 12's SEQ form keeps — since
// a second row would cost 64 more registers under 36 fp64 accumulators (DESIGN.md 3.19 has the compiler's figures).  What the
// members share per row — F_ext[t] and X[t][0..K) of each of the 1 + NP scenarios — is staged into LDS by one thread per row,
// FIVEEQ_BLOCK rows a time; the model's constants come from the kernel arguments.  No floating-point atomics, no scratch; no
// output bit depends on the launch shape, on a stride or on how rows or members are split over calls.  NaN is not skipped: it
// reaches the sums of its member from its row on, and nobody else's.
#pragma once

namespace fiveeq {

constexpr int PULSE_MAX = 3;                                   // FIVEEQ_MAX_PULSES
constexpr int PULSE_MAX_HORIZONS = 8;                          // FIVEEQ_MAX_HORIZONS
constexpr int PULSE_NO_HORIZON = 0x7fffffff;

// the arguments of one launch besides the model: n members from column 0 of every row (the host offsets the pointers for the
// ragged tail's launch)
template <typename T>
struct PulseArgs {
    int n_gas, n_rows, n, n_steps, n_fext, n_hor, row0;
    int scen[1 + PULSE_MAX];                                   // the base scenario, then the pulses' scenarios
    int gas[PULSE_MAX];                                        // the pulsed gas of each pulse
    int hor[PULSE_MAX_HORIZONS];                               // strictly increasing row counts n_h >= 1
    const T* C;                                                // element (s, k, g, m) at C[s c_scen + k c_row + g c_gas + m]
    int64_t c_scen, c_row, c_gas;
    const T* Trows;                                            // element (s, k, m) at Trows[s t_scen + k t_row + m]
    int64_t t_scen, t_row;
    const int* steps;                                          // [n_rows]
    const T* drive;                                            // [S][n_steps][DRIVE_STRIDE], F_ext at [6]
    const T* fs;                                               // [G + K][ld], gas rows first; NULL: the plain sum F += F_g
    const T* X;                                                // [S][n_steps][MAX_FEXT]
    int64_t ld;
    double* out;                                               // [5][NP][n_hor][ld_out]: I_F, I_T, I_C, dT, dC
    int64_t ld_out;
    double* io;                                                // [3][NP][ld]: I_F, I_T, I_C before the first row / after the last
};

// 13.  VEC: every row pointer and stride allows 16-byte accesses, out too, and n is a multiple of the lane's members (the host
// has checked, and hands the ragged tail to a second launch without VEC).  A step outside [0, n_steps) is clamped into it: the
// kernel never reads outside the tables (the caller owes valid steps).  Columns [n, ..) of out and io are never written.
template <typename T, bool VEC, int NP>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void pulse_response_kernel(const KModel<T> km, const PulseArgs<T> a) {
    constexpr int M = METRICS_LANE<T>, NS = 1 + NP;
    __shared__ T s_fext[FIVEEQ_BLOCK][NS];
    __shared__ T s_x[FIVEEQ_BLOCK][NS][MAX_FEXT];
    const int tid = threadIdx.x;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + tid) * M;              // the lane's first member
    const bool active = m < a.n;                                                  // (no early return: the lane takes part in the barriers)
    const int live = !active ? 0 : a.n - m < M ? (int)(a.n - m) : M;              // members of this lane that exist

    // per member, once: the scales and the carried sums; member j read at column min(j, live - 1) like the rows: what a
    // missing member holds is never stored
    T sg[MAX_GAS][M], sx[MAX_FEXT][M];
    double I_F[NP][M], I_T[NP][M], I_C[NP][M];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int64_t col = m + (j < live ? j : live - 1);
#pragma unroll
        for (int g = 0; g < MAX_GAS; ++g) sg[g][j] = active && a.fs && g < a.n_gas ? a.fs[g * a.ld + col] : T(1);
#pragma unroll
        for (int x = 0; x < MAX_FEXT; ++x) sx[x][j] = active && a.fs && x < a.n_fext ? a.fs[(a.n_gas + x) * a.ld + col] : T(0);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            I_F[p][j] = active ? a.io[(0 * NP + p) * a.ld + col] : 0.0;
            I_T[p][j] = active ? a.io[(1 * NP + p) * a.ld + col] : 0.0;
            I_C[p][j] = active ? a.io[(2 * NP + p) * a.ld + col] : 0.0;
        }
    }
    // the next horizon the rows can reach (wave-uniform): the first whose last row n_h - 1 is not behind row0
    int h = 0;
    while (h < a.n_hor && a.hor[h] - 1 < a.row0) ++h;
    int r_next = h < a.n_hor ? a.hor[h] - 1 : PULSE_NO_HORIZON;

    for (int kc = 0; kc < a.n_rows; kc += FIVEEQ_BLOCK) {
        // ---- the shared records of rows [kc, kc + FIVEEQ_BLOCK), every scenario of the call: one thread per row ------------
        __syncthreads();                                       // the last chunk's records are read to their end
        if (kc + tid < a.n_rows) {
            int t = a.steps[kc + tid];
            t = t < 0 ? 0 : t >= a.n_steps ? a.n_steps - 1 : t;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t rec = (int64_t)a.scen[s] * a.n_steps + t;
                s_fext[tid][s] = a.drive[rec * DRIVE_STRIDE + 6];
#pragma unroll
                for (int x = 0; x < MAX_FEXT; ++x) s_x[tid][s][x] = a.X && x < a.n_fext ? a.X[rec * MAX_FEXT + x] : T(0);
            }
        }
        __syncthreads();
        if (!active) continue;
        const int nr = a.n_rows - kc < FIVEEQ_BLOCK ? a.n_rows - kc : FIVEEQ_BLOCK;
        // ---- the row loop: the (1 + NP)(G + 1) loads of one row step in flight before the first is used -------------------
        for (int i = 0; i < nr; ++i) {
            const int k = kc + i;
            MetricsLoad<T, VEC> c[NS][MAX_GAS], tr[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const T* pc = a.C + a.scen[s] * a.c_scen + (int64_t)k * a.c_row + m;
#pragma unroll
                for (int g = 0; g < MAX_GAS; ++g)
                    if (g < a.n_gas) c[s][g].load(pc + g * a.c_gas, live);
                tr[s].load(a.Trows + a.scen[s] * a.t_scen + (int64_t)k * a.t_row + m, live);
            }
            T Fb[M];
            forcrows_F<T, VEC>(km, a.n_gas, a.n_fext, a.fs != nullptr, s_fext[i][0], s_x[i][0], c[0], sg, sx, Fb, [](int, const T (&)[M]) {});
            const bool hit = a.row0 + k == r_next;             // a horizon ends with this row (wave-uniform)
            const int64_t hs = a.n_hor * a.ld_out;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                T Fp[M];
                forcrows_F<T, VEC>(km, a.n_gas, a.n_fext, a.fs != nullptr, s_fext[i][1 + p], s_x[i][1 + p], c[1 + p], sg, sx, Fp,
                                   [](int, const T (&)[M]) {});
                double dT[M], dC[M];
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    const double dF = (double)Fp[j] - (double)Fb[j];
                    dT[j] = (double)tr[1 + p].v[j] - (double)tr[0].v[j];
                    dC[j] = 0.0;
#pragma unroll
                    for (int g = 0; g < MAX_GAS; ++g)          // the pulsed gas: a wave-uniform pick among register rows
                        if (g == a.gas[p]) dC[j] = (double)c[1 + p][g].v[j] - (double)c[0][g].v[j];
                    I_F[p][j] = I_F[p][j] + dF;
                    I_T[p][j] = I_T[p][j] + dT[j];
                    I_C[p][j] = I_C[p][j] + dC[j];
                }
                if (hit) {
                    double* o = a.out + (p * a.n_hor + h) * a.ld_out + m;
                    forcrows_store<double, M, VEC>(o, I_F[p], live);
                    forcrows_store<double, M, VEC>(o + 1 * NP * hs, I_T[p], live);
                    forcrows_store<double, M, VEC>(o + 2 * NP * hs, I_C[p], live);
                    forcrows_store<double, M, VEC>(o + 3 * NP * hs, dT, live);
                    forcrows_store<double, M, VEC>(o + 4 * NP * hs, dC, live);
                }
            }
            if (hit) {
                ++h;
                r_next = h < a.n_hor ? a.hor[h] - 1 : PULSE_NO_HORIZON;
            }
        }
    }

    if (active) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                if (j < live) {
                    a.io[(0 * NP + p) * a.ld + m + j] = I_F[p][j];
                    a.io[(1 * NP + p) * a.ld + m + j] = I_T[p][j];
                    a.io[(2 * NP + p) * a.ld + m + j] = I_C[p][j];
                }
            }
        }
    }
}

}  // namespace fiveeq
