// fiveeq_score.hpp — kernel 11: SCORING STORED ROWS against observed records (include/fiveeq.h, "SCORING STORED ROWS").
// Part of fiveeq_device.hpp, which includes it after fiveeq_diag.hpp: include that header, not this one.
//
// One streaming pass over stored rows — element (k, j, m) at rows[k row_stride + j q_stride + m] — folds, per member and
// quantity j, the three misfit accumulators (A, U, V) of the record obs[j] by misfit_update() (fiveeq_member.hpp), the function
// the stepping kernels call: in row order, the value widened exactly, every operation rounded on its own.  The pass is
// therefore the in-loop misfit bit for bit, for every launch shape, split of the rows into calls and shard split.
//   11  score_rows_kernel<T, VEC>   VEC: 16-byte row loads (every lane has all its members), else element loads — the ragged
//                                   tail, unaligned rows
// A lane owns METRICS_LANE<T> consecutive members (16 bytes of a row).  The quantities are walked one after the other, so a lane
// holds the 3 accumulators of its members of ONE quantity in registers while that quantity's rows stream by: each accumulator
// crosses HBM once (24 B in, 24 B out per member and quantity), and one kernel serves every n_q with the registers of one.
// DEAD ROWS ARE NOT STREAMED.  Per quantity the workgroup first compacts, in LDS, the list of the rows whose record is live
// (p_t != 0 || b_t != 0): SCORE_CHUNK rows a time, four per thread, by wave ballots.  The row loop then walks that list — row
// index and step come out of LDS wave-uniform (readfirstlane), the record o, p, b by scalar loads — so that the loads of the
// next SCORE_UNROLL LIVE rows are in flight whatever lies between them: no branch on a dead row, no load of it, no wait for it.
// No atomics, no scratch; LDS holds the live list only.
#pragma once

namespace fiveeq {

constexpr int SCORE_MAX_Q = 4;                                 // FIVEEQ_MAX_SCORE_Q
constexpr int SCORE_UNROLL = 8;                                // live rows whose loads are issued before the first is used (16-byte loads)
constexpr int SCORE_UNROLL_NARROW = 4;                         // the same on the element-load path: 4 M loads, each with its own address
constexpr int SCORE_PASSES = 4;                                // rows per thread and chunk of the live list
constexpr int SCORE_CHUNK = SCORE_PASSES * FIVEEQ_BLOCK;       // rows per chunk: 8 KiB of LDS (row index, step)
constexpr int SCORE_WAVES = FIVEEQ_BLOCK / 64;
template <typename T> constexpr int SCORE_TILE = METRICS_LANE<T> * FIVEEQ_BLOCK;    // members per workgroup

// One live row of the lane: the record of step t of the quantity (ob = its table, wave-uniform: scalar loads), the row's values
// widened exactly, misfit_update() per member.
template <typename T, bool VEC>
__device__ __forceinline__ void score_row(const MetricsLoad<T, VEC>& row, const double* __restrict__ ob, const int t,
                                          double (&A)[METRICS_LANE<T>], double (&U)[METRICS_LANE<T>], double (&V)[METRICS_LANE<T>]) {
    constexpr int M = METRICS_LANE<T>;
    const double* rec = ob + (int64_t)t * 4;
    const double o_t = rec[0], p_t = rec[1], b_t = rec[2];
    double Tw[M];
    row.widen(Tw);
#pragma unroll
    for (int c = 0; c < M; ++c) misfit_update(o_t, p_t, b_t, Tw[c], A[c], U[c], V[c]);
}

// 11.  rows, steps [n_rows], obs [n_q][n_steps][4], misfit [n_q][3][ld_m] as in include/fiveeq.h; n members from column 0 of
// rows and misfit (the host offsets both for the ragged tail's launch).  VEC: rows, row_stride and q_stride allow 16-byte loads
// and n is a multiple of the lane's members (the host has checked).  A step outside [0, n_steps) is never looked up: its row is
// skipped.  Columns [n, ld_m) of misfit are never written, and a quantity without a live row is not written at all.
template <typename T, bool VEC>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void score_rows_kernel(const int n_q, const int n_rows, const int n, const T* __restrict__ rows,
                                                                  const int64_t row_stride, const int64_t q_stride,
                                                                  const int* __restrict__ steps, const double* __restrict__ obs,
                                                                  const int n_steps, double* __restrict__ misfit, const int64_t ld_m) {
    constexpr int M = METRICS_LANE<T>, UN = VEC ? SCORE_UNROLL : SCORE_UNROLL_NARROW;
    __shared__ int s_row[SCORE_CHUNK], s_step[SCORE_CHUNK];
    __shared__ unsigned long long s_mask[SCORE_PASSES][SCORE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + tid) * M;              // the lane's first member
    const bool active = m < n;                                                    // (no early return: the lane takes part in the barriers)
    const int live = !active ? 0 : n - m < M ? (int)(n - m) : M;                  // members of this lane that exist

    for (int j = 0; j < n_q; ++j) {
        const double* ob = obs + (int64_t)j * n_steps * 4;
        double* acc = misfit + (int64_t)j * 3 * ld_m + m;
        // the accumulators handed in; member c read at column min(c, live - 1) like the rows: what a missing member holds is never stored
        double A[M], U[M], V[M];
#pragma unroll
        for (int c = 0; c < M; ++c) {
            const int cc = c < live ? c : live - 1;
            A[c] = active ? acc[cc] : 0.0;
            U[c] = active ? acc[ld_m + cc] : 0.0;
            V[c] = active ? acc[2 * ld_m + cc] : 0.0;
        }
        bool any = false;
        for (int k0 = 0; k0 < n_rows; k0 += SCORE_CHUNK) {
            // ---- the live list of rows [k0, k0 + SCORE_CHUNK), in row order -------------------------------------------------
            bool fl[SCORE_PASSES];
            int tt[SCORE_PASSES];
#pragma unroll
            for (int p = 0; p < SCORE_PASSES; ++p) {
                const int k = k0 + p * FIVEEQ_BLOCK + tid;
                fl[p] = false, tt[p] = 0;
                if (k < n_rows) {
                    tt[p] = steps[k];
                    if ((unsigned)tt[p] < (unsigned)n_steps) {
                        const double* rec = ob + (int64_t)tt[p] * 4;
                        fl[p] = rec[1] != 0.0 || rec[2] != 0.0;
                    }
                }
                const unsigned long long mask = __ballot(fl[p]);
                if (lane == 0) s_mask[p][wave] = mask;
            }
            __syncthreads();
            int before[SCORE_PASSES], run = 0;
#pragma unroll
            for (int p = 0; p < SCORE_PASSES; ++p) {
#pragma unroll
                for (int w = 0; w < SCORE_WAVES; ++w) {
                    const unsigned long long mask = s_mask[p][w];
                    if (w == wave) before[p] = run + __popcll(mask & ((1ull << lane) - 1ull));
                    run += __popcll(mask);
                }
            }
#pragma unroll
            for (int p = 0; p < SCORE_PASSES; ++p) {
                if (fl[p]) {
                    s_row[before[p]] = k0 + p * FIVEEQ_BLOCK + tid;
                    s_step[before[p]] = tt[p];
                }
            }
            __syncthreads();
            const int n_live = __builtin_amdgcn_readfirstlane(run);
            any = any || n_live > 0;
            // ---- the row loop over the live rows: UN loads in flight before the first is used ------------------------------
            if (active) {
                const T* p0 = rows + (int64_t)j * q_stride + m;
                int i = 0;
                for (; i + UN <= n_live; i += UN) {
                    MetricsLoad<T, VEC> row[UN];
#pragma unroll
                    for (int u = 0; u < UN; ++u)
                        row[u].load(p0 + (int64_t)__builtin_amdgcn_readfirstlane(s_row[i + u]) * row_stride, live);
#pragma unroll
                    for (int u = 0; u < UN; ++u)
                        score_row<T, VEC>(row[u], ob, __builtin_amdgcn_readfirstlane(s_step[i + u]), A, U, V);
                }
                for (; i < n_live; ++i) {
                    MetricsLoad<T, VEC> row;
                    row.load(p0 + (int64_t)__builtin_amdgcn_readfirstlane(s_row[i]) * row_stride, live);
                    score_row<T, VEC>(row, ob, __builtin_amdgcn_readfirstlane(s_step[i]), A, U, V);
                }
            }
            __syncthreads();                                   // the list is read to its end before the next chunk overwrites it
        }
        if (any) {
#pragma unroll
            for (int c = 0; c < M; ++c) {
                if (c < live) {
                    acc[c] = A[c];
                    acc[ld_m + c] = U[c];
                    acc[2 * ld_m + c] = V[c];
                }
            }
        }
    }
}

}  // namespace fiveeq
