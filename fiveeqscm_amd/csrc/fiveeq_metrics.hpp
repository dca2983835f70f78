// fiveeq_metrics.hpp — kernel 9: per-member TRAJECTORY METRICS of stored rows (include/fiveeq.h, "TRAJECTORY METRICS").
// Part of fiveeq_device.hpp, which includes it after fiveeq_resample.hpp: include that header, not this one.
//
// One streaming pass over the stored T rows [n_scen][n_rows][ld] folds, per member and scenario: the peak and the step that
// first attains it, per level the first step at or above it and the number of rows at or above it, per step window the sum of
// the rows inside it, and the number of NaN rows.  Every result is an integer or an fp64 sum taken in row order, one rounded
// add per row: the same bits for every launch shape, every split of the rows into calls and every shard split.
//   9  traj_metrics_kernel<T, FIRST, NL, VEC>   FIRST: the call initialises the state; else it continues the state it is handed;
//                                               NL: the number of levels — a kernel per count, so that a call pays registers and
//                                               comparisons for the levels it asked for; VEC: 16-byte row loads (every lane has
//                                               all its members), else element loads — the ragged tail, unaligned rows
// A lane owns METRICS_LANE<T> consecutive members (16 bytes of a row) for the whole row loop, the state in registers; grid.y
// is the scenario.  No workgroup synchronises with anything: no LDS, no barrier, no atomics.
#pragma once

namespace fiveeq {

constexpr int METRICS_MAX_LEVELS = 8;                          // FIVEEQ_MAX_LEVELS
constexpr int METRICS_MAX_WINDOWS = 4;                         // FIVEEQ_MAX_WINDOWS
constexpr int METRICS_UNROLL = 8;                              // rows whose loads are issued before the first is used (16-byte loads)
constexpr int METRICS_UNROLL_NARROW = 2;                       // the same on the element-load path: 2 M loads, each with its own address
template <typename T> constexpr int METRICS_LANE = 16 / (int)sizeof(T);              // members per lane: 2 (fp64), 4 (fp32)
template <typename T> constexpr int METRICS_TILE = METRICS_LANE<T> * FIVEEQ_BLOCK;  // members per workgroup

typedef double met_f64x2 __attribute__((ext_vector_type(2)));
typedef float met_f32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct MetricsVec;
template <> struct MetricsVec<double> { using V = met_f64x2; };
template <> struct MetricsVec<float> { using V = met_f32x4; };

// levels and windows, by value in the kernel arguments: wave-uniform, read from scalar registers
struct MetricsSpec {
    double level[METRICS_MAX_LEVELS];
    int win[METRICS_MAX_WINDOWS][2];                           // [a, b): the steps a <= t < b
    int n_levels, n_windows;
};

// the state of a lane's M members under NL levels.  Every index below is a constant after unrolling (the loop over the windows
// runs to its MAXIMUM under a wave-uniform guard), so the arrays are registers, never scratch.
template <int M, int NL>
struct MetricsState {
    double peak[M], wsum[METRICS_MAX_WINDOWS][M];
    int t_peak[M], n_nan[M], first[NL > 0 ? NL : 1][M], n_above[NL > 0 ? NL : 1][M];
};

// THE ROW UPDATE: the definition of include/fiveeq.h, operation for operation.  t is the row's model step (wave-uniform); Tw
// the row's values widened exactly.  A NaN fails every comparison, so it touches only n_nan and the window sums.
template <int M, int NL>
__device__ __forceinline__ void metrics_row(const MetricsSpec& sp, const int t, const double (&Tw)[M], MetricsState<M, NL>& s) {
#pragma unroll
    for (int j = 0; j < M; ++j) {
        s.n_nan[j] += Tw[j] != Tw[j] ? 1 : 0;
        const bool up = Tw[j] > s.peak[j];                     // strict: the earliest step attaining the peak is kept
        s.peak[j] = up ? Tw[j] : s.peak[j];
        s.t_peak[j] = up ? t : s.t_peak[j];
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const bool at = Tw[j] >= sp.level[l];
            s.n_above[l][j] += at ? 1 : 0;
            s.first[l][j] = at && s.first[l][j] < 0 ? t : s.first[l][j];
        }
    }
#pragma unroll
    for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) {
        if (w < sp.n_windows && sp.win[w][0] <= t && t < sp.win[w][1]) {
#pragma unroll
            for (int j = 0; j < M; ++j) s.wsum[w][j] = s.wsum[w][j] + Tw[j];        // one rounded add; NaN propagates
        }
    }
}

// One row of the lane: VEC, one 16-byte non-temporal load (the caller has checked the alignment and that all M members
// exist); else M element loads, member j read at column min(j, live - 1) — inside the row whatever j, and what a missing
// member computes is never stored.
template <typename T, bool VEC>
struct MetricsLoad {
    using V = typename MetricsVec<T>::V;
    static constexpr int M = METRICS_LANE<T>;
    V v;
    __device__ __forceinline__ void load(const T* p, const int live) {
        if constexpr (VEC) v = load_row<V, true>(reinterpret_cast<const V*>(p));
        else {
#pragma unroll
            for (int j = 0; j < M; ++j) v[j] = load_row<T, true>(p + (j < live ? j : live - 1));
        }
    }
    __device__ __forceinline__ void widen(double (&Tw)[M]) const {
#pragma unroll
        for (int j = 0; j < M; ++j) Tw[j] = (double)v[j];
    }
};

// the row loop of one lane: rows k = 0 .. n_rows - 1 at p + k ld, the loads of U rows in flight before the first is used
// (the rows are ld elements apart: one load in flight per lane is a latency-bound pass)
template <typename T, bool VEC, int NL>
__device__ __forceinline__ void metrics_rows(const T* __restrict__ p, const int64_t ld, const int n_rows, const int* __restrict__ steps,
                                             const MetricsSpec& sp, const int live, MetricsState<METRICS_LANE<T>, NL>& s) {
    constexpr int M = METRICS_LANE<T>, U = VEC ? METRICS_UNROLL : METRICS_UNROLL_NARROW;
    double Tw[M];
    int k = 0;
    for (; k + U <= n_rows; k += U) {
        MetricsLoad<T, VEC> row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u].load(p + (int64_t)(k + u) * ld, live);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u].widen(Tw);
            metrics_row<M, NL>(sp, steps[k + u], Tw, s);
        }
    }
    for (; k < n_rows; ++k) {
        MetricsLoad<T, VEC> row;
        row.load(p + (int64_t)k * ld, live);
        row.widen(Tw);
        metrics_row<M, NL>(sp, steps[k], Tw, s);
    }
}

// 9.  rows [n_scen][n_rows][ld] (scenario blocks scen_stride elements apart), steps [n_rows]; the state blocks
// fmet [n_scen][1 + W][ld] fp64 = (peak, wsum[w]) and imet [n_scen][2 + 2 L][ld] int32 = (t_peak, n_nan, first[l], n_above[l]).
// VEC: rows, scen_stride and ld allow 16-byte loads and n is a multiple of the lane's members (the host has checked, and hands
// the ragged tail of fewer members than a lane's to a second launch without VEC).  Columns [n, ld) of the state blocks are
// never written, and FIRST never reads the state blocks.
template <typename T, bool FIRST, int NL, bool VEC>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void traj_metrics_kernel(const int n_rows, const int n, const int64_t ld, const T* __restrict__ rows,
                                                                    const int64_t scen_stride, const int* __restrict__ steps,
                                                                    const MetricsSpec sp, double* __restrict__ fmet,
                                                                    int* __restrict__ imet) {
    constexpr int M = METRICS_LANE<T>;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x) * M;      // the lane's first member
    if (m >= n) return;
    const int live = n - m < M ? (int)(n - m) : M;                                // members of this lane that exist
    constexpr int L = NL;
    const int W = sp.n_windows;
    double* fm = fmet + (int64_t)blockIdx.y * (1 + W) * ld + m;
    int* im = imet + (int64_t)blockIdx.y * (2 + 2 * L) * ld + m;

    // FIRST: the initial state.  Else the state handed in, member j read at column min(j, live - 1) like the rows: no branch
    // around a load, and what a missing member holds is never stored.
    MetricsState<M, NL> s;
#pragma unroll
    for (int j = 0; j < M; ++j) {
        const int c = j < live ? j : live - 1;
        s.peak[j] = FIRST ? -__builtin_huge_val() : fm[c];
        s.t_peak[j] = FIRST ? -1 : im[c];
        s.n_nan[j] = FIRST ? 0 : im[ld + c];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            s.first[l][j] = FIRST ? -1 : im[(2 + l) * ld + c];
            s.n_above[l][j] = FIRST ? 0 : im[(2 + L + l) * ld + c];
        }
#pragma unroll
        for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) s.wsum[w][j] = !FIRST && w < W ? fm[(1 + w) * ld + c] : 0.0;
    }

    const T* p = rows + (int64_t)blockIdx.y * scen_stride + m;
    metrics_rows<T, VEC, NL>(p, ld, n_rows, steps, sp, live, s);

    // the state's addresses are formed again here (the empty asm hides that fm and im are the pointers the loads above used):
    // kept across the row loop they would cost two registers per state word and member, and with them the occupancy
    asm volatile("" : "+v"(fm), "+v"(im));
#pragma unroll
    for (int j = 0; j < M; ++j) {
        if (j < live) {
            fm[j] = s.peak[j];
            im[j] = s.t_peak[j];
            im[ld + j] = s.n_nan[j];
        }
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (j < live) {
                im[(2 + l) * ld + j] = s.first[l][j];
                im[(2 + L + l) * ld + j] = s.n_above[l][j];
            }
        }
    }
#pragma unroll
    for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) {
        if (w < W) {
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (j < live) fm[(1 + w) * ld + j] = s.wsum[w][j];
        }
    }
}

}  // namespace fiveeq
