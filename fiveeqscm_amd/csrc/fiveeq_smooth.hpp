// fiveeq_smooth.hpp — kernels 15a / 15b: per-member RUNNING MEANS and LINEAR-TREND SUMS of stored rows (include/fiveeq.h, "RUNNING
// MEANS AND TRENDS").  Part of fiveeq_device.hpp, which includes it after fiveeq_metrics.hpp: include that
// header, not this one.
//
// Both are streaming passes over rows [n_scen][n_rows][ld] in the layout of the metrics pass (fiveeq_metrics.hpp): a lane owns
// METRICS_LANE<T> consecutive members (16 bytes of a row) for the whole row loop, grid.y is the scenario, VEC is the
// instantiation with 16-byte non-temporal row loads (every lane has all its members), the other one takes element loads — the
// ragged tail, unaligned rows.  No workgroup synchronises with anything: no barrier, no atomics.
//   15a running_mean_kernel<T, VEC>   out[k] = (x[k] + x[k+1] + .. + x[k+window-1]) / window, the sum taken in ascending row order
//                                     from the window's first row for EVERY output — no sliding update, so an output depends on
//                                     its own rows only.  The last `window` rows live in a lane-private ring in LDS.
//   15b window_trend_kernel<T, FIRST, VEC>   per step window (sx, stx) = (sum of T, sum of (t - a) T) over the rows inside it;
//                                     registers only, the state carried in and out like the metrics pass's.
#pragma once

namespace fiveeq {

constexpr int SMOOTH_MAX_WINDOW = 32;                          // FIVEEQ_MAX_SMOOTH_WINDOW
// threads per workgroup of running_mean_kernel: ONE wave.  The ring costs 16 bytes x window per lane whatever the block, no
// lane ever looks at another's slots, and a wave-sized workgroup packs the CU's LDS in steps of window KiB instead of 4 window
// KiB: 5 waves per CU instead of 4 at window 32, 22 instead of 20 at window 7, and never more than 32 KiB of dynamic LDS per
// workgroup, so no launch has to raise the kernel's dynamic-LDS limit.
constexpr int SMOOTH_BLOCK = 64;
template <typename T> constexpr int SMOOTH_TILE = METRICS_LANE<T> * SMOOTH_BLOCK;               // members per workgroup of 15a
template <typename T> constexpr int TREND_TILE = METRICS_LANE<T> * FIVEEQ_BLOCK;                // members per workgroup of 15b

// One row of the lane, as MetricsLoad: VEC, one 16-byte non-temporal load; else M element loads, member j read at column
// min(j, live - 1) — inside the row whatever j, and what a missing member computes is never stored.  A struct of this
// header's own: an instantiation shared with the kernels that existed (MetricsLoad<T, false>, load_row<T, true>) changes the
// machine code the compiler emits for THEM (30 kernels of the metrics, score, forcing-rows and pulse passes, profiles/r27).
template <typename T, bool VEC>
struct SmoothLoad {
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
    __device__ __forceinline__ void widen(double (&Tw)[M]) const {
#pragma unroll
        for (int j = 0; j < M; ++j) Tw[j] = (double)v[j];
    }
};

// the lane-private ring of running_mean_kernel: slot s of lane l at [s][l], 16 bytes each (a wave's access is contiguous);
// dynamic LDS of SMOOTH_BLOCK * 16 * window bytes
extern __shared__ __attribute__((aligned(16))) unsigned char smooth_lds[];

// The ring and the output cursor of one lane.  push() takes the next row of the sequence; once `window` rows are held it
// forms the output of the window that ends at this row — the definition of include/fiveeq.h, operation for operation — and
// stores it at the cursor.
template <typename T, bool VEC>
struct SmoothLane {
    using V = typename MetricsVec<T>::V;
    static constexpr int M = METRICS_LANE<T>;
    V* ring;                                                   // the lane's slot 0; slot s at ring[s * SMOOTH_BLOCK]
    double* out;                                               // the lane's members of the next output row
    int64_t ld;
    int window, slot, held, live;                              // slot: where the next row goes = the OLDEST row once window are held
    double wd;                                                 // (double)window

    __device__ __forceinline__ void add(double (&s)[M], const V v) const {
#pragma unroll
        for (int j = 0; j < M; ++j) s[j] = s[j] + (double)v[j];                     // exact widening, one rounded add
    }
    __device__ __forceinline__ void push(const V v) {
        ring[slot * SMOOTH_BLOCK] = v;
        slot = slot + 1 == window ? 0 : slot + 1;
        if (held + 1 < window) {
            ++held;
            return;
        }
        // rows k .. k + window - 1 sit in slots slot .. window - 1, then 0 .. slot - 1
        double s[M];
        const V first = ring[slot * SMOOTH_BLOCK];
#pragma unroll
        for (int j = 0; j < M; ++j) s[j] = (double)first[j];
#pragma unroll 4
        for (int q = slot + 1; q < window; ++q) add(s, ring[q * SMOOTH_BLOCK]);
#pragma unroll 4
        for (int q = 0; q < slot; ++q) add(s, ring[q * SMOOTH_BLOCK]);
#pragma unroll
        for (int j = 0; j < M; ++j) s[j] = s[j] / wd;                                // one IEEE division: no reciprocal multiply
        if constexpr (VEC) {
            if constexpr (M == 2) {
                *reinterpret_cast<met_f64x2*>(out) = met_f64x2{s[0], s[1]};
            } else {
                reinterpret_cast<met_f64x2*>(out)[0] = met_f64x2{s[0], s[1]};
                reinterpret_cast<met_f64x2*>(out)[1] = met_f64x2{s[2], s[3]};
            }
        } else {
#pragma unroll
            for (int j = 0; j < M; ++j)
                if (j < live) out[j] = s[j];
        }
        out += ld;
    }
    // n rows at p + k ld, the loads of U rows in flight before the first is pushed (as metrics_rows)
    __device__ __forceinline__ void rows(const T* __restrict__ p, const int n) {
        constexpr int U = VEC ? METRICS_UNROLL : METRICS_UNROLL_NARROW;
        int k = 0;
        for (; k + U <= n; k += U) {
            SmoothLoad<T, VEC> row[U];
#pragma unroll
            for (int u = 0; u < U; ++u) row[u].load(p + (int64_t)(k + u) * ld, live);
#pragma unroll
            for (int u = 0; u < U; ++u) push(row[u].v);
        }
        for (; k < n; ++k) {
            SmoothLoad<T, VEC> row;
            row.load(p + (int64_t)k * ld, live);
            push(row.v);
        }
    }
};

// 15a.  The sequence x = tail [n_scen][n_tail][ld] (the rows before row 0, 0 <= n_tail <= window - 1; scenario blocks
// tail_scen_stride apart) followed by rows [n_scen][n_rows][ld] (scen_stride apart); out [n_scen][n_out][ld] fp64
// (out_scen_stride apart), n_out = n_tail + n_rows - window + 1 >= 1 (the host launches nothing otherwise).  VEC: rows, tail,
// out and their strides allow 16-byte accesses and n is a multiple of the lane's members (the host has checked, and hands the
// ragged tail of members to a launch without VEC).  Columns [n, ld) of out are never written.
template <typename T, bool VEC>
__global__ __launch_bounds__(SMOOTH_BLOCK) void running_mean_kernel(const int n_rows, const int n, const int64_t ld, const T* __restrict__ rows,
                                                                    const int64_t scen_stride, const int window, const int n_tail,
                                                                    const T* __restrict__ tail, const int64_t tail_scen_stride,
                                                                    double* __restrict__ out, const int64_t out_scen_stride) {
    constexpr int M = METRICS_LANE<T>;
    const int64_t m = ((int64_t)blockIdx.x * SMOOTH_BLOCK + threadIdx.x) * M;     // the lane's first member
    if (m >= n) return;
    SmoothLane<T, VEC> lane;
    lane.ring = reinterpret_cast<typename MetricsVec<T>::V*>(smooth_lds) + threadIdx.x;
    lane.out = out + (int64_t)blockIdx.y * out_scen_stride + m;
    lane.ld = ld;
    lane.window = window, lane.slot = 0, lane.held = 0;
    lane.live = n - m < M ? (int)(n - m) : M;                                     // members of this lane that exist
    lane.wd = (double)window;
    if (n_tail > 0) lane.rows(tail + (int64_t)blockIdx.y * tail_scen_stride + m, n_tail);
    lane.rows(rows + (int64_t)blockIdx.y * scen_stride + m, n_rows);
}

// windows of 15b by value in the kernel arguments: wave-uniform, read from scalar registers
struct TrendSpec {
    int win[METRICS_MAX_WINDOWS][2];                           // [a, b): the steps a <= t < b
    int n_windows;
};

// THE ROW UPDATE of 15b: the definition of include/fiveeq.h, operation for operation (contraction is off: the product is
// rounded, then the add).  The loop over the windows runs to its MAXIMUM under a wave-uniform guard, so the sums are registers.
template <int M>
__device__ __forceinline__ void trend_row(const TrendSpec& sp, const int t, const double (&Tw)[M], double (&sx)[METRICS_MAX_WINDOWS][M],
                                          double (&stx)[METRICS_MAX_WINDOWS][M]) {
#pragma unroll
    for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) {
        if (w < sp.n_windows && sp.win[w][0] <= t && t < sp.win[w][1]) {
            const double u = (double)(t - sp.win[w][0]);
#pragma unroll
            for (int j = 0; j < M; ++j) {
                sx[w][j] = sx[w][j] + Tw[j];
                const double p = u * Tw[j];
                stx[w][j] = stx[w][j] + p;
            }
        }
    }
}

// 15b.  rows [n_scen][n_rows][ld] (scen_stride apart), steps [n_rows]; the state tsum [n_scen][2 W][ld] fp64 = (sx[w], stx[w])
// per window.  FIRST: the call starts from 0 and never reads tsum; else it continues the state it is handed.  Columns [n, ld)
// of tsum are never written.
template <typename T, bool FIRST, bool VEC>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void window_trend_kernel(const int n_rows, const int n, const int64_t ld, const T* __restrict__ rows,
                                                                    const int64_t scen_stride, const int* __restrict__ steps,
                                                                    const TrendSpec sp, double* __restrict__ tsum) {
    constexpr int M = METRICS_LANE<T>, U = VEC ? METRICS_UNROLL : METRICS_UNROLL_NARROW;
    const int64_t m = ((int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x) * M;
    if (m >= n) return;
    const int live = n - m < M ? (int)(n - m) : M;
    const int W = sp.n_windows;
    double* ts = tsum + (int64_t)blockIdx.y * 2 * W * ld + m;
    double sx[METRICS_MAX_WINDOWS][M], stx[METRICS_MAX_WINDOWS][M];
#pragma unroll
    for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) {
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int c = j < live ? j : live - 1;             // a missing member reads inside the row; it is never stored
            sx[w][j] = !FIRST && w < W ? ts[(2 * w) * ld + c] : 0.0;
            stx[w][j] = !FIRST && w < W ? ts[(2 * w + 1) * ld + c] : 0.0;
        }
    }
    const T* p = rows + (int64_t)blockIdx.y * scen_stride + m;
    double Tw[M];
    int k = 0;
    for (; k + U <= n_rows; k += U) {
        SmoothLoad<T, VEC> row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) row[u].load(p + (int64_t)(k + u) * ld, live);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            row[u].widen(Tw);
            trend_row<M>(sp, steps[k + u], Tw, sx, stx);
        }
    }
    for (; k < n_rows; ++k) {
        SmoothLoad<T, VEC> row;
        row.load(p + (int64_t)k * ld, live);
        row.widen(Tw);
        trend_row<M>(sp, steps[k], Tw, sx, stx);
    }
#pragma unroll
    for (int w = 0; w < METRICS_MAX_WINDOWS; ++w) {
        if (w < W) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                if (j < live) {
                    ts[(2 * w) * ld + j] = sx[w][j];
                    ts[(2 * w + 1) * ld + j] = stx[w][j];
                }
            }
        }
    }
}

}  // namespace fiveeq
