// fiveeq_wsummary.hpp — kernels 7a-7d: the WEIGHTED end-of-run summary (include/fiveeq.h, "WEIGHTED SUMMARY").
// Part of fiveeq_device.hpp, which includes it after fiveeq_summary.hpp: include that header, not this one.
//
// The passes of kernels 6a-6d over (value, weight) pairs.  Weights are INTEGERS (uint64, at most 2^32 each, fewer than 2^31
// members over all ranks), shared by the rows: every sum of weights is an exact 64-bit integer sum, so LDS / global atomics
// and all-reduces in any order give the same bits, and the percentile — the smallest x whose cumulative weight reaches an
// integer rank — is exact and the same for every shard split.  A member of weight 0 does not exist for these passes,
// whatever its value (NaN and inf included).
//   7a  wrow_moments_kernel + fold   sum w x, sum w x^2, sum w^2 (fp64, fixed order), min / max / count over w > 0, sum w
//   7b  whist_rows_kernel            bins of WEIGHT between the extrema 7a wrote (per-row ranges in device memory)
//   7c  wselect_bins_kernel          the (value, weight) pairs of the host-marked bins, compacted
//   7d  wselect_pick_kernel          per (row, percentile): radix selection on sums of weight
#pragma once

namespace fiveeq {

constexpr unsigned long long WEIGHT_ONE = 1ull << 32;          // the largest weight a member may carry
constexpr int WMOM_WORDS = 8;                                  // words of 8 bytes per row record of 7a (layout: include/fiveeq.h)
constexpr unsigned long long WFLAG_NAN = 1ull, WFLAG_RANGE = 2ull;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh);
    return v;
}

// Every member of [m0, m1) of a row with its weight, one call f(value, weight, have) per lane and member.  Whole waves
// iterate together — lanes past the end of the chunk call f with have = false and weight 0 — so f may be a wave-level
// operation.  `wide`: 16-byte loads of values and of weights (the row, its stride and the weights are 16-byte aligned);
// m0 is a multiple of 4 * FIVEEQ_BLOCK (the host's chunking), which keeps every lane's address aligned.
template <typename T, typename F>
__device__ __forceinline__ void wfor_members(const T* __restrict__ x, const unsigned long long* __restrict__ w, const int64_t m0,
                                             const int64_t m1, const bool wide, F&& f) {
    using WV = typename Wide<T>::V;
    constexpr int WN = Wide<T>::N;
    constexpr int64_t STEP = (int64_t)WN * FIVEEQ_BLOCK;
    int64_t wm = m0 + (int64_t)(threadIdx.x & ~63) * WN;        // the wave's first member: the loop bounds are wave-uniform
    int64_t m = m0 + (int64_t)threadIdx.x * WN;
    auto weights_of = [&](const int64_t at, unsigned long long (&ws)[WN]) {
#pragma unroll
        for (int j = 0; j < WN; j += 2) {
            const ulonglong2 p = *reinterpret_cast<const ulonglong2*>(w + at + j);
            ws[j] = p.x, ws[j + 1] = p.y;
        }
    };
    if (wide) {
        for (; wm + STEP + 64 * WN <= m1; wm += 2 * STEP, m += 2 * STEP) {      // two independent groups of loads in flight
            const WV a = *reinterpret_cast<const WV*>(x + m);
            const WV b = *reinterpret_cast<const WV*>(x + m + STEP);
            unsigned long long wa[WN], wb[WN];
            weights_of(m, wa);
            weights_of(m + STEP, wb);
#pragma unroll
            for (int j = 0; j < WN; ++j) f(wide_get(a, j), wa[j], true);
#pragma unroll
            for (int j = 0; j < WN; ++j) f(wide_get(b, j), wb[j], true);
        }
    }
    for (; wm < m1; wm += STEP, m += STEP) {
        if (wide && wm + 64 * WN <= m1) {
            const WV a = *reinterpret_cast<const WV*>(x + m);
            unsigned long long wa[WN];
            weights_of(m, wa);
#pragma unroll
            for (int j = 0; j < WN; ++j) f(wide_get(a, j), wa[j], true);
        } else {                                                  // unaligned rows, and the ragged tail of the last chunk
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const bool have = m + j < m1;
                f(have ? x[m + j] : T(0), have ? w[m + j] : 0ull, have);
            }
        }
    }
}
template <typename T>
__device__ __forceinline__ bool wrows_wide(const T* x, const int64_t ld, const unsigned long long* w) {
    return ((((uintptr_t)x) | ((uintptr_t)(ld * sizeof(T))) | ((uintptr_t)w)) & 15) == 0;
}

// 7a.  partial[row][chunk][8] / moments[row][8], words of 8 bytes:
//   0 sum w x   1 sum w x^2   2 sum w^2   3 min   4 max                       fp64; over the members with w > 0
//   5 count of w > 0   6 flags (WFLAG_NAN: a NaN value with w > 0; WFLAG_RANGE: a weight above 2^32)   7 sum w       uint64
// Sums in a fixed order (lane-strided, xor-shuffle tree, wave order, chunk order in the fold): the same bits on every run.
// min / max ignore NaNs, the fp64 sums propagate them.
struct WMoments {
    double s1, s2, sw2, mn, mx;
    unsigned long long cnt, flags, sw;
};
__device__ __forceinline__ WMoments wmoments_zero() {
    const double inf = __builtin_inf();
    return WMoments{0.0, 0.0, 0.0, inf, -inf, 0ull, 0ull, 0ull};
}
__device__ __forceinline__ void wmoments_wave(WMoments& a) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        a.s1 += __shfl_xor(a.s1, sh);
        a.s2 += __shfl_xor(a.s2, sh);
        a.sw2 += __shfl_xor(a.sw2, sh);
        a.mn = fmin(a.mn, __shfl_xor(a.mn, sh));
        a.mx = fmax(a.mx, __shfl_xor(a.mx, sh));
        a.cnt += __shfl_xor(a.cnt, sh);
        a.flags |= __shfl_xor(a.flags, sh);
        a.sw += __shfl_xor(a.sw, sh);
    }
}
__device__ __forceinline__ void wmoments_store(double* o, const WMoments& a) {
    o[0] = a.s1, o[1] = a.s2, o[2] = a.sw2, o[3] = a.mn, o[4] = a.mx;
    unsigned long long* u = reinterpret_cast<unsigned long long*>(o);
    u[5] = a.cnt, u[6] = a.flags, u[7] = a.sw;
}
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void wrow_moments_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                    const T* __restrict__ rows,
                                                                    const unsigned long long* __restrict__ weights,
                                                                    double* __restrict__ partial) {
    __shared__ double red[FIVEEQ_BLOCK / 64][WMOM_WORDS];
    const int64_t row = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * chunk;          // chunk is a multiple of 4 * FIVEEQ_BLOCK (host)
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    WMoments a = wmoments_zero();
    wfor_members(x, weights, m0, m1, wrows_wide(x, ld, weights), [&](const T xv, const unsigned long long w, const bool) {
        if (w != 0ull) {
            const double v = (double)xv, wd = (double)w;    // exact: w <= 2^32
            const double wx = wd * v;
            a.s1 += wx;
            a.s2 = __builtin_fma(wx, v, a.s2);
            a.sw2 = __builtin_fma(wd, wd, a.sw2);
            a.mn = fmin(a.mn, v);
            a.mx = fmax(a.mx, v);
            a.cnt += 1ull;
            a.flags |= (v != v ? WFLAG_NAN : 0ull) | (w > WEIGHT_ONE ? WFLAG_RANGE : 0ull);
            a.sw += w;
        }
    });
    wmoments_wave(a);
    if ((threadIdx.x & 63) == 0) wmoments_store(red[threadIdx.x >> 6], a);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long* u0 = reinterpret_cast<const unsigned long long*>(red[0]);
        WMoments t{red[0][0], red[0][1], red[0][2], red[0][3], red[0][4], u0[5], u0[6], u0[7]};
#pragma unroll
        for (int wv = 1; wv < FIVEEQ_BLOCK / 64; ++wv) {
            const unsigned long long* u = reinterpret_cast<const unsigned long long*>(red[wv]);
            t.s1 += red[wv][0];
            t.s2 += red[wv][1];
            t.sw2 += red[wv][2];
            t.mn = fmin(t.mn, red[wv][3]);
            t.mx = fmax(t.mx, red[wv][4]);
            t.cnt += u[5];
            t.flags |= u[6];
            t.sw += u[7];
        }
        wmoments_store(partial + (row * gridDim.x + blockIdx.x) * WMOM_WORDS, t);
    }
}
// moments[row][8] = the partials of a row folded in a fixed order (one wave per row)
__global__ __launch_bounds__(64) void wrow_moments_fold_kernel(const int64_t chunks, const double* __restrict__ partial,
                                                               double* __restrict__ moments) {
    const int64_t row = blockIdx.x;
    WMoments a = wmoments_zero();
    for (int64_t c = threadIdx.x; c < chunks; c += 64) {
        const double* p = partial + (row * chunks + c) * WMOM_WORDS;
        const unsigned long long* u = reinterpret_cast<const unsigned long long*>(p);
        a.s1 += p[0];
        a.s2 += p[1];
        a.sw2 += p[2];
        a.mn = fmin(a.mn, p[3]);
        a.mx = fmax(a.mx, p[4]);
        a.cnt += u[5];
        a.flags |= u[6];
        a.sw += u[7];
    }
    wmoments_wave(a);
    if (threadIdx.x == 0) wmoments_store(moments + row * WMOM_WORDS, a);
}

// 7b.  hist[row][bin] += the WEIGHT of the members with w > 0 whose value falls in the bin (hist_bin, the rule of kernel 4,
// with the row's (lo, hi) read from device memory; a row with hi <= lo lands in bin 0; a NaN has no bin).  One workgroup =
// one row x one chunk of members: a privatised LDS histogram of 64-bit sums (ds_add_u64), then the non-zero bins are added to
// the global counters with 64-bit vector atomics.  Integer adds: exact, and the same bits in any order.
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void whist_rows_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                  const T* __restrict__ rows,
                                                                  const unsigned long long* __restrict__ weights,
                                                                  const double* __restrict__ ranges, const int n_bins,
                                                                  unsigned long long* __restrict__ hist) {
    __shared__ unsigned long long h[HIST_MAX_BINS];
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) h[b] = 0ull;
    __syncthreads();
    const int64_t row = blockIdx.y;
    const double lo = ranges[row * 2], hi = ranges[row * 2 + 1];
    const HistRule<T> rule = make_rule(T(0), lo, hi > lo ? (double)n_bins / (hi - lo) : 0.0, n_bins);
    const int64_t m0 = (int64_t)blockIdx.x * chunk;          // chunk is a multiple of 4 * FIVEEQ_BLOCK (host)
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    wfor_members(x, weights, m0, m1, wrows_wide(x, ld, weights), [&](const T v, const unsigned long long w, const bool) {
        const unsigned int b = hist_bin(rule, v);
        if (w != 0ull && b != (unsigned int)BIN_NAN) atomicAdd(&h[b], w);
    });
    __syncthreads();
    unsigned long long* out = hist + row * n_bins;
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) {
        const unsigned long long c = h[b];
        if (c) atomicAdd(&out[b], c);
    }
}

// 7c.  SELECTION of (value, weight) pairs: the members with w > 0 whose bin (the rule and ranges of 7b, bit for bit) is
// marked in binmask[row] are appended to cand[row][...] / candw[row][...] (same place in both; any order).  Compaction as in
// select_bins_kernel: ballot, consecutive places in a workgroup LDS buffer, ONE global atomic per workgroup; a workgroup whose
// buffer is full appends directly.  cand_n[row] counts every candidate, stored or not.
constexpr int WSELECT_LDS_CAND = 2048;
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void wselect_bins_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                    const T* __restrict__ rows,
                                                                    const unsigned long long* __restrict__ weights,
                                                                    const double* __restrict__ ranges, const int n_bins,
                                                                    const unsigned int* __restrict__ binmask, T* __restrict__ cand,
                                                                    unsigned long long* __restrict__ candw, const int64_t cap,
                                                                    unsigned long long* __restrict__ cand_n) {
    __shared__ unsigned int mask_s[HIST_MAX_BINS / 32];
    __shared__ T buf[WSELECT_LDS_CAND];
    __shared__ unsigned long long bufw[WSELECT_LDS_CAND];
    __shared__ unsigned int buf_next, buf_valid;
    __shared__ unsigned long long g_base;
    const int64_t row = blockIdx.y;
    const int mask_words = (n_bins + 31) >> 5;
    if ((int)threadIdx.x < mask_words) mask_s[threadIdx.x] = binmask[row * mask_words + threadIdx.x];
    if (threadIdx.x == 0) {
        buf_next = 0u;
        buf_valid = 0xffffffffu;
    }
    __syncthreads();
    const double lo = ranges[row * 2], hi = ranges[row * 2 + 1];
    const HistRule<T> rule = make_rule(T(0), lo, hi > lo ? (double)n_bins / (hi - lo) : 0.0, n_bins);      // 7b's rule for this row
    const int64_t m0 = (int64_t)blockIdx.x * chunk;
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    T* const out = cand + row * cap;
    unsigned long long* const outw = candw + row * cap;
    const int lane = threadIdx.x & 63;
    wfor_members(x, weights, m0, m1, wrows_wide(x, ld, weights), [&](const T v, const unsigned long long w, const bool have) {
        const unsigned int b = hist_bin(rule, v);
        const bool is_c = have && w != 0ull && b != (unsigned int)BIN_NAN && ((mask_s[b >> 5] >> (b & 31u)) & 1u);
        const unsigned long long cm = __ballot(is_c);
        if (cm != 0ull) {                                        // wave-uniform
            const unsigned int total = (unsigned int)__popcll(cm);
            const unsigned int rank = (unsigned int)__popcll(cm & ((1ull << lane) - 1ull));
            unsigned int pos = 0u;
            if (lane == 0) pos = atomicAdd(&buf_next, total);
            pos = (unsigned int)__builtin_amdgcn_readfirstlane((int)pos);
            if (pos + total <= (unsigned int)WSELECT_LDS_CAND) {
                if (is_c) buf[pos + rank] = v, bufw[pos + rank] = w;
            } else {                                             // the workgroup's buffer is full: straight to the row's buffer
                if (lane == 0) atomicMin(&buf_valid, pos);
                unsigned long long gp = 0ull;
                if (lane == 0) gp = atomicAdd(&cand_n[row], (unsigned long long)total);
                gp = ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(gp >> 32)) << 32) |
                     (unsigned int)__builtin_amdgcn_readfirstlane((int)(gp & 0xffffffffull));
                if (is_c && (int64_t)(gp + rank) < cap) out[gp + rank] = v, outw[gp + rank] = w;
            }
        }
    });
    __syncthreads();
    const unsigned int kept = min(min(buf_next, buf_valid), (unsigned int)WSELECT_LDS_CAND);
    if (kept) {
        if (threadIdx.x == 0) g_base = atomicAdd(&cand_n[row], (unsigned long long)kept);
        __syncthreads();
        const unsigned long long gb = g_base;
        for (unsigned int i = threadIdx.x; i < kept; i += FIVEEQ_BLOCK)
            if ((int64_t)(gb + i) < cap) out[gb + i] = buf[i], outw[gb + i] = bufw[i];
    }
}

// 7d.  PICK.  targets[row][q] = t >= 1: the wanted value is the smallest candidate x with (sum of the weights of the
// candidates <= x) >= t — host bookkeeping on the histogram of 7b: the weight of the marked bins below the percentile's bin,
// plus k_p minus the weight of ALL bins below it.  One 1024-thread workgroup per (row, target) finds it by RADIX SELECTION on
// the order-preserving integer image of the values (SortKey): 11 bits per pass from the top, a 2048-bin LDS histogram of the
// WEIGHT of the candidates that share the prefix found so far, one wave scans it and descends into the digit b with
// cumw[b-1] < t <= cumw[b], carrying t - cumw[b-1].  No sort; any number of candidates — the whole row when every member
// fell into one bin.  pool / poolw [row][seg][width]: values and weights as they arrived (one segment per rank on the root),
// seg_n[row][seg] valid entries each (more than width: taken as width).  picked[row][q] fp64; NaN when t < 1 or the
// candidates weigh less than t.
template <typename T>
__global__ __launch_bounds__(PICK_BLOCK) void wselect_pick_kernel(
    const int n_seg, const int64_t width, const T* __restrict__ pool, const unsigned long long* __restrict__ poolw,
    const unsigned long long* __restrict__ seg_n, const int n_targets, const long long* __restrict__ targets /* [rows][n_targets] */,
    double* __restrict__ picked) {
    using K = SortKey<T>;
    using U = typename K::U;
    __shared__ unsigned long long hist[1 << PICK_DIGIT];
    __shared__ long long target_s;               // remaining weight rank within the current prefix; < 1: no such candidate
    __shared__ U prefix_s;
    const int64_t row = blockIdx.x;
    const int q = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* const x = pool + row * n_seg * width;
    const unsigned long long* const xw = poolw + row * n_seg * width;
    if (threadIdx.x == 0) {
        target_s = targets[row * n_targets + q];
        prefix_s = (U)0;
    }
    __syncthreads();
    for (int hi = K::BITS; hi > 0 && target_s >= 1;) {                    // workgroup-uniform (target_s is read after a barrier)
        const int lo = hi > PICK_DIGIT ? hi - PICK_DIGIT : 0;
        const int nb = hi - lo;
        for (int i = threadIdx.x; i < (1 << nb); i += PICK_BLOCK) hist[i] = 0ull;
        __syncthreads();
        const U prefix = prefix_s;
        for (int g = 0; g < n_seg; ++g) {
            const int64_t cnt = min((int64_t)seg_n[row * n_seg + g], width);
            const T* xs = x + g * width;
            const unsigned long long* ws = xw + g * width;
            // whole waves iterate together.  A wave whose 64 candidates all fall into ONE digit (the top passes: every candidate
            // shares sign and exponent) adds their summed weight once instead of serialising 64 LDS atomics on one address.
            auto tally = [&](const T v, const unsigned long long w, const bool have) {
                const U key = K::of(v);
                const bool match = have && w != 0ull && (hi >= K::BITS || (key >> hi) == prefix);
                const unsigned int b = match ? (unsigned int)((key >> lo) & (U)((1u << nb) - 1u)) : ~0u;
                const unsigned int b0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)b);
                if (__ballot(b != b0) == 0ull) {                          // wave-uniform
                    if (b0 != ~0u) {
                        const unsigned long long s = wave_sum_u64(w);
                        if (lane == 0) atomicAdd(&hist[b0], s);
                    }
                } else if (match) {
                    atomicAdd(&hist[b], w);
                }
            };
            int64_t base = (int64_t)wave * 64;
            for (; base + PICK_BLOCK + 64 <= cnt; base += 2 * PICK_BLOCK) {              // two independent pairs of loads in flight
                const T v0 = xs[base + lane], v1 = xs[base + PICK_BLOCK + lane];
                const unsigned long long w0 = ws[base + lane], w1 = ws[base + PICK_BLOCK + lane];
                tally(v0, w0, true);
                tally(v1, w1, true);
            }
            for (; base < cnt; base += PICK_BLOCK) {
                const bool have = base + lane < cnt;
                tally(have ? xs[base + lane] : T(0), have ? ws[base + lane] : 0ull, have);
            }
        }
        __syncthreads();
        if (wave == 0) {                                                  // which digit holds the target?  lane l owns bins [l*per, (l+1)*per)
            const int per = (1 << nb) / 64;                               // 32 (11 bits) or 16 (10 bits)
            const unsigned long long t = (unsigned long long)target_s;
            unsigned long long mine = 0ull;
            for (int i = 0; i < per; ++i) mine += hist[lane * per + i];
            unsigned long long incl = mine;                               // inclusive prefix sum over the lanes
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) {
                const unsigned long long up = __shfl_up(incl, sh);
                if (lane >= sh) incl += up;
            }
            const unsigned long long before = incl - mine;
            const unsigned long long total = __shfl(incl, 63);
            if (t > total) {
                if (lane == 0) target_s = -1;                             // the candidates weigh less than the target
            } else if (t > before && t <= incl) {                         // exactly one lane
                unsigned long long rem = t - before;
                int b = lane * per;
                while (rem > hist[b]) rem -= hist[b++];
                target_s = (long long)rem;
                prefix_s = (nb < K::BITS ? (prefix << nb) : (U)0) | (U)b;
            }
        }
        __syncthreads();
        hi = lo;
    }
    if (threadIdx.x == 0) picked[row * n_targets + q] = target_s < 1 ? __builtin_nan("") : K::back(prefix_s);
}

}  // namespace fiveeq
