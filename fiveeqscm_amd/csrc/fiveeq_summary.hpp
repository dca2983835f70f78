// fiveeq_summary.hpp — kernels 3 to 6: the reference's function, the Latin hypercube, histograms of rows and the end-of-run summary passes.
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

template <typename T>
__device__ __forceinline__ void store_stream(T* p, T v) { *p = v; }   // plain store (hfc_conc_kernel only; the step kernels' stored rows go through their NT policy)

// ---------------------------------------------------------------------------------
// LDS counter increment with ONE round of wave-level aggregation (the histogram passes and the pick pass).  In the first decades of a run every member's T sits in a
// handful of bins: 64 lanes adding to the same LDS dword serialise (the first two 64-step chunks of a streamed run took
// 1.9 and 0.8 ms in the histogram pass against 0.35 ms later).
// So: the wave looks at the counter of its first lane; if at least 16 lanes want that same counter, ONE of them adds their
// number and the others of the group add nothing; every other lane adds as usual.  `key` identifies the counter (the bin;
// ~0u = this lane has nothing to count), `p` / `inc` are where and what this lane would add.  All lanes of the wave that
// are active at the call site must call it (it is a wave-level operation on the active lanes).
__device__ __forceinline__ void wave_lds_add(unsigned int* p, const unsigned int inc, const unsigned int key) {
    const unsigned int k0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)key);
    const unsigned long long same = __ballot(key == k0);
    const int n_same = __popcll(same);
    if (n_same >= 16) {                                               // wave-uniform
        if (key == k0) {
            if (k0 != ~0u && (int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(p, inc * (unsigned int)n_same);
        } else if (key != ~0u) {
            atomicAdd(p, inc);
        }
    } else if (key != ~0u) {
        atomicAdd(p, inc);
    }
}

// ---------------------------------------------------------------------------------
// Kernel 5 — shard-computable Latin hypercube.  u[k][m - m0] for members m0 <= m < m0 + n of a
// design over n_total members: u = (pi_k(m) + jitter_k(m)) / n_total, pi_k a KEYED BIJECTION of
// [0, n_total) (4-round balanced Feistel network on the next even power of two, cycle-walked back
// into range), jitter a 24-bit counter-based hash placed mid-cell, so u lies strictly inside
// stratum pi_k(m).  Pure function of (seed, dimension, m, n_total): any rank computes exactly its
// own members, on its own device, and the design is the same for every world size.  Integer
// arithmetic + one fp64 add that is EXACT for n_total <= 2^28 (28 stratum bits + 25 jitter bits <= 53; the C ABI
// refuses larger designs) + one correctly rounded division: params.lhs_rows (NumPy) reproduces it bit for bit.
// ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t lhs_mix64(uint64_t z) {      // splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t lhs_dim_key(uint64_t seed, int dim) {
    return lhs_mix64(seed + 0x9e3779b97f4a7c15ULL * (uint64_t)(dim + 1));
}
__host__ __device__ __forceinline__ uint64_t lhs_permute(uint64_t m, uint64_t n_total, int half_bits, uint64_t key) {
    const uint64_t mask = (1ULL << half_bits) - 1ULL;
    uint64_t x = m;
    do {
        uint64_t left = x >> half_bits, right = x & mask;
#pragma unroll
        for (int rnd = 0; rnd < 4; ++rnd) {
            const uint64_t f = lhs_mix64(right ^ (key + 0xd1342543de82ef95ULL * (uint64_t)(rnd + 1))) & mask;
            const uint64_t nl = right;
            right = left ^ f;
            left = nl;
        }
        x = (left << half_bits) | right;
    } while (x >= n_total);                                    // cycle-walk: the domain is < 4 n_total
    return x;
}
__global__ __launch_bounds__(FIVEEQ_BLOCK) void lhs_kernel(const uint64_t seed, const int64_t n_total, const int half_bits,
                                                           const int64_t m0, const int64_t n, const int dim0,
                                                           const int64_t ld, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int dim = dim0 + (int)blockIdx.y;
    const uint64_t key = lhs_dim_key(seed, dim);
    const uint64_t m = (uint64_t)(m0 + i);
    const uint64_t stratum = lhs_permute(m, (uint64_t)n_total, half_bits, key);
    const uint64_t jbits = lhs_mix64(m ^ (key * 0xff51afd7ed558ccdULL + 0xc4ceb9fe1a85ec53ULL)) >> 40;   // 24 bits
    const double jitter = ((double)jbits + 0.5) * 0x1.0p-24;                                               // (0, 1)
    out[(int64_t)blockIdx.y * ld + i] = ((double)stratum + jitter) / (double)n_total;
}

// ---------------------------------------------------------------------------------
// Kernel 3 — ensemble form of the reference's calculate_hfc_conc
// (U_FaIR/concentrations.py:5: emissions[0]*exp(-time)): out[k][m] = e0[m]*exp(-time[k]).
// exp(-time[k]) is shared by every member: each workgroup evaluates a tile of 256 time
// points once into LDS, then every lane scales its member by the staged factors.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(FIVEEQ_BLOCK) void hfc_conc_kernel(
    const int64_t n, const int64_t ld, const int n_time,
    const double* __restrict__ e0, const double* __restrict__ time, double* __restrict__ out) {
    __shared__ double decay[FIVEEQ_BLOCK];
    const int64_t m = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    const bool active = m < n;
    const double e = active ? e0[m] : 0.0;
    for (int k0 = 0; k0 < n_time; k0 += FIVEEQ_BLOCK) {
        const int nk = min(FIVEEQ_BLOCK, n_time - k0);
        __syncthreads();
        if ((int)threadIdx.x < nk) decay[threadIdx.x] = exp(-time[k0 + threadIdx.x]);
        __syncthreads();
        if (active)
            for (int k = 0; k < nk; ++k) store_stream(&out[(int64_t)(k0 + k) * ld + m], e * decay[k]);
    }
}

// ---------------------------------------------------------------------------------
// Kernel 4 — fixed-bin histograms of stored rows (all-timestep percentiles).
// hist[row][bin] += #members with lo + bin*w <= x < lo + (bin+1)*w ; values outside [lo, hi) go to
// the edge bins, NaNs are skipped.  One workgroup = one row x one chunk of members: privatised LDS
// histogram (ds_add_u32), then only the non-zero bins are added to the global 64-bit counters.  The
// host sizes the chunk so that the grid still fills the chip (>= ~2048 workgroups) but no finer: the
// global atomics of the flush, not the read, were the cost at 16384 members per chunk (60 us per
// 12.5M-member row in round 1).  Reads each stored value once: 8 (4) B per member and row.
// ---------------------------------------------------------------------------------
constexpr int HIST_CHUNK_MIN = 16384;
constexpr int HIST_MAX_BINS = 4096;
// (Tried in round 4 and not kept: 2 or 4 SUB-HISTOGRAMS per workgroup, lane l counting into number l mod n, bank-shifted, to
// spare the LDS atomic unit same-address collisions.  The passes got SLOWER — 5.4 -> 7.6 -> 13.4 us per 12.5M-member row of
// bin indices — because the larger LDS footprint halves / quarters the resident waves: these passes run at the box's plain
// copy rate for their access width and are bound by memory-level parallelism, not by LDS atomics.  profiles/r04/ab_variants.txt)

template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void hist_rows_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                 const T* __restrict__ rows, const double lo_all,
                                                                 const double inv_w_all, const int n_bins,
                                                                 unsigned long long* __restrict__ hist,
                                                                 const double* __restrict__ ranges /* [rows][2] or nullptr */) {
    __shared__ unsigned int h[HIST_MAX_BINS];
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) h[b] = 0u;
    __syncthreads();
    const int64_t row = blockIdx.y;
    // ranges != nullptr: every row has its own (lo, hi) in device memory (the summary pass: each row's global extrema);
    // a row with hi <= lo is constant and lands in bin 0
    const double lo = ranges ? ranges[row * 2] : lo_all;
    const double inv_w = ranges ? (ranges[row * 2 + 1] > lo ? (double)n_bins / (ranges[row * 2 + 1] - lo) : 0.0) : inv_w_all;
    const int64_t m0 = (int64_t)blockIdx.x * chunk;
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    const HistRule<T> rule = make_rule(T(0), lo, inv_w, n_bins);
    auto count = [&](const T xv) {
        const unsigned int b = hist_bin(rule, xv);                                    // a NaN has no bin and is not counted
        const bool ok = b != (unsigned int)BIN_NAN;
        wave_lds_add(&h[ok ? b : 0u], 1u, ok ? b : ~0u);
    };
    // the same value counted with a PLAIN LDS atomic: for rows that do not crowd into a few bins (see hist_bins_kernel: the
    // crowding test of wave_lds_add runs once per group of four loads, on the first of them)
    auto count_plain = [&](const T xv) {
        const unsigned int b = hist_bin(rule, xv);
        if (b != (unsigned int)BIN_NAN) atomicAdd(&h[b], 1u);
    };
    int64_t m = m0 + threadIdx.x;
    for (; m + 3 * FIVEEQ_BLOCK < m1; m += 4 * FIVEEQ_BLOCK) {      // four independent loads in flight per lane
        const T v0 = x[m], v1 = x[m + FIVEEQ_BLOCK], v2 = x[m + 2 * FIVEEQ_BLOCK], v3 = x[m + 3 * FIVEEQ_BLOCK];
        const unsigned int b0 = hist_bin(rule, v0);
        const unsigned int k0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)b0);
        if (__popcll(__ballot(b0 == k0)) >= 16) {                    // wave-uniform: a crowded row
            count(v0);
            count(v1);
            count(v2);
            count(v3);
        } else {
            count_plain(v0);
            count_plain(v1);
            count_plain(v2);
            count_plain(v3);
        }
    }
    for (; m < m1; m += FIVEEQ_BLOCK) count(x[m]);
    __syncthreads();
    unsigned long long* out = hist + row * n_bins;
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) {
        const unsigned int c = h[b];
        if (c) atomicAdd(&out[b], (unsigned long long)c);
    }
}

// ---------------------------------------------------------------------------------
// Kernel 4b — the pass of the bin-index ring: hist[row][b] += #members whose stored bin index is b (BIN_NAN skipped).
// Same grid shape and LDS privatisation as hist_rows_kernel; reads 2 bytes per member and row, four members per 8-byte load.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(FIVEEQ_BLOCK) void hist_bins_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                 const unsigned short* __restrict__ rows, const int n_bins,
                                                                 unsigned long long* __restrict__ hist) {
    __shared__ unsigned int h[HIST_MAX_BINS];
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) h[b] = 0u;
    __syncthreads();
    const int64_t row = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * chunk;          // chunk is a multiple of 8 * FIVEEQ_BLOCK (host)
    const int64_t m1 = min(m0 + chunk, n);
    const unsigned short* x = rows + row * ld;
    auto count = [&](const unsigned int b) {
        const bool ok = b < (unsigned int)n_bins;
        wave_lds_add(&h[ok ? b : 0u], 1u, ok ? b : ~0u);
    };
    // rows 16-byte aligned: 8 members per lane and load (1 KiB per wave-instruction: the box copies 17 % faster at 16 than at
    // 8 bytes per lane), two loads in flight, over the whole strides of 8 x 256 members; what is left of the chunk (fewer
    // than 2048 members, only in the row's last chunk) goes one member per lane
    const bool wide = ((((uintptr_t)x) | ((uintptr_t)(ld * 2))) & 15) == 0;
    int64_t m = m0 + (int64_t)threadIdx.x * 4;
    if (wide) {
        // Eight members per lane.  The wave-level aggregation of wave_lds_add exists for rows whose members crowd into a
        // handful of bins (the first decades of a run); it costs ~12 instructions per member, and beside a VALU-bound fused
        // kernel this pass is paid in ISSUE SLOTS, not in bandwidth.  So the crowding test runs ONCE per load, on the lane's
        // first member: a crowded row takes the aggregated path for all eight, every other row plain LDS atomics.
        auto count8 = [&](const uint4 v) {
            const unsigned int b0 = v.x & 0xffffu;
            const unsigned int k0 = (unsigned int)__builtin_amdgcn_readfirstlane((int)b0);
            if (__popcll(__ballot(b0 == k0)) >= 16) {                   // wave-uniform
                count(b0);
                count(v.x >> 16);
                count(v.y & 0xffffu);
                count(v.y >> 16);
                count(v.z & 0xffffu);
                count(v.z >> 16);
                count(v.w & 0xffffu);
                count(v.w >> 16);
            } else {
                auto plain = [&](const unsigned int b) {
                    if (b < (unsigned int)n_bins) atomicAdd(&h[b], 1u);
                };
                plain(b0);
                plain(v.x >> 16);
                plain(v.y & 0xffffu);
                plain(v.y >> 16);
                plain(v.z & 0xffffu);
                plain(v.z >> 16);
                plain(v.w & 0xffffu);
                plain(v.w >> 16);
            }
        };
        constexpr int64_t STRIDE = 8 * FIVEEQ_BLOCK;
        const int64_t whole = m0 + (m1 - m0) / STRIDE * STRIDE;
        int64_t m8 = m0 + (int64_t)threadIdx.x * 8;
        for (; m8 + STRIDE < whole; m8 += 2 * STRIDE) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + m8);
            const uint4 u = *reinterpret_cast<const uint4*>(x + m8 + STRIDE);
            count8(v);
            count8(u);
        }
        if (m8 < whole) count8(*reinterpret_cast<const uint4*>(x + m8));
        for (int64_t r = whole + threadIdx.x; r < m1; r += FIVEEQ_BLOCK) count(x[r]);
        m = m1;
    }
    for (; m < m1; m += 4 * FIVEEQ_BLOCK)                     // unaligned rows, and the ragged tail of the last chunk
        for (int j = 0; j < 4 && m + j < m1; ++j) count(x[m + j]);
    __syncthreads();
    unsigned long long* out = hist + row * n_bins;
    for (int b = threadIdx.x; b < n_bins; b += FIVEEQ_BLOCK) {
        const unsigned int c = h[b];
        if (c) atomicAdd(&out[b], (unsigned long long)c);
    }
}

// ---------------------------------------------------------------------------------
// Kernels 6a-6c — the END-OF-RUN SUMMARY as HIP passes (form (i): exact percentiles by selection).
// The host side (fiveeqscm_amd/distributed.py) needs, per output row of T over this rank's members:
//   6a  the moments (sum, sum of squares, min, max)                      row_moments_kernel + row_moments_fold_kernel
//   --  a 4096-bin histogram between the GLOBAL min and max              hist_rows_kernel with per-row ranges (RANGED)
//   6c  the members of the histogram bins that hold the wanted order statistics, compacted                     select_bins_kernel
//   6d  the order statistics, picked out of those candidates by radix selection                                select_pick_kernel
// Each pass reads the rows once with 16-byte loads; nothing else of the ensemble's size moves.
// ---------------------------------------------------------------------------------
template <typename T> struct Wide;                       // 16 bytes of row per lane and load
template <> struct Wide<double> { using V = double2; static constexpr int N = 2; };
template <> struct Wide<float> { using V = float4; static constexpr int N = 4; };
__device__ __forceinline__ double wide_get(const double2& v, int i) { return i == 0 ? v.x : v.y; }
__device__ __forceinline__ float wide_get(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// 6a.  partial[row][chunk][4] = (sum, sum of squares, min, max) of members [chunk * `chunk`, ...) of the row, fp64 sums
// of the exactly converted elements; min / max ignore NaNs (like the kernels' own wave records), the sums propagate them.
// Fixed summation order (lane-strided, xor-shuffle tree, wave order): the same bits on every run.
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void row_moments_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                   const T* __restrict__ rows, double* __restrict__ partial) {
    using WV = typename Wide<T>::V;
    constexpr int WN = Wide<T>::N;
    __shared__ double red[FIVEEQ_BLOCK / 64][4];
    const int64_t row = blockIdx.y;
    const int64_t m0 = (int64_t)blockIdx.x * chunk;          // chunk is a multiple of WN * FIVEEQ_BLOCK (host)
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    const double inf = __builtin_inf();
    double s1 = 0.0, s2 = 0.0, mn = inf, mx = -inf;
    auto take = [&](const T xv) {
        const double v = (double)xv;
        s1 += v;
        s2 = __builtin_fma(v, v, s2);
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    };
    const bool wide = ((((uintptr_t)x) | ((uintptr_t)(ld * sizeof(T)))) & 15) == 0;
    int64_t m = m0 + (int64_t)threadIdx.x * WN;
    if (wide) {
        for (; m + 2 * WN * FIVEEQ_BLOCK + WN - 1 < m1; m += 3 * WN * FIVEEQ_BLOCK) {     // three independent loads in flight
            const WV a = *reinterpret_cast<const WV*>(x + m);
            const WV b = *reinterpret_cast<const WV*>(x + m + WN * FIVEEQ_BLOCK);
            const WV c = *reinterpret_cast<const WV*>(x + m + 2 * WN * FIVEEQ_BLOCK);
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(a, j));
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(b, j));
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(c, j));
        }
        for (; m + WN - 1 < m1; m += WN * FIVEEQ_BLOCK) {
            const WV a = *reinterpret_cast<const WV*>(x + m);
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(a, j));
        }
    }
    for (; m < m1; m += WN * FIVEEQ_BLOCK)                      // unaligned rows, and the ragged tail of the last chunk
        for (int j = 0; j < WN && m + j < m1; ++j) take(x[m + j]);
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        s1 += __shfl_xor(s1, sh);
        s2 += __shfl_xor(s2, sh);
        mn = fmin(mn, __shfl_xor(mn, sh));
        mx = fmax(mx, __shfl_xor(mx, sh));
    }
    if ((threadIdx.x & 63) == 0) {
        double* r = red[threadIdx.x >> 6];
        r[0] = s1, r[1] = s2, r[2] = mn, r[3] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = red[0][0], b = red[0][1], c = red[0][2], d = red[0][3];
#pragma unroll
        for (int w = 1; w < FIVEEQ_BLOCK / 64; ++w) {
            a += red[w][0];
            b += red[w][1];
            c = fmin(c, red[w][2]);
            d = fmax(d, red[w][3]);
        }
        double* o = partial + (row * gridDim.x + blockIdx.x) * 4;
        o[0] = a, o[1] = b, o[2] = c, o[3] = d;
    }
}
// moments[row][4] = the partials of a row folded in a fixed order (one wave per row)
__global__ __launch_bounds__(64) void row_moments_fold_kernel(const int64_t chunks, const double* __restrict__ partial,
                                                              double* __restrict__ moments) {
    const int64_t row = blockIdx.x;
    const double inf = __builtin_inf();
    double s1 = 0.0, s2 = 0.0, mn = inf, mx = -inf;
    for (int64_t c = threadIdx.x; c < chunks; c += 64) {
        const double* p = partial + (row * chunks + c) * 4;
        s1 += p[0];
        s2 += p[1];
        mn = fmin(mn, p[2]);
        mx = fmax(mx, p[3]);
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        s1 += __shfl_xor(s1, sh);
        s2 += __shfl_xor(s2, sh);
        mn = fmin(mn, __shfl_xor(mn, sh));
        mx = fmax(mx, __shfl_xor(mx, sh));
    }
    if (threadIdx.x == 0) {
        double* o = moments + row * 4;
        o[0] = s1, o[1] = s2, o[2] = mn, o[3] = mx;
    }
}

// 6c.  SELECTION.  The histogram of pass 2 says, exactly, how many members lie in each bin, and the bin rule is monotone in
// the value: the order statistic of global index i lies in the bin b with cdf[b-1] <= i < cdf[b], and is the
// (i - cdf[b-1])-th smallest member OF THAT BIN.  So the host marks the bins that hold wanted order statistics
// (binmask[row]: one bit per bin) and this pass, computing every member's bin with the SAME rule from the same (lo, hi),
// appends the members of marked bins — the CANDIDATES, a few thousandths of the row — to cand[row][...] (any order).
// Compaction: the wave's candidates take consecutive places in a workgroup LDS buffer (one LDS atomic per wave-load that has
// any), which is appended to the row's global buffer with ONE global atomic per workgroup; a workgroup whose buffer is full
// (a row with heavy ties) appends its further candidates directly.  cand_n[row] counts every candidate, stored or not; the
// host sizes cap from the histogram, so it never overflows unless the caller passed a smaller one.
constexpr int SELECT_LDS_CAND = 2048;
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void select_bins_kernel(const int64_t n, const int64_t ld, const int64_t chunk,
                                                                   const T* __restrict__ rows, const double* __restrict__ ranges,
                                                                   const int n_bins, const unsigned int* __restrict__ binmask,
                                                                   T* __restrict__ cand, const int64_t cap,
                                                                   unsigned long long* __restrict__ cand_n) {
    using WV = typename Wide<T>::V;
    constexpr int WN = Wide<T>::N;
    __shared__ unsigned int mask_s[HIST_MAX_BINS / 32];
    __shared__ T buf[SELECT_LDS_CAND];
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
    const HistRule<T> rule = make_rule(T(0), lo, hi > lo ? (double)n_bins / (hi - lo) : 0.0, n_bins);      // pass 2's rule for this row
    const int64_t m0 = (int64_t)blockIdx.x * chunk;             // chunk is a multiple of WN * FIVEEQ_BLOCK (host)
    const int64_t m1 = min(m0 + chunk, n);
    const T* x = rows + row * ld;
    T* const out = cand + row * cap;
    const int lane = threadIdx.x & 63;

    // one value per lane: place it if its bin is marked.  `have` = this lane holds a member.
    auto take = [&](const T v, const bool have) {
        const unsigned int b = hist_bin(rule, v);
        const bool is_c = have && b != (unsigned int)BIN_NAN && ((mask_s[b >> 5] >> (b & 31u)) & 1u);
        const unsigned long long cm = __ballot(is_c);
        if (cm != 0ull) {                                        // wave-uniform; a few per cent of the wave-loads of a smooth row
            const unsigned int total = (unsigned int)__popcll(cm);
            const unsigned int rank = (unsigned int)__popcll(cm & ((1ull << lane) - 1ull));
            unsigned int pos = 0u;
            if (lane == 0) pos = atomicAdd(&buf_next, total);
            pos = (unsigned int)__builtin_amdgcn_readfirstlane((int)pos);
            if (pos + total <= (unsigned int)SELECT_LDS_CAND) {
                if (is_c) buf[pos + rank] = v;
            } else {                                             // the workgroup's buffer is full: straight to the row's buffer
                if (lane == 0) atomicMin(&buf_valid, pos);
                unsigned long long gp = 0ull;
                if (lane == 0) gp = atomicAdd(&cand_n[row], (unsigned long long)total);
                gp = ((unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(gp >> 32)) << 32) |
                     (unsigned int)__builtin_amdgcn_readfirstlane((int)(gp & 0xffffffffull));
                if (is_c && (int64_t)(gp + rank) < cap) out[gp + rank] = v;
            }
        }
    };
    const bool wide = ((((uintptr_t)x) | ((uintptr_t)(ld * sizeof(T)))) & 15) == 0;
    // every lane of a wave runs the same number of iterations (take() is a wave-level operation): the loop bound is on the
    // wave's first member, lanes past the end of the chunk carry have = false
    const int64_t wave_m = m0 + (int64_t)(threadIdx.x & ~63) * WN;
    int64_t m = m0 + (int64_t)threadIdx.x * WN;
    constexpr int64_t STEP = (int64_t)WN * FIVEEQ_BLOCK;
    int64_t wm = wave_m;
    if (wide) {
        for (; wm + STEP + 64 * WN <= m1; wm += 2 * STEP, m += 2 * STEP) {      // two independent 16-byte loads in flight
            const WV a = *reinterpret_cast<const WV*>(x + m);
            const WV b = *reinterpret_cast<const WV*>(x + m + STEP);
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(a, j), true);
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(b, j), true);
        }
    }
    for (; wm < m1; wm += STEP, m += STEP) {
        if (wide && wm + 64 * WN <= m1) {
            const WV a = *reinterpret_cast<const WV*>(x + m);
#pragma unroll
            for (int j = 0; j < WN; ++j) take(wide_get(a, j), true);
        } else {
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const bool have = m + j < m1;
                take(have ? x[m + j] : T(0), have);
            }
        }
    }
    __syncthreads();
    const unsigned int kept = min(min(buf_next, buf_valid), (unsigned int)SELECT_LDS_CAND);
    if (kept) {
        if (threadIdx.x == 0) g_base = atomicAdd(&cand_n[row], (unsigned long long)kept);
        __syncthreads();
        const unsigned long long gb = g_base;
        for (unsigned int i = threadIdx.x; i < kept; i += FIVEEQ_BLOCK)
            if ((int64_t)(gb + i) < cap) out[gb + i] = buf[i];
    }
}

// 6d.  PICK.  The order statistics themselves, read off the candidates WITHOUT sorting them.  ranks[row][q] is where target q
// sits among the row's candidates taken in ascending order — integer bookkeeping on the histogram, done by the host BEFORE
// the selection pass ran (for the order statistic of index i in bin b: the members of marked bins below b, plus i - cdf[b-1]) —
// so selection and pick run back to back with no host round trip between them.  One 1024-thread workgroup per (row, target)
// finds the candidate of that rank by RADIX SELECTION on the order-preserving integer image of the values: 11 bits per pass
// from the top, a 2048-bin LDS histogram of the candidates that share the target's prefix so far (wave-aggregated: in the
// top pass every candidate shares one bin), one wave then walks the bins to the one holding the rank.  3 (fp32) or 6 (fp64)
// passes over a few thousand to a few hundred thousand L2-resident values.  pool[row][seg][width] holds the candidates as
// they arrived: one segment (this rank's cand buffer), or one per rank on the root; seg_n[row][seg] valid entries each.
// Out: picked[row][n_targets] fp64; NaN when the rank is negative or not below the row's number of candidates.
constexpr int PICK_BLOCK = 1024;
template <typename T> struct SortKey;
template <> struct SortKey<float> {
    using U = unsigned int;
    static constexpr int BITS = 32;
    static __device__ __forceinline__ U of(float v) {
        const U u = __float_as_uint(v);
        return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    }
    static __device__ __forceinline__ double back(U k) {
        return (double)__uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
    }
};
template <> struct SortKey<double> {
    using U = unsigned long long;
    static constexpr int BITS = 64;
    static __device__ __forceinline__ U of(double v) {
        const U u = (U)__double_as_longlong(v);
        return u ^ ((u >> 63) ? 0xffffffffffffffffull : 0x8000000000000000ull);
    }
    static __device__ __forceinline__ double back(U k) {
        return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : 0xffffffffffffffffull)));
    }
};

constexpr int PICK_DIGIT = 11;                      // bits per radix pass: 2048 LDS bins; 3 passes for fp32, 6 for fp64
template <typename T>
__global__ __launch_bounds__(PICK_BLOCK) void select_pick_kernel(
    const int n_seg, const int64_t width, const T* __restrict__ pool, const unsigned long long* __restrict__ seg_n,
    const int n_targets, const long long* __restrict__ ranks /* [rows][n_targets] */, double* __restrict__ picked) {
    using K = SortKey<T>;
    using U = typename K::U;
    __shared__ unsigned int hist[1 << PICK_DIGIT];
    __shared__ long long rank_s;                 // remaining rank within the current prefix; < 0: no such candidate
    __shared__ U prefix_s;
    const int64_t row = blockIdx.x;
    const int q = blockIdx.y;                    // ONE target per workgroup: (rows x targets) workgroups share the chip
    const int Q = n_targets;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T* const x = pool + row * n_seg * width;
    if (threadIdx.x == 0) {
        long long total = 0;                                  // a segment holds at most `width` stored candidates, whatever was FOUND
        for (int g = 0; g < n_seg; ++g) total += min((long long)seg_n[row * n_seg + g], (long long)width);
        long long r = ranks[row * Q + q];
        if (r < 0 || r >= total) r = -1;
        rank_s = r;
        prefix_s = (U)0;
    }
    __syncthreads();
    if (rank_s >= 0) {                                                   // workgroup-uniform
        for (int hi = K::BITS; hi > 0;) {
            const int lo = hi > PICK_DIGIT ? hi - PICK_DIGIT : 0;
            const int nb = hi - lo;
            for (int i = threadIdx.x; i < (1 << nb); i += PICK_BLOCK) hist[i] = 0u;
            __syncthreads();
            const U prefix = prefix_s;
            for (int g = 0; g < n_seg; ++g) {
                const int64_t cnt = min((int64_t)seg_n[row * n_seg + g], width);
                const T* xs = x + g * width;
                // whole waves iterate together (wave_lds_add is a wave-level operation)
                auto tally = [&](const T v, const bool have) {
                    const U key = K::of(v);
                    const bool match = have && (hi >= K::BITS || (key >> hi) == prefix);
                    const unsigned int b = (unsigned int)((key >> lo) & (U)((1u << nb) - 1u));
                    wave_lds_add(&hist[b], 1u, match ? b : ~0u);
                };
                int64_t base = (int64_t)wave * 64;
                for (; base + 3 * PICK_BLOCK + 64 <= cnt; base += 4 * PICK_BLOCK) {      // four independent loads in flight
                    const T v0 = xs[base + lane], v1 = xs[base + PICK_BLOCK + lane], v2 = xs[base + 2 * PICK_BLOCK + lane],
                            v3 = xs[base + 3 * PICK_BLOCK + lane];
                    tally(v0, true);
                    tally(v1, true);
                    tally(v2, true);
                    tally(v3, true);
                }
                for (; base < cnt; base += PICK_BLOCK) {
                    const bool have = base + lane < cnt;
                    tally(have ? xs[base + lane] : T(0), have);
                }
            }
            __syncthreads();
            if (wave == 0) {                                             // which bin holds the rank?  lane l owns bins [l*per, (l+1)*per)
                const int per = (1 << nb) / 64;                          // 32 (11 bits) or 16 (10 bits)
                const long long r = rank_s;
                unsigned int mine = 0u;
                for (int i = 0; i < per; ++i) mine += hist[lane * per + i];
                unsigned int incl = mine;                                // inclusive prefix sum over the lanes
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) {
                    const unsigned int up = __shfl_up(incl, sh);
                    if (lane >= sh) incl += up;
                }
                const long long before = (long long)incl - mine;
                if (r >= before && r < (long long)incl) {                // exactly one lane: the counts sum to more than r
                    long long rem = r - before;
                    int b = lane * per;
                    while (rem >= (long long)hist[b]) rem -= hist[b++];
                    rank_s = rem;
                    prefix_s = (nb < K::BITS ? (prefix << nb) : (U)0) | (U)b;
                }
            }
            __syncthreads();
            hi = lo;
        }
    }
    if (threadIdx.x == 0) picked[row * Q + q] = rank_s < 0 ? __builtin_nan("") : K::back(prefix_s);
}

}  // namespace fiveeq
