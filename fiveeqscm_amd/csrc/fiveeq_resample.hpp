// fiveeq_resample.hpp — kernels 8a-8c: systematic RESAMPLING of a weighted ensemble (include/fiveeq.h, "RESAMPLING").
// Part of fiveeq_device.hpp, which includes it after fiveeq_wsummary.hpp: include that header, not this one.
//
// (members, integer weights) -> a dense equal-weight ensemble: output j is a copy of the first member whose inclusive
// cumulative weight exceeds the integer position p_j = floor((j W + rho) / M).  Every quantity that decides a copy is a
// 64-bit integer, so the result is the same bits for every shard split and world size.
//   8a  wscan_sums_kernel, wscan_spine_kernel, wscan_tiles_kernel   inclusive scan of the weights: reduce, then scan
//   8b  resample_pick_kernel                                        per output: upper bound of its position in the scan
//   8c  gather_rows_kernel                                          rows_out[r][k] = rows_in[r][src[k]], every row in one launch
// No kernel waits on another workgroup: the scan is three launches (tile sums, a scan of the tile sums by ONE workgroup, tile
// scans), ordered by the stream.
#pragma once

namespace fiveeq {

constexpr int WSCAN_ITEMS = 4;                                 // consecutive weights per lane: two 16-byte loads
constexpr int WSCAN_TILE = WSCAN_ITEMS * FIVEEQ_BLOCK;         // weights per workgroup of 8a
constexpr int WSCAN_WORDS = 2;                                 // workspace words per tile: its sum, its flags

// exclusive prefix sum of v over the threads of a FIVEEQ_BLOCK workgroup (thread order), and the workgroup's total.  Two
// barriers: `tot` may be used again right after the call.
__device__ __forceinline__ unsigned long long block_scan_u64(const unsigned long long v, unsigned long long (&tot)[FIVEEQ_BLOCK / 64],
                                                             unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const unsigned long long up = __shfl_up(incl, sh);
        if (lane >= sh) incl += up;
    }
    if (lane == 63) tot[wave] = incl;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
#pragma unroll
    for (int wv = 0; wv < FIVEEQ_BLOCK / 64; ++wv) {
        const unsigned long long t = tot[wv];
        before += wv < wave ? t : 0ull;
        all += t;
    }
    __syncthreads();
    total = all;
    return before + incl - v;
}

// the WSCAN_ITEMS weights of this lane: members [m, m + WSCAN_ITEMS) of n, 0 past the end.  `wide`: w is 16-byte aligned
// (m is a multiple of 4, so every lane's address is).
__device__ __forceinline__ void wscan_load(const unsigned long long* __restrict__ w, const int64_t m, const int64_t n, const bool wide,
                                           unsigned long long (&x)[WSCAN_ITEMS]) {
    if (wide && m + WSCAN_ITEMS <= n) {
#pragma unroll
        for (int j = 0; j < WSCAN_ITEMS; j += 2) {
            const ulonglong2 p = *reinterpret_cast<const ulonglong2*>(w + m + j);
            x[j] = p.x, x[j + 1] = p.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < WSCAN_ITEMS; ++j) x[j] = m + j < n ? w[m + j] : 0ull;
    }
}

// 8a (1).  partial[tile] = (sum of the tile's weights, WFLAG_RANGE if one of them is above 2^32).  Sums wrap modulo 2^64
// when the weights break the contract; the flag then says so.
__global__ __launch_bounds__(FIVEEQ_BLOCK) void wscan_sums_kernel(const int64_t n, const unsigned long long* __restrict__ w,
                                                                  unsigned long long* __restrict__ partial) {
    __shared__ unsigned long long red[FIVEEQ_BLOCK / 64][2];
    const int64_t m = (int64_t)blockIdx.x * WSCAN_TILE + (int64_t)threadIdx.x * WSCAN_ITEMS;
    unsigned long long x[WSCAN_ITEMS];
    wscan_load(w, m, n, (((uintptr_t)w) & 15) == 0, x);
    unsigned long long s = 0ull, big = 0ull;
#pragma unroll
    for (int j = 0; j < WSCAN_ITEMS; ++j) {
        s += x[j];
        big |= x[j] > WEIGHT_ONE ? 1ull : 0ull;
    }
    s = wave_sum_u64(s);
    const unsigned long long any = __ballot(big != 0ull);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = s, red[threadIdx.x >> 6][1] = any;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0ull, f = 0ull;
#pragma unroll
        for (int wv = 0; wv < FIVEEQ_BLOCK / 64; ++wv) t += red[wv][0], f |= red[wv][1];
        partial[(int64_t)blockIdx.x * WSCAN_WORDS] = t;
        partial[(int64_t)blockIdx.x * WSCAN_WORDS + 1] = f ? WFLAG_RANGE : 0ull;
    }
}

// 8a (2).  ONE workgroup: the tile sums become their exclusive prefix sums, in place (rounds of FIVEEQ_BLOCK tiles, the
// total of the rounds before carried in a register); flags[0] = the OR of the tiles' flags (written, not accumulated).
__global__ __launch_bounds__(FIVEEQ_BLOCK) void wscan_spine_kernel(const int64_t tiles, unsigned long long* __restrict__ partial,
                                                                   unsigned long long* __restrict__ flags) {
    __shared__ unsigned long long tot[FIVEEQ_BLOCK / 64];
    unsigned long long carry = 0ull, f = 0ull;
    for (int64_t base = 0; base < tiles; base += FIVEEQ_BLOCK) {          // workgroup-uniform bounds
        const int64_t i = base + threadIdx.x;
        const bool have = i < tiles;
        const unsigned long long v = have ? partial[i * WSCAN_WORDS] : 0ull;
        f |= have ? partial[i * WSCAN_WORDS + 1] : 0ull;
        unsigned long long total;
        const unsigned long long before = block_scan_u64(v, tot, total);
        if (have) partial[i * WSCAN_WORDS] = carry + before;
        carry += total;
    }
    const int any = __syncthreads_or(f != 0ull);
    if (threadIdx.x == 0) flags[0] = any ? WFLAG_RANGE : 0ull;
}

// 8a (3).  cum[m] = (the weight of the tiles before this one, from (2)) + the inclusive prefix sum inside the tile.
__global__ __launch_bounds__(FIVEEQ_BLOCK) void wscan_tiles_kernel(const int64_t n, const unsigned long long* __restrict__ w,
                                                                   const unsigned long long* __restrict__ partial,
                                                                   unsigned long long* __restrict__ cum) {
    __shared__ unsigned long long tot[FIVEEQ_BLOCK / 64];
    const int64_t m = (int64_t)blockIdx.x * WSCAN_TILE + (int64_t)threadIdx.x * WSCAN_ITEMS;
    unsigned long long x[WSCAN_ITEMS];
    wscan_load(w, m, n, (((uintptr_t)w) & 15) == 0, x);
#pragma unroll
    for (int j = 1; j < WSCAN_ITEMS; ++j) x[j] += x[j - 1];
    unsigned long long total;
    const unsigned long long before = partial[(int64_t)blockIdx.x * WSCAN_WORDS] + block_scan_u64(x[WSCAN_ITEMS - 1], tot, total);
    if ((((uintptr_t)cum) & 15) == 0 && m + WSCAN_ITEMS <= n) {
#pragma unroll
        for (int j = 0; j < WSCAN_ITEMS; j += 2)
            *reinterpret_cast<ulonglong2*>(cum + m + j) = make_ulonglong2(before + x[j], before + x[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < WSCAN_ITEMS; ++j)
            if (m + j < n) cum[m + j] = before + x[j];
    }
}

// 8b.  src[k] = the first member m of this shard with cum[m] > p_j - c_lo, j = j0 + k, where
//   p_j = floor((j W + rho) / M) = j q + a + (j s + b) div M      (W = q M + s, rho = a M + b on the host; 0 <= s, b < M)
// in 64-bit arithmetic: j s + b < 2^62 and j q + a <= p_j < W < 2^63.  The shard owns the cumulative range [c_lo, c_lo +
// cum[n - 1]) and is handed only outputs whose positions fall inside it; a position outside (the caller's error) clamps to
// the shard's first / last member, so src is always a valid index.
// One plain binary search per output.  (The positions are monotone in j, so a workgroup can search its first and last
// output first and the others between those two answers only: measured 1.1-1.3 times SLOWER at 1M and 12.5M members — two
// lanes walk the whole depth alone before the others start — and not kept; profiles/r12/resample.txt.)
constexpr int PICK_SRC_BLOCK = FIVEEQ_BLOCK;
__device__ __forceinline__ int64_t resample_upper(const unsigned long long* __restrict__ cum, int64_t lo, int64_t hi,
                                                  const unsigned long long t) {
    while (lo < hi) {                                          // the answer lies in [lo, hi]: cum[hi] > t is taken for granted
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ unsigned long long resample_target(const unsigned long long j, const unsigned long long c_lo,
                                                              const unsigned long long M, const unsigned long long q,
                                                              const unsigned long long a, const unsigned long long s,
                                                              const unsigned long long b) {
    const unsigned long long p = j * q + a + (j * s + b) / M;
    return p > c_lo ? p - c_lo : 0ull;
}
__global__ __launch_bounds__(PICK_SRC_BLOCK) void resample_pick_kernel(const int64_t n, const unsigned long long* __restrict__ cum,
                                                                       const unsigned long long c_lo, const unsigned long long M,
                                                                       const unsigned long long q, const unsigned long long a,
                                                                       const unsigned long long s, const unsigned long long b,
                                                                       const int64_t j0, const int64_t n_out, int* __restrict__ src) {
    const int64_t k = (int64_t)blockIdx.x * PICK_SRC_BLOCK + threadIdx.x;
    if (k < n_out) src[k] = (int)resample_upper(cum, 0, n - 1, resample_target((unsigned long long)(j0 + k), c_lo, M, q, a, s, b));
}

// 8c.  rows_out[r][k] = rows_in[r][src[k]], k < n_out: a lane loads its index once and walks the rows, four loads in flight.
// The writes are coalesced; src is non-decreasing when it comes from 8b, so a wave's reads fall into few cache lines.
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void gather_rows_kernel(const int n_rows, const int64_t n_out, const int64_t ld_in,
                                                                   const T* __restrict__ rows_in, const int64_t ld_out,
                                                                   T* __restrict__ rows_out, const int* __restrict__ src) {
    const int64_t k = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (k >= n_out) return;
    const int m = src[k];
    if (m < 0 || m >= ld_in) return;                           // not an index into a row (the caller's error): nothing is read
    const T* in = rows_in + m;
    T* out = rows_out + k;
    int r = 0;
    for (; r + 4 <= n_rows; r += 4) {
        const T v0 = in[(r + 0) * ld_in], v1 = in[(r + 1) * ld_in], v2 = in[(r + 2) * ld_in], v3 = in[(r + 3) * ld_in];
        out[(r + 0) * ld_out] = v0, out[(r + 1) * ld_out] = v1, out[(r + 2) * ld_out] = v2, out[(r + 3) * ld_out] = v3;
    }
    for (; r < n_rows; ++r) out[r * ld_out] = in[r * ld_in];
}

}  // namespace fiveeq
