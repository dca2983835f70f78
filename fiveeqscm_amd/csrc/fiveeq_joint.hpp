// fiveeq_joint.hpp — kernels 10a / 10b: JOINT STATISTICS of per-member rows (include/fiveeq.h, "JOINT STATISTICS").
// Part of fiveeq_device.hpp, which includes it after fiveeq_metrics.hpp: include that header, not this one.
//
// Two passes over x rows [n_x][ld_x] and y rows [n_y][ld_y] of the same members under the integer weights of the weighted
// summary (uint64, at most 2^32 each; a member of weight 0 does not exist, whatever its values):
//   10a  joint_moments_kernel + folds   co[i][j] = sum fe_fma(dx_i, wd dy_j, .), the margins (sum wd d, sum (wd d) d) of every row,
//                                        sum w / count / flags, the weight of the NaN members per row
//   10b  cond_sums_kernel + folds       per x row the members fall into bins between edges; per (x row, bin, y row) sum wd dy_j,
//                                        per (x row, bin) the integer weight, per x row the weight of its NaN members
// One workgroup = one chunk of JOINT_CHUNK members x one tile of rows: (a) JOINT_TX x rows by JOINT_TY y rows, (b) one x row,
// COND_TB bins and COND_TY y rows.  Every fp64 sum is taken in ONE order: a lane takes the members m0 + lane WN + j + k STEP in
// that order (the same in the 16-byte and the element load path), the 64 lanes of a wave are added by an xor-shuffle tree, the
// waves in wave order, the chunks by the fold (lane-strided, then the same tree).  That order does not know which tile a pair
// sits in, so the tiling cannot change a bit, and there is no floating-point atomic anywhere: the bins of (b) are registers
// under compile-time indices.  Integer sums (weights, counts) use LDS integer atomics where that is simpler: exact in any order.
// partial [word][chunk]: every word is written by exactly one tile, so the workspace needs no initialisation.
#pragma once

namespace fiveeq {

constexpr int JOINT_MAX_ROWS = 32;                             // fiveeq_max_joint_rows()
constexpr int JOINT_MAX_BINS = 32;                             // fiveeq_max_cond_bins()
constexpr int JOINT_TX = 4, JOINT_TY = 4;                      // (a): x rows by y rows per workgroup — 16 co-moments a lane
constexpr int COND_TB = 16, COND_TY = 4;                       // (b): bins by y rows per workgroup — 64 bin sums a lane
constexpr int JOINT_CHUNK = 4096;                              // members per chunk: a multiple of 4 * FIVEEQ_BLOCK, and of nothing else
static_assert(JOINT_CHUNK % (4 * FIVEEQ_BLOCK) == 0, "a chunk is whole 16-byte loads of every lane, fp32 and fp64");

// Every member of [m0, m1) with weight > 0, one call f(values of the NR rows widened to fp64, weight) per lane and member, in
// the lane's member order.  wide: 16-byte loads of the rows and the weights where all of a lane's WN members exist; m0 is a
// multiple of JOINT_CHUNK, which keeps every lane's address aligned.
template <typename T, int NR, typename F>
__device__ __forceinline__ void joint_for_members(const T* const (&p)[NR], const unsigned long long* __restrict__ w, const int64_t m0,
                                                  const int64_t m1, const bool wide, F&& f) {
    using WV = typename Wide<T>::V;
    constexpr int WN = Wide<T>::N;
    constexpr int64_t STEP = (int64_t)WN * FIVEEQ_BLOCK;
    for (int64_t m = m0 + (int64_t)threadIdx.x * WN; m < m1; m += STEP) {
        T v[NR][WN];
        unsigned long long ws[WN];
        if (wide && m + WN <= m1) {
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const WV a = *reinterpret_cast<const WV*>(p[r] + m);
#pragma unroll
                for (int j = 0; j < WN; ++j) v[r][j] = wide_get(a, j);
            }
#pragma unroll
            for (int j = 0; j < WN; j += 2) {
                const ulonglong2 q = *reinterpret_cast<const ulonglong2*>(w + m + j);
                ws[j] = q.x, ws[j + 1] = q.y;
            }
        } else {                                                  // unaligned rows, and the ragged end of the last chunk
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const bool have = m + j < m1;
                ws[j] = have ? w[m + j] : 0ull;
#pragma unroll
                for (int r = 0; r < NR; ++r) v[r][j] = have ? p[r][m + j] : T(0);
            }
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            if (ws[j] != 0ull) {
                double d[NR];
#pragma unroll
                for (int r = 0; r < NR; ++r) d[r] = (double)v[r][j];
                f(d, ws[j]);
            }
        }
    }
}
template <typename T>
__device__ __forceinline__ bool joint_wide(const T* x, const int64_t ld_x, const T* y, const int64_t ld_y, const unsigned long long* w) {
    return ((((uintptr_t)x) | ((uintptr_t)(ld_x * sizeof(T))) | ((uintptr_t)y) | ((uintptr_t)(ld_y * sizeof(T))) | ((uintptr_t)w)) & 15) == 0;
}

// the workgroup's sum of one word per lane, in the fixed order: xor-shuffle tree within the wave, then the waves in wave order.
// red [FIVEEQ_BLOCK / 64][NW] is the workgroup's LDS; word k of it belongs to this value.  The caller synchronises, then
// block_word() of thread k returns the sum.
__device__ __forceinline__ void wave_word(double v, double* red, const int nw, const int k) {
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) v += __shfl_xor(v, sh);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * nw + k] = v;
}
__device__ __forceinline__ void wave_word(unsigned long long v, double* red, const int nw, const int k) {
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) reinterpret_cast<unsigned long long*>(red)[(threadIdx.x >> 6) * nw + k] = v;
}
__device__ __forceinline__ double block_word_f64(const double* red, const int nw, const int k) {
    double t = red[k];
#pragma unroll
    for (int wv = 1; wv < FIVEEQ_BLOCK / 64; ++wv) t += red[wv * nw + k];
    return t;
}
__device__ __forceinline__ unsigned long long block_word_u64(const double* red, const int nw, const int k) {
    const unsigned long long* u = reinterpret_cast<const unsigned long long*>(red);
    unsigned long long t = u[k];
#pragma unroll
    for (int wv = 1; wv < FIVEEQ_BLOCK / 64; ++wv) t += u[wv * nw + k];
    return t;
}

// 10a.  Words of a chunk's record (partial[word * chunks + chunk], 8 bytes each), with R = n_x + n_y:
//   [i n_y + j] co   |   n_x n_y + [2 r, 2 r + 1] margins of row r (x rows, then y rows)   |   n_x n_y + 2 R + [r] NaN weight of row r
//   |   n_x n_y + 3 R + [0, 1, 2] sum w, count of w > 0, WFLAG_RANGE
// The tile (tx, ty) owns the co words of its pairs; the x margins belong to the tiles ty == 0, the y margins to tx == 0, the
// last three words to tile (0, 0).  A tile at the edge reads its last row again in place of the rows that do not exist and
// stores nothing for them.
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void joint_moments_kernel(const int64_t n, const int n_x, const int64_t ld_x,
                                                                     const T* __restrict__ x, const int n_y, const int64_t ld_y,
                                                                     const T* __restrict__ y,
                                                                     const unsigned long long* __restrict__ weights,
                                                                     const double* __restrict__ pivots, double* __restrict__ partial) {
    constexpr int TX = JOINT_TX, TY = JOINT_TY, TR = TX + TY, NW = TX * TY + 3 * TR + 3;
    __shared__ double red[(FIVEEQ_BLOCK / 64) * NW];
    const int tiles_y = (n_y + TY - 1) / TY;
    const int tx = (int)blockIdx.y / tiles_y, ty = (int)blockIdx.y % tiles_y;
    const int i0 = tx * TX, j0 = ty * TY;
    const bool own_x = ty == 0, own_y = tx == 0;              // workgroup-uniform
    const T* p[TR];
    double c[TR];
#pragma unroll
    for (int r = 0; r < TX; ++r) {
        const int i = min(i0 + r, n_x - 1);
        p[r] = x + (int64_t)i * ld_x;
        c[r] = pivots[i];
    }
#pragma unroll
    for (int r = 0; r < TY; ++r) {
        const int j = min(j0 + r, n_y - 1);
        p[TX + r] = y + (int64_t)j * ld_y;
        c[TX + r] = pivots[n_x + j];
    }
    const int64_t m0 = (int64_t)blockIdx.x * JOINT_CHUNK;
    const int64_t m1 = min(m0 + (int64_t)JOINT_CHUNK, n);

    double co[TX][TY], s1[TR], s2[TR];
    unsigned long long nanw[TR], sw = 0ull, cnt = 0ull, flags = 0ull;
#pragma unroll
    for (int r = 0; r < TR; ++r) s1[r] = 0.0, s2[r] = 0.0, nanw[r] = 0ull;
#pragma unroll
    for (int i = 0; i < TX; ++i)
#pragma unroll
        for (int j = 0; j < TY; ++j) co[i][j] = 0.0;

    joint_for_members<T, TR>(p, weights, m0, m1, joint_wide(x, ld_x, y, ld_y, weights), [&](const double (&v)[TR], const unsigned long long w) {
        const double wd = (double)w;                          // exact: w <= 2^32 (a larger one raises WFLAG_RANGE)
        double d[TR], pw[TR];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            d[r] = v[r] - c[r];
            pw[r] = wd * d[r];
        }
#pragma unroll
        for (int i = 0; i < TX; ++i)
#pragma unroll
            for (int j = 0; j < TY; ++j) co[i][j] = fe_fma(d[i], pw[TX + j], co[i][j]);
        if (own_x) {
#pragma unroll
            for (int r = 0; r < TX; ++r) {
                s1[r] = s1[r] + pw[r];
                s2[r] = fe_fma(pw[r], d[r], s2[r]);
                nanw[r] += v[r] != v[r] ? w : 0ull;
            }
        }
        if (own_y) {
#pragma unroll
            for (int r = TX; r < TR; ++r) {
                s1[r] = s1[r] + pw[r];
                s2[r] = fe_fma(pw[r], d[r], s2[r]);
                nanw[r] += v[r] != v[r] ? w : 0ull;
            }
        }
        sw += w;
        cnt += 1ull;
        flags |= w > WEIGHT_ONE ? WFLAG_RANGE : 0ull;
    });

    // the record of this chunk and tile: word k of red, then thread k folds the waves and stores the word if the tile owns it
#pragma unroll
    for (int i = 0; i < TX; ++i)
#pragma unroll
        for (int j = 0; j < TY; ++j) wave_word(co[i][j], red, NW, i * TY + j);
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        wave_word(s1[r], red, NW, TX * TY + 2 * r);
        wave_word(s2[r], red, NW, TX * TY + 2 * r + 1);
        wave_word(nanw[r], red, NW, TX * TY + 2 * TR + r);
    }
    wave_word(sw, red, NW, TX * TY + 3 * TR);
    wave_word(cnt, red, NW, TX * TY + 3 * TR + 1);
    wave_word(flags, red, NW, TX * TY + 3 * TR + 2);          // the number of lanes that saw one: non-zero is the flag
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= NW) return;
    const int64_t chunks = gridDim.x, R = n_x + n_y, base = (int64_t)n_x * n_y;
    unsigned long long* const upart = reinterpret_cast<unsigned long long*>(partial);
    if (k < TX * TY) {
        const int i = i0 + k / TY, j = j0 + k % TY;
        if (i < n_x && j < n_y) partial[((int64_t)i * n_y + j) * chunks + blockIdx.x] = block_word_f64(red, NW, k);
    } else if (k < TX * TY + 3 * TR) {
        const bool is_nan = k >= TX * TY + 2 * TR;
        const int r = is_nan ? k - (TX * TY + 2 * TR) : (k - TX * TY) / 2;     // the tile's row: x rows, then y rows
        const bool is_x = r < TX;
        const int row = is_x ? i0 + r : j0 + (r - TX);
        if (is_x ? (own_x && row < n_x) : (own_y && row < n_y)) {
            const int64_t g = is_x ? row : n_x + row;
            if (is_nan) upart[(base + 2 * R + g) * chunks + blockIdx.x] = block_word_u64(red, NW, k);
            else partial[(base + 2 * g + ((k - TX * TY) & 1)) * chunks + blockIdx.x] = block_word_f64(red, NW, k);
        }
    } else if (own_x && own_y) {
        const int q = k - (TX * TY + 3 * TR);
        const unsigned long long t = block_word_u64(red, NW, k);
        upart[(base + 3 * R + q) * chunks + blockIdx.x] = q == 2 ? (t ? WFLAG_RANGE : 0ull) : t;
    }
}

// the folds: out[word] = the chunk records of the word added in a fixed order (one wave per word: lane-strided, then the tree)
__global__ __launch_bounds__(64) void joint_fold_f64_kernel(const int64_t chunks, const double* __restrict__ partial, double* __restrict__ out) {
    const double* p = partial + (int64_t)blockIdx.x * chunks;
    double a = 0.0;
    for (int64_t ch = threadIdx.x; ch < chunks; ch += 64) a += p[ch];
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) a += __shfl_xor(a, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}
__global__ __launch_bounds__(64) void joint_fold_u64_kernel(const int64_t chunks, const unsigned long long* __restrict__ partial,
                                                            unsigned long long* __restrict__ out) {
    const unsigned long long* p = partial + (int64_t)blockIdx.x * chunks;
    unsigned long long a = 0ull;
    for (int64_t ch = threadIdx.x; ch < chunks; ch += 64) a += p[ch];
    a = wave_sum_u64(a);
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}
// info[4] = (sum w, count of w > 0, flags, 0): the two sums, the range flag of any chunk, and WFLAG_NAN when any of the
// n_rows rows has NaN weight in any chunk.  nanpart: the n_rows * chunks NaN-weight words, tail: the three info words.
__global__ __launch_bounds__(64) void joint_fold_info_kernel(const int64_t chunks, const int64_t n_rows,
                                                             const unsigned long long* __restrict__ nanpart,
                                                             const unsigned long long* __restrict__ tail,
                                                             unsigned long long* __restrict__ info) {
    unsigned long long sw = 0ull, cnt = 0ull, fl = 0ull;
    for (int64_t ch = threadIdx.x; ch < chunks; ch += 64) {
        sw += tail[ch];
        cnt += tail[chunks + ch];
        fl |= tail[2 * chunks + ch];
    }
    for (int64_t k = threadIdx.x; k < n_rows * chunks; k += 64) fl |= nanpart[k] ? WFLAG_NAN : 0ull;
    sw = wave_sum_u64(sw);
    cnt = wave_sum_u64(cnt);
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) fl |= __shfl_xor(fl, sh);
    if (threadIdx.x == 0) info[0] = sw, info[1] = cnt, info[2] = fl, info[3] = 0ull;
}

// 10b.  One workgroup = one chunk x (x row i, group g of COND_TB bins, tile ty of COND_TY y rows).  THE BIN of a member under x
// row i: b = #{k : edges[i][k] < x_i} — a value equal to an edge belongs to the lower bin; the edges of the row (non-decreasing)
// sit in LDS, padded with +inf to 32, and the count is a five-step lower bound.  A NaN x_i has no bin: its weight goes to xnan[i].  The lane's bin sums
// acc[bin][y row] are registers (every index a constant after unrolling); binw and xnan are LDS integer sums.
// Words of a chunk's record: [(i n_bins + b) n_y + j] sums | n_x n_bins n_y + [i n_bins + b] binw | n_x n_bins (n_y + 1) + [i] xnan;
// binw belongs to the tiles ty == 0, xnan to (g, ty) == (0, 0).
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void cond_sums_kernel(const int64_t n, const int n_x, const int64_t ld_x, const T* __restrict__ x,
                                                                 const int n_y, const int64_t ld_y, const T* __restrict__ y,
                                                                 const unsigned long long* __restrict__ weights, const int n_bins,
                                                                 const double* __restrict__ edges, const double* __restrict__ pivots,
                                                                 double* __restrict__ partial) {
    constexpr int TB = COND_TB, TY = COND_TY, NW = TB * TY;
    __shared__ double red[(FIVEEQ_BLOCK / 64) * NW];
    __shared__ unsigned long long h[TB + 1];                  // the weight per bin of the group, then the NaN weight
    __shared__ double ed[JOINT_MAX_BINS];                     // the row's edges, +inf from n_bins - 1 on: never below a value
    const int groups = (n_bins + TB - 1) / TB, tiles_y = (n_y + TY - 1) / TY;
    const int ty = (int)blockIdx.y % tiles_y, g = ((int)blockIdx.y / tiles_y) % groups, i = (int)blockIdx.y / (tiles_y * groups);
    const int b0 = g * TB, j0 = ty * TY;
    if (threadIdx.x <= TB) h[threadIdx.x] = 0ull;
    if (threadIdx.x < JOINT_MAX_BINS) ed[threadIdx.x] = (int)threadIdx.x < n_bins - 1 ? edges[(int64_t)i * (n_bins - 1) + threadIdx.x] : __builtin_inf();
    __syncthreads();
    const T* p[1 + TY];
    double c[TY];
    p[0] = x + (int64_t)i * ld_x;
#pragma unroll
    for (int r = 0; r < TY; ++r) {
        const int j = min(j0 + r, n_y - 1);
        p[1 + r] = y + (int64_t)j * ld_y;
        c[r] = pivots[j];
    }
    const int64_t m0 = (int64_t)blockIdx.x * JOINT_CHUNK;
    const int64_t m1 = min(m0 + (int64_t)JOINT_CHUNK, n);
    const bool own_w = ty == 0;

    double acc[TB][TY];
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
        for (int j = 0; j < TY; ++j) acc[b][j] = 0.0;

    joint_for_members<T, 1 + TY>(p, weights, m0, m1, joint_wide(x, ld_x, y, ld_y, weights), [&](const double (&v)[1 + TY], const unsigned long long w) {
        const double xv = v[0];
        if (xv != xv) {
            if (own_w && g == 0) atomicAdd(&h[TB], w);
            return;
        }
        int b = 0;                                            // the number of edges below xv: the lower bound in the sorted row
#pragma unroll
        for (int step = JOINT_MAX_BINS / 2; step >= 1; step >>= 1) b += ed[b + step - 1] < xv ? step : 0;
        const int lb = b - b0;
        if (lb < 0 || lb >= TB) return;
        const double wd = (double)w;
        double t[TY];
#pragma unroll
        for (int j = 0; j < TY; ++j) t[j] = wd * (v[1 + j] - c[j]);
#pragma unroll
        for (int bb = 0; bb < TB; ++bb) {                     // a select per bin, not an index: the sums stay registers
#pragma unroll
            for (int j = 0; j < TY; ++j) acc[bb][j] = acc[bb][j] + (lb == bb ? t[j] : 0.0);
        }
        if (own_w) atomicAdd(&h[lb], w);
    });

#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
        for (int j = 0; j < TY; ++j) wave_word(acc[b][j], red, NW, b * TY + j);
    __syncthreads();
    const int k = threadIdx.x;
    const int64_t chunks = gridDim.x;
    unsigned long long* const upart = reinterpret_cast<unsigned long long*>(partial);
    if (k < NW) {
        const int b = b0 + k / TY, j = j0 + k % TY;
        if (b < n_bins && j < n_y) partial[(((int64_t)i * n_bins + b) * n_y + j) * chunks + blockIdx.x] = block_word_f64(red, NW, k);
    }
    if (own_w && k < TB && b0 + k < n_bins)
        upart[((int64_t)n_x * n_bins * n_y + (int64_t)i * n_bins + b0 + k) * chunks + blockIdx.x] = h[k];
    if (own_w && g == 0 && k == TB) upart[((int64_t)n_x * n_bins * (n_y + 1) + i) * chunks + blockIdx.x] = h[TB];
}

}  // namespace fiveeq
