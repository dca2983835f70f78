// fiveeq_stats.hpp — per-wave statistics records of T and the histogram bin rule.
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Per-wave summary statistics of T for one step: (sum, sum of squares, min, max) over the wave's
// active members, in fp64, written to stats[(wave * n_steps + t) * 4 .. +3] (wave-major, so a
// member sub-range of a larger run addresses its records with a plain pointer offset).
// The 64 lanes are folded in registers with DPP moves (row_shr 1/2/4/8 inside each row of 16
// lanes, then row_bcast15 and row_bcast31 across rows: the gfx9 wave-reduce ladder); lanes with no
// DPP source receive the operation's neutral element.  The total lands in lane 63, which writes
// the 32-byte record.  (A first version used LDS fp64 atomics on one address per wave: 64-way
// serialised, +54 % on the fused kernel; the DPP ladder costs a few hundred cycles per wave-step.)
// One record per wave and step (0.5 B per member-step) replaces the T trajectory when only
// moments are wanted.
// ---------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move_f64(const double v, const double neutral) {
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(neutral), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(neutral), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
struct OpAdd { static __device__ __forceinline__ double f(double a, double b) { return a + b; } };
struct OpMin { static __device__ __forceinline__ double f(double a, double b) { return fmin(a, b); } };
struct OpMax { static __device__ __forceinline__ double f(double a, double b) { return fmax(a, b); } };
template <typename Op>
__device__ __forceinline__ double wave_reduce_to_lane63(double v, const double neutral) {
    v = Op::f(v, dpp_move_f64<0x111, 0xf>(v, neutral));   // row_shr:1
    v = Op::f(v, dpp_move_f64<0x112, 0xf>(v, neutral));   // row_shr:2
    v = Op::f(v, dpp_move_f64<0x114, 0xf>(v, neutral));   // row_shr:4
    v = Op::f(v, dpp_move_f64<0x118, 0xf>(v, neutral));   // row_shr:8   -> lane 15 of each row = row total
    v = Op::f(v, dpp_move_f64<0x142, 0xa>(v, neutral));   // row_bcast:15 into rows 1 and 3
    v = Op::f(v, dpp_move_f64<0x143, 0xc>(v, neutral));   // row_bcast:31 into rows 2 and 3 -> lane 63 = total
    return v;
}

template <typename T>
__device__ __forceinline__ void wave_stats(const bool active, const T Tn, double* __restrict__ out) {
    const double inf = __builtin_inf();
    const double v = (double)Tn;
    const double s1 = wave_reduce_to_lane63<OpAdd>(active ? v : 0.0, 0.0);
    const double s2 = wave_reduce_to_lane63<OpAdd>(active ? v * v : 0.0, 0.0);
    // fmin / fmax drop a NaN operand but keep NaN when BOTH are: a NaN member enters the extrema as the neutral element, so a
    // record whose members are all NaN has min = +inf, max = -inf here as in wave_stats_flush() below
    const bool ordered = active && v == v;
    const double mn = wave_reduce_to_lane63<OpMin>(ordered ? v : inf, inf);
    const double mx = wave_reduce_to_lane63<OpMax>(ordered ? v : -inf, -inf);
    if ((threadIdx.x & 63) == 63) {
        out[0] = s1;
        out[1] = s2;
        out[2] = mn;
        out[3] = mx;
    }
}

// Packed lanes (two members per lane): the wave covers 128 consecutive members, lanes 0..31 the first 64 and lanes
// 32..63 the second 64, so the ladder stops one step early (no row_bcast:31) and lane 31 / lane 63 write the two
// 64-member records — the record layout [ceil(N/64)][n_steps][4] is the same for every kernel shape.
template <typename Op>
__device__ __forceinline__ double wave_reduce_to_lanes_31_63(double v, const double neutral) {
    v = Op::f(v, dpp_move_f64<0x111, 0xf>(v, neutral));   // row_shr:1
    v = Op::f(v, dpp_move_f64<0x112, 0xf>(v, neutral));   // row_shr:2
    v = Op::f(v, dpp_move_f64<0x114, 0xf>(v, neutral));   // row_shr:4
    v = Op::f(v, dpp_move_f64<0x118, 0xf>(v, neutral));   // row_shr:8
    v = Op::f(v, dpp_move_f64<0x142, 0xa>(v, neutral));   // row_bcast:15 into rows 1 and 3 -> lanes 31, 63 = half totals
    return v;
}
__device__ __forceinline__ void wave_stats(const bool a0, const bool a1, const float2v Tn, double* __restrict__ out_lo,
                                           double* __restrict__ out_hi /* nullptr: the wave has <= 64 members */) {
    const double inf = __builtin_inf();
    const double x = (double)Tn.x, y = (double)Tn.y;
    const double s1 = wave_reduce_to_lanes_31_63<OpAdd>((a0 ? x : 0.0) + (a1 ? y : 0.0), 0.0);
    const double s2 = wave_reduce_to_lanes_31_63<OpAdd>((a0 ? x * x : 0.0) + (a1 ? y * y : 0.0), 0.0);
    const bool o0 = a0 && x == x, o1 = a1 && y == y;      // (a NaN member: the neutral element, as above)
    const double mn = wave_reduce_to_lanes_31_63<OpMin>(fmin(o0 ? x : inf, o1 ? y : inf), inf);
    const double mx = wave_reduce_to_lanes_31_63<OpMax>(fmax(o0 ? x : -inf, o1 ? y : -inf), -inf);
    const int lane = threadIdx.x & 63;
    double* const out = lane == 31 ? out_lo : (lane == 63 ? out_hi : nullptr);
    if (out != nullptr) {
        out[0] = s1;
        out[1] = s2;
        out[2] = mn;
        out[3] = mx;
    }
}

// ---------------------------------------------------------------------------------
// The time-fused kernel produces one T per lane EVERY step, so it batches the statistics instead
// of running the DPP ladder per step (which costs +20 % fp64 / +70 % fp32 there): each wave parks
// its T values in a wave-private LDS tile [STAT_STEPS][64 (+1 pad)], and every STAT_STEPS steps
// the tile is reduced TRANSPOSED: lane l owns step j = l % 8 and the eighth p = l / 8 of that
// step's 64 members, folds its 8 values serially in fp64, and the 8 partials per step are combined
// with three xor-shuffles (8, 16, 32).  Row stride 65 elements makes both the row writes and the
// strided reads bank-conflict-free (bank = j + 8 p + i mod 32).  A wave's LDS operations complete
// in program order, so only compiler (wavefront-scope) fences are needed, no barrier.
// ---------------------------------------------------------------------------------
constexpr int STAT_STEPS = 8;
constexpr int STAT_ROW = 65;
// min / max as ONE instruction.  fmin()/fmax() on a value the compiler cannot prove canonical get a v_max(x, x) in front
// (sNaN quieting) — 56 of them in the fused kernel's statistics flush; the values here come out of the model's FMAs.  A NaN
// operand is ignored by v_min / v_max like by fmin / fmax (IEEE mode), so the record of a wave with a NaN member is the same.
// The folds START from the neutral element (+inf / -inf), like the partial-wave path below: a record whose members are ALL NaN
// then has min = +inf, max = -inf by every route (started from the first value it had NaN extrema; wave_stats() above feeds
// its ladder the neutral element for a NaN member to the same end).
__device__ __forceinline__ float fe_min_raw(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float fe_max_raw(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double fe_min_raw(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double fe_max_raw(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <typename T>
__device__ __forceinline__ void wave_stats_flush(const T* tile /* [STAT_STEPS][STAT_ROW] */, const int count,
                                                 const int n_valid, double* __restrict__ out, const int64_t stride) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int lane = threadIdx.x & 63;
    const int j = lane & (STAT_STEPS - 1), p = lane >> 3;
    const double inf = __builtin_inf();
    double s1 = 0.0, s2 = 0.0, mn, mx;
    if (n_valid >= 64) {                                   // a full wave (all but the ensemble's last): no per-value tests, and
        T lo_v = (T)inf, hi_v = (T)-inf;                   // min / max in the values' own precision (exact), converted once
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const T t = tile[j * STAT_ROW + p * 8 + i];
            const double v = (double)t;
            s1 += v;
            s2 = __builtin_fma(v, v, s2);
            lo_v = fe_min_raw(lo_v, t);
            hi_v = fe_max_raw(hi_v, t);
        }
        mn = (double)lo_v;
        mx = (double)hi_v;
    } else {
        mn = inf;
        mx = -inf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = p * 8 + i;
            const double v = (double)tile[j * STAT_ROW + idx];
            if (idx < n_valid) {
                s1 += v;
                s2 = __builtin_fma(v, v, s2);
                mn = fmin(mn, v);
                mx = fmax(mx, v);
            }
        }
    }
#pragma unroll
    for (int sh = 8; sh < 64; sh <<= 1) {
        s1 += __shfl_xor(s1, sh);
        s2 += __shfl_xor(s2, sh);
        mn = fmin(mn, __shfl_xor(mn, sh));
        mx = fmax(mx, __shfl_xor(mx, sh));
    }
    if (p == 0 && j < count) {
        double* o = out + (int64_t)j * stride;
        o[0] = s1;
        o[1] = s2;
        o[2] = mn;
        o[3] = mx;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Packed lanes: the tile row holds the wave's 64 float2 values (128 members); lane l owns step j = l % 8 and lanes
// 8p .. 8p+7 of it (members 16p .. 16p+15), p = l / 8; p < 4 is the wave's first 64-member record, p >= 4 its second.
__device__ __forceinline__ void wave_stats_flush(const float2v* tile /* [STAT_STEPS][STAT_ROW] */, const int count,
                                                 const int n_valid /* members of this wave, <= 128 */,
                                                 double* __restrict__ out_lo, double* __restrict__ out_hi, const int64_t stride) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const int lane = threadIdx.x & 63;
    const int j = lane & (STAT_STEPS - 1), p = lane >> 3;
    const double inf = __builtin_inf();
    double s1 = 0.0, s2 = 0.0, mn, mx;
    if (n_valid >= 128) {                                  // a full wave: same order of the sums as below, no per-value tests
        float lo_v = (float)inf, hi_v = (float)-inf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float2v v2 = tile[j * STAT_ROW + p * 8 + i];
            const double x = (double)v2.x, y = (double)v2.y;
            s1 += x;
            s2 = __builtin_fma(x, x, s2);
            s1 += y;
            s2 = __builtin_fma(y, y, s2);
            lo_v = fe_min_raw(fe_min_raw(lo_v, v2.x), v2.y);
            hi_v = fe_max_raw(fe_max_raw(hi_v, v2.x), v2.y);
        }
        mn = (double)lo_v;
        mx = (double)hi_v;
    } else {
        mn = inf;
        mx = -inf;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = p * 8 + i;
            const float2v v2 = tile[j * STAT_ROW + idx];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double v = (double)(c == 0 ? v2.x : v2.y);
                if (2 * idx + c < n_valid) {
                    s1 += v;
                    s2 = __builtin_fma(v, v, s2);
                    mn = fmin(mn, v);
                    mx = fmax(mx, v);
                }
            }
        }
    }
#pragma unroll
    for (int sh = 8; sh < 32; sh <<= 1) {
        s1 += __shfl_xor(s1, sh);
        s2 += __shfl_xor(s2, sh);
        mn = fmin(mn, __shfl_xor(mn, sh));
        mx = fmax(mx, __shfl_xor(mx, sh));
    }
    double* const out = p == 0 ? out_lo : (p == 4 ? out_hi : nullptr);
    if (out != nullptr && j < count) {
        double* o = out + (int64_t)j * stride;
        o[0] = s1;
        o[1] = s2;
        o[2] = mn;
        o[3] = mx;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

constexpr unsigned short BIN_NAN = 0xFFFFu;
// THE BIN RULE — one definition per row precision, used by every kernel that bins a value (the in-loop forms of the step /
// fused kernels, hist_rows_kernel on stored rows, the summary's selection pass), so that "the same counts bit for
// bit" between them is a property of this struct.  (lo, inv_w = n_bins / (hi - lo), n_bins) come in as fp64:
//   fp64 rows:  pos = (v - lo) * inv_w                      in fp64
//   fp32 rows:  pos = fma(v, (float)inv_w, (float)(-lo * inv_w))    in fp32 — one (packed) FMA where the fp64 form cost ~10
//               quarter-rate instructions per lane in kernels whose ceiling is VALU issue (round 4).  Against the fp64 form a
//               member changes bin only within ~2^-23 max(|lo|, |hi|) inv_w of a bin edge (the rounding of scale and offset,
//               in bins): 2^-12 bin for a range that starts near zero (|lo| inv_w ~ n_bins <= 4096, e.g. temperature
//               anomalies), more for a range far from zero in units of its own width (lo = 280, hi = 295, 4096 bins: 0.01 bin)
//               — rows in such absolute units want a range shifted to the anomaly, or fp64 rows
//   bin = pos clamped to [0, n_bins - 1] and truncated; outliers land in the edge bins; a NaN has no bin (BIN_NAN).
// Both forms are monotone in v (rounding is), which the summary's selection relies on: members of a lower bin are <= members
// of a higher one.
// The rule's three constants are plain values (an object with methods made the compiler park it in LDS — promote-alloca — in
// the one-wave step kernel: 768 B of LDS, -1 wave/SIMD, +17 % on the per-step + bins form; measured, profiles/r04/ab_variants.txt).
template <typename S> struct HistRule;
template <> struct HistRule<double> {
    double lo, inv_w, top;
};
template <> struct HistRule<float> {
    float scale, offset, top;
};
__device__ __forceinline__ HistRule<double> make_rule(const double, const double lo, const double inv_w, const int n_bins) {
    return HistRule<double>{lo, inv_w, (double)(n_bins - 1)};
}
__device__ __forceinline__ HistRule<float> make_rule(const float, const double lo, const double inv_w, const int n_bins) {
    // scale and offset are kept FINITE (a range narrower than ~1e-35 would overflow them): pos is then never inf - inf, so a
    // finite or infinite member always clamps into [0, n_bins - 1] and no index can leave the histogram
    const double big = 3.0e38;
    const float scale = (float)fmin(fmax(inv_w, -big), big), offset = (float)fmin(fmax(-lo * inv_w, -big), big);
    return HistRule<float>{scale, offset, (float)(n_bins - 1)};
}
__device__ __forceinline__ unsigned int hist_bin(const HistRule<double> r, const double v) {
    const double pos = (v - r.lo) * r.inv_w;
    const unsigned int b = (unsigned int)(int)fmin(fmax(pos, 0.0), r.top);          // NaN pos -> 0 (fmax / fmin drop the NaN)
    return v == v ? b : (unsigned int)BIN_NAN;
}
__device__ __forceinline__ unsigned int hist_bin_of_pos(const HistRule<float> r, const float pos, const float v) {
    const unsigned int b = (unsigned int)(int)__builtin_amdgcn_fmed3f(pos, 0.0f, r.top);       // v_med3_f32: the clamp in one op
    return v == v ? b : (unsigned int)BIN_NAN;
}
// (rounds 2-3 binned fp32 rows by the fp64 formula — convert, subtract, multiply, clamp, truncate: ~10 quarter-rate instructions
// per lane; the A/B against this one fp32 FMA is profiles/r04/ab_variants.txt, the knob is gone)
__device__ __forceinline__ unsigned int hist_bin(const HistRule<float> r, const float v) {
    return hist_bin_of_pos(r, __builtin_fmaf(v, r.scale, r.offset), v);
}
// two members of a packed lane: one v_pk_fma_f32; returns bin(v.x) | bin(v.y) << 16
__device__ __forceinline__ unsigned int hist_bin2(const HistRule<float> r, const float2v v) {
    const float2v pos = __builtin_elementwise_fma(v, (float2v)r.scale, (float2v)r.offset);
    return hist_bin_of_pos(r, pos.x, v.x) | (hist_bin_of_pos(r, pos.y, v.y) << 16);
}
// The histogram bin of T at o, the lane's slot in the ring row of its step (bin_ring [ring_rows][ld], row t mod ring_rows:
// a scalar row offset), 2 bytes per member.  A packed lane stores both members' bins with one 4-byte store.
template <typename T, typename V>
__device__ __forceinline__ void store_bin(unsigned short* o, const HistRule<T> rule, const V Tn, const bool full) {
    if constexpr (Lane<V>::W == 1) {
        *o = (unsigned short)hist_bin(rule, Tn);
    } else {
        const unsigned int b01 = hist_bin2(rule, Tn);
        if (full) *reinterpret_cast<unsigned int*>(o) = b01;
        else *o = (unsigned short)(b01 & 0xffffu);
    }
}

}  // namespace fiveeq
