// fiveeq_noise.hpp — kernel 14: per-member AR(1) noise rows (noise_rows_kernel), the generator of member_forcing rows.
// Part of fiveeq_device.hpp, which includes it after fiveeq_summary.hpp (lhs_mix64): include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 14 — SHARD-COMPUTABLE AR(1) NOISE.  rows[t - t_begin][m] = xi_t of member M = m0 + m,
//     xi_t = phi_m xi_{t-1} + s_m z_t(M),        s_m = sigma_m sqrt(1 - phi_m^2) (formed by the host in fp64)
// with z_t(M) a counter-based deviate: a pure function of (seed, M, t), so any rank computes exactly its own members and
// steps, and the rows do not depend on the launch shape, ld, how the members are cut into shards (m0) or how [0, n_steps) is
// cut into calls (xi_state carries xi between them).
//
// THE DEVIATE is integer arithmetic only — fiveeqscm_amd.forcing.ar1_noise_rows_host (NumPy) reproduces it bit for bit:
//     key(seed, M, t, j) = lhs_mix64(seed + 0x9e3779b97f4a7c15 (M + 1))  ^  0xd1342543de82ef95 (6 (t + 1) + j + 1)
//     word_j = lhs_mix64(key(seed, M, t, j)),  j = 0 .. 5        (all 64-bit wrapping; t >= -1, so the counter is >= 1)
//     sum    = the twelve 32-bit halves of the six words, added as integers  (< 12 * 2^32 < 2^36: exact)
//     z      = (sum - 6 (2^32 - 1)) * 2^-32                      (a 37-bit integer times a power of two: exact in fp64)
// |z| <= 6 (1 - 2^-32); the mean is 0 and, each half being uniform on [0, 2^32), the variance is 12 (2^64 - 1) / 12 / 2^64 =
// 1 - 2^-64; the excess kurtosis of a sum of twelve uniforms is -1.2 / 12 = -0.1.
//
// THE RECURSION runs in fp64 whatever the row precision, every operation rounded on its own (contraction is off in this file,
// no fma is written — like misfit_update()):  w = s_m * z_t;  xi_t = phi_m * xi_{t-1} + w.  phi and s are read in the
// row precision and widened exactly; fp32 rows are xi_t rounded once on store, xi_state stays fp64.
//
// THE STATIONARY START is the draw at counter t = -1 times sigma_m.  Convention: the call [t_begin, t_end) = [-1, 0) runs that one
// step through the same recursion and stores NO row; with xi_state zeroed and s = sigma it leaves xi_state = sigma_m z_{-1}(M)
// (phi * 0 + w = w exactly).  One member per lane, time sequential inside the lane, each row stored coalesced.
// ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint64_t noise_member_key(uint64_t seed, uint64_t M) {
    return lhs_mix64(seed + 0x9e3779b97f4a7c15ULL * (M + 1ULL));
}
__host__ __device__ __forceinline__ uint64_t noise_key(uint64_t member_key, int t, int j) {
    return member_key ^ (0xd1342543de82ef95ULL * ((uint64_t)((int64_t)t + 1) * 6ULL + (uint64_t)j + 1ULL));
}
__host__ __device__ __forceinline__ double noise_deviate(uint64_t member_key, int t) {
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const uint64_t word = lhs_mix64(noise_key(member_key, t, j));
        sum += (word >> 32) + (word & 0xffffffffULL);
    }
    return (double)((int64_t)sum - 6LL * 0xffffffffLL) * 0x1.0p-32;
}

template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void noise_rows_kernel(const uint64_t seed, const int64_t m0, const int64_t n,
                                                                  const int64_t ld, const int t_begin, const int t_end,
                                                                  const T* __restrict__ phi, const T* __restrict__ s,
                                                                  double* __restrict__ xi_state, T* __restrict__ rows) {
    const int64_t m = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (m >= n) return;
    const uint64_t mk = noise_member_key(seed, (uint64_t)(m0 + m));
    const double ph = (double)phi[m], sm = (double)s[m];
    double xi = xi_state[m];
    for (int t = t_begin; t < t_end; ++t) {
        const double w = sm * noise_deviate(mk, t);
        xi = ph * xi + w;
        if (t >= 0) rows[(int64_t)(t - t_begin) * ld + m] = (T)xi;       // (t = -1: the start call, which stores no row)
    }
    xi_state[m] = xi;
}

}  // namespace fiveeq
