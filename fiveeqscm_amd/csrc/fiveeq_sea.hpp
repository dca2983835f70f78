// fiveeq_sea.hpp — kernel 19: per-member sea-level rise rows from stored warming and heat uptake (sea_level_rows_kernel).
// Part of fiveeq_device.hpp, which includes it after fiveeq_aerosol.hpp (fe_expm1_neg: fiveeq_math.hpp): include that header,
// not this one.
#pragma once

#ifndef FIVEEQ_SEA_MAX
#define FIVEEQ_SEA_MAX 6          // components per member: em1, a, b, T0, cap, S per component in registers, 6 * 6 fp64 = 72 VGPRs per lane
#endif
#ifndef FIVEEQ_SEA_UNROLL
#define FIVEEQ_SEA_UNROLL 4       // rows whose T (and H) loads the row loop issues before it uses the first
#endif

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 19 — SEA-LEVEL ROWS.  Each member carries J <= FIVEEQ_SEA_MAX contributions to global-mean sea-level rise (thermal
// expansion, glaciers, the ice sheets' surface balance and discharge, land water, ...), each with the member's OWN parameters
// (tau, a, b, T0, cap), driven by the member's stored warming T.  A component is of kind
//     relax   dS/dt = (Seq(T) - S) / tau    (Mengel et al. 2016), advanced exactly over one step with the row's T held, or
//     rate    dS/dt = Seq(T)                (the semi-empirical form of Rahmstorf 2007),
// with  Seq(T) = (a + b x) x,  x = T - T0,  capped from above at cap (finite ice; +inf: no cap).  An optional thermosteric term
// adds eta[m] H[t][m], H the heat-uptake rows of the forcing-rows pass.
//
// THE ARITHMETIC is fp64 whatever the precision of the T rows (T is widened exactly), every operation rounded on its own
// (contraction is off in this file, no fma is written — like fiveeq_minor.hpp).
// Once per call, for each relax component j of the lane's member:
//     x     = -dt / tau_j          (IEEE division)
//     em1_j = fe_expm1_neg(x)      (the pinned primitive of fiveeq_math.hpp: what fiveeq_math_probe_f64(op = 0) returns for x)
// Per scenario s and row t, with Tt = (double)T[s][t][m], for j ascending:
//     x = Tt - T0_j;  p = b_j * x;  c = a_j + p;  e = c * x;  if (e > cap_j) e = cap_j;     // a NaN e stays NaN
//     relax:  v = S_j - e;  w = em1_j * v;  S_j = S_j + w
//     rate:   w = dt * e;   S_j = S_j + w
// then
//     acc = heat ? eta * H[s][t][m] : 0.0;     for j ascending: acc = acc + S_j;     total[s][t][m] = acc
//     comps[s][t][j][m] = S_j                  (when component rows are asked for)
// and after the last row S is written back.
//
// CONSEQUENCES.  The bits depend on (T, H, eta, the parameters, S, dt) only: not on the launch shape, ld, how the members are cut
// into shards, or how the rows are cut into calls — S carries the state between calls and em1 is recomputed from the same tau,
// so it has the same bits.  A NaN in a member's T row makes e, hence that member's state, NaN from that row on; it touches no
// other lane.
//
// One member per lane (blockIdx.y: the scenario), time sequential inside the lane, one coalesced load and one coalesced store
// per row (plus the H load and J component stores where asked for).  Nothing is reused, so there is no LDS and no tiling; the
// only latency the lane could not hide by itself is the row load in front of the recurrence, so the loads of
// FIVEEQ_SEA_UNROLL rows are issued before the first is used (they do not depend on the state).  Inactive components
// (j >= n_comp) are skipped by uniform branches, never computed with neutral values.
// ---------------------------------------------------------------------------------
struct SeaLane {
    double em1[FIVEEQ_SEA_MAX], a[FIVEEQ_SEA_MAX], b[FIVEEQ_SEA_MAX], T0[FIVEEQ_SEA_MAX], cap[FIVEEQ_SEA_MAX], S[FIVEEQ_SEA_MAX];
};

// one row of one member: the components advanced by Tt, the total and the component rows stored
__device__ __forceinline__ void sea_level_row(SeaLane& L, const int n_comp, const int rate_mask, const double dt, const double Tt,
                                              const double h, const bool with_heat, const double eta, double* __restrict__ tot,
                                              double* __restrict__ cmp, const int64_t ld_out) {
#pragma unroll
    for (int j = 0; j < FIVEEQ_SEA_MAX; ++j) {
        if (j < n_comp) {
            const double x = Tt - L.T0[j];
            const double p = L.b[j] * x;
            const double c = L.a[j] + p;
            double e = c * x;
            if (e > L.cap[j]) e = L.cap[j];
            if (rate_mask >> j & 1) {
                const double w = dt * e;
                L.S[j] = L.S[j] + w;
            } else {
                const double v = L.S[j] - e;
                const double w = L.em1[j] * v;
                L.S[j] = L.S[j] + w;
            }
        }
    }
    double acc = with_heat ? eta * h : 0.0;
#pragma unroll
    for (int j = 0; j < FIVEEQ_SEA_MAX; ++j)
        if (j < n_comp) acc = acc + L.S[j];
    *tot = acc;
    if (cmp) {
#pragma unroll
        for (int j = 0; j < FIVEEQ_SEA_MAX; ++j)
            if (j < n_comp) cmp[(int64_t)j * ld_out] = L.S[j];
    }
}

template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void sea_level_rows_kernel(
    const int n_comp, const int rate_mask, const int64_t n, const int64_t ld, const int n_rows, const double dt,
    const T* __restrict__ T_rows, const int64_t t_row, const int64_t t_scen, const double* __restrict__ par,
    const double* __restrict__ heat, const int64_t h_row, const int64_t h_scen, const double* __restrict__ eta_row,
    double* __restrict__ S_io, double* __restrict__ total, double* __restrict__ comps, const int64_t ld_out) {
    const int64_t m = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (m >= n) return;
    const int64_t s = blockIdx.y;
    const int64_t plane = (int64_t)n_comp * ld;                  // one parameter of every component: par is [5][n_comp][ld]
    SeaLane L;
    double* __restrict__ S = S_io + s * plane + m;
#pragma unroll
    for (int j = 0; j < FIVEEQ_SEA_MAX; ++j) {
        L.em1[j] = L.a[j] = L.b[j] = L.T0[j] = L.cap[j] = L.S[j] = 0.0;
        if (j < n_comp) {
            const double* __restrict__ pj = par + (int64_t)j * ld + m;
            if (!(rate_mask >> j & 1)) {
                const double x = -dt / pj[0];
                L.em1[j] = fe_expm1_neg(x);
            }
            L.a[j] = pj[plane];
            L.b[j] = pj[2 * plane];
            L.T0[j] = pj[3 * plane];
            L.cap[j] = pj[4 * plane];
            L.S[j] = S[(int64_t)j * ld];
        }
    }
    const bool with_heat = heat != nullptr;
    const double eta = with_heat ? eta_row[m] : 0.0;
    const T* __restrict__ Tp = T_rows + s * t_scen + m;
    const double* __restrict__ Hp = with_heat ? heat + s * h_scen + m : nullptr;
    double* __restrict__ tot = total + s * n_rows * ld_out + m;
    const int64_t cmp_row = (int64_t)n_comp * ld_out;            // one row of comps: [n_comp][ld_out]
    double* __restrict__ cmp = comps ? comps + s * n_rows * cmp_row + m : nullptr;
    int t = 0;
    for (; t + FIVEEQ_SEA_UNROLL <= n_rows; t += FIVEEQ_SEA_UNROLL) {
        double Tt[FIVEEQ_SEA_UNROLL], h[FIVEEQ_SEA_UNROLL];
#pragma unroll
        for (int u = 0; u < FIVEEQ_SEA_UNROLL; ++u) {
            Tt[u] = (double)Tp[(int64_t)(t + u) * t_row];
            h[u] = with_heat ? Hp[(int64_t)(t + u) * h_row] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < FIVEEQ_SEA_UNROLL; ++u)
            sea_level_row(L, n_comp, rate_mask, dt, Tt[u], h[u], with_heat, eta, tot + (int64_t)(t + u) * ld_out,
                          cmp ? cmp + (int64_t)(t + u) * cmp_row : nullptr, ld_out);
    }
    for (; t < n_rows; ++t) {
        const double Tt = (double)Tp[(int64_t)t * t_row];
        const double h = with_heat ? Hp[(int64_t)t * h_row] : 0.0;
        sea_level_row(L, n_comp, rate_mask, dt, Tt, h, with_heat, eta, tot + (int64_t)t * ld_out,
                      cmp ? cmp + (int64_t)t * cmp_row : nullptr, ld_out);
    }
#pragma unroll
    for (int j = 0; j < FIVEEQ_SEA_MAX; ++j)
        if (j < n_comp) S[(int64_t)j * ld] = L.S[j];
}

}  // namespace fiveeq
