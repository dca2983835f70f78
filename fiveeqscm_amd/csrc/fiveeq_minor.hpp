// fiveeq_minor.hpp — kernel 17: per-member minor-gas forcing rows (minor_rows_kernel), the second generator of member_forcing rows.
// Part of fiveeq_device.hpp, which includes it after fiveeq_carbon.hpp (fe_expm1_neg: fiveeq_math.hpp): include that header,
// not this one.
#pragma once

#ifndef FIVEEQ_MINOR_MAX
#define FIVEEQ_MINOR_MAX 8        // species per call: R, em1, a, eff per species in registers, 4 * 8 fp64 = 64 VGPRs per lane
#endif

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 17 — SHARD-COMPUTABLE MINOR-GAS FORCING ROWS.  K <= FIVEEQ_MINOR_MAX constant-lifetime species (HFCs, PFCs, SF6, ...),
// each a one-pool reservoir with no state dependence, advanced by the exact step of minor_gases.step_minor_gases,
//     R <- R + expm1(-dt / tau) (R - tau c E),
// with each member's OWN lifetime tau and radiative efficiency eff; the emissions E [n_rows][K] and emis2conc c [K] are shared.
//     rows[t][m] = (accumulate ? rows[t][m] : 0) + sum_k eff_k[m] R_k[m]  after step t.
//
// THE ARITHMETIC is fp64 whatever the row precision, every operation rounded on its own (contraction is off in this file, no
// fma is written — like fiveeq_noise.hpp).  tau and eff are read in the row precision and widened exactly.
// Once per call, for species k of the lane's member:
//     x   = -dt / tau_k          (IEEE division, not fe_rcp)
//     em1 = fe_expm1_neg(x)      (the pinned primitive of fiveeq_math.hpp: what fiveeq_math_probe_f64(op = 0) returns for x)
//     a   = tau_k * c_k
// Per step t, for k ascending:
//     u = a * E[t][k];   v = R_k - u;   w = em1 * v;   R_k = R_k + w
// then the row value, for k ascending:
//     acc = accumulate ? (double)rows[t][m] : 0.0;     p = eff_k * R_k;   acc = acc + p;     rows[t][m] = (T)acc
//
// CONSEQUENCES.  The bits depend on (tau, eff, c, E, R0, dt) only: not on the launch shape, ld, how the members are cut into
// shards, or how [0, n_steps) is cut into calls — R carries the state between calls and em1 is recomputed from the same tau, so
// it has the same bits.  For fp64 rows, chained accumulate calls over consecutive species groups equal ONE ordered sum over all
// species bit for bit (acc starts from the stored fp64 value).  For fp32 rows each call rounds once at its store, so the
// grouping is part of the definition: consecutive groups of FIVEEQ_MINOR_MAX in species order, the last one shorter
// (minor_gases.minor_gas_rows).  With accumulate the rows may already hold something else — AR(1) noise, say — and the minor
// gases are added on top without a third buffer.
//
// One member per lane, time sequential inside the lane, one coalesced row store per step.  The emission row of a step is read
// at wave-uniform addresses (t, k and n_species are uniform: scalar loads through the constant cache); inactive species
// (k >= n_species) are skipped by uniform branches, never computed with neutral values (a +0 added to a -0 would change bits).
// ---------------------------------------------------------------------------------
struct MinorC {
    double c[FIVEEQ_MINOR_MAX];      // emis2conc, by value in the launch
};

template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void minor_rows_kernel(const int n_species, const int64_t n, const int64_t ld,
                                                                  const int n_rows, const double dt, const MinorC cc,
                                                                  const double* __restrict__ emis, const T* __restrict__ tau,
                                                                  const T* __restrict__ eff, double* __restrict__ R,
                                                                  T* __restrict__ rows, const int accumulate) {
    const int64_t m = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (m >= n) return;
    double Rk[FIVEEQ_MINOR_MAX], em1[FIVEEQ_MINOR_MAX], a[FIVEEQ_MINOR_MAX], ef[FIVEEQ_MINOR_MAX];
#pragma unroll
    for (int k = 0; k < FIVEEQ_MINOR_MAX; ++k) {
        Rk[k] = em1[k] = a[k] = ef[k] = 0.0;
        if (k < n_species) {
            const double tk = (double)tau[(int64_t)k * ld + m];
            const double x = -dt / tk;
            em1[k] = fe_expm1_neg(x);
            a[k] = tk * cc.c[k];
            ef[k] = (double)eff[(int64_t)k * ld + m];
            Rk[k] = R[(int64_t)k * ld + m];
        }
    }
    for (int t = 0; t < n_rows; ++t) {
        const double* __restrict__ e = emis + (int64_t)t * n_species;
        T* __restrict__ out = rows + (int64_t)t * ld + m;
        double acc = accumulate ? (double)*out : 0.0;
#pragma unroll
        for (int k = 0; k < FIVEEQ_MINOR_MAX; ++k) {
            if (k < n_species) {
                const double u = a[k] * e[k];
                const double v = Rk[k] - u;
                const double w = em1[k] * v;
                Rk[k] = Rk[k] + w;
            }
        }
#pragma unroll
        for (int k = 0; k < FIVEEQ_MINOR_MAX; ++k) {
            if (k < n_species) {
                const double p = ef[k] * Rk[k];
                acc = acc + p;
            }
        }
        *out = (T)acc;
    }
#pragma unroll
    for (int k = 0; k < FIVEEQ_MINOR_MAX; ++k)
        if (k < n_species) R[(int64_t)k * ld + m] = Rk[k];
}

}  // namespace fiveeq
