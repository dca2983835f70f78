// fiveeq_aerosol.hpp — kernel 18: per-member aerosol forcing rows from emissions (aerosol_rows_kernel), the third generator of
// member_forcing rows.  Part of fiveeq_device.hpp, which includes it after fiveeq_minor.hpp (fe_log: fiveeq_math.hpp): include
// that header, not this one.
#pragma once

#ifndef FIVEEQ_AEROSOL_MAX
#define FIVEEQ_AEROSOL_MAX 8      // species per call: ari and 1 / s per species in registers, 2 * 8 fp64 = 32 VGPRs per lane
#endif

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Kernel 18 — SHARD-COMPUTABLE AEROSOL FORCING ROWS.  K <= FIVEEQ_AEROSOL_MAX short-lived forcers (SO2, BC, OC, NH3, ...) whose
// emissions E [n_rows][K] and reference (pre-industrial) emissions base [K] the members share, turned into each member's OWN
// aerosol forcing: the aerosol-radiation term, a per-member linear mix of the species, and the aerosol-cloud term, which
// saturates with each member's own shape parameters s_k,
//     rows[t][m] = (accumulate ? rows[t][m] : 0) + sum_k ari_k[m] (E[t][k] - base_k)
//                  - beta[m] ( ln(1 + sum_{k in mask} E[t][k] / s_k[m]) - ln(1 + sum_{k in mask} base_k / s_k[m]) ).
//
// THE ARITHMETIC is fp64 whatever the row precision, every operation rounded on its own (contraction is off in this file, no
// fma is written — like fiveeq_minor.hpp and fiveeq_noise.hpp; fe_log is the pinned primitive and keeps the fma it is written
// with).  ari, s and beta are read in the row precision and widened exactly.
// Once per call, for the lane's member:
//     for k ascending, bit k of aci_mask set:   g_k = 1.0 / s_k          (IEEE division, not fe_rcp)
//     x = 0.0;  for k ascending in the mask:    p = g_k * base_k;  x = x + p
//     y0 = 1.0 + x;   L0 = fe_log(y0)           (what fiveeq_math_probe_f64(op = 2) returns for y0)
// Per step t:
//     acc = accumulate ? (double)rows[t][m] : 0.0
//     for k ascending, k < n_species:           e = E[t][k] - base_k;  p = ari_k * e;  acc = acc + p
//     if aci_mask != 0:
//         x = 0.0;  for k ascending in the mask: p = g_k * E[t][k];  x = x + p
//         y = 1.0 + x;  L = fe_log(y);  v = L - L0;  w = beta * v;  acc = acc - w
//     rows[t][m] = (T)acc
// With aci_mask == 0 the rows `shape` and `beta` are not read (they may be NULL).
//
// CONSEQUENCES.  The bits depend on (E, base, ari, s, beta, aci_mask) only: not on the launch shape, ld, how the members are
// cut into shards, or how the steps are cut into calls — there is no state to carry, and g_k and L0 are recomputed from the
// same values by the same operations.  A step whose emissions equal base forms L by the very operations that formed L0, so
// v = +0, e = +0 for every species, and the step contributes exactly +0: a table equal to base at every step gives all-zero
// rows, and by the contract of member_forcing= that is the run without them, bit for bit.
//
// DOMAIN: E >= 0, base >= 0, s > 0 with 1 / s finite — so y >= 1, finite and normal, fe_log's domain.  The wrapper
// (aerosols.aerosol_rows) enforces it; the kernel does not guard it.
//
// One member per lane, time sequential inside the lane, one coalesced row store per step.  The emission record of a step is
// read at wave-uniform addresses (t, k, n_species and aci_mask are uniform: scalar loads through the constant cache); species
// at k >= n_species and species outside aci_mask are skipped by uniform branches, never computed with neutral values.  An
// accumulating call loads the stored element of step t + 1 before the arithmetic of step t, so the load's latency lies under
// a step's arithmetic instead of ahead of it (the address is another row: the order of the accesses to any one element stays
// load, then store).
// ---------------------------------------------------------------------------------
struct AerosolBase {
    double b[FIVEEQ_AEROSOL_MAX];    // reference emissions, by value in the launch
};

// the steps of one lane.  ACC (an accumulating call) is a template parameter so that the writing call's loop holds no load at
// all: with one loop for both, the wait for the row element read ahead also waits for the previous step's store.
template <bool ACC, typename T>
__device__ __forceinline__ void aerosol_steps(const int n_species, const int aci_mask, const int64_t ld, const int n_rows,
                                              const AerosolBase& bb, const double* __restrict__ emis,
                                              const double (&ar)[FIVEEQ_AEROSOL_MAX], const double (&g)[FIVEEQ_AEROSOL_MAX],
                                              const double bt, const double L0, T* __restrict__ out) {
    double stored = ACC ? (double)*out : 0.0;                    // n_rows >= 1: the launcher returns before a launch without rows
    for (int t = 0; t < n_rows; ++t) {
        const double* __restrict__ e = emis + (int64_t)t * n_species;
        double acc = stored;
        if (ACC && t + 1 < n_rows) stored = (double)out[ld];
        double x = 0.0;                                          // acc and x are two chains, each in ascending k: one pass over k
#pragma unroll
        for (int k = 0; k < FIVEEQ_AEROSOL_MAX; ++k) {
            if (k < n_species) {
                const double ek = e[k];
                const double d = ek - bb.b[k];
                const double p = ar[k] * d;
                acc = acc + p;
                if ((aci_mask >> k) & 1) {
                    const double q = g[k] * ek;
                    x = x + q;
                }
            }
        }
        if (aci_mask != 0) {
            const double y = 1.0 + x;
            const double L = fe_log(y);
            const double v = L - L0;
            const double w = bt * v;
            acc = acc - w;
        }
        *out = (T)acc;
        out += ld;
    }
}

template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void aerosol_rows_kernel(const int n_species, const int aci_mask, const int64_t n,
                                                                    const int64_t ld, const int n_rows, const AerosolBase bb,
                                                                    const double* __restrict__ emis, const T* __restrict__ ari,
                                                                    const T* __restrict__ shape, const T* __restrict__ beta,
                                                                    T* __restrict__ rows, const int accumulate) {
    const int64_t m = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if (m >= n) return;
    double ar[FIVEEQ_AEROSOL_MAX], g[FIVEEQ_AEROSOL_MAX];
#pragma unroll
    for (int k = 0; k < FIVEEQ_AEROSOL_MAX; ++k) {
        ar[k] = g[k] = 0.0;
        if (k < n_species) {
            ar[k] = (double)ari[(int64_t)k * ld + m];
            if ((aci_mask >> k) & 1) g[k] = 1.0 / (double)shape[(int64_t)k * ld + m];
        }
    }
    double bt = 0.0, L0 = 0.0;
    if (aci_mask != 0) {
        bt = (double)beta[m];
        double x = 0.0;
#pragma unroll
        for (int k = 0; k < FIVEEQ_AEROSOL_MAX; ++k) {
            if ((aci_mask >> k) & 1) {
                const double p = g[k] * bb.b[k];
                x = x + p;
            }
        }
        const double y0 = 1.0 + x;
        L0 = fe_log(y0);
    }
    if (accumulate)
        aerosol_steps<true, T>(n_species, aci_mask, ld, n_rows, bb, emis, ar, g, bt, L0, rows + m);
    else
        aerosol_steps<false, T>(n_species, aci_mask, ld, n_rows, bb, emis, ar, g, bt, L0, rows + m);
}

}  // namespace fiveeq
