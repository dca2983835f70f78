// fiveeq_device.hpp — gfx950 device code for the five-equation FaIR ensemble step.
//
// Written for MI355X (CDNA4, wave64) only.  The path is element-wise over ensemble
// members: one member per lane, struct-of-arrays rows so that a wave's 64 lanes read
// 64 consecutive elements of each row (512 B per wave-instruction at fp64), no MFMA.
//
// The reference (stujen/fiveEqSCM @ v0) has no implementation of these equations
// (only `emissions[0]*exp(-time)`, U_FaIR/concentrations.py:4-5); the function
// split of fiveeq_member.hpp follows the names it reserves at .coveragerc:12-19
// (alpha_val, step_conc, step_forc, step_temp).  See include/fiveeq.h for the model.
//
// The kernels, by the header that holds them:
//   fiveeq_step.hpp     1   step_kernel        one timestep per launch — the north-star form; HBM-bound, A = w(2SP + 4G + 7) per member-step
//                       1s  step_scen_kernel   the same under several emission scenarios
//                       1m  step_mforc_kernel  the same with a per-member forcing row per step (2m: fused_mforc_kernel)
//   fiveeq_fused.hpp    2   fused_kernel       time-fused (and, INV = true, concentration-driven); state in registers; VALU-bound
//   fiveeq_small.hpp    2c  small_kernel       small ensembles: one member per quad of lanes (pool per lane), the model in registers
//                       2d  small_multi_kernel, small_octet_kernel: the same for several gases
//   fiveeq_summary.hpp  3   hfc_conc_kernel    the reference's one function over an ensemble
//                       4   hist_rows_kernel   fixed-bin histograms (+ moments) of rows: the pass of the streamed histogram pipelines
//                       5   lhs_kernel         shard-computable Latin hypercube (keyed Feistel bijection)
//                       6   row_moments_kernel, select_bins_kernel, select_pick_kernel: the end-of-run summary
//   fiveeq_wsummary.hpp 7   wrow_moments_kernel, whist_rows_kernel, wselect_bins_kernel, wselect_pick_kernel: the weighted summary
//   fiveeq_resample.hpp 8   wscan_*_kernel, resample_pick_kernel, gather_rows_kernel: resampling a weighted ensemble
//   fiveeq_metrics.hpp  9   traj_metrics_kernel per-member peak, level crossings and window sums of the stored rows, in one streaming pass
//   fiveeq_joint.hpp    10  joint_moments_kernel, cond_sums_kernel and their folds: co-moments and conditional sums of per-member rows
//   fiveeq_diag.hpp     stream_copy_kernel, stream_copy_wide_kernel, stream_copy_nt_kernel, math_probe_kernel, busy_kernel
//   fiveeq_score.hpp    11  score_rows_kernel   the misfit accumulators of stored rows against observed records, live rows only
//   fiveeq_forcrows.hpp 12 forcing_rows_kernel the forcing, energy imbalance and heat uptake of a run recomputed from its stored rows
//   fiveeq_pulse.hpp    13 pulse_response_kernel the forcing, warming and concentration response to emission pulses, summed to horizons
//   fiveeq_noise.hpp    14 noise_rows_kernel    per-member AR(1) noise rows from a counter-based integer deviate (member_forcing rows)
//   fiveeq_smooth.hpp   15 running_mean_kernel, window_trend_kernel: per-member running means and linear-trend sums of stored rows
//   fiveeq_carbon.hpp   16 carbon_rows_kernel   airborne emissions, cumulative emissions and uptake, airborne fraction, iIRF, alpha and sink from stored rows
//   fiveeq_minor.hpp    17 minor_rows_kernel    per-member forcing rows of constant-lifetime minor gases, each member's own lifetime and efficiency
//   fiveeq_aerosol.hpp  18 aerosol_rows_kernel  per-member aerosol forcing rows (ERFari + ERFaci) from shared emissions, each member's own coefficients
//   fiveeq_sea.hpp      19 sea_level_rows_kernel per-member sea-level rise rows from stored T rows (and heat-uptake rows), each member's own components
// and what they share: fiveeq_math.hpp (the model struct, lane types, fe_* math), fiveeq_stats.hpp (per-wave statistics, the bin
// rule), fiveeq_member.hpp (member_step(), gas_forcing(), the misfit update, the lane's member span and row access).
// All model arithmetic is member_step(): every kernel that steps the model gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Floating-point contraction is OFF for this translation unit (here, ahead of every header below, and in csrc/Makefile): the compiler never
// decides which a*b+c fuse.  Every fused multiply-add of the model step is written as fe_fma() (fiveeq_math.hpp), so
// "per-step == fused == K-step == small == graph bit for bit" and the distance to the CPU oracle are properties of this
// source, not of a hipcc release.
#pragma clang fp contract(off)

#ifndef FIVEEQ_BLOCK
#define FIVEEQ_BLOCK 256          // threads per workgroup of the fused / inverse / utility kernels (4 waves)
#endif
#ifndef FIVEEQ_STEP_BLOCK
#define FIVEEQ_STEP_BLOCK 64      // threads per workgroup of the per-step kernel: ONE wave (measured best, fiveeq_step.hpp)
#endif
// (Experiments that lost — device-library math, non-temporal trajectory stores, model constants in SGPRs —
// are recorded in profiles/r01/ab_variants.txt; their code paths are gone.)
#ifndef FIVEEQ_SMALL_BLOCK
#define FIVEEQ_SMALL_BLOCK 256    // threads per workgroup of the small-ensemble kernel: four waves, one per SIMD of a CU (measured, fiveeq_small.hpp)
#endif
#ifndef FIVEEQ_FUSED_CHUNK
#define FIVEEQ_FUSED_CHUNK 125    // drive-table steps staged into LDS per refill (fused kernel)
#endif

namespace fiveeq {

constexpr int MAX_GAS = 3;
constexpr int MAX_POOLS = 4;
constexpr int DRIVE_STRIDE = 8;

}  // namespace fiveeq

#include "fiveeq_math.hpp"
#include "fiveeq_stats.hpp"
#include "fiveeq_member.hpp"
#include "fiveeq_step.hpp"
#include "fiveeq_fused.hpp"
#include "fiveeq_small.hpp"
#include "fiveeq_summary.hpp"
#include "fiveeq_wsummary.hpp"
#include "fiveeq_resample.hpp"
#include "fiveeq_metrics.hpp"
#include "fiveeq_smooth.hpp"
#include "fiveeq_joint.hpp"
#include "fiveeq_diag.hpp"
#include "fiveeq_score.hpp"
#include "fiveeq_forcrows.hpp"
#include "fiveeq_pulse.hpp"
#include "fiveeq_noise.hpp"
#include "fiveeq_carbon.hpp"
#include "fiveeq_minor.hpp"
#include "fiveeq_aerosol.hpp"
#include "fiveeq_sea.hpp"
