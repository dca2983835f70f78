/*
 * fiveeq.h — C ABI of the MI355X (gfx950) ensemble engine for the five-equation
 * FaIR simple climate model.   Library: fiveeqscm_amd/csrc/libfiveeq_hip.so
 *
 * WHAT THIS REPLACES IN THE REFERENCE (stujen/fiveEqSCM @ v0)
 *   The reference has NO native code and NO FFI: its whole
 *   runtime is the Python function
 *       calculate_hfc_conc(emissions, time, lifetime)   U_FaIR/concentrations.py:4-5
 *   (duplicate: example/concentrations.py:4-5).  The five equations its README
 *   announces (README.md:2,6,8) — pool decay R_i, iIRF->alpha, concentration C,
 *   forcing F, two thermal boxes T_j — are not implemented there; the only trace
 *   of the intended function split is the list of names at .coveragerc:12-19
 *   (step_conc, step_forc, step_temp, g_1, g_0, alpha_val, k_q).  Each entry
 *   point below cites the reference item it stands behind, or says "new".
 *
 * CONVENTIONS
 *   - Plain C: pointers, sizes, one POD struct.  No torch / C++ types.
 *   - Every `dev` pointer is DEVICE memory owned by the caller (the Python host
 *     passes torch-ROCm tensor data_ptr()s).  The library allocates nothing on
 *     the device, never synchronises the stream (launches are asynchronous) and is
 *     safe to call concurrently from several threads on different streams / devices.
 *     ALL the state it keeps: the thread-local error string (fiveeq_last_error), and TWO
 *     process-wide words, the fp32 packing switch of fiveeq_set_f32_packing and the row cache
 *     policy of fiveeq_set_row_policy — atomics that every call reads once, so a call in flight
 *     while another thread flips one runs entirely with the old or entirely with the new setting
 *     (every setting gives the same bits).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - Return value: 0 = success; <0 = error (FIVEEQ_E_*), message retrievable
 *     with fiveeq_last_error() on the same thread.  Arguments are validated on
 *     the host BEFORE any launch: a bad shape never reaches the GPU.
 *   - Struct-of-arrays over ensemble members.  A "row" is one quantity for all
 *     members: row k of array X starts at X + k*ld; member m is element m of the
 *     row (0 <= m < n_members <= ld).  `ld` (leading dimension, in elements)
 *     lets a caller run a sub-range of a larger allocation — e.g. the host's chunk-major schedule
 *     for ensembles larger than the Infinity Cache: all steps for members [0, c), then [c, 2c), ...
 *
 * MODEL STEP (identical arithmetic in every kernel; fp64 or fp32)
 *     T_old = S_0 + S_1
 *     per gas g:  G_a  = (sum_i R_gi) / c_g ;   G_u = cumE_g - G_a
 *                 iIRF = min(r0 + rC*G_u + rT*T_old + ra*G_a, iirf_max)
 *                 alpha= g0 * exp(iIRF / g1)
 *                 R_gi+= expm1(-dt/(alpha*tau_i)) * (R_gi - a_i*c_g*E_g*alpha*tau_i)
 *                 C_g  = C0_g + sum_i R_gi
 *                 F   += f1*ln(C_g/C0_g) + f2*(C_g-C0_g) + f3*(sqrt(C_g)-sqrt(C0_g))
 *     F += F_ext ;  S_j += expm1(-dt/d_j) * (S_j - q_j*F) ;  T = S_0 + S_1
 */
#ifndef FIVEEQ_H
#define FIVEEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FIVEEQ_ABI_VERSION   13
#define FIVEEQ_MAX_GAS       3
#define FIVEEQ_MAX_POOLS     4
#define FIVEEQ_N_BOX         2
#define FIVEEQ_DRIVE_STRIDE  8   /* elements per step in the drive table, below */
#define FIVEEQ_LHS_MAX_TOTAL (1LL << 28)   /* largest Latin-hypercube design (members): stratum + jitter stays an exact fp64 sum */

#define FIVEEQ_OK             0
#define FIVEEQ_E_INVALID     -1  /* bad argument (NULL pointer, size, range) */
#define FIVEEQ_E_UNSUPPORTED -2  /* pool layout not instantiated */
#define FIVEEQ_E_HIP         -3  /* a HIP runtime call failed */

/* Shared (not per-member) parameters of one gas.  Active pools are the first
 * n_pools entries of a[] / tau[].  g0 and g1 are the alpha-closure constants
 * (host helpers g_0 / g_1; names from .coveragerc:15-16 of the reference). */
typedef struct fiveeq_gas {
    double  a[FIVEEQ_MAX_POOLS];    /* pool fractions                       */
    double  tau[FIVEEQ_MAX_POOLS];  /* pool time-scales, years              */
    double  g0, g1;                 /* alpha = g0 * exp(iIRF / g1)          */
    double  ra;                     /* iIRF sensitivity to own burden G_a   */
    double  C0;                     /* pre-industrial concentration         */
    double  emis2conc;              /* c_g: concentration units per emission unit */
    double  f[3];                   /* forcing coefficients: log, linear, sqrt */
    int32_t n_pools;                /* 1..4                                  */
    int32_t reserved;
} fiveeq_gas;

/* Whole shared model.  Always given in double; the f32 entry points round it.
 * ACCURACY OF THE _f32 ENTRY POINTS, against 50-digit arithmetic over the 24 golden members x 750 steps
 * (tests/test_golden_fiveeq.py): C within 2.9e-6 relative, T within 1.7e-5 (test bounds 5e-6 / 3e-5 + 2e-6 K).  What bounds
 * it is the fp32 rounding of the STATE carried through 750 steps (~13 ulp of C at the end), not the transcendental forms:
 * with a two-step expm1 reduction, a Newton step on the reciprocal and an fdlibm-style logarithm in place of the hardware
 * v_rcp_f32 / v_log_f32 forms the same members changed 48 of 840 stored values and no worst case, for +21 % on the
 * time-fused kernel (profiles/r05/fp32_math_ab.txt; the variant was measured at commit 51b82a6 and not kept).  A run that
 * needs more digits than that runs the _f64 entry points. */
typedef struct fiveeq_model {
    fiveeq_gas gas[FIVEEQ_MAX_GAS];
    double  d[FIVEEQ_N_BOX];        /* thermal-box time-scales, years       */
    double  iirf_max;               /* clip on iIRF (e.g. 97)               */
    double  dt;                     /* step length, years                   */
    int32_t n_gas;                  /* 1..3                                  */
    int32_t reserved;
} fiveeq_model;

/* Array shapes used below (G = n_gas, SP = sum of n_pools over gases):
 *   drive   dev [n_steps][8]   shared by all members, per step:
 *                              [0..2] E_g (emission rate), [3..5] cumulative emissions BEFORE
 *                              the step, [6] F_ext, [7] OUTPUT ROW of this step: the step's C and
 *                              T are stored at row k = (int)drive[t][7] of C_traj / T_traj if
 *                              0 <= k < n_rows, and not stored otherwise (store every step:
 *                              drive[t][7] = t, n_rows = n_steps)
 *   r       dev [3*G][ld]      rows g*3+0/1/2 = r0, rC, rT of gas g (per member)
 *   q       dev [2][ld]        thermal-box coefficients (per member)
 *   R       dev [SP][ld]       pool contents, gas-major, in/out
 *   S       dev [2][ld]        thermal-box temperatures, in/out
 *   C_traj  dev [n_rows][G][ld]  concentrations of the stored steps (may be NULL)
 *   T_traj  dev [n_rows][ld]     temperature of the stored steps    (may be NULL)
 *   T_stats dev [W][n_steps][4]  fp64 (also for the f32 entry points), W = fiveeq_stats_waves(n_members):
 *                              per wave of 64 members and per step (sum T, sum T^2, min T, max T);
 *                              folding over W gives the ensemble moments of every step without a
 *                              stored trajectory (may be NULL).  Every step in the range writes its
 *                              record in all W wave rows.  Wave-major on purpose: a call on the member
 *                              sub-range starting at member m0 (a multiple of 64) addresses its part of
 *                              a larger buffer as T_stats + (m0/64)*n_steps*4.
 */

/* new — library identification */
int         fiveeq_abi_version(void);
const char *fiveeq_last_error(void);
/* new — sha256 (hex) of the sources this library was compiled from, concatenated in the order of csrc/Makefile's SRCS:
 * fiveeq_capi.hip, fiveeq_device.hpp and the headers it includes, include/fiveeq.h — stamped by csrc/Makefile ("unstamped" otherwise).  A binding that
 * sits next to those sources recomputes it and refuses a library built from other text (fiveeqscm_amd/_capi.py). */
const char *fiveeq_source_hash(void);
/* new — the experiment knobs this library was compiled with (-DFIVEEQ_STEP_WAVES=..., -DFIVEEQ_FUSED_CHUNK=..., non-default
 * block sizes ...), space-separated; "" for the product build. */
const char *fiveeq_build_flags(void);
/* new — sizeof(fiveeq_model) as the library was compiled, for binding self-checks */
int64_t     fiveeq_sizeof_model(void);
/* new — 1 if (n_gas, n_pools[]) has a compiled kernel, else 0 */
int         fiveeq_layout_supported(int32_t n_gas, const int32_t *n_pools);
/* new — W of T_stats: ceil(n_members / 64) */
int64_t     fiveeq_stats_waves(int64_t n_members);

/* ONE TIMESTEP, ONE LAUNCH: the north-star hot path.  Stands where the
 * reference intended step_conc + alpha_val + step_forc + step_temp
 * (.coveragerc:12-14,17 — names only; no reference code exists).
 * Reads state/params from HBM, writes state back, writes the step's C, T rows and stats. */
int fiveeq_step_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                    const double *drive, int32_t n_steps, int32_t t,
                    const double *r, const double *q, double *R, double *S,
                    double *C_traj, double *T_traj, int32_t n_rows, double *T_stats, void *stream);
int fiveeq_step_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                    const float *drive, int32_t n_steps, int32_t t,
                    const float *r, const float *q, float *R, float *S,
                    float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void *stream);

/* Steps t_begin <= t < t_end as (t_end - t_begin) launches of the kernel above,
 * enqueued back-to-back on `stream` from C (no Python per step). */
int fiveeq_run_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                   const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                   const double *r, const double *q, double *R, double *S,
                   double *C_traj, double *T_traj, int32_t n_rows, double *T_stats, void *stream);
int fiveeq_run_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                   const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                   const float *r, const float *q, float *R, float *S,
                   float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void *stream);

/* The same launch sequence captured once into a hipGraph ("plan") and replayed:
 * removes per-launch host cost for small ensembles.  The plan bakes in the
 * pointers; they must stay valid until fiveeq_plan_destroy. */
int fiveeq_plan_create_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const double *r, const double *q, double *R, double *S,
                           double *C_traj, double *T_traj, int32_t n_rows, double *T_stats, void **plan_out);
int fiveeq_plan_create_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const float *r, const float *q, float *R, float *S,
                           float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void **plan_out);
int fiveeq_plan_launch(void *plan, void *stream);
int fiveeq_plan_destroy(void *plan);

/* TIME-FUSED variant: one launch advances t_begin..t_end with
 * the member's state held in registers; only the stored C/T rows and the stats are written per
 * step.  Same arithmetic, bit-identical results to the per-step path. */
int fiveeq_run_fused_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const double *r, const double *q, double *R, double *S,
                         double *C_traj, double *T_traj, int32_t n_rows, double *T_stats, void *stream);
int fiveeq_run_fused_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const float *r, const float *q, float *R, float *S,
                         float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void *stream);

/* K STEPS PER LAUNCH: the time-fused kernel over consecutive spans of k_steps
 * — state and parameters cross HBM once per k_steps instead of every step, A_K = w(G+1)[stored rows]
 * + w(2SP+3G+6)/k_steps.  The form for ensembles too small to hide the ~2 us dependent-launch boundary
 * behind one step of HBM traffic (10k members: 2.6 us per launch against 0.2 us of traffic).
 * Bit-identical results to the per-step path. */
int fiveeq_run_ksteps_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                          const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                          const double *r, const double *q, double *R, double *S,
                          double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                          int32_t k_steps, void *stream);
int fiveeq_run_ksteps_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                          const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                          const float *r, const float *q, float *R, float *S,
                          float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                          int32_t k_steps, void *stream);

/* CONSTRAINED RUNS — the in-loop misfit against an observed series (new, ABI v12).  Replaces storing every T row of the
 * observed period and scoring it afterwards (170 steps x N x w bytes): each member carries three fp64 accumulators
 * misfit dev [3][ld] = (A, U, V), read and written in place (zero them before the first step of the window).
 *   obs dev [n_steps][4] fp64, shared: per step t (o_t, p_t, b_t, 0) — o_t the observed anomaly, p_t = 1/sigma_t^2 (0 = no
 *       observation), b_t the baseline weight (1/n_ref inside the reference period, else 0).
 * With Tw = T after step t (the value T_traj would store; fp32 widened exactly) every form updates, in step order and with
 * each operation rounded separately (no fma):
 *     A = A + b_t Tw;  d = Tw - o_t;  pd = p_t d;  U = U + pd;  V = V + pd d
 * and leaves the rows untouched on steps with p_t == 0 && b_t == 0.  The score of the baseline-corrected series is then
 * chi2 = V - 2 A U + A^2 P with P = sum_t p_t (= sum_t p_t (T_t - mean_ref T - o_t)^2), computed by the caller.
 * Everything else — C_traj, T_traj, the row map, T_stats, R, S — exactly as in fiveeq_run_* / fiveeq_run_ksteps_*, bit for
 * bit; the accumulators are the same bits in every form and for every split of the range into calls.
 *   form FIVEEQ_FORM_PER_STEP: one launch of the per-step kernel per step (fiveeq_run_*); the obs record is read with scalar
 *       loads and a step inside the window moves 48 B more per member (24 read + 24 written), one outside it nothing more;
 *   form FIVEEQ_FORM_FUSED: the time-fused kernel over spans of k_steps (0 = one launch for the range; fiveeq_run_fused_* /
 *       fiveeq_run_ksteps_*): the accumulators stay on chip — in a lane-private LDS slot, not registers, so that every
 *       layout keeps its plain kernel's waves per SIMD — and cross HBM once per launch (48 B per member).  fp32 {4} runs
 *       one member per lane (no packed misfit form for that layout); fp32 4 + 1 + 1 packs two members per lane as usual.
 * Pool layouts {4} and 4 + 1 + 1 only (fiveeq_misfit_layout_supported); not in the small-ensemble, concentration-driven,
 * compensated or histogram-ring forms.  FIVEEQ_E_INVALID for NULL or unaligned obs / misfit, an unknown form, k_steps < 0,
 * a step range outside [0, n_steps) or a layout without a misfit form — before anything is launched. */
#define FIVEEQ_FORM_PER_STEP 0
#define FIVEEQ_FORM_FUSED    1
int fiveeq_run_obs_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                       const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                       const double *r, const double *q, double *R, double *S,
                       double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                       const double *obs, double *misfit, int32_t form, int32_t k_steps, void *stream);
int fiveeq_run_obs_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                       const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                       const float *r, const float *q, float *R, float *S,
                       float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                       const double *obs, double *misfit, int32_t form, int32_t k_steps, void *stream);
/* new — fiveeq_plan_create_* of the per-step form above: the launches of [t_begin, t_end) with the misfit, captured once;
 * the plan bakes in obs and misfit too. */
int fiveeq_plan_create_obs_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                               const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                               const double *r, const double *q, double *R, double *S,
                               double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                               const double *obs, double *misfit, void **plan_out);
int fiveeq_plan_create_obs_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                               const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                               const float *r, const float *q, float *R, float *S,
                               float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                               const double *obs, double *misfit, void **plan_out);
/* new — 1 if the pool layout has the misfit forms above, else 0 */
int fiveeq_misfit_layout_supported(int32_t n_gas, const int32_t *n_pools);

/* SCENARIOS — one parameter ensemble under several emission scenarios at once (new, ABI v13).  Every parameter member m is
 * advanced under each of n_scen scenarios s, and member-scenario (m, s) is bit for bit member m of fiveeq_run_* /
 * fiveeq_run_ksteps_* run with scenario s's drive table: the kernels call the same model step.  Members and scenarios never
 * interact.  Layouts (every scenario stride derives from ld, so a member sub-range [m0, m0 + n) is a pointer offset):
 *   drive  dev [n_scen][n_steps][8]       one drive table per scenario (column 7, the row map, the same in each)
 *   r, q   dev [3G][ld], [2][ld]          SHARED by the scenarios
 *   R, S   dev [n_scen][SP][ld], [n_scen][2][ld]
 *   C_traj dev [n_scen][n_rows][G][ld] or NULL;   T_traj dev [n_scen][n_rows][ld] or NULL
 *   T_stats dev [n_scen][fiveeq_stats_waves(ld)][n_steps][4] or NULL
 *   form FIVEEQ_FORM_PER_STEP: one launch per step; a lane loads its member's 3G + 2 parameter rows ONCE and advances the
 *       member under all n_scen scenarios (the drive records are read as wave-uniform scalar loads), so a member-scenario-
 *       step moves w (2 SP + 4 + (G + 1) stored) + w (3G + 2) / n_scen bytes;
 *   form FIVEEQ_FORM_FUSED: the time-fused kernel over spans of k_steps (0 = one launch for the range), one grid row of
 *       workgroups per scenario (each stages its own scenario's drive chunk).
 * Every pool layout.  FIVEEQ_E_INVALID for n_scen outside [1, fiveeq_max_scenarios()], a NULL drive or state pointer, an
 * unknown form, k_steps < 0 or a step range outside [0, n_steps) — before anything is launched.
 * The scenario axis combines with the per-member forcing scales (fiveeq_run_scen_forc_*, under FORCING SCALES below); not
 * with the misfit, the histogram ring, the concentration-driven, the compensated or the small-ensemble forms. */
int fiveeq_run_scen_f64(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                        const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const double *r, const double *q, double *R, double *S,
                        double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                        int32_t form, int32_t k_steps, void *stream);
int fiveeq_run_scen_f32(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                        const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const float *r, const float *q, float *R, float *S,
                        float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                        int32_t form, int32_t k_steps, void *stream);
/* new — fiveeq_plan_create_* of the per-step form above: the launches of [t_begin, t_end) captured once */
int fiveeq_plan_create_scen_f64(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                                const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const double *r, const double *q, double *R, double *S,
                                double *C_traj, double *T_traj, int32_t n_rows, double *T_stats, void **plan_out);
int fiveeq_plan_create_scen_f32(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                                const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const float *r, const float *q, float *R, float *S,
                                float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void **plan_out);
/* new — the largest n_scen the scenario forms take (64) */
int32_t fiveeq_max_scenarios(void);

/* FORCING SCALES — per-member scale factors on the gas and external forcings (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, no
 * existing prototype or struct changes, sizeof(fiveeq_model) stays 448 — a caller built against the v13 header keeps working
 * and finds the new symbols by name).  A member carries G + n_fext factors: sg_g per gas and sx_k per external forcing
 * category, 0 <= n_fext <= fiveeq_max_fext() (4); the run carries a shared table of category forcings.  Layouts:
 *   fscale dev [G + n_fext][ld]   kernel precision; gas rows first, then one row per category
 *   fext   dev [n_steps][4]       kernel precision, shared: the forcing of category k during step t at [t][k]; columns
 *                                 k >= n_fext are not read; may be NULL iff n_fext == 0
 * The total forcing of step t becomes, every fma a single rounding,
 *     F = drive[t][6];   F = fma(sx_k, fext[t][k], F), k = 0 .. n_fext-1;   F = fma(sg_g, F_g, F), g = 0 .. G-1
 * with F_g the forcing of gas g exactly as the plain step computes it; nothing else of the step differs.  fma(1, F_g, F) is
 * F + F_g with the same rounding, so unit scales with n_fext == 0, or with an all-zero table, give fiveeq_run_* bit for bit.
 * obs / misfit: both NULL = no misfit; both set = the in-loop misfit of CONSTRAINED RUNS above, the same bits as there.
 *   form FIVEEQ_FORM_PER_STEP: one launch per step; the lane loads its G + n_fext scale rows with its other rows (w (G + n_fext)
 *       bytes more per member-step) and the step's table record is read with scalar loads;
 *   form FIVEEQ_FORM_FUSED: the time-fused kernel over spans of k_steps (0 = one launch for the range): the scales stay on
 *       chip for the span and the table chunk is staged through LDS beside the drive chunk.
 * Every form gives the same bits, fp32 packed or not.  Pool layouts {4} and 4 + 1 + 1 (fiveeq_forcing_layout_supported); not
 * in the small-ensemble, compensated or histogram-ring forms; under the scenario axis through
 * fiveeq_run_scen_forc_* below (without the misfit); concentration-driven through fiveeq_run_inverse_forc_*.  FIVEEQ_E_INVALID for a NULL or
 * misaligned fscale, n_fext outside 0..4, a NULL fext with n_fext > 0, exactly one of obs / misfit set, a layout without the
 * form, an unknown form, k_steps < 0 or a step range outside [0, n_steps) — before anything is launched. */
int fiveeq_run_forc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                        const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const double *r, const double *q, double *R, double *S,
                        double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                        const double *fscale, const double *fext, int32_t n_fext,
                        const double *obs, double *misfit, int32_t form, int32_t k_steps, void *stream);
int fiveeq_run_forc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                        const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const float *r, const float *q, float *R, float *S,
                        float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                        const float *fscale, const float *fext, int32_t n_fext,
                        const double *obs, double *misfit, int32_t form, int32_t k_steps, void *stream);
/* fiveeq_plan_create_* of the per-step form above; the plan bakes in fscale, fext, obs and misfit too */
int fiveeq_plan_create_forc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const double *r, const double *q, double *R, double *S,
                                double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                                const double *fscale, const double *fext, int32_t n_fext,
                                const double *obs, double *misfit, void **plan_out);
int fiveeq_plan_create_forc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const float *r, const float *q, float *R, float *S,
                                float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                                const float *fscale, const float *fext, int32_t n_fext,
                                const double *obs, double *misfit, void **plan_out);
/* MEMBER FORCING — a per-member forcing series that changes every step (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, no existing
 * prototype or struct changes, sizeof(fiveeq_model) stays 448).  What carries internal variability (fiveeq_noise_rows_* below)
 * or a member's own aerosol or volcanic history.  The arguments of fiveeq_run_forc_* up to misfit, then
 *   mforc        dev [n_mforc_rows][ld]   kernel precision: the forcing member m adds during step t at [t][m]; row t is read
 *                                         by step t, so rows [t_begin, t_end) are read by a call
 *   n_mforc_rows                          rows of mforc, >= t_end
 * then form, k_steps, stream (or plan_out).  Step t of member m opens its forcing with ONE add,
 *     F = drive[t][6] + mforc[t][m]
 * and goes on with the category fmas and the gas fmas exactly as FORCING SCALES above; nothing else of the step differs.
 * All-zero rows give fiveeq_run_forc_* bit for bit (no drive[t][6] being -0); rows uniform over the members, x_t, give
 * fiveeq_run_forc_* on a drive table with F_ext'[t] = fl(drive[t][6] + x_t) formed in kernel precision.  fscale is required
 * as there; unit scale rows with n_fext == 0 (fext NULL) run the rows alone.
 *   form FIVEEQ_FORM_PER_STEP: the row is one more coalesced row load issued with the lane's other rows, w bytes more per
 *       member-step;
 *   form FIVEEQ_FORM_FUSED: the lane loads its element of row t + 1 while it computes step t; w bytes per member-step here too
 *       (the row is streamed, not resident).
 * Packed fp32 lanes load their two members as one 8-byte access (mforc 8-byte aligned and ld even, else the scalar kernels:
 * the same bits).  Every form gives the same bits.  Pool layouts {4} and 4 + 1 + 1, with and without obs / misfit; not under
 * the scenario axis, nor in the small-ensemble, compensated, histogram-ring or concentration-driven forms.  FIVEEQ_E_INVALID
 * for everything fiveeq_run_forc_* refuses, a NULL or misaligned mforc and n_mforc_rows < t_end — before anything is launched. */
int fiveeq_run_mforc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const double *r, const double *q, double *R, double *S,
                         double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                         const double *fscale, const double *fext, int32_t n_fext,
                         const double *obs, double *misfit, const double *mforc, int32_t n_mforc_rows,
                         int32_t form, int32_t k_steps, void *stream);
int fiveeq_run_mforc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const float *r, const float *q, float *R, float *S,
                         float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                         const float *fscale, const float *fext, int32_t n_fext,
                         const double *obs, double *misfit, const float *mforc, int32_t n_mforc_rows,
                         int32_t form, int32_t k_steps, void *stream);
/* fiveeq_plan_create_* of the per-step form above; the plan bakes in fscale, fext, obs, misfit and mforc too */
int fiveeq_plan_create_mforc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                 const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                 const double *r, const double *q, double *R, double *S,
                                 double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                                 const double *fscale, const double *fext, int32_t n_fext,
                                 const double *obs, double *misfit, const double *mforc, int32_t n_mforc_rows,
                                 void **plan_out);
int fiveeq_plan_create_mforc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                 const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                 const float *r, const float *q, float *R, float *S,
                                 float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                                 const float *fscale, const float *fext, int32_t n_fext,
                                 const double *obs, double *misfit, const float *mforc, int32_t n_mforc_rows,
                                 void **plan_out);
/* AR(1) NOISE ROWS — shard-computable per-member internal variability (new; additive): rows[t - t_begin][m] = xi_t of member
 * M = m0 + m for t_begin <= t < t_end, 0 <= m < n_members,
 *     xi_t = phi_m xi_{t-1} + s_m z_t(M)
 * with z_t(M) a counter-based deviate computed in INTEGER arithmetic from (seed, M, t) alone: six splitmix64 words
 * mix64(mix64(seed + 0x9e3779b97f4a7c15 (M + 1)) ^ 0xd1342543de82ef95 (6 (t + 1) + j + 1)), j = 0..5, their twelve 32-bit halves
 * summed (< 2^36, exact), z = (sum - 6 (2^32 - 1)) 2^-32 converted to fp64 exactly: |z| <= 6, mean 0, variance 1 - 2^-64,
 * excess kurtosis -0.1.  The recursion runs in fp64, w = s_m z_t then xi_t = phi_m xi_{t-1} + w, each operation rounded on its
 * own (no fma).  The bits depend on (seed, M, t, phi_m, s_m) only: not on the launch shape, ld, the m0 split, or how the steps
 * are cut into calls.  Layouts:
 *   phi, s    dev [ld]   kernel precision (widened exactly); s = sigma sqrt(1 - phi^2) gives a stationary standard deviation sigma
 *   xi_state  dev [ld]   fp64, in/out: xi_{t_begin - 1} in, xi_{t_end - 1} out
 *   rows      dev [t_end - t_begin][ld]   kernel precision; _f32 rounds xi_t once on store and keeps the fp64 xi_state
 * THE STATIONARY START is the draw at counter t = -1 times sigma_m: the call with [t_begin, t_end) = [-1, 0) runs that one
 * step through the same recursion and stores no row (rows may be NULL); with xi_state zeroed and s = sigma it leaves
 * xi_state = sigma_m z_{-1}(M).  Columns [n_members, ld) of rows and xi_state are not touched.  FIVEEQ_E_INVALID for
 * n_members outside 1..2^31-1, n_members > ld, m0 < 0, a range that is neither 0 <= t_begin <= t_end nor [-1, 0), NULL or
 * misaligned pointers — before anything is launched.  Host twin (bit-identical): fiveeqscm_amd.forcing.ar1_noise_rows_host. */
int fiveeq_noise_rows_f64(uint64_t seed, int64_t m0, int64_t n_members, int64_t ld, int32_t t_begin, int32_t t_end,
                          const double *phi, const double *s, double *xi_state, double *rows, void *stream);
int fiveeq_noise_rows_f32(uint64_t seed, int64_t m0, int64_t n_members, int64_t ld, int32_t t_begin, int32_t t_end,
                          const float *phi, const float *s, double *xi_state, float *rows, void *stream);
/* MINOR-GAS FORCING ROWS — per-member forcing of constant-lifetime species (HFCs, PFCs, SF6, ...) with each member's own
 * lifetime and radiative efficiency (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, sizeof(fiveeq_model) stays 448).  The second
 * generator of member-forcing rows beside fiveeq_noise_rows_*: n_species <= 8 one-pool reservoirs without state dependence,
 * advanced by the exact step R <- R + expm1(-dt / tau) (R - tau c E), their forcing summed into rows[t][m].
 *   n_species                          1..8 species in this call
 *   n_members, ld                      members of the shard, row length of tau, eff, R and rows
 *   n_rows                             steps of the call, >= 0; 0 is a successful no-op after the checks
 *   dt                                 step length (yr), finite and > 0
 *   c      HOST [n_species] fp64       emis2conc (concentration units per emission unit), copied by value into the launch
 *   emis   dev [n_rows][n_species] fp64   emissions of each step, shared by the members
 *   tau    dev [n_species][ld]         kernel precision (widened exactly): each member's lifetime (yr), > 0
 *   eff    dev [n_species][ld]         kernel precision (widened exactly): each member's radiative efficiency
 *   R      dev [n_species][ld] fp64    in/out: the concentration above its baseline before the first step in, after the last out
 *   rows   dev [n_rows][ld]            kernel precision
 *   accumulate                         0: rows are written; 1: the forcing is added onto what the rows hold
 * THE ARITHMETIC is fp64 whatever the kernel precision, each operation rounded on its own (no fma).  Once per call, for species
 * k of member m:   x = -dt / tau_k (IEEE division);   em1 = expm1(x) by the library's own primitive — the value
 * fiveeq_math_probe_f64(op = 0) returns for x;   a = tau_k * c_k.  Per step t, for k ascending:
 *     u = a * emis[t][k];   v = R_k - u;   w = em1 * v;   R_k = R_k + w
 * then, for k ascending from acc = accumulate ? (double)rows[t][m] : 0.0:
 *     p = eff_k * R_k;   acc = acc + p          and   rows[t][m] = acc rounded once to the kernel precision.
 * The bits depend on (tau, eff, c, emis, R, dt) only: not on the launch shape, ld, how the members are cut into shards or how
 * the steps are cut into calls (R carries the state; em1 is recomputed from the same tau).  For fp64 rows, chained accumulate = 1
 * calls over consecutive species groups equal one ordered sum over all species bit for bit; fp32 rows round once per call at
 * the store, so a grouping is part of their definition (fiveeqscm_amd.minor_gases.minor_gas_rows: consecutive groups of 8).
 * Columns [n_members, ld) of rows and R are not touched.  FIVEEQ_E_INVALID for n_species outside 1..8, n_members outside
 * 1..2^31-1, n_members > ld, n_rows < 0, dt not finite or <= 0, a NULL c, a non-finite c[k], accumulate other than 0 or 1,
 * NULL or misaligned pointers (in this order) — before anything is launched.  Host twin (bit-identical given the same em1):
 * fiveeqscm_amd.minor_gases.minor_gas_rows_host. */
int fiveeq_minor_rows_f64(int32_t n_species, int64_t n_members, int64_t ld, int32_t n_rows, double dt, const double *c,
                          const double *emis, const double *tau, const double *eff, double *R, double *rows,
                          int32_t accumulate, void *stream);
int fiveeq_minor_rows_f32(int32_t n_species, int64_t n_members, int64_t ld, int32_t n_rows, double dt, const double *c,
                          const double *emis, const float *tau, const float *eff, double *R, float *rows,
                          int32_t accumulate, void *stream);
/* AEROSOL FORCING ROWS — per-member aerosol forcing (ERFari + ERFaci) from a shared table of short-lived-forcer emissions (SO2,
 * BC, OC, NH3, ...) with each member's own coefficients (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, sizeof(fiveeq_model) stays
 * 448).  The third generator of member-forcing rows beside fiveeq_noise_rows_* and fiveeq_minor_rows_*: a linear
 * aerosol-radiation mix of n_species <= 8 species and one saturating aerosol-cloud term over the species of aci_mask,
 *     rows[t][m] = sum_k ari_k (emis[t][k] - base_k) - beta (ln(1 + sum_mask emis[t][k] / s_k) - ln(1 + sum_mask base_k / s_k)).
 *   n_species                          1..8 species in this call (the cloud term's sum cannot be split across calls)
 *   aci_mask                           bit k set: species k enters the cloud term; no bit at or above n_species; 0: no cloud term
 *   n_members, ld                      members of the shard, row length of ari, shape, beta and rows
 *   n_rows                             steps of the call, >= 0; 0 is a successful no-op after the checks
 *   base   HOST [n_species] fp64       reference (pre-industrial) emissions, finite and >= 0, copied by value into the launch
 *   emis   dev [n_rows][n_species] fp64   emissions of each step, shared by the members, >= 0
 *   ari    dev [n_species][ld]         kernel precision (widened exactly): each member's W m-2 per emission unit
 *   shape  dev [n_species][ld]         kernel precision (widened exactly): each member's s_k in emission units, > 0 with a
 *                                      finite reciprocal; read for the species of aci_mask only
 *   beta   dev [ld]                    kernel precision (widened exactly): each member's cloud-term scale, W m-2
 *   rows   dev [n_rows][ld]            kernel precision
 *   accumulate                         0: rows are written; 1: the forcing is added onto what the rows hold
 * With aci_mask == 0 shape and beta are not read and may be NULL.
 * THE ARITHMETIC is fp64 whatever the kernel precision, each operation rounded on its own (no fma outside the logarithm).  Once
 * per call, for member m:
 *     for k ascending, bit k of aci_mask set:   g_k = 1.0 / s_k          (IEEE division)
 *     x = 0.0;  for k ascending in the mask:    p = g_k * base_k;  x = x + p
 *     y0 = 1.0 + x;   L0 = ln(y0) by the library's own primitive — the value fiveeq_math_probe_f64(op = 2) returns for y0.
 * Per step t:
 *     acc = accumulate ? (double)rows[t][m] : 0.0
 *     for k ascending, k < n_species:           e = emis[t][k] - base_k;  p = ari_k * e;  acc = acc + p
 *     if aci_mask != 0:
 *         x = 0.0;  for k ascending in the mask: p = g_k * emis[t][k];  x = x + p
 *         y = 1.0 + x;  L = ln(y) (the same primitive);  v = L - L0;  w = beta * v;  acc = acc - w
 *     rows[t][m] = acc rounded once to the kernel precision.
 * The bits depend on (emis, base, ari, shape, beta, aci_mask) only: not on the launch shape, ld, how the members are cut into
 * shards or how the steps are cut into calls (there is no state to carry).  A step whose emissions equal base forms L by the
 * operations that formed L0 and contributes exactly +0: a table equal to base at every step gives all-zero rows — by the
 * contract of MEMBER FORCING the run without them, bit for bit.  Domain: emis >= 0, base >= 0, s > 0 with 1 / s finite, so that
 * y >= 1 is finite and normal; the Python wrapper enforces it for emis and the device rows, the kernel does not guard it.
 * Columns [n_members, ld) of rows are not touched.  FIVEEQ_E_INVALID for n_species outside 1..8, an aci_mask that is negative
 * or has a bit at or above n_species, n_members outside 1..2^31-1, n_members > ld, n_rows < 0, a NULL base, a base[k] that is
 * not finite or negative, accumulate other than 0 or 1, NULL or misaligned pointers (shape and beta required iff
 * aci_mask != 0) — in this order, before anything is launched.  Host twin (bit-identical given the same logarithm):
 * fiveeqscm_amd.aerosols.aerosol_rows_host. */
int fiveeq_aerosol_rows_f64(int32_t n_species, int32_t aci_mask, int64_t n_members, int64_t ld, int32_t n_rows,
                            const double *base, const double *emis, const double *ari, const double *shape,
                            const double *beta, double *rows, int32_t accumulate, void *stream);
int fiveeq_aerosol_rows_f32(int32_t n_species, int32_t aci_mask, int64_t n_members, int64_t ld, int32_t n_rows,
                            const double *base, const double *emis, const float *ari, const float *shape,
                            const float *beta, float *rows, int32_t accumulate, void *stream);
/* SEA-LEVEL ROWS — per-member global-mean sea-level rise from the STORED warming rows (and, optionally, the heat-uptake rows H of
 * fiveeq_forcing_rows_*), each member with its own components (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, sizeof(fiveeq_model)
 * stays 448).  A member has n_comp <= 6 components (thermal expansion, glaciers, ice-sheet surface balance and discharge, land
 * water, ...), each of one of two kinds:
 *     relax   dS/dt = (Seq(T) - S) / tau   (Mengel et al. 2016), advanced exactly over one step with the row's T held
 *     rate    dS/dt = Seq(T)               (the semi-empirical form of Rahmstorf 2007)
 * with Seq(T) = (a + b x) x, x = T - T0, capped from above at cap (finite ice; +inf: no cap).  The pass is unit-agnostic.
 *   n_scen                              1..64 scenarios, all in one launch; the parameters and eta are shared by them
 *   n_comp                              1..6 components
 *   rate_mask                           bit j set: component j is of kind rate; no bit at or above n_comp
 *   n_members, ld                       members of the shard; row length of par, eta and S_io
 *   n_rows                              rows of the call, each ONE model step after the one before, >= 0; 0 is a successful
 *                                       no-op after the checks
 *   dt                                  the model step, finite and > 0
 *   T_rows dev                          the stored warming in the kernel precision (widened exactly): element (s, t, m) at
 *                                       T_rows[s t_scen_stride + t t_row_stride + m]; both strides >= ld
 *   par    dev [5][n_comp][ld] fp64     tau, a, b, T0, cap in this order; tau is read for the relax components only (> 0)
 *   heat   dev fp64, may be NULL        H: element (s, t, m) at heat[s h_scen_stride + t h_row_stride + m], strides >= ld
 *   eta    dev [ld] fp64                each member's expansion efficiency; required iff heat is given, not read without it
 *   S_io   dev [n_scen][n_comp][ld] fp64   every component's state before the first row in, after the last row out
 *   total  dev [n_scen][n_rows][ld_out] fp64
 *   comps  dev [n_scen][n_rows][n_comp][ld_out] fp64, may be NULL: the component rows
 *   ld_out                              row length of total and comps, >= n_members
 * THE ARITHMETIC is fp64 whatever the kernel precision, each operation rounded on its own (no fma).  Once per call, for each
 * relax component j of member m:   x = -dt / tau_j (IEEE division);   em1_j = expm1(x) by the library's own primitive — the
 * value fiveeq_math_probe_f64(op = 0) returns for x.  Per scenario s and row t, with Tt = (double)T[s][t][m], for j ascending:
 *     x = Tt - T0_j;  p = b_j * x;  c = a_j + p;  e = c * x;  if (e > cap_j) e = cap_j;        (a NaN e stays NaN)
 *     relax:  v = S_j - e;  w = em1_j * v;  S_j = S_j + w
 *     rate:   w = dt * e;   S_j = S_j + w
 * then   acc = heat ? eta * H[s][t][m] : 0.0;   for j ascending: acc = acc + S_j;   total[s][t][m] = acc;
 * comps[s][t][j][m] = S_j.  After the last row S_io holds S.  Components at or above n_comp do not exist: they are skipped,
 * not computed with neutral values.
 * The bits depend on (T, H, eta, par, S, dt) only: not on the launch shape, ld, how the members are cut into shards or how the
 * rows are cut into calls (S_io carries the state, em1 is recomputed from the same tau).  A NaN in a member's T row makes that
 * member's state NaN from that row on and touches no other member.  Columns [n_members, ld) of S_io and [n_members, ld_out) of
 * total and comps are not touched.  FIVEEQ_E_INVALID for n_scen outside 1..64, n_comp outside 1..6, a rate_mask that is negative
 * or has a bit at or above n_comp, n_members outside 1..2^31-1, ld < n_members, n_rows < 0, a dt that is not finite and > 0,
 * t_row_stride or t_scen_stride < ld, with heat: h_row_stride or h_scen_stride < ld, then a NULL eta; ld_out < n_members; NULL
 * T_rows, par, S_io or total; misaligned pointers (the kernel precision's size for T_rows, 8 bytes for the others) — in this
 * order, before anything is launched.  Host twin (bit-identical given the same expm1):
 * fiveeqscm_amd.sea_level.sea_level_rows_host. */
int fiveeq_sea_level_rows_f64(int32_t n_scen, int32_t n_comp, int32_t rate_mask, int64_t n_members, int64_t ld, int32_t n_rows,
                              double dt, const double *T_rows, int64_t t_row_stride, int64_t t_scen_stride, const double *par,
                              const double *heat, int64_t h_row_stride, int64_t h_scen_stride, const double *eta, double *S_io,
                              double *total, double *comps, int64_t ld_out, void *stream);
int fiveeq_sea_level_rows_f32(int32_t n_scen, int32_t n_comp, int32_t rate_mask, int64_t n_members, int64_t ld, int32_t n_rows,
                              double dt, const float *T_rows, int64_t t_row_stride, int64_t t_scen_stride, const double *par,
                              const double *heat, int64_t h_row_stride, int64_t h_scen_stride, const double *eta, double *S_io,
                              double *total, double *comps, int64_t ld_out, void *stream);
/* FORCING SCALES UNDER THE SCENARIO AXIS (new; additive, FIVEEQ_ABI_VERSION stays 13): fiveeq_run_scen_* / fiveeq_plan_create_scen_*
 * with the forcing scales of fiveeq_run_forc_*.  The arguments of the scenario calls, then
 *   fscale dev [G + n_fext][ld]          SHARED by the scenarios, like r and q
 *   fext   dev [n_scen][n_steps][4]      one category table per scenario (aerosol and other external forcings differ from one
 *                                        scenario to the next); may be NULL iff n_fext == 0
 * then form, k_steps, stream (or plan_out).  Member-scenario (m, s) is bit for bit member m of fiveeq_run_forc_* (obs = misfit =
 * NULL) run with scenario s's drive table and category table, in both forms, fp32 packed or not.
 *   form FIVEEQ_FORM_PER_STEP: the lane loads its G + n_fext scale rows ONCE beside its parameter rows for all scenarios —
 *       w (G + n_fext) / n_scen bytes more per member-scenario-step — and reads scenario s's table record with scalar loads;
 *   form FIVEEQ_FORM_FUSED: a grid row of workgroups per scenario, each staging its own scenario's table chunk.
 * Pool layouts {4} and 4 + 1 + 1; no misfit.  FIVEEQ_E_INVALID for a NULL or misaligned fscale, n_fext outside
 * 0..fiveeq_max_fext(), a NULL fext with n_fext > 0, n_scen outside 1..fiveeq_max_scenarios(), a layout without the forcing
 * form, an unknown form, k_steps < 0 or a step range outside [0, n_steps) — before anything is launched. */
int fiveeq_run_scen_forc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                             const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                             const double *r, const double *q, double *R, double *S,
                             double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                             const double *fscale, const double *fext, int32_t n_fext,
                             int32_t form, int32_t k_steps, void *stream);
int fiveeq_run_scen_forc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                             const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                             const float *r, const float *q, float *R, float *S,
                             float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                             const float *fscale, const float *fext, int32_t n_fext,
                             int32_t form, int32_t k_steps, void *stream);
/* fiveeq_plan_create_* of the per-step form above; the plan bakes in fscale and fext too */
int fiveeq_plan_create_scen_forc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                                     const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                     const double *r, const double *q, double *R, double *S,
                                     double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                                     const double *fscale, const double *fext, int32_t n_fext, void **plan_out);
int fiveeq_plan_create_scen_forc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld, int32_t n_scen,
                                     const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                     const float *r, const float *q, float *R, float *S,
                                     float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                                     const float *fscale, const float *fext, int32_t n_fext, void **plan_out);
/* 1 if the pool layout has the forcing forms above, else 0 */
int fiveeq_forcing_layout_supported(int32_t n_gas, const int32_t *n_pools);
/* the largest n_fext the forcing forms take (4) */
int32_t fiveeq_max_fext(void);

/* SMALL ENSEMBLES (BASELINE configs[1], 10k CO2-only members): the time-fused step with ONE MEMBER
 * SPREAD OVER SEVERAL LANES.  An ensemble of fewer waves than the chip has SIMDs (1024) is bound by the number of
 * instructions one wave issues per step; with lanes_per_member = 4 (pool layouts {4}: a lone 4-pool gas) lane 4m + i carries
 * pool i of member m — one expm1 chain per wave-step instead of four, the two sums over pools folded with DPP moves in the
 * per-step kernel's order ((R0 + R1) + R2) + R3 — and the shared model stays in registers instead of LDS.  4x the waves of
 * fiveeq_run_fused_*, 16 members per wave.  lanes_per_member: 4, 8 (new, ABI v11: the 4 + 1 + 1 layout on an OCTET of lanes —
 * gas 0's four pools on lanes 0-3, the single pools of gases 1 and 2 on lanes 4 and 5: every lane runs one gas's closure, one
 * expm1 chain and one forcing, a third of the one-lane form's instructions per wave; T_stats must be NULL for it), 1 (one member
 * per lane with the model in registers: every compiled layout, several gases included) or 0 = the widest form the layout has
 * (fiveeq_small_lanes; the one-lane form when a 4 + 1 + 1 run asks for statistics).  One launch for the
 * whole span; C_traj, T_traj, the row map and T_stats as in the other entry points (the statistics records are the fused
 * kernel's bit for bit).  Same arithmetic operation for operation: bit-identical results to the per-step path.
 * Ahead of the fused kernel while the ensemble is launch-bound — about 64 members per CU for the quad form, a few hundred
 * thousand members for the one-lane form (10k members, us per step: CO2-only fp64 0.42 against 0.73, three gases fp64 0.94
 * against 1.38, fp32 0.51 against 1.16). */
int fiveeq_run_small_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const double *r, const double *q, double *R, double *S,
                         double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                         int32_t lanes_per_member, void *stream);
int fiveeq_run_small_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const float *r, const float *q, float *R, float *S,
                         float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                         int32_t lanes_per_member, void *stream);
/* new (ABI v11) — THE COMPENSATED fp32 FORM of the time-fused kernel (opt-in; BASELINE configs[4]'s natural mode: 100M fp32
 * members with the state in registers).  Two changes against fiveeq_run_fused_f32 / fiveeq_run_ksteps_f32 / _fused_bins_f32,
 * whose arguments it takes (k_steps: steps per launch, >= t_end - t_begin = one launch; bin_ring = NULL: no histogram ring and
 * lo / hi / n_bins / ring_rows are ignored):
 *   (1) every POOL carries a second register word holding the rounding error of its own update, fed back into the next one
 *       (Kahan's summation with the increment's product fused into the first add): +3 instructions per pool and step, NO HBM
 *       bytes — the words start at zero in every launch and are dropped at its end, so R / S in memory stay plain fp32 rows (a
 *       run relaunched every k_steps steps loses at most one rounding per pool and launch).  The two thermal boxes are not
 *       compensated: once (2) is in place their rounding is 4e-7 of T;
 *   (2) the forcing is computed from the EXCESS C - C0 = sum_i R_i, not from the rounded C: ln(C/C0) as log1p((C - C0)/C0),
 *       sqrt(C) - sqrt(C0) as (C - C0) / (sqrt(C) + sqrt(C0)).  In fp32 the default form loses the small excess of the first
 *       decades to the rounding of C itself, and THAT is what bounds T in fp32, not the state.
 * Worst relative error against 50-digit arithmetic over the 24 golden members x 750 steps: C 2.9e-6 -> 1.8e-7 (the rounding of
 * the stored C itself), T (1e-2 K floor) 1.7e-5 -> 7e-7; cost on the VALU-bound fused kernel: profiles/r06/fp32_compensated.txt.
 * It is its own arithmetic: results are NOT bit-identical to the default forms (which stay bit-identical among themselves), and
 * the kernels that keep the state in HBM (step / run / run_bins / plan) do not have it. */
int fiveeq_run_fused_comp_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                              const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                              const float *r, const float *q, float *R, float *S,
                              float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, int32_t k_steps,
                              double lo, double hi, int32_t n_bins, uint16_t *bin_ring, int32_t ring_rows, void *stream);
/* new (ABI v11) — the same compensated arithmetic on the SMALL-ENSEMBLE kernel (one member per lane, the model in registers; every
 * compiled layout): what a launch-bound fp32 ensemble takes instead of the fused kernel (10k three-gas members: about half the
 * time per step).  One launch for the whole span; arguments of fiveeq_run_fused_f32; the words are dropped at the end of the call. */
int fiveeq_run_small_comp_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                              const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                              const float *r, const float *q, float *R, float *S,
                              float *C_traj, float *T_traj, int32_t n_rows, double *T_stats, void *stream);
/* lanes per member of the widest small-ensemble form compiled for (n_gas, n_pools[]): 4 (a lone 4-pool gas), 8 (4 + 1 + 1),
 * 1 (every other compiled layout), or 0 = the layout has no kernel at all */
int32_t fiveeq_small_lanes(int32_t n_gas, const int32_t *n_pools);

/* The fp32 entry points (step / run / run_fused / run_ksteps / run_*bins / plan_create _f32) compute TWO members per
 * lane with packed fp32 instructions and 8-byte row accesses whenever the rows allow it (ld even, every row pointer
 * 8-byte aligned, n_members >= 2), and one member per lane otherwise; both give the same bits.  This switch forces the
 * one-member-per-lane kernels (on = 0) or re-enables packing (on != 0, the default); returns the previous setting.
 * Process-wide (an atomic word, see CONVENTIONS); meant for measurements and tests. */
int fiveeq_set_f32_packing(int on);

/* CACHE POLICY OF THE PER-STEP KERNEL'S ROWS (new).  The step / run / plan_create entry points read every state and parameter
 * row once per step.  While those rows fit the 256 MiB Infinity Cache they are served from it at the next step (the default
 * policy; what a chunk-major schedule arranges for large ensembles).  A launch whose rows cannot survive until the next step
 * takes the STREAMED form instead: the same kernel with non-temporal loads and stores (bit-identical results; -4.5 % per step
 * at 8M fp64 members, -9 % at 4M; +11...13 % — the wrong form — on a cache-resident 1-2M-member ensemble).
 * FIVEEQ_ROWS_AUTO (the default) decides per call: streamed when n_members x (SP + 2 + 3G + 2) words >= the cache AND
 * ld x the same >= twice the cache (ld = the row length: the whole ensemble this call's members are a sub-range of).
 * fiveeq_set_row_policy forces one form process-wide (an atomic word read once per call, see CONVENTIONS; returns the previous
 * setting, or FIVEEQ_E_INVALID for a value that is none of the three) — meant for measurements and tests.
 * fiveeq_rows_streamed: 1 / 0 = the form a per-step launch of that shape would take now.  The stored C / T rows are written
 * non-temporally in every form (written once, never re-read by a stepping kernel).  The streamed-histogram per-step form
 * (fiveeq_run_bins_*) always takes the default policy. */
#define FIVEEQ_ROWS_CACHED      0
#define FIVEEQ_ROWS_STREAMED    1
#define FIVEEQ_ROWS_AUTO        2
int fiveeq_set_row_policy(int32_t policy);
int fiveeq_rows_streamed(int32_t n_gas, const int32_t *n_pools, int64_t n_members, int64_t ld, int32_t word_bytes);

/* CONCENTRATION-DRIVEN (inverse) mode (the reference's module name
 * `concentrations` hints at it, no reference code exists).  drive[t][0..2] hold the TARGET
 * concentration of each gas at the end of step t (shared by all members; columns 3..5 unused);
 * cumE dev [G][ld] is per-member cumulative-emission state (in/out, start at 0); the emission rate
 * that reaches the target is diagnosed per member and step from the same pool equations and
 * written to E_traj dev [n_rows][G][ld] (row map as above); pools, boxes, T and T_stats advance
 * exactly as in the forward path.  One launch for the whole span (time-fused form). */
int fiveeq_run_inverse_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const double *r, const double *q, double *R, double *S, double *cumE,
                           double *E_traj, double *T_traj, int32_t n_rows, double *T_stats, void *stream);
int fiveeq_run_inverse_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const float *r, const float *q, float *R, float *S, float *cumE,
                           float *E_traj, float *T_traj, int32_t n_rows, double *T_stats, void *stream);

/* CONCENTRATION-DRIVEN RUNS WITH FORCING SCALES AND THE IN-LOOP MISFIT (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, no existing
 * prototype or struct changes, sizeof(fiveeq_model) stays 448).  The arguments of fiveeq_run_inverse_*, then fscale, fext,
 * n_fext of FORCING SCALES and obs, misfit of CONSTRAINED RUNS above (the same layouts), then stream.  The gas step is the
 * inverse step as it stands: the target concentrations are reached whatever the scales, E_traj and cumE do not see them in
 * the step that forms them.  The forcing of the step is accumulated as in the forward forcing form,
 *     F = drive[t][6];   F = fma(sx_k, fext[t][k], F), k = 0 .. n_fext-1;   F = fma(sg_g, F_g, F), g = 0 .. G-1
 * with F_g the forcing of the concentration gas g reached, so T, the boxes — and through T the next step's emissions — carry
 * the member's scales; the misfit is accumulated from T exactly as in the forward forms.
 *   fscale  may be NULL: no scales; then n_fext must be 0 (fext is not read);
 *   obs, misfit  both NULL (no misfit) or both set;
 *   all three NULL: the call IS fiveeq_run_inverse_* (the same kernel).
 * Unit scales with n_fext == 0, or with an all-zero table, give fiveeq_run_inverse_* bit for bit; obs / misfit change nothing
 * but the misfit rows.  One launch for the whole span: the scales stay on chip, the table chunk is staged through LDS beside
 * the drive chunk, the accumulators cross HBM once.  One member per lane in both precisions.  Pool layouts {4} and 4 + 1 + 1
 * for the scales and for the misfit (any compiled layout with all three NULL).  FIVEEQ_E_INVALID, in this order and before
 * anything is launched: the base arguments as fiveeq_run_inverse_* reports them, a NULL cumE, n_fext outside 0..4, a NULL
 * fscale with n_fext > 0, a misaligned fscale, a NULL fext with n_fext > 0, a misaligned fext, a layout without the forcing
 * form, exactly one of obs / misfit set, misaligned obs / misfit, a layout without the misfit form. */
int fiveeq_run_inverse_forc_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const double *r, const double *q, double *R, double *S, double *cumE,
                                double *E_traj, double *T_traj, int32_t n_rows, double *T_stats,
                                const double *fscale, const double *fext, int32_t n_fext,
                                const double *obs, double *misfit, void *stream);
int fiveeq_run_inverse_forc_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                const float *r, const float *q, float *R, float *S, float *cumE,
                                float *E_traj, float *T_traj, int32_t n_rows, double *T_stats,
                                const float *fscale, const float *fext, int32_t n_fext,
                                const double *obs, double *misfit, void *stream);

/* MIXED DRIVE — emission-driven and concentration-driven gases in one run (new; ADDITIVE: FIVEEQ_ABI_VERSION stays 13, no existing
 * prototype or struct changes, sizeof(fiveeq_model) stays 448).  conc_mask selects the driver of each gas: bit g set, gas g is
 * CONCENTRATION-DRIVEN; bit g clear, EMISSION-DRIVEN.  The arguments are those of fiveeq_run_inverse_forc_* with conc_mask behind
 * T_stats.  One drive table [n_steps][8] as everywhere:
 *   an emission-driven gas       drive[t][g] = E_g, drive[t][3 + g] = the shared cumulative emissions BEFORE step t (the forward
 *                                convention); row g of X_traj [n_rows][G][ld] receives C_g; cumE row g is NEVER READ AND NEVER
 *                                WRITTEN;
 *   a concentration-driven gas   drive[t][g] = the target concentration at the end of step t, drive[t][3 + g] is not read (the
 *                                inverse convention); cumE row g is the member's cumulative emissions (in/out, start at 0); row g
 *                                of X_traj receives the diagnosed E_g.
 * Each gas takes the forward or the inverse gas step exactly as it stands; the forcing is accumulated in the order of the other
 * forms (drive[t][6], the categories, then gases 0 .. G-1), the thermal step is unchanged.  fscale, fext, n_fext, obs and misfit
 * follow the NULL rules of fiveeq_run_inverse_forc_*.  Time-fused: one launch for the span, one member per lane in both
 * precisions.  By the mask:
 *   conc_mask == 0             the call IS the forward time-fused call on these arguments — fiveeq_run_fused_*, or
 *                              fiveeq_run_forc_* (with scales) / fiveeq_run_obs_* (misfit alone) with FIVEEQ_FORM_FUSED and
 *                              k_steps = 0 — bit for bit; cumE may be NULL;
 *   conc_mask == (1 << G) - 1  the call IS fiveeq_run_inverse_forc_*, bit for bit;
 *   a proper mask              the mixed kernels: pool layout 4 + 1 + 1, all six masks, with and without the scales and the misfit.
 * Refused before anything is launched, in this order: FIVEEQ_E_INVALID for the base arguments as fiveeq_run_inverse_* reports
 * them; a negative conc_mask; a conc_mask with a bit at or above n_gas; a NULL cumE with a non-zero conc_mask; then every refusal
 * of fiveeq_run_inverse_forc_* from n_fext on, in its order; last, FIVEEQ_E_UNSUPPORTED for a proper mask on a pool layout without
 * the mixed form.  fiveeq_mixed_layout_supported: 1 when fiveeq_run_mixed_* runs conc_mask on the layout (masks 0 and all-gases
 * on every compiled layout), else 0 — a negative mask or one with a bit at or above n_gas included. */
int fiveeq_run_mixed_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const double *r, const double *q, double *R, double *S, double *cumE,
                         double *X_traj, double *T_traj, int32_t n_rows, double *T_stats,
                         int32_t conc_mask, const double *fscale, const double *fext, int32_t n_fext,
                         const double *obs, double *misfit, void *stream);
int fiveeq_run_mixed_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                         const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                         const float *r, const float *q, float *R, float *S, float *cumE,
                         float *X_traj, float *T_traj, int32_t n_rows, double *T_stats,
                         int32_t conc_mask, const float *fscale, const float *fext, int32_t n_fext,
                         const double *obs, double *misfit, void *stream);
int fiveeq_mixed_layout_supported(int32_t n_gas, const int32_t *n_pools, int32_t conc_mask);

/* Ensemble form of the reference's one function,
 *   calculate_hfc_conc(emissions, time, lifetime) = emissions[0]*exp(-time)
 * (U_FaIR/concentrations.py:4-5): out[k][m] = e0[m] * exp(-time[k]).
 *   e0 dev [n_members], time dev [n_time], out dev [n_time][ld]. */
int fiveeq_hfc_conc_f64(int64_t n_members, int64_t ld, int32_t n_time,
                        const double *e0, const double *time, double *out, void *stream);

/* new — fixed-bin histograms of stored rows, for all-timestep percentiles with a tiny exchange
 * (SURVEY.md section 8e-ii): hist[row][b] += number of members with lo + b*w <= rows[row][m] < lo + (b+1)*w,
 * w = (hi - lo)/n_bins; values outside [lo, hi) are counted in the edge bins, NaNs are skipped.
 * THE BIN RULE, shared bit for bit by every entry point that bins a value (these, the bin indices of fiveeq_run_*bins_*,
 * the summary's selection): with inv_w = n_bins/(hi - lo),
 *   _f64:  bin = trunc(clamp((x - lo) * inv_w, 0, n_bins - 1))                        evaluated in fp64
 *   _f32:  bin = trunc(clamp(fma(x, (float)inv_w, (float)(-lo*inv_w)), 0, n_bins - 1)) evaluated in fp32 (one FMA per
 *          member).  Monotone in x like the fp64 formula; against it a member changes bin only within
 *          ~2^-23 * max(|lo|, |hi|) * inv_w of a bin edge (in bins): 2^-12 bin for a range that starts near zero such as
 *          temperature anomalies, 0.01 bin for lo = 280, hi = 295, n_bins = 4096 — express rows in absolute units far from zero
 *          as anomalies, or keep them in fp64, if that matters.
 *   rows dev [n_rows][ld] (e.g. T_traj), hist dev [n_rows][n_bins] uint64, ACCUMULATED INTO (zero it first;
 *   several shards / calls may add into the same histogram), 1 <= n_bins <= 4096, n_rows <= 65535. */
int fiveeq_hist_rows_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                         double lo, double hi, int32_t n_bins, uint64_t *hist, void *stream);
int fiveeq_hist_rows_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                         double lo, double hi, int32_t n_bins, uint64_t *hist, void *stream);
/* new — the END-OF-RUN SUMMARY as HIP passes (form (i): exact percentiles of T at selected output
 * times over ALL members by SELECTION, so that the ensemble does not travel; host side: fiveeqscm_amd/distributed.py).
 * All three read rows dev [n_rows][ld] once, 16 bytes per lane and load.
 *
 * (1) moments dev [n_rows][4] fp64 = (sum, sum of squares, min, max) of each row's n_members values — fp64 sums of the
 *     exactly converted elements in a fixed order (same bits every run); min / max ignore NaNs, the sums propagate them.
 *     partial dev [n_rows][K][4] fp64 is workspace, K = fiveeq_row_moments_chunks(n_rows, n_members). */
int64_t fiveeq_row_moments_chunks(int32_t n_rows, int64_t n_members);
int fiveeq_row_moments_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                           double *partial, double *moments, void *stream);
int fiveeq_row_moments_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                           double *partial, double *moments, void *stream);
/* (2) fiveeq_hist_rows_* with a range PER ROW read from device memory — ranges dev [n_rows][2] fp64 = (lo, hi), e.g. each
 *     row's global extrema, so that no host round trip sits between the moments and the histogram; a row with hi <= lo is
 *     constant and is counted in bin 0. */
int fiveeq_hist_rows_ranged_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                                const double *ranges, int32_t n_bins, uint64_t *hist, void *stream);
int fiveeq_hist_rows_ranged_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                                const double *ranges, int32_t n_bins, uint64_t *hist, void *stream);
/* (3) selection.  The histogram of (2) holds exact counts and the bin rule is monotone in the value, so the order statistic
 *     of global index i lies in the bin b with cdf[b-1] <= i < cdf[b] and is the (i - cdf[b-1])-th smallest member of it.
 *     binmask dev [n_rows][ceil(n_bins/32)] uint32 marks, per row, the bins that hold wanted order statistics (bit b%32 of
 *     word b/32); the pass recomputes every member's bin with the rule and the ranges of (2), bit for bit, and appends the
 *     members of marked bins — the candidates — to cand dev [n_rows][cap] (any order within a row).  cand_n dev [n_rows]
 *     uint64, ACCUMULATED INTO, counts the candidates FOUND; those beyond cap are counted but not stored. */
int fiveeq_select_bins_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                           const double *ranges, int32_t n_bins, const uint32_t *binmask,
                           double *cand, int64_t cap, uint64_t *cand_n, void *stream);
int fiveeq_select_bins_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                           const double *ranges, int32_t n_bins, const uint32_t *binmask,
                           float *cand, int64_t cap, uint64_t *cand_n, void *stream);
/* (4) pick: the order statistics, read off the candidates without sorting them.  ranks dev [n_rows][n_targets] int64: where
 *     each target sits among the row's candidates in ascending order (host bookkeeping on the histogram: the members of
 *     marked bins below the target's bin, plus i - cdf[b-1]); one workgroup per (row, target) finds the candidate of that
 *     rank by radix selection.  pool dev [n_rows][n_seg][width]: the candidates as they arrived, seg_n dev [n_rows][n_seg]
 *     valid entries per segment (one segment: cand / cand_n of (3); on the root of a multi-rank exchange: one segment per
 *     rank).  A segment holds at most `width` STORED candidates: seg_n entries beyond width (cand_n of (3) counts what it
 *     found, also past cap) are taken as width.  picked dev [n_rows][n_targets] fp64; NaN where the rank is negative or not
 *     below the number of stored candidates. */
int fiveeq_select_pick_f64(int32_t n_rows, int32_t n_seg, int64_t width, const double *pool, const uint64_t *seg_n,
                           int32_t n_targets, const int64_t *ranks, double *picked, void *stream);
int fiveeq_select_pick_f32(int32_t n_rows, int32_t n_seg, int64_t width, const float *pool, const uint64_t *seg_n,
                           int32_t n_targets, const int64_t *ranks, double *picked, void *stream);

/* new — WEIGHTED SUMMARY: the passes above over (value, weight) pairs, for importance-weighted ensembles (DESIGN.md section
 * 3.11; host side: fiveeqscm_amd/distributed.py gather_weighted_summary, weights: fiveeqscm_amd/constrain.py
 * importance_weights).  Additive: no symbol above changes.
 *
 * DEFINITION.  A row x of n members over all ranks carries INTEGER weights w, 0 <= w_i <= 2^32, n < 2^31, W = sum w < 2^63.
 * Integer sums are exact and order-independent, so atomics, shard splits and all-reduces cannot change a bit of what follows.
 *   percentile p   the smallest x_i with  sum_{x_j <= x_i} w_j >= k_p  (the inverted CDF), where
 *                  k_p = max(1, ceil(p / 100 * W)) with p taken as the EXACT rational value of the number handed in and the
 *                  product evaluated in integer / rational arithmetic on the host: no floating-point product decides a rank.
 *   weight 0       the member does not exist, whatever its value (NaN and +-inf included).
 *   NaN, w > 0     the row's percentiles, mean and std are NaN (min / max ignore the NaN).
 *   W == 0         over all ranks: an error (ValueError on every rank).
 *   moments        mean = sum w x / W, var = sum w x^2 / W - mean^2, min / max over the members with w > 0; the three sums
 *                  (and sum w^2) accumulated in fp64 in a fixed order per rank, merged over the ranks in rank order.
 *   ess            W^2 / sum w^2 (fp64);  count = the members with w > 0;  weight_sum = W, exact.
 * weights dev [n_members] uint64, shared by the rows; rows dev [n_rows][ld] as above.  Pointers must be aligned to their
 * element size; rows, ld * sizeof(element) and weights aligned to 16 bytes get 16-byte loads.
 *
 * (1w) moments dev [n_rows][8], words of 8 bytes: 0 sum w x, 1 sum w x^2, 2 sum w^2, 3 min, 4 max (fp64; members with
 *      w > 0) | 5 count of w > 0, 6 flags (bit 0: a NaN value with w > 0; bit 1: a weight above 2^32 — the caller's
 *      error), 7 sum w (uint64 bit patterns).  partial dev [n_rows][K][8] is workspace, K = fiveeq_wrow_moments_chunks. */
int64_t fiveeq_wrow_moments_chunks(int32_t n_rows, int64_t n_members);
int fiveeq_wrow_moments_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows, const uint64_t *weights,
                            double *partial, double *moments, void *stream);
int fiveeq_wrow_moments_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows, const uint64_t *weights,
                            double *partial, double *moments, void *stream);
/* (2w) hist[row][b] += the WEIGHT of the members with w > 0 in bin b — THE BIN RULE above with ranges dev [n_rows][2] fp64 =
 *      (lo, hi) read from device memory (the extrema of (1w)); hi <= lo: bin 0; a NaN has no bin.  hist dev
 *      [n_rows][n_bins] uint64, ACCUMULATED INTO; 1 <= n_bins <= 4096. */
int fiveeq_whist_rows_ranged_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows, const uint64_t *weights,
                                 const double *ranges, int32_t n_bins, uint64_t *hist, void *stream);
int fiveeq_whist_rows_ranged_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows, const uint64_t *weights,
                                 const double *ranges, int32_t n_bins, uint64_t *hist, void *stream);
/* (3w) selection: the (value, weight) pairs of the members with w > 0 in the bins binmask marks (as in (3)) are appended to
 *      cand / candw dev [n_rows][cap] (same place in both, any order within a row); cand_n dev [n_rows] uint64, ACCUMULATED
 *      INTO, counts the candidates FOUND; those beyond cap are counted but not stored.  The weighted histogram does not
 *      count members: size cap from the count of w > 0 of (1w). */
int fiveeq_wselect_bins_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double *rows, const uint64_t *weights,
                            const double *ranges, int32_t n_bins, const uint32_t *binmask,
                            double *cand, uint64_t *candw, int64_t cap, uint64_t *cand_n, void *stream);
int fiveeq_wselect_bins_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float *rows, const uint64_t *weights,
                            const double *ranges, int32_t n_bins, const uint32_t *binmask,
                            float *cand, uint64_t *candw, int64_t cap, uint64_t *cand_n, void *stream);
/* (4w) pick: picked[row][q] = the smallest candidate x whose cumulative candidate weight (candidates <= x) reaches
 *      targets[row][q] >= 1 — host bookkeeping on the histogram of (2w): the weight of the marked bins below the
 *      percentile's bin, plus k_p minus the weight of all bins below it.  One workgroup per (row, target), radix selection
 *      on sums of weight, no sort, any number of candidates (the whole row when every member fell into one bin).  pool /
 *      poolw dev [n_rows][n_seg][width], seg_n dev [n_rows][n_seg] as in (4).  picked dev [n_rows][n_targets] fp64; NaN
 *      where the target is below 1 or above the candidates' weight. */
int fiveeq_wselect_pick_f64(int32_t n_rows, int32_t n_seg, int64_t width, const double *pool, const uint64_t *poolw,
                            const uint64_t *seg_n, int32_t n_targets, const int64_t *targets, double *picked, void *stream);
int fiveeq_wselect_pick_f32(int32_t n_rows, int32_t n_seg, int64_t width, const float *pool, const uint64_t *poolw,
                            const uint64_t *seg_n, int32_t n_targets, const int64_t *targets, double *picked, void *stream);

/* new — RESAMPLING: (members, integer weights) -> a dense, equal-weight ensemble of M members, for branching, checkpointing
 * and unweighted tools (host side: fiveeqscm_amd/constrain.py resample, EnsembleEngine.resampled).
 * Additive: no symbol above changes, FIVEEQ_ABI_VERSION stays 13.
 *
 * DEFINITION.  Systematic resampling in integer arithmetic, so that shard splits, atomics and the world size cannot change
 * a bit.  Members m = 0 .. n-1 over all ranks in rank order; integer weights 0 <= w_m <= 2^32, n < 2^31, 1 <= W = sum w < 2^63
 * (the contract of WEIGHTED SUMMARY); c_m = sum_{i <= m} w_i the inclusive cumulative weight.  M outputs, 1 <= M < 2^31, and an
 * integer offset rho, 0 <= rho < W.  Output j (0 <= j < M) sits at the position
 *     p_j = floor((j W + rho) / M)
 * and is a copy of source(j) = the first m with c_m > p_j.  Hence a member of weight 0 is never drawn, member m is drawn
 * floor(M w_m / W) or ceil(M w_m / W) times, and the outputs come in non-decreasing source order.
 *   overflow-free  the host splits W = q M + s and rho = a M + b (0 <= s, b < M; arbitrary-precision integers); then
 *                  p_j = j q + a + (j s + b) div M, with j s + b < 2^62 and j q + a <= p_j < W: 64-bit on the device.
 *   shards         a rank whose members own the cumulative range [C_lo, C_hi) owns the outputs [j(C_lo), j(C_hi)),
 *                  j(C) = min(M, max(0, ceil((C M - rho) / W))) on the host.  The ranks' output shards concatenated in rank
 *                  order are the global list — for every world size and split, with empty shards and shards of zero mass.
 *   masks          weights in {0, 1}, M = W, rho = 0: p_j = j, and the output is the accepted members, each once, in order.
 *   offset         rho = (the first 8 bytes, little-endian, of sha256("<seed>:<M>:<W>")) mod W; no seed: rho = 0.
 *
 * (1r) scan: cum[m] = w_0 + ... + w_m (modulo 2^64), m < n_members; cum[n_members - 1] is the shard's weight sum.  flags dev
 *      [1] is WRITTEN: bit 1 (the convention of (1w)) when a weight is above 2^32 — the caller's error, and cum then means
 *      nothing.  Reduce, then scan: tile sums, a scan of the tile sums by one workgroup, tile scans — three launches ordered
 *      by the stream; no kernel waits on another workgroup.  Integer sums: the same bits in any order.  partial dev
 *      [fiveeq_wscan_chunks(n_members)] uint64 is workspace (two words per tile of 1024 weights).  weights / cum aligned to 16
 *      bytes get 16-byte accesses.  1 <= n_members < 2^31. */
int64_t fiveeq_wscan_chunks(int64_t n_members);
int fiveeq_wscan(int64_t n_members, const uint64_t *weights, uint64_t *partial, uint64_t *cum, uint64_t *flags, void *stream);
/* (2r) pick: src[k] = the first LOCAL member m with cum[m] > p_{j0 + k} - c_lo, k < n_out: the upper bound of the position in
 *      this shard's scan, c_lo the weight of the shards before it.  (M, q, a, s, b) as above; [j0, j0 + n_out) must be the
 *      shard's own outputs (a position outside the shard's range is clamped to its first / last member: src always holds
 *      valid indices).  src dev [n_out] int32.  1 <= M < 2^31, 0 <= s, b < M, q, a, j0, n_out >= 0, j0 + n_out <= M, and
 *      the last position below 2^63.  n_out == 0: nothing to do. */
int fiveeq_resample_pick(int64_t n_members, const uint64_t *cum, uint64_t c_lo, int64_t M, int64_t q, int64_t a, int64_t s,
                         int64_t b, int64_t j0, int64_t n_out, int32_t *src, void *stream);
/* (3r) gather: rows_out[r][k] = rows_in[r][src[k]], r < n_rows, k < n_out, all rows in one launch.  rows_in dev
 *      [n_rows][ld_in], rows_out dev [n_rows][ld_out], ld_out >= n_out; nothing is written beyond column n_out.  0 <= src[k] <
 *      ld_in (a column whose index is not is left unwritten and nothing is read for it).  n_out == 0 or n_rows == 0:
 *      nothing to do. */
int fiveeq_gather_rows_f64(int32_t n_rows, int64_t n_out, int64_t ld_in, const double *rows_in, int64_t ld_out, double *rows_out,
                           const int32_t *src, void *stream);
int fiveeq_gather_rows_f32(int32_t n_rows, int64_t n_out, int64_t ld_in, const float *rows_in, int64_t ld_out, float *rows_out,
                           const int32_t *src, void *stream);

/* new — TRAJECTORY METRICS: per member (and scenario), from the STORED T rows of a run, what an overshoot is judged by: the
 * peak and when it is reached, when each warming level is first crossed and for how many stored steps it is held, and sums
 * over step windows (a 2081-2100 mean) — DESIGN.md section 3.13; host side: fiveeqscm_amd/metrics.py,
 * EnsembleEngine.trajectory_metrics.  Additive: no symbol above changes, FIVEEQ_ABI_VERSION stays 13.
 *
 * ONE streaming pass over rows dev [n_scen][n_rows][ld] (scenario blocks scen_stride elements apart; with n_scen == 1
 * scen_stride is not used), all metrics at once, the per-member state carried in and out so that the rows can come in
 * blocks.  steps dev [n_rows] int32: entry k is the model step row k holds.  levels HOST [n_levels] fp64, 0 <= n_levels <=
 * fiveeq_max_levels() (FIVEEQ_MAX_LEVELS); windows HOST [n_windows][2] int32 = [a_w, b_w), 0 <= n_windows <=
 * fiveeq_max_windows() (FIVEEQ_MAX_WINDOWS); both are copied by the call.  The state of member m of scenario s:
 *     fmet dev [n_scen][1 + n_windows][ld] fp64:      peak, then wsum[w]
 *     imet dev [n_scen][2 + 2 n_levels][ld] int32:    t_peak, n_nan, then first[l], then n_above[l]
 * DEFINITION.  Tw = the row value widened exactly to fp64.  For every row k in row order, t = steps[k]:
 *     if Tw is NaN:        n_nan += 1                (a NaN fails every comparison: no part in peak / first / n_above)
 *     if Tw > peak:        peak = Tw; t_peak = t     (strict: the EARLIEST step attaining the peak is kept)
 *     for each level l:    if Tw >= level_l: n_above[l] += 1; if first[l] < 0: first[l] = t
 *     for each window w:   if a_w <= t < b_w: wsum[w] = wsum[w] + Tw       (one rounded fp64 add; NaN propagates)
 * first_call != 0: the call starts from peak = -inf, t_peak = -1, first = -1, counts and sums 0 and does NOT read the state
 * blocks; first_call == 0: it continues the state it is handed.  Rows [0, k) in one call and rows [k, n) in a second give
 * the bits of one call: every result is an integer or an fp64 sum in row order, so launch shape, row split and shard split
 * cannot change a bit.  n_rows == 0 with first_call: the state is initialised; without: nothing is done.  Columns
 * [n_members, ld) of the state blocks are never written.
 * THE CALLER OWES: steps strictly increasing within a call and across the calls of one state (steps is device memory: the
 * library cannot look; fiveeqscm_amd/metrics.py checks) — "first" and "earliest" mean row order.
 * FIVEEQ_E_INVALID, before anything is launched, for: n_scen outside 1..fiveeq_max_scenarios(); n_rows < 0; n_members < 1 or
 * >= 2^31; ld < n_members; scen_stride < n_rows * ld with n_scen > 1; n_levels / n_windows out of range; a NaN level; a
 * window with a > b or a < 0; a NULL pointer (rows / steps may be NULL with n_rows == 0, levels / windows with a count of
 * 0); a pointer not aligned to its element (rows, steps 4, fmet 8, imet 4).  Rows aligned to 16 bytes with ld (and
 * scen_stride) a multiple of 16 bytes get 16-byte loads — an optimisation, not a contract. */
#define FIVEEQ_MAX_LEVELS   8
#define FIVEEQ_MAX_WINDOWS  4
int32_t fiveeq_max_levels(void);
int32_t fiveeq_max_windows(void);
/* the kernel's shape, for tests that pick their sizes at its edges: members per workgroup for rows of elem_bytes (8 or 4; 0
 * for anything else), and the rows whose loads the row loop issues before it uses the first (wide != 0: the 16-byte loads;
 * 0: the element loads) */
int32_t fiveeq_metrics_tile(int32_t elem_bytes);
int32_t fiveeq_metrics_unroll(int32_t wide);
int fiveeq_traj_metrics_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                            int64_t scen_stride, const int32_t *steps, int32_t n_levels, const double *levels,
                            int32_t n_windows, const int32_t *windows, double *fmet, int32_t *imet, int32_t first_call,
                            void *stream);
int fiveeq_traj_metrics_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                            int64_t scen_stride, const int32_t *steps, int32_t n_levels, const double *levels,
                            int32_t n_windows, const int32_t *windows, double *fmet, int32_t *imet, int32_t first_call,
                            void *stream);

/* new — RUNNING MEANS AND TRENDS: the two noise-robust reductions of a member's stored rows — the running mean over `window`
 * consecutive rows (a warming level is the first 20-year MEAN at or above it, not the first warm year of a member with
 * internal variability) and, per step window, the sums a least-squares trend is formed from — DESIGN.md section 3.22; host
 * side: fiveeqscm_amd/smooth.py, EnsembleEngine.running_mean / window_trends.  Additive: no symbol above changes,
 * FIVEEQ_ABI_VERSION stays 13.
 *
 * Both are streaming passes over rows dev [n_scen][n_rows][ld] (scenario blocks scen_stride elements apart; with n_scen == 1
 * no scenario stride is used), per member and scenario, every value widened exactly to fp64.
 *
 * (a) RUNNING MEAN.  tail dev [n_scen][n_tail][ld] (blocks tail_scen_stride apart), 0 <= n_tail <= window - 1: the rows that
 * precede row 0, kept from an earlier call; tail and rows are ONE sequence x[0 .. n_tail + n_rows).  out dev
 * [n_scen][n_out][ld] fp64 (blocks out_scen_stride apart), n_out = max(0, n_tail + n_rows - window + 1); ONE ld for rows, tail
 * and out.  1 <= window <= fiveeq_max_smooth_window() (FIVEEQ_MAX_SMOOTH_WINDOW).
 * DEFINITION, operation for operation, for every k in [0, n_out):
 *     s = (double) x[k]                                    exact
 *     for i = 1 .. window - 1:  s = s + (double) x[k + i]  one rounded fp64 add each, ASCENDING row order
 *     out[k] = s / (double) window                         one correctly rounded IEEE division (no reciprocal multiply)
 * Every output is summed afresh from its own `window` rows in a fixed order — there is no sliding add / subtract update —
 * so launch shape, row split (through tail) and member split cannot change a bit: rows [0, k) in one call and rows [k, n)
 * with tail = the last min(window - 1, k) rows in a second give, concatenated, the bits of one call.  A NaN row makes exactly
 * the `window` outputs that contain it NaN, for that member only; window == 1 returns the rows widened.  n_out == 0:
 * nothing is launched.  Columns [n_members, ld) of out are never written.
 *
 * (b) WINDOW TREND SUMS.  steps dev [n_rows] int32: entry k is the model step row k holds.  windows HOST [n_windows][2] int32 =
 * [a_w, b_w), 0 <= n_windows <= fiveeq_max_windows(); copied by the call.  The state of member m of scenario s:
 *     tsum dev [n_scen][2 n_windows][ld] fp64:      (sx[w], stx[w]) per window, scenario blocks 2 n_windows ld apart
 * DEFINITION.  For every row k in row order, t = steps[k], Tw the value widened, for each window w with a_w <= t < b_w:
 *     u      = (double) (t - a_w)                          exact
 *     sx[w]  = sx[w] + Tw                                  one rounded add
 *     stx[w] = stx[w] + (u * Tw)                           the product rounded, THEN the add rounded: no fused multiply-add
 * NaN propagates.  first_call != 0: the call starts from 0 and does NOT read tsum; first_call == 0: it continues the state it
 * is handed; rows [0, k) in one call and rows [k, n) in the next give the bits of one call.  n_rows == 0 with first_call: the
 * state is zeroed; without: nothing is done; n_windows == 0: nothing is done.  Columns [n_members, ld) of tsum are never
 * written.  The least-squares slope over window w, with n, su = sum u and suu = sum u^2 over the stored steps inside it
 * (integers the caller knows): (n stx - su sx) / (n suu - su^2) per step.
 * THE CALLER OWES: (a) rows evenly spaced in time, in time order, tail the rows directly before them (a mean over unevenly
 * stored rows is not a mean over time; fiveeqscm_amd/smooth.py checks the steps); (b) steps in row order across the calls of
 * one state.
 * FIVEEQ_E_INVALID, before anything is launched, for: n_scen outside 1..fiveeq_max_scenarios(); n_rows < 0; n_members < 1 or
 * >= 2^31; ld < n_members; with n_scen > 1 scen_stride < n_rows * ld, tail_scen_stride < n_tail * ld or out_scen_stride <
 * n_out * ld; window outside 1..FIVEEQ_MAX_SMOOTH_WINDOW; n_tail outside 0..window - 1; n_windows outside
 * 0..FIVEEQ_MAX_WINDOWS; a window with a > b or a < 0; a NULL pointer that is needed (rows / steps are not with n_rows == 0,
 * tail with n_tail == 0, out with n_out == 0, windows / tsum with n_windows == 0); a pointer not aligned to its element (rows,
 * tail; steps 4; out, tsum 8).  Rows, tail and out aligned to 16 bytes with ld (and the scenario strides) a multiple of 16
 * bytes get 16-byte accesses — an optimisation, not a contract. */
#define FIVEEQ_MAX_SMOOTH_WINDOW 32
int32_t fiveeq_max_smooth_window(void);
/* the kernels' shape, for tests that pick their sizes at its edges: members per workgroup of the running mean for rows of
 * elem_bytes (8 or 4; 0 for anything else), and the rows whose loads both row loops issue before they use the first
 * (wide != 0: the 16-byte loads; 0: the element loads) */
int32_t fiveeq_smooth_tile(int32_t elem_bytes);
int32_t fiveeq_smooth_unroll(int32_t wide);
int fiveeq_running_mean_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                            int64_t scen_stride, int32_t window, int32_t n_tail, const double *tail, int64_t tail_scen_stride,
                            double *out, int64_t out_scen_stride, void *stream);
int fiveeq_running_mean_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                            int64_t scen_stride, int32_t window, int32_t n_tail, const float *tail, int64_t tail_scen_stride,
                            double *out, int64_t out_scen_stride, void *stream);
int fiveeq_window_trends_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                             int64_t scen_stride, const int32_t *steps, int32_t n_windows, const int32_t *windows, double *tsum,
                             int32_t first_call, void *stream);
int fiveeq_window_trends_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                             int64_t scen_stride, const int32_t *steps, int32_t n_windows, const int32_t *windows, double *tsum,
                             int32_t first_call, void *stream);

/* new — JOINT STATISTICS: co-moments and conditional sums of per-member rows, for covariances, correlations, regression slopes
 * and first-order variance-based sensitivity indices of outputs against parameters, under the integer weights of WEIGHTED
 * SUMMARY — DESIGN.md section 3.14; host side: fiveeqscm_amd/joint.py, EnsembleEngine.drivers.  Additive: no symbol above
 * changes, FIVEEQ_ABI_VERSION stays 13.
 *
 * x dev [n_x][ld_x], y dev [n_y][ld_y]: rows of the same n_members members, one element type per call, every value widened
 * exactly to fp64.  weights dev [n_members] uint64, required, 0 <= w <= 2^32 (the contract of WEIGHTED SUMMARY); a member of
 * weight 0 does not exist for either pass, whatever its values (NaN and +-inf included).  1 <= n_x, n_y <=
 * fiveeq_max_joint_rows() (32); ld_x, ld_y >= n_members; 1 <= n_members < 2^31.  x, y, ld * sizeof(element) and weights aligned
 * to 16 bytes get 16-byte loads, anything else element loads: the same bits either way.
 *
 * (a) CO-MOMENTS.  pivots dev [n_x + n_y] fp64 = (cx, then cy).  Per member with w > 0, one rounding per written operation:
 *         wd = (double) w;   dx_i = x_i - cx_i;   dy_j = y_j - cy_j;   p_j = wd * dy_j;   px_i = wd * dx_i
 *         co[i][j]      = fma(dx_i, p_j, co[i][j])
 *         margins[r][0] = margins[r][0] + p_r;   margins[r][1] = fma(p_r, d_r, margins[r][1])      r: the x rows, then the y rows
 *     co dev [n_x][n_y] fp64; margins dev [n_x + n_y][2] fp64; info dev [4] uint64 = (sum w, exact; the count of w > 0; flags; 0)
 *     with flag bit 0: a NaN value with w > 0 in any row, bit 1: a weight above 2^32 — the caller's error; nanrows dev
 *     [n_x + n_y] uint64 = the weight of the members with w > 0 whose value in that row is NaN.  A NaN propagates through the
 *     fp64 sums of the rows it sits in, and through no others: pair (i, j) is NaN exactly when nanrows of x row i or y row j
 *     is not 0 (or a sum overflows).
 * (b) CONDITIONAL SUMS.  edges dev [n_x][n_bins - 1] fp64, non-decreasing per row (NULL allowed with n_bins == 1); 1 <= n_bins
 *     <= fiveeq_max_cond_bins() (32); pivots dev [n_y] fp64 = cy.  THE BIN of member m under x row i:
 *         b = #{ k : edges[i][k] < x_i }
 *     — a value equal to an edge belongs to the LOWER bin, which is the bin an inverted-CDF percentile edge closes.  A NaN x_i
 *     with w > 0 has no bin: its weight is added to xnan[i].
 *         sums[i][b][j] = sums[i][b][j] + wd * (y_j - cy_j)          dev [n_x][n_bins][n_y] fp64
 *         binw[i][b]   += w                                          dev [n_x][n_bins] uint64, exact
 *         xnan[i]      += w                                          dev [n_x] uint64
 * ORDER.  Every fp64 sum is taken in one fixed order — the lane-strided member order within a chunk of fiveeq_joint_tile(2)
 * members, a fixed tree over the lanes and waves of the workgroup, chunk order in the fold — and there is no floating-point
 * atomic: the bits depend on n_members, the values, the weights, the pivots and the edges only, not on ld, alignment, on how
 * the rows are tiled over workgroups (a call over 32 x 32 rows gives the bits of the calls over its sub-blocks) or on
 * repetition.  The integer outputs are exact.  All outputs are WRITTEN, not accumulated into.
 * partial dev: workspace of fiveeq_joint_chunks(n_members) * W 8-byte words, W = fiveeq_joint_moments_words(n_x, n_y) for (a)
 * and fiveeq_cond_sums_words(n_x, n_y, n_bins) for (b); it needs no initialisation.  The library allocates nothing and never
 * synchronises.
 * FIVEEQ_E_INVALID, before anything is launched and with fiveeq_last_error() naming the argument, for: n_members < 1 or
 * >= 2^31; n_x, n_y or n_bins outside their limits; ld_x or ld_y < n_members; a NULL pointer; a pointer not aligned to its
 * element (x, y; 8 bytes for everything else). */
int32_t fiveeq_max_joint_rows(void);
int32_t fiveeq_max_cond_bins(void);
/* the kernels' shape — not part of the ABI; for tests that pick their sizes at its edges.  which = 0, 1: x rows, y rows per
 * workgroup of (a); 2: members per chunk; 3, 4: members per lane and load of fp64, fp32 rows; 5, 6: bins, y rows per workgroup
 * of (b); 7: lanes per workgroup; anything else: 0 */
int32_t fiveeq_joint_tile(int32_t which);
int64_t fiveeq_joint_chunks(int64_t n_members);
int64_t fiveeq_joint_moments_words(int32_t n_x, int32_t n_y);
int64_t fiveeq_cond_sums_words(int32_t n_x, int32_t n_y, int32_t n_bins);
int fiveeq_joint_moments_f64(int64_t n_members, int32_t n_x, int64_t ld_x, const double *x, int32_t n_y, int64_t ld_y,
                             const double *y, const uint64_t *weights, const double *pivots, double *partial, double *co,
                             double *margins, uint64_t *info, uint64_t *nanrows, void *stream);
int fiveeq_joint_moments_f32(int64_t n_members, int32_t n_x, int64_t ld_x, const float *x, int32_t n_y, int64_t ld_y,
                             const float *y, const uint64_t *weights, const double *pivots, double *partial, double *co,
                             double *margins, uint64_t *info, uint64_t *nanrows, void *stream);
int fiveeq_cond_sums_f64(int64_t n_members, int32_t n_x, int64_t ld_x, const double *x, int32_t n_y, int64_t ld_y,
                         const double *y, const uint64_t *weights, int32_t n_bins, const double *edges, const double *pivots,
                         double *partial, double *sums, uint64_t *binw, uint64_t *xnan, void *stream);
int fiveeq_cond_sums_f32(int64_t n_members, int32_t n_x, int64_t ld_x, const float *x, int32_t n_y, int64_t ld_y,
                         const float *y, const uint64_t *weights, int32_t n_bins, const double *edges, const double *pivots,
                         double *partial, double *sums, uint64_t *binw, uint64_t *xnan, void *stream);

/* new — SCORING STORED ROWS: the misfit of CONSTRAINED RUNS computed from the STORED rows of a run, against observed records of
 * any stored quantity (T, the concentration of a gas) and for runs of every mode, pool layout and precision — DESIGN.md section
 * 3.15; host side: fiveeqscm_amd/constrain.py score_rows, EnsembleEngine.score.  Additive: no symbol above changes,
 * FIVEEQ_ABI_VERSION stays 13.
 *
 * ONE streaming pass.  The element of row k, quantity j, member m is rows[k * row_stride + j * q_stride + m]: the C rows
 * [n_rows][G][ld] of a run are row_stride = G * ld, q_stride = ld; its T rows are n_q = 1 (q_stride is then not used; with
 * n_rows == 1 row_stride is not).  1 <= n_q <= fiveeq_max_score_quantities() (FIVEEQ_MAX_SCORE_Q).  steps dev [n_rows] int32:
 * entry k is the model step row k holds.  obs dev [n_q][n_steps][4] fp64: one table of CONSTRAINED RUNS per quantity, (o_t, p_t,
 * b_t, 0) per step.  misfit dev [n_q][3][ld_m] fp64 = (A, U, V) per quantity, READ AND WRITTEN IN PLACE: the caller zeroes it
 * (the contract of fiveeq_run_obs_*).  ld_m is independent of the row strides.
 * DEFINITION.  For the rows in row order, t = steps[k], and for each quantity j with the record (o, p, b) = obs[j][t]:
 *     if p == 0 && b == 0:  the accumulators of j are untouched, and the row's elements of j do not matter (NaN included: they
 *                           are not read)
 *     else, with Tw the element widened exactly to fp64, each operation rounded on its own (no fma):
 *                           A = A + b * Tw;  d = Tw - o;  pd = p * d;  U = U + pd;  V = V + pd * d
 * — the device function the stepping kernels call, so the pass gives, bit for bit, the misfit a run carrying the same record
 * in-loop gives.  CONSEQUENCES: rows [0, k) in one call and rows [k, n) in a second give the bits of one call; any member
 * sub-range gives the bits of the whole (shards exchange nothing); launch shape and alignment cannot change a bit (rows aligned
 * to 16 bytes with strides a multiple of 16 bytes get 16-byte loads — an optimisation, not a contract); columns [n_members, ld_m)
 * of misfit are never written; n_rows == 0 does nothing.  Rows whose record is dead are not streamed: the pass reads
 * sizeof(element) * n_members per live row-quantity and 48 * n_members per quantity.
 * THE CALLER OWES: steps strictly increasing within a call and across the calls of one misfit block, and every step inside
 * [0, n_steps) (steps is device memory: the library cannot look; constrain.score_rows checks.  The kernel never reads outside
 * the tables: a row whose step lies outside is skipped).
 * FIVEEQ_E_INVALID, before anything is launched and with fiveeq_last_error() naming the argument, for: n_q outside
 * 1..FIVEEQ_MAX_SCORE_Q; n_rows < 0; n_members < 1 or >= 2^31; ld_m < n_members; |q_stride| < n_members with n_q > 1;
 * row_stride < n_members with n_rows > 1; n_steps < 1; a NULL pointer (rows and steps may be NULL with n_rows == 0); a
 * pointer not aligned to its element (rows; steps 4; obs and misfit 8). */
#define FIVEEQ_MAX_SCORE_Q  4
int32_t fiveeq_max_score_quantities(void);
/* the kernel's shape, for tests that pick their sizes at its edges: members per workgroup for rows of elem_bytes (8 or 4; 0
 * for anything else), and the LIVE rows whose loads the row loop issues before it uses the first (wide != 0: the 16-byte
 * loads; 0: the element loads) */
int32_t fiveeq_score_tile(int32_t elem_bytes);
int32_t fiveeq_score_unroll(int32_t wide);
int fiveeq_score_rows_f64(int32_t n_q, int32_t n_rows, int64_t n_members, const double *rows, int64_t row_stride,
                          int64_t q_stride, const int32_t *steps, const double *obs, int32_t n_steps, double *misfit,
                          int64_t ld_m, void *stream);
int fiveeq_score_rows_f32(int32_t n_q, int32_t n_rows, int64_t n_members, const float *rows, int64_t row_stride,
                          int64_t q_stride, const int32_t *steps, const double *obs, int32_t n_steps, double *misfit,
                          int64_t ld_m, void *stream);

/* new — FORCING ROWS: the effective radiative forcing F, its split by gas F_g, the top-of-atmosphere energy imbalance N and the
 * cumulated heat uptake H of a run, DIAGNOSED FROM ITS STORED ROWS, for runs of every mode and precision — DESIGN.md section
 * 3.17; host side: fiveeqscm_amd/diagnose.py forcing_rows, EnsembleEngine.forcing_rows.  Additive: no symbol above changes,
 * FIVEEQ_ABI_VERSION stays 13, fiveeq_sizeof_model() stays 448.
 *
 * ONE streaming pass.  The concentration of row k, gas g, member m is C_rows[k * c_row_stride + g * c_gas_stride + m] (the C
 * rows [n_rows][G][ld] of a run: c_row_stride = G * ld, c_gas_stride = ld), the warming T_rows[k * t_row_stride + m].  steps dev
 * [n_rows] int32: entry k is the model step row k holds.  drive dev [n_steps][8] as in the stepping entry points (F_ext at
 * [6]).  q dev [2][ld].  fscale dev [G + n_fext][ld] (gas rows first) and fext dev [n_steps][fiveeq_max_fext()] as in FORCING
 * SCALES; both NULL (n_fext 0) for a run without forcing scales.  All in the precision of the entry point.
 * DEFINITION.  For the rows in row order, t = steps[k], per member, every operation rounded on its own in the rows' precision:
 *     F_g = f2 (C_g - C0) + f1 ln(C_g / C0) + f3 (sqrt C_g - sqrt C0)      the device function the stepping kernels call: the
 *                                                                         same coefficient tests, the same C > 0 guard
 *     F   = F_ext[t];  F = fma(sx_k, X[t][k], F), k < n_fext;  F = fma(sg_g, F_g, F)     with fscale;    F = F + F_g   without
 *     N   = F - T / (q0 + q1)                 IEEE division.  The two-box model's equilibrium is T = (q0 + q1) F: its feedback
 *                                             parameter is 1 / (q0 + q1), and N its top-of-atmosphere imbalance
 *     H   = H + dt * (double)N                fp64 in both precisions, W yr m-2; no fma
 *     S_j = fma(em1_d[j], fma(-q_j, F, S_j), S_j);  T' = S_0 + S_1               THE REPLAY, with S_io only
 * — so F is, bit for bit, the F the run's stepping kernel formed at that step (every non-compensated, emission-driven form),
 * and the replay proves it: *n_mismatch is INCREASED by the number of (row, member) whose T' differs in bits from the stored T
 * (NaN equal to NaN; the caller zeroes it).
 * OUTPUTS, each nullable, written for columns [0, n_members) only: F [n_rows][ld_out], F_gas [n_rows][G][ld_out], N
 * [n_rows][ld_out] in the rows' precision, H [n_rows][ld_out] fp64 (H after row k).  CARRIED STATE, in / out and nullable: H_io
 * [ld] fp64 (H before the first row; NULL with H: 0, and nothing is handed back) and S_io [2][ld] (the boxes before the first
 * row; asks for the replay, needs n_mismatch).  H and the replay take the rows as consecutive model steps: THE CALLER OWES
 * that, and steps inside [0, n_steps) (steps is device memory: diagnose.forcing_rows checks; the kernel clamps a step into the
 * tables and never reads outside them).
 * CONSEQUENCES: rows [0, k) in one call and rows [k, n) in a second with H_io / S_io carried give the bits of one call; any
 * member sub-range gives the bits of the whole; launch shape, strides and alignment cannot change a bit (rows and outputs
 * aligned to 16 bytes with strides a multiple of 16 bytes get 16-byte accesses — an optimisation, not a contract).  Without H,
 * H_io and S_io the rows are independent and are spread over the grid; with one of them a lane carries its members through
 * all rows.  Nothing is allocated, nothing synchronises.  The pass moves sizeof(element) * (G + [T read]) + the outputs asked
 * for per member-row; the T rows are read only for N, H, H_io or S_io.
 * FIVEEQ_E_UNSUPPORTED for a pool layout outside fiveeq_layout_supported.  FIVEEQ_E_INVALID, before anything is launched and
 * with fiveeq_last_error() naming the argument, for: an invalid model; n_rows < 0; n_members < 1 or >= 2^31; ld < n_members;
 * ld_out < n_members with an output; c_row_stride < n_members with n_rows > 1; |c_gas_stride| < n_members with G > 1;
 * t_row_stride < n_members with T_rows and n_rows > 1; N, H, H_io or S_io without T_rows; S_io without n_mismatch; n_fext
 * outside 0..fiveeq_max_fext(); fscale without fext or fext without fscale when n_fext > 0; n_fext > 0 with neither; n_steps < 1;
 * a NULL C_rows, steps, drive or q (C_rows and steps may be NULL with n_rows == 0); a pointer not aligned to its element. */
/* members per workgroup for rows of elem_bytes (8 or 4; 0 for anything else), for tests that pick their sizes at its edges */
int32_t fiveeq_forcing_rows_tile(int32_t elem_bytes);
int fiveeq_forcing_rows_f64(const fiveeq_model *model, int32_t n_rows, int64_t n_members, int64_t ld, const double *C_rows,
                            int64_t c_row_stride, int64_t c_gas_stride, const double *T_rows, int64_t t_row_stride,
                            const int32_t *steps, const double *drive, int32_t n_steps, const double *q, const double *fscale,
                            int32_t n_fext, const double *fext, double *F, double *F_gas, double *N, double *H, int64_t ld_out,
                            double *H_io, double *S_io, uint64_t *n_mismatch, void *stream);
int fiveeq_forcing_rows_f32(const fiveeq_model *model, int32_t n_rows, int64_t n_members, int64_t ld, const float *C_rows,
                            int64_t c_row_stride, int64_t c_gas_stride, const float *T_rows, int64_t t_row_stride,
                            const int32_t *steps, const float *drive, int32_t n_steps, const float *q, const float *fscale,
                            int32_t n_fext, const float *fext, float *F, float *F_gas, float *N, double *H, int64_t ld_out,
                            double *H_io, float *S_io, uint64_t *n_mismatch, void *stream);

/* new — PULSE RESPONSE: what a unit emission of a gas is worth, per member — the response of forcing, warming and concentration
 * to emission pulses, summed to time horizons, FROM THE STORED ROWS of a scenario engine that ran "baseline" and "baseline +
 * pulse of gas g" for the same members — DESIGN.md section 3.19; host side: fiveeqscm_amd/pulse.py pulse_response,
 * EnsembleEngine.pulse_response.  Additive: no symbol above changes, FIVEEQ_ABI_VERSION stays 13, fiveeq_sizeof_model() stays 448.
 *
 * ONE streaming pass.  The concentration of scenario s, row k, gas g, member m is C_rows[s * c_scen_stride + k * c_row_stride +
 * g * c_gas_stride + m] (the C rows [S][n_rows][G][ld] of a scenario engine), the warming T_rows[s * t_scen_stride + k *
 * t_row_stride + m].  steps dev [n_rows] int32: entry k is the model step row k holds.  drive dev [n_scen][n_steps][8] (F_ext at
 * [6]), fscale dev [G + n_fext][ld] and fext dev [n_scen][n_steps][fiveeq_max_fext()] as in SCENARIOS and FORCING SCALES; fscale
 * and fext both NULL (n_fext 0) for a run without forcing scales.  All in the precision of the entry point.  base: the base
 * scenario b.  pulse_scen, pulse_gas HOST [n_pulses] int32: pulse p is scenario s_p != b with gas g_p pulsed, 1 <= n_pulses <=
 * fiveeq_max_pulses() (FIVEEQ_MAX_PULSES).  horizons HOST [n_horizons] int32, 1 <= n_horizons <= fiveeq_max_horizons()
 * (FIVEEQ_MAX_HORIZONS): strictly increasing ROW COUNTS n_h >= 1, counted from the first row of the experiment; row0 is the
 * number of rows earlier calls have covered (0 for the first call).
 * DEFINITION.  For the rows in row order, per member and pulse p, every operation rounded on its own:
 *     F_b, F_p = the forcing of scenario b / s_p at the row, formed exactly as FORCING ROWS forms F (the same device function)
 *     dF_p = (double)F_p - (double)F_b;   dT_p = (double)T[s_p] - (double)T[b];   dC_p = (double)C[s_p][g_p] - (double)C[b][g_p]
 *     I_F_p = I_F_p + dF_p;   I_T_p = I_T_p + dT_p;   I_C_p = I_C_p + dC_p        fp64 in both precisions; no fma
 * — the rectangle rule over end-of-step values (times dt on the host), the convention of the heat uptake H.  When row0 + k ==
 * n_h - 1 the values AFTER that row are written to out [5][n_pulses][n_horizons][ld_out] fp64 = (I_F, I_T, I_C, dT, dC) at
 * [.][p][h], columns [0, n_members).  A horizon the rows of this call do not end on is NOT written (the caller pre-fills out,
 * e.g. with NaN).  CARRIED STATE io [3][n_pulses][ld] fp64, in / out: (I_F, I_T, I_C) before the first row and after the last;
 * the caller zeroes it before the first call.  NaN is not skipped: a NaN input makes the sums it enters NaN from that row on,
 * for that member only.
 * CONSEQUENCES: rows [0, k) in one call and rows [k, n) in a second (row0 = k, io carried) give the bits of one call; any
 * member sub-range gives the bits of the whole; launch shape, strides and alignment cannot change a bit.  THE CALLER OWES rows
 * of consecutive model steps and steps inside [0, n_steps) (the kernel clamps a step into the tables and never reads outside
 * them).  Nothing is allocated, nothing synchronises.  The pass reads sizeof(element) * (1 + n_pulses)(G + 1) per member-row.
 * FIVEEQ_E_UNSUPPORTED for a pool layout outside fiveeq_layout_supported.  FIVEEQ_E_INVALID, before anything is launched and
 * with fiveeq_last_error() naming the argument, for: an invalid model; n_rows < 0; row0 < 0 or row0 + n_rows >= 2^31; n_members
 * < 1 or >= 2^31; ld or ld_out < n_members; n_scen < 2; n_pulses or n_horizons out of range; a NULL pulse_scen, pulse_gas or
 * horizons; base or a pulse's scenario outside [0, n_scen); a pulse naming the base scenario; a pulse's gas outside [0, G); a
 * horizon < 1 or not above its predecessor; c_row_stride or t_row_stride < n_members with n_rows > 1; |c_gas_stride| <
 * n_members with G > 1; |c_scen_stride| or |t_scen_stride| < n_members (rows that overlap); n_fext outside 0..fiveeq_max_fext();
 * fscale without fext or fext without fscale when n_fext > 0; n_steps < 1; a NULL C_rows, T_rows or steps (allowed with n_rows
 * == 0), drive, out or io; a pointer not aligned to its element. */
#define FIVEEQ_MAX_PULSES   3
#define FIVEEQ_MAX_HORIZONS 8
int32_t fiveeq_max_pulses(void);
int32_t fiveeq_max_horizons(void);
int fiveeq_pulse_response_f64(const fiveeq_model *model, int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld,
                              const double *C_rows, int64_t c_scen_stride, int64_t c_row_stride, int64_t c_gas_stride,
                              const double *T_rows, int64_t t_scen_stride, int64_t t_row_stride, const int32_t *steps,
                              const double *drive, int32_t n_steps, const double *fscale, int32_t n_fext, const double *fext,
                              int32_t base, int32_t n_pulses, const int32_t *pulse_scen, const int32_t *pulse_gas,
                              int32_t n_horizons, const int32_t *horizons, int32_t row0, double *out, int64_t ld_out,
                              double *io, void *stream);
int fiveeq_pulse_response_f32(const fiveeq_model *model, int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld,
                              const float *C_rows, int64_t c_scen_stride, int64_t c_row_stride, int64_t c_gas_stride,
                              const float *T_rows, int64_t t_scen_stride, int64_t t_row_stride, const int32_t *steps,
                              const float *drive, int32_t n_steps, const float *fscale, int32_t n_fext, const float *fext,
                              int32_t base, int32_t n_pulses, const int32_t *pulse_scen, const int32_t *pulse_gas,
                              int32_t n_horizons, const int32_t *horizons, int32_t row0, double *out, int64_t ld_out,
                              double *io, void *stream);

/* new — SINGLE-VALUED PARAMETER ROWS: the per-step form without the loads of the parameter rows whose members all hold one value
 * — DESIGN.md section 3.16; host side: EnsembleEngine(uniform_rows=).  Additive: no symbol above changes, FIVEEQ_ABI_VERSION
 * stays 13, fiveeq_sizeof_model() stays 448.
 *
 * The rows are numbered as the kernels read them: row k of r (k < 3 n_gas; gas-major r0, rC, rT) is bit k, row j of q is bit
 * 3 n_gas + j; values [3 n_gas + 2] is indexed the same way.
 *
 * fiveeq_uniform_rows_*: ONE device pass over r dev [n_r_rows][ld] (n_r_rows = 3 n_gas) and q dev [2][ld].  A row is
 * single-valued iff all n_members of its members are BITWISE equal to its first: a row of +0.0 with one -0.0 is not, a row of
 * one NaN bit pattern is.  Columns [n_members, ld) are not examined.  The call SYNCHRONISES stream and returns, in HOST memory,
 * *mask_out (the bits of the single-valued rows) and values_out [n_r_rows + 2] (the first member of EVERY row, single-valued or
 * not).  FIVEEQ_E_INVALID for n_members < 1, ld < n_members, n_r_rows not 3, 6 or 9, a NULL or misaligned pointer.
 *
 * fiveeq_run_uniform_* / fiveeq_plan_create_uniform_*: fiveeq_run_* / fiveeq_plan_create_* (same arguments, same results bit for
 * bit) plus (mask, values).  THE MASK IS THE CALLER'S PROMISE: a row whose bit is set is NEVER READ — every member takes
 * values[k] — so the contents of its device memory are irrelevant (r and q themselves must still be valid pointers).  values is
 * host memory, copied during the call; entries of rows whose bit is clear are not looked at.  mask == 0, or a pool layout
 * without the form (it is compiled for pools {4} and 4 + 1 + 1, fp64 and fp32 packed or not, both row policies), launches
 * exactly what fiveeq_run_* launches.  FIVEEQ_E_INVALID for bits at or above 3 n_gas + 2, and for a non-zero mask with values
 * NULL (checked right behind the base arguments).  Per member-step the launch moves sizeof(element) bytes less per masked row. */
int fiveeq_uniform_rows_f64(int64_t n_members, int64_t ld, int32_t n_r_rows, const double *r, const double *q,
                            uint32_t *mask_out, double *values_out, void *stream);
int fiveeq_uniform_rows_f32(int64_t n_members, int64_t ld, int32_t n_r_rows, const float *r, const float *q,
                            uint32_t *mask_out, float *values_out, void *stream);
int fiveeq_run_uniform_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const double *r, const double *q, double *R, double *S, double *C_traj, double *T_traj,
                           int32_t n_rows, double *T_stats, uint32_t mask, const double *values /* host, 3G+2 */, void *stream);
int fiveeq_run_uniform_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                           const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                           const float *r, const float *q, float *R, float *S, float *C_traj, float *T_traj,
                           int32_t n_rows, double *T_stats, uint32_t mask, const float *values /* host, 3G+2 */, void *stream);
int fiveeq_plan_create_uniform_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                   const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                   const double *r, const double *q, double *R, double *S, double *C_traj, double *T_traj,
                                   int32_t n_rows, double *T_stats, uint32_t mask, const double *values, void **plan_out);
int fiveeq_plan_create_uniform_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                                   const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                                   const float *r, const float *q, float *R, float *S, float *C_traj, float *T_traj,
                                   int32_t n_rows, double *T_stats, uint32_t mask, const float *values, void **plan_out);

/* STREAMED HISTOGRAMS through a ring of BIN INDICES (round 3).  fiveeq_run_fused_bins_* is
 * fiveeq_run_fused_* (same arguments, same results, C_traj / T_traj / T_stats as there) that ALSO writes, for every step t of
 * the span and every member m, the histogram bin of T(t, m) — the rule of fiveeq_hist_rows_* with (hist_lo, hist_hi, n_bins),
 * bit for bit; 0xFFFF for a NaN — as one uint16 into bin_ring dev [ring_rows][ld] at row t mod ring_rows: 2 bytes per
 * member-step where a ring of T rows takes 4 or 8.  fiveeq_hist_bins then counts rows of such indices into
 * hist dev [n_rows][n_bins] uint64 (ACCUMULATED INTO).  The caller runs spans of at most ring_rows steps and drains the
 * ring between them (EnsembleEngine does, on a second stream).  The pass does not see T: per-step moments, if wanted,
 * come from T_stats.  fiveeq_hist_bins skips every index >= n_bins (0xFFFF among them) and changes nothing outside
 * hist[row][0 .. n_bins - 1] of the n_rows rows it is given. */
int fiveeq_run_fused_bins_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                              const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                              const double *r, const double *q, double *R, double *S,
                              double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                              double hist_lo, double hist_hi, int32_t n_bins,
                              uint16_t *bin_ring, int32_t ring_rows, void *stream);
int fiveeq_run_fused_bins_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                              const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                              const float *r, const float *q, float *R, float *S,
                              float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                              double hist_lo, double hist_hi, int32_t n_bins,
                              uint16_t *bin_ring, int32_t ring_rows, void *stream);
int fiveeq_hist_bins(int32_t n_rows, int64_t n_members, int64_t ld, const uint16_t *bins, int32_t n_bins,
                     uint64_t *hist, void *stream);
/* the same for the PER-STEP form: fiveeq_run_* (one launch per timestep) whose kernel also writes the bin index of T —
 * 2 bytes per member-step on top of the step's w(2 SP + 4 G + 7), where a ring of T rows adds w written + w re-read */
int fiveeq_run_bins_f64(const fiveeq_model *model, int64_t n_members, int64_t ld,
                        const double *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const double *r, const double *q, double *R, double *S,
                        double *C_traj, double *T_traj, int32_t n_rows, double *T_stats,
                        double hist_lo, double hist_hi, int32_t n_bins,
                        uint16_t *bin_ring, int32_t ring_rows, void *stream);
int fiveeq_run_bins_f32(const fiveeq_model *model, int64_t n_members, int64_t ld,
                        const float *drive, int32_t n_steps, int32_t t_begin, int32_t t_end,
                        const float *r, const float *q, float *R, float *S,
                        float *C_traj, float *T_traj, int32_t n_rows, double *T_stats,
                        double hist_lo, double hist_hi, int32_t n_bins,
                        uint16_t *bin_ring, int32_t ring_rows, void *stream);

/* new — shard-computable Latin hypercube: out[k][i] = u_{dim0+k}(m0 + i),
 * 0 <= i < n_members, 0 <= k < n_dim, for a design over n_total members:
 *     u_d(m) = (pi_d(m) + jitter_d(m)) / n_total
 * with pi_d a keyed bijection of [0, n_total) (cycle-walked 4-round Feistel network) and jitter a
 * 24-bit counter-based hash in (0,1): exactly one member per stratum and dimension, and a pure
 * function of (seed, d, m, n_total) — every rank computes only its own members, on its own device,
 * and gets the same design whatever the world size.  out dev [n_dim][ld] fp64.
 * 1 <= n_total <= FIVEEQ_LHS_MAX_TOTAL (2^28): up to there pi + jitter (28 + 25 bits) is an exact fp64 sum, so u lies
 * strictly inside its stratum; larger designs are refused rather than rounded onto a stratum edge.
 * Host twin (bit-identical): fiveeqscm_amd.params.lhs_rows. */
int fiveeq_lhs_rows_f64(uint64_t seed, int64_t n_total, int64_t m0, int64_t n_members,
                        int32_t dim0, int32_t n_dim, int64_t ld, double *out, void *stream);
/* the same rows into HOST memory, computed on the calling thread by the same functions (no GPU needed) */
int fiveeq_lhs_rows_host_f64(uint64_t seed, int64_t n_total, int64_t m0, int64_t n_members,
                             int32_t dim0, int32_t n_dim, int64_t ld, double *out);

/* new — diagnostic: STREAM-style copy dst[i] = src[i], i < n, with the SAME access shape as the
 * step kernel (one 8-byte element per lane, 512 B per wave-instruction, grid sized the same way).
 * Used to measure the achievable copy bandwidth on the box and to calibrate the rocprofv3
 * FETCH_SIZE / WRITE_SIZE counters on a known byte count (MI355X_MICROARCH.md, HBM section). */
int fiveeq_stream_copy_f64(int64_t n, const double *src, double *dst, void *stream);
/* the same copy with 16 B per lane (n even, pointers 16-byte aligned): the box's best plain copy */
int fiveeq_stream_copy_wide_f64(int64_t n, const double *src, double *dst, void *stream);
/* the same copy, 8 B per lane, NON-TEMPORAL loads and stores, one workgroup per 8 KiB (n a multiple of 1024): the fastest
 * plain copy measured on MI355X (tools/microbench/hbm_rates.hip) — the ceiling bench.py's hbm_resident figure is held against */
int fiveeq_stream_copy_nt_f64(int64_t n, const double *src, double *dst, void *stream);
/* new — diagnostic: ONE wave that runs `iterations` (0..1e8) dependent fp64 FMAs (~3.5 ns each) and writes one double to
 * `out`: a launch of known duration that occupies one SIMD.  Two of them on two streams take the time of one when the streams
 * run side by side and of two when they share a hardware queue — how the Python host picks the side streams of its two-stream
 * schedules (a stream that shares the caller's hardware queue costs the per-step form +12 %). */
int fiveeq_busy(int64_t iterations, double *out, void *stream);

/* new — CARBON ROWS: the airborne emissions G_a, the cumulative emissions, the cumulative uptake G_u, the airborne fraction, the
 * iIRF100, the lifetime scaling alpha and the sink flux of a run, DIAGNOSED FROM ITS STORED ROWS, for runs of every mode, drive
 * and precision — DESIGN.md section 3.23; host side: fiveeqscm_amd/carbon.py carbon_rows, EnsembleEngine.carbon_rows.  Additive:
 * no symbol above changes, FIVEEQ_ABI_VERSION stays 13, fiveeq_sizeof_model() stays 448.
 *
 * ONE streaming pass.  The stored value of row k, gas g, member m is rows[k * c_row_stride + g * c_gas_stride + m] (the C rows
 * [n_rows][G][ld] of a run — which hold the diagnosed EMISSIONS of a concentration-driven gas), the warming T_rows[k *
 * t_row_stride + m].  steps dev [n_rows] int32: entry k is the model step row k holds.  drive dev [n_steps][8] as in the stepping
 * entry points (E_g, or the target C_g of a concentration-driven gas, at [g]).  cum_end dev [n_steps][FIVEEQ_MAX_GAS]: the
 * cumulative emissions at the END of each step — the host's fp64 cumsum(E dt), which is what column 3 + g of step t + 1 of the
 * drive table holds, rounded to the precision of the entry point.  r dev [3 G][ld] (r0, rC, rT of gas 0, then gas 1, ...).
 * conc_mask: bit g set = gas g was concentration-driven (MIXED DRIVE).  gas_mask: the gases to diagnose, n_sel of them; output
 * (k, slot, m) is out[(k * n_sel + slot) * ld_out + m], slot counting the selected gases below g.
 * DEFINITION.  For the rows in row order, t = steps[k], per selected gas and member, every operation rounded on its own in the
 * rows' precision unless an fma is written:
 *     emission-driven gas:        C_g = the stored row;  E = drive[t][g];  cumE = cum_end[t][g]
 *     concentration-driven gas:   C_g = drive[t][g];  E = the stored row;  cum = fma(E, dt, cum);  cumE = cum    (the statement
 *                                 of the stepping kernel: cum after the last row is the engine's cumE, bit for bit)
 *     airborne = G_a = (C_g - C0) * (1 / emis2conc)
 *     uptake   = G_u = cumE - G_a
 *     fraction = G_a / cumE                                          IEEE division: 0/0 and x/0 as IEEE gives them
 *     iirf     = min(fma(ra, G_a, fma(rT, T, fma(rC, G_u, r0))), iirf_max)       the statements of the stepping kernels;
 *     alpha    = g0 exp(iirf / g1)                                   min is IEEE minNum: a NaN iIRF reads iirf_max
 *     sink     = E - (G_a - G_a_prev) / dt                           IEEE division; G_a_prev: the row before, ga_io for the first
 * T is the row's stored T, so iirf and alpha of the row of step t are what step t + 1 uses.  A NaN stored value makes that
 * row's airborne, uptake, fraction and sink (and the next row's sink) NaN and its iirf / alpha those of iirf_max; cumE of an
 * emission-driven gas is the shared table whatever the rows hold; a NaN stored E of a concentration-driven gas stays in cum.
 * OUTPUTS, each nullable, [n_rows][n_sel][ld_out] in the rows' precision, written for columns [0, n_members) only.  CARRIED
 * STATE, in / out and nullable: cum_io [G][ld] (cum of the concentration-driven gases before the first row; needed for their
 * cumE, uptake, fraction, iirf, alpha) and ga_io [G][ld] (G_a before the first row; needed for sink); rows of unselected gases
 * are neither read nor written.  Both take the rows as consecutive model steps: THE CALLER OWES that, and steps inside
 * [0, n_steps) (carbon.carbon_rows checks; the kernel clamps a step into the tables and never reads outside them).
 * CONSEQUENCES: rows [0, k) in one call and rows [k, n) in a second with cum_io / ga_io carried give the bits of one call; any
 * member sub-range gives the bits of the whole; launch shape, strides and alignment cannot change a bit (rows and outputs
 * aligned to 16 bytes with strides a multiple of 16 bytes get 16-byte accesses — an optimisation, not a contract).  Without
 * cum_io and ga_io the rows are independent and are spread over the grid; with one of them a lane carries its members through
 * all rows.  Nothing is allocated, nothing synchronises.  The T rows and r are read only for iirf or alpha.
 * FIVEEQ_E_UNSUPPORTED for a pool layout outside fiveeq_layout_supported.  FIVEEQ_E_INVALID, before anything is launched and
 * with fiveeq_last_error() naming the argument, for: an invalid model; n_rows < 0; n_members < 1 or >= 2^31; ld < n_members;
 * ld_out < n_members with an output; c_row_stride < n_members with n_rows > 1; |c_gas_stride| < n_members with G > 1;
 * t_row_stride < n_members with T_rows and n_rows > 1; a conc_mask or gas_mask naming a gas the model has not, an empty
 * gas_mask; iirf or alpha without T_rows or r; sink without ga_io; cumE, uptake, fraction, iirf or alpha of a selected
 * concentration-driven gas without cum_io, of a selected emission-driven gas without cum_end; n_steps < 1; a NULL rows, steps
 * or drive (rows and steps may be NULL with n_rows == 0); a pointer not aligned to its element. */
/* members per workgroup for rows of elem_bytes (8 or 4; 0 for anything else); rows in flight per lane (wide: 16-byte accesses,
 * seq: with carried state); rows per workgroup of the row-parallel form — for tests that pick their sizes at these edges */
int32_t fiveeq_carbon_rows_tile(int32_t elem_bytes);
int32_t fiveeq_carbon_rows_unroll(int32_t wide, int32_t seq);
int32_t fiveeq_carbon_rows_yrows(void);
int fiveeq_carbon_rows_f64(const fiveeq_model *model, int32_t n_rows, int64_t n_members, int64_t ld, const double *rows,
                           int64_t c_row_stride, int64_t c_gas_stride, const double *T_rows, int64_t t_row_stride,
                           const int32_t *steps, const double *drive, const double *cum_end, int32_t n_steps, const double *r,
                           int32_t conc_mask, int32_t gas_mask, double *airborne, double *cumE, double *uptake, double *fraction,
                           double *iirf, double *alpha, double *sink, int64_t ld_out, double *cum_io, double *ga_io, void *stream);
int fiveeq_carbon_rows_f32(const fiveeq_model *model, int32_t n_rows, int64_t n_members, int64_t ld, const float *rows,
                           int64_t c_row_stride, int64_t c_gas_stride, const float *T_rows, int64_t t_row_stride,
                           const int32_t *steps, const float *drive, const float *cum_end, int32_t n_steps, const float *r,
                           int32_t conc_mask, int32_t gas_mask, float *airborne, float *cumE, float *uptake, float *fraction,
                           float *iirf, float *alpha, float *sink, int64_t ld_out, float *cum_io, float *ga_io, void *stream);

/* new — diagnostic: y[i] = f(x[i]) with one of the kernels' own fp64 math primitives, so tests can
 * pin each against a CPU libm to the ulp.  op: 0 expm1 (x <= 0), 1 exp, 2 log (x > 0, finite normal),
 * 3 sqrt (x > 0, finite normal), 4 reciprocal (x > 0, finite normal).  _f32 only: op + 8 evaluates the PACKED twin of
 * the primitive (two members per lane, fiveeq_set_f32_packing above) on the element pairs (x[2i], x[2i+1]), n even:
 * it must return the scalar routine's bits. */
int fiveeq_math_probe_f64(int32_t op, int64_t n, const double *x, double *y, void *stream);
int fiveeq_math_probe_f32(int32_t op, int64_t n, const float *x, float *y, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FIVEEQ_H */
