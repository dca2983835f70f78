// fiveeq_capi.hip — the C ABI declared in include/fiveeq.h: host-side validation,
// model preparation and kernel dispatch.  gfx950 only; build with
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared -I include fiveeq_capi.hip -o libfiveeq_hip.so
#include "fiveeq.h"
#include "fiveeq_device.hpp"

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <type_traits>

#ifndef FIVEEQ_FUSED_DYN_LDS
#define FIVEEQ_FUSED_DYN_LDS 0     // experiment knob: unused dynamic LDS per fused workgroup, to cap occupancy
#endif

namespace {

using namespace fiveeq;

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(FIVEEQ_E_HIP, "%s failed: %s (%d)", #expr, hipGetErrorString(e_), (int)e_); \
    } while (0)

// ---- argument checks the passes share: each leaves its message and returns the code, or FIVEEQ_OK ------------
// A pass calls them in the order it documents, so the first bad argument names itself; `name` is the argument's
// name where the message carries it.
constexpr int64_t MEMBERS_MAX = 0x7fffffffLL;               // members of a shard and outputs: int32 indices
bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }
int check_n_rows(int32_t n_rows) { return n_rows < 0 ? fail(FIVEEQ_E_INVALID, "n_rows=%d must be >= 0", n_rows) : FIVEEQ_OK; }
int check_members(int64_t n) {
    return n < 1 || n > MEMBERS_MAX ? fail(FIVEEQ_E_INVALID, "n_members=%lld outside 1..2^31-1", (long long)n) : FIVEEQ_OK;
}
// a leading dimension, or a stride that cannot be negative, spans the members
int check_ld(const char* name, int64_t ld, int64_t n) {
    return ld < n ? fail(FIVEEQ_E_INVALID, "%s=%lld < n_members=%lld", name, (long long)ld, (long long)n) : FIVEEQ_OK;
}
// a signed stride spans the members in either direction
int check_stride(const char* name, int64_t stride, int64_t n) {
    const int64_t mag = stride < 0 ? -stride : stride;
    return mag < n ? fail(FIVEEQ_E_INVALID, "|%s|=%lld < n_members=%lld", name, (long long)mag, (long long)n) : FIVEEQ_OK;
}
int check_n_bins(int32_t n_bins) {
    return n_bins < 1 || n_bins > HIST_MAX_BINS ? fail(FIVEEQ_E_INVALID, "n_bins=%d outside 1..%d", n_bins, HIST_MAX_BINS) : FIVEEQ_OK;
}
// pointers by name: the first NULL among the required ones, then the first misaligned one (NULL counts as aligned)
struct NamedPtr {
    const char* name;
    const void* p;
    size_t align = 1;
    bool required = true;
};
using NamedPtrs = std::initializer_list<NamedPtr>;
int check_not_null(NamedPtrs ptrs) {
    for (const NamedPtr& a : ptrs)
        if (a.required && !a.p) return fail(FIVEEQ_E_INVALID, "%s is NULL", a.name);
    return FIVEEQ_OK;
}
int check_aligned(NamedPtrs ptrs) {
    for (const NamedPtr& a : ptrs)
        if (misaligned(a.p, a.align)) return fail(FIVEEQ_E_INVALID, "%s must be %d-byte aligned", a.name, (int)a.align);
    return FIVEEQ_OK;
}
// the optional forcing scales of a stored-row pass: fscale and the table fext come together, and categories need both
int check_fext(int32_t n_fext, const void* fscale, const void* fext) {
    if (n_fext < 0 || n_fext > MAX_FEXT) return fail(FIVEEQ_E_INVALID, "n_fext=%d outside 0..%d", n_fext, MAX_FEXT);
    if (n_fext > 0 && fscale && !fext) return fail(FIVEEQ_E_INVALID, "fscale with n_fext=%d categories needs fext: fext is NULL", n_fext);
    if (n_fext > 0 && fext && !fscale) return fail(FIVEEQ_E_INVALID, "fext with n_fext=%d categories needs fscale: fscale is NULL", n_fext);
    if (n_fext > 0 && !fscale) return fail(FIVEEQ_E_INVALID, "n_fext=%d without fscale and fext", n_fext);
    return FIVEEQ_OK;
}
// workgroups of `chunk` members each over n members: the x extent of a grid
int member_chunks(int64_t n, int64_t chunk, int64_t* chunks) {
    *chunks = (n + chunk - 1) / chunk;
    return *chunks > 0x7fffffffLL ? fail(FIVEEQ_E_INVALID, "n_members too large") : FIVEEQ_OK;
}

// ---- the wide / narrow split of a pass over stored rows -------------------------------------------------------
// 16-byte accesses where every lane's address of every row the pass reads or writes (the member index a multiple of the
// lane's members) is aligned — the pass's own `wide` condition on its bases and strides: the members [0, n_vec) in whole
// lanes.  The ragged tail (fewer members than a lane's) and unaligned rows take the element accesses, in a launch of their
// own on the columns from n_vec.
template <typename T>
constexpr int64_t PER16 = 16 / (int64_t)sizeof(T);
template <typename T>
int64_t wide_members(bool wide, int64_t n) { return wide ? n / PER16<T> * PER16<T> : 0; }
// launch(std::true_type / std::false_type: 16-byte or element accesses, first member, members)
template <typename Launch>
void launch_split(int64_t n_vec, int64_t n, const Launch& launch) {
    if (n_vec > 0) launch(std::true_type{}, (int64_t)0, n_vec);
    if (n_vec < n) launch(std::false_type{}, n_vec, n - n_vec);
}
// f(std::integral_constant<int, N>) for the N of LO..HI that v is; the caller has checked that v is one of them
template <int LO, int HI, typename F>
void dispatch_count(int v, const F& f) {
    if constexpr (LO == HI) f(std::integral_constant<int, LO>{});
    else if (v == LO) f(std::integral_constant<int, LO>{});
    else dispatch_count<LO + 1, HI>(v, f);
}

// ---- pool layouts with a compiled kernel --------------------------------------------------
// X(P0, P1, P2): pools of gas 0, 1, 2 (0 = gas absent).  CO2-like gases carry 4 pools,
// single-lifetime gases (CH4, N2O, HFCs) carry 1.
#define FIVEEQ_LAYOUTS(X) \
    X(1, 0, 0) X(2, 0, 0) X(3, 0, 0) X(4, 0, 0) \
    X(1, 1, 0) X(4, 1, 0) X(4, 4, 0)            \
    X(1, 1, 1) X(4, 1, 1) X(4, 4, 1) X(4, 4, 4)

// the layout code of n_gas <= 3 pool counts: P0 P1 P2 as decimal digits (0 = gas absent)
int layout_code(int n_gas, const int32_t* n_pools) {
    int p[3] = {0, 0, 0};
    for (int g = 0; g < n_gas; ++g) p[g] = n_pools[g];
    return p[0] * 100 + p[1] * 10 + p[2];
}
int layout_code(const fiveeq_model* m) {
    int32_t p[3] = {0, 0, 0};
    for (int g = 0; g < m->n_gas; ++g) p[g] = m->gas[g].n_pools;
    return layout_code(3, p);
}

// the refusals of a layout, one text each
int no_kernel(int code) { return fail(FIVEEQ_E_UNSUPPORTED, "pool layout %03d has no compiled kernel", code); }
int no_misfit_form(int code) { return fail(FIVEEQ_E_INVALID, "pool layout %03d has no misfit form", code); }
int no_forcing_form(int code) { return fail(FIVEEQ_E_INVALID, "pool layout %03d has no forcing form", code); }

bool layout_ok(int code) {
    switch (code) {
#define X(a, b, c) case (a) * 100 + (b) * 10 + (c):
        FIVEEQ_LAYOUTS(X)
#undef X
        return true;
        default:
            return false;
    }
}

// ---- validation (host; nothing reaches the GPU unless this passes) -------------------------
int check_model(const fiveeq_model* m) {
    if (!m) return fail(FIVEEQ_E_INVALID, "model is NULL");
    if (m->n_gas < 1 || m->n_gas > FIVEEQ_MAX_GAS)
        return fail(FIVEEQ_E_INVALID, "n_gas=%d outside 1..%d", m->n_gas, FIVEEQ_MAX_GAS);
    if (!(m->dt > 0.0) || !std::isfinite(m->dt)) return fail(FIVEEQ_E_INVALID, "dt=%g must be finite and > 0", m->dt);
    for (int j = 0; j < FIVEEQ_N_BOX; ++j)
        if (!(m->d[j] > 0.0) || !std::isfinite(m->d[j]))
            return fail(FIVEEQ_E_INVALID, "d[%d]=%g must be finite and > 0", j, m->d[j]);
    if (std::isnan(m->iirf_max)) return fail(FIVEEQ_E_INVALID, "iirf_max is NaN");
    for (int g = 0; g < m->n_gas; ++g) {
        const fiveeq_gas& gs = m->gas[g];
        if (gs.n_pools < 1 || gs.n_pools > FIVEEQ_MAX_POOLS)
            return fail(FIVEEQ_E_INVALID, "gas %d: n_pools=%d outside 1..%d", g, gs.n_pools, FIVEEQ_MAX_POOLS);
        for (int i = 0; i < gs.n_pools; ++i)
            if (!(gs.tau[i] > 0.0) || !std::isfinite(gs.tau[i]) || !std::isfinite(gs.a[i]))
                return fail(FIVEEQ_E_INVALID, "gas %d pool %d: a=%g tau=%g invalid", g, i, gs.a[i], gs.tau[i]);
        if (!(gs.g1 != 0.0) || !std::isfinite(gs.g1) || !std::isfinite(gs.g0))
            return fail(FIVEEQ_E_INVALID, "gas %d: g0=%g g1=%g invalid", g, gs.g0, gs.g1);
        if (!(gs.C0 > 0.0) || !std::isfinite(gs.C0)) return fail(FIVEEQ_E_INVALID, "gas %d: C0=%g must be > 0", g, gs.C0);
        if (!(gs.emis2conc > 0.0) || !std::isfinite(gs.emis2conc))
            return fail(FIVEEQ_E_INVALID, "gas %d: emis2conc=%g must be > 0", g, gs.emis2conc);
    }
    if (!layout_ok(layout_code(m))) return no_kernel(layout_code(m));
    return FIVEEQ_OK;
}

int check_run(const fiveeq_model* m, int64_t n, int64_t ld, const void* drive, int32_t n_steps, int32_t t_begin,
              int32_t t_end, const void* r, const void* q, const void* R, const void* S) {
    if (int rc = check_model(m)) return rc;
    if (n < 1) return fail(FIVEEQ_E_INVALID, "n_members=%lld must be >= 1", (long long)n);
    if (ld < n) return fail(FIVEEQ_E_INVALID, "ld=%lld < n_members=%lld", (long long)ld, (long long)n);
    if (n_steps < 1) return fail(FIVEEQ_E_INVALID, "n_steps=%d must be >= 1", n_steps);
    if (t_begin < 0 || t_end > n_steps || t_begin > t_end)
        return fail(FIVEEQ_E_INVALID, "step range [%d,%d) outside [0,%d)", t_begin, t_end, n_steps);
    if (!drive || !r || !q || !R || !S)
        return fail(FIVEEQ_E_INVALID, "NULL device pointer (drive=%p r=%p q=%p R=%p S=%p)", drive, r, q, R, S);
    return FIVEEQ_OK;
}

// ---- model -> kernel-precision constants ---------------------------------------------------
template <typename T>
KModel<T> make_kmodel(const fiveeq_model* m) {
    KModel<T> km;
    std::memset(&km, 0, sizeof km);
    for (int g = 0; g < m->n_gas; ++g) {
        const fiveeq_gas& gs = m->gas[g];
        KGas<T>& kg = km.gas[g];
        for (int i = 0; i < gs.n_pools; ++i) {
            kg.ndt_over_tau[i] = (T)(-m->dt / gs.tau[i]);
            kg.atc[i] = (T)(gs.a[i] * gs.tau[i] * gs.emis2conc);
        }
        kg.g0 = (T)gs.g0;
        kg.inv_g1 = (T)(1.0 / gs.g1);
        kg.ra = (T)gs.ra;
        kg.inv_c = (T)(1.0 / gs.emis2conc);
        kg.C0 = (T)gs.C0;
        kg.inv_C0 = (T)(1.0 / gs.C0);
        kg.sqrtC0 = (T)std::sqrt(gs.C0);
        kg.f1 = (T)gs.f[0];
        kg.f2 = (T)gs.f[1];
        kg.f3 = (T)gs.f[2];
    }
    for (int j = 0; j < 2; ++j) km.em1_d[j] = (T)std::expm1(-m->dt / m->d[j]);
    km.iirf_max = (T)m->iirf_max;
    km.dt = (T)m->dt;
    return km;
}

// One member per lane, one 256-thread workgroup per 256 members (3907 workgroups at 1M members,
// >> 256 CUs); workgroup b owns the same members in every launch.
int64_t member_blocks(int64_t n) { return (n + FIVEEQ_BLOCK - 1) / FIVEEQ_BLOCK; }

// the workgroups of one launch over n members, per_block of them per workgroup
int grid_blocks(int64_t n, int64_t per_block, unsigned& blocks) {
    const int64_t b = (n + per_block - 1) / per_block;
    if (b > 0x7fffffffLL) return fail(FIVEEQ_E_INVALID, "n_members too large for one launch");
    blocks = (unsigned)b;
    return FIVEEQ_OK;
}

// the bin-index ring of the streamed histograms (step_kernel / fused_kernel <..., BINS = true>)
struct BinRing {
    unsigned short* ring = nullptr;
    int ring_rows = 0;
    double lo = 0.0, inv_w = 0.0;
    int n_bins = 0;
};

// the misfit accumulators of the constrained forms (step_kernel / fused_kernel <..., MISFIT = true>): obs [n_steps][4] and
// misfit [3][ld], fp64 both
struct MisfitRows {
    const double* obs = nullptr;
    double* misfit = nullptr;
};

// the per-member forcing scales (step_kernel / step_scen_kernel / fused_kernel <..., FORC = true>): fscale [G + n_fext][ld] in
// kernel precision, gas rows first, and the shared table fext [n_steps][MAX_FEXT] (the scenario forms: one table per scenario,
// [n_scen][n_steps][MAX_FEXT])
template <typename T>
struct ForcRows {
    const T* fscale = nullptr;
    const T* fext = nullptr;
    int n_fext = 0;
};

// the fifteen arguments every stepping entry point takes (model ... T_stats), in the order of the C ABI: each extern "C"
// wrapper brace-initialises one
template <typename T>
struct BaseArgs {
    const fiveeq_model* m;
    int64_t n, ld;
    const T* drive;
    int32_t n_steps, t_begin, t_end;
    const T *r, *q;
    T *R, *S, *C_traj, *T_traj;
    int32_t n_rows;
    double* stats;
};

// everything one C-ABI call hands its launches: filled by make_args() and the checker of each optional feature
template <typename T>
struct RunArgs : BaseArgs<T> {
    KModel<T> km;
    int code;
    int n_gas;
    int packing;                 // the fp32 packing switch as this call found it
    bool stream_rows;            // the per-step launches of this call take the STREAMED (non-temporal) row form
    bool scen = false;           // the call is of a scenario family (step_scen_kernel, fused_kernel<.., SCEN>), whatever n_scen
    int n_scen;                  // scenarios (the scenario forms; 1 without the scenario axis)
    T* cumE = nullptr;           // the inverse form's cumulative emissions
    int conc_mask = 0;           // the mixed drive's per-gas mask (fiveeq_run_mixed: bit g set = gas g concentration-driven)
    BinRing br;                  // the histogram forms' ring (else none)
    MisfitRows mf;               // the constrained forms' accumulators (else none)
    ForcRows<T> fc;              // the forcing forms' scale rows and table (else none)
    const T* mforc = nullptr;    // the member-forcing forms' rows [n_steps][ld] (else none)
    UniformRows<T> uni{};        // the single-valued parameter rows of fiveeq_run_uniform (mask 0: every row is loaded)
};

// ---- packed fp32 lanes: two members per lane (fiveeq_math.hpp, "Lane value types") ----------------------------
// The fp32 entry points run the packed kernels whenever the rows allow 8-byte accesses: even row stride, every row
// pointer 8-byte aligned, at least two members.  Otherwise (odd ld, a sub-range starting at an odd member) the
// one-member-per-lane kernels run; both give the same bits.  fiveeq_set_f32_packing(0) forces the scalar kernels (A/B
// measurements, and the tests that compare the two).
// Process-wide and changeable at any time from any thread: a relaxed atomic, read ONCE per C-ABI call (make_args), so that
// every launch of one call takes the same kernel shape.
std::atomic<int> g_f32_packing{1};

// ---- cache policy of the per-step kernel's state and parameter rows (fiveeq_step.hpp, step_kernel<..., NT>) --------------
// STREAMED (non-temporal) pays exactly when the rows of this launch cannot be in the Infinity Cache at the next step:
//   * the launch's own rows fill it: n members x (S (SP + 2) + 3G + 2) words >= the cache, for S scenarios (1 without the
//     scenario axis: each scenario carries its own state rows, the parameter rows are shared) — false for the chunks of a
//     chunk-major schedule (the engine sizes them to fit), true for an unchunked multi-million-member launch; and
//   * the ensemble they are a part of (row length ld: the halves of a two-stream split share the cache) is at least twice
//     the cache — between one and two cache sizes the default policy still hits often enough to win (2M fp64 members, 304 MB:
//     +13 % streamed; 4M: -9 %; profiles/r05/step_row_policy_ab.txt).
// fiveeq_set_row_policy overrides the rule process-wide (A/B measurements, the bit-identity tests); like the packing switch
// it is a relaxed atomic read ONCE per C-ABI call.
constexpr int64_t INFINITY_CACHE_BYTES = (int64_t)256 << 20;       // MI355X (MI355X_MICROARCH.md)
std::atomic<int> g_row_policy{FIVEEQ_ROWS_AUTO};

bool rows_streamed(int policy, int n_gas, int sum_pools, int n_scen, int64_t n, int64_t ld, int word) {
    if (policy != FIVEEQ_ROWS_AUTO) return policy == FIVEEQ_ROWS_STREAMED;
    const int64_t per_member = (int64_t)word * ((int64_t)n_scen * (sum_pools + 2) + 3 * n_gas + 2);
    return n * per_member >= INFINITY_CACHE_BYTES && ld * per_member >= 2 * INFINITY_CACHE_BYTES;
}

template <typename T>
struct LaneOf {
    using Packed = T;                              // fp64 has no packed VALU forms: one member per lane
    static bool can_pack(const RunArgs<T>&) { return false; }
};
template <>
struct LaneOf<float> {
    using Packed = float2v;
    static bool can_pack(const RunArgs<float>& a) {
        if (!a.packing || a.n < 2 || (a.ld & 1)) return false;
        const uintptr_t bits = (uintptr_t)a.r | (uintptr_t)a.q | (uintptr_t)a.R | (uintptr_t)a.S | (uintptr_t)a.C_traj |
                               (uintptr_t)a.T_traj;
        return (bits & 7u) == 0;
    }
};

// the layouts with MISFIT instantiations: a lone 4-pool gas (CO2-only) and 4 + 1 + 1 (CO2, CH4, N2O)
constexpr bool misfit_layout(int p0, int p1, int p2) { return (p0 == 4 && p1 == 0 && p2 == 0) || (p0 == 4 && p1 == 1 && p2 == 1); }
constexpr bool misfit_layout(int code) { return misfit_layout(code / 100, code / 10 % 10, code % 10); }
// ... and the PACKED fp32 fused kernel carries it for 4 + 1 + 1 only.  For {4} the two members' accumulators (12 KiB of LDS per
// workgroup on top of 20 KiB) would cost the packed form two waves per SIMD (6 -> 4); those runs take the one-member-per-lane
// fp32 fused kernel, which keeps its plain counterpart's 7 waves (same bits either way: packed lanes mirror the scalar ones).
constexpr bool misfit_packed_fused(int p0, int p1, int p2) { return p0 == 4 && p1 == 1 && p2 == 1; }
// the layouts with FORC instantiations: those that have the misfit form, with which it combines
constexpr bool forcing_layout(int p0, int p1, int p2) { return misfit_layout(p0, p1, p2); }
constexpr bool forcing_layout(int code) { return misfit_layout(code); }
// the layouts with step_uniform_kernel instantiations: the same line again
constexpr bool uniform_layout(int p0, int p1, int p2) { return misfit_layout(p0, p1, p2); }
constexpr bool uniform_layout(int code) { return misfit_layout(code); }
// the layouts with fused_mixed_kernel instantiations (a proper per-gas drive mask): 4 + 1 + 1
constexpr bool mixed_layout(int code) { return code == 411; }

// ---- the two launchers: one step of the per-step kernel, one span [t_begin, t_end) of the time-fused kernel ----------------
// The compile-time flags pick the kernel family; packing, the row policy and the pool layout are decided here per launch.
// SCEN: the scenario axis (step_scen_kernel; the fused kernel with the scenario as blockIdx.y).
// FORC: the per-member forcing scales (with or without MISFIT, or with SCEN: the scale rows shared by the scenarios, a table
// per scenario).
// MFORC: a per-member forcing row per step on top of FORC (step_mforc_kernel, fused_mforc_kernel), with or without MISFIT.
template <typename T, bool BINS = false, bool MISFIT = false, bool SCEN = false, bool FORC = false, bool MFORC = false>
int launch_step(const RunArgs<T>& a, int t, hipStream_t st) {
    using P = typename LaneOf<T>::Packed;
    static_assert(BINS + MISFIT + SCEN <= 1, "the histogram ring, the misfit and the scenario axis are separate forms");
    static_assert(!FORC || !BINS, "the forcing scales combine with the misfit or the scenario axis only");
    static_assert(!MFORC || (FORC && !SCEN), "the member-forcing rows ride on the forcing-scale forms without the scenario axis");
    const bool packed = LaneOf<T>::can_pack(a) && (!BINS || (((uintptr_t)a.br.ring) & 3) == 0) &&
                        (!FORC || (((uintptr_t)a.fc.fscale) & 7) == 0) && (!MFORC || (((uintptr_t)a.mforc) & 7) == 0);
    unsigned blocks;
    if (int rc = grid_blocks(a.n, (int64_t)FIVEEQ_STEP_BLOCK * (packed ? 2 : 1), blocks)) return rc;
    const dim3 grid(blocks), block(FIVEEQ_STEP_BLOCK);
    switch (a.code) {
#define FIVEEQ_STEP_LAUNCH(V, p0, p1, p2, NT)                                                                                     \
    do {                                                                                                                          \
        if constexpr (MFORC)                                                                                                      \
            hipLaunchKernelGGL((step_mforc_kernel<V, p0, p1, p2, MISFIT>), grid, block, 0, st, a.km, a.drive, a.n_steps, t, a.n,  \
                               a.ld, a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats, a.mf.obs, a.mf.misfit,            \
                               a.fc.fscale, a.fc.fext, a.fc.n_fext, a.mforc);                                                     \
        else if constexpr (SCEN)                                                                                                  \
            hipLaunchKernelGGL((step_scen_kernel<V, p0, p1, p2, NT, FORC>), grid, block, 0, st, a.km, a.drive, a.n_steps, t, a.n, \
                               a.ld, a.n_scen, a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats, a.fc.fscale, a.fc.fext, \
                               a.fc.n_fext);                                                                                      \
        else                                                                                                                      \
            hipLaunchKernelGGL((step_kernel<V, p0, p1, p2, BINS, NT, MISFIT, FORC>), grid, block, 0, st, a.km, a.drive,           \
                               a.n_steps, t, a.n, a.ld, a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats, a.br.ring,     \
                               a.br.ring_rows, a.br.lo, a.br.inv_w, a.br.n_bins, a.mf.obs, a.mf.misfit, a.fc.fscale, a.fc.fext,   \
                               a.fc.n_fext);                                                                                      \
    } while (0)
#define FIVEEQ_UNIFORM_LAUNCH(V, p0, p1, p2, NT)                                                                            \
    hipLaunchKernelGGL((step_uniform_kernel<V, p0, p1, p2, NT>), grid, block, 0, st, a.km, a.drive, a.n_steps, t, a.n, a.ld,    \
                       a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats, a.uni)
#define X(p0, p1, p2)                                                                             \
    case (p0) * 100 + (p1) * 10 + (p2):                                                           \
        if constexpr (MISFIT && !misfit_layout(p0, p1, p2)) {                                     \
            return no_misfit_form(a.code);                                                        \
        } else if constexpr (FORC && !forcing_layout(p0, p1, p2)) {                               \
            return no_forcing_form(a.code);                                                       \
        } else {                                                                                  \
            /* the single-valued rows: plain launches of the layouts that carry the form (a.uni.mask is 0 elsewhere) */ \
            if constexpr (!BINS && !MISFIT && !FORC && !SCEN && uniform_layout(p0, p1, p2)) {     \
                if (a.uni.mask != 0) {                                                            \
                    if (a.stream_rows) {                                                          \
                        if (packed) FIVEEQ_UNIFORM_LAUNCH(P, p0, p1, p2, true);                   \
                        else FIVEEQ_UNIFORM_LAUNCH(T, p0, p1, p2, true);                          \
                    } else {                                                                      \
                        if (packed) FIVEEQ_UNIFORM_LAUNCH(P, p0, p1, p2, false);                  \
                        else FIVEEQ_UNIFORM_LAUNCH(T, p0, p1, p2, false);                         \
                    }                                                                             \
                    break;                                                                        \
                }                                                                                 \
            }                                                                                     \
            /* the streamed row form: plain and scenario launches only (the engine schedules misfit runs chunk-major) */ \
            if constexpr (!BINS && !MISFIT && !FORC) {                                                   \
                if (a.stream_rows) {                                                              \
                    if (packed) FIVEEQ_STEP_LAUNCH(P, p0, p1, p2, true);                          \
                    else FIVEEQ_STEP_LAUNCH(T, p0, p1, p2, true);                                 \
                    break;                                                                        \
                }                                                                                 \
            }                                                                                     \
            if (packed) FIVEEQ_STEP_LAUNCH(P, p0, p1, p2, false);                                 \
            else FIVEEQ_STEP_LAUNCH(T, p0, p1, p2, false);                                        \
        }                                                                                         \
        break;
        FIVEEQ_LAYOUTS(X)
#undef X
#undef FIVEEQ_UNIFORM_LAUNCH
#undef FIVEEQ_STEP_LAUNCH
        default:
            return no_kernel(a.code);
    }
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

template <typename T, bool INV = false, bool BINS = false, bool COMP = false, bool MISFIT = false, bool SCEN = false,
          bool FORC = false, bool MFORC = false>
int launch_fused(const RunArgs<T>& a, int t_begin, int t_end, hipStream_t st) {
    using P = typename LaneOf<T>::Packed;
    static_assert(!MFORC || (FORC && !INV && !SCEN), "the member-forcing rows ride on the forward forcing-scale forms only");
    static_assert(!FORC || (!BINS && !COMP), "the forcing scales are carried by the plain forward and inverse forms only");
    static_assert(!MISFIT || (!BINS && !COMP), "the misfit is carried by the plain forward and inverse forms only");
    static_assert(!SCEN || (!INV && !BINS && !COMP && !MISFIT), "the scenario axis is carried by the plain forward form only");
    constexpr bool HAS_PACKED = !INV && !std::is_same<P, T>::value;     // the inverse form has no packed instantiation
    // packed lanes store two 2-byte bin indices as one 4-byte word: the ring rows must be 4-byte aligned too; the misfit forms
    // have a packed instantiation for some layouts only (misfit_packed_fused) — decided HERE, before the grid is sized for it
    const bool packed = HAS_PACKED && (!MISFIT || misfit_packed_fused(a.code / 100, a.code / 10 % 10, a.code % 10)) &&
                        LaneOf<T>::can_pack(a) && (!BINS || (((uintptr_t)a.br.ring) & 3) == 0) &&
                        (!FORC || (((uintptr_t)a.fc.fscale) & 7) == 0) && (!MFORC || (((uintptr_t)a.mforc) & 7) == 0);
    unsigned blocks;
    if (int rc = grid_blocks(a.n, (int64_t)FIVEEQ_BLOCK * (packed ? 2 : 1), blocks)) return rc;
    const dim3 grid(blocks, (unsigned)a.n_scen), block(FIVEEQ_BLOCK);     // the scenarios are rows of the grid
    switch (a.code) {
#define FIVEEQ_FUSED_LAUNCH(V, p0, p1, p2, I)                                                                                    \
    do {                                                                                                                         \
        if constexpr (MFORC)                                                                                                     \
            hipLaunchKernelGGL((fused_mforc_kernel<V, p0, p1, p2, MISFIT>), grid, block, FIVEEQ_FUSED_DYN_LDS, st, a.km, a.drive, \
                               a.n_steps, t_begin, t_end, a.n, a.ld, a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats,  \
                               a.mf.obs, a.mf.misfit, a.fc.fscale, a.fc.fext, a.fc.n_fext, a.mforc);                             \
        else                                                                                                                     \
            hipLaunchKernelGGL((fused_kernel<V, p0, p1, p2, I, BINS, COMP, MISFIT, SCEN, FORC>), grid, block,                    \
                               FIVEEQ_FUSED_DYN_LDS, st, a.km, a.drive, a.n_steps, t_begin, t_end, a.n, a.ld, a.r, a.q, a.R,     \
                               a.S, a.cumE, a.C_traj, a.T_traj, a.n_rows, a.stats, a.br.ring, a.br.ring_rows, a.br.lo,           \
                               a.br.inv_w, a.br.n_bins, a.mf.obs, a.mf.misfit, a.fc.fscale, a.fc.fext, a.fc.n_fext);             \
    } while (0)
#define X(p0, p1, p2)                                                                                  \
    case (p0) * 100 + (p1) * 10 + (p2):                                                                \
        if constexpr (MISFIT && !misfit_layout(p0, p1, p2)) {                                          \
            return no_misfit_form(a.code);                                                             \
        } else if constexpr (FORC && !forcing_layout(p0, p1, p2)) {                                    \
            return no_forcing_form(a.code);                                                            \
        } else {                                                                                       \
            if constexpr (HAS_PACKED && (!MISFIT || misfit_packed_fused(p0, p1, p2))) {                \
                if (packed) {                                                                          \
                    FIVEEQ_FUSED_LAUNCH(P, p0, p1, p2, false);                                                   \
                    break;                                                                             \
                }                                                                                      \
            }                                                                                          \
            FIVEEQ_FUSED_LAUNCH(T, p0, p1, p2, INV);                                                           \
        }                                                                                              \
        break;
        FIVEEQ_LAYOUTS(X)
#undef X
#undef FIVEEQ_FUSED_LAUNCH
        default:
            return no_kernel(a.code);
    }
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// ---- the two drivers: every stepping entry point launches through one of them -------------------------------------------
// per step: launch(t) for each timestep t of [t_begin, t_end)
template <typename T, typename Launch>
int each_step(const RunArgs<T>& a, Launch&& launch) {
    for (int t = a.t_begin; t < a.t_end; ++t)
        if (int rc = launch(t)) return rc;
    return FIVEEQ_OK;
}

// per span: launch(t0, t1) over consecutive spans of k_steps steps (0, or more than the range: one span, the whole range)
template <typename T, typename Launch>
int each_span(const RunArgs<T>& a, int k_steps, Launch&& launch) {
    if (k_steps == 0 || k_steps > a.t_end - a.t_begin) k_steps = a.t_end - a.t_begin;   // also keeps t + k_steps inside int32
    for (int t = a.t_begin; t < a.t_end; t += k_steps)
        if (int rc = launch(t, t + k_steps < a.t_end ? t + k_steps : a.t_end)) return rc;
    return FIVEEQ_OK;
}

// ---- validation of one call: make_args() for what every stepping entry point takes, one checker per optional feature ------
template <typename T>
int make_args(RunArgs<T>& a, const BaseArgs<T>& b, int32_t n_scen = 1) {
    if (int rc = check_run(b.m, b.n, b.ld, b.drive, b.n_steps, b.t_begin, b.t_end, b.r, b.q, b.R, b.S)) return rc;
    if (b.n_rows < 0) return fail(FIVEEQ_E_INVALID, "n_rows=%d must be >= 0", b.n_rows);
    static_cast<BaseArgs<T>&>(a) = b;
    a.km = make_kmodel<T>(b.m);
    a.code = layout_code(b.m);
    a.n_gas = b.m->n_gas;
    a.packing = g_f32_packing.load(std::memory_order_relaxed);
    int sum_pools = 0;
    for (int g = 0; g < b.m->n_gas; ++g) sum_pools += b.m->gas[g].n_pools;
    a.stream_rows = rows_streamed(g_row_policy.load(std::memory_order_relaxed), b.m->n_gas, sum_pools, n_scen, b.n, b.ld,
                                  (int)sizeof(T));
    a.n_scen = n_scen;
    return FIVEEQ_OK;
}

// the bin-index ring (where the ring is optional, the caller leaves a NULL ring unchecked)
template <typename T>
int check_ring(RunArgs<T>& a, double lo, double hi, int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows) {
    if (n_bins < 1 || n_bins > HIST_MAX_BINS) return fail(FIVEEQ_E_INVALID, "n_bins=%d outside 1..%d", n_bins, HIST_MAX_BINS);
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi)) return fail(FIVEEQ_E_INVALID, "need finite lo < hi");
    if (!bin_ring) return fail(FIVEEQ_E_INVALID, "bin_ring is NULL");
    if (ring_rows < 1) return fail(FIVEEQ_E_INVALID, "ring_rows=%d must be >= 1", ring_rows);
    if (((uintptr_t)bin_ring) & 1) return fail(FIVEEQ_E_INVALID, "bin_ring must be 2-byte aligned");
    a.br.ring = bin_ring;
    a.br.ring_rows = ring_rows;
    a.br.lo = lo;
    a.br.inv_w = (double)n_bins / (hi - lo);
    a.br.n_bins = n_bins;
    return FIVEEQ_OK;
}

// the misfit accumulators, and a pool layout that carries them
template <typename T>
int check_misfit(RunArgs<T>& a, const double* obs, double* misfit) {
    if (!obs || !misfit) return fail(FIVEEQ_E_INVALID, "NULL misfit pointer (obs=%p misfit=%p)", (const void*)obs, (void*)misfit);
    if ((((uintptr_t)obs) | ((uintptr_t)misfit)) & 7) return fail(FIVEEQ_E_INVALID, "obs and misfit must be 8-byte aligned");
    if (!misfit_layout(a.code))
        return fail(FIVEEQ_E_INVALID, "pool layout %03d has no misfit form (pools {4} and 4+1+1 have)", a.code);
    a.mf.obs = obs;
    a.mf.misfit = misfit;
    return FIVEEQ_OK;
}

// the per-member forcing scales: the scale rows, the shared table of n_fext categories, and a pool layout that carries them
template <typename T>
int check_forcing(RunArgs<T>& a, const T* fscale, const T* fext, int32_t n_fext) {
    if (n_fext < 0 || n_fext > MAX_FEXT) return fail(FIVEEQ_E_INVALID, "n_fext=%d outside 0..%d", n_fext, MAX_FEXT);
    if (!fscale) return fail(FIVEEQ_E_INVALID, "fscale is NULL");
    if (((uintptr_t)fscale) & (sizeof(T) - 1)) return fail(FIVEEQ_E_INVALID, "fscale must be %d-byte aligned", (int)sizeof(T));
    if (n_fext > 0 && !fext) return fail(FIVEEQ_E_INVALID, "fext is NULL with n_fext=%d", n_fext);
    if (((uintptr_t)fext) & (sizeof(T) - 1)) return fail(FIVEEQ_E_INVALID, "fext must be %d-byte aligned", (int)sizeof(T));
    if (!forcing_layout(a.code))
        return fail(FIVEEQ_E_INVALID, "pool layout %03d has no forcing form (pools {4} and 4+1+1 have)", a.code);
    a.fc.fscale = fscale;
    a.fc.fext = n_fext > 0 ? fext : fscale;      // n_fext == 0: no kernel reads the table (no record, no staging); kept non-NULL
    a.fc.n_fext = n_fext;
    return FIVEEQ_OK;
}

// the member-forcing rows mforc [n_mforc_rows][ld] of a forcing-scale call (check_forcing has passed: the layout carries the
// form): present, aligned to the kernel's word, and long enough for the steps of this call
template <typename T>
int check_mforc(RunArgs<T>& a, const T* mforc, int32_t n_mforc_rows) {
    if (int rc = check_not_null({{"mforc", mforc}})) return rc;
    if (int rc = check_aligned({{"mforc", mforc, sizeof(T)}})) return rc;
    if (n_mforc_rows < a.t_end)
        return fail(FIVEEQ_E_INVALID, "n_mforc_rows=%d < t_end=%d: mforc holds one row per step from step 0", n_mforc_rows, a.t_end);
    a.mforc = mforc;
    return FIVEEQ_OK;
}

// the single-valued parameter rows (step_uniform_kernel): the caller's mask over the 3G rows of r and the 2 of q, and their
// values (host).  A layout without the form keeps mask 0 and launches what the plain call launches.
template <typename T>
int check_uniform(RunArgs<T>& a, uint32_t mask, const T* values) {
    const int n_rows = 3 * a.n_gas + 2;
    if (mask >> n_rows) return fail(FIVEEQ_E_INVALID, "uniform mask 0x%x has bits at or above %d (3 n_gas + 2 rows)", mask, n_rows);
    if (mask != 0 && !values) return fail(FIVEEQ_E_INVALID, "uniform values is NULL with mask 0x%x", mask);
    if (mask == 0 || !uniform_layout(a.code)) return FIVEEQ_OK;
    a.uni.mask = mask;
    for (int k = 0; k < n_rows; ++k) a.uni.val[k] = (mask >> k) & 1u ? values[k] : T(0);
    return FIVEEQ_OK;
}

// the per-gas drive mask of fiveeq_run_mixed: bit g set = gas g is concentration-driven; no bit at or above the model's n_gas
template <typename T>
int check_conc_mask(RunArgs<T>& a, int32_t conc_mask) {
    if (conc_mask < 0) return fail(FIVEEQ_E_INVALID, "conc_mask=%d must be >= 0", conc_mask);
    if (conc_mask >> a.n_gas)
        return fail(FIVEEQ_E_INVALID, "conc_mask=0x%x has bits at or above n_gas=%d", (unsigned)conc_mask, a.n_gas);
    a.conc_mask = conc_mask;
    return FIVEEQ_OK;
}

// the scenario axis: one parameter ensemble under n_scen emission scenarios (step_scen_kernel, fused_kernel<.., SCEN>)
constexpr int MAX_SCENARIOS = 64;
int check_scen(int32_t n_scen) {
    if (n_scen < 1 || n_scen > MAX_SCENARIOS) return fail(FIVEEQ_E_INVALID, "n_scen=%d outside 1..%d", n_scen, MAX_SCENARIOS);
    return FIVEEQ_OK;
}

// the form of a run (FIVEEQ_FORM_*) and its span length: k_min is 1 where k_steps has no "whole range" value 0
int check_form(int32_t form, int32_t k_steps, int32_t k_min) {
    if (form != FIVEEQ_FORM_PER_STEP && form != FIVEEQ_FORM_FUSED)
        return fail(FIVEEQ_E_INVALID, "form=%d: FIVEEQ_FORM_PER_STEP (0) or FIVEEQ_FORM_FUSED (1)", form);
    if (k_steps < k_min) return fail(FIVEEQ_E_INVALID, "k_steps=%d must be >= %d", k_steps, k_min);
    return FIVEEQ_OK;
}

// ---- the entry points (validated: nothing is launched before every check has passed) ---------------------------------------
// What a forward call carries beyond the base arguments, in the order of the C ABI: the scenario axis and its count
// (fiveeq_run_scen, fiveeq_run_scen_forc), the forcing rows (fiveeq_run_forc, fiveeq_run_scen_forc) and the misfit rows —
// REQUIRED by fiveeq_run_obs, OPTIONAL for fiveeq_run_forc (obs and misfit both NULL, or both set); the same for the
// plan_create twins.  The plain family (fiveeq_step/run/run_fused/run_ksteps, fiveeq_plan_create) carries none: {}.
enum Use { ABSENT, OPTIONAL, REQUIRED };
template <typename T>
struct Features {
    bool scen = false;           // a scenario family: n_scen is the caller's, checked whatever its value
    int32_t n_scen = 1;
    bool forc = false;           // a forcing family: fc is the caller's
    ForcRows<T> fc;
    Use misfit = ABSENT;
    MisfitRows mf;
    bool uniform = false;        // fiveeq_run_uniform / fiveeq_plan_create_uniform: mask and values are the caller's
    uint32_t mask = 0;
    const T* values = nullptr;   // host, 3G + 2
    bool inv = false;            // fiveeq_run_inverse_forc: cumE is the caller's, required
    T* cumE = nullptr;
    bool mforc = false;          // fiveeq_run_mforc / fiveeq_plan_create_mforc (a forcing family: forc is set too): the rows are the caller's
    const T* mforc_rows = nullptr;
    int32_t n_mforc_rows = 0;
    bool mixed = false;          // fiveeq_run_mixed: conc_mask is the caller's (inv is set when it names a gas)
    int32_t conc_mask = 0;
};

// Every check of a forward call but its last (the form of a run, the range of a plan), in the ONE order every family reports
// in (tests/test_forward_precedence_cpu.py): the scenario count, [a plan: plan_out, cleared before anything else,] the base
// arguments, the forcing rows, obs and misfit given together, the misfit rows; the single-valued rows of the plain family's
// uniform twins come right behind the base arguments, and so does the cumE of fiveeq_run_inverse_forc — with the drive mask of
// fiveeq_run_mixed in front of it — and a proper mask on a layout without the mixed form (FIVEEQ_E_UNSUPPORTED) comes last.
template <typename T>
int prepare(RunArgs<T>& a, const BaseArgs<T>& b, const Features<T>& f, bool plan = false, void** plan_out = nullptr) {
    if (plan_out) *plan_out = nullptr;
    if (int rc = f.scen ? check_scen(f.n_scen) : FIVEEQ_OK) return rc;
    if (plan && !plan_out) return fail(FIVEEQ_E_INVALID, "plan_out is NULL");
    if (int rc = make_args(a, b, f.n_scen)) return rc;
    a.scen = f.scen;
    if (int rc = f.mixed ? check_conc_mask(a, f.conc_mask) : FIVEEQ_OK) return rc;
    if (f.inv) {
        if (!f.cumE) return fail(FIVEEQ_E_INVALID, "cumE is NULL");
        a.cumE = f.cumE;
    }
    if (int rc = f.uniform ? check_uniform(a, f.mask, f.values) : FIVEEQ_OK) return rc;
    if (int rc = f.forc ? check_forcing(a, f.fc.fscale, f.fc.fext, f.fc.n_fext) : FIVEEQ_OK) return rc;
    if (int rc = f.mforc ? check_mforc(a, f.mforc_rows, f.n_mforc_rows) : FIVEEQ_OK) return rc;
    if (f.misfit == OPTIONAL && (f.mf.obs == nullptr) != (f.mf.misfit == nullptr))
        return fail(FIVEEQ_E_INVALID, "obs and misfit go together: both NULL (no misfit) or both set (obs=%p misfit=%p)",
                    (const void*)f.mf.obs, (void*)f.mf.misfit);
    if (f.misfit == REQUIRED || (f.misfit == OPTIONAL && f.mf.obs))
        if (int rc = check_misfit(a, f.mf.obs, f.mf.misfit)) return rc;
    if (f.mixed && a.conc_mask != 0 && a.conc_mask != (1 << a.n_gas) - 1 && !mixed_layout(a.code))
        return fail(FIVEEQ_E_UNSUPPORTED, "pool layout %03d has no mixed-drive form for conc_mask=0x%x (pools 4+1+1 have)", a.code,
                    (unsigned)a.conc_mask);
    return FIVEEQ_OK;
}

// one kernel family: one launch per step, or the fused kernel over spans of k_steps steps
template <typename T, bool MISFIT, bool SCEN, bool FORC, bool MFORC = false>
int run_family(const RunArgs<T>& a, int32_t form, int32_t k_steps, hipStream_t st) {
    if (form == FIVEEQ_FORM_PER_STEP)
        return each_step(a, [&](int t) { return launch_step<T, false, MISFIT, SCEN, FORC, MFORC>(a, t, st); });
    return each_span(a, k_steps,
                     [&](int t0, int t1) { return launch_fused<T, false, false, false, MISFIT, SCEN, FORC, MFORC>(a, t0, t1, st); });
}

// the forward model in the family prepare() found: plain, MISFIT, SCEN, FORC, FORC + MISFIT, SCEN + FORC, or FORC + MFORC with or
// without MISFIT (the eight that are compiled) — picked once per C call, outside the launch loops
template <typename T>
int run_form(const RunArgs<T>& a, int32_t form, int32_t k_steps, hipStream_t st) {
    const bool forc = a.fc.fscale != nullptr, misfit = a.mf.misfit != nullptr;
    if (a.scen)
        return forc ? run_family<T, false, true, true>(a, form, k_steps, st) : run_family<T, false, true, false>(a, form, k_steps, st);
    if (a.mforc != nullptr)
        return misfit ? run_family<T, true, false, true, true>(a, form, k_steps, st)
                      : run_family<T, false, false, true, true>(a, form, k_steps, st);
    if (forc)
        return misfit ? run_family<T, true, false, true>(a, form, k_steps, st) : run_family<T, false, false, true>(a, form, k_steps, st);
    return misfit ? run_family<T, true, false, false>(a, form, k_steps, st) : run_family<T, false, false, false>(a, form, k_steps, st);
}

// every fiveeq_run_* of the forward model (k_min: 1 for fiveeq_run_ksteps, whose k_steps has no "whole range" value 0)
template <typename T>
int run_forward(const BaseArgs<T>& b, const Features<T>& f, int32_t form, int32_t k_steps, int32_t k_min, void* stream) {
    RunArgs<T> a;
    if (int rc = prepare(a, b, f)) return rc;
    if (int rc = check_form(form, k_steps, k_min)) return rc;
    return run_form(a, form, k_steps, (hipStream_t)stream);
}

// the streamed histograms: the per-step or the fused kernel <.., BINS = true> writing every member's bin into the ring
template <typename T, bool FUSED>
int run_bins(const BaseArgs<T>& b, double lo, double hi, int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    RunArgs<T> a;
    if (int rc = make_args(a, b)) return rc;
    if (int rc = check_ring(a, lo, hi, n_bins, bin_ring, ring_rows)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (FUSED) return each_span(a, 0, [&](int t0, int t1) { return launch_fused<T, false, true>(a, t0, t1, st); });
    return each_step(a, [&](int t) { return launch_step<T, true>(a, t, st); });
}

template <typename T>
int run_inverse(const BaseArgs<T>& b, T* cumE, void* stream) {        // (C_traj: the diagnosed emissions E_traj)
    RunArgs<T> a;
    if (int rc = make_args(a, b)) return rc;
    if (!cumE) return fail(FIVEEQ_E_INVALID, "cumE is NULL");
    a.cumE = cumE;
    hipStream_t st = (hipStream_t)stream;
    return each_span(a, 0, [&](int t0, int t1) { return launch_fused<T, true>(a, t0, t1, st); });
}

// the inverse kernel in the carrier prepare() found (plain, MISFIT, FORC, FORC + MISFIT): one launch for the span
template <typename T>
int run_inverse_span(const RunArgs<T>& a, hipStream_t st) {
    const bool forc = a.fc.fscale != nullptr, misfit = a.mf.misfit != nullptr;
    return each_span(a, 0, [&](int t0, int t1) {
        if (forc)
            return misfit ? launch_fused<T, true, false, false, true, false, true>(a, t0, t1, st)
                          : launch_fused<T, true, false, false, false, false, true>(a, t0, t1, st);
        return misfit ? launch_fused<T, true, false, false, true>(a, t0, t1, st) : launch_fused<T, true>(a, t0, t1, st);
    });
}

// the concentration-driven form with the forcing scales and / or the misfit: fscale NULL = no scales (then n_fext must be 0: a
// count without rows is check_forcing's "fscale is NULL"), obs and misfit both NULL = no misfit, all three NULL = the plain
// inverse kernel.  Validated by prepare() in the order of the forward families, cumE right behind the base arguments; one
// launch for the span.
template <typename T>
int run_inverse_forc(const BaseArgs<T>& b, T* cumE, const ForcRows<T>& fc, const MisfitRows& mf, void* stream) {
    RunArgs<T> a;
    Features<T> f;
    f.forc = fc.fscale != nullptr || fc.n_fext != 0;
    f.fc = fc;
    f.misfit = OPTIONAL;
    f.mf = mf;
    f.inv = true;
    f.cumE = cumE;
    if (int rc = prepare(a, b, f)) return rc;
    return run_inverse_span(a, (hipStream_t)stream);
}

// ---- the mixed drive: a per-gas mask of concentration-driven gases (fused_mixed_kernel) ---------------------------------------
// one span of the mixed kernel of a.conc_mask (a proper mask, and a layout with the form: prepare() has seen to both)
template <typename T, bool MISFIT, bool FORC>
int launch_mixed(const RunArgs<T>& a, int t_begin, int t_end, hipStream_t st) {
    unsigned blocks;
    if (int rc = grid_blocks(a.n, FIVEEQ_BLOCK, blocks)) return rc;
    const dim3 grid(blocks), block(FIVEEQ_BLOCK);
    switch (a.conc_mask) {
#define X(cm)                                                                                                                    \
    case cm:                                                                                                                     \
        hipLaunchKernelGGL((fused_mixed_kernel<T, 4, 1, 1, cm, MISFIT, FORC>), grid, block, FIVEEQ_FUSED_DYN_LDS, st, a.km, a.drive, \
                           a.n_steps, t_begin, t_end, a.n, a.ld, a.r, a.q, a.R, a.S, a.cumE, a.C_traj, a.T_traj, a.n_rows, a.stats, \
                           a.mf.obs, a.mf.misfit, a.fc.fscale, a.fc.fext, a.fc.n_fext);                                            \
        break;
        X(1) X(2) X(3) X(4) X(5) X(6)
#undef X
        default:
            return fail(FIVEEQ_E_UNSUPPORTED, "conc_mask=0x%x has no mixed-drive kernel", (unsigned)a.conc_mask);
    }
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// fiveeq_run_mixed: validated by prepare() like fiveeq_run_inverse_forc, the mask in front of cumE; then by the mask
//   0            the forward time-fused call on these arguments (fiveeq_run_fused, or fiveeq_run_forc / fiveeq_run_obs with
//                FIVEEQ_FORM_FUSED and k_steps = 0: run_form), one launch for the range, cumE untouched;
//   every gas    fiveeq_run_inverse_forc's launches;
//   proper       the mixed kernel in the carrier (plain, FORC, MISFIT, FORC + MISFIT) those two pick among.
template <typename T>
int run_mixed(const BaseArgs<T>& b, T* cumE, int32_t conc_mask, const ForcRows<T>& fc, const MisfitRows& mf, void* stream) {
    RunArgs<T> a;
    Features<T> f;
    f.forc = fc.fscale != nullptr || fc.n_fext != 0;
    f.fc = fc;
    f.misfit = OPTIONAL;
    f.mf = mf;
    f.mixed = true;
    f.conc_mask = conc_mask;
    f.inv = conc_mask != 0;
    f.cumE = cumE;
    if (int rc = prepare(a, b, f)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a.conc_mask == 0) return run_form(a, FIVEEQ_FORM_FUSED, 0, st);
    const bool forc = a.fc.fscale != nullptr, misfit = a.mf.misfit != nullptr;
    if (a.conc_mask == (1 << a.n_gas) - 1) return run_inverse_span(a, st);
    return each_span(a, 0, [&](int t0, int t1) {
        if (forc) return misfit ? launch_mixed<T, true, true>(a, t0, t1, st) : launch_mixed<T, false, true>(a, t0, t1, st);
        return misfit ? launch_mixed<T, true, false>(a, t0, t1, st) : launch_mixed<T, false, false>(a, t0, t1, st);
    });
}

// ---- the compensated fp32 form: the fused kernel <.., COMP = true> over spans of k_steps, with or without the bin ring ----
int run_fused_comp(const BaseArgs<float>& b, int32_t k_steps, double lo, double hi, int32_t n_bins, uint16_t* bin_ring,
                   int32_t ring_rows, void* stream) {
    RunArgs<float> a;
    if (int rc = make_args(a, b)) return rc;
    if (int rc = check_form(FIVEEQ_FORM_FUSED, k_steps, 1)) return rc;
    if (int rc = bin_ring ? check_ring(a, lo, hi, n_bins, bin_ring, ring_rows) : FIVEEQ_OK) return rc;     // optional here
    hipStream_t st = (hipStream_t)stream;
    return each_span(a, k_steps, [&](int t0, int t1) {
        return bin_ring ? launch_fused<float, false, true, true>(a, t0, t1, st) : launch_fused<float, false, false, true>(a, t0, t1, st);
    });
}

// ---- small ensembles: one member per quad of lanes (small_kernel), several gases one per lane (small_multi_kernel) -----
// lanes per member of the widest small-ensemble form compiled for a layout: 4 for a lone 4-pool gas (a quad), 8 for 4 + 1 + 1
// (an octet: small_octet_kernel), 1 for every other compiled layout, 0 = none
int small_lanes(int code) { return code == 400 ? 4 : (code == 411 ? 8 : (layout_ok(code) ? 1 : 0)); }

// COMP: the compensated fp32 form, small_multi_kernel<.., COMP = true> for every layout, one member per lane
template <typename T, bool COMP = false>
int run_small(const BaseArgs<T>& b, int32_t lanes, void* stream) {
    static_assert(!COMP || std::is_same<T, float>::value, "the compensated form is fp32");
    RunArgs<T> a;
    if (int rc = make_args(a, b)) return rc;
    const int32_t t_begin = a.t_begin, t_end = a.t_end;
    const int widest = small_lanes(a.code);
    if (lanes == 0) lanes = (widest == 8 && a.stats != nullptr) ? 1 : widest;      // the octet form writes no statistics records
    if (lanes != 1 && lanes != widest)
        return fail(FIVEEQ_E_INVALID, "lanes_per_member=%d: pool layout %03d takes 1%s", lanes, a.code,
                    widest == 4 ? " or 4" : (widest == 8 ? " or 8" : ""));
    if (lanes == 8 && a.stats != nullptr)
        return fail(FIVEEQ_E_INVALID, "lanes_per_member=8 writes no per-wave statistics (T_stats must be NULL): use 1");
    if (t_begin == t_end) return FIVEEQ_OK;
    unsigned blocks;
    if (int rc = grid_blocks(a.n, FIVEEQ_SMALL_BLOCK / lanes, blocks)) return rc;
    const dim3 grid(blocks), block(FIVEEQ_SMALL_BLOCK);
    hipStream_t st = (hipStream_t)stream;
#define FIVEEQ_SMALL_ARGS st, a.km, a.drive, a.n_steps, t_begin, t_end, a.n, a.ld, a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows, a.stats
    const bool st_on = a.stats != nullptr;
    if constexpr (COMP) {
        switch (a.code) {
#define X(p0, p1, p2)                                                                                                   \
    case (p0) * 100 + (p1) * 10 + (p2):                                                                                 \
        if (st_on) hipLaunchKernelGGL((small_multi_kernel<float, p0, p1, p2, true, true>), grid, block, 0, FIVEEQ_SMALL_ARGS); \
        else hipLaunchKernelGGL((small_multi_kernel<float, p0, p1, p2, false, true>), grid, block, 0, FIVEEQ_SMALL_ARGS);      \
        break;
            FIVEEQ_LAYOUTS(X)
#undef X
            default: return no_kernel(a.code);
        }
    } else {
#define FIVEEQ_SMALL1(p0, lpm)                                                                                     \
    if (st_on) hipLaunchKernelGGL((small_kernel<T, p0, lpm, true>), grid, block, 0, FIVEEQ_SMALL_ARGS);            \
    else hipLaunchKernelGGL((small_kernel<T, p0, lpm, false>), grid, block, 0, FIVEEQ_SMALL_ARGS);                 \
    break;
        switch (a.code * 10 + lanes) {
            case 1001: FIVEEQ_SMALL1(1, 1)
            case 2001: FIVEEQ_SMALL1(2, 1)
            case 3001: FIVEEQ_SMALL1(3, 1)
            case 4001: FIVEEQ_SMALL1(4, 1)
            case 4004: FIVEEQ_SMALL1(4, 4)
            case 4118:
                hipLaunchKernelGGL((small_octet_kernel<T>), grid, block, 0, st, a.km, a.drive, a.n_steps, t_begin, t_end, a.n, a.ld,
                                   a.r, a.q, a.R, a.S, a.C_traj, a.T_traj, a.n_rows);
                break;
#define X(p0, p1, p2)                                                                                              \
    case ((p0) * 100 + (p1) * 10 + (p2)) * 10 + 1:                                                                 \
        if constexpr ((p1) > 0) {                                                                                  \
            if (st_on) hipLaunchKernelGGL((small_multi_kernel<T, p0, p1, p2, true>), grid, block, 0, FIVEEQ_SMALL_ARGS);  \
            else hipLaunchKernelGGL((small_multi_kernel<T, p0, p1, p2, false>), grid, block, 0, FIVEEQ_SMALL_ARGS);       \
        }                                                                                                          \
        break;
            X(1, 1, 0) X(4, 1, 0) X(4, 4, 0) X(1, 1, 1) X(4, 1, 1) X(4, 4, 1) X(4, 4, 4)
#undef X
            default: return no_kernel(a.code);
        }
#undef FIVEEQ_SMALL1
    }
#undef FIVEEQ_SMALL_ARGS
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// ---- the scan for single-valued parameter rows (uniform_rows_kernel): one device pass, synchronous ------------------------
template <typename T>
int uniform_rows(int64_t n, int64_t ld, int32_t n_r, const T* r, const T* q, uint32_t* mask_out, T* values_out, void* stream) {
    using U = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
    constexpr int MAX_ROWS = 3 * MAX_GAS + 2;
    if (n < 1) return fail(FIVEEQ_E_INVALID, "n_members=%lld must be >= 1", (long long)n);
    if (ld < n) return fail(FIVEEQ_E_INVALID, "ld=%lld < n_members=%lld", (long long)ld, (long long)n);
    if (n_r < 3 || n_r > 3 * MAX_GAS || n_r % 3) return fail(FIVEEQ_E_INVALID, "n_r_rows=%d: 3 rows per gas, 1..%d gases", n_r, MAX_GAS);
    if (!r || !q) return fail(FIVEEQ_E_INVALID, "NULL device pointer (r=%p q=%p)", (const void*)r, (const void*)q);
    if ((((uintptr_t)r) | ((uintptr_t)q)) & (sizeof(T) - 1)) return fail(FIVEEQ_E_INVALID, "r and q must be %d-byte aligned", (int)sizeof(T));
    if (!mask_out || !values_out)
        return fail(FIVEEQ_E_INVALID, "NULL output pointer (mask_out=%p values_out=%p)", (void*)mask_out, (void*)values_out);
    const int rows = n_r + 2;
    struct Out {
        U first[MAX_ROWS];
        unsigned int differs;
    } host;
    Out* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, sizeof(Out)));
    hipStream_t st = (hipStream_t)stream;
    int64_t bx = (n + (int64_t)FIVEEQ_BLOCK * 8 - 1) / ((int64_t)FIVEEQ_BLOCK * 8);        // >= 8 members per lane, at most 1024
    if (bx > 1024) bx = 1024;                                                              // workgroups per row
    hipError_t e = hipMemsetAsync(dev, 0, sizeof(Out), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((uniform_rows_kernel<U>), dim3((unsigned)bx, (unsigned)rows), dim3(FIVEEQ_BLOCK), 0, st, n, ld, (int)n_r,
                           (const U*)r, (const U*)q, &dev->differs, dev->first);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&host, dev, sizeof(Out), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(FIVEEQ_E_HIP, "the scan for single-valued rows failed: %s (%d)", hipGetErrorString(e), (int)e);
    *mask_out = ~host.differs & ((1u << rows) - 1u);
    std::memcpy(values_out, host.first, (size_t)rows * sizeof(T));
    return FIVEEQ_OK;
}

// ---- plans: a per-step run captured into a hipGraph -----------------------------------------------------------------------
struct Plan {
    uint32_t magic;
    hipGraph_t graph;
    hipGraphExec_t exec;
};
constexpr uint32_t PLAN_MAGIC = 0x35455146u;  // "FQE5"

// the plan of run_form(FIVEEQ_FORM_PER_STEP) for the family the call is of: that very run, enqueued on a capture stream
template <typename T>
int plan_create(const BaseArgs<T>& b, const Features<T>& f, void** plan_out) {
    RunArgs<T> a;
    if (int rc = prepare(a, b, f, true, plan_out)) return rc;
    if (a.t_begin == a.t_end) return fail(FIVEEQ_E_INVALID, "empty step range for a plan");
    hipStream_t cap = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(cap);
        return fail(FIVEEQ_E_HIP, "hipStreamBeginCapture failed: %s", hipGetErrorString(e));
    }
    const int rc = run_form(a, FIVEEQ_FORM_PER_STEP, 0, cap);
    e = hipStreamEndCapture(cap, &graph);
    (void)hipStreamDestroy(cap);
    if (rc != FIVEEQ_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    if (e != hipSuccess) return fail(FIVEEQ_E_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGraphDestroy(graph);
        return fail(FIVEEQ_E_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    Plan* p = new (std::nothrow) Plan{PLAN_MAGIC, graph, exec};
    if (!p) {
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        return fail(FIVEEQ_E_INVALID, "out of host memory");
    }
    *plan_out = p;
    return FIVEEQ_OK;
}

// what fiveeq_run_mforc / fiveeq_plan_create_mforc carry: fiveeq_run_forc's features (the scales, the optional misfit) and the
// member-forcing rows
template <typename T>
Features<T> mforc_features(const ForcRows<T>& fc, const MisfitRows& mf, const T* mforc, int32_t n_mforc_rows) {
    Features<T> f;
    f.forc = true;
    f.fc = fc;
    f.misfit = OPTIONAL;
    f.mf = mf;
    f.mforc = true;
    f.mforc_rows = mforc;
    f.n_mforc_rows = n_mforc_rows;
    return f;
}

// ---- per-member AR(1) noise rows (noise_rows_kernel): every check, then one launch ---------------------------------------
// [t_begin, t_end) = [-1, 0) is the start call (fiveeq_noise.hpp): it stores no row, so rows may be NULL there.
template <typename T>
int noise_rows(uint64_t seed, int64_t m0, int64_t n, int64_t ld, int32_t t_begin, int32_t t_end, const T* phi, const T* s,
               double* xi_state, T* rows, void* stream) {
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (m0 < 0) return fail(FIVEEQ_E_INVALID, "m0=%lld must be >= 0", (long long)m0);
    const bool start = t_begin == -1;
    if (t_begin < -1 || t_end < t_begin || (start && t_end != 0))
        return fail(FIVEEQ_E_INVALID, "step range [%d,%d): want 0 <= t_begin <= t_end, or [-1,0) for the stationary start", t_begin,
                    t_end);
    if (int rc = check_not_null({{"phi", phi}, {"s", s}, {"xi_state", xi_state}, {"rows", rows, 1, !start}})) return rc;
    if (int rc = check_aligned({{"phi", phi, sizeof(T)}, {"s", s, sizeof(T)}, {"xi_state", xi_state, 8}, {"rows", rows, sizeof(T)}}))
        return rc;
    if (t_begin == t_end) return FIVEEQ_OK;
    unsigned blocks;
    if (int rc = grid_blocks(n, FIVEEQ_BLOCK, blocks)) return rc;
    hipLaunchKernelGGL((noise_rows_kernel<T>), dim3(blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, seed, m0, n, ld, (int)t_begin,
                       (int)t_end, phi, s, xi_state, rows);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// ---- per-member minor-gas forcing rows (minor_rows_kernel): every check, then one launch ----------------------------------
template <typename T>
int minor_rows(int32_t n_species, int64_t n, int64_t ld, int32_t n_rows, double dt, const double* c, const double* emis, const T* tau,
               const T* eff, double* R, T* rows, int32_t accumulate, void* stream) {
    if (n_species < 1 || n_species > FIVEEQ_MINOR_MAX)
        return fail(FIVEEQ_E_INVALID, "n_species=%d outside 1..%d", n_species, FIVEEQ_MINOR_MAX);
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(FIVEEQ_E_INVALID, "dt=%g must be finite and > 0", dt);
    if (int rc = check_not_null({{"c", c}})) return rc;
    MinorC cc = {};
    for (int k = 0; k < n_species; ++k) {
        if (!std::isfinite(c[k])) return fail(FIVEEQ_E_INVALID, "c[%d]=%g is not finite", k, c[k]);
        cc.c[k] = c[k];
    }
    if (accumulate != 0 && accumulate != 1) return fail(FIVEEQ_E_INVALID, "accumulate=%d must be 0 or 1", accumulate);
    if (int rc = check_not_null({{"emis", emis}, {"tau", tau}, {"eff", eff}, {"R", R}, {"rows", rows}})) return rc;
    if (int rc = check_aligned({{"emis", emis, 8}, {"tau", tau, sizeof(T)}, {"eff", eff, sizeof(T)}, {"R", R, 8}, {"rows", rows, sizeof(T)}}))
        return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    unsigned blocks;
    if (int rc = grid_blocks(n, FIVEEQ_BLOCK, blocks)) return rc;
    hipLaunchKernelGGL((minor_rows_kernel<T>), dim3(blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, (int)n_species, n, ld,
                       (int)n_rows, dt, cc, emis, tau, eff, R, rows, (int)accumulate);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// ---- per-member aerosol forcing rows (aerosol_rows_kernel): every check, then one launch ----------------------------------
// shape and beta belong to the cloud term: required iff aci_mask != 0, never read without it.
template <typename T>
int aerosol_rows(int32_t n_species, int32_t aci_mask, int64_t n, int64_t ld, int32_t n_rows, const double* base, const double* emis,
                 const T* ari, const T* shape, const T* beta, T* rows, int32_t accumulate, void* stream) {
    if (n_species < 1 || n_species > FIVEEQ_AEROSOL_MAX)
        return fail(FIVEEQ_E_INVALID, "n_species=%d outside 1..%d", n_species, FIVEEQ_AEROSOL_MAX);
    if (aci_mask < 0 || (aci_mask >> n_species) != 0)
        return fail(FIVEEQ_E_INVALID, "aci_mask=0x%x has a bit outside the %d species", (unsigned)aci_mask, n_species);
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_not_null({{"base", base}})) return rc;
    AerosolBase bb = {};
    for (int k = 0; k < n_species; ++k) {
        if (!std::isfinite(base[k]) || base[k] < 0.0) return fail(FIVEEQ_E_INVALID, "base[%d]=%g must be finite and >= 0", k, base[k]);
        bb.b[k] = base[k];
    }
    if (accumulate != 0 && accumulate != 1) return fail(FIVEEQ_E_INVALID, "accumulate=%d must be 0 or 1", accumulate);
    const bool cloud = aci_mask != 0;
    if (int rc = check_not_null({{"emis", emis}, {"ari", ari}, {"shape", shape, 1, cloud}, {"beta", beta, 1, cloud}, {"rows", rows}}))
        return rc;
    if (int rc = check_aligned({{"emis", emis, 8}, {"ari", ari, sizeof(T)}, {"shape", shape, sizeof(T)}, {"beta", beta, sizeof(T)},
                                {"rows", rows, sizeof(T)}}))
        return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    unsigned blocks;
    if (int rc = grid_blocks(n, FIVEEQ_BLOCK, blocks)) return rc;
    hipLaunchKernelGGL((aerosol_rows_kernel<T>), dim3(blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, (int)n_species, (int)aci_mask,
                       n, ld, (int)n_rows, bb, emis, ari, shape, beta, rows, (int)accumulate);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

// ---- per-member sea-level rows (sea_level_rows_kernel): every check, then one launch over (members, scenarios) ------------
// heat and eta belong to the thermosteric term: eta is required iff heat is given, never read without it.
template <typename T>
int sea_level_rows(int32_t n_scen, int32_t n_comp, int32_t rate_mask, int64_t n, int64_t ld, int32_t n_rows, double dt, const T* T_rows,
                   int64_t t_row, int64_t t_scen, const double* par, const double* heat, int64_t h_row, int64_t h_scen,
                   const double* eta, double* S_io, double* total, double* comps, int64_t ld_out, void* stream) {
    if (int rc = check_scen(n_scen)) return rc;
    if (n_comp < 1 || n_comp > FIVEEQ_SEA_MAX) return fail(FIVEEQ_E_INVALID, "n_comp=%d outside 1..%d", n_comp, FIVEEQ_SEA_MAX);
    if (rate_mask < 0 || (rate_mask >> n_comp) != 0)
        return fail(FIVEEQ_E_INVALID, "rate_mask=0x%x has a bit outside the %d components", (unsigned)rate_mask, n_comp);
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(FIVEEQ_E_INVALID, "dt=%g must be finite and > 0", dt);
    const auto spans = [&](const char* name, int64_t stride) {       // a stride, or the outputs' row length, spans a row of ld
        return stride < ld ? fail(FIVEEQ_E_INVALID, "%s=%lld < ld=%lld", name, (long long)stride, (long long)ld) : FIVEEQ_OK;
    };
    if (int rc = spans("t_row_stride", t_row)) return rc;
    if (int rc = spans("t_scen_stride", t_scen)) return rc;
    if (heat) {
        if (int rc = spans("h_row_stride", h_row)) return rc;
        if (int rc = spans("h_scen_stride", h_scen)) return rc;
        if (!eta) return fail(FIVEEQ_E_INVALID, "heat without eta: eta is NULL");
    }
    if (int rc = check_ld("ld_out", ld_out, n)) return rc;
    if (int rc = check_not_null({{"T_rows", T_rows}, {"par", par}, {"S_io", S_io}, {"total", total}})) return rc;
    if (int rc = check_aligned({{"T_rows", T_rows, sizeof(T)}, {"par", par, 8}, {"heat", heat, 8}, {"eta", eta, 8}, {"S_io", S_io, 8},
                                {"total", total, 8}, {"comps", comps, 8}}))
        return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    unsigned blocks;
    if (int rc = grid_blocks(n, FIVEEQ_BLOCK, blocks)) return rc;
    hipLaunchKernelGGL((sea_level_rows_kernel<T>), dim3(blocks, (unsigned)n_scen), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, (int)n_comp,
                       (int)rate_mask, n, ld, (int)n_rows, dt, T_rows, t_row, t_scen, par, heat, h_row, h_scen, heat ? eta : nullptr, S_io,
                       total, comps, ld_out);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

}  // namespace

// =============================================================================================
extern "C" {

int fiveeq_abi_version(void) { return FIVEEQ_ABI_VERSION; }
#ifndef FIVEEQ_SOURCE_HASH
#define FIVEEQ_SOURCE_HASH "unstamped"      // built outside csrc/Makefile: the Python binding refuses such a library
#endif
const char* fiveeq_source_hash(void) { return FIVEEQ_SOURCE_HASH; }
#define FIVEEQ_STR2(x) #x
#define FIVEEQ_STR(x) FIVEEQ_STR2(x)
const char* fiveeq_build_flags(void) {
    return ""
#ifdef FIVEEQ_STEP_WAVES
           " FIVEEQ_STEP_WAVES=" FIVEEQ_STR(FIVEEQ_STEP_WAVES)
#endif
#if FIVEEQ_FUSED_DYN_LDS != 0
           " FIVEEQ_FUSED_DYN_LDS=" FIVEEQ_STR(FIVEEQ_FUSED_DYN_LDS)
#endif
#if FIVEEQ_BLOCK != 256
           " FIVEEQ_BLOCK=" FIVEEQ_STR(FIVEEQ_BLOCK)
#endif
#if FIVEEQ_SMALL_BLOCK != 256
           " FIVEEQ_SMALL_BLOCK=" FIVEEQ_STR(FIVEEQ_SMALL_BLOCK)
#endif
#if FIVEEQ_STEP_BLOCK != 64
           " FIVEEQ_STEP_BLOCK=" FIVEEQ_STR(FIVEEQ_STEP_BLOCK)
#endif
#if FIVEEQ_FUSED_CHUNK != 125
           " FIVEEQ_FUSED_CHUNK=" FIVEEQ_STR(FIVEEQ_FUSED_CHUNK)
#endif
        ;
}
const char* fiveeq_last_error(void) { return g_err; }
int64_t fiveeq_sizeof_model(void) { return (int64_t)sizeof(fiveeq_model); }
int64_t fiveeq_stats_waves(int64_t n_members) { return n_members < 1 ? 0 : (n_members + 63) / 64; }

int fiveeq_layout_supported(int32_t n_gas, const int32_t* n_pools) {
    if (!n_pools || n_gas < 1 || n_gas > FIVEEQ_MAX_GAS) return 0;
    for (int g = 0; g < n_gas; ++g)
        if (n_pools[g] < 1 || n_pools[g] > FIVEEQ_MAX_POOLS) return 0;
    return layout_ok(layout_code(n_gas, n_pools)) ? 1 : 0;
}

int fiveeq_step_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                    int32_t t, const double* r, const double* q, double* R, double* S, double* C_traj, double* T_traj,
                    int32_t n_rows, double* T_stats, void* stream) {
    if (t < 0 || t >= n_steps) return fail(FIVEEQ_E_INVALID, "t=%d outside [0,%d)", t, n_steps);
    return run_forward<double>({model, n_members, ld, drive, n_steps, t, t + 1, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_run_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                   int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                   double* T_traj, int32_t n_rows, double* T_stats, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_run_fused_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                         int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                         double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {}, FIVEEQ_FORM_FUSED, 0, 0, stream);
}
int fiveeq_plan_create_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                           int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                           double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {}, plan_out);
}
int fiveeq_step_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                    int32_t t, const float* r, const float* q, float* R, float* S, float* C_traj, float* T_traj,
                    int32_t n_rows, double* T_stats, void* stream) {
    if (t < 0 || t >= n_steps) return fail(FIVEEQ_E_INVALID, "t=%d outside [0,%d)", t, n_steps);
    return run_forward<float>({model, n_members, ld, drive, n_steps, t, t + 1, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_run_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                   int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                   float* T_traj, int32_t n_rows, double* T_stats, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_run_fused_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                         int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                         float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {}, FIVEEQ_FORM_FUSED, 0, 0, stream);
}
int fiveeq_run_fused_bins_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                              int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                              double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, double hist_lo,
                              double hist_hi, int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    return run_bins<double, true>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                                  hist_lo, hist_hi, n_bins, bin_ring, ring_rows, stream);
}
int fiveeq_run_fused_bins_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                              int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                              float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, double hist_lo,
                              double hist_hi, int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    return run_bins<float, true>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                                 hist_lo, hist_hi, n_bins, bin_ring, ring_rows, stream);
}
int fiveeq_run_bins_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                        int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S,
                        double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, double hist_lo, double hist_hi,
                        int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    return run_bins<double, false>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                                   hist_lo, hist_hi, n_bins, bin_ring, ring_rows, stream);
}
int fiveeq_run_bins_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                        int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S,
                        float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, double hist_lo, double hist_hi,
                        int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    return run_bins<float, false>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                                  hist_lo, hist_hi, n_bins, bin_ring, ring_rows, stream);
}
int fiveeq_plan_create_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                           int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                           float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {}, plan_out);
}

int fiveeq_uniform_rows_f64(int64_t n_members, int64_t ld, int32_t n_r_rows, const double* r, const double* q, uint32_t* mask_out,
                            double* values_out, void* stream) {
    return uniform_rows<double>(n_members, ld, n_r_rows, r, q, mask_out, values_out, stream);
}
int fiveeq_uniform_rows_f32(int64_t n_members, int64_t ld, int32_t n_r_rows, const float* r, const float* q, uint32_t* mask_out,
                            float* values_out, void* stream) {
    return uniform_rows<float>(n_members, ld, n_r_rows, r, q, mask_out, values_out, stream);
}
int fiveeq_run_uniform_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                           int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                           double* T_traj, int32_t n_rows, double* T_stats, uint32_t mask, const double* values, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, false, {}, ABSENT, {}, true, mask, values}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_run_uniform_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                           int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                           float* T_traj, int32_t n_rows, double* T_stats, uint32_t mask, const float* values, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, false, {}, ABSENT, {}, true, mask, values}, FIVEEQ_FORM_PER_STEP, 0, 0, stream);
}
int fiveeq_plan_create_uniform_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                                   int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S,
                                   double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, uint32_t mask,
                                   const double* values, void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, false, {}, ABSENT, {}, true, mask, values}, plan_out);
}
int fiveeq_plan_create_uniform_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                                   int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S,
                                   float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, uint32_t mask,
                                   const float* values, void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, false, {}, ABSENT, {}, true, mask, values}, plan_out);
}

int fiveeq_run_inverse_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                           int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q,
                           double* R, double* S, double* cumE, double* E_traj, double* T_traj, int32_t n_rows,
                           double* T_stats, void* stream) {
    return run_inverse<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, E_traj, T_traj, n_rows, T_stats},
                               cumE, stream);
}
int fiveeq_run_inverse_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                           int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                           float* S, float* cumE, float* E_traj, float* T_traj, int32_t n_rows, double* T_stats,
                           void* stream) {
    return run_inverse<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, E_traj, T_traj, n_rows, T_stats},
                              cumE, stream);
}
int fiveeq_run_inverse_forc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                                int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q,
                                double* R, double* S, double* cumE, double* E_traj, double* T_traj, int32_t n_rows,
                                double* T_stats, const double* fscale, const double* fext, int32_t n_fext,
                                const double* obs, double* misfit, void* stream) {
    return run_inverse_forc<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, E_traj, T_traj, n_rows, T_stats},
                                    cumE, {fscale, fext, n_fext}, {obs, misfit}, stream);
}
int fiveeq_run_inverse_forc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                                int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                                float* S, float* cumE, float* E_traj, float* T_traj, int32_t n_rows, double* T_stats,
                                const float* fscale, const float* fext, int32_t n_fext, const double* obs, double* misfit,
                                void* stream) {
    return run_inverse_forc<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, E_traj, T_traj, n_rows, T_stats},
                                   cumE, {fscale, fext, n_fext}, {obs, misfit}, stream);
}

int fiveeq_run_mixed_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                         int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* cumE,
                         double* X_traj, double* T_traj, int32_t n_rows, double* T_stats, int32_t conc_mask, const double* fscale,
                         const double* fext, int32_t n_fext, const double* obs, double* misfit, void* stream) {
    return run_mixed<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, X_traj, T_traj, n_rows, T_stats},
                             cumE, conc_mask, {fscale, fext, n_fext}, {obs, misfit}, stream);
}
int fiveeq_run_mixed_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                         int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* cumE,
                         float* X_traj, float* T_traj, int32_t n_rows, double* T_stats, int32_t conc_mask, const float* fscale,
                         const float* fext, int32_t n_fext, const double* obs, double* misfit, void* stream) {
    return run_mixed<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, X_traj, T_traj, n_rows, T_stats},
                            cumE, conc_mask, {fscale, fext, n_fext}, {obs, misfit}, stream);
}
int fiveeq_mixed_layout_supported(int32_t n_gas, const int32_t* n_pools, int32_t conc_mask) {
    if (!fiveeq_layout_supported(n_gas, n_pools) || conc_mask < 0 || conc_mask >> n_gas) return 0;
    if (conc_mask == 0 || conc_mask == (1 << n_gas) - 1) return 1;              // the forward and the inverse kernels: every layout
    return mixed_layout(layout_code(n_gas, n_pools)) ? 1 : 0;
}

int fiveeq_run_ksteps_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                          int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                          double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, int32_t k_steps,
                          void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {}, FIVEEQ_FORM_FUSED, k_steps, 1, stream);
}
int fiveeq_run_ksteps_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                          int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                          float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, int32_t k_steps,
                          void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {}, FIVEEQ_FORM_FUSED, k_steps, 1, stream);
}
int fiveeq_run_fused_comp_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                              int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                              float* T_traj, int32_t n_rows, double* T_stats, int32_t k_steps, double lo, double hi,
                              int32_t n_bins, uint16_t* bin_ring, int32_t ring_rows, void* stream) {
    return run_fused_comp({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                          k_steps, lo, hi, n_bins, bin_ring, ring_rows, stream);
}
int fiveeq_run_small_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive,
                         int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                         double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, int32_t lanes_per_member,
                         void* stream) {
    return run_small<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                             lanes_per_member, stream);
}
int fiveeq_run_small_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive,
                         int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                         float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, int32_t lanes_per_member,
                         void* stream) {
    return run_small<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                            lanes_per_member, stream);
}
int fiveeq_run_small_comp_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                              int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                              float* T_traj, int32_t n_rows, double* T_stats, void* stream) {
    return run_small<float, true>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                                  1, stream);
}
int fiveeq_run_obs_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                       int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                       double* T_traj, int32_t n_rows, double* T_stats, const double* obs, double* misfit, int32_t form,
                       int32_t k_steps, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, false, {}, REQUIRED, {obs, misfit}}, form, k_steps, 0, stream);
}
int fiveeq_run_obs_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                       int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                       float* T_traj, int32_t n_rows, double* T_stats, const double* obs, double* misfit, int32_t form,
                       int32_t k_steps, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, false, {}, REQUIRED, {obs, misfit}}, form, k_steps, 0, stream);
}
int fiveeq_plan_create_obs_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                               int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S,
                               double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, const double* obs, double* misfit,
                               void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, false, {}, REQUIRED, {obs, misfit}}, plan_out);
}
int fiveeq_plan_create_obs_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                               int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S,
                               float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, const double* obs, double* misfit,
                               void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, false, {}, REQUIRED, {obs, misfit}}, plan_out);
}
int fiveeq_misfit_layout_supported(int32_t n_gas, const int32_t* n_pools) {
    return fiveeq_layout_supported(n_gas, n_pools) && misfit_layout(layout_code(n_gas, n_pools)) ? 1 : 0;
}

int fiveeq_run_scen_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const double* drive,
                        int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S,
                        double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, int32_t form, int32_t k_steps,
                        void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {true, n_scen}, form, k_steps, 0, stream);
}
int fiveeq_run_scen_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const float* drive,
                        int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S,
                        float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, int32_t form, int32_t k_steps,
                        void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {true, n_scen}, form, k_steps, 0, stream);
}
int fiveeq_plan_create_scen_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const double* drive,
                                int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                                double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {true, n_scen}, plan_out);
}
int fiveeq_plan_create_scen_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const float* drive,
                                int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                                float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {true, n_scen}, plan_out);
}
int32_t fiveeq_max_scenarios(void) { return MAX_SCENARIOS; }
int fiveeq_run_scen_forc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const double* drive,
                             int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                             double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats, const double* fscale,
                             const double* fext, int32_t n_fext, int32_t form, int32_t k_steps, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {true, n_scen, true, {fscale, fext, n_fext}}, form, k_steps, 0, stream);
}
int fiveeq_run_scen_forc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const float* drive,
                             int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S,
                             float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, const float* fscale, const float* fext,
                             int32_t n_fext, int32_t form, int32_t k_steps, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {true, n_scen, true, {fscale, fext, n_fext}}, form, k_steps, 0, stream);
}
int fiveeq_plan_create_scen_forc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const double* drive,
                                     int32_t n_steps, int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R,
                                     double* S, double* C_traj, double* T_traj, int32_t n_rows, double* T_stats,
                                     const double* fscale, const double* fext, int32_t n_fext, void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {true, n_scen, true, {fscale, fext, n_fext}}, plan_out);
}
int fiveeq_plan_create_scen_forc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, int32_t n_scen, const float* drive,
                                     int32_t n_steps, int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R,
                                     float* S, float* C_traj, float* T_traj, int32_t n_rows, double* T_stats, const float* fscale,
                                     const float* fext, int32_t n_fext, void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {true, n_scen, true, {fscale, fext, n_fext}}, plan_out);
}

int fiveeq_run_forc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                        int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                        double* T_traj, int32_t n_rows, double* T_stats, const double* fscale, const double* fext, int32_t n_fext,
                        const double* obs, double* misfit, int32_t form, int32_t k_steps, void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, true, {fscale, fext, n_fext}, OPTIONAL, {obs, misfit}}, form, k_steps, 0, stream);
}
int fiveeq_plan_create_forc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                                int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                                double* T_traj, int32_t n_rows, double* T_stats, const double* fscale, const double* fext,
                                int32_t n_fext, const double* obs, double* misfit, void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                               {false, 1, true, {fscale, fext, n_fext}, OPTIONAL, {obs, misfit}}, plan_out);
}
int fiveeq_run_forc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                        int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                        float* T_traj, int32_t n_rows, double* T_stats, const float* fscale, const float* fext, int32_t n_fext,
                        const double* obs, double* misfit, int32_t form, int32_t k_steps, void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, true, {fscale, fext, n_fext}, OPTIONAL, {obs, misfit}}, form, k_steps, 0, stream);
}
int fiveeq_plan_create_forc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                                int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                                float* T_traj, int32_t n_rows, double* T_stats, const float* fscale, const float* fext,
                                int32_t n_fext, const double* obs, double* misfit, void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                              {false, 1, true, {fscale, fext, n_fext}, OPTIONAL, {obs, misfit}}, plan_out);
}
int fiveeq_run_mforc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                         int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                         double* T_traj, int32_t n_rows, double* T_stats, const double* fscale, const double* fext, int32_t n_fext,
                         const double* obs, double* misfit, const double* mforc, int32_t n_mforc_rows, int32_t form, int32_t k_steps,
                         void* stream) {
    return run_forward<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                            mforc_features<double>({fscale, fext, n_fext}, {obs, misfit}, mforc, n_mforc_rows), form, k_steps, 0, stream);
}
int fiveeq_plan_create_mforc_f64(const fiveeq_model* model, int64_t n_members, int64_t ld, const double* drive, int32_t n_steps,
                                 int32_t t_begin, int32_t t_end, const double* r, const double* q, double* R, double* S, double* C_traj,
                                 double* T_traj, int32_t n_rows, double* T_stats, const double* fscale, const double* fext,
                                 int32_t n_fext, const double* obs, double* misfit, const double* mforc, int32_t n_mforc_rows,
                                 void** plan_out) {
    return plan_create<double>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                            mforc_features<double>({fscale, fext, n_fext}, {obs, misfit}, mforc, n_mforc_rows), plan_out);
}
int fiveeq_noise_rows_f64(uint64_t seed, int64_t m0, int64_t n_members, int64_t ld, int32_t t_begin, int32_t t_end, const double* phi,
                          const double* s, double* xi_state, double* rows, void* stream) {
    return noise_rows<double>(seed, m0, n_members, ld, t_begin, t_end, phi, s, xi_state, rows, stream);
}
int fiveeq_run_mforc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                         int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                         float* T_traj, int32_t n_rows, double* T_stats, const float* fscale, const float* fext, int32_t n_fext,
                         const double* obs, double* misfit, const float* mforc, int32_t n_mforc_rows, int32_t form, int32_t k_steps,
                         void* stream) {
    return run_forward<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                            mforc_features<float>({fscale, fext, n_fext}, {obs, misfit}, mforc, n_mforc_rows), form, k_steps, 0, stream);
}
int fiveeq_plan_create_mforc_f32(const fiveeq_model* model, int64_t n_members, int64_t ld, const float* drive, int32_t n_steps,
                                 int32_t t_begin, int32_t t_end, const float* r, const float* q, float* R, float* S, float* C_traj,
                                 float* T_traj, int32_t n_rows, double* T_stats, const float* fscale, const float* fext,
                                 int32_t n_fext, const double* obs, double* misfit, const float* mforc, int32_t n_mforc_rows,
                                 void** plan_out) {
    return plan_create<float>({model, n_members, ld, drive, n_steps, t_begin, t_end, r, q, R, S, C_traj, T_traj, n_rows, T_stats},
                            mforc_features<float>({fscale, fext, n_fext}, {obs, misfit}, mforc, n_mforc_rows), plan_out);
}
int fiveeq_noise_rows_f32(uint64_t seed, int64_t m0, int64_t n_members, int64_t ld, int32_t t_begin, int32_t t_end, const float* phi,
                          const float* s, double* xi_state, float* rows, void* stream) {
    return noise_rows<float>(seed, m0, n_members, ld, t_begin, t_end, phi, s, xi_state, rows, stream);
}
int fiveeq_minor_rows_f64(int32_t n_species, int64_t n_members, int64_t ld, int32_t n_rows, double dt, const double* c,
                          const double* emis, const double* tau, const double* eff, double* R, double* rows, int32_t accumulate,
                          void* stream) {
    return minor_rows<double>(n_species, n_members, ld, n_rows, dt, c, emis, tau, eff, R, rows, accumulate, stream);
}
int fiveeq_minor_rows_f32(int32_t n_species, int64_t n_members, int64_t ld, int32_t n_rows, double dt, const double* c,
                          const double* emis, const float* tau, const float* eff, double* R, float* rows, int32_t accumulate,
                          void* stream) {
    return minor_rows<float>(n_species, n_members, ld, n_rows, dt, c, emis, tau, eff, R, rows, accumulate, stream);
}
int fiveeq_aerosol_rows_f64(int32_t n_species, int32_t aci_mask, int64_t n_members, int64_t ld, int32_t n_rows, const double* base,
                            const double* emis, const double* ari, const double* shape, const double* beta, double* rows,
                            int32_t accumulate, void* stream) {
    return aerosol_rows<double>(n_species, aci_mask, n_members, ld, n_rows, base, emis, ari, shape, beta, rows, accumulate, stream);
}
int fiveeq_aerosol_rows_f32(int32_t n_species, int32_t aci_mask, int64_t n_members, int64_t ld, int32_t n_rows, const double* base,
                            const double* emis, const float* ari, const float* shape, const float* beta, float* rows,
                            int32_t accumulate, void* stream) {
    return aerosol_rows<float>(n_species, aci_mask, n_members, ld, n_rows, base, emis, ari, shape, beta, rows, accumulate, stream);
}
int fiveeq_sea_level_rows_f64(int32_t n_scen, int32_t n_comp, int32_t rate_mask, int64_t n_members, int64_t ld, int32_t n_rows, double dt,
                              const double* T_rows, int64_t t_row_stride, int64_t t_scen_stride, const double* par, const double* heat,
                              int64_t h_row_stride, int64_t h_scen_stride, const double* eta, double* S_io, double* total, double* comps,
                              int64_t ld_out, void* stream) {
    return sea_level_rows<double>(n_scen, n_comp, rate_mask, n_members, ld, n_rows, dt, T_rows, t_row_stride, t_scen_stride, par, heat,
                                  h_row_stride, h_scen_stride, eta, S_io, total, comps, ld_out, stream);
}
int fiveeq_sea_level_rows_f32(int32_t n_scen, int32_t n_comp, int32_t rate_mask, int64_t n_members, int64_t ld, int32_t n_rows, double dt,
                              const float* T_rows, int64_t t_row_stride, int64_t t_scen_stride, const double* par, const double* heat,
                              int64_t h_row_stride, int64_t h_scen_stride, const double* eta, double* S_io, double* total, double* comps,
                              int64_t ld_out, void* stream) {
    return sea_level_rows<float>(n_scen, n_comp, rate_mask, n_members, ld, n_rows, dt, T_rows, t_row_stride, t_scen_stride, par, heat,
                                 h_row_stride, h_scen_stride, eta, S_io, total, comps, ld_out, stream);
}
int fiveeq_forcing_layout_supported(int32_t n_gas, const int32_t* n_pools) {
    return fiveeq_layout_supported(n_gas, n_pools) && forcing_layout(layout_code(n_gas, n_pools)) ? 1 : 0;
}
int32_t fiveeq_max_fext(void) { return MAX_FEXT; }

int32_t fiveeq_small_lanes(int32_t n_gas, const int32_t* n_pools) {
    return fiveeq_layout_supported(n_gas, n_pools) ? small_lanes(layout_code(n_gas, n_pools)) : 0;
}
int fiveeq_set_f32_packing(int on) { return g_f32_packing.exchange(on ? 1 : 0, std::memory_order_relaxed); }

int fiveeq_set_row_policy(int32_t policy) {
    if (policy != FIVEEQ_ROWS_AUTO && policy != FIVEEQ_ROWS_CACHED && policy != FIVEEQ_ROWS_STREAMED)
        return fail(FIVEEQ_E_INVALID, "row policy %d: want FIVEEQ_ROWS_CACHED (0), _STREAMED (1) or _AUTO (2)", policy);
    return g_row_policy.exchange(policy, std::memory_order_relaxed);
}

int fiveeq_rows_streamed(int32_t n_gas, const int32_t* n_pools, int64_t n_members, int64_t ld, int32_t word_bytes) {
    if (n_gas < 1 || n_gas > FIVEEQ_MAX_GAS || !n_pools || n_members < 0 || ld < n_members || (word_bytes != 4 && word_bytes != 8))
        return fail(FIVEEQ_E_INVALID, "fiveeq_rows_streamed: bad shape");
    int sum_pools = 0;
    for (int g = 0; g < n_gas; ++g) sum_pools += n_pools[g];
    return rows_streamed(g_row_policy.load(std::memory_order_relaxed), n_gas, sum_pools, 1, n_members, ld, word_bytes) ? 1 : 0;
}

static int lhs_check(int64_t n_total, int64_t m0, int64_t n_members, int32_t dim0, int32_t n_dim, int64_t ld) {
    // 2^28: stratum (28 bits) + the 24-bit jitter placed mid-cell (25 fractional bits) is then an EXACT fp64 sum, so u lies
    // strictly inside its stratum; beyond that the sum would round and could touch the stratum edge
    if (n_total < 1 || n_total > FIVEEQ_LHS_MAX_TOTAL)
        return fail(FIVEEQ_E_INVALID, "n_total=%lld outside 1..2^28", (long long)n_total);
    if (m0 < 0 || n_members < 0 || m0 + n_members > n_total)
        return fail(FIVEEQ_E_INVALID, "members [%lld, %lld) outside [0, %lld)", (long long)m0, (long long)(m0 + n_members),
                    (long long)n_total);
    if (dim0 < 0 || n_dim < 0 || n_dim > 65535) return fail(FIVEEQ_E_INVALID, "dim0=%d n_dim=%d invalid", dim0, n_dim);
    if (ld < n_members) return fail(FIVEEQ_E_INVALID, "ld < n_members");
    return FIVEEQ_OK;
}
static int lhs_half_bits(int64_t n_total) {
    int bits = 2;                                            // even number of bits with 2^bits >= n_total
    while (bits < 62 && (1LL << bits) < n_total) bits += 2;
    return bits / 2;
}

int fiveeq_lhs_rows_host_f64(uint64_t seed, int64_t n_total, int64_t m0, int64_t n_members, int32_t dim0, int32_t n_dim,
                             int64_t ld, double* out) {
    if (int rc = lhs_check(n_total, m0, n_members, dim0, n_dim, ld)) return rc;
    if (n_members == 0 || n_dim == 0) return FIVEEQ_OK;
    if (!out) return fail(FIVEEQ_E_INVALID, "NULL pointer");
    const int half = lhs_half_bits(n_total);
    for (int k = 0; k < n_dim; ++k) {
        const uint64_t key = fiveeq::lhs_dim_key(seed, dim0 + k);
        for (int64_t i = 0; i < n_members; ++i) {
            const uint64_t m = (uint64_t)(m0 + i);
            const uint64_t stratum = fiveeq::lhs_permute(m, (uint64_t)n_total, half, key);
            const uint64_t jbits = fiveeq::lhs_mix64(m ^ (key * 0xff51afd7ed558ccdULL + 0xc4ceb9fe1a85ec53ULL)) >> 40;
            out[(int64_t)k * ld + i] = ((double)stratum + ((double)jbits + 0.5) * 0x1.0p-24) / (double)n_total;
        }
    }
    return FIVEEQ_OK;
}

int fiveeq_lhs_rows_f64(uint64_t seed, int64_t n_total, int64_t m0, int64_t n_members, int32_t dim0, int32_t n_dim,
                        int64_t ld, double* out, void* stream) {
    if (int rc = lhs_check(n_total, m0, n_members, dim0, n_dim, ld)) return rc;
    if (n_members == 0 || n_dim == 0) return FIVEEQ_OK;
    if (!out) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    const int64_t blocks = member_blocks(n_members);
    if (blocks > 0x7fffffffLL) return fail(FIVEEQ_E_INVALID, "n_members too large for one launch");
    hipLaunchKernelGGL(fiveeq::lhs_kernel, dim3((unsigned)blocks, (unsigned)n_dim), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream,
                       seed, n_total, lhs_half_bits(n_total), m0, n_members, dim0, ld, out);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

int fiveeq_plan_launch(void* plan, void* stream) {
    Plan* p = static_cast<Plan*>(plan);
    if (!p || p->magic != PLAN_MAGIC) return fail(FIVEEQ_E_INVALID, "not a live fiveeq plan");
    HIP_TRY(hipGraphLaunch(p->exec, (hipStream_t)stream));
    return FIVEEQ_OK;
}

int fiveeq_plan_destroy(void* plan) {
    Plan* p = static_cast<Plan*>(plan);
    if (!p || p->magic != PLAN_MAGIC) return fail(FIVEEQ_E_INVALID, "not a live fiveeq plan");
    p->magic = 0;
    hipError_t e1 = hipGraphExecDestroy(p->exec);
    hipError_t e2 = hipGraphDestroy(p->graph);
    delete p;
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(FIVEEQ_E_HIP, "graph destroy failed");
    return FIVEEQ_OK;
}

int fiveeq_hfc_conc_f64(int64_t n_members, int64_t ld, int32_t n_time, const double* e0, const double* time,
                        double* out, void* stream) {
    if (n_members < 1) return fail(FIVEEQ_E_INVALID, "n_members=%lld must be >= 1", (long long)n_members);
    if (ld < n_members) return fail(FIVEEQ_E_INVALID, "ld < n_members");
    if (n_time < 0) return fail(FIVEEQ_E_INVALID, "n_time=%d must be >= 0", n_time);
    if (n_time == 0) return FIVEEQ_OK;
    if (!e0 || !time || !out) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    const int64_t blocks = (n_members + FIVEEQ_BLOCK - 1) / FIVEEQ_BLOCK;
    if (blocks > 0x7fffffffLL) return fail(FIVEEQ_E_INVALID, "n_members too large");
    hipLaunchKernelGGL(fiveeq::hfc_conc_kernel, dim3((unsigned)blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream,
                       n_members, ld, n_time, e0, time, out);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

int fiveeq_stream_copy_wide_f64(int64_t n, const double* src, double* dst, void* stream) {
    if (n < 2 || (n & 1)) return fail(FIVEEQ_E_INVALID, "n=%lld must be even and >= 2", (long long)n);
    if (!src || !dst) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (((uintptr_t)src | (uintptr_t)dst) & 15) return fail(FIVEEQ_E_INVALID, "pointers must be 16-byte aligned");
    const int64_t n2 = n / 2;
    const int64_t tiles = (n2 + 4 * FIVEEQ_BLOCK - 1) / (4 * FIVEEQ_BLOCK);
    const int64_t blocks = tiles < 16384 ? tiles : 16384;
    hipLaunchKernelGGL(fiveeq::stream_copy_wide_kernel, dim3((unsigned)blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream,
                       n2, reinterpret_cast<const double2*>(src), reinterpret_cast<double2*>(dst));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

int fiveeq_busy(int64_t iterations, double* out, void* stream) {
    if (iterations < 0 || iterations > 100000000LL) return fail(FIVEEQ_E_INVALID, "iterations=%lld outside 0..1e8", (long long)iterations);
    if (!out) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(fiveeq::busy_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, iterations, out);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

int fiveeq_stream_copy_nt_f64(int64_t n, const double* src, double* dst, void* stream) {
    if (n < 1 || n % (4 * FIVEEQ_BLOCK)) return fail(FIVEEQ_E_INVALID, "n=%lld must be a positive multiple of %d", (long long)n, 4 * FIVEEQ_BLOCK);
    if (!src || !dst) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    const int64_t blocks = n / (4 * FIVEEQ_BLOCK);
    if (blocks > 0x7fffffffLL) return fail(FIVEEQ_E_INVALID, "n too large for one launch");
    hipLaunchKernelGGL(fiveeq::stream_copy_nt_kernel, dim3((unsigned)blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, n, src, dst);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

int fiveeq_stream_copy_f64(int64_t n, const double* src, double* dst, void* stream) {
    if (n < 1) return fail(FIVEEQ_E_INVALID, "n=%lld must be >= 1", (long long)n);
    if (!src || !dst) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(fiveeq::stream_copy_kernel, dim3((unsigned)(member_blocks(n) < 8192 ? member_blocks(n) : 8192)), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, src, dst);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

}  // extern "C"

namespace {
// members per workgroup of the histogram pass: as coarse as still gives ~2048 workgroups over all rows
// (fewer, fuller flushes of the LDS histogram), a multiple of the block size
int64_t hist_chunk(int32_t n_rows, int64_t n) {
    int64_t chunk = (n * (n_rows > 0 ? n_rows : 1) + 2047) / 2048;
    if (chunk < fiveeq::HIST_CHUNK_MIN) chunk = fiveeq::HIST_CHUNK_MIN;
    return (chunk + FIVEEQ_BLOCK - 1) / FIVEEQ_BLOCK * FIVEEQ_BLOCK;
}
// the chunk of a ranged histogram (the summaries': a few rows): every workgroup zeroes and flushes all n_bins counters, which
// at 2048 workgroups of 18k members each is a third of the pass (68 us for 3 x 12.5M fp32 values at 4096 bins, 40 at 1024 bins)
// — at least 8 members per bin and workgroup, in whole `unit`s: 47 us.  (The ring passes count 64+ rows per launch and are
// far beyond that already.)
int64_t ranged_chunk(int64_t chunk, int32_t n_bins, int64_t unit) {
    const int64_t floor_ = (8LL * n_bins + unit - 1) / unit * unit;
    return chunk < floor_ ? floor_ : chunk;
}
// the sizes of both counting passes
int hist_check(int32_t n_rows, int64_t n, int64_t ld, int32_t n_bins) {
    if (int rc = check_n_rows(n_rows)) return rc;
    if (n < 1 || ld < n) return fail(FIVEEQ_E_INVALID, "n_members=%lld, ld=%lld invalid", (long long)n, (long long)ld);
    return check_n_bins(n_bins);
}

template <typename T>
int hist_rows(int32_t n_rows, int64_t n, int64_t ld, const T* rows, double lo, double hi, int32_t n_bins,
              uint64_t* hist, void* stream, const double* ranges = nullptr) {
    if (int rc = hist_check(n_rows, n, ld, n_bins)) return rc;
    if (!ranges && (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi))) return fail(FIVEEQ_E_INVALID, "need finite lo < hi");
    if (n_rows == 0) return FIVEEQ_OK;
    if (!rows || !hist) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (n_rows > 65535) return fail(FIVEEQ_E_INVALID, "n_rows=%d exceeds the 65535 rows of one launch", n_rows);
    const int64_t chunk = ranges ? ranged_chunk(hist_chunk(n_rows, n), n_bins, FIVEEQ_BLOCK) : hist_chunk(n_rows, n);
    int64_t chunks;
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    const double inv_w = ranges ? 0.0 : (double)n_bins / (hi - lo);
    hipLaunchKernelGGL(fiveeq::hist_rows_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, lo, inv_w, n_bins, reinterpret_cast<unsigned long long*>(hist),
                       ranges);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}

template <typename T>
int math_probe(int32_t op, int64_t n, const T* x, T* y, void* stream) {
    const bool packed_op = sizeof(T) == 4 && op >= 8 && op <= 12;          // fp32: the packed twin on element pairs
    if ((op < 0 || op > 4) && !packed_op) return fail(FIVEEQ_E_INVALID, "op=%d outside 0..4 (fp32: also 8..12)", op);
    if (n < 1) return fail(FIVEEQ_E_INVALID, "n=%lld must be >= 1", (long long)n);
    if (packed_op && (n & 1)) return fail(FIVEEQ_E_INVALID, "packed ops need an even n");
    if (!x || !y) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    const int64_t blocks = member_blocks(n);
    if (blocks > 0x7fffffffLL) return fail(FIVEEQ_E_INVALID, "n too large");
    hipLaunchKernelGGL(fiveeq::math_probe_kernel<T>, dim3((unsigned)blocks), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream,
                       op, n, x, y);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace

extern "C" {
int fiveeq_hist_rows_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, double lo, double hi,
                         int32_t n_bins, uint64_t* hist, void* stream) {
    return hist_rows<double>(n_rows, n_members, ld, rows, lo, hi, n_bins, hist, stream);
}
int fiveeq_hist_bins(int32_t n_rows, int64_t n_members, int64_t ld, const uint16_t* bins, int32_t n_bins, uint64_t* hist,
                     void* stream) {
    if (int rc = hist_check(n_rows, n_members, ld, n_bins)) return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    if (!bins || !hist) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (n_rows > 65535) return fail(FIVEEQ_E_INVALID, "n_rows=%d exceeds the 65535 rows of one launch", n_rows);
    int64_t chunk = hist_chunk(n_rows, n_members), chunks;
    chunk = (chunk + 8 * FIVEEQ_BLOCK - 1) / (8 * FIVEEQ_BLOCK) * (8 * FIVEEQ_BLOCK);      // eight members per lane and load
    if (int rc = member_chunks(n_members, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::hist_bins_kernel, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n_members, ld, chunk, bins, n_bins, reinterpret_cast<unsigned long long*>(hist));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
int fiveeq_hist_rows_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, double lo, double hi,
                         int32_t n_bins, uint64_t* hist, void* stream) {
    return hist_rows<float>(n_rows, n_members, ld, rows, lo, hi, n_bins, hist, stream);
}
// ---- end-of-run summary passes (kernels 6a-6c) ----------------------------------------------------------------
}  // extern "C"
namespace {
// members per workgroup of a summary pass: the histogram pass's chunking, rounded to whole 16-byte-per-lane loads
int64_t summary_chunk(int32_t n_rows, int64_t n) {
    const int64_t unit = 4 * FIVEEQ_BLOCK;                  // 4 floats / 2 doubles per lane: a multiple of both
    return (hist_chunk(n_rows, n) + unit - 1) / unit * unit;
}
int summary_check(int32_t n_rows, int64_t n, int64_t ld, const void* rows) {
    if (int rc = check_n_rows(n_rows)) return rc;
    if (n_rows > 65535) return fail(FIVEEQ_E_INVALID, "n_rows=%d exceeds the 65535 rows of one launch", n_rows);
    if (n < 1 || ld < n) return fail(FIVEEQ_E_INVALID, "n_members=%lld, ld=%lld invalid", (long long)n, (long long)ld);
    if (n_rows > 0 && !rows) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    return FIVEEQ_OK;
}
template <typename T>
int row_moments(int32_t n_rows, int64_t n, int64_t ld, const T* rows, double* partial, double* moments, void* stream) {
    if (int rc = summary_check(n_rows, n, ld, rows)) return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    if (!partial || !moments) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    int64_t chunk = summary_chunk(n_rows, n), chunks;
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::row_moments_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, partial);
    hipLaunchKernelGGL(fiveeq::row_moments_fold_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, chunks,
                       partial, moments);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int select_bins(int32_t n_rows, int64_t n, int64_t ld, const T* rows, const double* ranges, int32_t n_bins,
                const uint32_t* binmask, T* cand, int64_t cap, uint64_t* cand_n, void* stream) {
    if (int rc = summary_check(n_rows, n, ld, rows)) return rc;
    if (int rc = check_n_bins(n_bins)) return rc;
    if (cap < 0) return fail(FIVEEQ_E_INVALID, "cap=%lld must be >= 0", (long long)cap);
    if (n_rows == 0) return FIVEEQ_OK;
    if (!ranges || !binmask || !cand_n || (cap > 0 && !cand)) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    int64_t chunk = summary_chunk(n_rows, n), chunks;
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::select_bins_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, ranges, n_bins, binmask, cand, cap,
                       reinterpret_cast<unsigned long long*>(cand_n));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int select_pick(int32_t n_rows, int32_t n_seg, int64_t width, const T* pool, const uint64_t* seg_n, int32_t n_targets,
                const int64_t* ranks, double* picked, void* stream) {
    if (n_rows < 0) return fail(FIVEEQ_E_INVALID, "n_rows=%d invalid", n_rows);
    if (n_seg < 1) return fail(FIVEEQ_E_INVALID, "n_seg=%d must be >= 1", n_seg);
    if (width < 0) return fail(FIVEEQ_E_INVALID, "width=%lld must be >= 0", (long long)width);
    if (n_targets < 1 || n_targets > 65535) return fail(FIVEEQ_E_INVALID, "n_targets=%d outside 1..65535", n_targets);
    if (n_rows == 0) return FIVEEQ_OK;
    if ((width > 0 && !pool) || !seg_n || !ranks || !picked) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    hipLaunchKernelGGL(fiveeq::select_pick_kernel<T>, dim3((unsigned)n_rows, (unsigned)n_targets), dim3(fiveeq::PICK_BLOCK), 0,
                       (hipStream_t)stream, n_seg, width, pool, reinterpret_cast<const unsigned long long*>(seg_n), n_targets,
                       reinterpret_cast<const long long*>(ranks), picked);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int fiveeq_select_pick_f64(int32_t n_rows, int32_t n_seg, int64_t width, const double* pool, const uint64_t* seg_n,
                           int32_t n_targets, const int64_t* ranks, double* picked, void* stream) {
    return select_pick<double>(n_rows, n_seg, width, pool, seg_n, n_targets, ranks, picked, stream);
}
int fiveeq_select_pick_f32(int32_t n_rows, int32_t n_seg, int64_t width, const float* pool, const uint64_t* seg_n,
                           int32_t n_targets, const int64_t* ranks, double* picked, void* stream) {
    return select_pick<float>(n_rows, n_seg, width, pool, seg_n, n_targets, ranks, picked, stream);
}
int64_t fiveeq_row_moments_chunks(int32_t n_rows, int64_t n_members) {
    if (n_rows < 1 || n_members < 1) return 0;
    const int64_t chunk = summary_chunk(n_rows, n_members);
    return (n_members + chunk - 1) / chunk;
}
int fiveeq_row_moments_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, double* partial,
                           double* moments, void* stream) {
    return row_moments<double>(n_rows, n_members, ld, rows, partial, moments, stream);
}
int fiveeq_row_moments_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, double* partial,
                           double* moments, void* stream) {
    return row_moments<float>(n_rows, n_members, ld, rows, partial, moments, stream);
}
int fiveeq_hist_rows_ranged_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, const double* ranges,
                                int32_t n_bins, uint64_t* hist, void* stream) {
    if (!ranges) return fail(FIVEEQ_E_INVALID, "ranges is NULL");
    return hist_rows<double>(n_rows, n_members, ld, rows, 0.0, 0.0, n_bins, hist, stream, ranges);
}
int fiveeq_hist_rows_ranged_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, const double* ranges,
                                int32_t n_bins, uint64_t* hist, void* stream) {
    if (!ranges) return fail(FIVEEQ_E_INVALID, "ranges is NULL");
    return hist_rows<float>(n_rows, n_members, ld, rows, 0.0, 0.0, n_bins, hist, stream, ranges);
}
int fiveeq_select_bins_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, const double* ranges,
                           int32_t n_bins, const uint32_t* binmask, double* cand, int64_t cap, uint64_t* cand_n, void* stream) {
    return select_bins<double>(n_rows, n_members, ld, rows, ranges, n_bins, binmask, cand, cap, cand_n, stream);
}
int fiveeq_select_bins_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, const double* ranges,
                           int32_t n_bins, const uint32_t* binmask, float* cand, int64_t cap, uint64_t* cand_n, void* stream) {
    return select_bins<float>(n_rows, n_members, ld, rows, ranges, n_bins, binmask, cand, cap, cand_n, stream);
}
// ---- weighted end-of-run summary passes (kernels 7a-7d) ------------------------------------------------------------
}  // extern "C"
namespace {
// the checks every weighted pass over rows shares: the sizes, the row pointer and the weights
template <typename T>
int wsummary_check(int32_t n_rows, int64_t n, int64_t ld, const T* rows, const uint64_t* weights) {
    if (int rc = summary_check(n_rows, n, ld, rows)) return rc;
    if (n_rows > 0 && !weights) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(rows, sizeof(T)) || misaligned(weights, 8)) return fail(FIVEEQ_E_INVALID, "rows / weights not aligned to their element size");
    return FIVEEQ_OK;
}
template <typename T>
int wrow_moments(int32_t n_rows, int64_t n, int64_t ld, const T* rows, const uint64_t* weights, double* partial, double* moments,
                 void* stream) {
    if (int rc = wsummary_check(n_rows, n, ld, rows, weights)) return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    if (!partial || !moments) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(partial, 8) || misaligned(moments, 8)) return fail(FIVEEQ_E_INVALID, "partial / moments not 8-byte aligned");
    int64_t chunk = summary_chunk(n_rows, n), chunks;
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::wrow_moments_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, reinterpret_cast<const unsigned long long*>(weights), partial);
    hipLaunchKernelGGL(fiveeq::wrow_moments_fold_kernel, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, chunks,
                       partial, moments);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int whist_rows(int32_t n_rows, int64_t n, int64_t ld, const T* rows, const uint64_t* weights, const double* ranges, int32_t n_bins,
               uint64_t* hist, void* stream) {
    if (int rc = wsummary_check(n_rows, n, ld, rows, weights)) return rc;
    if (int rc = check_n_bins(n_bins)) return rc;
    if (n_rows == 0) return FIVEEQ_OK;
    if (!ranges || !hist) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(ranges, 8) || misaligned(hist, 8)) return fail(FIVEEQ_E_INVALID, "ranges / hist not 8-byte aligned");
    int64_t chunk = ranged_chunk(summary_chunk(n_rows, n), n_bins, 4 * FIVEEQ_BLOCK), chunks;      // in whole 16-byte loads
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::whist_rows_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, reinterpret_cast<const unsigned long long*>(weights), ranges, n_bins,
                       reinterpret_cast<unsigned long long*>(hist));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int wselect_bins(int32_t n_rows, int64_t n, int64_t ld, const T* rows, const uint64_t* weights, const double* ranges,
                 int32_t n_bins, const uint32_t* binmask, T* cand, uint64_t* candw, int64_t cap, uint64_t* cand_n, void* stream) {
    if (int rc = wsummary_check(n_rows, n, ld, rows, weights)) return rc;
    if (int rc = check_n_bins(n_bins)) return rc;
    if (cap < 0) return fail(FIVEEQ_E_INVALID, "cap=%lld must be >= 0", (long long)cap);
    if (n_rows == 0) return FIVEEQ_OK;
    if (!ranges || !binmask || !cand_n || (cap > 0 && (!cand || !candw))) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(ranges, 8) || misaligned(binmask, 4) || misaligned(cand, sizeof(T)) || misaligned(candw, 8) || misaligned(cand_n, 8))
        return fail(FIVEEQ_E_INVALID, "ranges / binmask / cand / candw / cand_n not aligned to their element size");
    int64_t chunk = summary_chunk(n_rows, n), chunks;
    if (int rc = member_chunks(n, chunk, &chunks)) return rc;
    hipLaunchKernelGGL(fiveeq::wselect_bins_kernel<T>, dim3((unsigned)chunks, (unsigned)n_rows), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n, ld, chunk, rows, reinterpret_cast<const unsigned long long*>(weights), ranges, n_bins,
                       binmask, cand, reinterpret_cast<unsigned long long*>(candw), cap, reinterpret_cast<unsigned long long*>(cand_n));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int wselect_pick(int32_t n_rows, int32_t n_seg, int64_t width, const T* pool, const uint64_t* poolw, const uint64_t* seg_n,
                 int32_t n_targets, const int64_t* targets, double* picked, void* stream) {
    if (n_rows < 0 || n_rows > 65535) return fail(FIVEEQ_E_INVALID, "n_rows=%d outside 0..65535", n_rows);
    if (n_seg < 1) return fail(FIVEEQ_E_INVALID, "n_seg=%d must be >= 1", n_seg);
    if (width < 0) return fail(FIVEEQ_E_INVALID, "width=%lld must be >= 0", (long long)width);
    if (n_targets < 1 || n_targets > 65535) return fail(FIVEEQ_E_INVALID, "n_targets=%d outside 1..65535", n_targets);
    if (n_rows == 0) return FIVEEQ_OK;
    if ((width > 0 && (!pool || !poolw)) || !seg_n || !targets || !picked) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(pool, sizeof(T)) || misaligned(poolw, 8) || misaligned(seg_n, 8) || misaligned(targets, 8) || misaligned(picked, 8))
        return fail(FIVEEQ_E_INVALID, "pool / poolw / seg_n / targets / picked not aligned to their element size");
    hipLaunchKernelGGL(fiveeq::wselect_pick_kernel<T>, dim3((unsigned)n_rows, (unsigned)n_targets), dim3(fiveeq::PICK_BLOCK), 0,
                       (hipStream_t)stream, n_seg, width, pool, reinterpret_cast<const unsigned long long*>(poolw),
                       reinterpret_cast<const unsigned long long*>(seg_n), n_targets, reinterpret_cast<const long long*>(targets),
                       picked);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int64_t fiveeq_wrow_moments_chunks(int32_t n_rows, int64_t n_members) { return fiveeq_row_moments_chunks(n_rows, n_members); }
int fiveeq_wrow_moments_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, const uint64_t* weights,
                            double* partial, double* moments, void* stream) {
    return wrow_moments<double>(n_rows, n_members, ld, rows, weights, partial, moments, stream);
}
int fiveeq_wrow_moments_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, const uint64_t* weights,
                            double* partial, double* moments, void* stream) {
    return wrow_moments<float>(n_rows, n_members, ld, rows, weights, partial, moments, stream);
}
int fiveeq_whist_rows_ranged_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, const uint64_t* weights,
                                 const double* ranges, int32_t n_bins, uint64_t* hist, void* stream) {
    return whist_rows<double>(n_rows, n_members, ld, rows, weights, ranges, n_bins, hist, stream);
}
int fiveeq_whist_rows_ranged_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, const uint64_t* weights,
                                 const double* ranges, int32_t n_bins, uint64_t* hist, void* stream) {
    return whist_rows<float>(n_rows, n_members, ld, rows, weights, ranges, n_bins, hist, stream);
}
int fiveeq_wselect_bins_f64(int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, const uint64_t* weights,
                            const double* ranges, int32_t n_bins, const uint32_t* binmask, double* cand, uint64_t* candw,
                            int64_t cap, uint64_t* cand_n, void* stream) {
    return wselect_bins<double>(n_rows, n_members, ld, rows, weights, ranges, n_bins, binmask, cand, candw, cap, cand_n, stream);
}
int fiveeq_wselect_bins_f32(int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, const uint64_t* weights,
                            const double* ranges, int32_t n_bins, const uint32_t* binmask, float* cand, uint64_t* candw,
                            int64_t cap, uint64_t* cand_n, void* stream) {
    return wselect_bins<float>(n_rows, n_members, ld, rows, weights, ranges, n_bins, binmask, cand, candw, cap, cand_n, stream);
}
int fiveeq_wselect_pick_f64(int32_t n_rows, int32_t n_seg, int64_t width, const double* pool, const uint64_t* poolw,
                            const uint64_t* seg_n, int32_t n_targets, const int64_t* targets, double* picked, void* stream) {
    return wselect_pick<double>(n_rows, n_seg, width, pool, poolw, seg_n, n_targets, targets, picked, stream);
}
int fiveeq_wselect_pick_f32(int32_t n_rows, int32_t n_seg, int64_t width, const float* pool, const uint64_t* poolw,
                            const uint64_t* seg_n, int32_t n_targets, const int64_t* targets, double* picked, void* stream) {
    return wselect_pick<float>(n_rows, n_seg, width, pool, poolw, seg_n, n_targets, targets, picked, stream);
}
// ---- resampling a weighted ensemble (kernels 8a-8c) ------------------------------------------------------------------------
}  // extern "C"
namespace {
template <typename T>
int gather_rows(int32_t n_rows, int64_t n_out, int64_t ld_in, const T* rows_in, int64_t ld_out, T* rows_out, const int32_t* src,
                void* stream) {
    if (int rc = check_n_rows(n_rows)) return rc;
    if (n_out < 0 || n_out > MEMBERS_MAX) return fail(FIVEEQ_E_INVALID, "n_out=%lld outside 0..2^31-1", (long long)n_out);
    if (ld_in < 1 || ld_in > MEMBERS_MAX) return fail(FIVEEQ_E_INVALID, "ld_in=%lld outside 1..2^31-1", (long long)ld_in);
    if (ld_out < n_out) return fail(FIVEEQ_E_INVALID, "ld_out=%lld < n_out=%lld", (long long)ld_out, (long long)n_out);
    if (n_rows == 0 || n_out == 0) return FIVEEQ_OK;
    if (!rows_in || !rows_out || !src) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(rows_in, sizeof(T)) || misaligned(rows_out, sizeof(T)) || misaligned(src, 4))
        return fail(FIVEEQ_E_INVALID, "rows_in / rows_out / src not aligned to their element size");
    hipLaunchKernelGGL(fiveeq::gather_rows_kernel<T>, dim3((unsigned)((n_out + FIVEEQ_BLOCK - 1) / FIVEEQ_BLOCK)), dim3(FIVEEQ_BLOCK), 0,
                       (hipStream_t)stream, n_rows, n_out, ld_in, rows_in, ld_out, rows_out, src);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int64_t fiveeq_wscan_chunks(int64_t n_members) {
    if (n_members < 1) return 0;
    return (n_members + fiveeq::WSCAN_TILE - 1) / fiveeq::WSCAN_TILE * fiveeq::WSCAN_WORDS;
}
int fiveeq_wscan(int64_t n_members, const uint64_t* weights, uint64_t* partial, uint64_t* cum, uint64_t* flags, void* stream) {
    if (int rc = check_members(n_members)) return rc;
    if (!weights || !partial || !cum || !flags) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(weights, 8) || misaligned(partial, 8) || misaligned(cum, 8) || misaligned(flags, 8))
        return fail(FIVEEQ_E_INVALID, "weights / partial / cum / flags not 8-byte aligned");
    const int64_t tiles = (n_members + fiveeq::WSCAN_TILE - 1) / fiveeq::WSCAN_TILE;
    const unsigned long long* w = reinterpret_cast<const unsigned long long*>(weights);
    unsigned long long* part = reinterpret_cast<unsigned long long*>(partial);
    hipLaunchKernelGGL(fiveeq::wscan_sums_kernel, dim3((unsigned)tiles), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, n_members, w, part);
    hipLaunchKernelGGL(fiveeq::wscan_spine_kernel, dim3(1), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, tiles, part,
                       reinterpret_cast<unsigned long long*>(flags));
    hipLaunchKernelGGL(fiveeq::wscan_tiles_kernel, dim3((unsigned)tiles), dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, n_members, w, part,
                       reinterpret_cast<unsigned long long*>(cum));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
int fiveeq_resample_pick(int64_t n_members, const uint64_t* cum, uint64_t c_lo, int64_t M, int64_t q, int64_t a, int64_t s, int64_t b,
                         int64_t j0, int64_t n_out, int32_t* src, void* stream) {
    if (int rc = check_members(n_members)) return rc;
    if (M < 1 || M > MEMBERS_MAX) return fail(FIVEEQ_E_INVALID, "M=%lld outside 1..2^31-1", (long long)M);
    if (q < 0 || a < 0) return fail(FIVEEQ_E_INVALID, "q=%lld, a=%lld must be >= 0", (long long)q, (long long)a);
    if (s < 0 || s >= M || b < 0 || b >= M)
        return fail(FIVEEQ_E_INVALID, "s=%lld, b=%lld outside [0, M=%lld)", (long long)s, (long long)b, (long long)M);
    if (j0 < 0 || n_out < 0 || j0 > M || n_out > M - j0)
        return fail(FIVEEQ_E_INVALID, "j0=%lld, n_out=%lld: not a range of the M=%lld outputs", (long long)j0, (long long)n_out, (long long)M);
    // the last position, (M - 1) q + a + ((M - 1) s + b) div M, must stay below 2^63 (it is below W for a plan of the host)
    const unsigned __int128 last = (unsigned __int128)(M - 1) * (unsigned __int128)q + (unsigned __int128)a +
                                   (unsigned __int128)(((M - 1) * s + b) / M);
    if (last > (unsigned __int128)INT64_MAX)
        return fail(FIVEEQ_E_INVALID, "q=%lld, a=%lld: positions beyond 2^63", (long long)q, (long long)a);
    if (n_out == 0) return FIVEEQ_OK;
    if (!cum || !src) return fail(FIVEEQ_E_INVALID, "NULL device pointer");
    if (misaligned(cum, 8) || misaligned(src, 4)) return fail(FIVEEQ_E_INVALID, "cum / src not aligned to their element size");
    hipLaunchKernelGGL(fiveeq::resample_pick_kernel, dim3((unsigned)((n_out + fiveeq::PICK_SRC_BLOCK - 1) / fiveeq::PICK_SRC_BLOCK)),
                       dim3(fiveeq::PICK_SRC_BLOCK), 0, (hipStream_t)stream, n_members, reinterpret_cast<const unsigned long long*>(cum),
                       (unsigned long long)c_lo, (unsigned long long)M, (unsigned long long)q, (unsigned long long)a,
                       (unsigned long long)s, (unsigned long long)b, j0, n_out, src);
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
int fiveeq_gather_rows_f64(int32_t n_rows, int64_t n_out, int64_t ld_in, const double* rows_in, int64_t ld_out, double* rows_out,
                           const int32_t* src, void* stream) {
    return gather_rows<double>(n_rows, n_out, ld_in, rows_in, ld_out, rows_out, src, stream);
}
int fiveeq_gather_rows_f32(int32_t n_rows, int64_t n_out, int64_t ld_in, const float* rows_in, int64_t ld_out, float* rows_out,
                           const int32_t* src, void* stream) {
    return gather_rows<float>(n_rows, n_out, ld_in, rows_in, ld_out, rows_out, src, stream);
}
// ---- per-member trajectory metrics of stored rows (kernel 9) ---------------------------------------------------------------
}  // extern "C"
namespace {
static_assert(fiveeq::METRICS_MAX_LEVELS == FIVEEQ_MAX_LEVELS && fiveeq::METRICS_MAX_WINDOWS == FIVEEQ_MAX_WINDOWS,
              "fiveeq_metrics.hpp and fiveeq.h disagree");
template <typename T>
int traj_metrics(int32_t n_scen, int32_t n_rows, int64_t n, int64_t ld, const T* rows, int64_t scen_stride, const int32_t* steps,
                 int32_t n_levels, const double* levels, int32_t n_windows, const int32_t* windows, double* fmet, int32_t* imet,
                 int32_t first_call, void* stream) {
    if (int rc = check_scen(n_scen)) return rc;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (n_scen > 1 && scen_stride < (int64_t)n_rows * ld)
        return fail(FIVEEQ_E_INVALID, "scen_stride=%lld < n_rows * ld = %lld", (long long)scen_stride, (long long)((int64_t)n_rows * ld));
    if (n_levels < 0 || n_levels > FIVEEQ_MAX_LEVELS) return fail(FIVEEQ_E_INVALID, "n_levels=%d outside 0..%d", n_levels, FIVEEQ_MAX_LEVELS);
    if (n_windows < 0 || n_windows > FIVEEQ_MAX_WINDOWS)
        return fail(FIVEEQ_E_INVALID, "n_windows=%d outside 0..%d", n_windows, FIVEEQ_MAX_WINDOWS);
    if (n_levels > 0 && !levels) return fail(FIVEEQ_E_INVALID, "levels is NULL with n_levels=%d", n_levels);
    if (n_windows > 0 && !windows) return fail(FIVEEQ_E_INVALID, "windows is NULL with n_windows=%d", n_windows);
    const NamedPtrs ptrs = {{"rows", rows, sizeof(T), n_rows > 0}, {"steps", steps, 4, n_rows > 0}, {"fmet", fmet, 8}, {"imet", imet, 4}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    fiveeq::MetricsSpec sp = {};
    for (int l = 0; l < n_levels; ++l) {
        if (std::isnan(levels[l])) return fail(FIVEEQ_E_INVALID, "levels[%d] is NaN", l);
        sp.level[l] = levels[l];
    }
    for (int w = 0; w < n_windows; ++w) {
        const int32_t a = windows[2 * w], b = windows[2 * w + 1];
        if (a < 0 || a > b) return fail(FIVEEQ_E_INVALID, "windows[%d] = [%d, %d): want 0 <= a <= b", w, a, b);
        sp.win[w][0] = a, sp.win[w][1] = b;
    }
    sp.n_levels = n_levels, sp.n_windows = n_windows;
    if (n_rows == 0 && !first_call) return FIVEEQ_OK;         // nothing to fold into the state
    // every row starts at rows + s scen_stride + k ld
    const bool wide = !misaligned(rows, 16) && ld % PER16<T> == 0 && (n_scen == 1 || scen_stride % PER16<T> == 0);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        dispatch_count<0, FIVEEQ_MAX_LEVELS>(n_levels, [&](auto nl) {          // a kernel per number of levels (fiveeq_metrics.hpp)
            const dim3 grid((unsigned)((members + fiveeq::METRICS_TILE<T> - 1) / fiveeq::METRICS_TILE<T>), (unsigned)n_scen);
            const auto launch = [&](auto first) {
                hipLaunchKernelGGL((fiveeq::traj_metrics_kernel<T, decltype(first)::value, decltype(nl)::value, decltype(vec)::value>), grid,
                                   dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, n_rows, (int)members, ld, rows + m0, scen_stride, steps, sp,
                                   fmet + m0, imet + m0);
            };
            if (first_call) launch(std::true_type{});
            else launch(std::false_type{});
        });
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_max_levels(void) { return FIVEEQ_MAX_LEVELS; }
int32_t fiveeq_max_windows(void) { return FIVEEQ_MAX_WINDOWS; }
int32_t fiveeq_metrics_tile(int32_t elem_bytes) {
    return elem_bytes == 8 ? fiveeq::METRICS_TILE<double> : elem_bytes == 4 ? fiveeq::METRICS_TILE<float> : 0;
}
int32_t fiveeq_metrics_unroll(int32_t wide) { return wide ? fiveeq::METRICS_UNROLL : fiveeq::METRICS_UNROLL_NARROW; }
int fiveeq_traj_metrics_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, int64_t scen_stride,
                            const int32_t* steps, int32_t n_levels, const double* levels, int32_t n_windows, const int32_t* windows,
                            double* fmet, int32_t* imet, int32_t first_call, void* stream) {
    return traj_metrics<double>(n_scen, n_rows, n_members, ld, rows, scen_stride, steps, n_levels, levels, n_windows, windows, fmet, imet,
                                first_call, stream);
}
int fiveeq_traj_metrics_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, int64_t scen_stride,
                            const int32_t* steps, int32_t n_levels, const double* levels, int32_t n_windows, const int32_t* windows,
                            double* fmet, int32_t* imet, int32_t first_call, void* stream) {
    return traj_metrics<float>(n_scen, n_rows, n_members, ld, rows, scen_stride, steps, n_levels, levels, n_windows, windows, fmet, imet,
                               first_call, stream);
}
// ---- running means and linear-trend sums of stored rows (kernels 15a / 15b) -------------------------------------------------
}  // extern "C"
namespace {
static_assert(fiveeq::SMOOTH_MAX_WINDOW == FIVEEQ_MAX_SMOOTH_WINDOW, "fiveeq_smooth.hpp and fiveeq.h disagree");
static_assert((size_t)fiveeq::SMOOTH_BLOCK * 16 * FIVEEQ_MAX_SMOOTH_WINDOW <= 64 * 1024,
              "running_mean_kernel's ring outgrows the default dynamic-LDS limit: the launcher would have to raise it");
// what both passes check first, in the order include/fiveeq.h lists it
int smooth_check(int32_t n_scen, int32_t n_rows, int64_t n, int64_t ld, int64_t scen_stride) {
    if (int rc = check_scen(n_scen)) return rc;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (n_scen > 1 && scen_stride < (int64_t)n_rows * ld)
        return fail(FIVEEQ_E_INVALID, "scen_stride=%lld < n_rows * ld = %lld", (long long)scen_stride, (long long)((int64_t)n_rows * ld));
    return FIVEEQ_OK;
}
template <typename T>
int running_mean(int32_t n_scen, int32_t n_rows, int64_t n, int64_t ld, const T* rows, int64_t scen_stride, int32_t window, int32_t n_tail,
                 const T* tail, int64_t tail_scen_stride, double* out, int64_t out_scen_stride, void* stream) {
    if (int rc = smooth_check(n_scen, n_rows, n, ld, scen_stride)) return rc;
    if (window < 1 || window > FIVEEQ_MAX_SMOOTH_WINDOW)
        return fail(FIVEEQ_E_INVALID, "window=%d outside 1..%d", window, FIVEEQ_MAX_SMOOTH_WINDOW);
    if (n_tail < 0 || n_tail > window - 1) return fail(FIVEEQ_E_INVALID, "n_tail=%d outside 0..window-1 = %d", n_tail, window - 1);
    const int64_t total = (int64_t)n_tail + n_rows, n_out = total >= window ? total - window + 1 : 0;
    if (n_scen > 1 && tail_scen_stride < (int64_t)n_tail * ld)
        return fail(FIVEEQ_E_INVALID, "tail_scen_stride=%lld < n_tail * ld = %lld", (long long)tail_scen_stride, (long long)((int64_t)n_tail * ld));
    if (n_scen > 1 && out_scen_stride < n_out * ld)
        return fail(FIVEEQ_E_INVALID, "out_scen_stride=%lld < n_out * ld = %lld", (long long)out_scen_stride, (long long)(n_out * ld));
    const NamedPtrs ptrs = {{"rows", rows, sizeof(T), n_rows > 0}, {"tail", tail, sizeof(T), n_tail > 0}, {"out", out, 8, n_out > 0}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    if (n_out == 0) return FIVEEQ_OK;                          // fewer rows than a window: no output
    // every row the pass touches starts at base + s stride + k ld: 16-byte accesses where all of them are aligned (out is
    // fp64: two elements per 16 bytes, which ld % PER16<T> == 0 covers for either T)
    const bool many = n_scen > 1;
    const bool wide = ld % PER16<T> == 0 && !misaligned(out, 16) && (!many || out_scen_stride % 2 == 0) &&
                      (n_rows == 0 || (!misaligned(rows, 16) && (!many || scen_stride % PER16<T> == 0))) &&
                      (n_tail == 0 || (!misaligned(tail, 16) && (!many || tail_scen_stride % PER16<T> == 0)));
    const size_t lds = (size_t)fiveeq::SMOOTH_BLOCK * 16 * (size_t)window;
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        const dim3 grid((unsigned)((members + fiveeq::SMOOTH_TILE<T> - 1) / fiveeq::SMOOTH_TILE<T>), (unsigned)n_scen);
        hipLaunchKernelGGL((fiveeq::running_mean_kernel<T, decltype(vec)::value>), grid, dim3(fiveeq::SMOOTH_BLOCK), lds, (hipStream_t)stream,
                           n_rows, (int)members, ld, rows ? rows + m0 : rows, scen_stride, window, n_tail, tail ? tail + m0 : tail,
                           tail_scen_stride, out + m0, out_scen_stride);
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int window_trends(int32_t n_scen, int32_t n_rows, int64_t n, int64_t ld, const T* rows, int64_t scen_stride, const int32_t* steps,
                  int32_t n_windows, const int32_t* windows, double* tsum, int32_t first_call, void* stream) {
    if (int rc = smooth_check(n_scen, n_rows, n, ld, scen_stride)) return rc;
    if (n_windows < 0 || n_windows > FIVEEQ_MAX_WINDOWS)
        return fail(FIVEEQ_E_INVALID, "n_windows=%d outside 0..%d", n_windows, FIVEEQ_MAX_WINDOWS);
    if (n_windows > 0 && !windows) return fail(FIVEEQ_E_INVALID, "windows is NULL with n_windows=%d", n_windows);
    const NamedPtrs ptrs = {{"rows", rows, sizeof(T), n_rows > 0}, {"steps", steps, 4, n_rows > 0}, {"tsum", tsum, 8, n_windows > 0}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    fiveeq::TrendSpec sp = {};
    for (int w = 0; w < n_windows; ++w) {
        const int32_t a = windows[2 * w], b = windows[2 * w + 1];
        if (a < 0 || a > b) return fail(FIVEEQ_E_INVALID, "windows[%d] = [%d, %d): want 0 <= a <= b", w, a, b);
        sp.win[w][0] = a, sp.win[w][1] = b;
    }
    sp.n_windows = n_windows;
    if (n_windows == 0 || (n_rows == 0 && !first_call)) return FIVEEQ_OK;         // no state, or nothing to fold into it
    const bool wide = !misaligned(rows, 16) && ld % PER16<T> == 0 && (n_scen == 1 || scen_stride % PER16<T> == 0);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        const dim3 grid((unsigned)((members + fiveeq::TREND_TILE<T> - 1) / fiveeq::TREND_TILE<T>), (unsigned)n_scen);
        const auto launch = [&](auto first) {
            hipLaunchKernelGGL((fiveeq::window_trend_kernel<T, decltype(first)::value, decltype(vec)::value>), grid, dim3(FIVEEQ_BLOCK), 0,
                               (hipStream_t)stream, n_rows, (int)members, ld, rows ? rows + m0 : rows, scen_stride, steps, sp, tsum + m0);
        };
        if (first_call) launch(std::true_type{});
        else launch(std::false_type{});
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_max_smooth_window(void) { return FIVEEQ_MAX_SMOOTH_WINDOW; }
int32_t fiveeq_smooth_tile(int32_t elem_bytes) {
    return elem_bytes == 8 ? fiveeq::SMOOTH_TILE<double> : elem_bytes == 4 ? fiveeq::SMOOTH_TILE<float> : 0;
}
int32_t fiveeq_smooth_unroll(int32_t wide) { return wide ? fiveeq::METRICS_UNROLL : fiveeq::METRICS_UNROLL_NARROW; }
int fiveeq_running_mean_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, int64_t scen_stride,
                            int32_t window, int32_t n_tail, const double* tail, int64_t tail_scen_stride, double* out,
                            int64_t out_scen_stride, void* stream) {
    return running_mean<double>(n_scen, n_rows, n_members, ld, rows, scen_stride, window, n_tail, tail, tail_scen_stride, out,
                                out_scen_stride, stream);
}
int fiveeq_running_mean_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, int64_t scen_stride,
                            int32_t window, int32_t n_tail, const float* tail, int64_t tail_scen_stride, double* out,
                            int64_t out_scen_stride, void* stream) {
    return running_mean<float>(n_scen, n_rows, n_members, ld, rows, scen_stride, window, n_tail, tail, tail_scen_stride, out,
                               out_scen_stride, stream);
}
int fiveeq_window_trends_f64(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, int64_t scen_stride,
                             const int32_t* steps, int32_t n_windows, const int32_t* windows, double* tsum, int32_t first_call,
                             void* stream) {
    return window_trends<double>(n_scen, n_rows, n_members, ld, rows, scen_stride, steps, n_windows, windows, tsum, first_call, stream);
}
int fiveeq_window_trends_f32(int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, int64_t scen_stride,
                             const int32_t* steps, int32_t n_windows, const int32_t* windows, double* tsum, int32_t first_call,
                             void* stream) {
    return window_trends<float>(n_scen, n_rows, n_members, ld, rows, scen_stride, steps, n_windows, windows, tsum, first_call, stream);
}
// ---- joint statistics of per-member rows (kernels 10a / 10b) ----------------------------------------------------------------
}  // extern "C"
namespace {
// the checks both joint passes share; every message names the argument
template <typename T>
int joint_check(int64_t n, int32_t n_x, int64_t ld_x, const T* x, int32_t n_y, int64_t ld_y, const T* y, const uint64_t* weights,
                const double* pivots, const double* partial) {
    if (int rc = check_members(n)) return rc;
    if (n_x < 1 || n_x > fiveeq::JOINT_MAX_ROWS) return fail(FIVEEQ_E_INVALID, "n_x=%d outside 1..%d", n_x, fiveeq::JOINT_MAX_ROWS);
    if (n_y < 1 || n_y > fiveeq::JOINT_MAX_ROWS) return fail(FIVEEQ_E_INVALID, "n_y=%d outside 1..%d", n_y, fiveeq::JOINT_MAX_ROWS);
    if (int rc = check_ld("ld_x", ld_x, n)) return rc;
    if (int rc = check_ld("ld_y", ld_y, n)) return rc;
    const NamedPtrs ptrs = {{"x", x, sizeof(T)}, {"y", y, sizeof(T)}, {"weights", weights, 8}, {"pivots", pivots, 8}, {"partial", partial, 8}};
    if (int rc = check_not_null(ptrs)) return rc;
    return check_aligned(ptrs);
}
template <typename T>
int joint_moments(int64_t n, int32_t n_x, int64_t ld_x, const T* x, int32_t n_y, int64_t ld_y, const T* y, const uint64_t* weights,
                  const double* pivots, double* partial, double* co, double* margins, uint64_t* info, uint64_t* nanrows, void* stream) {
    if (int rc = joint_check(n, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial)) return rc;
    const NamedPtrs ptrs = {{"co", co, 8}, {"margins", margins, 8}, {"info", info, 8}, {"nanrows", nanrows, 8}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    const int64_t chunks = fiveeq_joint_chunks(n), R = n_x + n_y, pairs = (int64_t)n_x * n_y;
    const unsigned tiles = (unsigned)(((n_x + fiveeq::JOINT_TX - 1) / fiveeq::JOINT_TX) * ((n_y + fiveeq::JOINT_TY - 1) / fiveeq::JOINT_TY));
    const hipStream_t st = (hipStream_t)stream;
    const unsigned long long* upart = reinterpret_cast<const unsigned long long*>(partial);
    hipLaunchKernelGGL(fiveeq::joint_moments_kernel<T>, dim3((unsigned)chunks, tiles), dim3(FIVEEQ_BLOCK), 0, st, n, n_x, ld_x, x, n_y,
                       ld_y, y, reinterpret_cast<const unsigned long long*>(weights), pivots, partial);
    hipLaunchKernelGGL(fiveeq::joint_fold_f64_kernel, dim3((unsigned)pairs), dim3(64), 0, st, chunks, partial, co);
    hipLaunchKernelGGL(fiveeq::joint_fold_f64_kernel, dim3((unsigned)(2 * R)), dim3(64), 0, st, chunks, partial + pairs * chunks, margins);
    hipLaunchKernelGGL(fiveeq::joint_fold_u64_kernel, dim3((unsigned)R), dim3(64), 0, st, chunks, upart + (pairs + 2 * R) * chunks,
                       reinterpret_cast<unsigned long long*>(nanrows));
    hipLaunchKernelGGL(fiveeq::joint_fold_info_kernel, dim3(1), dim3(64), 0, st, chunks, R, upart + (pairs + 2 * R) * chunks,
                       upart + (pairs + 3 * R) * chunks, reinterpret_cast<unsigned long long*>(info));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
template <typename T>
int cond_sums(int64_t n, int32_t n_x, int64_t ld_x, const T* x, int32_t n_y, int64_t ld_y, const T* y, const uint64_t* weights,
              int32_t n_bins, const double* edges, const double* pivots, double* partial, double* sums, uint64_t* binw, uint64_t* xnan,
              void* stream) {
    if (int rc = joint_check(n, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial)) return rc;
    if (n_bins < 1 || n_bins > fiveeq::JOINT_MAX_BINS) return fail(FIVEEQ_E_INVALID, "n_bins=%d outside 1..%d", n_bins, fiveeq::JOINT_MAX_BINS);
    if (n_bins > 1 && !edges) return fail(FIVEEQ_E_INVALID, "edges is NULL with n_bins=%d", n_bins);
    const NamedPtrs ptrs = {{"edges", edges, 8, false}, {"sums", sums, 8}, {"binw", binw, 8}, {"xnan", xnan, 8}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    const int64_t chunks = fiveeq_joint_chunks(n), cells = (int64_t)n_x * n_bins;
    const unsigned tiles = (unsigned)(n_x * ((n_bins + fiveeq::COND_TB - 1) / fiveeq::COND_TB) * ((n_y + fiveeq::COND_TY - 1) / fiveeq::COND_TY));
    const hipStream_t st = (hipStream_t)stream;
    const unsigned long long* upart = reinterpret_cast<const unsigned long long*>(partial);
    hipLaunchKernelGGL(fiveeq::cond_sums_kernel<T>, dim3((unsigned)chunks, tiles), dim3(FIVEEQ_BLOCK), 0, st, n, n_x, ld_x, x, n_y, ld_y, y,
                       reinterpret_cast<const unsigned long long*>(weights), n_bins, edges, pivots, partial);
    hipLaunchKernelGGL(fiveeq::joint_fold_f64_kernel, dim3((unsigned)(cells * n_y)), dim3(64), 0, st, chunks, partial, sums);
    hipLaunchKernelGGL(fiveeq::joint_fold_u64_kernel, dim3((unsigned)cells), dim3(64), 0, st, chunks, upart + cells * n_y * chunks,
                       reinterpret_cast<unsigned long long*>(binw));
    hipLaunchKernelGGL(fiveeq::joint_fold_u64_kernel, dim3((unsigned)n_x), dim3(64), 0, st, chunks, upart + cells * (n_y + 1) * chunks,
                       reinterpret_cast<unsigned long long*>(xnan));
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_max_joint_rows(void) { return fiveeq::JOINT_MAX_ROWS; }
int32_t fiveeq_max_cond_bins(void) { return fiveeq::JOINT_MAX_BINS; }
int32_t fiveeq_joint_tile(int32_t which) {
    switch (which) {
        case 0: return fiveeq::JOINT_TX;
        case 1: return fiveeq::JOINT_TY;
        case 2: return fiveeq::JOINT_CHUNK;
        case 3: return fiveeq::Wide<double>::N;
        case 4: return fiveeq::Wide<float>::N;
        case 5: return fiveeq::COND_TB;
        case 6: return fiveeq::COND_TY;
        case 7: return FIVEEQ_BLOCK;
        default: return 0;
    }
}
int64_t fiveeq_joint_chunks(int64_t n_members) {
    return n_members < 1 ? 0 : (n_members + fiveeq::JOINT_CHUNK - 1) / fiveeq::JOINT_CHUNK;
}
int64_t fiveeq_joint_moments_words(int32_t n_x, int32_t n_y) { return (int64_t)n_x * n_y + 3 * (int64_t)(n_x + n_y) + 3; }
int64_t fiveeq_cond_sums_words(int32_t n_x, int32_t n_y, int32_t n_bins) { return (int64_t)n_x * n_bins * (n_y + 1) + n_x; }
int fiveeq_joint_moments_f64(int64_t n_members, int32_t n_x, int64_t ld_x, const double* x, int32_t n_y, int64_t ld_y, const double* y,
                             const uint64_t* weights, const double* pivots, double* partial, double* co, double* margins,
                             uint64_t* info, uint64_t* nanrows, void* stream) {
    return joint_moments<double>(n_members, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial, co, margins, info, nanrows, stream);
}
int fiveeq_joint_moments_f32(int64_t n_members, int32_t n_x, int64_t ld_x, const float* x, int32_t n_y, int64_t ld_y, const float* y,
                             const uint64_t* weights, const double* pivots, double* partial, double* co, double* margins,
                             uint64_t* info, uint64_t* nanrows, void* stream) {
    return joint_moments<float>(n_members, n_x, ld_x, x, n_y, ld_y, y, weights, pivots, partial, co, margins, info, nanrows, stream);
}
int fiveeq_cond_sums_f64(int64_t n_members, int32_t n_x, int64_t ld_x, const double* x, int32_t n_y, int64_t ld_y, const double* y,
                         const uint64_t* weights, int32_t n_bins, const double* edges, const double* pivots, double* partial,
                         double* sums, uint64_t* binw, uint64_t* xnan, void* stream) {
    return cond_sums<double>(n_members, n_x, ld_x, x, n_y, ld_y, y, weights, n_bins, edges, pivots, partial, sums, binw, xnan, stream);
}
int fiveeq_cond_sums_f32(int64_t n_members, int32_t n_x, int64_t ld_x, const float* x, int32_t n_y, int64_t ld_y, const float* y,
                         const uint64_t* weights, int32_t n_bins, const double* edges, const double* pivots, double* partial,
                         double* sums, uint64_t* binw, uint64_t* xnan, void* stream) {
    return cond_sums<float>(n_members, n_x, ld_x, x, n_y, ld_y, y, weights, n_bins, edges, pivots, partial, sums, binw, xnan, stream);
}
int fiveeq_math_probe_f64(int32_t op, int64_t n, const double* x, double* y, void* stream) {
    return math_probe<double>(op, n, x, y, stream);
}
int fiveeq_math_probe_f32(int32_t op, int64_t n, const float* x, float* y, void* stream) {
    return math_probe<float>(op, n, x, y, stream);
}
// ---- scoring stored rows against observed records (kernel 11) ----------------------------------------------------------------
}  // extern "C"
namespace {
static_assert(fiveeq::SCORE_MAX_Q == FIVEEQ_MAX_SCORE_Q, "fiveeq_score.hpp and fiveeq.h disagree");
template <typename T>
int score_rows(int32_t n_q, int32_t n_rows, int64_t n, const T* rows, int64_t row_stride, int64_t q_stride, const int32_t* steps,
               const double* obs, int32_t n_steps, double* misfit, int64_t ld_m, void* stream) {
    if (n_q < 1 || n_q > FIVEEQ_MAX_SCORE_Q) return fail(FIVEEQ_E_INVALID, "n_q=%d outside 1..%d", n_q, FIVEEQ_MAX_SCORE_Q);
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld_m", ld_m, n)) return rc;
    if (int rc = n_q > 1 ? check_stride("q_stride", q_stride, n) : FIVEEQ_OK) return rc;
    if (int rc = n_rows > 1 ? check_ld("row_stride", row_stride, n) : FIVEEQ_OK) return rc;
    if (n_steps < 1) return fail(FIVEEQ_E_INVALID, "n_steps=%d must be >= 1", n_steps);
    const NamedPtrs ptrs = {{"rows", rows, sizeof(T), n_rows > 0}, {"steps", steps, 4, n_rows > 0}, {"obs", obs, 8}, {"misfit", misfit, 8}};
    if (int rc = check_not_null(ptrs)) return rc;
    if (int rc = check_aligned(ptrs)) return rc;
    if (n_rows == 0) return FIVEEQ_OK;                         // nothing to fold into the accumulators
    // every row starts at rows + k row_stride + j q_stride
    const bool wide = !misaligned(rows, 16) && (n_rows == 1 || row_stride % PER16<T> == 0) && (n_q == 1 || q_stride % PER16<T> == 0);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        const dim3 grid((unsigned)((members + fiveeq::SCORE_TILE<T> - 1) / fiveeq::SCORE_TILE<T>));
        hipLaunchKernelGGL((fiveeq::score_rows_kernel<T, decltype(vec)::value>), grid, dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, n_q, n_rows,
                           (int)members, rows + m0, row_stride, q_stride, steps, obs, n_steps, misfit + m0, ld_m);
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_max_score_quantities(void) { return FIVEEQ_MAX_SCORE_Q; }
int32_t fiveeq_score_tile(int32_t elem_bytes) {
    return elem_bytes == 8 ? fiveeq::SCORE_TILE<double> : elem_bytes == 4 ? fiveeq::SCORE_TILE<float> : 0;
}
int32_t fiveeq_score_unroll(int32_t wide) { return wide ? fiveeq::SCORE_UNROLL : fiveeq::SCORE_UNROLL_NARROW; }
int fiveeq_score_rows_f64(int32_t n_q, int32_t n_rows, int64_t n_members, const double* rows, int64_t row_stride, int64_t q_stride,
                          const int32_t* steps, const double* obs, int32_t n_steps, double* misfit, int64_t ld_m, void* stream) {
    return score_rows<double>(n_q, n_rows, n_members, rows, row_stride, q_stride, steps, obs, n_steps, misfit, ld_m, stream);
}
int fiveeq_score_rows_f32(int32_t n_q, int32_t n_rows, int64_t n_members, const float* rows, int64_t row_stride, int64_t q_stride,
                          const int32_t* steps, const double* obs, int32_t n_steps, double* misfit, int64_t ld_m, void* stream) {
    return score_rows<float>(n_q, n_rows, n_members, rows, row_stride, q_stride, steps, obs, n_steps, misfit, ld_m, stream);
}
// ---- forcing, energy imbalance and heat uptake from stored rows (kernel 12) --------------------------------------------------
}  // extern "C"
namespace {
template <typename T>
int forcing_rows(const fiveeq_model* model, int32_t n_rows, int64_t n, int64_t ld, const T* C, int64_t c_row, int64_t c_gas, const T* Trows,
                 int64_t t_row, const int32_t* steps, const T* drive, int32_t n_steps, const T* q, const T* fscale, int32_t n_fext,
                 const T* fext, T* F, T* Fg, T* Nout, double* H, int64_t ld_out, double* H_io, T* S_io, uint64_t* n_mismatch,
                 void* stream) {
    if (int rc = check_model(model)) return rc;
    const int G = model->n_gas;
    const bool outs = F || Fg || Nout || H;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = outs ? check_ld("ld_out", ld_out, n) : FIVEEQ_OK) return rc;
    if (int rc = n_rows > 1 ? check_ld("c_row_stride", c_row, n) : FIVEEQ_OK) return rc;
    if (int rc = G > 1 ? check_stride("c_gas_stride", c_gas, n) : FIVEEQ_OK) return rc;
    if (int rc = Trows && n_rows > 1 ? check_ld("t_row_stride", t_row, n) : FIVEEQ_OK) return rc;
    if (!Trows && (Nout || H || H_io)) return fail(FIVEEQ_E_INVALID, "N / H / H_io need T_rows: T_rows is NULL");
    if (!Trows && S_io) return fail(FIVEEQ_E_INVALID, "S_io (the replay) needs T_rows: T_rows is NULL");
    if (S_io && !n_mismatch) return fail(FIVEEQ_E_INVALID, "S_io (the replay) needs n_mismatch: n_mismatch is NULL");
    if (int rc = check_fext(n_fext, fscale, fext)) return rc;
    if (n_steps < 1) return fail(FIVEEQ_E_INVALID, "n_steps=%d must be >= 1", n_steps);
    if (int rc = check_not_null({{"C_rows", C, 1, n_rows > 0}, {"steps", steps, 4, n_rows > 0}, {"drive", drive}, {"q", q}})) return rc;
    const void* elem[] = {C, Trows, drive, q, fscale, fext, F, Fg, Nout, S_io};
    for (const void* p : elem)
        if (misaligned(p, sizeof(T))) return fail(FIVEEQ_E_INVALID, "a row pointer (%p) is not %d-byte aligned", p, (int)sizeof(T));
    if (int rc = check_aligned({{"steps", steps, 4}})) return rc;
    if (misaligned(H, 8) || misaligned(H_io, 8) || misaligned(n_mismatch, 8))
        return fail(FIVEEQ_E_INVALID, "H, H_io and n_mismatch must be 8-byte aligned");
    if (n_rows == 0) return FIVEEQ_OK;                         // no row: no output row, and the carried state stays what it is
    const bool seq = H || H_io || S_io;
    fiveeq::ForcRowsArgs<T> a;
    a.n_gas = G, a.n_rows = n_rows, a.n = 0, a.n_steps = n_steps, a.n_fext = fscale ? n_fext : 0;
    a.C = C, a.c_row = n_rows > 1 ? c_row : 0, a.c_gas = G > 1 ? c_gas : 0;
    a.Trows = Nout || seq ? Trows : nullptr, a.t_row = n_rows > 1 ? t_row : 0;       // the T rows are read only when something needs them
    a.steps = steps, a.drive = drive, a.q = q, a.fs = fscale, a.X = fscale ? fext : nullptr, a.ld = ld;
    a.F = F, a.Fg = Fg, a.N = Nout, a.H = H, a.ld_out = ld_out, a.H_io = H_io, a.S_io = S_io;
    a.n_mismatch = reinterpret_cast<unsigned long long*>(n_mismatch), a.dt = model->dt;
    const bool wide = !misaligned(C, 16) && !misaligned(a.Trows, 16) && !misaligned(F, 16) && !misaligned(Fg, 16) &&
                      !misaligned(Nout, 16) && !misaligned(H, 16) && a.c_row % PER16<T> == 0 && a.c_gas % PER16<T> == 0 &&
                      (!a.Trows || a.t_row % PER16<T> == 0) && (!outs || ld_out % PER16<T> == 0);
    const KModel<T> km = make_kmodel<T>(model);
    const unsigned gy = seq ? 1u : (unsigned)((n_rows + fiveeq::FORCROWS_YROWS - 1) / fiveeq::FORCROWS_YROWS);
    if (gy > 65535u) return fail(FIVEEQ_E_INVALID, "n_rows=%d too many for one row-parallel launch: at most %d", n_rows, 65535 * fiveeq::FORCROWS_YROWS);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        fiveeq::ForcRowsArgs<T> b = a;
        b.n = (int)members;
        b.C += m0, b.q += m0;
        if (b.Trows) b.Trows += m0;
        if (b.fs) b.fs += m0;
        if (b.F) b.F += m0;
        if (b.Fg) b.Fg += m0;
        if (b.N) b.N += m0;
        if (b.H) b.H += m0;
        if (b.H_io) b.H_io += m0;
        if (b.S_io) b.S_io += m0;
        const dim3 grid((unsigned)((members + fiveeq::FORCROWS_TILE<T> - 1) / fiveeq::FORCROWS_TILE<T>), gy);
        constexpr bool VEC = decltype(vec)::value;
        if (seq) hipLaunchKernelGGL((fiveeq::forcing_rows_kernel<T, VEC, true>), grid, dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, km, b);
        else hipLaunchKernelGGL((fiveeq::forcing_rows_kernel<T, VEC, false>), grid, dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, km, b);
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_forcing_rows_tile(int32_t elem_bytes) {
    return elem_bytes == 8 ? fiveeq::FORCROWS_TILE<double> : elem_bytes == 4 ? fiveeq::FORCROWS_TILE<float> : 0;
}
int fiveeq_forcing_rows_f64(const fiveeq_model* model, int32_t n_rows, int64_t n_members, int64_t ld, const double* C_rows,
                            int64_t c_row_stride, int64_t c_gas_stride, const double* T_rows, int64_t t_row_stride, const int32_t* steps,
                            const double* drive, int32_t n_steps, const double* q, const double* fscale, int32_t n_fext,
                            const double* fext, double* F, double* F_gas, double* N, double* H, int64_t ld_out, double* H_io,
                            double* S_io, uint64_t* n_mismatch, void* stream) {
    return forcing_rows<double>(model, n_rows, n_members, ld, C_rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive, n_steps,
                                q, fscale, n_fext, fext, F, F_gas, N, H, ld_out, H_io, S_io, n_mismatch, stream);
}
int fiveeq_forcing_rows_f32(const fiveeq_model* model, int32_t n_rows, int64_t n_members, int64_t ld, const float* C_rows,
                            int64_t c_row_stride, int64_t c_gas_stride, const float* T_rows, int64_t t_row_stride, const int32_t* steps,
                            const float* drive, int32_t n_steps, const float* q, const float* fscale, int32_t n_fext, const float* fext,
                            float* F, float* F_gas, float* N, double* H, int64_t ld_out, double* H_io, float* S_io,
                            uint64_t* n_mismatch, void* stream) {
    return forcing_rows<float>(model, n_rows, n_members, ld, C_rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive, n_steps,
                               q, fscale, n_fext, fext, F, F_gas, N, H, ld_out, H_io, S_io, n_mismatch, stream);
}
// ---- the response to emission pulses from the stored rows of a scenario engine (kernel 13) -----------------------------------
}  // extern "C"
namespace {
template <typename T>
int pulse_response(const fiveeq_model* model, int32_t n_scen, int32_t n_rows, int64_t n, int64_t ld, const T* C, int64_t c_scen,
                   int64_t c_row, int64_t c_gas, const T* Trows, int64_t t_scen, int64_t t_row, const int32_t* steps, const T* drive,
                   int32_t n_steps, const T* fscale, int32_t n_fext, const T* fext, int32_t base, int32_t n_pulses,
                   const int32_t* pulse_scen, const int32_t* pulse_gas, int32_t n_hor, const int32_t* horizons, int32_t row0,
                   double* out, int64_t ld_out, double* io, void* stream) {
    if (int rc = check_model(model)) return rc;
    const int G = model->n_gas;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (row0 < 0 || row0 > INT32_MAX - n_rows) return fail(FIVEEQ_E_INVALID, "row0=%d with n_rows=%d outside 0..2^31-1", row0, n_rows);
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = check_ld("ld_out", ld_out, n)) return rc;
    if (n_scen < 2) return fail(FIVEEQ_E_INVALID, "n_scen=%d: a base scenario and at least one pulse scenario are needed", n_scen);
    if (n_pulses < 1 || n_pulses > FIVEEQ_MAX_PULSES) return fail(FIVEEQ_E_INVALID, "n_pulses=%d outside 1..%d", n_pulses, FIVEEQ_MAX_PULSES);
    if (n_hor < 1 || n_hor > FIVEEQ_MAX_HORIZONS) return fail(FIVEEQ_E_INVALID, "n_horizons=%d outside 1..%d", n_hor, FIVEEQ_MAX_HORIZONS);
    if (!pulse_scen || !pulse_gas) return fail(FIVEEQ_E_INVALID, "pulse_scen / pulse_gas is NULL");
    if (!horizons) return fail(FIVEEQ_E_INVALID, "horizons is NULL");
    if (base < 0 || base >= n_scen) return fail(FIVEEQ_E_INVALID, "base=%d outside the scenarios 0..%d", base, n_scen - 1);
    for (int p = 0; p < n_pulses; ++p) {
        if (pulse_scen[p] < 0 || pulse_scen[p] >= n_scen)
            return fail(FIVEEQ_E_INVALID, "pulse %d: scenario %d outside the scenarios 0..%d", p, pulse_scen[p], n_scen - 1);
        if (pulse_scen[p] == base) return fail(FIVEEQ_E_INVALID, "pulse %d names the base scenario %d", p, base);
        if (pulse_gas[p] < 0 || pulse_gas[p] >= G) return fail(FIVEEQ_E_INVALID, "pulse %d: gas %d outside the gases 0..%d", p, pulse_gas[p], G - 1);
    }
    for (int h = 0; h < n_hor; ++h) {
        if (horizons[h] < 1) return fail(FIVEEQ_E_INVALID, "horizon %d: %d rows; a horizon is a row count >= 1", h, horizons[h]);
        if (h > 0 && horizons[h] <= horizons[h - 1])
            return fail(FIVEEQ_E_INVALID, "horizons must be strictly increasing: horizon %d is %d after %d", h, horizons[h], horizons[h - 1]);
    }
    if (int rc = n_rows > 1 ? check_ld("c_row_stride", c_row, n) : FIVEEQ_OK) return rc;
    if (int rc = G > 1 ? check_stride("c_gas_stride", c_gas, n) : FIVEEQ_OK) return rc;
    if (int rc = check_stride("c_scen_stride", c_scen, n)) return rc;
    if (int rc = n_rows > 1 ? check_ld("t_row_stride", t_row, n) : FIVEEQ_OK) return rc;
    if (int rc = check_stride("t_scen_stride", t_scen, n)) return rc;
    if (int rc = check_fext(n_fext, fscale, fext)) return rc;
    if (n_steps < 1) return fail(FIVEEQ_E_INVALID, "n_steps=%d must be >= 1", n_steps);
    if (int rc = check_not_null({{"C_rows", C, 1, n_rows > 0}, {"T_rows", Trows, 1, n_rows > 0}, {"steps", steps, 4, n_rows > 0},
                                 {"drive", drive}, {"out", out}, {"io", io}}))
        return rc;
    const void* elem[] = {C, Trows, drive, fscale, fext};
    for (const void* p : elem)
        if (misaligned(p, sizeof(T))) return fail(FIVEEQ_E_INVALID, "a row pointer (%p) is not %d-byte aligned", p, (int)sizeof(T));
    if (int rc = check_aligned({{"steps", steps, 4}})) return rc;
    if (misaligned(out, 8) || misaligned(io, 8)) return fail(FIVEEQ_E_INVALID, "out and io must be 8-byte aligned");
    if (n_rows == 0) return FIVEEQ_OK;                         // no row: nothing is written, and the carried sums stay what they are
    fiveeq::PulseArgs<T> a;
    a.n_gas = G, a.n_rows = n_rows, a.n = 0, a.n_steps = n_steps, a.n_fext = fscale ? n_fext : 0, a.n_hor = n_hor, a.row0 = row0;
    a.scen[0] = base;
    for (int p = 0; p < fiveeq::PULSE_MAX; ++p) {
        a.scen[1 + p] = p < n_pulses ? pulse_scen[p] : base;
        a.gas[p] = p < n_pulses ? pulse_gas[p] : 0;
    }
    for (int h = 0; h < fiveeq::PULSE_MAX_HORIZONS; ++h) a.hor[h] = h < n_hor ? horizons[h] : fiveeq::PULSE_NO_HORIZON;
    a.C = C, a.c_scen = c_scen, a.c_row = n_rows > 1 ? c_row : 0, a.c_gas = G > 1 ? c_gas : 0;
    a.Trows = Trows, a.t_scen = t_scen, a.t_row = n_rows > 1 ? t_row : 0;
    a.steps = steps, a.drive = drive, a.fs = fscale, a.X = fscale ? fext : nullptr, a.ld = ld;
    a.out = out, a.ld_out = ld_out, a.io = io;
    const bool wide = !misaligned(C, 16) && !misaligned(Trows, 16) && !misaligned(out, 16) && a.c_scen % PER16<T> == 0 &&
                      a.c_row % PER16<T> == 0 && a.c_gas % PER16<T> == 0 && a.t_scen % PER16<T> == 0 && a.t_row % PER16<T> == 0 &&
                      ld_out % 2 == 0;
    const KModel<T> km = make_kmodel<T>(model);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        fiveeq::PulseArgs<T> b = a;
        b.n = (int)members;
        b.C += m0, b.Trows += m0, b.out += m0, b.io += m0;
        if (b.fs) b.fs += m0;
        const dim3 grid((unsigned)((members + fiveeq::METRICS_TILE<T> - 1) / fiveeq::METRICS_TILE<T>));
        dispatch_count<1, FIVEEQ_MAX_PULSES>(n_pulses, [&](auto np) {
            hipLaunchKernelGGL((fiveeq::pulse_response_kernel<T, decltype(vec)::value, decltype(np)::value>), grid, dim3(FIVEEQ_BLOCK), 0,
                               (hipStream_t)stream, km, b);
        });
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_max_pulses(void) { return FIVEEQ_MAX_PULSES; }
int32_t fiveeq_max_horizons(void) { return FIVEEQ_MAX_HORIZONS; }
int fiveeq_pulse_response_f64(const fiveeq_model* model, int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const double* C_rows,
                              int64_t c_scen_stride, int64_t c_row_stride, int64_t c_gas_stride, const double* T_rows,
                              int64_t t_scen_stride, int64_t t_row_stride, const int32_t* steps, const double* drive, int32_t n_steps,
                              const double* fscale, int32_t n_fext, const double* fext, int32_t base, int32_t n_pulses,
                              const int32_t* pulse_scen, const int32_t* pulse_gas, int32_t n_horizons, const int32_t* horizons,
                              int32_t row0, double* out, int64_t ld_out, double* io, void* stream) {
    return pulse_response<double>(model, n_scen, n_rows, n_members, ld, C_rows, c_scen_stride, c_row_stride, c_gas_stride, T_rows,
                                  t_scen_stride, t_row_stride, steps, drive, n_steps, fscale, n_fext, fext, base, n_pulses, pulse_scen,
                                  pulse_gas, n_horizons, horizons, row0, out, ld_out, io, stream);
}
int fiveeq_pulse_response_f32(const fiveeq_model* model, int32_t n_scen, int32_t n_rows, int64_t n_members, int64_t ld, const float* C_rows,
                              int64_t c_scen_stride, int64_t c_row_stride, int64_t c_gas_stride, const float* T_rows,
                              int64_t t_scen_stride, int64_t t_row_stride, const int32_t* steps, const float* drive, int32_t n_steps,
                              const float* fscale, int32_t n_fext, const float* fext, int32_t base, int32_t n_pulses,
                              const int32_t* pulse_scen, const int32_t* pulse_gas, int32_t n_horizons, const int32_t* horizons,
                              int32_t row0, double* out, int64_t ld_out, double* io, void* stream) {
    return pulse_response<float>(model, n_scen, n_rows, n_members, ld, C_rows, c_scen_stride, c_row_stride, c_gas_stride, T_rows,
                                 t_scen_stride, t_row_stride, steps, drive, n_steps, fscale, n_fext, fext, base, n_pulses, pulse_scen,
                                 pulse_gas, n_horizons, horizons, row0, out, ld_out, io, stream);
}
// ---- airborne fraction, uptake, alpha and sinks from stored rows (kernel 16) --------------------------------------------------
}  // extern "C"
namespace {
template <typename T>
int carbon_rows(const fiveeq_model* model, int32_t n_rows, int64_t n, int64_t ld, const T* rows, int64_t c_row, int64_t c_gas, const T* Trows,
                int64_t t_row, const int32_t* steps, const T* drive, const T* cum_end, int32_t n_steps, const T* r, int32_t conc_mask,
                int32_t gas_mask, T* airborne, T* cumE, T* uptake, T* fraction, T* iirf, T* alpha, T* sink, int64_t ld_out, T* cum_io,
                T* ga_io, void* stream) {
    if (int rc = check_model(model)) return rc;
    const int G = model->n_gas, all = (1 << G) - 1;
    const bool outs = airborne || cumE || uptake || fraction || iirf || alpha || sink;
    const bool want_alpha = iirf || alpha;
    if (int rc = check_n_rows(n_rows)) return rc;
    if (int rc = check_members(n)) return rc;
    if (int rc = check_ld("ld", ld, n)) return rc;
    if (int rc = outs ? check_ld("ld_out", ld_out, n) : FIVEEQ_OK) return rc;
    if (int rc = n_rows > 1 ? check_ld("c_row_stride", c_row, n) : FIVEEQ_OK) return rc;
    if (int rc = G > 1 ? check_stride("c_gas_stride", c_gas, n) : FIVEEQ_OK) return rc;
    if (int rc = Trows && n_rows > 1 ? check_ld("t_row_stride", t_row, n) : FIVEEQ_OK) return rc;
    if (conc_mask < 0 || conc_mask > all) return fail(FIVEEQ_E_INVALID, "conc_mask=%d names a gas outside the model's %d", conc_mask, G);
    if (gas_mask < 1 || gas_mask > all) return fail(FIVEEQ_E_INVALID, "gas_mask=%d: want at least one gas, and none outside the model's %d", gas_mask, G);
    if (want_alpha && !Trows) return fail(FIVEEQ_E_INVALID, "iirf / alpha need T_rows: T_rows is NULL");
    if (want_alpha && !r) return fail(FIVEEQ_E_INVALID, "iirf / alpha need the r rows: r is NULL");
    if (sink && !ga_io) return fail(FIVEEQ_E_INVALID, "sink needs ga_io (G_a before the first row): ga_io is NULL");
    if ((gas_mask & conc_mask) && (cumE || uptake || fraction || want_alpha) && !cum_io)
        return fail(FIVEEQ_E_INVALID, "cumE, uptake, fraction, iirf and alpha of a concentration-driven gas need cum_io: cum_io is NULL");
    if ((gas_mask & ~conc_mask) && (cumE || uptake || fraction || want_alpha) && !cum_end)
        return fail(FIVEEQ_E_INVALID, "cumE, uptake, fraction, iirf and alpha of an emission-driven gas need cum_end: cum_end is NULL");
    if (n_steps < 1) return fail(FIVEEQ_E_INVALID, "n_steps=%d must be >= 1", n_steps);
    if (int rc = check_not_null({{"rows", rows, 1, n_rows > 0}, {"steps", steps, 4, n_rows > 0}, {"drive", drive}})) return rc;
    const void* elem[] = {rows, Trows, drive, cum_end, r, airborne, cumE, uptake, fraction, iirf, alpha, sink, cum_io, ga_io};
    for (const void* p : elem)
        if (misaligned(p, sizeof(T))) return fail(FIVEEQ_E_INVALID, "a row pointer (%p) is not %d-byte aligned", p, (int)sizeof(T));
    if (int rc = check_aligned({{"steps", steps, 4}})) return rc;
    if (n_rows == 0) return FIVEEQ_OK;                         // no row: no output row, and the carried state stays what it is
    const bool seq = cum_io || ga_io;
    int n_sel = 0;
    for (int g = 0; g < G; ++g) n_sel += gas_mask >> g & 1;
    fiveeq::CarbonArgs<T> a;
    a.n_gas = G, a.n_rows = n_rows, a.n = 0, a.n_steps = n_steps, a.conc_mask = conc_mask, a.gas_mask = gas_mask, a.n_sel = n_sel;
    a.rows = rows, a.c_row = n_rows > 1 ? c_row : 0, a.c_gas = G > 1 ? c_gas : 0;
    a.Trows = want_alpha ? Trows : nullptr, a.t_row = n_rows > 1 ? t_row : 0;         // the T rows are read only when something needs them
    a.steps = steps, a.drive = drive, a.cum_end = cum_end, a.r = want_alpha ? r : nullptr, a.ld = ld;
    T* const out[fiveeq::CARBON_N_OUT] = {airborne, cumE, uptake, fraction, iirf, alpha, sink};
    bool wide = !misaligned(rows, 16) && !misaligned(a.Trows, 16) && a.c_row % PER16<T> == 0 && a.c_gas % PER16<T> == 0 &&
                (!a.Trows || a.t_row % PER16<T> == 0) && (!outs || ld_out % PER16<T> == 0);
    for (int o = 0; o < fiveeq::CARBON_N_OUT; ++o) a.out[o] = out[o], wide = wide && !misaligned(out[o], 16);
    a.ld_out = ld_out, a.cum_io = cum_io, a.ga_io = ga_io;
    const KModel<T> km = make_kmodel<T>(model);
    const unsigned gy = seq ? 1u : (unsigned)((n_rows + fiveeq::CARBON_YROWS - 1) / fiveeq::CARBON_YROWS);
    if (gy > 65535u) return fail(FIVEEQ_E_INVALID, "n_rows=%d too many for one row-parallel launch: at most %d", n_rows, 65535 * fiveeq::CARBON_YROWS);
    launch_split(wide_members<T>(wide, n), n, [&](auto vec, int64_t m0, int64_t members) {
        fiveeq::CarbonArgs<T> b = a;
        b.n = (int)members;
        b.rows += m0;
        if (b.Trows) b.Trows += m0;
        if (b.r) b.r += m0;
        for (int o = 0; o < fiveeq::CARBON_N_OUT; ++o)
            if (b.out[o]) b.out[o] += m0;
        if (b.cum_io) b.cum_io += m0;
        if (b.ga_io) b.ga_io += m0;
        const dim3 grid((unsigned)((members + fiveeq::CARBON_TILE<T> - 1) / fiveeq::CARBON_TILE<T>), gy);
        constexpr bool VEC = decltype(vec)::value;
        if (seq) hipLaunchKernelGGL((fiveeq::carbon_rows_kernel<T, VEC, true>), grid, dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, km, b);
        else hipLaunchKernelGGL((fiveeq::carbon_rows_kernel<T, VEC, false>), grid, dim3(FIVEEQ_BLOCK), 0, (hipStream_t)stream, km, b);
    });
    HIP_TRY(hipGetLastError());
    return FIVEEQ_OK;
}
}  // namespace
extern "C" {
int32_t fiveeq_carbon_rows_tile(int32_t elem_bytes) {
    return elem_bytes == 8 ? fiveeq::CARBON_TILE<double> : elem_bytes == 4 ? fiveeq::CARBON_TILE<float> : 0;
}
int32_t fiveeq_carbon_rows_unroll(int32_t wide, int32_t seq) {
    return wide ? (seq ? fiveeq::CARBON_UNROLL<true, true> : fiveeq::CARBON_UNROLL<true, false>)
                : (seq ? fiveeq::CARBON_UNROLL<false, true> : fiveeq::CARBON_UNROLL<false, false>);
}
int32_t fiveeq_carbon_rows_yrows(void) { return fiveeq::CARBON_YROWS; }
int fiveeq_carbon_rows_f64(const fiveeq_model* model, int32_t n_rows, int64_t n_members, int64_t ld, const double* rows, int64_t c_row_stride,
                           int64_t c_gas_stride, const double* T_rows, int64_t t_row_stride, const int32_t* steps, const double* drive,
                           const double* cum_end, int32_t n_steps, const double* r, int32_t conc_mask, int32_t gas_mask, double* airborne,
                           double* cumE, double* uptake, double* fraction, double* iirf, double* alpha, double* sink, int64_t ld_out,
                           double* cum_io, double* ga_io, void* stream) {
    return carbon_rows<double>(model, n_rows, n_members, ld, rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive, cum_end,
                               n_steps, r, conc_mask, gas_mask, airborne, cumE, uptake, fraction, iirf, alpha, sink, ld_out, cum_io, ga_io,
                               stream);
}
int fiveeq_carbon_rows_f32(const fiveeq_model* model, int32_t n_rows, int64_t n_members, int64_t ld, const float* rows, int64_t c_row_stride,
                           int64_t c_gas_stride, const float* T_rows, int64_t t_row_stride, const int32_t* steps, const float* drive,
                           const float* cum_end, int32_t n_steps, const float* r, int32_t conc_mask, int32_t gas_mask, float* airborne,
                           float* cumE, float* uptake, float* fraction, float* iirf, float* alpha, float* sink, int64_t ld_out,
                           float* cum_io, float* ga_io, void* stream) {
    return carbon_rows<float>(model, n_rows, n_members, ld, rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive, cum_end,
                              n_steps, r, conc_mask, gas_mask, airborne, cumE, uptake, fraction, iirf, alpha, sink, ld_out, cum_io, ga_io,
                              stream);
}

}  // extern "C"
