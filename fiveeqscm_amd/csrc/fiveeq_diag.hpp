// fiveeq_diag.hpp — diagnostics: copies, the math probe, the busy kernel.
// Part of fiveeq_device.hpp, which includes it after the shared constants: include that header, not this one.
#pragma once

namespace fiveeq {

// ---------------------------------------------------------------------------------
// Diagnostic — STREAM copy with the step kernel's access shape (8 B per lane), used to
// measure achievable bandwidth and to calibrate the FETCH_SIZE / WRITE_SIZE counters.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(FIVEEQ_BLOCK) void stream_copy_kernel(const int64_t n, const double* __restrict__ src,
                                                                   double* __restrict__ dst) {
    // four independent 8-byte loads in flight per lane, like the step kernel's row loads
    const int64_t stride = (int64_t)gridDim.x * FIVEEQ_BLOCK;
    int64_t i = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
        const double v0 = src[i], v1 = src[i + stride], v2 = src[i + 2 * stride], v3 = src[i + 3 * stride];
        dst[i] = v0;
        dst[i + stride] = v1;
        dst[i + 2 * stride] = v2;
        dst[i + 3 * stride] = v3;
    }
    for (; i < n; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------------
// Diagnostic — evaluate one of the hand-written math primitives over an array, so that tests can
// pin each of them against a CPU libm to the ulp, independently of the model.
// op: 0 expm1 (x <= 0), 1 exp, 2 log (x > 0), 3 sqrt (x > 0), 4 reciprocal (x > 0).
// fp32 only: op + 8 evaluates the PACKED twin (two members per lane) of the same primitive on the element pairs
// (x[2i], x[2i+1]) — it must give the scalar routine's bits (n even).
// ---------------------------------------------------------------------------------
template <typename V>
__device__ __forceinline__ V math_probe_eval(const int op, const V v) {
    switch (op) {
        case 0: return fe_expm1_neg(v);
        case 1: return fe_exp(v);
        case 2: return fe_log(v);
        case 3: return fe_sqrt(v);
        default: return fe_rcp(v);
    }
}
template <typename T>
__global__ __launch_bounds__(FIVEEQ_BLOCK) void math_probe_kernel(const int op, const int64_t n,
                                                                  const T* __restrict__ x, T* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * FIVEEQ_BLOCK + threadIdx.x;
    if constexpr (sizeof(T) == 4) {
        if (op >= 8) {
            if (2 * i + 1 < n) {
                const float2v r = math_probe_eval(op - 8, float2v{x[2 * i], x[2 * i + 1]});
                y[2 * i] = r.x;
                y[2 * i + 1] = r.y;
            }
            return;
        }
    }
    if (i >= n) return;
    y[i] = math_probe_eval(op, x[i]);
}

// Same copy with 16 B per lane (the widest access, 1 KiB per wave-instruction) and four loads in
// flight: the best plain copy this box does, quoted beside the 8 B/lane figure.  n must be even and
// both pointers 16-byte aligned (checked on the host).
__global__ __launch_bounds__(FIVEEQ_BLOCK) void stream_copy_wide_kernel(const int64_t n2, const double2* __restrict__ src,
                                                                        double2* __restrict__ dst) {
    // each workgroup copies contiguous 16 KiB tiles (4 x 256 lanes x 16 B), four loads in flight per lane
    const int64_t tile = 4 * FIVEEQ_BLOCK;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < n2; base += (int64_t)gridDim.x * tile) {
        const int64_t i = base + threadIdx.x;
        if (base + tile <= n2) {
            const double2 v0 = src[i], v1 = src[i + FIVEEQ_BLOCK], v2 = src[i + 2 * FIVEEQ_BLOCK], v3 = src[i + 3 * FIVEEQ_BLOCK];
            dst[i] = v0;
            dst[i + FIVEEQ_BLOCK] = v1;
            dst[i + 2 * FIVEEQ_BLOCK] = v2;
            dst[i + 3 * FIVEEQ_BLOCK] = v3;
        } else {
            for (int64_t j = i; j < n2; j += FIVEEQ_BLOCK) dst[j] = src[j];
        }
    }
}

// The copy with the NON-TEMPORAL policy on both sides: 8 B per lane, four loads in flight, one workgroup per 8 KiB tile
// (tools/microbench/hbm_rates.hip: the fastest copy of the shapes tried on MI355X, 6.3 TB/s against 5.6-5.8 for the default
// policy at either width — nothing of a 2 GiB copy is worth keeping in the Infinity Cache).  n a multiple of 1024.
__global__ __launch_bounds__(FIVEEQ_BLOCK) void stream_copy_nt_kernel(const int64_t n, const double* __restrict__ src,
                                                                      double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * (4 * FIVEEQ_BLOCK) + threadIdx.x;
    if (i + 3 * FIVEEQ_BLOCK >= n) return;
    const double v0 = __builtin_nontemporal_load(src + i), v1 = __builtin_nontemporal_load(src + i + FIVEEQ_BLOCK),
                 v2 = __builtin_nontemporal_load(src + i + 2 * FIVEEQ_BLOCK), v3 = __builtin_nontemporal_load(src + i + 3 * FIVEEQ_BLOCK);
    __builtin_nontemporal_store(v0, dst + i);
    __builtin_nontemporal_store(v1, dst + i + FIVEEQ_BLOCK);
    __builtin_nontemporal_store(v2, dst + i + 2 * FIVEEQ_BLOCK);
    __builtin_nontemporal_store(v3, dst + i + 3 * FIVEEQ_BLOCK);
}

// A kernel that does nothing for a known time: ONE wave, `iters` dependent fp64 FMAs (~3.5 ns each).  The host uses two of
// them to find out whether two HIP streams really run side by side (streams that share a hardware queue do not:
// fiveeqscm_amd/tuning.py, concurrent_side_streams).  Bounded by construction: the host caps iters.
__global__ __launch_bounds__(64) void busy_kernel(const int64_t iters, double* __restrict__ out) {
    double x = 1.0e-9 * (double)threadIdx.x;
    for (int64_t i = 0; i < iters; ++i) x = fe_fma(x, 0.999999, 1.0e-9);
    if (threadIdx.x == 0) out[0] = x;
}

}  // namespace fiveeq
