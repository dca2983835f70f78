// Host sanitizer run of the argument checks of fiveeq_run_mforc_* / fiveeq_plan_create_mforc_* and fiveeq_noise_rows_*: a
// stand-alone program that compiles the library's translation unit into itself and calls the entry points with their refusal
// cases.  Every call must return FIVEEQ_E_INVALID on the host, before any HIP call, so it runs without a GPU; the fake
// pointers are never dereferenced.  Host code only is instrumented:
//   hipcc -O1 -g -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I include -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/sanitize_member_forcing.hip -o /tmp/sanitize_member_forcing
//   /tmp/sanitize_member_forcing        # prints the cases and "ok"; a sanitizer report or a wrong code exits non-zero
#include "../fiveeqscm_amd/csrc/fiveeq_capi.hip"

#include <cstdio>
#include <cstring>

namespace {

int failures = 0;

void expect(const char* what, int rc, int want, const char* needle) {
    const char* msg = fiveeq_last_error();
    const bool ok = rc == want && (needle == nullptr || std::strstr(msg, needle) != nullptr);
    std::printf("%-58s rc %2d  %s%s\n", what, rc, ok ? "" : "UNEXPECTED: ", rc == FIVEEQ_OK ? "" : msg);
    if (!ok) ++failures;
}

fiveeq_model co2_model() {
    fiveeq_model m;
    std::memset(&m, 0, sizeof m);
    m.n_gas = 1;
    m.dt = 1.0;
    m.d[0] = 239.0;
    m.d[1] = 4.1;
    m.iirf_max = 97.0;
    fiveeq_gas& g = m.gas[0];
    const double a[4] = {0.2173, 0.2240, 0.2824, 0.2763}, tau[4] = {1e6, 394.4, 36.54, 4.304};
    for (int i = 0; i < 4; ++i) {
        g.a[i] = a[i];
        g.tau[i] = tau[i];
    }
    g.n_pools = 4;
    g.g0 = 0.0107;
    g.g1 = 11.41;
    g.C0 = 278.0;
    g.emis2conc = 0.4688;
    g.f[0] = 5.754;
    return m;
}

template <typename T>
void family(const char* sfx) {
    std::printf("-- %s\n", sfx);
    fiveeq_model m = co2_model();
    T* const p = reinterpret_cast<T*>(0x10000);
    T* const odd = reinterpret_cast<T*>(0x10001);
    double* const d = reinterpret_cast<double*>(0x20000);
    void* plan = nullptr;
    auto run = [&](int64_t n, int64_t ld, int t0, int t1, const T* fscale, const T* fext, int n_fext, const double* obs,
                   double* misfit, const T* mforc, int rows, int form, int k) {
        if constexpr (sizeof(T) == 8)
            return fiveeq_run_mforc_f64(&m, n, ld, p, 4, t0, t1, p, p, p, p, nullptr, nullptr, 0, nullptr, fscale, fext, n_fext, obs,
                                        misfit, mforc, rows, form, k, nullptr);
        else
            return fiveeq_run_mforc_f32(&m, n, ld, p, 4, t0, t1, p, p, p, p, nullptr, nullptr, 0, nullptr, fscale, fext, n_fext, obs,
                                        misfit, mforc, rows, form, k, nullptr);
    };
    auto create = [&](int t1, const T* fscale, const T* mforc, int rows, void** out) {
        if constexpr (sizeof(T) == 8)
            return fiveeq_plan_create_mforc_f64(&m, 8, 8, p, 4, 0, t1, p, p, p, p, nullptr, nullptr, 0, nullptr, fscale, nullptr, 0,
                                                nullptr, nullptr, mforc, rows, out);
        else
            return fiveeq_plan_create_mforc_f32(&m, 8, 8, p, 4, 0, t1, p, p, p, p, nullptr, nullptr, 0, nullptr, fscale, nullptr, 0,
                                                nullptr, nullptr, mforc, rows, out);
    };
    auto noise = [&](int64_t m0, int64_t n, int64_t ld, int t0, int t1, const T* phi, const T* s, double* xi, T* rows) {
        if constexpr (sizeof(T) == 8) return fiveeq_noise_rows_f64(1, m0, n, ld, t0, t1, phi, s, xi, rows, nullptr);
        else return fiveeq_noise_rows_f32(1, m0, n, ld, t0, t1, phi, s, xi, rows, nullptr);
    };
    const int E = FIVEEQ_E_INVALID, PS = FIVEEQ_FORM_PER_STEP;
    expect("run_mforc: NULL mforc", run(8, 8, 0, 4, p, p, 2, nullptr, nullptr, nullptr, 4, PS, 0), E, "mforc is NULL");
    expect("run_mforc: misaligned mforc", run(8, 8, 0, 4, p, p, 2, nullptr, nullptr, odd, 4, PS, 0), E, "mforc must be");
    expect("run_mforc: n_mforc_rows < t_end", run(8, 8, 0, 4, p, p, 2, nullptr, nullptr, p, 3, PS, 0), E, "n_mforc_rows=3");
    expect("run_mforc: NULL fscale", run(8, 8, 0, 4, nullptr, p, 2, nullptr, nullptr, p, 4, PS, 0), E, "fscale is NULL");
    expect("run_mforc: NULL fext with a category", run(8, 8, 0, 4, p, nullptr, 1, nullptr, nullptr, p, 4, PS, 0), E, "fext is NULL");
    expect("run_mforc: obs without misfit", run(8, 8, 0, 4, p, p, 2, d, nullptr, p, 4, PS, 0), E, "go together");
    expect("run_mforc: bad step range", run(8, 8, 3, 2, p, p, 2, nullptr, nullptr, p, 4, PS, 0), E, "step range");
    expect("run_mforc: n_members > ld", run(9, 8, 0, 4, p, p, 2, nullptr, nullptr, p, 4, PS, 0), E, "ld=");
    expect("run_mforc: unknown form", run(8, 8, 0, 4, p, nullptr, 0, nullptr, nullptr, p, 4, 2, 0), E, "form=2");
    expect("run_mforc: k_steps < 0", run(8, 8, 0, 4, p, nullptr, 0, nullptr, nullptr, p, 4, FIVEEQ_FORM_FUSED, -1), E, "k_steps=-1");
    expect("run_mforc: empty range, unit scales alone", run(8, 8, 2, 2, p, nullptr, 0, nullptr, nullptr, p, 4, PS, 0), FIVEEQ_OK, nullptr);
    m.n_gas = 2;                                     // pools 4 + 1: a compiled layout without the form
    m.gas[1] = m.gas[0];
    m.gas[1].n_pools = 1;
    expect("run_mforc: a layout without the form", run(8, 8, 0, 4, p, p, 2, nullptr, nullptr, p, 4, PS, 0), E, "no forcing form");
    m.n_gas = 1;
    plan = reinterpret_cast<void*>(0xdead);
    expect("plan_create_mforc: NULL mforc", create(4, p, nullptr, 4, &plan), E, "mforc is NULL");
    if (plan != nullptr) ++failures;
    expect("plan_create_mforc: n_mforc_rows < t_end", create(4, p, p, 1, &plan), E, "n_mforc_rows=1");
    expect("plan_create_mforc: NULL plan_out", create(4, p, p, 4, nullptr), E, "plan_out is NULL");
    expect("plan_create_mforc: step range", create(5, p, p, 5, &plan), E, "step range");

    expect("noise_rows: NULL phi", noise(0, 8, 8, 0, 4, nullptr, p, d, p), E, "phi is NULL");
    expect("noise_rows: NULL s", noise(0, 8, 8, 0, 4, p, nullptr, d, p), E, "s is NULL");
    expect("noise_rows: NULL xi_state", noise(0, 8, 8, 0, 4, p, p, nullptr, p), E, "xi_state is NULL");
    expect("noise_rows: NULL rows", noise(0, 8, 8, 0, 4, p, p, d, nullptr), E, "rows is NULL");
    expect("noise_rows: misaligned rows", noise(0, 8, 8, 0, 4, p, p, d, odd), E, "rows must be");
    expect("noise_rows: misaligned xi_state", noise(0, 8, 8, 0, 4, p, p, reinterpret_cast<double*>(0x20004), p), E, "xi_state must be");
    expect("noise_rows: t_end < t_begin", noise(0, 8, 8, 3, 2, p, p, d, p), E, "step range");
    expect("noise_rows: t_begin < -1", noise(0, 8, 8, -2, 0, p, p, d, p), E, "step range");
    expect("noise_rows: [-1, 1)", noise(0, 8, 8, -1, 1, p, p, d, p), E, "step range");
    expect("noise_rows: n_members > ld", noise(0, 9, 8, 0, 4, p, p, d, p), E, "ld=8 < n_members=9");
    expect("noise_rows: n_members < 1", noise(0, 0, 8, 0, 4, p, p, d, p), E, "n_members");
    expect("noise_rows: m0 < 0", noise(-1, 8, 8, 0, 4, p, p, d, p), E, "m0=-1");
    expect("noise_rows: empty range", noise(0, 8, 8, 2, 2, p, p, d, p), FIVEEQ_OK, nullptr);
}

}  // namespace

int main() {
    family<double>("f64");
    family<float>("f32");
    // the deviate on the host: the bound the header documents, over a strip of members and counters
    double worst = 0.0;
    for (uint64_t M = 0; M < 4096; ++M)
        for (int t = -1; t < 64; ++t) worst = std::fmax(worst, std::fabs(fiveeq::noise_deviate(fiveeq::noise_member_key(7, M), t)));
    std::printf("max |z| over 4096 members x 65 counters: %.6f\n", worst);
    if (!(worst <= 6.0)) ++failures;
    std::printf(failures ? "%d FAILURES\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
