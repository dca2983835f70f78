"""An independent scalar statement of the sea-level rows' arithmetic (include/fiveeq.h, "SEA-LEVEL ROWS"): plain Python floats,
one member at a time, em1 handed in.  Shares no code with fiveeqscm_amd.sea_level; the tests hold the NumPy twin to it bit for
bit, and the twin is what the device rows are held to.  Also the closed forms for a constant T, evaluated with mpmath."""
import struct


def widen(value, f32):
    """The fp64 value of `value` as a row of the kernel precision holds it."""
    return struct.unpack("f", struct.pack("f", value))[0] if f32 else float(value)


def member_rows(T, kinds, tau, a, b, T0, cap, S0, em1, dt, heat=None, eta=None, f32=False):
    """One member of one scenario.  T: n_rows values; kinds: J strings "relax" / "rate"; tau, a, b, T0, cap, S0, em1: J floats
    each (em1[j] is read for relax components only); heat: n_rows floats with the float eta, or None.
    Returns (total [n_rows], comps [n_rows][J], S after the last row [J])."""
    J = len(kinds)
    S = [float(v) for v in S0]
    total, comps = [], []
    for t in range(len(T)):
        Tt = widen(T[t], f32)
        for j in range(J):
            x = Tt - float(T0[j])
            p = float(b[j]) * x
            c = float(a[j]) + p
            e = c * x
            if e > float(cap[j]):
                e = float(cap[j])
            if kinds[j] == "rate":
                w = float(dt) * e
            else:
                v = S[j] - e
                w = float(em1[j]) * v
            S[j] = S[j] + w
        acc = float(eta) * float(heat[t]) if heat is not None else 0.0
        for j in range(J):
            acc = acc + S[j]
        total.append(acc)
        comps.append(list(S))
    return total, comps, S


def rows_scalar(T, kinds, par, S0, em1, dt, heat=None, eta=None, f32=False):
    """Every member of every scenario: T [Sc][n_rows][n], par [5][J][n] (tau, a, b, T0, cap), S0 [Sc][J][n], em1 [J][n], heat like
    T, eta [n].  Returns nested lists total [Sc][n_rows][n], comps [Sc][n_rows][J][n], S_end [Sc][J][n]."""
    Sc, K, n = len(T), len(T[0]), len(T[0][0])
    J = len(kinds)
    total = [[[None] * n for _ in range(K)] for _ in range(Sc)]
    comps = [[[[None] * n for _ in range(J)] for _ in range(K)] for _ in range(Sc)]
    S_end = [[[None] * n for _ in range(J)] for _ in range(Sc)]
    for s in range(Sc):
        for m in range(n):
            col = lambda i: [par[i][j][m] for j in range(J)]                              # noqa: E731
            tot, cmp, S = member_rows([T[s][t][m] for t in range(K)], kinds, col(0), col(1), col(2), col(3), col(4),
                                      [S0[s][j][m] for j in range(J)], [em1[j][m] for j in range(J)], dt,
                                      None if heat is None else [heat[s][t][m] for t in range(K)],
                                      None if eta is None else eta[m], f32)
            for t in range(K):
                total[s][t][m] = tot[t]
                for j in range(J):
                    comps[s][t][j][m] = cmp[t][j]
            for j in range(J):
                S_end[s][j][m] = S[j]
    return total, comps, S_end


# ---- the closed-form case both accuracy tests share --------------------------------------------------------------------------
# 300 steps of constant T; component 0 relax, component 1 rate; members = tau in {2, 50, 3000} years x four parameter classes
# (plain; a cap that binds; T0 above T, so x < 0 and a falling level; a quadratic term with a start above equilibrium).
# CLOSED_FORM_MEASURED is the largest relative error |S - S_mp| / |S_mp| the NumPy twin with np.expm1 showed against the
# 50-digit closed form over every member, both components and the rows CLOSED_FORM_ROWS (measured by
# tests/test_sea_level_cpu.py::test_closed_form..., glibc's expm1); the assertion, on the CPU and on the device, is 4 times
# that: the margin covers an expm1 that differs by an ulp, it is not a value picked in advance.
CLOSED_FORM_STEPS = 300
CLOSED_FORM_ROWS = (0, 9, 99, 299)
CLOSED_FORM_TAUS = (2.0, 50.0, 3000.0)
CLOSED_FORM_MEASURED = 3.54e-15       # 3.531e-15 at row 300 of the rate component, member 3; the relax components: 7.4e-16
CLOSED_FORM_BOUND = 4 * CLOSED_FORM_MEASURED
CLOSED_FORM_KINDS = ("relax", "rate")


def closed_form_case():
    """(T [300][n], par [5][2][n], S0 [2][n], dt) as nested lists of floats, n = 12."""
    classes = [  # T, (a, b, T0, cap) of the relax component, the same of the rate component, S0 of both
        (2.3, (0.31, 0.0, 0.1, float("inf")), (0.0017, 0.0, 0.2, float("inf")), (0.05, 0.02)),
        (3.1, (0.42, 0.03, 0.0, 0.55), (0.0021, 0.0004, 0.0, 0.0031), (0.01, 0.0)),
        (0.4, (0.27, 0.05, 1.4, float("inf")), (0.0012, 0.0, 1.0, float("inf")), (-0.03, -0.01)),
        (1.7, (0.12, 0.08, -0.3, float("inf")), (0.0009, 0.0002, -0.2, float("inf")), (0.9, 0.11)),
    ]
    cols = [(tau, c) for tau in CLOSED_FORM_TAUS for c in classes]
    T = [[c[0] for _, c in cols] for _ in range(CLOSED_FORM_STEPS)]
    par = [[[tau for tau, _ in cols], [tau for tau, _ in cols]]]
    for i in range(4):
        par.append([[c[1][i] for _, c in cols], [c[2][i] for _, c in cols]])
    S0 = [[c[3][0] for _, c in cols], [c[3][1] for _, c in cols]]
    return T, par, S0, 1.0


def closed_form_worst(comps):
    """The largest relative error of comps [300][2][n] (indexable: lists or an array) against the 50-digit closed form over
    CLOSED_FORM_ROWS, with where it was met."""
    import mpmath
    T, par, S0, dt = closed_form_case()
    worst, where = 0.0, None
    for t in CLOSED_FORM_ROWS:
        for j, kind in enumerate(CLOSED_FORM_KINDS):
            for m in range(len(T[0])):
                want = closed_form(kind, T[0][m], par[0][j][m], par[1][j][m], par[2][j][m], par[3][j][m], par[4][j][m], S0[j][m], dt, t + 1)
                with mpmath.workdps(50):
                    err = float(abs((mpmath.mpf(float(comps[t][j][m])) - want) / want))
                if err > worst:
                    worst, where = err, (t, kind, m)
    return worst, where


def closed_form(kind, T, tau, a, b, T0, cap, S0, dt, n_steps, digits=50):
    """A component under constant T after n_steps steps, as an mpmath number at `digits` digits:
    relax  Seq + (S0 - Seq) exp(-n dt / tau);   rate  S0 + n dt Seq;   Seq = min((a + b x) x, cap), x = T - T0, from the
    fp64 inputs taken exactly."""
    import mpmath
    with mpmath.workdps(digits):
        x = mpmath.mpf(T) - mpmath.mpf(T0)
        seq = (mpmath.mpf(a) + mpmath.mpf(b) * x) * x
        if cap != float("inf") and seq > mpmath.mpf(cap):
            seq = mpmath.mpf(cap)
        if kind == "rate":
            return mpmath.mpf(S0) + n_steps * mpmath.mpf(dt) * seq
        return seq + (mpmath.mpf(S0) - seq) * mpmath.exp(-n_steps * mpmath.mpf(dt) / mpmath.mpf(tau))
