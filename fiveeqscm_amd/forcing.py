"""Per-member forcing uncertainty (round 8): external forcing categories that every member scales by its own factor.

The run carries a shared table X [n_steps, K] — the forcing of category k during step t (aerosol, other anthropogenic,
volcanic, solar, ...; K <= 4) — and every member G + K scale factors: sg_g on the forcing of gas g, sx_k on category k
(include/fiveeq.h, "FORCING SCALES").  The total forcing of a step is

    F = F_ext(t);   F = fma(sx_k, X[t, k], F), k = 0 .. K-1;   F = fma(sg_g, F_g, F), g = 0 .. G-1

so unit scales with no category (or an all-zero table) are the plain run bit for bit.

    fx = ExternalForcings.from_csv("forcing.csv", ("AEROSOL", "VOLCANIC"), run_years)
    s = params.sample_forcing_scales(base, n_total, lo, hi, ranges=[(1, 1)] * G + [(0.3, 2.0), (0.5, 1.5)])
    p["f_scale"], p["fx_scale"] = s[:G], s[G:]
    eng = EnsembleEngine(p, N, E, forcing=fx, observations=obs)

An engine with the scenario axis takes a ScenarioForcings: one table per scenario, the scale rows shared by the scenarios.

    proj = EnsembleEngine(p, N, E_s, forcing=ScenarioForcings([fx_low, fx_mid, fx_high]), R0=eng.R, S0=eng.S)
"""
import hashlib

import numpy as np

from . import _capi
from .scenario import _read_year_table


class ExternalForcings:
    """The shared table of external forcing categories, X [n_steps, K] fp64 with 0 <= K <= 4, and a name per category.
    Validated and read-only; `sha256` covers the table's shape, its bytes and the names."""

    def __init__(self, table, names=None):
        t = np.array(table, dtype=np.float64, order="C")
        if t.ndim == 1:
            t = t.reshape(-1, 1)
        if t.ndim != 2 or t.shape[0] < 1:
            raise ValueError(f"forcing table: shape {t.shape}, want [n_steps, K]")
        if t.shape[1] > _capi.MAX_FEXT:
            raise ValueError(f"forcing table: {t.shape[1]} categories, at most {_capi.MAX_FEXT}")
        if not np.isfinite(t).all():
            raise ValueError("forcing table: non-finite entries")
        names = [f"fx{k}" for k in range(t.shape[1])] if names is None else [str(n) for n in names]
        if len(names) != t.shape[1]:
            raise ValueError(f"forcing table: {len(names)} names for {t.shape[1]} categories")
        if len(set(names)) != len(names):
            raise ValueError(f"forcing table: category names {names} repeat")
        self.table = t
        self.table.setflags(write=False)
        self.names = tuple(names)
        h = hashlib.sha256(repr((t.shape, self.names)).encode())
        h.update(t.tobytes())
        self.sha256 = h.hexdigest()

    @property
    def n_steps(self):
        return int(self.table.shape[0])

    @property
    def n_categories(self):
        return int(self.table.shape[1])

    def padded(self):
        """[n_steps, 4] fp64: the table as the C ABI takes it (columns past K zero; the kernels do not read them)."""
        out = np.zeros((self.n_steps, _capi.MAX_FEXT), dtype=np.float64)
        out[:, :self.n_categories] = self.table
        return out

    @classmethod
    def from_csv(cls, path, names, run_years):
        """Read a CSV with a year column and named forcing columns (free-text lines, a row of column names holding every
        requested name, then one row per year: the row layout of scenario.read_emissions_csv) and match it to the run's
        steps by year: X[t, k] is column names[k] at run_years[t].  Every run year must be in the file."""
        names = [str(n) for n in names]
        if not names:
            raise ValueError("from_csv: no category names")
        header, table = _read_year_table(path, lambda cells: all(n in cells for n in names),
                                         f"a row naming the columns {names}")
        ry = np.asarray(run_years, dtype=np.float64).reshape(-1)
        years = table[:, 0]
        idx = np.searchsorted(years, ry)
        ok = (idx < years.size) & (years[np.minimum(idx, years.size - 1)] == ry)
        if not ok.all():
            raise ValueError(f"{path}: run years {ry[~ok][:5].tolist()} are not in the file")
        cols = np.stack([table[idx, header.index(n)] for n in names], axis=1)
        if not np.isfinite(cols).all():
            raise ValueError(f"{path}: missing values in the forcing columns")
        return cls(cols, names)


class ScenarioForcings:
    """One table of external forcing categories PER EMISSION SCENARIO, X [S, n_steps, K] fp64 with 0 <= K <= 4, and one set of
    category names: what an engine with the scenario axis takes as forcing= (aerosol and other external forcings differ from
    one scenario to the next; the members' scale rows are shared by the scenarios).  Validated and read-only like
    ExternalForcings; `sha256` covers the shape, every table byte and the names.  Built from an array, from a sequence of
    ExternalForcings with equal names and steps, with `shared(fx, S)` (one table under every scenario) or `from_csvs`."""

    def __init__(self, tables, names=None):
        if isinstance(tables, (list, tuple)) and len(tables) and all(isinstance(x, ExternalForcings) for x in tables):
            first = tables[0]
            for i, x in enumerate(tables):
                if x.names != first.names:
                    raise ValueError(f"scenario forcings: scenario {i} has categories {x.names}, scenario 0 {first.names}")
                if x.n_steps != first.n_steps:
                    raise ValueError(f"scenario forcings: scenario {i} has {x.n_steps} steps, scenario 0 {first.n_steps}")
            if names is not None and tuple(str(n) for n in names) != first.names:
                raise ValueError(f"scenario forcings: names {tuple(names)} are not the tables' {first.names}")
            names = first.names
            t = np.stack([x.table for x in tables])
        else:
            try:
                t = np.array(tables, dtype=np.float64, order="C")
            except ValueError as exc:
                raise ValueError(f"scenario forcings: the tables do not stack to [S, n_steps, K] ({exc})") from None
        if t.ndim != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"scenario forcings: shape {t.shape}, want [S, n_steps, K]")
        if t.shape[2] > _capi.MAX_FEXT:
            raise ValueError(f"scenario forcings: {t.shape[2]} categories, at most {_capi.MAX_FEXT}")
        if not np.isfinite(t).all():
            raise ValueError("scenario forcings: non-finite entries")
        names = [f"fx{k}" for k in range(t.shape[2])] if names is None else [str(n) for n in names]
        if len(names) != t.shape[2]:
            raise ValueError(f"scenario forcings: {len(names)} names for {t.shape[2]} categories")
        if len(set(names)) != len(names):
            raise ValueError(f"scenario forcings: category names {names} repeat")
        self.table = np.ascontiguousarray(t)
        self.table.setflags(write=False)
        self.names = tuple(names)
        h = hashlib.sha256(repr((t.shape, self.names)).encode())
        h.update(self.table.tobytes())
        self.sha256 = h.hexdigest()

    @property
    def n_scenarios(self):
        return int(self.table.shape[0])

    @property
    def n_steps(self):
        return int(self.table.shape[1])

    @property
    def n_categories(self):
        return int(self.table.shape[2])

    def scenario(self, s):
        """Scenario s's table as an ExternalForcings: what a single-scenario forcing= engine on that scenario takes."""
        return ExternalForcings(self.table[int(s)], self.names)

    def padded(self):
        """[S, n_steps, 4] fp64: the tables as the C ABI takes them (columns past K zero; the kernels do not read them)."""
        out = np.zeros((self.n_scenarios, self.n_steps, _capi.MAX_FEXT), dtype=np.float64)
        out[:, :, :self.n_categories] = self.table
        return out

    @classmethod
    def shared(cls, fx, n_scenarios):
        """The one table `fx` (ExternalForcings) under each of n_scenarios scenarios."""
        S = int(n_scenarios)
        if S < 1:
            raise ValueError(f"scenario forcings: n_scenarios={n_scenarios} must be >= 1")
        return cls([fx] * S)

    @classmethod
    def from_csvs(cls, paths, names, run_years):
        """One CSV per scenario (ExternalForcings.from_csv each: the same category names and run years in every file)."""
        paths = list(paths)
        if not paths:
            raise ValueError("from_csvs: no scenario files")
        return cls([ExternalForcings.from_csv(p, names, run_years) for p in paths])


# ------------------------------------------------------------------------------------
# Per-member AR(1) internal variability: rows [n_steps, N] for EnsembleEngine(member_forcing=...).  xi_t = phi xi_{t-1} + s z_t
# with s = sigma sqrt(1 - phi^2) and z_t(M) a counter-based deviate that is a pure function of (seed, M, t), computed in
# integer arithmetic (include/fiveeq.h, "AR(1) NOISE ROWS"; csrc/fiveeq_noise.hpp): a rank computes exactly its shard — on its
# GPU through fiveeq_noise_rows_*, or on the host with the NumPy twin below, bit for bit the same numbers — and the rows do
# not depend on the world size or on how the steps are cut into calls.
# ------------------------------------------------------------------------------------
NOISE_SEED = 20261020


def _noise_deviates(seed, members, steps):
    """z [len(steps), len(members)] fp64: the deviate of member M at counter t (t >= -1), the key construction of
    csrc/fiveeq_noise.hpp (noise_member_key, noise_key, noise_deviate) in wrapping uint64 arithmetic."""
    from .params import _mix64
    M = np.asarray(members, dtype=np.uint64).reshape(1, -1)
    t = np.asarray(steps, dtype=np.int64).reshape(-1, 1)
    if t.size and t.min() < -1:
        raise ValueError("noise deviates: counters start at t = -1")
    with np.errstate(over="ignore"):
        mk = _mix64(np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (M + np.uint64(1)))
        total = np.zeros((t.shape[0], M.shape[1]), dtype=np.uint64)
        for j in range(6):
            counter = (t + 1).astype(np.uint64) * np.uint64(6) + np.uint64(j + 1)
            word = _mix64(mk ^ (np.uint64(0xD1342543DE82EF95) * counter))
            total += (word >> np.uint64(32)) + (word & np.uint64(0xFFFFFFFF))
    return (total.astype(np.int64) - np.int64(6 * 0xFFFFFFFF)).astype(np.float64) * 2.0 ** -32


def ar1_noise_steps_host(seed, members, t_begin, t_end, phi, s, xi_state, dtype=np.float64):
    """The twin of ONE fiveeq_noise_rows_* call: steps [t_begin, t_end) of `members` (global indices) from xi_state (fp64, not
    modified).  phi and s are taken in `dtype` (the kernel precision) and widened.  Returns (rows [t_end - t_begin, n] in
    dtype, xi_state after); [-1, 0) is the start call, which returns no rows."""
    members = np.asarray(members)
    ph = np.asarray(phi, dtype=dtype).astype(np.float64)
    sm = np.asarray(s, dtype=dtype).astype(np.float64)
    xi = np.array(xi_state, dtype=np.float64, copy=True)
    start = t_begin == -1
    if t_begin < -1 or t_end < t_begin or (start and t_end != 0):
        raise ValueError(f"step range [{t_begin},{t_end}): want 0 <= t_begin <= t_end, or [-1,0) for the stationary start")
    z = _noise_deviates(seed, members, np.arange(t_begin, t_end))
    rows = np.empty((0 if start else t_end - t_begin, members.size), dtype=dtype)
    for i in range(t_end - t_begin):
        w = sm * z[i]
        xi = ph * xi + w
        if not start:
            rows[i] = xi.astype(dtype)
    return rows, xi


def _member_rows(x, n_total, lo, hi, name):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 0:
        return np.full(hi - lo, float(x))
    if x.shape == (n_total,):
        return x[lo:hi].copy()
    if x.shape == (hi - lo,):
        return x.copy()
    raise ValueError(f"{name}: a scalar, or a row of the {n_total} members of the design or of the {hi - lo} of the shard")


def _ar1_setup(n_total, n_steps, sigma, phi, lo, hi):
    hi = n_total if hi is None else hi
    if not 0 <= lo <= hi <= n_total:
        raise ValueError(f"members [{lo}, {hi}) outside [0, {n_total})")
    if n_steps < 0:
        raise ValueError(f"n_steps={n_steps} must be >= 0")
    sg, ph = _member_rows(sigma, n_total, lo, hi, "sigma"), _member_rows(phi, n_total, lo, hi, "phi")
    if not (np.isfinite(sg).all() and (sg >= 0).all()):
        raise ValueError("sigma: want finite values >= 0")
    if not (np.abs(ph) < 1).all():
        raise ValueError("phi: want |phi| < 1 (a stationary AR(1) process)")
    return hi, sg, ph, sg * np.sqrt(1.0 - ph * ph)           # s = sigma sqrt(1 - phi^2), in fp64 on the host


def ar1_noise_rows_host(n_total, n_steps, sigma, phi, lo=0, hi=None, seed=NOISE_SEED, dtype=np.float64):
    """[n_steps, hi - lo]: the rows of ar1_noise_rows computed on the host with NumPy, bit for bit (dtype np.float64 or
    np.float32)."""
    hi, sg, ph, s = _ar1_setup(n_total, n_steps, sigma, phi, lo, hi)
    members = np.arange(lo, hi)
    _, xi = ar1_noise_steps_host(seed, members, -1, 0, ph, sg, np.zeros(hi - lo), dtype)     # xi_{-1} = sigma z_{-1}
    return ar1_noise_steps_host(seed, members, 0, n_steps, ph, s, xi, dtype)[0]


def ar1_noise_rows(n_total, n_steps, sigma, phi, lo=0, hi=None, seed=NOISE_SEED, device=None, dtype=None):
    """[n_steps, hi - lo] on `device`: per-member AR(1) noise for members [lo, hi) of an n_total-member ensemble, stationary
    with standard deviation sigma and lag-1 autocorrelation phi (scalars, or per-member rows over the design or the shard;
    W m-2 when the rows go into EnsembleEngine(member_forcing=...)).  The start is the draw at counter t = -1 times sigma.
    One HIP pass (fiveeq_noise_rows_*), two calls: the start, then the steps.  dtype: torch.float64 (default) or
    torch.float32 — the recursion runs in fp64 either way and fp32 rows are rounded once.  Memory: n_steps (hi - lo) w bytes."""
    import torch

    from ._rowargs import call, ptr
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    hi, sg, ph, s = _ar1_setup(n_total, n_steps, sigma, phi, lo, hi)
    dev = torch.device("cuda" if device is None else device)
    n = hi - lo
    rows = torch.empty((n_steps, n), dtype=dtype, device=dev)
    if n == 0 or n_steps == 0:
        return rows
    up = lambda a: torch.from_numpy(a).to(dev, dtype)                               # noqa: E731
    ph_d, s_d, sg_d = up(ph), up(s), up(sg)
    xi = torch.zeros(n, dtype=torch.float64, device=dev)
    lib = _capi.load()
    call(lib, _capi, "fiveeq_noise_rows", dtype, dev, int(seed), int(lo), n, n, -1, 0, ptr(ph_d), ptr(sg_d), ptr(xi), None)
    call(lib, _capi, "fiveeq_noise_rows", dtype, dev, int(seed), int(lo), n, n, 0, int(n_steps), ptr(ph_d), ptr(s_d), ptr(xi),
         ptr(rows))
    return rows
