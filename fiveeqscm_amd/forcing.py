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
