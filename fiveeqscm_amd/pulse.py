"""Per-member emission metrics — AGWP, AGTP, iAGTP, the airborne fraction of a pulse and the ratios GWP and GTP — from PULSE
EXPERIMENTS: one scenario engine runs "baseline" and "baseline + a pulse of gas g" for the same members, and ONE streaming HIP
pass over its stored rows (include/fiveeq.h, "PULSE RESPONSE"; csrc/fiveeq_pulse.hpp) forms, per member, the differences of
forcing, warming and concentration between each pulse scenario and the base and sums them to the time horizons:

    exp = pulse_experiment(E, t0=250, pulses=[(0, 100.0), (1, 500.0), (2, 30.0)], n_rows=500)
    eng = EnsembleEngine(params, N, exp.emissions, scenario_names=exp.scenario_names, output_steps=exp.output_steps)
    eng.run()
    res = eng.pulse_response(exp, horizons=(20, 100, 500))
    res.gwp(0)[1, 1]                                   # [N] device row: GWP-100 of CH4 against CO2, per member

    I_F, I_T, I_C [P, H, N]   sums over the first n_h rows of dF, dT, dC (pulse scenario minus base), fp64
    dT, dC        [P, H, N]   the differences in the horizon's last row

The forcing of each scenario is recomputed from its stored C rows by the device function the stepping kernels call, so dF is
the difference of the two runs' own forcings, bit for bit.  Rows [p, h] of every result are [N] device rows: they go into
distributed.gather_summary / gather_weighted_summary as one-row blocks (`x[p, h:h + 1]`), into joint.sensitivity and
EnsembleEngine.drivers as y.  Device rows only: there is no CPU path (_pulse_host.py is the NumPy twin of the tests).
"""
import ctypes
from dataclasses import dataclass

import numpy as np


@dataclass
class PulseExperiment:
    """What pulse_experiment returns.  emissions [1 + P, n_steps, G]: the baseline, then the baseline with pulse p; scenario_names
    ("base", "pulse:<gas>", ...); output_steps = range(t0, t0 + n_rows): the rows a pulse response needs stored; pulses: the
    table ((gas, size), ...), pulse p being scenario 1 + p; t0: the step that carries the pulses."""
    emissions: np.ndarray
    scenario_names: tuple
    output_steps: range
    pulses: tuple
    t0: int


def pulse_experiment(emissions, t0, pulses, n_rows, dt=1.0):
    """The emission scenarios of a pulse experiment.  emissions [n_steps, G]: the baseline (rates per year).  pulses: a sequence
    of (gas, size), `size` in that gas's emission units, added as the RATE size / dt in step t0 of that gas only.  n_rows: the
    rows to store from t0 on (the longest horizon).  Pass `.emissions`, `.scenario_names` and `.output_steps` to
    EnsembleEngine(...), and the experiment to EnsembleEngine.pulse_response.  ValueError unless 0 <= t0, t0 + n_rows <= n_steps,
    the sizes are finite and not zero, and the gases are distinct gases of the baseline."""
    from . import _capi
    E = np.asarray(emissions, dtype=np.float64)
    if E.ndim != 2:
        raise ValueError("emissions: want a [n_steps, G] baseline")
    n_steps, G = E.shape
    t0, n_rows, dt = int(t0), int(n_rows), float(dt)
    if not dt > 0.0:
        raise ValueError("dt must be positive")
    if t0 < 0 or n_rows < 1 or t0 + n_rows > n_steps:
        raise ValueError(f"t0={t0}, n_rows={n_rows}: want 0 <= t0, n_rows >= 1 and t0 + n_rows <= n_steps = {n_steps}")
    table = tuple((int(g), float(size)) for g, size in pulses)
    if not 1 <= len(table) <= _capi.MAX_PULSES:
        raise ValueError(f"pulses: {len(table)} pulses; want 1..{_capi.MAX_PULSES}")
    gases = [g for g, _ in table]
    if len(set(gases)) != len(gases):
        raise ValueError(f"pulses: gases {gases} are not distinct")
    for g, size in table:
        if not 0 <= g < G:
            raise ValueError(f"pulses: gas {g} outside the baseline's gases 0..{G - 1}")
        if not np.isfinite(size) or size == 0.0:
            raise ValueError(f"pulses: size {size} of gas {g}; want a finite size that is not zero")
    out = np.repeat(E[None], 1 + len(table), axis=0)
    for p, (g, size) in enumerate(table):
        out[1 + p, t0, g] += size / dt
    return PulseExperiment(out, ("base",) + tuple(f"pulse:{g}" for g in gases), range(t0, t0 + n_rows), table, t0)


@dataclass
class PulseState:
    """The carried state of a pulse response whose rows come in several calls: the running sums [3, P, N] fp64 after the rows
    given so far, their number, and the horizon outputs written so far."""
    sums: object
    rows: int
    out: object


@dataclass
class PulseResponse:
    """What pulse_response returns.  I_F, I_T, I_C, dT, dC [P, H, N]: fp64 device tensors, NaN where the rows given so far do not
    reach the horizon.  state: PulseState, for a later call over LATER rows.  horizons [H] row counts; pulses ((scenario, gas),
    ...); sizes [P] in each gas's emission units; emis2conc [P] of each pulsed gas; dt.
    The metrics are one fp64 torch operation per element and factor: agwp = dt * I_F / size (W yr m-2 per emission unit), agtp =
    dT / size (K per unit), iagtp = dt * I_T / size (K yr per unit), irf = dC / (size * emis2conc[g]) (the airborne fraction of
    the pulse), gwp / gtp the ratios of agwp / agtp to those of a reference pulse."""
    I_F: object
    I_T: object
    I_C: object
    dT: object
    dC: object
    state: PulseState
    horizons: tuple
    pulses: tuple
    sizes: tuple
    emis2conc: tuple
    dt: float

    def _per(self, values):
        import torch
        return torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.I_F.device).reshape(-1, 1, 1)

    def agwp(self):
        return self.dt * self.I_F / self._per(self.sizes)

    def agtp(self):
        return self.dT / self._per(self.sizes)

    def iagtp(self):
        return self.dt * self.I_T / self._per(self.sizes)

    def irf(self):
        return self.dC / self._per(s * c for s, c in zip(self.sizes, self.emis2conc))

    def _index(self, reference):
        gases = [g for _, g in self.pulses]
        if reference not in gases:
            raise ValueError(f"reference: no pulse of gas {reference!r}; the pulses are of gases {gases}")
        return gases.index(reference)

    def _ratio(self, x, reference, mass_kg):
        r = self._index(reference)
        if mass_kg is not None:
            if len(mass_kg) != len(self.pulses):
                raise ValueError(f"mass_kg: {len(mass_kg)} masses for {len(self.pulses)} pulses")
            x = x / self._per(mass_kg)
        return x / x[r:r + 1]

    def gwp(self, reference, mass_kg=None):
        """agwp() of every pulse over agwp() of the pulse of gas `reference` [P, H, N]: per emission unit of each gas, or, with
        mass_kg [P] (the kilograms ONE emission unit of each pulse's gas weighs), per kilogram: (agwp / mass_kg) / (agwp /
        mass_kg)[reference]."""
        return self._ratio(self.agwp(), reference, mass_kg)

    def gtp(self, reference, mass_kg=None):
        """The same ratio of agtp()."""
        return self._ratio(self.agtp(), reference, mass_kg)


def pulse_response(C_rows, T_rows, steps, params, *, q=None, F_ext, dt, base, pulses, horizons, fscale=None, X=None, state=None):
    """The response to emission pulses from the STORED rows of a scenario engine — one streaming HIP pass.
    C_rows [S, n_rows, G, N], T_rows [S, n_rows, N]: fp32 / fp64 rows ON THE GPU (engine.C, engine.T, or row / member slices of
    them), read in place whenever the member stride is 1, copied otherwise.  steps [n_rows]: the model step each row holds —
    CONSECUTIVE steps, the first of them the step that carries the pulses (ValueError otherwise, naming the first gap).  params:
    the parameter dict of the run.  q is not read (the pass forms no imbalance); it is accepted so that the call reads like
    diagnose.forcing_rows.  F_ext: the scenarios' drive tables [S, n_steps, 8] on the device in the rows' precision
    (engine.drive), or the external forcing as a host array [n_steps] (shared) or [S, n_steps].  dt: the run's step.  base: the
    base scenario.  pulses: a sequence of (scenario, gas, size), 1..3 of them, no scenario the base; size in the gas's emission
    units.  horizons: 1..8 strictly increasing ROW COUNTS, counted from the first row of the experiment.  fscale [G + K, N]
    device rows and X (a ScenarioForcings, a host table [S, n_steps, K], or engine.fext, the device table [S, n_steps, 4]): the
    forcing scales of a forcing= run; both None for a plain run.  state: the `.state` of an earlier call over EARLIER rows of the
    same experiment (same pulses and horizons): the result is that of one call over all the rows; it is not written into.
    THE SUM is the rectangle rule over END-OF-STEP values — agwp(n) = dt * sum of dF over the first n rows — the convention of
    the heat uptake H of diagnose.forcing_rows.  PRECISION: the differences are formed in fp64 from the rows as stored; fp32
    rows give fp32's resolution of a small difference of large forcings (an ulp of a 3 W m-2 forcing is 2.4e-7 W m-2), so fp64
    is the intended precision for metrics.
    TypeError for host rows: there is no CPU path.  Runs on the current stream; reads its inputs, allocates its results.
    Returns PulseResponse."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, drive_table, forcing_tables, model_steps, ptr, steps_i32, steps_in_tables, walk_in_place
    from .diagnose import check_consecutive
    from .forcing import ScenarioForcings
    from .params import make_model
    if not isinstance(C_rows, torch.Tensor) or C_rows.dim() != 4:
        raise ValueError("C_rows: want a tensor [S, n_rows, G, N]")
    if not C_rows.is_cuda or C_rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"C_rows must be fp32 / fp64 rows on a GPU (got {C_rows.dtype} on {C_rows.device}): the pulse response runs "
                        "through the HIP kernel and has no CPU fallback")
    S, K, G, N = C_rows.shape
    dev, dtp = C_rows.device, C_rows.dtype
    model = make_model(params, dt)
    if int(model.n_gas) != G:
        raise ValueError(f"C_rows hold {G} gases, params {int(model.n_gas)}")
    if N < 1:
        raise ValueError("C_rows: no members")
    if S < 2:
        raise ValueError("C_rows: a pulse response needs the base scenario and at least one pulse scenario")
    st = model_steps(steps, K, increasing=False)
    check_consecutive(st, "the pulse response")
    T_rows = dev_rows(T_rows, (S, K, N), "T_rows", dtp, dev)
    # the pulses and the horizons
    table = tuple((int(s), int(g), float(size)) for s, g, size in pulses)
    if not 1 <= len(table) <= _capi.MAX_PULSES:
        raise ValueError(f"pulses: {len(table)} pulses; want 1..{_capi.MAX_PULSES}")
    base = int(base)
    if not 0 <= base < S:
        raise ValueError(f"base: scenario {base} outside 0..{S - 1}")
    for s, g, size in table:
        if not 0 <= s < S or s == base:
            raise ValueError(f"pulses: scenario {s}; want a scenario 0..{S - 1} other than the base {base}")
        if not 0 <= g < G:
            raise ValueError(f"pulses: gas {g} outside 0..{G - 1}")
        if not np.isfinite(size) or size == 0.0:
            raise ValueError(f"pulses: size {size}; want a finite size that is not zero")
    hz = tuple(int(h) for h in horizons)
    if not 1 <= len(hz) <= _capi.MAX_HORIZONS or hz[0] < 1 or any(b <= a for a, b in zip(hz, hz[1:])):
        raise ValueError(f"horizons: {hz}; want 1..{_capi.MAX_HORIZONS} strictly increasing row counts >= 1")
    P, H = len(table), len(hz)

    # the shared tables, one per scenario: F_ext as drive tables, X padded to the C ABI's four columns
    drive = drive_table(F_ext, (S,), "F_ext (the scenarios' drive tables)", dtp, dev)
    n_steps = int(drive.shape[1])
    steps_in_tables(st, n_steps)

    def host_table(X):
        fx = X if isinstance(X, ScenarioForcings) else ScenarioForcings(np.asarray(X, dtype=np.float64))
        if fx.n_scenarios != S or fx.n_steps != n_steps:
            raise ValueError(f"X: tables of {fx.n_scenarios} scenarios x {fx.n_steps} steps; the rows hold {S} x {n_steps}")
        return fx

    n_fext, fext, fscale = forcing_tables(
        fscale, X, (S,), G, N, n_steps, dtp, dev, x_name="X (the scenarios' device tables)", host_table=host_table,
        together="fscale and X come together: the scale rows and the category tables of a forcing= run")
    ld = N
    if fscale is not None:
        fscale, (ld,) = walk_in_place(fscale, N, always=(0,))      # the carried sums take ld from one row of scales as from several
    x, (c_scen, c_row, c_gas) = walk_in_place(C_rows, N, always=(0,))
    tr, (t_scen, t_row) = walk_in_place(T_rows, N, always=(0,))
    # every output row starts 16-byte aligned; the carried sums are laid out with the scales' row stride
    ld_out = (N + 1) // 2 * 2
    row0 = 0
    if state is None:
        out = torch.full((5, P, H, ld_out), float("nan"), dtype=torch.float64, device=dev)[..., :N]
        io = torch.zeros((3, P, ld), dtype=torch.float64, device=dev)[..., :N]
    else:
        if not isinstance(state, PulseState):
            raise ValueError("state: want the .state of an earlier pulse_response")
        row0 = int(state.rows)
        out = torch.empty((5, P, H, ld_out), dtype=torch.float64, device=dev)[..., :N]
        out.copy_(dev_rows(state.out, (5, P, H, N), "state.out", torch.float64, dev))
        io = torch.empty((3, P, ld), dtype=torch.float64, device=dev)[..., :N]
        io.copy_(dev_rows(state.sums, (3, P, N), "state.sums", torch.float64, dev))
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)                                  # noqa: E731
    st32 = steps_i32(st, dev)
    call(_capi.load(), _capi, "fiveeq_pulse_response", dtp, dev, ctypes.byref(model), S, K, N, ld, ptr(x) if K else None, c_scen,
         c_row, c_gas, ptr(tr) if K else None, t_scen, t_row, ptr(st32) if K else None, ptr(drive), n_steps, ptr(fscale), n_fext,
         ptr(fext), base, P, i32([s for s, _, _ in table]), i32([g for _, g, _ in table]), H, i32(hz), row0, ptr(out), ld_out, ptr(io))
    c = np.asarray(params["emis2conc"], dtype=np.float64).reshape(G)
    return PulseResponse(out[0], out[1], out[2], out[3], out[4], PulseState(io, row0 + K, out), hz,
                         tuple((s, g) for s, g, _ in table), tuple(size for _, _, size in table),
                         tuple(float(c[g]) for _, g, _ in table), float(dt))
