"""Synthetic RCP-like emissions and the shared per-step "drive" table.

The reference (stujen/fiveEqSCM @ v0) ships no emissions data (SURVEY.md
section 2, negative inventory); the deterministic series below are the ones
frozen in SURVEY.md section 8d.  They are shared by every ensemble member.
"""
import hashlib

import numpy as np

from ._capi import DRIVE_STRIDE, MAX_GAS

N_STEPS_DEFAULT = 750   # years 1765..2514, dt = 1 yr


def _sigma(x):
    return 1.0 / (1.0 + np.exp(-x))


def rcp_like_emissions(n_steps=N_STEPS_DEFAULT, n_gas=3):
    """[n_steps, n_gas] fp64.  Columns: CO2 (GtC/yr), CH4 (Mt CH4/yr), N2O (Mt N2O-N2/yr).

    CO2: 12 s((t-230)/25) (1 - 1.1 s((t-330)/20)), clipped at >= -1  (peak ~9.7 GtC/yr near
    step 282, -1 GtC/yr from ~step 400: an overshoot scenario);
    CH4: 300 s((t-200)/40) (1 - 0.5 s((t-330)/30));   N2O: 10 s((t-220)/50);   s = logistic.
    """
    if not 1 <= n_gas <= MAX_GAS:
        raise ValueError(f"n_gas={n_gas} outside 1..{MAX_GAS}")
    t = np.arange(n_steps, dtype=np.float64)
    co2 = np.maximum(12.0 * _sigma((t - 230.0) / 25.0) * (1.0 - 1.1 * _sigma((t - 330.0) / 20.0)), -1.0)
    ch4 = 300.0 * _sigma((t - 200.0) / 40.0) * (1.0 - 0.5 * _sigma((t - 330.0) / 30.0))
    n2o = 10.0 * _sigma((t - 220.0) / 50.0)
    return np.stack([co2, ch4, n2o][:n_gas], axis=1)


def emissions_sha256(E):
    return hashlib.sha256(np.ascontiguousarray(E, dtype=np.float64).tobytes()).hexdigest()


def concentration_mask(concentration_gases, n_gas):
    """The per-gas drive mask of a mixed run (include/fiveeq.h "MIXED DRIVE"): bit g set for every gas index in
    `concentration_gases` (a sequence of distinct integers in 0 .. n_gas - 1; empty: every gas emission-driven)."""
    try:
        gases = [int(g) for g in concentration_gases]
        exact = all(g == x for g, x in zip(gases, concentration_gases))
    except (TypeError, ValueError) as exc:
        raise ValueError(f"concentration_gases={concentration_gases!r}: want a sequence of gas indices") from exc
    if not exact or any(not 0 <= g < n_gas for g in gases):
        raise ValueError(f"concentration_gases={list(concentration_gases)!r}: want gas indices in 0..{n_gas - 1}")
    if len(set(gases)) != len(gases):
        raise ValueError(f"concentration_gases={gases!r}: a gas is named twice")
    return sum(1 << g for g in gases)


def make_drive(emissions, F_ext=None, dt=1.0, output_steps=None, concentration_driven=False, *, concentrations=None,
               concentration_gases=None):
    """emissions [n_steps, G] (or [n_steps]) -> drive [n_steps, 8] fp64 (include/fiveeq.h):
    cols 0..2 E_g, cols 3..5 cumulative emissions BEFORE the step, col 6 F_ext, col 7 the output
    row the step's C/T are stored at (-1: not stored).  output_steps=None stores every step at
    row t; otherwise the listed steps are stored at rows 0, 1, ... in increasing step order.
    concentration_driven=True: `emissions` holds target concentrations (end of step) for the
    inverse mode; cols 3..5 stay zero.
    THE PER-GAS FORM (concentration_gases= a sequence of gas indices, with concentrations= [n_steps, G]; the mixed drive):
    cols g and 3 + g of every other gas are built from `emissions` as for a forward run (col 3 + g the cumulative emissions
    before the step); col g of a gas in concentration_gases holds its target from `concentrations` and its col 3 + g is zero.
    The `emissions` column of a concentration-driven gas and the `concentrations` column of an emission-driven one are
    ignored (NaN allowed there); `emissions` may be None when every gas is named, `concentrations` when none is."""
    if concentration_gases is not None:
        if concentration_driven:
            raise ValueError("concentration_gases= is the per-gas form: leave concentration_driven False")
        given = [np.asarray(x, dtype=np.float64) for x in (emissions, concentrations) if x is not None]
        given = [x[:, None] if x.ndim == 1 else x for x in given]
        if not given or any(x.ndim != 2 or x.shape != given[0].shape for x in given):
            raise ValueError("emissions and concentrations: want two arrays of one shape [n_steps, G]")
        G = given[0].shape[1] if 1 <= given[0].shape[1] <= MAX_GAS else 0
        mask = concentration_mask(concentration_gases, G) if G else 0
        src = {False: emissions, True: concentrations}
        for conc in (False, True):
            if src[conc] is None and any(bool(mask >> g & 1) == conc for g in range(G)):
                raise ValueError(f"{'concentrations' if conc else 'emissions'} is None, but a gas is "
                                 f"{'concentration' if conc else 'emission'}-driven")
        E = np.zeros(given[0].shape)
        for g in range(G):
            x = np.asarray(src[bool(mask >> g & 1)], dtype=np.float64)
            E[:, g] = x if x.ndim == 1 else x[:, g]
        forward = [g for g in range(G) if not mask >> g & 1]     # the gases whose cols g, 3 + g are a forward run's
    else:
        forward = None
        if concentrations is not None:
            raise ValueError("concentrations= needs concentration_gases=")
        E = np.asarray(emissions, dtype=np.float64)
    if E.ndim == 1:
        E = E[:, None]
    if E.ndim != 2 or not 1 <= E.shape[1] <= MAX_GAS or E.shape[0] < 1:
        raise ValueError(f"emissions shape {E.shape}: want [n_steps>=1, 1..{MAX_GAS}]")
    if not np.all(np.isfinite(E)):
        raise ValueError("emissions contain non-finite values")
    n_steps, G = E.shape
    drive = np.zeros((n_steps, DRIVE_STRIDE), dtype=np.float64)
    drive[:, :G] = E
    if forward is not None:               # the per-gas form: the emission-driven gases' columns only
        drive[1:, [3 + g for g in forward]] = np.cumsum(E[:, forward] * dt, axis=0)[:-1]
    elif not concentration_driven:        # inverse mode: cumulative emissions are per-member state
        drive[1:, 3:3 + G] = np.cumsum(E * dt, axis=0)[:-1]
    if F_ext is not None:
        F_ext = np.asarray(F_ext, dtype=np.float64).reshape(-1)
        if F_ext.shape[0] != n_steps:
            raise ValueError(f"F_ext has {F_ext.shape[0]} steps, emissions {n_steps}")
        drive[:, 6] = F_ext
    if output_steps is None:
        drive[:, 7] = np.arange(n_steps)
    else:
        steps = np.unique(np.asarray(output_steps, dtype=np.int64).reshape(-1))
        if steps.size and (steps[0] < 0 or steps[-1] >= n_steps):
            raise ValueError(f"output_steps outside [0, {n_steps})")
        drive[:, 7] = -1.0
        drive[steps, 7] = np.arange(steps.size)
    return drive


def make_scenario_drive(emissions, F_ext=None, dt=1.0, output_steps=None):
    """The drive tables of S emission scenarios, stacked: emissions [S, n_steps, G] (or a sequence of S [n_steps, G]
    arrays) -> drive [S, n_steps, 8] fp64, scenario s being make_drive(emissions[s], F_ext[s], dt, output_steps) — each
    scenario's own cumulative-emission columns, ONE row map (column 7) for all.  F_ext: None, [n_steps] (shared) or
    [S, n_steps]."""
    try:
        E = np.asarray(emissions, dtype=np.float64)
    except ValueError as exc:
        raise ValueError("scenario emissions: every scenario needs the same [n_steps, G] shape") from exc
    if E.ndim != 3 or E.shape[0] < 1:
        raise ValueError(f"scenario emissions shape {E.shape}: want [S>=1, n_steps, G]")
    S, n_steps = E.shape[0], E.shape[1]
    if F_ext is None:
        F = [None] * S
    else:
        F = np.asarray(F_ext, dtype=np.float64)
        if F.ndim == 1 and F.shape[0] == n_steps:
            F = [F] * S
        elif F.shape != (S, n_steps):
            raise ValueError(f"F_ext shape {F.shape}: want [{n_steps}] or [{S}, {n_steps}]")
    return np.stack([make_drive(E[s], F[s], dt, output_steps) for s in range(S)])
