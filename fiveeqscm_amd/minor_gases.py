"""Constant-lifetime minor gases (HFCs, PFCs, SF6, ...) as a shared forcing series.

The reference's one function models exactly such a species: a reservoir that decays with a fixed
lifetime, `emissions[0] * exp(-time)` (U_FaIR/concentrations.py:4-5).  In the five-equation
framework these gases are the special case of one pool with no state dependence (rC = rT = ra = 0,
alpha = 1): linear, and — because their emissions and parameters are shared by every ensemble member
— identical for all members.  They therefore need no per-member state on the GPU at all: their
concentrations are advanced once on the host with the same exact-step formula the kernels use,
    R <- R + expm1(-dt/tau) * (R - tau * c * E),     C = C0 + R,
and their summed forcing  sum_k eff_k * (C_k - C0_k)  enters the ensemble run as `F_ext`.
"""
import numpy as np


def step_minor_gases(emissions, lifetime, emis2conc, rad_eff, C0=0.0, R0=0.0, dt=1.0):
    """emissions [n_steps, K] (emission units / yr); lifetime [K] yr; emis2conc [K] concentration units per
    emission unit; rad_eff [K] W m^-2 per concentration unit; C0, R0 scalars or [K].
    Returns (conc [n_steps, K] at the END of each step, forcing [n_steps] = sum_k rad_eff_k (C_k - C0_k))."""
    E = np.asarray(emissions, dtype=np.float64)
    if E.ndim == 1:
        E = E[:, None]
    n_steps, K = E.shape
    tau = np.broadcast_to(np.asarray(lifetime, dtype=np.float64), (K,))
    c = np.broadcast_to(np.asarray(emis2conc, dtype=np.float64), (K,))
    eff = np.broadcast_to(np.asarray(rad_eff, dtype=np.float64), (K,))
    C0 = np.broadcast_to(np.asarray(C0, dtype=np.float64), (K,))
    if np.any(tau <= 0) or not np.all(np.isfinite(E)):
        raise ValueError("lifetimes must be > 0 and emissions finite")
    em1 = np.expm1(-dt / tau)
    R = np.array(np.broadcast_to(np.asarray(R0, dtype=np.float64), (K,)), dtype=np.float64)
    conc = np.empty((n_steps, K))
    for t in range(n_steps):
        R = R + em1 * (R - tau * c * E[t])
        conc[t] = C0 + R
    return conc, (conc - C0) @ eff


# ------------------------------------------------------------------------------------
# Per-member minor-gas forcing rows: the same step with each member's OWN lifetime and radiative efficiency, as rows
# [n_steps, N] for EnsembleEngine(member_forcing=...).  One HIP pass (fiveeq_minor_rows_*, csrc/fiveeq_minor.hpp; the arithmetic
# is stated in include/fiveeq.h, "MINOR-GAS FORCING ROWS") over at most 8 species per call; more species go in consecutive
# groups of 8, each later group accumulating onto the rows.  A rank computes exactly its shard [lo, hi), and the rows do not
# depend on the world size or on how the steps are cut into calls (R0= / .R carry the state).
# ------------------------------------------------------------------------------------
MINOR_MAX = 8                      # FIVEEQ_MINOR_MAX: species per call of fiveeq_minor_rows_*


class MinorGasRows:
    """What minor_gas_rows / minor_gas_rows_host return: `rows` [n_steps, n] (the summed forcing, W m-2), `R` [K, n] fp64 (each
    species' concentration above its baseline after the last step: R0= of the call that continues the steps) and `species`
    (K, the species summed into the rows)."""

    def __init__(self, rows, R, species):
        self.rows, self.R, self.species = rows, R, species


def _species_rows(x, K, n_total, lo, hi, name):
    """x as fp64 [K, hi - lo]: a value per species [K] (a scalar for K = 1), or per-member rows [K, n_total] (sliced to the shard)
    or [K, hi - lo]."""
    x = np.asarray(x, dtype=np.float64)
    n = hi - lo
    if x.ndim == 0 and K == 1:
        x = x.reshape(1)
    if x.shape == (K,):
        return np.repeat(x[:, None], n, axis=1)
    if x.shape == (K, n_total):
        return np.array(x[:, lo:hi], order="C")              # a copy: R0 is advanced in place, the caller's is not
    if x.shape == (K, n):
        return x.copy()
    raise ValueError(f"{name}: want [{K}] (a value per species), or rows [{K}, {n_total}] over the design or [{K}, {n}] over the shard")


def _minor_setup(emissions, lifetime, emis2conc, rad_eff, n_total, lo, hi, R0, dt, dtype):
    """The checked host arguments (E [n_steps, K], tau, eff, R [K, n] fp64, c [K], hi) of both forms."""
    E = np.asarray(emissions, dtype=np.float64)
    if E.ndim == 1:
        E = E[:, None]
    if E.ndim != 2 or E.shape[1] < 1:
        raise ValueError("emissions: want [n_steps, K] with K >= 1 species")
    n_steps, K = E.shape
    hi = n_total if hi is None else hi
    if not 0 <= lo <= hi <= n_total:
        raise ValueError(f"members [{lo}, {hi}) outside [0, {n_total})")
    if not np.isfinite(E).all():
        raise ValueError("emissions: want finite values")
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"dt={dt} must be finite and > 0")
    tau = _species_rows(lifetime, K, n_total, lo, hi, "lifetime")
    tq = tau.astype(dtype)                                  # as the kernel reads them
    if not (np.isfinite(tau).all() and (tau > 0).all() and np.isfinite(tq).all() and (tq > 0).all()):
        raise ValueError(f"lifetime: want finite values > 0 (in {np.dtype(dtype)} too)")
    eff = _species_rows(rad_eff, K, n_total, lo, hi, "rad_eff")
    c = np.asarray(emis2conc, dtype=np.float64)
    c = np.array(np.broadcast_to(c, (K,)) if c.ndim == 0 else c, dtype=np.float64)
    if c.shape != (K,) or not np.isfinite(c).all():
        raise ValueError(f"emis2conc: want {K} finite values, one per species")
    R = np.zeros((K, hi - lo)) if R0 is None else _species_rows(R0, K, n_total, lo, hi, "R0")
    return E, tau, eff, R, c, hi


def minor_steps_host(E, c, tau, eff, R, rows, accumulate, em1=None, dt=1.0, dtype=np.float64):
    """The twin of ONE fiveeq_minor_rows_* call: E [n_rows, k] and c [k] of k <= 8 species, tau / eff [k, n] taken in `dtype`
    (the kernel precision) and widened, R [k, n] fp64 advanced IN PLACE, rows [n_rows, n] of `dtype` written (accumulate
    False) or added onto IN PLACE.  em1 [k, n]: expm1(-dt / tau) from another source than np.expm1 (the device primitive's own
    bits, for a test)."""
    k = E.shape[1]
    if not 1 <= k <= MINOR_MAX:
        raise ValueError(f"n_species={k} outside 1..{MINOR_MAX}")
    tk = np.asarray(tau, dtype=dtype).astype(np.float64)
    ef = np.asarray(eff, dtype=dtype).astype(np.float64)
    em1 = np.expm1(-dt / tk) if em1 is None else np.asarray(em1, dtype=np.float64)
    a = tk * np.asarray(c, dtype=np.float64)[:, None]
    for t in range(E.shape[0]):
        for j in range(k):
            u = a[j] * E[t, j]
            v = R[j] - u
            w = em1[j] * v
            R[j] = R[j] + w
        acc = rows[t].astype(np.float64) if accumulate else np.zeros(R.shape[1])
        for j in range(k):
            p = ef[j] * R[j]
            acc = acc + p
        rows[t] = acc.astype(dtype)


def minor_gas_rows_host(emissions, lifetime, emis2conc, rad_eff, n_total, lo=0, hi=None, R0=None, dt=1.0, into=None, em1=None,
                        dtype=np.float64):
    """minor_gas_rows computed on the host with NumPy: the same calls, the same groups of 8 species, fp32 rows rounded once per
    group.  em1 [K, hi - lo] replaces np.expm1(-dt / tau) (given the device primitive's bits the twin is bit-identical to the
    device rows; np.expm1 itself may differ from it in the last bits).  into: a NumPy array [n_steps, hi - lo] of `dtype`,
    updated in place."""
    E, tau, eff, R, c, hi = _minor_setup(emissions, lifetime, emis2conc, rad_eff, n_total, lo, hi, R0, dt, dtype)
    n_steps, K = E.shape
    n = hi - lo
    if em1 is not None:
        em1 = np.asarray(em1, dtype=np.float64)
        if em1.shape != (K, n):
            raise ValueError(f"em1: want [{K}, {n}]")
    if into is None:
        rows = np.empty((n_steps, n), dtype=dtype)
    else:
        rows = into
        if not isinstance(rows, np.ndarray) or rows.shape != (n_steps, n) or rows.dtype != np.dtype(dtype):
            raise ValueError(f"into: want a {np.dtype(dtype)} array of shape [{n_steps}, {n}]")
    if n and n_steps:
        for k0 in range(0, K, MINOR_MAX):
            g = slice(k0, min(k0 + MINOR_MAX, K))
            minor_steps_host(E[:, g], c[g], tau[g], eff[g], R[g], rows, into is not None or k0 > 0,
                             None if em1 is None else em1[g], dt, dtype)
    return MinorGasRows(rows, R, K)


def minor_gas_rows(emissions, lifetime, emis2conc, rad_eff, n_total, lo=0, hi=None, R0=None, dt=1.0, into=None, device=None,
                   dtype=None):
    """The summed forcing of K >= 1 constant-lifetime species for members [lo, hi) of an n_total-member ensemble, each member
    with its OWN lifetime and radiative efficiency: `.rows` [n_steps, hi - lo] on `device` for
    EnsembleEngine(member_forcing=...), `.R` [K, hi - lo] fp64 on the device (R0= of the call that continues the steps),
    `.species` = K.

    emissions [n_steps, K], shared by the members (finite); emis2conc [K] (or a scalar), shared.  lifetime (finite, > 0) and
    rad_eff: a value per species [K], or per-member rows [K, n_total] (sliced to the shard) or [K, hi - lo]; R0 likewise
    (default 0).  Step of species k:  R <- R + expm1(-dt / tau) (R - tau c E)  in fp64 (step_minor_gases' step), then
    rows[t] = sum_k eff_k R_k in species order.  One HIP pass (fiveeq_minor_rows_*) per consecutive group of 8 species: the
    first writes the rows (adds onto them with into=), the later ones add.  fp64 rows equal one ordered sum over all K
    species; fp32 rows (dtype=torch.float32) are rounded once per group.  into: an existing [n_steps, hi - lo] tensor of
    `dtype` on `device` — noise rows, say — updated in place and returned as `.rows`.  An empty shard or n_steps == 0 returns
    empty rows without a call.  Memory: n_steps (hi - lo) w bytes of rows plus (2 w + 8) K (hi - lo) of parameters and state."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, ptr
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    E, tau, eff, R, c, hi = _minor_setup(emissions, lifetime, emis2conc, rad_eff, n_total, lo, hi, R0, dt,
                                         np.float64 if dtype == torch.float64 else np.float32)
    n_steps, K = E.shape
    n = hi - lo
    dev = torch.device("cuda" if device is None else device) if into is None else into.device
    if into is None:
        rows = torch.empty((n_steps, n), dtype=dtype, device=dev)
    else:
        rows = dev_rows(into, (n_steps, n), "into", dtype, dev)
        if not rows.is_contiguous():
            raise ValueError("into: want a contiguous tensor (it is updated in place)")
    R_d = torch.from_numpy(R).to(dev)
    if n == 0 or n_steps == 0:
        return MinorGasRows(rows, R_d, K)
    tau_d, eff_d = torch.from_numpy(tau).to(dev, dtype), torch.from_numpy(eff).to(dev, dtype)
    lib = _capi.load()
    for k0 in range(0, K, MINOR_MAX):
        k1 = min(k0 + MINOR_MAX, K)
        E_d = torch.from_numpy(np.ascontiguousarray(E[:, k0:k1])).to(dev)
        c_g = np.ascontiguousarray(c[k0:k1])
        call(lib, _capi, "fiveeq_minor_rows", dtype, dev, k1 - k0, n, n, int(n_steps), float(dt), c_g.ctypes.data, ptr(E_d),
             ptr(tau_d[k0:k1]), ptr(eff_d[k0:k1]), ptr(R_d[k0:k1]), ptr(rows), int(into is not None or k0 > 0))
    return MinorGasRows(rows, R_d, K)
