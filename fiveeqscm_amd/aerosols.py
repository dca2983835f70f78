"""Per-member aerosol forcing rows from emissions: ERFari + ERFaci as rows [n_steps, N] for EnsembleEngine(member_forcing=...).

A shared table of short-lived-forcer emissions E [n_steps, K] (SO2, BC, OC, NH3, ...) and its reference (pre-industrial) record
base [K] become each member's OWN aerosol forcing history,
    F[t] = sum_k ari_k (E[t, k] - base_k)  -  beta ( ln(1 + sum_{k in aci} E[t, k] / s_k) - ln(1 + sum_{k in aci} base_k / s_k) ),
the aerosol-radiation term a per-member linear mix of the species and the aerosol-cloud term saturating with the member's own
shape parameters s_k: a strong-cooling and a weak-cooling member disagree on WHEN the cooling peaked, which a scaled shared
series (forcing=ExternalForcings(...) with an fx_scale row) cannot express.

One HIP pass (fiveeq_aerosol_rows_*, csrc/fiveeq_aerosol.hpp; the arithmetic is stated in include/fiveeq.h, "AEROSOL FORCING
ROWS") over at most 8 species.  A rank computes exactly its shard [lo, hi); the rows do not depend on the world size or on how
the steps are cut into calls (there is no state to carry).  aci_scale_for_target derives each member's beta from a sampled
present-day ERFaci, the calibration FaIR users expect.
"""
import numpy as np

from .minor_gases import _species_rows

AEROSOL_MAX = 8                    # FIVEEQ_AEROSOL_MAX: species per call of fiveeq_aerosol_rows_*; the cloud term's sum cannot be split


class AerosolRows:
    """What aerosol_rows / aerosol_rows_host return: `rows` [n_steps, n] (the aerosol forcing, W m-2) and `species` (K).  The
    host twin also leaves `y` [n_steps, n] and `y0` [n] fp64, the arguments of the cloud term's logarithms (None without a
    cloud term and on the device form)."""

    def __init__(self, rows, species, y=None, y0=None):
        self.rows, self.species, self.y, self.y0 = rows, species, y, y0


def _host(x):
    """x as it lies on the host: a torch tensor is downloaded, anything else is left to NumPy."""
    return x.detach().cpu().numpy() if hasattr(x, "detach") else x


def _member_row(x, n_total, lo, hi, name):
    """x as fp64 [hi - lo]: a scalar, or a value per member [n_total] (sliced to the shard) or [hi - lo]."""
    x = np.asarray(_host(x), dtype=np.float64)
    n = hi - lo
    if x.ndim == 0:
        return np.full(n, float(x))
    if x.shape == (n_total,):
        return np.array(x[lo:hi])
    if x.shape == (n,):
        return x.copy()
    raise ValueError(f"{name}: want a scalar, or a value per member [{n_total}] over the design or [{n}] over the shard")


def _aci_mask(aci, K):
    if aci is None:
        return [True] * K
    a = np.asarray(aci)
    if a.shape != (K,) or a.dtype != np.bool_:
        raise ValueError(f"aci: want {K} booleans, one per species (None: every species enters the cloud term)")
    return [bool(v) for v in a]


def _aerosol_setup(emissions, base, ari, shape, beta, n_total, lo, hi, aci, dtype):
    """The checked host arguments (E [n_steps, K], b [K], ari [K, n], s [K, n], beta [n], in_aci [K] booleans, hi) of both
    forms.  s is 1 where the cloud term does not read it, beta 0 without a cloud term."""
    E = np.asarray(emissions, dtype=np.float64)
    if E.ndim == 1:
        E = E[:, None]
    if E.ndim != 2 or E.shape[1] < 1:
        raise ValueError("emissions: want [n_steps, K] with K >= 1 species")
    n_steps, K = E.shape
    if K > AEROSOL_MAX:
        raise ValueError(f"emissions: K={K} species, at most {AEROSOL_MAX} (the cloud term's sum cannot be split across calls)")
    hi = n_total if hi is None else hi
    if not 0 <= lo <= hi <= n_total:
        raise ValueError(f"members [{lo}, {hi}) outside [0, {n_total})")
    if not (np.isfinite(E).all() and (E >= 0).all()):
        raise ValueError("emissions: want finite values >= 0")
    b = np.asarray(base, dtype=np.float64)
    b = b.reshape(1) if b.ndim == 0 and K == 1 else b
    if b.shape != (K,) or not (np.isfinite(b).all() and (b >= 0).all()):
        raise ValueError(f"base: want {K} finite values >= 0, one per species")
    in_aci = _aci_mask(aci, K)
    n = hi - lo
    A = _species_rows(_host(ari), K, n_total, lo, hi, "ari")
    if not (np.isfinite(A).all() and np.isfinite(A.astype(dtype)).all()):
        raise ValueError(f"ari: want finite values (in {np.dtype(dtype)} too)")
    if any(in_aci):
        S = _species_rows(_host(shape), K, n_total, lo, hi, "shape")
        S[[k for k in range(K) if not in_aci[k]]] = 1.0                         # not read: nothing to refuse there
        sq = S.astype(dtype).astype(np.float64)                                 # as the kernel reads them
        with np.errstate(divide="ignore", over="ignore"):
            ok = np.isfinite(S).all() and (S > 0).all() and np.isfinite(sq).all() and (sq > 0).all() and np.isfinite(1.0 / sq).all()
        if not ok:
            raise ValueError(f"shape: want finite values > 0 with a finite reciprocal (in {np.dtype(dtype)} too) for the species in aci")
        B = _member_row(beta, n_total, lo, hi, "beta")
        if not (np.isfinite(B).all() and np.isfinite(B.astype(dtype)).all()):
            raise ValueError(f"beta: want finite values (in {np.dtype(dtype)} too)")
    else:
        S, B = np.ones((K, n)), np.zeros(n)
    return E, b, A, S, B, in_aci, hi


def aerosol_steps_host(E, b, ari, shape, beta, in_aci, rows, accumulate, log=np.log, dtype=np.float64):
    """The twin of ONE fiveeq_aerosol_rows_* call, operation for operation: E [n_rows, K], b [K], ari / shape [K, n] and beta [n]
    taken in `dtype` (the kernel precision) and widened, rows [n_rows, n] of `dtype` written (accumulate False) or added onto
    IN PLACE.  log: applied ONCE to the fp64 array [n_rows + 1, n] of y0 and every step's y.  Returns (y [n_rows, n], y0 [n]),
    or (None, None) without a cloud term."""
    n_rows, K = E.shape
    if not 1 <= K <= AEROSOL_MAX:
        raise ValueError(f"n_species={K} outside 1..{AEROSOL_MAX}")
    n = rows.shape[1]
    aq = np.asarray(ari, dtype=dtype).astype(np.float64)
    cloud = [k for k in range(K) if in_aci[k]]
    y = y0 = None
    if cloud:
        sq = np.asarray(shape, dtype=dtype).astype(np.float64)
        bq = np.asarray(beta, dtype=dtype).astype(np.float64)
        g = {k: 1.0 / sq[k] for k in cloud}
        Y = np.empty((n_rows + 1, n))
        for i in range(n_rows + 1):
            x = np.zeros(n)
            for k in cloud:
                p = g[k] * (b[k] if i == 0 else E[i - 1, k])
                x = x + p
            Y[i] = 1.0 + x
        L = np.asarray(log(Y), dtype=np.float64)
        if L.shape != Y.shape:
            raise ValueError("log: want a callable that maps an fp64 array to an fp64 array of the same shape")
        y0, y = Y[0], Y[1:]
    for t in range(n_rows):
        acc = rows[t].astype(np.float64) if accumulate else np.zeros(n)
        for k in range(K):
            e = E[t, k] - b[k]
            p = aq[k] * e
            acc = acc + p
        if cloud:
            v = L[t + 1] - L[0]
            w = bq * v
            acc = acc - w
        rows[t] = acc.astype(dtype)
    return y, y0


def aerosol_rows_host(emissions, base, ari, shape, beta, n_total, lo=0, hi=None, aci=None, into=None, log=np.log,
                      dtype=np.float64):
    """aerosol_rows computed on the host with NumPy: the same operation list.  log: a callable applied to fp64 arrays of y
    (given the device primitive's bits — fiveeq_math_probe_f64(op = 2) — the twin is bit-identical to the device rows; np.log
    itself may differ from it in the last bits).  into: a NumPy array [n_steps, hi - lo] of `dtype`, updated in place."""
    E, b, A, S, B, in_aci, hi = _aerosol_setup(emissions, base, ari, shape, beta, n_total, lo, hi, aci, dtype)
    n_steps, K = E.shape
    n = hi - lo
    if into is None:
        rows = np.empty((n_steps, n), dtype=dtype)
    else:
        rows = into
        if not isinstance(rows, np.ndarray) or rows.shape != (n_steps, n) or rows.dtype != np.dtype(dtype):
            raise ValueError(f"into: want a {np.dtype(dtype)} array of shape [{n_steps}, {n}]")
    y = y0 = None
    if n and n_steps:
        y, y0 = aerosol_steps_host(E, b, A, S, B, in_aci, rows, into is not None, log, dtype)
    return AerosolRows(rows, K, y, y0)


def aerosol_rows(emissions, base, ari, shape, beta, n_total, lo=0, hi=None, aci=None, into=None, device=None, dtype=None):
    """The aerosol forcing of K <= 8 short-lived forcers for members [lo, hi) of an n_total-member ensemble, each member with
    its OWN aerosol-radiation coefficients, cloud-term shape parameters and cloud-term scale: `.rows` [n_steps, hi - lo] on
    `device` for EnsembleEngine(member_forcing=...), `.species` = K.

    emissions [n_steps, K] and base [K] (the reference, pre-industrial emissions): host arrays shared by the members, finite
    and >= 0.  ari (W m-2 per emission unit) and shape (s_k, emission units): a value per species [K], or per-member rows
    [K, n_total] (sliced to the shard) or [K, hi - lo].  beta (W m-2): a scalar, [n_total] or [hi - lo].  aci: K booleans, the
    species that enter the cloud term (None: every species); shape must be finite and > 0 with a finite reciprocal, in the row
    precision too, for those species, and is not read for the others; with no species in aci, shape and beta may be None.
        rows[t] = sum_k ari_k (E[t, k] - base_k) - beta (ln(1 + sum_aci E[t, k] / s_k) - ln(1 + sum_aci base_k / s_k))
    in fp64, operation for operation as include/fiveeq.h states it ("AEROSOL FORCING ROWS"); fp32 rows (dtype=torch.float32)
    are rounded once at the store.  emissions equal to base at every step give rows of +0.0: the run without them, bit for bit.
    K > 8 is refused: the cloud term's sum cannot be split across calls.  into: an existing contiguous [n_steps, hi - lo] tensor
    of `dtype` on `device` — AR(1) noise or minor-gas rows, say — updated in place and returned as `.rows`.  An empty shard or
    n_steps == 0 returns empty rows without a call.  Memory: n_steps (hi - lo) w bytes of rows plus (2 K + 1) (hi - lo) w of
    parameters."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, ptr
    dtype = torch.float64 if dtype is None else dtype
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    E, b, A, S, B, in_aci, hi = _aerosol_setup(emissions, base, ari, shape, beta, n_total, lo, hi, aci,
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
    if n == 0 or n_steps == 0:
        return AerosolRows(rows, K)
    mask = sum(1 << k for k in range(K) if in_aci[k])
    E_d = torch.from_numpy(np.ascontiguousarray(E)).to(dev)
    A_d = torch.from_numpy(A).to(dev, dtype)
    S_d = torch.from_numpy(S).to(dev, dtype) if mask else None
    B_d = torch.from_numpy(B).to(dev, dtype) if mask else None
    b = np.ascontiguousarray(b)
    call(_capi.load(), _capi, "fiveeq_aerosol_rows", dtype, dev, K, mask, n, n, int(n_steps), b.ctypes.data, ptr(E_d), ptr(A_d),
         ptr(S_d), ptr(B_d), ptr(rows), int(into is not None))
    return AerosolRows(rows, K)


# ------------------------------------------------------------------------------------
# The calibration: a sampled present-day ERFaci per member -> that member's beta.
# ------------------------------------------------------------------------------------
def _window(window, n_steps):
    try:
        a, b = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError("window: want (a, b), the rows [a, b) the cloud term is averaged over") from None
    if not 0 <= a < b <= n_steps:
        raise ValueError(f"window: rows [{a}, {b}) outside [0, {n_steps}) or empty")
    return a, b


def _refuse_zero_mean(zero, lo):
    if zero.size:
        raise ValueError(f"member {lo + int(zero[0])}: its cloud term averages to 0 over the window (emissions equal to base there?): "
                         "no beta gives it the target")


def aci_scale_for_target_host(emissions, base, shape, target, window, n_total, lo=0, hi=None, aci=None, log=np.log,
                              dtype=np.float64):
    """aci_scale_for_target on the host with NumPy, the same operations: beta [hi - lo] fp64."""
    E = np.asarray(emissions, dtype=np.float64)
    E = E[:, None] if E.ndim == 1 else E
    a, b = _window(window, E.shape[0])
    hi = n_total if hi is None else hi
    unit = aerosol_rows_host(E[a:b], base, np.zeros(E.shape[1]), shape, 1.0, n_total, lo, hi, aci, log=log, dtype=dtype)
    tgt = _member_row(target, n_total, lo, hi, "target")
    if not np.isfinite(tgt).all():
        raise ValueError("target: want finite values")
    if hi == lo:
        return np.zeros(0)
    total = unit.rows[0].astype(np.float64)
    for t in range(1, b - a):
        total = total + unit.rows[t].astype(np.float64)
    mean = total / float(b - a)
    _refuse_zero_mean(np.flatnonzero(mean == 0.0), lo)
    return tgt / mean


def aci_scale_for_target(emissions, base, shape, target, window, n_total, lo=0, hi=None, aci=None, device=None, dtype=None):
    """Each member's cloud-term scale beta [hi - lo] (an fp64 tensor on `device`) such that its cloud term
    -beta (ln(1 + sum_aci E / s) - ln(1 + sum_aci base / s)), averaged over the rows window = (a, b) — present day, say —
    equals that member's `target` (a scalar, [n_total] or [hi - lo]; negative for cooling).  The calibration of the published
    FaIR ensembles: sample a present-day ERFaci and the shape parameters, derive beta.

    One aerosol_rows call over rows [a, b) with ari = 0 and beta = 1 (rows of `dtype`, the precision the run's rows will have),
    the rows added one by one in ascending order as elementwise fp64 adds, one division by b - a, then beta = target / mean:
    elementwise IEEE operations, so beta has the same bits for any shard split.  A member whose mean is 0 is refused by name.
    Pass the result as aerosol_rows(beta=...)."""
    import torch
    E = np.asarray(emissions, dtype=np.float64)
    E = E[:, None] if E.ndim == 1 else E
    a, b = _window(window, E.shape[0])
    hi = n_total if hi is None else hi
    unit = aerosol_rows(E[a:b], base, np.zeros(E.shape[1]), shape, 1.0, n_total, lo, hi, aci, device=device, dtype=dtype)
    tgt = _member_row(target, n_total, lo, hi, "target")
    if not np.isfinite(tgt).all():
        raise ValueError("target: want finite values")
    if hi == lo:
        return torch.zeros(0, dtype=torch.float64, device=unit.rows.device)
    total = unit.rows[0].to(torch.float64)
    for t in range(1, b - a):
        total = total + unit.rows[t].to(torch.float64)
    mean = total / float(b - a)
    _refuse_zero_mean(torch.nonzero(mean == 0.0).reshape(-1).cpu().numpy(), lo)
    return torch.from_numpy(tgt).to(mean.device) / mean
