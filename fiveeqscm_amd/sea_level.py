"""Global-mean sea-level rise of every member, from the STORED warming rows (and, optionally, the stored heat uptake).

Sea-level rise is not an elementwise function of a row: every contribution integrates the member's own warming path with the
member's own time-scale and sensitivity.  Each member therefore carries J <= 6 components (thermal expansion, glaciers, Greenland
and Antarctic surface balance and discharge, land water, ...), each of one of two kinds,

    relax   dS/dt = (Seq(T) - S) / tau     Mengel et al. 2016 (PNAS 113:2597; equilibria after Levermann et al. 2013), advanced
                                           EXACTLY over one model step with the row's T held:  S <- S + expm1(-dt / tau) (S - Seq)
    rate    dS/dt = Seq(T)                 the semi-empirical form of Rahmstorf 2007:           S <- S + dt Seq

with  Seq(T) = (a + b x) x,  x = T - T0,  capped from above at `cap` (finite ice; +inf: no cap), and an optional thermosteric
term  eta[m] H[t][m]  on top, H the heat-uptake rows of forcing_rows(want=("H",)) and eta each member's expansion efficiency
(metres per W yr m-2).  The pass is unit-agnostic; the documents use metres and kelvin.

    sl = sea_level_rows(eng.T, eng.out_steps, components, dt=eng.dt)          # or eng.sea_level_rows(components)
    m = trajectory_metrics(sl.total, sl.steps, levels=(0.5,))                 # m.first: the first year at or above 0.5 m
    chi = score_rows(sl.relative_to((95, 115)).total, sl.steps, tide_gauges)  # records are anomalies

One HIP pass (fiveeq_sea_level_rows_*, csrc/fiveeq_sea.hpp; the arithmetic is stated in include/fiveeq.h, "SEA-LEVEL ROWS"): one
member per lane, time sequential, fp64 whatever the precision of the T rows.  The bits depend on the inputs only: not on the
launch shape, on how the members are cut into shards or on how the rows are cut into calls (`state=` carries the components).
Device rows only: there is no CPU path (sea_level_rows_host is the NumPy twin of the tests, bit-identical given the device
expm1).
"""
from dataclasses import dataclass

import numpy as np

SEA_MAX = 6                        # FIVEEQ_SEA_MAX: components per member of fiveeq_sea_level_rows_*
KINDS = ("relax", "rate")
WANT = ("total", "components")
_PARAMS = ("tau", "a", "b", "T0", "cap")        # the order of the C ABI's parameter block


class SeaLevelComponents:
    """The J <= 6 components of every member.  names [J]; kind: "relax" or "rate" per component (one string: all); tau, a, b,
    T0, cap: a value per component [J] (a scalar for J = 1), or per-member rows [J, n_total] over the design (sliced to the
    shard) or [J, hi - lo] over the shard — every per-member parameter over the same members.
    tau: the relaxation time in the units of dt, finite and > 0 for a relax component (not read for a rate component);
    a, b, T0 finite:  Seq = (a + b (T - T0)) (T - T0);  cap: the upper bound of Seq, +inf for none, not NaN.
    ValueError otherwise, naming the parameter."""

    def __init__(self, names, kind, tau, a, b, T0, cap):
        self.names = tuple(str(x) for x in ((names,) if isinstance(names, str) else names))
        J = len(self.names)
        if not 1 <= J <= SEA_MAX:
            raise ValueError(f"{J} components: want 1..{SEA_MAX}")
        self.kind = (kind,) * J if isinstance(kind, str) else tuple(kind)
        if len(self.kind) != J or any(k not in KINDS for k in self.kind):
            raise ValueError(f"kind: want {J} of {KINDS}, got {self.kind!r}")
        self.n_comp = J
        self.rate_mask = sum(1 << j for j, k in enumerate(self.kind) if k == "rate")
        self.n_design = None                                   # the members the per-member rows cover, None without any
        vals = {}
        for name, x in zip(_PARAMS, (tau, a, b, T0, cap)):
            x = np.asarray(x, dtype=np.float64)
            if x.ndim == 0 and J == 1:
                x = x.reshape(1)
            if x.ndim not in (1, 2) or x.shape[0] != J or (x.ndim == 2 and x.shape[1] < 1):
                raise ValueError(f"{name}: want [{J}] (a value per component) or per-member rows [{J}, members]")
            if x.ndim == 2:
                if self.n_design not in (None, x.shape[1]):
                    raise ValueError(f"{name}: rows over {x.shape[1]} members, the other parameters' over {self.n_design}")
                self.n_design = int(x.shape[1])
            vals[name] = x.copy()
        relax = [j for j in range(J) if self.kind[j] == "relax"]
        t = vals["tau"][relax]
        if not (np.isfinite(t).all() and (t > 0).all()):
            raise ValueError("tau: want finite values > 0 for every relax component")
        for name in ("a", "b", "T0"):
            if not np.isfinite(vals[name]).all():
                raise ValueError(f"{name}: want finite values")
        if np.isnan(vals["cap"]).any():
            raise ValueError("cap: NaN (+inf means no cap)")
        self.tau, self.a, self.b, self.T0, self.cap = (vals[name] for name in _PARAMS)

    def block(self, n, members=None):
        """The C ABI's parameter block, fp64 [5, J, n] in the order tau, a, b, T0, cap, for the n members [lo, hi) = `members`
        of the design (default [0, n)): per-member rows over the design are sliced, rows over exactly hi - lo members are
        the shard's own."""
        lo, hi = (0, n) if members is None else (int(members[0]), int(members[1]))
        if not 0 <= lo <= hi or hi - lo != n:
            raise ValueError(f"members [{lo}, {hi}) for rows of {n} members")
        out = np.empty((5, self.n_comp, n))
        for i, name in enumerate(_PARAMS):
            x = getattr(self, name)
            if x.ndim == 1:
                out[i] = x[:, None]
            elif hi <= x.shape[1]:
                out[i] = x[:, lo:hi]
            elif x.shape[1] == n:
                out[i] = x
            else:
                raise ValueError(f"{name}: rows over {x.shape[1]} members cover neither members [{lo}, {hi}) of a design nor a shard of {n}")
        return out


@dataclass
class SeaLevelRows:
    """What sea_level_rows / sea_level_rows_host return.  total [n_rows, N] ([S, n_rows, N] with a scenario axis): fp64, the
    sum of the components (plus eta H) after each row; components [n_rows, J, N] ([S, n_rows, J, N]): each component after each
    row; either is None when not asked for.  S_end [J, N] ([S, J, N]): the components after the last row — with `steps`, what
    a `state=` call continues from.  steps: int64 [n_rows], the model step each row holds."""
    total: object
    components: object
    S_end: object
    steps: np.ndarray

    def relative_to(self, window):
        """The rows minus each member's mean over the stored steps a <= t < b of `window` = (a, b): anomalies, which is what
        tide-gauge and altimetry records are.  Elementwise torch (NumPy for the twin's result) on the rows as they are; the
        result has no S_end and cannot serve as state=."""
        a, b = int(window[0]), int(window[1])
        sel = np.nonzero((self.steps >= a) & (self.steps < b))[0]
        if sel.size == 0:
            raise ValueError(f"window [{a}, {b}) holds none of the rows' steps")
        k0, k1 = int(sel[0]), int(sel[-1]) + 1                 # the steps are consecutive

        def anomaly(x, trailing):                              # trailing: the axes behind the row axis
            if x is None:
                return None
            axis = len(x.shape) - 1 - trailing
            ref = x[(slice(None),) * axis + (slice(k0, k1),)]
            return x - (ref.mean(axis=axis, keepdims=True) if isinstance(x, np.ndarray) else ref.mean(dim=axis, keepdim=True))

        return SeaLevelRows(anomaly(self.total, 1), anomaly(self.components, 2), None, self.steps)


def _plan(K, N, lead, steps, components, dt, heat, expansion, state, want, members):
    """The checks both forms share.  Returns (steps int64, the parameter block [5, J, N], eta [N] or None, the state before
    the first row or None for zeros, whether component rows are wanted)."""
    from .diagnose import check_consecutive
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in WANT for w in want):
        raise ValueError(f"want: {want!r}; any of {WANT}")
    if not isinstance(components, SeaLevelComponents):
        raise ValueError("components: want a SeaLevelComponents")
    if N < 1:
        raise ValueError("T_rows: no members")
    st = np.asarray(steps)                                     # (not _rowargs.model_steps: the twin runs without torch)
    if st.shape != (K,) or (K and not np.issubdtype(st.dtype, np.integer)):
        raise ValueError(f"steps: want {K} integers, one per row")
    st = st.astype(np.int64)
    check_consecutive(st, "the sea-level integration")
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"dt={dt} must be finite and > 0")
    if (heat is None) != (expansion is None):
        raise ValueError("expansion= (each member's eta) and heat= (the H rows of forcing_rows) come together; without H rows "
                         "model the expansion as a relax component")
    eta = None
    if expansion is not None:
        eta = np.asarray(expansion.detach().cpu() if hasattr(expansion, "detach") else expansion, dtype=np.float64)
        eta = np.array(np.broadcast_to(eta, (N,)) if eta.ndim == 0 else eta)
        if eta.shape != (N,) or not np.isfinite(eta).all():
            raise ValueError(f"expansion: want a finite value, or one per member [{N}]")
    par = components.block(N, members)
    S0 = None
    if state is not None:
        S0 = state
        if isinstance(state, SeaLevelRows):
            if state.S_end is None:
                raise ValueError("state: rows without S_end (a relative_to() result) cannot be continued")
            if K and state.steps.size and st[0] != state.steps[-1] + 1:
                raise ValueError(f"steps: the first new step {int(st[0])} does not follow the state's last step "
                                 f"{int(state.steps[-1])}: a gap would silently shorten the integration")
            S0 = state.S_end
        if tuple(S0.shape) != lead + (components.n_comp, N):
            raise ValueError(f"state: want the components before the first row, {list(lead + (components.n_comp, N))}, got {list(S0.shape)}")
    return st, par, eta, S0, "components" in want, "total" in want


def sea_steps_host(T, par, rate_mask, dt, S, heat=None, eta=None, em1=None, comps=False):
    """The twin of ONE fiveeq_sea_level_rows_* call, operation for operation: T [Sc, K, n] of the kernel precision (widened
    here), par [5, J, n], S [Sc, J, n] fp64 advanced IN PLACE, heat [Sc, K, n] fp64 with eta [n], or None.  em1 [J, n]:
    expm1(-dt / tau) from another source than np.expm1 (the device primitive's own bits, for a test); read for the relax
    components only.  Returns (total [Sc, K, n], comps [Sc, K, J, n] or None)."""
    Sc, K, n = T.shape
    J = par.shape[1]
    if not 1 <= J <= SEA_MAX:
        raise ValueError(f"n_comp={J} outside 1..{SEA_MAX}")
    tau, a, b, T0, cap = par
    rate = [bool(rate_mask >> j & 1) for j in range(J)]
    with np.errstate(all="ignore"):
        if em1 is None:
            em1 = np.zeros((J, n))
            for j in range(J):
                if not rate[j]:
                    em1[j] = np.expm1(-dt / tau[j])
        em1 = np.asarray(em1, dtype=np.float64)
        total = np.empty((Sc, K, n))
        rows = np.empty((Sc, K, J, n)) if comps else None
        for t in range(K):
            Tt = T[:, t].astype(np.float64)
            for j in range(J):
                x = Tt - T0[j]
                p = b[j] * x
                c = a[j] + p
                e = c * x
                e = np.where(e > cap[j], cap[j], e)
                if rate[j]:
                    w = dt * e
                else:
                    v = S[:, j] - e
                    w = em1[j] * v
                S[:, j] = S[:, j] + w
            acc = eta * heat[:, t] if heat is not None else np.zeros((Sc, n))
            for j in range(J):
                acc = acc + S[:, j]
            total[:, t] = acc
            if comps:
                rows[:, t] = S
    return total, rows


def sea_level_rows_host(T_rows, steps, components, *, dt, heat=None, expansion=None, state=None, want=("total",), members=None,
                        em1=None, dtype=None):
    """sea_level_rows computed on the host with NumPy: the same operation list on NumPy rows.  dtype: the precision the T
    rows are taken in (default: float32 for float32 rows, else float64).  em1 [J, N] replaces np.expm1(-dt / tau) (given the
    device primitive's bits the twin is bit-identical to the device rows; np.expm1 itself may differ from it in the last
    bits).  state: an earlier result of this function, or S0 [.., J, N]; the caller's arrays are not advanced."""
    T = np.asarray(T_rows)
    if T.ndim not in (2, 3):
        raise ValueError("T_rows: want rows [n_rows, N] or [S, n_rows, N]")
    dtype = np.dtype(dtype if dtype is not None else (np.float32 if T.dtype == np.float32 else np.float64))
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("dtype must be float64 or float32")
    scen = T.ndim == 3
    x = (T if scen else T[None]).astype(dtype)
    Sc, K, N = x.shape
    lead = (Sc,) if scen else ()
    st, par, eta, S0, comps, total = _plan(K, N, lead, steps, components, dt, heat, expansion, state, want, members)
    J = components.n_comp
    h = None
    if heat is not None:
        h = np.asarray(heat, dtype=np.float64)
        if h.shape != T.shape:
            raise ValueError(f"heat: want fp64 rows of shape {list(T.shape)}")
        h = h if scen else h[None]
    S = np.zeros((Sc, J, N)) if S0 is None else np.array(np.asarray(S0, dtype=np.float64).reshape(Sc, J, N))
    if em1 is not None:
        em1 = np.asarray(em1, dtype=np.float64)
        if em1.shape != (J, N):
            raise ValueError(f"em1: want [{J}, {N}]")
    tot, rows = sea_steps_host(x, par, components.rate_mask, float(dt), S, h, eta, em1, comps)
    drop = (lambda v: v) if scen else (lambda v: v[0])
    return SeaLevelRows(drop(tot) if total else None, drop(rows) if comps else None, drop(S), st)


def sea_level_rows(T_rows, steps, components, *, dt, heat=None, expansion=None, state=None, want=("total",), members=None):
    """The sea-level rise of every member after each stored row — one streaming HIP pass (fiveeq_sea_level_rows_*).
    T_rows [n_rows, N] or [S, n_rows, N]: the stored warming, fp32 / fp64 ON THE GPU (engine.T, or row / member slices of it),
    read in place whenever the member stride is 1 and every leading axis of extent > 1 lies at least N apart, copied
    otherwise.  steps [n_rows]: the model step each row holds — CONSECUTIVE steps (ValueError otherwise, naming the first gap:
    every row advances the components by one dt, so a gap would silently shorten the integration).  components: a
    SeaLevelComponents, its per-member rows over these N members (or over the design, with members=(lo, hi) the range these N
    columns are).  dt: the run's step.
    heat [.., n_rows, N] fp64 on the same device with expansion (a value or [N], each member's eta): the thermosteric term
    eta H on top of the components, H the heat-uptake rows of forcing_rows(want=("H",)).  Runs for which H does not exist —
    member_forcing= runs, whose forcing the forcing-rows pass does not recompute — use a relax component for the expansion
    instead.
    want: any of "total", "components".  state: the result of an earlier call over the rows directly before these (its last
    step plus one must be the first step here, else ValueError), or the components before the first row S0 [.., J, N]
    (default 0): the outputs of the calls, concatenated, are bit for bit those of one call over all the rows.
    The arithmetic is fp64 whatever the rows' precision; a NaN in a member's T row makes that member NaN from that row on and
    touches no other member.  TypeError for host rows: there is no CPU path.  Runs on the current stream; reads its inputs,
    allocates its results.  Returns SeaLevelRows (total, components, S_end, steps): `.total` goes where stored rows go —
    trajectory_metrics (levels in metres), score_rows, gather_summary, running_mean, window_trends, drivers.
    Memory: 8 n_rows N bytes of total (J times that of component rows) plus 8 (6 J + 1) N of parameters and state."""
    import torch

    from . import _capi
    from ._rowargs import call, dev_rows, ptr, walk_in_place
    if not isinstance(T_rows, torch.Tensor) or T_rows.dim() not in (2, 3):
        raise ValueError("T_rows: want a tensor [n_rows, N] or [S, n_rows, N]")
    if not T_rows.is_cuda or T_rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"T_rows must be fp32 / fp64 rows on a GPU (got {T_rows.dtype} on {T_rows.device}): the sea-level rows run "
                        "through the HIP kernel and have no CPU fallback")
    scen = T_rows.dim() == 3
    x = T_rows if scen else T_rows.unsqueeze(0)
    Sc, K, N = (int(v) for v in x.shape)
    lead = (Sc,) if scen else ()
    dev = T_rows.device
    st, par, eta, S0, comps, total = _plan(K, N, lead, steps, components, dt, heat, expansion, state, want, members)
    J = components.n_comp
    h, h_scen, h_row = None, N, N
    if heat is not None:
        h = dev_rows(heat, tuple(T_rows.shape), "heat", torch.float64, dev)
        h, (h_scen, h_row) = walk_in_place(h if scen else h.unsqueeze(0), N)
    S_io = torch.zeros((Sc, J, N), dtype=torch.float64, device=dev)
    if S0 is not None:
        S_io.copy_((S0 if isinstance(S0, torch.Tensor) else torch.from_numpy(np.asarray(S0, dtype=np.float64))).reshape(Sc, J, N))
    tot = torch.empty((Sc, K, N), dtype=torch.float64, device=dev)
    rows = torch.empty((Sc, K, J, N), dtype=torch.float64, device=dev) if comps else None
    if K:
        x, (t_scen, t_row) = walk_in_place(x, N)
        par_d = torch.from_numpy(par).to(dev)
        eta_d = None if eta is None else torch.from_numpy(eta).to(dev)
        call(_capi.load(), _capi, "fiveeq_sea_level_rows", T_rows.dtype, dev, Sc, J, components.rate_mask, N, N, K, float(dt), ptr(x),
             t_row, t_scen, ptr(par_d), ptr(h), h_row, h_scen, ptr(eta_d), ptr(S_io), ptr(tot), ptr(rows), N)
    drop = (lambda v: v) if scen else (lambda v: v[0])
    return SeaLevelRows(drop(tot) if total else None, drop(rows) if comps else None, drop(S_io), st)
