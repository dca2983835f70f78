"""Python host of the ensemble engine: torch-ROCm tensors own the memory, the C ABI
(include/fiveeq.h) does the work.  One engine = one device = one member shard.

Data layout in HBM (struct-of-arrays over members; N = members of this shard):
    r      [3G, N]   rows g*3 + (0,1,2) = r0, rC, rT of gas g
    q      [2,  N]   thermal-box coefficients
    R      [SP, N]   pool contents, gas-major (SP = sum of active pools)
    S      [2,  N]   thermal-box temperatures
    drive  [n_steps, 8]   shared: E_g, cumulative E_g before the step, F_ext, output row
    C      [n_rows, G, N]    concentrations of the stored steps (all steps, a selection, or none)
    T      [n_rows, N]       temperature of the stored steps
    T_stats[W, n_steps, 4]   optional per-wave (sum, sum^2, min, max) of T, W = ceil(N/64), fp64 (0.5 B per member-step:
                             allocated by the first run that writes wave records, not at construction)
    T_hist [n_steps, n_bins] optional fixed-bin histogram of T for EVERY step (int64), filled through a ring of 2-byte bin
                             indices that a histogram pass drains while the next steps are computed

There is no CPU path: constructing an engine without a GPU, or without the built
HIP library, raises.  (The reference's own function, `calculate_hfc_conc`, is a
NumPy one-liner and lives in fiveeqscm_amd.concentrations.)
"""
import ctypes
import os

import numpy as np
import torch

from . import _capi
from ._rowargs import bool_mask, int_weights
from .checkpoint import CheckpointMixin
from .emissions import concentration_mask, emissions_sha256, make_drive, make_scenario_drive
from .forcing import ScenarioForcings
from .params import make_model, n_gas_of, pools_of
from .tuning import (_env_choice, _env_positive, calibrate, concurrent_side_streams,  # noqa: F401  (calibrate: part of this
                     side_stream_report)                                               # module's interface)

_DTYPES = {torch.float64: "f64", torch.float32: "f32"}
INFINITY_CACHE_BYTES = 256 << 20     # MI355X die-level L3 (MI355X_MICROARCH.md); sizes the chunk-major schedule
# ... whose chunks hold at most this share of it in state + parameter rows: the per-step rate of a chunk-major run is flat from
# 0.55 to 0.85 of the cache and falls off above (8M fp64 members, two streams: 0.88-0.89 of 8 TB/s up to 0.8, 0.82-0.84 at
# 0.9-0.95; 25M fp32: 0.905-0.914 up to 0.85, 0.844 at 0.95; profiles/r05/chunk_share_sweep.txt; rounds 2-4 filled the whole
# cache, 0.965 after rounding).  An ensemble that fits the cache by itself is not chunked (0.91 up to 0.96 of the cache, 0.82 at
# 1.02), and the chunks are EVEN: a small ragged last chunk runs its steps launch-bound (2.4M members as 1179648 + 1179648 +
# 40704: 0.877; as 2 x 1.2M: 0.909; profiles/r05/chunk_share_sweep.txt, second table).
CHUNK_CACHE_SHARE = 0.7              # (0.8 is as good or better at 4M, 16M and 25M members and 3.5 % worse at 8M: third table of that file)


# The two box-dependent figures the schedules are derived from.  The defaults are what rounds 1-3 measured on MI355X; another
# box (or a future driver) can set them from the environment, or measure them with `calibrate()` below, which overwrites these
# module attributes — engines created afterwards use the new values.
HBM_STREAM_BYTES_PER_S = _env_positive("FIVEEQ_HBM_STREAM_BYTES_PER_S", 6.7e12)    # ceiling of the per-step kernel
LAUNCH_BOUNDARY_S = _env_positive("FIVEEQ_LAUNCH_BOUNDARY_S", 2.0e-6)              # dependent-launch boundary on one stream (measured 1.5-2.6 us)
PER_STEP_SPLIT_MIN_S = 16.0e-6       # a per-step launch is split over two streams from this much traffic time on
PER_STEP_BLOCK = 25                  # steps enqueued per part before switching to the next part's stream
FUSED_SPAN_STEPS = 128               # mode='fused': steps per launch for ensembles of few rounds of waves (see fused_span)
FUSED_SPAN_MAX_ROUNDS = 8.0          # ... up to this many rounds of 4 waves per SIMD
FUSED_SPAN_MIN_ROUNDS = 0.25         # ... and from this many on
# mode='auto' on a LAUNCH-BOUND ensemble (auto_k_steps() > 1) takes the small-ensemble kernel (include/fiveeq.h,
# fiveeq_run_small_*): for a lone 4-pool gas one member per QUAD of lanes while the quads' waves get a SIMD each (one
# 256-thread workgroup per CU: 64 members per CU, 16384 on an MI355X; past that two waves share a SIMD and the unspread form
# is ahead), else one member per lane (fp64 CO2-only, us per step: 0.41 / 0.54 / 0.73 quad / one lane / fused kernel at 10k
# members, 0.89 / 1.09 one lane / fused at 110k, 1.74 / 1.90 at 250k; three gases: 0.94 / 1.38 at 10k, 1.66 / 1.98 at 110k,
# 2.40 / 2.65 at 150k: profiles/r05/small_ensemble_ab.txt, small_ensemble_multigas_ab.txt, auto_window_sweep.txt)
SMALL_QUAD_MEMBERS_PER_CU = 64
# ... and the 4 + 1 + 1 layout one member per OCTET of lanes (round 6, small_octet_kernel: 8 members per wave) up to this many
# members per CU; past it the one-lane form (profiles/r06/small_octet_ab.txt)
SMALL_OCTET_MEMBERS_PER_CU = 64
KSTEPS_LAUNCH_BOUND = 128            # steps per launch of the K-step form on a launch-bound ensemble (2 / 8 / 32 / 128 steps per
                                     # launch at 110k three-gas members: 4.42 / 2.70 / 2.13 / 1.97 us per step; one launch: 1.98)


def _rows(x, K, N, name):
    if isinstance(x, torch.Tensor):                    # already on a device (params.sample_ensemble_shard)
        if tuple(x.shape) != (K, N):
            raise ValueError(f"{name}: tensor shape {tuple(x.shape)}, want [{K},{N}]")
        return x
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 0:
        x = x.reshape(1)
    if x.ndim == 1:
        if x.shape[0] != K:
            raise ValueError(f"{name}: shape {x.shape}, want [{K}] or [{K},{N}]")
        return np.broadcast_to(x[:, None], (K, N))
    if x.shape != (K, N):
        raise ValueError(f"{name}: shape {x.shape}, want [{K}] or [{K},{N}]")
    return x


def _joined(eng, stream=None):
    """Before a reader looks at the engine's rows: `stream` (default: the current one) waits for what run(..., join=False) left
    outstanding.  (A function: the CPU tests call the readers on a stub engine that has no join().)"""
    if eng._ps_unjoined:
        eng.join(stream)


def _stored_rows_slice(rows):
    """rows= of a reader of the stored rows, as a slice."""
    sel = slice(None) if rows is None else rows
    if not isinstance(sel, slice) or sel.step not in (None, 1):
        raise ValueError("rows: want a slice of the stored rows with step 1 (or None for all)")
    return sel


def _is_scenario_set(emissions):
    """True for emissions of several scenarios: a 3-D array, or a sequence of 2-D [n_steps, G] arrays."""
    if isinstance(emissions, (list, tuple)):
        return len(emissions) > 0 and all(np.ndim(e) == 2 for e in emissions)
    return np.ndim(emissions) == 3


class EnsembleEngine(CheckpointMixin):
    """Advance N ensemble members of the five-equation model on one MI355X."""

    MODES = ("per_step", "graph", "fused", "ksteps", "small", "auto")
    # concentration_driven=True together with forcing= / observations=: refused here, carried by ConcentrationDrivenEngine below
    _INVERSE_CALIBRATION = False

    def __init__(self, params, n_members, emissions, *, F_ext=None, dt=1.0, dtype=torch.float64,
                 device=None, store_trajectory=True, output_steps=None, store_concentrations=True,
                 collect_stats=False, hist=None, hist_ring_steps="auto", concentration_driven=False,
                 chunk_members="auto", per_step_streams="auto", fused_span="auto", small_lanes="auto", compensated=False,
                 R0=None, S0=None, lib_path=None, observations=None, scenario_names=None, forcing=None,
                 uniform_rows="auto", member_forcing=None):
        """store_trajectory / output_steps: True stores C, T of every step; a list of step indices
        stores only those (rows in increasing step order, see `out_steps`); False stores nothing.
        store_concentrations=False keeps only the T rows (a 100M-member fp32 run then stores 4 B instead
        of 16 B per member and stored step).
        collect_stats: also accumulate per-step ensemble moments of T on the device (`stats()`).
        hist=(lo, hi, n_bins): allocate `T_hist` [n_steps, n_bins] (int64), the fixed-bin histogram of T of
        EVERY step, for all-timestep percentiles (distributed.histogram_percentiles) without a stored
        trajectory.  The stepping kernel also writes each member's BIN INDEX (uint16: 2 bytes per member-step) into a ring of
        `hist_ring_steps` steps, which a histogram pass counts into T_hist — same counts bit for bit as a histogram of
        stored rows:
          run(mode="fused")    two ring slots, the pass drains one on a second HIP stream while the fused kernel fills the
                               other ("auto" ring length: what 8 GB hold, at most 128 steps: 6.4 GB at 12.5M members);
          run(mode="per_step") one slot, counted right behind its steps.
        concentration_driven: inverse mode — `emissions` holds the TARGET concentrations [n_steps, G]
        at the end of each step (shared by all members); the per-member emissions that reach them
        are diagnosed into `self.E` ([n_rows, G, N], aliasing `self.C`), and `self.cumE` [G, N] is
        extra per-member state.  Runs through `run()` as one time-fused launch per call.
        chunk_members: per-step / graph runs of ensembles whose state + parameters exceed the 256 MiB
        Infinity Cache are scheduled chunk-major — all requested steps for members [0, c), then
        [c, 2c), ... — so each chunk's rows stay cache-resident between its consecutive launches
        (0.89-0.91 of 8 TB/s from 4M to 100M members against 0.70-0.79 streamed from HBM; bit-identical results: members
        never interact).  "auto" sizes a chunk's rows to at most CHUNK_CACHE_SHARE of the cache, in even chunks; an int forces c; None / 0 disables it
        (the library then runs such launches with non-temporal row accesses, include/fiveeq.h "CACHE POLICY").
        per_step_streams: mode='per_step' launches each timestep as this many kernels over contiguous member parts, each
        part's launches on its own HIP stream, so that one part's launch tail and ramp overlap the other part's kernel
        (members never interact, so nothing orders the parts against each other).  Two parts: -6.5 % per step at 1M fp64
        members (36.9 -> 34.5 us), -8 % at 0.5M, -2 % at 4M, +10 % at 0.25M (profiles/r03/two_stream_*.txt), bit-identical
        results.  "auto": 2 when one step moves at least ~16 us of traffic, else 1; an int forces it.
        fused_span: mode='fused' covers the requested steps with launches of this many steps (None: one launch).  A SIMD serves
        its oldest wave first, so the waves of a long launch finish in tiers and a launch with FEW rounds of waves ends in a
        long tail; relaunching the same kernel resets the ages (the state crosses HBM once per span: nothing at 128 steps).
        "auto": FUSED_SPAN_STEPS when the ensemble is between FUSED_SPAN_MIN_ROUNDS and FUSED_SPAN_MAX_ROUNDS rounds of resident
        waves, else one launch (profiles/r03/relaunch_sweep.txt).  Bit-identical either way.
        compensated (fp32 only, opt-in): modes 'fused' / 'ksteps' run the COMPENSATED form of the time-fused kernel
        (include/fiveeq.h, fiveeq_run_fused_comp_f32): every pool carries the rounding error of its own update in a second
        register word (no HBM bytes) and the forcing is computed from the excess C - C0 — worst error against 50-digit
        arithmetic C 2.9e-6 -> 1.8e-7, T 1.7e-5 -> 7e-7.  Its own arithmetic: not bit-identical to the default forms; the modes
        that keep the state in HBM between launches ('per_step', 'graph') refuse it; mode 'small' runs it one member per lane
        (fiveeq_run_small_comp_f32), which is what 'auto' takes for a launch-bound ensemble.
        small_lanes: mode='small' (no in-loop histograms): lanes per member, 4 (a lone 4-pool gas: one pool per lane of a
        quad), 8 (the 4 + 1 + 1 layout: one pool per lane of an octet; no collect_stats), 1 (any layout), or "auto" = the widest
        form the layout has while the ensemble is small enough for it (SMALL_*_MEMBERS_PER_CU), else 1.
        observations: a constrain.Observations table over this run's steps.  Every member then carries its misfit
        accumulators `misfit` [3, N] fp64 (A, U, V: include/fiveeq.h "CONSTRAINED RUNS") through modes 'per_step', 'graph',
        'fused' and 'ksteps' — the same bits in each, and C, T, R, S exactly as without it; `chi2()` scores the members.
        Pool layouts {4} and 4 + 1 + 1; not with compensated=True, concentration_driven=True or hist=, and never in mode
        'small' ('auto' takes 'per_step', 'ksteps' or 'fused' instead).
        SCENARIOS: `emissions` of shape [S, n_steps, G] (or a sequence of S [n_steps, G] arrays) advances every parameter
        member under each of the S emission scenarios (include/fiveeq.h "SCENARIOS"): member-scenario (m, s) is bit for bit
        member m of a one-scenario engine on scenario s.  The parameter rows are shared; R [S, SP, N], S [S, 2, N],
        C [S, n_rows, G, N], T [S, n_rows, N] and the statistics carry one slice per scenario (stats(), stats_sums(),
        gather_summary() and T_histogram() then take scenario=).  F_ext: [n_steps] (shared) or [S, n_steps]; R0 / S0: one
        [SP, N] / [2, N] state for every scenario, or [S, ...].  scenario_names: S labels (default "0", "1", ...).  Modes
        'per_step', 'graph', 'fused', 'ksteps' and 'auto' (never 'small'); not with concentration_driven=True, hist=,
        observations= or compensated=True.  `n_scenarios` is S (1 for an engine without the scenario axis).  With
        forcing=ScenarioForcings (below) every member-scenario also carries its member's forcing scales.
        forcing: a forcing.ExternalForcings table [n_steps, K] (K <= 4 categories, K = 0 allowed).  Every member then scales
        the forcing of gas g by params["f_scale"][g] and category k by params["fx_scale"][k] ([G] / [K] shared or [G, N] /
        [K, N] per member, default 1; include/fiveeq.h "FORCING SCALES"): F = F_ext + sum_k sx_k X[t, k] + sum_g sg_g F_g, every
        term one fma.  `fscale` [G + K, N] holds the rows, gas rows first.  Modes 'per_step', 'graph', 'fused', 'ksteps' and
        'auto' (never 'small'), the same bits in each; works with observations=, chunk-major schedules, the two-stream
        halves, step sub-ranges and R0 / S0; unit scales with K = 0 or a zero table are the plain run bit for bit.  Pool
        layouts {4} and 4 + 1 + 1; not with hist=, concentration_driven=True or compensated=True.
        WITH THE SCENARIO AXIS forcing= is a forcing.ScenarioForcings — one table per scenario, [S, n_steps, K], its
        n_scenarios the emissions' S — and the f_scale / fx_scale rows are shared by the scenarios: member-scenario (m, s) is bit
        for bit member m of a single-scenario forcing= engine on scenario s's emissions, F_ext and table, in every mode.  (One
        ExternalForcings table with several scenarios is refused: say ScenarioForcings.shared(fx, S) if that is what is meant.)
        uniform_rows: "auto" (the default) scans the parameter rows `r` [3G, N] and `q` [2, N] ONCE, here, for rows whose N
        members all hold the same bits (a parameter the study does not perturb; the structural zeros of the multi-gas
        defaults), and the plain per-step launches (modes 'per_step' and 'graph', step()) then take such a row's value from
        the kernel arguments instead of loading it at every step (include/fiveeq.h "SINGLE-VALUED PARAMETER ROWS"): w bytes
        less per member-step and row, the same bits.  `uniform_rows` names what was found, e.g. ("rC[1]", "rC[2]", "rT[2]").
        `r` and `q` are READ-ONLY after construction: nothing in the package writes into them (checkpoints restore state
        only, resampled() builds a new engine); a caller who overwrites them anyway calls refresh_uniform_rows() afterwards.
        False keeps every load.  Pool layouts without the form ({4} and 4 + 1 + 1 have it) and the other families (scenario
        axis, observations=, forcing=, hist=) report the rows and run as before.
        member_forcing: a tensor [n_steps, N] on the engine's device and in its dtype — a forcing series of each member's OWN
        that changes every step (include/fiveeq.h "MEMBER FORCING"): internal variability (forcing.ar1_noise_rows), the
        minor gases with each member's own lifetimes and radiative efficiencies (minor_gases.minor_gas_rows(...).rows; with
        into= on top of noise rows), or a member's own aerosol or volcanic history.  Step t of member m opens its forcing F = F_ext[t] + member_forcing[t, m]
        (one add), then the category and gas terms of forcing= as above.  Alone (unit scales, no category) or with forcing=
        and / or observations=; modes 'per_step', 'graph', 'fused', 'ksteps' and 'auto' (never 'small'), the same bits in each;
        all-zero rows are the forcing= run bit for bit.  The rows are kept as given (not copied when contiguous), are read-only
        to the engine, and take n_steps N w bytes; a checkpoint names them by sha256.  Pool layouts {4} and 4 + 1 + 1; not with
        the scenario axis, compensated=True, hist= or concentration_driven=True."""
        if dtype not in _DTYPES:
            raise ValueError("dtype must be torch.float64 or torch.float32")
        self.lib = _capi.load(lib_path)    # raises if the HIP library is not built
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the ensemble engine has no CPU fallback")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.type != "cuda":
            raise ValueError(f"device {self.device}: the engine runs on a GPU only")
        self.dtype = dtype
        self._sfx = _DTYPES[dtype]
        self._w = 8 if dtype == torch.float64 else 4
        self.n_members = N = int(n_members)
        if N < 1:
            raise ValueError("n_members must be >= 1")
        self.params = params
        self.n_gas = G = n_gas_of(params)
        self.pools = pools_of(params)
        self.sum_pools = SP = sum(self.pools)
        self.dt = float(dt)
        self.model = make_model(params, dt)
        n_pools = (ctypes.c_int32 * G)(*self.pools)
        if not self.lib.fiveeq_layout_supported(G, n_pools):
            raise _capi.FiveEqError(_capi.E_UNSUPPORTED, f"pool layout {self.pools} has no compiled kernel")
        self.small_widest = int(self.lib.fiveeq_small_lanes(G, n_pools))     # 4, 1, or 0 = the layout has no small-ensemble form

        if not store_trajectory:
            output_steps = []
        self.concentration_driven = bool(concentration_driven)
        self.compensated = bool(compensated)
        if self.compensated and (dtype != torch.float32 or self.concentration_driven):
            raise ValueError("compensated=True is an fp32 form of the emission-driven step (fp64 does not need it)")
        # the scenario axis: a 3-D emissions array or a sequence of 2-D ones (both of which make_drive refuses)
        self.scenario_axis = _is_scenario_set(emissions)
        if self.scenario_axis:
            if self.concentration_driven or hist is not None or observations is not None or self.compensated:
                raise ValueError("an engine with several emission scenarios runs the plain emission-driven forms only: not "
                                 "with concentration_driven=True, hist=, observations= or compensated=True")
            drive = make_scenario_drive(emissions, F_ext, dt, output_steps)
            self.n_scenarios = Sc = int(drive.shape[0])
            max_s = int(self.lib.fiveeq_max_scenarios())
            if Sc > max_s:
                raise ValueError(f"{Sc} scenarios: at most {max_s} per engine")
            names = [str(i) for i in range(Sc)] if scenario_names is None else [str(x) for x in scenario_names]
            if len(names) != Sc:
                raise ValueError(f"scenario_names: {len(names)} names for {Sc} scenarios")
            self.scenario_names = names
            self.drive_sha256 = emissions_sha256(drive)
            row_map = drive[0]
        else:
            if scenario_names is not None:
                raise ValueError("scenario_names= needs emissions of several scenarios ([S, n_steps, G])")
            drive = self._make_drive(emissions, F_ext, dt, output_steps)
            self.n_scenarios = Sc = 1
            self.scenario_names = None
            row_map = drive
        self.out_steps = np.nonzero(row_map[:, 7] >= 0)[0]          # step index of each stored row
        self.n_rows = int(self.out_steps.size)
        if drive[..., G:3].any():
            raise ValueError("emissions carry more gases than the parameter set")
        self.n_steps = int(row_map.shape[0])
        # the cumulative emissions at the END of each step, fp64 [(S,) n_steps, G] — what column 3 + g of step t + 1 holds, with
        # the last step's: the shared table of carbon_rows() (the columns of concentration-driven gases are not used)
        self._cum_end = np.cumsum(drive[..., :G] * float(dt), axis=-2)
        lead = (Sc,) if self.scenario_axis else ()          # the leading scenario axis of the state, rows and records

        dev, dt_ = self.device, dtype
        with torch.cuda.device(dev):
            self.drive = torch.from_numpy(drive).to(dev, dt_).contiguous()
            prm_rows = {k: _rows(params[k], G, N, k) for k in ("r0", "rC", "rT")}
            q_rows = _rows(params["q"], 2, N, "q")
            if any(isinstance(v, torch.Tensor) for v in list(prm_rows.values()) + [q_rows]):
                as_t = lambda v: v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, order="C"))  # noqa: E731
                self.r = torch.stack([as_t(prm_rows[k])[g].to(dev, dt_) for g in range(G) for k in ("r0", "rC", "rT")])
                self.q = as_t(q_rows).to(dev, dt_).contiguous()
            else:
                rows = np.concatenate([np.stack([prm_rows[k][g] for k in ("r0", "rC", "rT")]) for g in range(G)],
                                      axis=0)                                  # [3G, N]
                self.r = torch.from_numpy(np.array(rows, dtype=np.float64, order="C")).to(dev, dt_).contiguous()
                self.q = torch.from_numpy(np.array(q_rows, dtype=np.float64, order="C")).to(dev, dt_).contiguous()
            self.R = torch.zeros(lead + (SP, N), dtype=dt_, device=dev)
            self.S = torch.zeros(lead + (2, N), dtype=dt_, device=dev)
            # zero-filled, not torch.empty: rows of steps that were not run read as 0 rather than as stale
            # device memory (and the fill touches every page once, at construction)
            self.C = (torch.zeros(lead + (self.n_rows, G, N), dtype=dt_, device=dev)
                      if self.n_rows and (store_concentrations or concentration_driven) else None)
            self.T = torch.zeros(lead + (self.n_rows, N), dtype=dt_, device=dev) if self.n_rows else None
            self.cumE = torch.zeros((G, N), dtype=dt_, device=dev) if self.concentration_driven else None
            self.E = self.C if self.concentration_driven else None
            self.n_waves = int(self.lib.fiveeq_stats_waves(N))
            self.collect_stats = bool(collect_stats)
            self.T_stats = None          # per-wave records: 4.7 GB at 12.5M members x 750 steps, so allocated on demand
            # per-step (count, sum, sum^2, min, max) folded from the wave records: what a checkpoint's "summaries" carry
            self._step_sums = (torch.zeros(lead + (self.n_steps, 5), dtype=torch.float64, device=dev) if collect_stats else None)
            self._step_sums_valid = np.zeros(self.n_steps, dtype=bool)     # steps whose folded sums (above) are current
            # steps whose moments THIS engine holds (wave records written by its launches, or records / folded sums restored
            # from a checkpoint): only these are saved as valid by state_dict("summaries")
            self._stats_have = np.zeros(self.n_steps, dtype=bool)
            self.hist_spec = None
            self.T_hist = None
            if hist is not None:
                lo_h, hi_h, nb = float(hist[0]), float(hist[1]), int(hist[2])
                if not (hi_h > lo_h) or not 1 <= nb <= 4096:
                    raise ValueError("hist=(lo, hi, n_bins): need lo < hi and 1 <= n_bins <= 4096")
                if self.concentration_driven:
                    raise ValueError("in-loop histograms are not available in concentration-driven mode")
                self.hist_spec = (lo_h, hi_h, nb)
                self.T_hist = torch.zeros((self.n_steps, nb), dtype=torch.int64, device=dev)
            if hist_ring_steps == "auto":      # as long as 8 GB of 2-byte bin indices allow, at most 128 steps: every chunk
                hist_ring_steps = min(128, max(8, (8 << 30) // (4 * N)))     # boundary is a state + parameter round trip
            self.hist_ring_steps = max(1, min(int(hist_ring_steps), self.n_steps))
            # where the streamed pipeline's histogram pass runs: "side" = a second HIP stream beside the next chunk's fused
            # kernel, "same" = behind each chunk on the caller's stream
            self.hist_pass_stream = _env_choice("FIVEEQ_HIST_PASS_STREAM", "side", ("side", "same"))
            self._bins = None            # the bin-index ring, allocated by the first run that fills T_hist
            self.observations, self.obs, self.misfit = None, None, None
            if observations is not None:
                if self.compensated or (self.concentration_driven and not self._INVERSE_CALIBRATION) or hist is not None:
                    raise ValueError("observations= cannot be combined with compensated=True, concentration_driven=True or "
                                     "hist=: the misfit is carried by the plain forward forms only")
                if not self.lib.fiveeq_misfit_layout_supported(G, n_pools):
                    raise ValueError(f"observations=: pool layout {self.pools} has no misfit form (pools [4] and [4, 1, 1] have)")
                table = np.asarray(observations.table, dtype=np.float64)
                if table.shape != (self.n_steps, 4):
                    raise ValueError(f"observations: table of {table.shape[0]} steps for a run of {self.n_steps}")
                self.observations = observations
                self.obs = torch.from_numpy(np.array(table, order="C")).to(dev)      # uploaded once
                self.misfit = torch.zeros((3, N), dtype=torch.float64, device=dev)
            self.forcing, self.fscale, self.fext = None, None, None
            if forcing is not None:
                for flag, why in ((hist is not None, "hist="),
                                  (self.concentration_driven and not self._INVERSE_CALIBRATION, "concentration_driven=True"),
                                  (self.compensated, "compensated=True")):
                    if flag:
                        raise ValueError(f"forcing= cannot be combined with {why}: the forcing scales are carried by the plain "
                                         "forward forms (with or without observations=, or with the scenario axis) only")
                per_scenario = isinstance(forcing, ScenarioForcings)
                if self.scenario_axis and not per_scenario:
                    raise ValueError("forcing= with emissions of several scenarios (the scenario axis) takes one table per "
                                     "scenario: pass a forcing.ScenarioForcings (ScenarioForcings.shared(fx, S) for one table "
                                     "under every scenario), not an ExternalForcings")
                if per_scenario and not self.scenario_axis:
                    raise ValueError("forcing=ScenarioForcings needs emissions of several scenarios ([S, n_steps, G]); a run of "
                                     "one scenario takes an ExternalForcings (ScenarioForcings.scenario(s))")
                if per_scenario and forcing.n_scenarios != Sc:
                    raise ValueError(f"forcing: tables of {forcing.n_scenarios} scenarios for emissions of {Sc}")
                if not self.lib.fiveeq_forcing_layout_supported(G, n_pools):
                    raise ValueError(f"forcing=: pool layout {self.pools} has no forcing form (pools [4] and [4, 1, 1] have)")
                if forcing.n_steps != self.n_steps:
                    raise ValueError(f"forcing: table of {forcing.n_steps} steps for a run of {self.n_steps}")
                Kx = forcing.n_categories
                self.forcing = forcing
                self.fext = torch.from_numpy(forcing.padded()).to(dev, dt_).contiguous()          # uploaded once
                rows = [_rows(params.get("f_scale", np.ones(G)), G, N, "f_scale")]
                if Kx:
                    rows.append(_rows(params.get("fx_scale", np.ones(Kx)), Kx, N, "fx_scale"))
                elif "fx_scale" in params and np.size(params["fx_scale"]):
                    raise ValueError("fx_scale given, but the forcing table has no category")
                as_t = lambda v: (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, order="C"))).to(dev, dt_)  # noqa: E731
                self.fscale = torch.cat([as_t(v) for v in rows]).contiguous()                   # [G + K, N], gas rows first
                if not bool(torch.isfinite(self.fscale).all()):
                    raise ValueError("f_scale / fx_scale: non-finite scale factors")
            elif "f_scale" in params or "fx_scale" in params:
                raise ValueError("f_scale / fx_scale need forcing= (ExternalForcings; a table without categories will do)")
            self.member_forcing, self._unit_fscale = None, None
            if member_forcing is not None:
                for flag, why in ((self.scenario_axis, "emissions of several scenarios (the scenario axis)"),
                                  (self.compensated, "compensated=True"), (hist is not None, "hist="),
                                  (self.concentration_driven, "concentration_driven=True")):
                    if flag:
                        raise ValueError(f"member_forcing= cannot be combined with {why}: the per-member forcing rows are "
                                         "carried by the plain forward forms (with or without forcing= and observations=) only")
                if not self.lib.fiveeq_forcing_layout_supported(G, n_pools):
                    raise ValueError(f"member_forcing=: pool layout {self.pools} has no member-forcing form (pools [4] and "
                                     "[4, 1, 1] have)")
                mf = member_forcing
                if (not isinstance(mf, torch.Tensor) or tuple(mf.shape) != (self.n_steps, N) or mf.dtype != dt_
                        or mf.device != dev):
                    raise ValueError(f"member_forcing: want a tensor of shape [{self.n_steps}, {N}] ({dt_}) on {dev}")
                self.member_forcing = mf.contiguous()
                if self.fscale is None:                          # without forcing=: unit gas scales, no category
                    self._unit_fscale = torch.ones((G, N), dtype=dt_, device=dev)
        n_frows = self._n_scale_rows()
        if chunk_members == "auto":
            chunk_members = self.auto_chunk(N, SP, G, dtype, n_scenarios=Sc, extra_rows=n_frows)
        self.chunk_members = int(chunk_members or 0) // 256 * 256
        if per_step_streams == "auto":
            t_step = (min(N, self.chunk_members or N) * self._w * (Sc * (2 * SP + G + 5) + 3 * G + 2 + n_frows)
                      / HBM_STREAM_BYTES_PER_S)
            per_step_streams = 2 if t_step >= PER_STEP_SPLIT_MIN_S else 1
        self.per_step_streams = max(1, int(per_step_streams))
        if fused_span not in ("auto", None) and int(fused_span) < 1:
            raise ValueError("fused_span must be 'auto', None or a positive number of steps")
        self.fused_span = fused_span if fused_span in ("auto", None) else int(fused_span)
        if small_lanes != "auto" and int(small_lanes) not in (1, 4, 8):
            raise ValueError("small_lanes must be 'auto', 1, 4 or 8")
        self.small_lanes = small_lanes if small_lanes == "auto" else int(small_lanes)
        # run(..., join=False) left work nobody has waited for: the streams of THAT run ([its main, its side streams]) — join()
        # waits for exactly these, whichever stream the consumer is on; None = nothing outstanding
        self._ps_unjoined = None
        self._R0 = None if R0 is None else self._initial_state(R0, SP, "R0")
        self._S0 = None if S0 is None else self._initial_state(S0, 2, "S0")
        self.t_next = 0                     # first step not yet run (bookkeeping for checkpoints)
        self.last_mode = None               # the mode the last run() used after resolving 'auto'
        self.reset_state()
        self._plans = {}
        if uniform_rows not in ("auto", False):
            raise ValueError("uniform_rows must be 'auto' or False")
        self._uniform_auto = uniform_rows == "auto"
        self.refresh_uniform_rows()
        with torch.cuda.device(self.device):
            self.probe_streams()            # construction is synchronous anyway: the one place the probe may clock streams

    def _make_drive(self, emissions, F_ext, dt, output_steps):
        """The drive table [n_steps, 8] of an engine without the scenario axis (MixedDriveEngine builds its per-gas form)."""
        return make_drive(emissions, F_ext, dt, output_steps, self.concentration_driven)

    def _scale_rows(self):
        """The scale rows the forcing kernels load: `fscale` of forcing=, or the unit rows of a member_forcing= engine without
        it; None for an engine with neither."""
        return self.fscale if self.fscale is not None else self._unit_fscale

    def _n_scale_rows(self):
        rows = self._scale_rows()
        return 0 if rows is None else int(rows.shape[0])

    def refresh_uniform_rows(self):
        """Scan `r` and `q` again for single-valued rows (fiveeq_uniform_rows_*: one device pass, synchronous) — for a caller
        who wrote into them after construction.  Drops the captured plans, which carry the old rows.  Returns `uniform_rows`;
        () with uniform_rows=False."""
        self.close()
        G = self.n_gas
        self._uniform_mask = 0
        self._uniform_values = ((ctypes.c_double if self._w == 8 else ctypes.c_float) * (3 * G + 2))()
        if self._uniform_auto:
            mask = ctypes.c_uint32(0)
            with torch.cuda.device(self.device):
                rc = self._fn("uniform_rows")(self.n_members, self.n_members, 3 * G, self._ptr(self.r), self._ptr(self.q),
                                              ctypes.byref(mask), self._uniform_values, self._stream())
            _capi.check(self.lib, rc)
            self._uniform_mask = int(mask.value)
        names = [f"{k}[{g}]" for g in range(G) for k in ("r0", "rC", "rT")] + ["q[0]", "q[1]"]
        self.uniform_rows = tuple(name for i, name in enumerate(names) if self._uniform_mask >> i & 1)
        return self.uniform_rows

    def _initial_state(self, x, K, name):
        """R0 / S0 as a host fp64 array: [K, N], or with the scenario axis [S, K, N] (a [K, N] state broadcast to every
        scenario)."""
        if isinstance(x, torch.Tensor):
            x = x.detach().double().cpu().numpy()
        x = np.asarray(x, dtype=np.float64)
        N = self.n_members
        if not self.scenario_axis:
            return x.reshape(K, N)
        if x.size == K * N:
            return np.broadcast_to(x.reshape(1, K, N), (self.n_scenarios, K, N)).copy()
        if x.shape != (self.n_scenarios, K, N):
            raise ValueError(f"{name}: shape {x.shape}, want [{K}, {N}] or [{self.n_scenarios}, {K}, {N}]")
        return x

    def _scen(self, scenario):
        """The scenario index a per-scenario accessor reads: required with the scenario axis, ignored without it."""
        if not self.scenario_axis:
            return None
        if scenario is None:
            raise ValueError(f"this engine runs {self.n_scenarios} scenarios: pass scenario= (0..{self.n_scenarios - 1})")
        s = int(scenario)
        if not 0 <= s < self.n_scenarios:
            raise ValueError(f"scenario {scenario}: the engine has scenarios 0..{self.n_scenarios - 1}")
        return s

    @staticmethod
    def auto_chunk(n_members, sum_pools, n_gas, dtype, cache_bytes=INFINITY_CACHE_BYTES, n_scenarios=1, extra_rows=0):
        """Members per chunk of the chunk-major schedule: the fewest EVEN chunks whose state + parameter rows take at most
        CHUNK_CACHE_SHARE of the Infinity Cache each (a multiple of 256 members); 0 = do not chunk: the ensemble's rows fit the
        cache by themselves.  With n_scenarios, every member carries that many copies of the state rows; extra_rows: further
        parameter rows per member (the forcing scales)."""
        w = 8 if dtype == torch.float64 else 4
        rows_bytes = n_members * w * (n_scenarios * (sum_pools + 2) + 3 * n_gas + 2 + extra_rows)
        if rows_bytes <= cache_bytes:
            return 0
        k = -(-rows_bytes // int(CHUNK_CACHE_SHARE * cache_bytes))
        return -(-n_members // (256 * k)) * 256

    def fused_span_steps(self, n_steps):
        """Steps per launch mode='fused' uses for a request of n_steps steps (see fused_span); n_steps = one launch."""
        n_steps = int(n_steps)
        if self.fused_span is None or n_steps <= 1:
            return n_steps
        if self.fused_span != "auto":
            return min(self.fused_span, n_steps)
        # packed fp32 lanes carry two members (with observations= only the 4 + 1 + 1 layout has a packed fused form)
        packs = self.dtype == torch.float32 and self.n_members % 2 == 0 and (self.observations is None or self.pools == [4, 1, 1])
        per_wave = 128 if packs else 64
        slots = 16 * torch.cuda.get_device_properties(self.device).multi_processor_count       # 4 waves on each of a CU's 4 SIMDs
        rounds = -(-self.n_members // per_wave) * self.n_scenarios / slots          # the scenarios are rows of the grid
        # (below a quarter of a round the launches themselves weigh more than the tail: 10k members lose 3 %)
        return min(FUSED_SPAN_STEPS, n_steps) if FUSED_SPAN_MIN_ROUNDS <= rounds <= FUSED_SPAN_MAX_ROUNDS else n_steps

    def auto_k_steps(self):
        """Steps per launch of the per-step family: 1 (the per-step kernel, the north-star form) while one step's HBM traffic
        hides the dependent-launch boundary (at least three boundaries' worth: ~160k three-gas fp64 members), otherwise —
        the ensemble is launch-bound, not bandwidth-bound — KSTEPS_LAUNCH_BOUND: state and parameters cross HBM once per
        launch, so nothing is gained by a shorter span (round 4 scaled K with the ensemble and ran 110k members at K = 2)."""
        t_step = self.n_members * self.n_scenarios * self.bytes_per_member_step("per_step") / HBM_STREAM_BYTES_PER_S
        return 1 if t_step >= 3.0 * LAUNCH_BOUNDARY_S else min(KSTEPS_LAUNCH_BOUND, self.n_steps)

    def mode_refusal(self, mode):
        """Why this engine does not run in `mode` (one of MODES but 'auto'): the text run() raises, or None.  THE statement of
        which modes serve which features; where several apply, the first in this order is reported."""
        forward = ("per_step", "graph", "fused", "ksteps")       # every mode but 'small'
        rules = (
            (self.T_hist is not None, ("fused", "per_step"),
             f"mode {mode!r} does not fill T_hist: use 'fused' or 'per_step' with hist="),
            (self.compensated, ("fused", "ksteps", "small"),
             f"mode {mode!r} has no compensated form: the compensation words live in registers, so only the "
             "time-fused kernel ('fused', 'ksteps') and the small-ensemble kernel ('small', one lane) carry them"),
            (self.scenario_axis, forward,
             "mode 'small' has no scenario form: use 'per_step', 'graph', 'fused', 'ksteps' or 'auto'"),
            (self.forcing is not None, forward,
             "mode 'small' does not carry the forcing scales of forcing=: use 'per_step', 'graph', 'fused', 'ksteps' or 'auto'"),
            (self.observations is not None, forward,
             "mode 'small' does not carry the misfit of observations=: use 'per_step', 'graph', 'fused', 'ksteps' or 'auto'"),
            (self.member_forcing is not None, forward,
             "mode 'small' does not carry the per-member forcing rows of member_forcing=: use 'per_step', 'graph', 'fused', "
             "'ksteps' or 'auto'"),
        )
        return next((text for has, modes, text in rules if has and mode not in modes), None)

    def small_form(self):
        """Lanes per member mode='small' would run with now (4 or 1); 0 = the small-ensemble kernel does not apply: a feature
        that mode does not serve (mode_refusal), the concentration-driven form, or a layout or small_lanes without one."""
        if not self.small_widest or self.concentration_driven or self.mode_refusal("small"):
            return 0
        if self.compensated:                                     # fiveeq_run_small_comp_f32: one member per lane, every layout
            return 1 if self.small_lanes in ("auto", 1) else 0
        octet_ok = self.small_widest == 8 and not self.collect_stats       # the octet form writes no per-wave statistics
        if self.small_lanes != "auto":
            if self.small_lanes == 8:
                return 8 if octet_ok else 0
            return self.small_lanes if self.small_lanes in (1, self.small_widest) else 0
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        if self.small_widest == 4 and self.n_members <= SMALL_QUAD_MEMBERS_PER_CU * cus:
            return 4
        if octet_ok and self.n_members <= SMALL_OCTET_MEMBERS_PER_CU * cus:
            return 8
        return 1

    def resolve_mode(self, mode, k_steps=None):
        """(mode, k_steps) run() uses for a request: 'auto' resolved, everything else as given.  'auto' is 'per_step' (the
        north-star form) while a step's HBM traffic hides the launch boundary; a launch-bound ensemble takes the small-ensemble
        kernel (small_form()) — or, with hist=, 'fused' (the streamed histogram pipeline, the fastest form that fills T_hist
        there: profiles/r04/auto_hist_table.txt); an explicit k_steps, or a run the small kernel does not serve, 'ksteps'."""
        if mode != "auto":
            return mode, k_steps
        if self.compensated:                                     # the compensation words live in registers: the time-fused kernel,
            launch_bound = (self.auto_k_steps() if k_steps is None else int(k_steps)) > 1     # or the small-ensemble one (one lane)
            return ("small" if launch_bound and k_steps is None and self.small_form() else "fused"), None
        k = self.auto_k_steps() if k_steps is None else int(k_steps)
        if k <= 1:
            return "per_step", None
        if self.T_hist is not None:
            return "fused", None
        if k_steps is None and self.small_form():
            return "small", None
        return "ksteps", k

    # -- state -------------------------------------------------------------------------
    def reset_state(self):
        """Back to the initial condition (zeros, or the R0/S0 given at construction) — the run accumulators too:
        `T_hist` ACCUMULATES over the runs that fill it (a step histogrammed twice counts twice), so it is zeroed here,
        and the per-step moment records are marked not-yet-written."""
        if self._ps_unjoined:
            self.join()
        if self._R0 is None:
            self.R.zero_()
        else:
            self.R.copy_(torch.from_numpy(self._R0).to(self.dtype))
        if self._S0 is None:
            self.S.zero_()
        else:
            self.S.copy_(torch.from_numpy(self._S0).to(self.dtype))
        if self.cumE is not None:
            self.cumE.zero_()
        if self.misfit is not None:
            self.misfit.zero_()
        if self.T_hist is not None:
            self.T_hist.zero_()
        self._step_sums_valid[:] = False
        self._stats_have[:] = False
        self.t_next = 0

    def _wave_stats(self):
        """The per-wave record buffer of the in-kernel statistics, allocated by the first launch that writes it."""
        if self.collect_stats and self.T_stats is None:
            lead = (self.n_scenarios,) if self.scenario_axis else ()
            self.T_stats = torch.zeros(lead + (self.n_waves, self.n_steps, 4), dtype=torch.float64, device=self.device)
        return self.T_stats

    # -- launches ----------------------------------------------------------------------
    def _stream(self, stream=None):
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(s.cuda_stream)

    def _ptr(self, t, byte_off=0):
        return ctypes.c_void_p(0 if t is None else t.data_ptr() + byte_off)

    def _run_args(self, t_begin, t_end, m0=0, n=None, *, n_scen=None, cumE=None):
        """C-ABI arguments (model ... T_stats) for members [m0, m0 + n) of this engine's rows (ld = N), with the two that some
        entry points take in between at their places: n_scen (the scenario families, after ld) and cumE (the inverse form,
        after S)."""
        N, w = self.n_members, self._w
        n = N if n is None else n
        return (ctypes.byref(self.model), n, N, *(() if n_scen is None else (n_scen,)), self._ptr(self.drive), self.n_steps,
                int(t_begin), int(t_end), self._ptr(self.r, m0 * w), self._ptr(self.q, m0 * w), self._ptr(self.R, m0 * w),
                self._ptr(self.S, m0 * w), *(() if cumE is None else (cumE,)), self._ptr(self.C, m0 * w),
                self._ptr(self.T, m0 * w), self.n_rows, self._ptr(self.T_stats, (m0 // 64) * self.n_steps * 4 * 8))

    def _fn(self, name):
        return getattr(self.lib, f"fiveeq_{name}_{self._sfx}")

    def _chunks(self):
        N, c = self.n_members, self.chunk_members
        if not c or c >= N:
            return [(0, N)]
        return [(m0, min(c, N - m0)) for m0 in range(0, N, c)]

    def _obs_args(self, m0=0):
        """(obs, misfit) C-ABI pointers for members [m0, ...) of the misfit rows (ld = N)."""
        return self._ptr(self.obs), self._ptr(self.misfit, m0 * 8)

    def _forward_calls(self):
        """The C calls of this engine's forward run, with the arguments of its feature bound: n_scen (the scenario axis, whose
        strides derive from ld = N), (obs, misfit) (observations=), (fscale, fext, n_fext) (forcing=, after n_scen's or before
        the misfit's), (mforc, n_mforc_rows) (member_forcing=, behind the misfit's: fiveeq_run_mforc, which takes fiveeq_run_forc's
        arguments first — unit scale rows and no category without forcing=) or none.  Returns
          per_step(t_begin, t_end, m0, n, stream)  one launch per step for members [m0, m0 + n);
          fused(t_begin, t_end, k, stream)         the fused kernel over spans of k steps, all members;
          plan(t_begin, t_end, m0, n, plan_out)    the per-step launches of members [m0, m0 + n) captured into a plan."""
        scen, obs, mforc = self.scenario_axis, self.observations is not None, self.member_forcing is not None
        forc = self.forcing is not None or mforc

        def args(t_begin, t_end, m0=0, n=None):
            a = self._run_args(t_begin, t_end, m0, n, n_scen=self.n_scenarios if scen else None)
            if forc:                                            # with scenarios: the scale rows shared, the tables [S, n_steps, 4]
                a += (self._ptr(self._scale_rows(), m0 * self._w), self._ptr(self.fext),
                      0 if self.forcing is None else self.forcing.n_categories)
            if obs:
                a += self._obs_args(m0)
            elif forc and not scen:                             # fiveeq_run_forc's (obs, misfit): both NULL without observations=
                a += (None, None)
            if mforc:
                a += (self._ptr(self.member_forcing, m0 * self._w), self.n_steps)
            return a

        if scen or forc or obs:
            sfx = "mforc" if mforc else "_".join(
                word for word, on in (("scen", scen), ("forc", forc), ("obs", obs and not forc)) if on)
            run, plan = self._fn("run_" + sfx), self._fn("plan_create_" + sfx)

            def per_step(t, t1, m0, n, s):
                return run(*args(t, t1, m0, n), _capi.FORM_PER_STEP, 0, self._stream(s))

            def fused(t, t1, k, s):
                return run(*args(t, t1), _capi.FORM_FUSED, int(k), self._stream(s))
        else:
            run_fused, ksteps = self._fn("run_fused"), self._fn("run_ksteps")
            # the per-step call and its plan: the uniform twins, which skip the loads of the single-valued rows (mask 0:
            # today's launches); uniform_rows=False keeps today's calls
            uni = (self._uniform_mask, self._uniform_values) if self._uniform_auto else ()
            run = self._fn("run_uniform" if uni else "run")
            create = self._fn("plan_create_uniform" if uni else "plan_create")

            def per_step(t, t1, m0, n, s):
                return run(*args(t, t1, m0, n), *uni, self._stream(s))

            def plan(*a):
                return create(*a[:-1], *uni, a[-1])

            def fused(t, t1, k, s):                             # k < 1 (an empty range): run_ksteps would refuse it
                return ksteps(*args(t, t1), int(k), self._stream(s)) if k >= 1 else run_fused(*args(t, t1), self._stream(s))

        return per_step, fused, lambda t, t1, m0, n, out: plan(*args(t, t1, m0, n), out)

    def _span_steps(self, mode, t_begin, t_end, k_steps):
        """Steps per launch of the time-fused kernel in mode 'fused' (fused_span_steps) or 'ksteps' (k_steps, default
        auto_k_steps())."""
        if mode == "fused":
            return self.fused_span_steps(t_end - t_begin)
        return max(self.auto_k_steps() if k_steps is None else int(k_steps), 1)

    def _run_inverse(self, t_begin, t_end, stream):
        return self._fn("run_inverse")(*self._run_args(t_begin, t_end, cumE=self._ptr(self.cumE)), self._stream(stream))

    def step(self, t, stream=None):
        """One timestep = one kernel launch (asynchronous)."""
        t = int(t)
        if self._ps_unjoined:                         # a run(..., join=False) may still be writing R, S, T_stats on the side streams
            self.join(stream)
        self._step_sums_valid[t] = False              # this launch writes the step's wave record: older folded moments are stale
        if self.collect_stats:
            self._stats_have[t] = True
        self._wave_stats()
        with torch.cuda.device(self.device):
            if self.concentration_driven:
                rc = self._run_inverse(t, t + 1, stream)
            else:
                rc = self._forward_calls()[0](t, t + 1, 0, None, stream)
        _capi.check(self.lib, rc)
        self.t_next = t + 1

    def run(self, t_begin=0, t_end=None, mode="per_step", stream=None, k_steps=None, join=True):
        """Advance steps [t_begin, t_end).  mode:
        'per_step' one launch per timestep, enqueued from C (the north-star form);
        'graph'    the same launches replayed from a captured hipGraph;
        'fused'    one launch, state in registers across all steps (with `hist=`: chunks of hist_ring_steps steps, T_hist
                   filled by the streamed pipeline, see __init__);
        'ksteps'   the fused kernel over consecutive spans of `k_steps` steps (default `auto_k_steps()`):
                   state crosses HBM once per k_steps — the per-step family's answer for launch-bound ensembles;
        'small'    the small-ensemble kernel (see small_lanes): the model in registers, one launch; a lone 4-pool gas: one member
                   per quad of lanes;
        'auto'     see resolve_mode().
        Every mode gives bit-identical results.
        join=False (mode 'per_step' on several streams only): do not make the caller's stream wait for the side streams at
        the end, and do not make the side streams wait for the caller's stream at the start of the NEXT such call — for
        back-to-back calls with nothing in between that touches the state on the caller's stream (bench.py's repeated
        blocks): a join is two cross-stream hops, ~20 us.  Call `join()` before anything consumes the results."""
        t_begin, t_end = int(t_begin), self.n_steps if t_end is None else int(t_end)
        if self._ps_unjoined and mode != "per_step":
            self.join(stream)
        mode, k_steps = self.resolve_mode(mode, k_steps)
        self.last_mode = mode            # what 'auto' resolved to (tests, bench.py's config.mode)
        if mode not in self.MODES:
            raise ValueError(f"unknown mode {mode!r}")
        refusal = self.mode_refusal(mode)
        if refusal:
            raise ValueError(refusal)
        if mode == "small" and not self.small_form():
            raise ValueError("mode 'small' serves runs without in-loop histograms or the inverse form, with 4 lanes per "
                             "member for a lone 4-pool gas only and 8 for pools [4, 1, 1] without collect_stats "
                             f"(pools {self.pools}, small_lanes={self.small_lanes!r})")
        with torch.cuda.device(self.device):
            self._wave_stats()
            self._step_sums_valid[t_begin:t_end] = False     # these launches write per-wave records: older folded sums are stale
            if self.collect_stats:
                self._stats_have[t_begin:t_end] = True
            if self.concentration_driven:
                rc = self._run_inverse(t_begin, t_end, stream)
            elif mode == "per_step":
                rc = self._run_per_step(t_begin, t_end, stream, join)
            elif mode == "fused" and self.T_hist is not None:
                rc = self._run_fused_bin_ring(t_begin, t_end, stream)
            elif mode == "small" and self.compensated:
                rc = self.lib.fiveeq_run_small_comp_f32(*self._run_args(t_begin, t_end), self._stream(stream))
            elif mode == "small":
                rc = self._fn("run_small")(*self._run_args(t_begin, t_end), self.small_form(), self._stream(stream))
            elif mode in ("fused", "ksteps"):                    # without a ring: one C call, the kernel relaunched every span
                span = self._span_steps(mode, t_begin, t_end, k_steps)
                if self.compensated:
                    rc = self.lib.fiveeq_run_fused_comp_f32(*self._run_args(t_begin, t_end), span, 0.0, 1.0, 1, None, 0,
                                                            self._stream(stream))
                else:
                    rc = self._forward_calls()[1](t_begin, t_end, span, stream)
            else:                                                # 'graph': one captured plan per (chunk, part), the parts of a
                plans = self.prepare_graph(t_begin, t_end)       # chunk replayed side by side on their own streams
                rc = self._on_part_streams(stream, True, lambda streams: self._first_error(
                    self.lib.fiveeq_plan_launch(plan, self._stream(streams[si]))
                    for plan, (_, _, si) in zip(plans, self.per_step_launches())))
        _capi.check(self.lib, rc)
        self.t_next = t_end

    @staticmethod
    def _first_error(codes):
        """The first non-zero return code of a sequence of C calls, which stops at it (a generator: later calls are not made)."""
        for rc in codes:
            if rc != _capi.OK:
                return rc
        return _capi.OK

    def per_step_launches(self):
        """[(first member, members, stream index)] of the kernels mode='per_step' launches for ONE timestep, in launch order:
        member chunks run one after the other (chunk-major, see chunk_members), the parts of a chunk side by side on
        per_step_streams streams (stream 0 = the caller's)."""
        out = []
        for m0, n in self._chunks():
            k = self.per_step_streams if n >= 512 * self.per_step_streams else 1
            cuts = [m0 + (i * n // k) // 256 * 256 for i in range(k)] + [m0 + n]
            out += [(cuts[i], cuts[i + 1] - cuts[i], i) for i in range(k)]
        return out

    def per_step_stream_list(self, stream=None):
        """The HIP streams mode='per_step' launches on: the caller's, then the side streams of the other parts."""
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        n_streams = 1 + max(i for _, _, i in self.per_step_launches())
        if n_streams == 1:
            return [main]
        # side streams PROBED to run beside `main` (a stream that shares main's hardware queue serialises the parts, +12 % per
        # step): probed at construction / by probe_streams(), never here — an unprobed main gets plain streams (tuning.py)
        return [main] + concurrent_side_streams(self.lib, main, n_streams - 1)

    def join(self, stream=None):
        """Make `stream` (default: the current stream) wait for everything run(..., join=False) left outstanding — on the
        streams THAT run used: its side streams and, when the consumer is another stream than the run's main, that main too."""
        pending, self._ps_unjoined = self._ps_unjoined, None
        if pending:
            consumer = stream if stream is not None else torch.cuda.current_stream(self.device)
            for s in pending:
                if s.cuda_stream != consumer.cuda_stream:
                    consumer.wait_stream(s)

    def probe_streams(self, stream=None):
        """Probe (tuning.concurrent_side_streams, probe=True) side streams for `stream` (default: the current one) so that the
        two-stream schedules launched from it really overlap.  SYNCHRONISES that stream: call it where that is harmless — the
        constructor does, for the stream current at construction; a caller that runs the engine on another stream of its own
        calls this once before its first run().  Returns side_stream_report()."""
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        want = self._side_streams_wanted()
        if want:
            if self._ps_unjoined:
                self.join(main)
            concurrent_side_streams(self.lib, main, want, probe=True)
        return self.side_stream_report(main)

    def _side_streams_wanted(self):
        n = max(i for _, _, i in self.per_step_launches())
        if self.T_hist is not None and self.hist_pass_stream == "side":
            n = max(n, 1)
        return n

    def side_stream_report(self, stream=None):
        """{"wanted", "probed", "passed", "candidates_tried", "probe_enabled"} for the side streams runs on `stream` use."""
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        want = self._side_streams_wanted()
        return {"wanted": want, **side_stream_report(main, want)}

    def _on_part_streams(self, stream, join, body):
        """Run body(streams) with the side streams ordered behind the caller's stream before it and (join=True) the caller's
        stream ordered behind them after it — the frame of every form that runs the parts of a chunk side by side."""
        streams = self.per_step_stream_list(stream)
        if self._ps_unjoined and [s.cuda_stream for s in self._ps_unjoined] != [s.cuda_stream for s in streams]:
            self.join(streams[0])                                # an unjoined run on OTHER streams: order this one behind it
        if not self._ps_unjoined:
            for s in streams[1:]:
                s.wait_stream(streams[0])                        # the state may have been touched on the caller's stream
        rc = body(streams)
        if len(streams) > 1:
            if join:
                for s in streams[1:]:
                    streams[0].wait_stream(s)
            self._ps_unjoined = None if join else list(streams)
        return rc

    def _per_step_schedule(self, t_begin, t_end, stream, join, block, launch):
        """The launch order of the per-step family: member chunks one after the other (chunk-major), within a chunk blocks of
        steps [t, t1) — t1 the next multiple of `block` past t (block = None: the whole range at once) — and within a block
        the parts of the chunk side by side, `launch(t, t1, m0, n, stream)` for each on its own stream."""
        layout = self.per_step_launches()
        firsts = [i for i, (_, _, si) in enumerate(layout) if si == 0] + [len(layout)]

        def body(streams):
            for a, b in zip(firsts[:-1], firsts[1:]):
                t = t_begin
                while t < t_end:
                    t1 = t_end if block is None else min(t_end, (t // block + 1) * block)
                    for m0, n, si in layout[a:b]:
                        rc = launch(t, t1, m0, n, streams[si])
                        if rc != _capi.OK:
                            return rc
                    t = t1
            return _capi.OK

        return self._on_part_streams(stream, join, body)

    def _run_per_step(self, t_begin, t_end, stream, join=True):
        """fiveeq_run_*: one launch per timestep and member part, enqueued from C.  With T_hist: fiveeq_run_bins_*, whose
        kernel also writes every member's histogram bin into a ring strip [S, N] of uint16 (row t mod S); after S steps each
        part counts its strip into T_hist (fiveeq_hist_bins) on its own stream — 2 bytes written + 2 read per member-step on
        top of the step's 124 / 248."""
        if self.T_hist is None:                                  # (hist= is never combined with the scenario axis or observations=)
            # several streams: short blocks keep every stream's queue fed; one stream: one C call per chunk
            block = PER_STEP_BLOCK if self.per_step_streams > 1 else None
            return self._per_step_schedule(t_begin, t_end, stream, join, block, self._forward_calls()[0])
        N, (lo_h, hi_h, nb) = self.n_members, self.hist_spec
        ring = self._bin_ring(slots=1)
        S, buf, run = ring["S"], ring["buf"][0], self._fn("run_bins")

        def launch(t, t1, m0, n, s):
            st = self._stream(s)
            return (run(*self._run_args(t, t1, m0, n), lo_h, hi_h, nb, self._ptr(buf, m0 * 2), S, st)
                    or self.lib.fiveeq_hist_bins(t1 - t, n, N, self._ptr(buf[t % S], m0 * 2), nb, self._ptr(self.T_hist[t:t1]), st))

        return self._per_step_schedule(t_begin, t_end, stream, True, S, launch)

    def _bin_ring(self, slots=2):
        """Ring [slots, S, N] of uint16 bin indices for the streamed histograms: mode 'fused' double-buffers (two slots), mode
        'per_step' counts each strip right behind its steps (one slot: half the memory); grown to two slots when a fused
        run follows a per-step one, rebuilt when hist_ring_steps changed."""
        N, S, dev = self.n_members, max(1, min(int(self.hist_ring_steps), self.n_steps)), self.device
        ring = self._bins
        if ring is None or ring["S"] != S or ring["buf"].shape[0] < slots:
            torch.cuda.synchronize(dev)
            self._bins = None
            self._bins = ring = {"S": S, "buf": torch.empty((slots, S, N), dtype=torch.int16, device=dev),
                                 "drained": [torch.cuda.Event(), torch.cuda.Event()]}
        return ring

    def _run_fused_bin_ring(self, t_begin, t_end, stream):
        """mode='fused' with hist=: chunks of S = hist_ring_steps steps.  Stream A (the caller's) runs
        fiveeq_run_fused_bins_* for chunk i: the ordinary fused kernel — stored C/T rows and per-wave statistics exactly as
        in a plain fused run — that also writes every member's histogram bin of every step into ring slot i % 2 (row t mod
        S).  Stream B waits for the chunk and counts the slot's rows into T_hist[t:t+S] (fiveeq_hist_bins); A reuses a slot
        only after B has drained it."""
        N, dev = self.n_members, self.device
        ring = self._bin_ring()
        S = ring["S"]
        main = stream if stream is not None else torch.cuda.current_stream(dev)
        side = main if self.hist_pass_stream == "same" else concurrent_side_streams(self.lib, main, 1)[0]
        side.wait_stream(main)
        lo_h, hi_h, nb = self.hist_spec

        def fused(t, t1, *ring):                                 # compensated: one launch per chunk either way, k_steps = the chunk
            a = self._run_args(t, t1)
            return (self.lib.fiveeq_run_fused_comp_f32(*a, t1 - t, *ring) if self.compensated
                    else self._fn("run_fused_bins")(*a, *ring))

        used = [False, False]
        rc, t, i = _capi.OK, t_begin, 0
        while t < t_end and rc == _capi.OK:
            t1 = min(t_end, (t // S + 1) * S)              # chunks end on multiples of S: row = t mod S never wraps
            slot = i % 2
            buf = ring["buf"][slot]
            if used[slot]:
                main.wait_event(ring["drained"][slot])
            rc = fused(t, t1, lo_h, hi_h, nb, self._ptr(buf), S, self._stream(main))
            side.wait_stream(main)
            if rc == _capi.OK:
                rc = self.lib.fiveeq_hist_bins(t1 - t, N, N, self._ptr(buf[t % S:]), nb, self._ptr(self.T_hist[t:t1]),
                                               self._stream(side))
                ring["drained"][slot].record(side)
                used[slot] = True
            t, i = t1, i + 1
        main.wait_stream(side)
        return rc

    def prepare_graph(self, t_begin=0, t_end=None):
        """Capture (once) the per-step launches of [t_begin, t_end) into hipGraph plans, one per launch of
        `per_step_launches()` (member chunk x part); returns the list of plans in that order."""
        t_end = self.n_steps if t_end is None else int(t_end)
        key = (int(t_begin), t_end)
        plans = self._plans.get(key)
        if plans is None:
            plans = []
            self._wave_stats()
            create = self._forward_calls()[2]
            with torch.cuda.device(self.device):
                for m0, n, _ in self.per_step_launches():
                    plan = ctypes.c_void_p()
                    _capi.check(self.lib, create(t_begin, t_end, m0, n, ctypes.byref(plan)))
                    plans.append(plan)
            self._plans[key] = plans
        return plans

    def close(self):
        for plans in self._plans.values():
            for plan in plans:
                self.lib.fiveeq_plan_destroy(plan)
        self._plans = {}

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    # -- on-device summary statistics -----------------------------------------------------
    def stats_sums(self, t_begin=0, t_end=None, scenario=None):
        """[n, 5] fp64 per step: (count, sum T, sum T^2, min T, max T) over this shard's members — folded over the
        per-wave records the kernels wrote (or, for steps a checkpoint's summaries brought, as folded by the saver).
        Additive across shards (fiveeqscm_amd.distributed.reduce_stats).  scenario: which scenario's moments (required
        with the scenario axis)."""
        if not self.collect_stats:
            raise RuntimeError("engine was built with collect_stats=False")
        sc = self._scen(scenario)
        _joined(self)
        t_end = self.n_steps if t_end is None else int(t_end)
        step_sums = self._step_sums if sc is None else self._step_sums[sc]
        valid = self._step_sums_valid[t_begin:t_end]
        if valid.all():                                          # everything came folded from a checkpoint
            return step_sums[t_begin:t_end].clone()
        recs = self._wave_stats()
        s = (recs if sc is None else recs[sc])[:, t_begin:t_end]     # [W, n, 4]
        cnt = torch.full((s.shape[1],), float(self.n_members), dtype=torch.float64, device=s.device)
        out = torch.stack([cnt, s[:, :, 0].sum(0), s[:, :, 1].sum(0), s[:, :, 2].min(0).values,
                           s[:, :, 3].max(0).values], dim=1)
        if valid.any():
            pick = torch.from_numpy(valid).to(out.device)
            out[pick] = step_sums[t_begin:t_end][pick]
        return out

    def stats(self, t_begin=0, t_end=None, scenario=None):
        """dict of per-step ensemble moments of T over this shard: mean, var (population), min, max (of `scenario` with the
        scenario axis)."""
        from .distributed import moments_from_sums
        return moments_from_sums(self.stats_sums(t_begin, t_end, scenario=scenario))

    def chi2(self):
        """[N] fp64 on the device: each member's score against the observations, chi2 = V - 2 A U + A^2 P
        (constrain.chi2_from_misfit).  Raises until the run has passed the last step with a nonzero weight: before that, A and
        the sums describe part of the window only."""
        if self.observations is None:
            raise RuntimeError("engine was built without observations=")
        last = self.observations.window[1]
        if self.t_next < last:
            raise RuntimeError(f"chi2: the run is at step {self.t_next}, the observation window ends at step {last}")
        _joined(self)
        from .constrain import chi2_from_misfit
        return chi2_from_misfit(self.misfit, self.observations.P)

    def gather_summary(self, steps, percentiles=(5.0, 50.0, 95.0), dst=0, group=None, stats=None, gas=None, accepted=None,
                       scenario=None, weights=None):
        """End-of-run summary of T — or, with `gas` = a gas index, of that gas's concentration C — at the stored `steps` over
        ALL members of all ranks (collective over `group`; see distributed.gather_summary): merged moments on every rank,
        exact percentiles on rank `dst`.  With collect_stats the moments of T come from the records the kernels wrote while
        stepping — the summary then reads the rows twice (histogram, selection) instead of three times.
        accepted: a boolean [N] mask of this shard's members (constrain.accept_*): the summary is then over the ACCEPTED
        members of all ranks only — the selected rows are compacted on the device and go through the same passes (the
        in-kernel moment records cover every member, so they are not used); `count` is the global number accepted.  A rank
        with no accepted member still takes part in every collective.  scenario: the scenario summarised (required with
        the scenario axis; `accepted` masks the members of that scenario).
        weights: integer weights of this shard's members, int64 [N] on the engine's device, 0..2^32 each
        (constrain.importance_weights): the summary is then the WEIGHTED one over all members of all ranks
        (distributed.gather_weighted_summary; include/fiveeq.h, "WEIGHTED SUMMARY") — exact weighted percentiles by the
        inverted CDF, and the result also holds weight_sum, ess, std and method = "weighted_inverted_cdf"; `count` is the
        global number of members with a positive weight.  Not together with `accepted`."""
        from .distributed import gather_summary, gather_weighted_summary
        if weights is not None and accepted is not None:
            raise ValueError("gather_summary: weights= and accepted= exclude each other (a weight of 0 drops a member)")
        sc = self._scen(scenario)
        stored = self.T if gas is None else self.C
        if stored is None or self.concentration_driven and gas is not None:
            raise RuntimeError(f"no stored {'T' if gas is None else 'C'} rows to summarise")
        if gas is not None and not 0 <= int(gas) < self.n_gas:
            raise ValueError(f"gas {gas}: the parameter set has gases 0..{self.n_gas - 1}")
        _joined(self)
        row_of = {int(t): r for r, t in enumerate(self.out_steps)}
        missing = [int(t) for t in steps if int(t) not in row_of]
        if missing:
            raise ValueError(f"steps {missing} are not stored (out_steps)")
        picked = [row_of[int(t)] for t in steps]
        T_rows = self.T if sc is None else self.T[sc]
        C_rows = None if self.C is None else (self.C if sc is None else self.C[sc])
        rows = T_rows[picked] if gas is None else C_rows[picked, int(gas)]
        if weights is not None:
            int_weights(weights, self.n_members, rows.device, check_range=False)
            return gather_weighted_summary(rows, weights, percentiles, dst=dst, group=group, stats=stats)
        if accepted is not None:
            mask = bool_mask(accepted, self.n_members, self.device)
            return gather_summary(rows[:, mask].contiguous(), percentiles, dst=dst, group=group, stats=stats)
        sums = None
        if gas is None and self.collect_stats and all(self._stats_have[int(t)] for t in steps):   # else: the moments pass over the rows
            sums = torch.cat([self.stats_sums(int(t), int(t) + 1, scenario=sc) for t in steps])[:, 1:5].contiguous()
        return gather_summary(rows, percentiles, dst=dst, group=group, stats=stats, local_sums=sums)

    def trajectory_metrics(self, levels=(), windows=(), scenario=None, state=None):
        """Per-member metrics of the stored T rows (metrics.trajectory_metrics over self.T and self.out_steps): peak and the
        step it is reached, per level the first stored step at or above it and the number of stored steps there, per step
        window [a, b) the sum and mean of the stored steps inside, the number of NaN rows — one streaming HIP pass.  With the
        scenario axis, scenario=None covers all scenarios in one launch and the results carry a leading [S] axis; an index
        covers that scenario.  Only reads the engine: R, S, T and C are untouched.  `peak` (as peak.reshape(1, -1)) goes
        straight into distributed.gather_summary / gather_weighted_summary as a one-row block."""
        from .metrics import trajectory_metrics
        if self.T is None or self.n_rows == 0:
            raise RuntimeError("no stored T rows: trajectory metrics need output_steps")
        _joined(self)
        rows = self.T[self._scen(scenario)] if self.scenario_axis and scenario is not None else self.T
        with torch.cuda.device(self.device):
            return trajectory_metrics(rows, self.out_steps, levels=levels, windows=windows, state=state)

    def _rows_to_smooth(self, what, scenario, gas, rows=None):
        """(rows, steps) of the stored T rows — or of gas `gas`'s stored C rows — for running_mean / window_trends."""
        if self.T is None or self.n_rows == 0:
            raise RuntimeError(f"no stored T rows: {what} needs output_steps")
        if gas is not None:
            if self.C is None or self.concentration_driven:
                raise RuntimeError(f"no stored C rows: {what} of a gas needs stored concentrations")
            if isinstance(gas, bool) or not isinstance(gas, (int, np.integer)) or not 0 <= int(gas) < self.n_gas:
                raise ValueError(f"gas {gas!r}: the parameter set has gases 0..{self.n_gas - 1}")
        sel = _stored_rows_slice(rows)
        _joined(self)
        stored = self.T if gas is None else self.C
        if self.scenario_axis and scenario is not None:
            stored = stored[self._scen(scenario)]
        stored = stored[..., sel, :] if gas is None else stored[..., sel, int(gas), :]
        return stored, self.out_steps[sel]

    def running_mean(self, window, align="centre", scenario=None, rows=None, gas=None):
        """The running mean over `window` consecutive stored T rows (gas=g: that gas's stored C rows), per member —
        smooth.running_mean over the stored rows and self.out_steps, which must be evenly spaced: one streaming HIP pass, every
        output summed afresh from its own rows.  rows: a slice of the stored rows (default: all).  With the scenario axis,
        scenario=None covers all scenarios in one launch and the result carries a leading [S] axis.  Returns
        smooth.SmoothedRows: `sm.rows, sm.steps` go where stored rows go — trajectory_metrics(sm.rows, sm.steps, levels=...)
        dates a warming level by the mean, not by the first warm year.  Only reads the engine."""
        from .smooth import running_mean
        stored, steps = self._rows_to_smooth("running_mean", scenario, gas, rows)
        with torch.cuda.device(self.device):
            return running_mean(stored, steps, window, align=align)

    def window_trends(self, windows, scenario=None, gas=None):
        """Least-squares linear trends of the stored T rows (gas=g: that gas's stored C rows) over up to 4 step windows
        [a, b), per member — smooth.window_trends over the stored rows, self.out_steps and the run's dt: slope in units per
        year, mean, and the sums they come from.  With the scenario axis, scenario=None covers all scenarios in one launch.
        Returns smooth.WindowTrends.  Only reads the engine."""
        from .smooth import window_trends
        stored, steps = self._rows_to_smooth("window_trends", scenario, gas)
        with torch.cuda.device(self.device):
            return window_trends(stored, steps, windows, dt=self.dt)

    def score(self, records, scenario=None):
        """Score the STORED rows against observed records (constrain.score_rows; include/fiveeq.h, "SCORING STORED ROWS").
        records: {"T": Observations, gas index: Observations, ...} — a record of warming against the stored T rows, a record of
        a gas's concentration (Observations.absolute) against its stored C rows; every table over this run's steps.  Works
        for every mode, pool layout and precision, since it only reads stored rows: one HIP pass over self.T, one over self.C
        (the gases asked for, in place).  ValueError if a live step of a record is not a stored step (a partial chi2 would be
        silent otherwise), for a gas record without stored concentrations, and with the scenario axis without scenario=.
        Returns constrain.Score: misfit[key], chi2[key], n_obs[key] and total = the chi2 added in the order T, gases ascending
        — which feeds accept_*, importance_weights and resample like chi2()."""
        from .constrain import Observations, Score, chi2_from_misfit, score_rows
        if not isinstance(records, dict) or not records:
            raise ValueError('records: want a dict {"T" or a gas index: Observations}')
        for g in records:
            if g != "T" and (isinstance(g, (bool, str)) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) < self.n_gas):
                raise ValueError(f'records: key {g!r}; want "T" or a gas index 0..{self.n_gas - 1}')
        gases = sorted(k for k in records if k != "T")
        order = (["T"] if "T" in records else []) + gases
        for key in order:
            if not isinstance(records[key], Observations):
                raise ValueError(f"records[{key!r}]: want a constrain.Observations")
            if records[key].n_steps != self.n_steps:
                raise ValueError(f"records[{key!r}]: table of {records[key].n_steps} steps for a run of {self.n_steps}")
        sc = self._scen(scenario)
        if self.T is None:
            raise ValueError("no stored rows to score: the engine was built with store_trajectory=False")
        if gases and (self.C is None or self.concentration_driven):
            raise ValueError(f"records of gases {[int(g) for g in gases]} need stored concentrations: this engine holds no C rows "
                             "(store_concentrations=False, or a concentration-driven run whose rows are emissions)")
        stored = set(int(t) for t in self.out_steps)
        for key in order:
            missing = [int(t) for t in records[key].live_steps if int(t) not in stored]
            if missing:
                raise ValueError(f"records[{key!r}]: {len(missing)} live steps of the record are not stored steps (out_steps), "
                                 f"first {missing[:5]}: the score would silently cover part of the record")
        _joined(self)
        misfit = {}
        if "T" in records:
            misfit["T"] = score_rows(self.T if sc is None else self.T[sc], self.out_steps, records["T"])
        if gases:
            C = self.C if sc is None else self.C[sc]
            g0, g1 = int(gases[0]), int(gases[-1])
            step = (g1 - g0) // (len(gases) - 1) if len(gases) > 1 else 1
            if list(range(g0, g1 + 1, step)) == [int(g) for g in gases]:
                picked = C[:, g0:g1 + 1:step]                       # a view: the pass strides over the gases not asked for
            else:
                picked = C[:, [int(g) for g in gases]]
            both = score_rows(picked, self.out_steps, [records[g] for g in gases])
            for i, g in enumerate(gases):
                misfit[g] = both[i]
        chi2 = {key: chi2_from_misfit(misfit[key], records[key].P) for key in order}
        total = chi2[order[0]]
        for key in order[1:]:
            total = total + chi2[key]
        return Score(misfit, chi2, total, {key: records[key].n_obs for key in order})

    def _need_stored_C(self, what, why_not_compensated, why_C):
        """The refusals of the passes that recompute the forcing from the stored C rows; `what` names the pass."""
        if self.compensated:
            raise ValueError(f"{what}: compensated=True takes its forcing from the UNROUNDED excess C - C0, which is not stored"
                             f"{why_not_compensated}")
        if self.C is None or self.T is None or self.n_rows == 0:
            raise ValueError(f"{what}: no stored concentrations (store_concentrations=False or no output_steps): {why_C}")

    def forcing_rows(self, want=("F",), rows=None, scenario=None, replay=False):
        """The effective radiative forcing F, its split by gas F_gas, the energy imbalance N = F - T / (q0 + q1) and the
        cumulated heat uptake H (W yr m-2; diagnose.W_YR_M2_TO_ZJ converts) of the STORED rows — diagnose.forcing_rows wired to
        this engine's C, T, out_steps, q, fscale, the scenario's drive and category table, dt and the initial box temperatures
        (include/fiveeq.h, "FORCING ROWS").  One streaming HIP pass that recomputes F with the device function the stepping
        kernels call: for every mode and precision, F is bit for bit what the run formed and dropped.
        want: any of "F", "F_gas", "N", "H".  rows: a slice of the stored rows (default: all).  With the scenario axis,
        scenario=None covers every scenario (one launch each) and the results carry a leading [S] axis (replay_mismatches: a
        list of S counts); an index covers that scenario.
        replay=True also repeats the thermal step on the diagnosed F from the initial box temperatures and returns
        replay_mismatches, the number of (row, member) whose replayed T differs in bits from the stored T (NaN equal to NaN), and
        S_end: 0 mismatches prove that the diagnosed F is the stepping kernel's F, and tell a user that stored rows belong to
        these parameters.  It needs every step from 0 stored.  "H" needs stored rows of consecutive steps (ValueError
        otherwise: a partial integral would be silent).
        Where the rows go: constrain.score_rows(res.H, steps, Observations...) against a heat-content record (res.F against an
        assessed forcing range alike); res.F[k:k + 1] into gather_summary / gather_weighted_summary; any row into drivers().
        ValueError without stored concentrations, for a concentration-driven engine (its C rows are emissions) and for
        compensated=True.  Joins unjoined per-step streams first.  Reads the engine; writes nothing into it.  Returns
        diagnose.ForcingRows."""
        from .diagnose import ForcingRows, forcing_rows
        if self.concentration_driven:
            raise ValueError("forcing_rows: a concentration-driven engine stores the diagnosed EMISSIONS in its C rows, not "
                             "concentrations; the forcing of its target concentrations is not diagnosed here")
        self._need_stored_C("forcing_rows", "; the stored C rows cannot reproduce that F", "F is recomputed from the stored C rows")
        if self.member_forcing is not None:
            raise ValueError("forcing_rows: the pass recomputes F from the shared tables and the scale rows; the per-member rows "
                             "of member_forcing= are not part of it")
        sel = _stored_rows_slice(rows)
        steps = self.out_steps[sel]
        if replay and (steps.size == 0 or steps[0] != 0 or np.any(np.diff(steps) != 1)):
            raise ValueError("forcing_rows(replay=True) repeats the run from its initial state: it needs every step from 0 stored "
                             f"and rows from the first (stored steps {steps[:3].tolist()}..: output_steps is a subset, or rows= "
                             "starts later)")
        _joined(self)

        def one(sc):
            pick = (lambda t: t) if sc is None else (lambda t: t[sc])
            S0 = None
            if replay:
                S0 = torch.zeros((2, self.n_members), dtype=self.dtype, device=self.device)
                if self._S0 is not None:
                    S0.copy_(torch.from_numpy(np.ascontiguousarray(self._S0 if sc is None else self._S0[sc])).to(self.dtype))
            with torch.cuda.device(self.device):
                return forcing_rows(pick(self.C)[sel], steps, self.params, q=self.q, F_ext=pick(self.drive), dt=self.dt,
                                    T_rows=pick(self.T)[sel], fscale=self.fscale,
                                    X=None if self.fext is None else pick(self.fext), want=want, S_begin=S0)

        if not self.scenario_axis:
            return one(None)
        if scenario is not None:
            return one(self._scen(scenario))
        parts = [one(s) for s in range(self.n_scenarios)]
        stack = lambda name: (None if getattr(parts[0], name) is None                                    # noqa: E731
                              else torch.stack([getattr(p, name) for p in parts]))
        return ForcingRows(stack("F"), stack("F_gas"), stack("N"), stack("H"), stack("S_end"),
                           [p.replay_mismatches for p in parts] if replay else None)

    def sea_level_rows(self, components, expansion=None, want=("total",), rows=None, scenario=None, state=None):
        """Each member's global-mean sea-level rise after every stored row — sea_level.sea_level_rows wired to this engine's
        stored T rows, out_steps (consecutive steps, ValueError otherwise) and dt, for this shard's members: `components`
        (a sea_level.SeaLevelComponents) gives its per-member rows over these n_members columns.  One streaming HIP pass, fp64.
        expansion: each member's eta (a value or [N]): the thermosteric term eta H is added, H taken from
        self.forcing_rows(want=("H",)) over the stored rows from the first one (so that a rows= slice sees the H of the whole
        run) — that method's refusals stand: no stored concentrations, a concentration-driven or compensated run, and
        member_forcing=, whose forcing is not recomputed; model the expansion of such runs as a relax component instead.
        want: any of "total", "components".  rows: a slice of the stored rows (default: all).  With the scenario axis,
        scenario=None covers all scenarios in one launch and the results carry a leading [S] axis; an index covers that
        scenario.  state: the result of an earlier call over the rows directly before these, or S0 [.., J, N].
        Reads the engine; writes nothing into it.  Returns sea_level.SeaLevelRows: `.total, .steps` go where stored rows go."""
        from .sea_level import sea_level_rows
        if self.T is None or self.n_rows == 0:
            raise RuntimeError("no stored T rows: sea_level_rows needs output_steps")
        sel = _stored_rows_slice(rows)
        sc = self._scen(scenario) if self.scenario_axis and scenario is not None else None
        heat = None
        if expansion is not None:
            start, stop, _ = sel.indices(self.n_rows)
            heat = self.forcing_rows(want=("H",), rows=slice(0, stop), scenario=sc).H[..., start:, :]
        _joined(self)
        T = self.T if sc is None else self.T[sc]
        with torch.cuda.device(self.device):
            return sea_level_rows(T[..., sel, :], self.out_steps[sel], components, dt=self.dt, heat=heat, expansion=expansion,
                                  state=state, want=want)

    def carbon_rows(self, want=("fraction",), gases=None, rows=None, scenario=None):
        """The carbon-cycle quantities of the STORED rows — carbon.carbon_rows wired to this engine's stored rows, T, out_steps,
        r rows, the scenario's drive table and its cumulative emissions, the drive mask, dt and the initial pools
        (include/fiveeq.h, "CARBON ROWS"): one streaming HIP pass.
        want: any of "airborne" (G_a), "cumE", "uptake" (G_u), "fraction" (the airborne fraction G_a / cumE), "iirf", "alpha"
        (the values the NEXT step uses: they are formed from the row's own C and T) and "sink" (E - dG_a / dt).  gases: the gas
        indices to diagnose, increasing (default: all); axis 1 of every result.  rows: a slice of the stored rows (default: all).
        With the scenario axis, scenario=None covers every scenario (one launch each) and the results carry a leading [S] axis;
        an index covers that scenario.
        A concentration-driven engine is served too: its rows hold the diagnosed emissions, its cumulative emissions are
        carried per member with the stepping kernel's own fma — carbon_rows(want=("cumE",)).cumE[-1] of a run with every step
        stored is `cumE`, bit for bit.
        "sink" and the cumE / uptake / fraction / iirf / alpha of a concentration-driven gas carry state through the rows: they
        need stored rows of consecutive steps FROM STEP 0 (ValueError otherwise: the engine does not keep G_a and the cumulative
        emissions of a later step; carbon.carbon_rows takes them as cum0= / airborne0=).  G_a before the first row comes from
        the initial pools (R0; 0 without).
        Where the rows go: constrain.score_rows(res.sink[:, 0], steps, Observations...) against a carbon-budget record;
        res.fraction[k:k + 1, 0] into gather_summary / gather_weighted_summary; any row into drivers().
        ValueError without stored concentrations and for compensated=True.  Joins unjoined per-step streams first.  Reads the
        engine; writes nothing into it.  Returns carbon.CarbonRows."""
        from .carbon import _NEED_CUM, CarbonRows, carbon_rows
        want = tuple(want)
        self._need_stored_C("carbon_rows", "; the stored C rows are the rounded sums", "the pass reads the stored C rows")
        G = self.n_gas
        conc_mask = getattr(self, "conc_mask", (1 << G) - 1 if self.concentration_driven else 0)
        conc = tuple(g for g in range(G) if conc_mask >> g & 1)
        picked = range(G) if gases is None else gases
        sel = _stored_rows_slice(rows)
        steps = self.out_steps[sel]
        carried = "sink" in want or (any(w in _NEED_CUM for w in want) and any(g in conc for g in picked))
        if carried and steps.size and steps[0] != 0:
            raise ValueError("carbon_rows: the sink flux and the cumulative emissions of a concentration-driven gas are carried "
                             f"through the rows from the run's initial state: they need rows from step 0 (first row: step "
                             f"{int(steps[0])}); carbon.carbon_rows takes the state of a later step as cum0= / airborne0=")
        _joined(self)

        def one(sc):
            pick = (lambda t: t) if sc is None else (lambda t: t[sc])
            ga0 = None
            if "sink" in want:
                ga0 = torch.zeros((G, self.n_members), dtype=self.dtype, device=self.device)
                if self._R0 is not None:
                    R0 = torch.from_numpy(np.ascontiguousarray(self._R0 if sc is None else self._R0[sc])).to(self.device, self.dtype)
                    off = 0
                    for g in range(G):
                        total = R0[off]
                        for i in range(1, self.pools[g]):
                            total = total + R0[off + i]
                        ga0[g] = total * torch.tensor(1.0 / float(self.model.gas[g].emis2conc), dtype=torch.float64).to(self.dtype)
                        off += self.pools[g]
            with torch.cuda.device(self.device):
                return carbon_rows(pick(self.C)[sel], steps, self.params, r=self.r, drive=pick(self.drive), dt=self.dt,
                                   T_rows=pick(self.T)[sel], concentration_gases=conc, gases=gases, want=want, airborne0=ga0,
                                   cum_table=self._cum_end if sc is None else self._cum_end[sc])

        if not self.scenario_axis:
            return one(None)
        if scenario is not None:
            return one(self._scen(scenario))
        parts = [one(s) for s in range(self.n_scenarios)]
        stack = lambda name: (None if getattr(parts[0], name) is None                                    # noqa: E731
                              else torch.stack([getattr(p, name) for p in parts]))
        return CarbonRows(*(stack(name) for name in ("airborne", "cumE", "uptake", "fraction", "iirf", "alpha", "sink", "cum_end",
                                                     "airborne_end")), gases=parts[0].gases)

    def pulse_response(self, experiment_or_pulses, horizons, base=0, rows=None):
        """Per-member emission metrics from this engine's stored rows — pulse.pulse_response wired to the engine's C, T,
        out_steps, drive tables, fscale and category tables (include/fiveeq.h, "PULSE RESPONSE"): the differences of forcing,
        warming and concentration between each pulse scenario and the base scenario, summed to the horizons, in ONE streaming
        HIP pass.  experiment_or_pulses: the pulse.PulseExperiment the engine was built from (pulse p is scenario 1 + p), or a
        sequence of (scenario, gas, size).  horizons: strictly increasing row counts (years at dt = 1), counted from the first
        stored row.  base: the base scenario.  rows: a slice of the stored rows (default: all); the first stored row must be
        the step that carries the pulses, or the sums miss the pulse's first years.
        ValueError for an engine without the scenario axis, without stored concentrations, for compensated=True (its forcing
        comes from the unrounded excess) and for stored rows that are not consecutive steps.  Joins unjoined per-step streams
        first.  Reads the engine; writes nothing into it.  Returns pulse.PulseResponse: agwp(), agtp(), iagtp(), irf(), gwp(),
        gtp(), whose rows [p, h] go into gather_summary / gather_weighted_summary and drivers() unchanged."""
        from .pulse import PulseExperiment, pulse_response
        if not self.scenario_axis:
            raise ValueError("pulse_response: this engine runs one scenario; a pulse response needs the base and the pulse scenarios "
                             "in ONE engine (emissions [S, n_steps, G], e.g. pulse.pulse_experiment(...).emissions)")
        self._need_stored_C("pulse_response", "", "the forcing of every scenario is recomputed from its stored C rows")
        sel = _stored_rows_slice(rows)
        if isinstance(experiment_or_pulses, PulseExperiment):
            table = [(1 + p, g, size) for p, (g, size) in enumerate(experiment_or_pulses.pulses)]
        else:
            table = list(experiment_or_pulses)
        _joined(self)
        with torch.cuda.device(self.device):
            return pulse_response(self.C[:, sel], self.T[:, sel], self.out_steps[sel], self.params, q=self.q, F_ext=self.drive, dt=self.dt,
                                  base=base, pulses=table, horizons=horizons, fscale=self.fscale, X=self.fext)

    def parameter_rows(self, names=None):
        """(names, rows [K, N]) — this shard's per-member parameters as device rows in the engine's dtype, in the order r0[g],
        rC[g], rT[g] per gas, q[0], q[1], ECS, TCR (params.ecs_tcr of the q rows) and, with forcing=, f_scale[g] and
        fx_scale[k].  names: the rows wanted, in the order wanted.  Reads the engine's rows; writes nothing."""
        from .params import ecs_tcr, forcing_2x
        G = self.n_gas
        have = [f"{k}[{g}]" for g in range(G) for k in ("r0", "rC", "rT")] + ["q[0]", "q[1]", "ECS", "TCR"]
        ecs, tcr = ecs_tcr(self.q, self.params["d"], forcing_2x(self.params))
        rows = [self.r, self.q, ecs[None], tcr[None]]
        if self.fscale is not None:
            have += [f"f_scale[{g}]" for g in range(G)] + [f"fx_scale[{k}]" for k in range(int(self.fscale.shape[0]) - G)]
            rows.append(self.fscale)
        rows = torch.cat(rows)
        if names is None:
            return have, rows
        names = list(names)
        unknown = [n for n in names if n not in have]
        if unknown:
            raise ValueError(f"parameter_rows: no rows {unknown}; this engine has {have}")
        return names, rows[[have.index(n) for n in names]].contiguous()

    def drivers(self, y, names=None, bins=16, weights=None, accepted=None, group=None):
        """Which parameter drives y: joint.sensitivity(parameter_rows(names), y, ...) — eta2, the correlations and slopes of
        the engine's parameter rows against y [Ky, N], any device rows of this shard's members (stored T rows,
        trajectory_metrics().peak[None], chi2()[None]; with the scenario axis, one scenario's rows).  At most 32 parameter rows
        a call: pass names= for a larger set.  Collective over `group`.  Returns joint.Sensitivity; its x axis follows
        parameter_rows(names)[0]."""
        from .joint import sensitivity
        _joined(self)
        x = self.parameter_rows(names)[1]
        with torch.cuda.device(self.device):
            return sensitivity(x, y, bins=bins, weights=weights, accepted=accepted, group=group)

    def resampled(self, plan):
        """(params, R0, S0) of the equal-weight ensemble `plan` (a constrain.Resample of this shard's members, from device
        weights) draws from this engine: ready for EnsembleEngine(params, plan.n_members, emissions, R0=R0, S0=S0, ...), which
        then continues, for each of its members k, the run of this engine's member plan.src[k] bit for bit.
        params is this engine's parameter dict with the per-member entries r0, rC, rT, q (and f_scale, fx_scale with
        forcing=) replaced by gathers of the engine's own device rows, in its dtype; R0 / S0 are gathers of the state R / S
        as it stands (the scenario axis is kept: [S, SP, M] / [S, 2, M]).  One fiveeq_gather_rows_* launch each.
        plan.n_members differs per rank and can be 0 — an engine needs at least one member.  Concentration-driven engines are
        refused: their cumulative emissions (cumE) are per-member state that would have to travel too.
        An engine with member_forcing= returns a FOURTH item: the drawn members' columns of its rows, [n_steps, M], for the new
        engine's member_forcing= — the continued run then reads, for its member k, the series of this engine's member
        plan.src[k]."""
        if self.concentration_driven:
            raise ValueError("resampled: a concentration-driven engine carries cumE, which the resampled triple does not hold")
        if not isinstance(plan.src, torch.Tensor) or plan.src.device != self.device or plan.n_source != self.n_members:
            raise ValueError(f"resampled: want a plan over this engine's {self.n_members} members with indices on {self.device}")
        _joined(self)
        G = self.n_gas
        with torch.cuda.device(self.device):
            r = plan.gather(self.r)                                  # [3 G, M], gas-major (r0, rC, rT)
            params = dict(self.params)
            params["r0"], params["rC"], params["rT"] = r[0::3], r[1::3], r[2::3]
            params["q"] = plan.gather(self.q)
            if self.fscale is not None:
                fs = plan.gather(self.fscale)                        # [G + K, M], gas rows first
                params["f_scale"] = fs[:G]
                if fs.shape[0] > G:
                    params["fx_scale"] = fs[G:]
            if self.member_forcing is not None:
                return params, plan.gather(self.R), plan.gather(self.S), plan.gather(self.member_forcing)
            return params, plan.gather(self.R), plan.gather(self.S)

    def T_histogram(self, lo, hi, n_bins=4096, rows=None, out=None, stream=None, scenario=None):
        """Fixed-bin histograms of the stored T rows on the device: int64 tensor [n_rows, n_bins]
        (bin b counts lo + b w <= T < lo + (b+1) w; outliers land in the edge bins).  `out` lets
        several calls / shards accumulate; percentiles: distributed.histogram_percentiles.  scenario: whose rows (required
        with the scenario axis)."""
        if self.T is None:
            raise RuntimeError("no stored T rows to histogram")
        sc = self._scen(scenario)
        _joined(self, stream)
        T_rows = self.T if sc is None else self.T[sc]
        x = T_rows if rows is None else T_rows[rows].contiguous()
        k = x.shape[0]
        if out is None:
            out = torch.zeros((k, int(n_bins)), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._fn("hist_rows")(k, self.n_members, x.shape[1], self._ptr(x), float(lo), float(hi), int(n_bins),
                                       self._ptr(out), self._stream(stream))
        _capi.check(self.lib, rc)
        return out

    def hist_edge_counts(self):
        """[n_steps, 2] int64: members counted in the first / last bin of T_hist per step.  Values outside [lo, hi) land
        there, so non-zero entries at steps whose true extremes lie inside the range mean the range was too tight for
        percentiles near that tail (compare with stats()['min'/'max'])."""
        if self.T_hist is None:
            raise RuntimeError("engine was built without hist=")
        _joined(self)
        return torch.stack([self.T_hist[:, 0], self.T_hist[:, -1]], dim=1)

    def fscale_sha256(self):
        """sha256 (hex) of the forcing scale rows as fp64 host bytes, [G + K, N] (None without forcing=): with
        `forcing.sha256`, what a checkpoint names the engine's forcing set by."""
        if self.fscale is None:
            return None
        import hashlib                                           # (not cached: `fscale` is the caller's to edit between runs)
        return hashlib.sha256(self.fscale.double().cpu().numpy().tobytes()).hexdigest()

    def member_forcing_sha256(self):
        """sha256 (hex) of the member_forcing rows as fp64 host bytes, [n_steps, N] (None without member_forcing=): what a
        checkpoint names the engine's per-member forcing series by."""
        if self.member_forcing is None:
            return None
        import hashlib                                           # (not cached, like fscale_sha256)
        return hashlib.sha256(self.member_forcing.double().cpu().numpy().tobytes()).hexdigest()

    # -- accounting ----------------------------------------------------------------------
    def bytes_per_member_step(self, mode="per_step", k_steps=None):
        """ALGORITHMIC HBM bytes per member-timestep — every parameter row counted as loaded: a plain
        per_step / graph run with single-valued rows (`uniform_rows`) moves w x len(uniform_rows) FEWER bytes per member-step
        than this count, and bench.py --full's roofline.frac, priced on this count, then prices bytes the kernel no longer
        moves.

        per_step:        w (2 SP + 4 G + 7)   [R,S read+write; r,q read; C,T write];
        fused / small:   w (G + 1) + w (2 SP + 3 G + 6) / steps per launch (n_steps; fused: fused_span, or with hist= the
                         ring length);
        ksteps:          w (G + 1) + w (2 SP + 3 G + 6) / k_steps  (state + parameters once per k_steps).
        Statistics add one 32-byte record per wave of 64 members and step; with `hist=` the bin ring adds 2 B written + 2 B
        read per member-step.  With `observations=` the misfit accumulators add, per_step: 48 B (3 fp64 read + written) per
        member and step of the observation window, averaged over the run's steps; the fused forms: 48 B per member and launch.
        With the scenario axis the count is per MEMBER-SCENARIO-step: per_step reads the parameter rows once for all S
        scenarios, w (2 SP + 4 + (G + 1) stored) + w (3G + 2) / S (with `forcing=`: w (3G + 2 + G + K) / S, the scale rows
        too are read once per member).
        With `forcing=` the G + K scale rows are parameter rows like r and q: per_step w (G + K) more per member-step, the
        fused forms w (G + K) more per member and launch.
        With `member_forcing=` the member's row element is read at EVERY step in every form — the rows are streamed, not
        resident: w more per member-step for per_step and the fused forms alike (and, without forcing=, the G unit scale rows
        count like forcing='s)."""
        w, G, SP = self._w, self.n_gas, self.sum_pools
        fr = self._n_scale_rows()
        out = ((G if self.C is not None else 0) + 1) * self.n_rows / self.n_steps      # stored rows only
        if self.member_forcing is not None:
            out += 1                                             # one row element per member-step, like a stored row
        extra = (32.0 / 64.0) if self.collect_stats else 0.0
        ring = 4.0 if (self.T_hist is not None and mode in ("fused", "per_step")) else 0.0
        if self.observations is not None:
            tab = self.observations.table
            if mode == "per_step":
                extra += 48.0 * np.count_nonzero((tab[:, 1] != 0) | (tab[:, 2] != 0)) / self.n_steps
        if mode == "per_step" and self.scenario_axis:
            return w * (2 * SP + 4 + out) + w * (3 * G + 2 + fr) / self.n_scenarios + extra
        if mode == "per_step":
            return w * (2 * SP + 3 * G + 6 + fr + out) + extra + ring
        if mode == "fused":
            span = min(self.hist_ring_steps, self.n_steps) if self.T_hist is not None else self.fused_span_steps(self.n_steps)
        elif mode == "ksteps":
            span = k_steps or self.auto_k_steps()
        elif mode == "small":
            span = self.n_steps
        else:
            raise ValueError(f"no byte count for mode {mode!r}")
        if self.observations is not None:
            extra += 48.0 / max(int(span), 1)
        return w * (out + (2 * SP + 3 * G + 6 + fr) / max(int(span), 1)) + extra + ring


class ConcentrationDrivenEngine(EnsembleEngine):
    """A concentration-driven (inverse) ensemble that carries per-member forcing scales and the in-loop misfit: the history
    leg of a calibration.  `concentrations` [n_steps, G] are the target concentrations at the end of each step, shared by
    all members; the emissions that reach them are diagnosed per member into `E` and cumulated in `cumE`, as
    EnsembleEngine(concentration_driven=True) does.  On top of that
        forcing=       a forcing.ExternalForcings table [n_steps, K]: the member scales the forcing of gas g by
                       params["f_scale"][g] and category k by params["fx_scale"][k] — F = F_ext + sum_k sx_k X[t, k] +
                       sum_g sg_g F_g, every term one fma, as in the forward forcing form;
        observations=  a constrain.Observations table: `misfit` [3, N] is accumulated in-loop from T; chi2() scores.
    Every other argument is EnsembleEngine's (concentration_driven itself is not one: it is always True).  One time-fused
    launch per run() call (fiveeq_run_inverse_forc_*, include/fiveeq.h): without forcing= and observations= that is the plain
    inverse kernel; unit scales with K = 0 or a zero table give its bits, and observations= changes nothing but `misfit`.  Pool
    layouts {4} and 4 + 1 + 1 for either feature.
    What an EnsembleEngine offers on its rows works here as there: fscale, misfit, chi2(), score() of T, stats(),
    gather_summary(), parameter_rows() and drivers() with the scale rows, state_dict() / load_state_dict() (cumE, misfit and
    the forcing identity travel), reset_state(), bytes_per_member_step().  Refused as for every concentration-driven engine:
    the scenario axis, hist=, compensated=True, mode 'small', forcing_rows() (the C rows hold emissions) and resampled()
    (cumE does not travel).
    A projection branches off through R0 / S0: EnsembleEngine(params, N, emissions, forcing=..., R0=hist.R, S0=hist.S) — the
    forward engine with the same f_scale / fx_scale rows continues T without a jump."""

    _INVERSE_CALIBRATION = True

    def __init__(self, params, n_members, concentrations, *, forcing=None, observations=None, **kw):
        if "concentration_driven" in kw:
            raise TypeError("ConcentrationDrivenEngine is always concentration-driven: concentration_driven= is not an argument")
        super().__init__(params, n_members, concentrations, concentration_driven=True, forcing=forcing,
                         observations=observations, **kw)

    def _run_inverse(self, t_begin, t_end, stream):
        forc = (None, None, 0) if self.fscale is None else (self._ptr(self.fscale), self._ptr(self.fext), self.forcing.n_categories)
        obs = (None, None) if self.misfit is None else self._obs_args()
        return self._fn("run_inverse_forc")(*self._run_args(t_begin, t_end, cumE=self._ptr(self.cumE)), *forc, *obs,
                                            self._stream(stream))


class MixedDriveEngine(ConcentrationDrivenEngine):
    """An ensemble whose gases are driven EACH ITS OWN WAY in one run: the gases named in `concentration_gases` follow the
    target concentrations `concentrations` [n_steps, G] (end of each step, shared by all members) and have their emissions
    diagnosed, every other gas takes the emissions `emissions` [n_steps, G] as a forward run does.  CO2 emission-driven with
    CH4 and N2O prescribed — MixedDriveEngine(params, N, E, C, (1, 2)) — is the "esm-hist" set-up and the history leg of a
    carbon-cycle calibration: r0 / rC / rT show in C of CO2 and in T; the converse, (0,), is a concentration pathway of CO2
    with its compatible emissions beside short-lived gases from inventories.  The `emissions` column of a
    concentration-driven gas and the `concentrations` column of an emission-driven gas are ignored (NaN allowed there).
        conc_mask   bit g set = gas g is concentration-driven (include/fiveeq.h "MIXED DRIVE");
        out_kind    per gas what its rows hold, e.g. ("C", "E", "E");
        X           [n_rows, G, N]: C of an emission-driven gas, the diagnosed E of a concentration-driven one (`C` and `E` are
                    the same tensor, as on every concentration-driven engine);
        cumE        [G, N]: the cumulative emissions of the concentration-driven gases; the rows of emission-driven gases stay
                    zero (the kernel neither reads nor writes them: their cumulative emissions are the drive table's).
    One time-fused launch per run() call (fiveeq_run_mixed_*).  An empty `concentration_gases` runs the forward time-fused
    kernel and a full one the inverse kernel, bit for bit; a proper selection needs pools [4, 1, 1].  forcing=,
    observations= and everything ConcentrationDrivenEngine offers on its rows work as there (fscale, misfit, chi2(), score()
    of T, stats(), gather_summary() of T, parameter_rows(), drivers(), reset_state(), bytes_per_member_step());
    state_dict() carries `conc_mask`, and load_state_dict() refuses a checkpoint of another mask.  Refused as for every
    concentration-driven engine: the scenario axis, hist=, compensated=True, mode 'small', forcing_rows(), resampled(),
    gas= summaries and gas records in score().  A projection branches off through R0 / S0 as from ConcentrationDrivenEngine."""

    def __init__(self, params, n_members, emissions, concentrations, concentration_gases, *, forcing=None, observations=None,
                 **kw):
        if _is_scenario_set(emissions) or _is_scenario_set(concentrations):
            raise ValueError("a mixed-drive engine runs one scenario: emissions and concentrations are [n_steps, G] (the "
                             "scenario axis is carried by the plain emission-driven forms only)")
        G = n_gas_of(params)
        self.conc_mask = concentration_mask(concentration_gases, G)
        self.concentration_gases = tuple(g for g in range(G) if self.conc_mask >> g & 1)
        self.out_kind = tuple("E" if self.conc_mask >> g & 1 else "C" for g in range(G))
        self._mixed_series = (emissions, concentrations)
        make_drive(emissions, kw.get("F_ext"), kw.get("dt", 1.0), kw.get("output_steps"), concentrations=concentrations,
                   concentration_gases=self.concentration_gases)          # the table's own refusals, before a device is asked for
        super().__init__(params, n_members, None, forcing=forcing, observations=observations, **kw)
        self.X = self.C
        n_pools = (ctypes.c_int32 * G)(*self.pools)
        if not self.lib.fiveeq_mixed_layout_supported(G, n_pools, self.conc_mask):
            raise _capi.FiveEqError(_capi.E_UNSUPPORTED, f"pool layout {self.pools} has no mixed-drive form for "
                                    f"concentration_gases={self.concentration_gases} (pools [4, 1, 1] have)")

    def _make_drive(self, emissions, F_ext, dt, output_steps):
        E, C = self._mixed_series
        return make_drive(E, F_ext, dt, output_steps, concentrations=C, concentration_gases=self.concentration_gases)

    def _run_inverse(self, t_begin, t_end, stream):
        forc = (None, None, 0) if self.fscale is None else (self._ptr(self.fscale), self._ptr(self.fext), self.forcing.n_categories)
        obs = (None, None) if self.misfit is None else self._obs_args()
        return self._fn("run_mixed")(*self._run_args(t_begin, t_end, cumE=self._ptr(self.cumE)), self.conc_mask, *forc, *obs,
                                     self._stream(stream))


def run_ensemble(emissions, params, n_members, *, F_ext=None, dt=1.0, dtype=torch.float64, device=None,
                 mode="per_step", output_steps=None, collect_stats=False, R0=None, S0=None):
    """Whole-series convenience wrapper: returns dict(C [n_rows,G,N], T [n_rows,N], R, S, out_steps
    [, T_stats]) of device tensors after a synchronise."""
    eng = EnsembleEngine(params, n_members, emissions, F_ext=F_ext, dt=dt, dtype=dtype, device=device,
                         output_steps=output_steps, collect_stats=collect_stats, R0=R0, S0=S0)
    eng.run(mode=mode)
    torch.cuda.synchronize(eng.device)
    out = {"C": eng.C, "T": eng.T, "R": eng.R, "S": eng.S, "out_steps": eng.out_steps}
    if collect_stats:
        out["T_stats"] = eng.stats()
    eng.close()
    return out
