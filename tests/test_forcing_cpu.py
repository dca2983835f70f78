"""Per-member forcing scales (include/fiveeq.h "FORCING SCALES"), the parts that need no GPU: the new symbols and their
host-side validation, the ExternalForcings table and its CSV reader, the sampler of the scale rows, and the checkpoint's
refusal of another forcing set."""
import ctypes
import os

import numpy as np
import pytest

from fiveeqscm_amd import _capi, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.checkpoint import CheckpointMixin
from fiveeqscm_amd.forcing import ExternalForcings
from forcing_reference import forcing_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(ROOT, "tests", "golden", "forcing_layout_sample.csv")


def test_the_new_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _capi.load()
    for name in ("fiveeq_run_forc_f64", "fiveeq_run_forc_f32", "fiveeq_plan_create_forc_f64", "fiveeq_plan_create_forc_f32",
                 "fiveeq_forcing_layout_supported", "fiveeq_max_fext"):
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_max_fext() == _capi.MAX_FEXT == 4
    assert lib.fiveeq_abi_version() == 13 and lib.fiveeq_sizeof_model() == 448      # additive: nothing existing changed
    ok = lambda *p: lib.fiveeq_forcing_layout_supported(len(p), (ctypes.c_int32 * len(p))(*p))  # noqa: E731
    assert ok(4) and ok(4, 1, 1)
    assert not ok(1) and not ok(4, 4, 4) and not ok(4, 1) and not ok(5) and not lib.fiveeq_forcing_layout_supported(1, None)


def _call(lib, sfx="f64", n_gas=3, plan=False, n=8, ld=8, n_steps=4, t0=0, t1=4, ptr=0x1000, fscale=0x2000,
          fext=0x3000, n_fext=2, obs=None, misfit=None, form=_capi.FORM_PER_STEP, k_steps=0):
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout without the forcing form
    p, vp = ctypes.c_void_p(ptr), ctypes.c_void_p
    head = (ctypes.byref(model), n, ld, p, n_steps, t0, t1, p, p, p, p, None, None, 0, None, vp(fscale), vp(fext), n_fext,
            vp(obs), vp(misfit))
    if plan:
        out = ctypes.c_void_p(0xDEAD)
        rc = getattr(lib, "fiveeq_plan_create_forc_" + sfx)(*head, ctypes.byref(out))
        assert out.value is None                    # no plan comes back from a refused call
        return rc
    return getattr(lib, "fiveeq_run_forc_" + sfx)(*head, form, k_steps, None)


@pytest.mark.parametrize("plan", [False, True])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_validation_rejects_bad_forcing_arguments_before_any_launch(sfx, plan):
    """Every call returns on the host with FIVEEQ_E_INVALID and a telling message: the (fake) pointers are never dereferenced
    and nothing is launched, so this runs without a GPU."""
    lib = _capi.load()
    cases = [
        (dict(fscale=0), "fscale is NULL"),
        (dict(fscale=0x2001), "fscale must be"),
        (dict(n_fext=-1), "n_fext=-1 outside 0..4"),
        (dict(n_fext=5), "n_fext=5 outside 0..4"),
        (dict(fext=0, n_fext=1), "fext is NULL with n_fext=1"),
        (dict(obs=0x4000), "obs and misfit go together"),
        (dict(misfit=0x4000), "obs and misfit go together"),
        (dict(obs=0x4001, misfit=0x5000), "8-byte aligned"),
        (dict(n_gas=2), "has no forcing form"),
        (dict(n=0), "n_members"),
        (dict(ld=4), "ld="),
        (dict(ptr=0), "NULL device pointer"),
        (dict(t0=3, t1=2), "step range"),
        (dict(t1=5), "step range"),
    ]
    if not plan:
        cases += [(dict(form=2), "form=2"), (dict(k_steps=-1), "k_steps=-1")]
    for kw, needle in cases:
        rc = _call(lib, sfx, plan=plan, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID, (kw, rc, msg)
        assert needle in msg, (kw, msg)


def test_external_forcings_validates_and_is_read_only():
    x = np.arange(12.0).reshape(4, 3)
    fx = ExternalForcings(x, ("aerosol", "volcanic", "solar"))
    assert (fx.n_steps, fx.n_categories, fx.names) == (4, 3, ("aerosol", "volcanic", "solar"))
    assert fx.padded().shape == (4, 4) and np.array_equal(fx.padded()[:, :3], x) and not fx.padded()[:, 3].any()
    with pytest.raises(ValueError):
        fx.table[0, 0] = 1.0                                      # read-only
    assert len(fx.sha256) == 64 and fx.sha256 == ExternalForcings(x.copy(), ("aerosol", "volcanic", "solar")).sha256
    assert fx.sha256 != ExternalForcings(x + 1e-9, fx.names).sha256
    assert fx.sha256 != ExternalForcings(x, ("aerosol", "solar", "volcanic")).sha256
    assert ExternalForcings(np.zeros((5, 0))).n_categories == 0                    # K = 0: gas scales only
    assert ExternalForcings(np.zeros(5)).table.shape == (5, 1)
    for bad, needle in ((np.zeros((4, 5)), "at most 4"), (np.zeros((0, 2)), "want \\[n_steps, K\\]"),
                        (np.zeros((2, 2, 2)), "want \\[n_steps, K\\]"), (np.array([[np.nan]]), "non-finite"),
                        (np.array([[np.inf, 0.0]]), "non-finite")):
        with pytest.raises(ValueError, match=needle):
            ExternalForcings(bad)
    with pytest.raises(ValueError, match="names for"):
        ExternalForcings(x, ("a", "b"))
    with pytest.raises(ValueError, match="repeat"):
        ExternalForcings(x, ("a", "b", "a"))


def test_from_csv_reads_named_columns_by_run_year(tmp_path):
    years = np.arange(1852.0, 1858.0)
    fx = ExternalForcings.from_csv(CSV, ("VOLCANIC", "AEROSOL"), years)            # any order, any sub-range of the years
    assert fx.names == ("VOLCANIC", "AEROSOL") and fx.table.shape == (6, 2)
    assert fx.table[:, 0].tolist() == [-1.5, -0.5, 0.0, 0.0, 0.0, -2.25]
    assert fx.table[:, 1].tolist() == [-0.075, -0.0875, -0.1, -0.1125, -0.125, -0.1375]
    with pytest.raises(ValueError, match="not in the file"):
        ExternalForcings.from_csv(CSV, ("SOLAR",), [1849.0, 1850.0])
    with pytest.raises(ValueError, match="no column-name row"):
        ExternalForcings.from_csv(CSV, ("OZONE",), years)
    with pytest.raises(ValueError, match="at most 4"):
        p = tmp_path / "five.csv"
        p.write_text("YEARS,A,B,C,D,E\n1850,1,2,3,4,5\n1851,1,2,3,4,5\n")
        ExternalForcings.from_csv(str(p), list("ABCDE"), [1850.0, 1851.0])
    p = tmp_path / "gap.csv"
    p.write_text("YEARS,A\n1850,1\n1851,\n")
    with pytest.raises(ValueError, match="missing values"):
        ExternalForcings.from_csv(str(p), ["A"], [1850.0, 1851.0])


def test_the_factored_row_parser_leaves_the_emissions_reader_as_it_was(tmp_path):
    E = np.random.default_rng(3).uniform(0.1, 9.0, (7, 3))
    years = 1990.0 + np.arange(7)
    path = str(tmp_path / "e.csv")
    scenario.write_emissions_csv(path, years, E)
    y, got = scenario.read_emissions_csv(path)
    assert np.array_equal(y, years) and np.array_equal(got, E)
    with pytest.raises(ValueError, match="expected species names such as FossilCO2, CH4, N2O"):
        scenario.read_emissions_csv(CSV)
    bad = tmp_path / "uneven.csv"
    bad.write_text("YEARS,CO2,CH4,N2O\n1990,1,1,1\n1991,1,1,1\n1993,1,1,1\n")
    with pytest.raises(ValueError, match="equal steps"):
        scenario.read_emissions_csv(str(bad))


RANGES = [(0.8, 1.2)] * 3 + [(0.3, 2.0), (0.5, 1.5), (1.0, 1.0)]


def test_sample_forcing_scales_is_independent_of_the_shard_split():
    base = prm.default_params("multigas")
    n_total = 1000
    whole = prm.sample_forcing_scales(base, n_total, ranges=RANGES)
    assert whole.shape == (6, n_total) and whole.dtype == np.float64
    for cuts in ([0, 1000], [0, 1, 500, 999, 1000], [0, 333, 666, 1000]):
        parts = [prm.sample_forcing_scales(3, n_total, lo, hi, RANGES) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate(parts, axis=1), whole), cuts
    for row, (a, b) in zip(whole, RANGES):
        assert row.min() >= a and row.max() <= b
        if a < b:                                                 # one member per stratum of the range
            strata = np.floor((row - a) / (b - a) * n_total).astype(int).clip(0, n_total - 1)
            assert np.unique(strata).size >= n_total - 2          # (the affine map's rounding may move a member across an edge)
    assert (whole[5] == 1.0).all()
    assert not np.array_equal(whole, prm.sample_forcing_scales(base, n_total, ranges=RANGES, seed=1234))
    with pytest.raises(ValueError):
        prm.sample_forcing_scales(base, n_total, ranges=[(2.0, 1.0)])
    with pytest.raises(ValueError):
        prm.sample_forcing_scales(base, n_total, ranges=[])


def test_sample_forcing_scales_uses_dimensions_after_the_parameter_draws():
    """The scale rows are dimensions 3G + 2 ... of the design that sample_ensemble_shard draws dimensions 0 .. 3G + 1 of: the
    parameter rows of a seed are the same with and without them, and the scales are new dimensions, not copies."""
    base = prm.default_params("multigas")
    n_total, G = 512, 3
    before = prm.sample_ensemble_shard(base, n_total, 100, 300)
    s = prm.sample_forcing_scales(base, n_total, 100, 300, RANGES)
    after = prm.sample_ensemble_shard(base, n_total, 100, 300)
    for k in ("r0", "rC", "rT", "q", "TCR", "ECS"):
        assert np.array_equal(before[k], after[k]), k
    want = prm.lhs_rows(n_total, list(range(3 * G + 2, 3 * G + 8)), 100, 300)
    for j, (a, b) in enumerate(RANGES):
        assert np.array_equal(s[j], (b - a) * want[j] + a)
    drawn = prm.lhs_rows(n_total, list(range(3 * G + 2)), 100, 300)
    assert all(not np.array_equal(want[j], drawn[d]) for j in range(6) for d in range(3 * G + 2))


class _Stub(CheckpointMixin):
    """The attributes load_state_dict() reads before it validates the forcing set."""
    cumE = misfit = observations = R = S = None
    scenario_axis = collect_stats = False

    def __init__(self, forcing, scales):
        self.forcing, self._scales = forcing, scales

    def fscale_sha256(self):
        import hashlib
        return None if self.forcing is None else hashlib.sha256(np.asarray(self._scales, dtype=np.float64).tobytes()).hexdigest()


def test_a_checkpoint_of_another_forcing_set_is_refused():
    fx = ExternalForcings(np.linspace(-1.0, 0.0, 10).reshape(5, 2))
    scales = np.ones((3, 4))
    mine = _Stub(fx, scales)
    state = {"forcing_sha256": fx.sha256, "fscale_sha256": mine.fscale_sha256()}
    for other in (_Stub(ExternalForcings(fx.table * 2.0), scales), _Stub(fx, scales * 1.5), _Stub(None, None)):
        with pytest.raises(ValueError, match="forcing set"):
            other.load_state_dict(state)
    with pytest.raises(ValueError, match="forcing set"):
        mine.load_state_dict({})                                  # a checkpoint of a run without forcing=
    with pytest.raises(KeyError, match="'R'"):
        mine.load_state_dict(state)                               # the same set passes the check and goes on to the state


def test_numpy_restatement_against_the_oracle():
    """The test reference itself: with unit scales and no category it is oracle.fiveeq_oracle.run; with scales it is the
    per-member oracle run on scaled coefficients and a summed F_ext, far inside the fp64 tolerance."""
    from fiveeqscm_amd import emissions
    from oracle import fiveeq_oracle as npo
    N, n_steps = 6, 60
    base = prm.default_params("multigas")
    p = prm.sample_ensemble_shard(base, N)
    E = emissions.rcp_like_emissions(n_steps, 3)
    Fx = 0.01 * np.arange(n_steps) / n_steps
    plain = npo.run(E, p, N, F_ext=Fx)
    got = forcing_numpy(E, p, N, np.zeros((n_steps, 0)), np.ones(3), np.zeros((0, N)), F_ext=Fx)
    for k in ("C", "T"):                      # (not bit for bit: the oracle sums the gas forcings before it adds F_ext)
        assert (np.abs(got[k] - plain[k]) <= 1e-10 * np.abs(plain[k]) + 1e-13).all(), k
    s = prm.sample_forcing_scales(base, N, ranges=RANGES[:5])
    X = np.stack([-np.linspace(0.0, 1.0, n_steps), np.where(np.arange(n_steps) % 17 == 5, -2.0, 0.0)], axis=1)
    got = forcing_numpy(E, p, N, ExternalForcings(X), s[:3], s[3:], F_ext=Fx)
    for m in range(N):
        pm = dict(p)
        for k in ("r0", "rC", "rT", "q"):
            pm[k] = np.asarray(p[k])[:, m:m + 1]
        pm["f"] = np.asarray(base["f"], float) * s[:3, m][:, None]
        ref = npo.run(E, pm, 1, F_ext=Fx + X @ s[3:, m])
        for a, b in ((got["C"][:, :, m], ref["C"][:, :, 0]), (got["T"][:, m], ref["T"][:, 0])):
            assert (np.abs(a - b) <= 1e-10 * np.abs(b) + 1e-13).all()
