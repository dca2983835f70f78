"""Forcing scales under the scenario axis (include/fiveeq.h "FORCING SCALES UNDER THE SCENARIO AXIS"), the parts that need no
GPU: the four new symbols and their host-side validation, the ScenarioForcings tables and their CSV reader, and the
checkpoint's refusal of another table set or other scale rows."""
import ctypes
import hashlib

import numpy as np
import pytest

from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.checkpoint import CheckpointMixin
from fiveeqscm_amd.forcing import ExternalForcings, ScenarioForcings

NEW = ("fiveeq_run_scen_forc_f64", "fiveeq_run_scen_forc_f32", "fiveeq_plan_create_scen_forc_f64",
       "fiveeq_plan_create_scen_forc_f32")


def test_the_four_symbols_are_exported_and_bound_and_the_abi_version_stays():
    lib = _capi.load()
    for name in NEW:
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert lib.fiveeq_abi_version() == 13 == _capi.ABI_VERSION and lib.fiveeq_sizeof_model() == 448
    # the arguments of fiveeq_run_scen_* / fiveeq_plan_create_scen_* with (fscale, fext, n_fext) before the trailing ones
    sig = _capi.SIGNATURES
    for sfx in ("f64", "f32"):
        scen, both = sig["fiveeq_run_scen_" + sfx][1], sig["fiveeq_run_scen_forc_" + sfx][1]
        assert both == scen[:-3] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + scen[-3:] and len(both) == 22
        scen, both = sig["fiveeq_plan_create_scen_" + sfx][1], sig["fiveeq_plan_create_scen_forc_" + sfx][1]
        assert both == scen[:-1] + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + scen[-1:] and len(both) == 20


def _call(lib, sfx="f64", n_gas=3, plan=False, n=8, ld=8, n_scen=2, n_steps=4, t0=0, t1=4, ptr=0x1000, fscale=0x2000,
          fext=0x3000, n_fext=2, form=_capi.FORM_PER_STEP, k_steps=0):
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout without the forcing form
    p, vp = ctypes.c_void_p(ptr), ctypes.c_void_p
    head = (ctypes.byref(model), n, ld, n_scen, p, n_steps, t0, t1, p, p, p, p, None, None, 0, None, vp(fscale), vp(fext),
            n_fext)
    if plan:
        out = ctypes.c_void_p(0xDEAD)
        rc = getattr(lib, "fiveeq_plan_create_scen_forc_" + sfx)(*head, ctypes.byref(out))
        assert out.value is None                    # no plan comes back from a refused call
        return rc
    return getattr(lib, "fiveeq_run_scen_forc_" + sfx)(*head, form, k_steps, None)


@pytest.mark.parametrize("plan", [False, True])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_bad_argument_is_refused_before_any_launch(sfx, plan):
    """Every call returns on the host with FIVEEQ_E_INVALID and a telling message: the (fake) pointers are never dereferenced
    and nothing is launched, so this runs without a GPU."""
    lib = _capi.load()
    max_s = lib.fiveeq_max_scenarios()
    cases = [
        (dict(fscale=0), "fscale is NULL"),
        (dict(fscale=0x2001), "fscale must be"),
        (dict(n_fext=-1), "n_fext=-1 outside 0..4"),
        (dict(n_fext=lib.fiveeq_max_fext() + 1), "n_fext=5 outside 0..4"),
        (dict(fext=0, n_fext=1), "fext is NULL with n_fext=1"),
        (dict(n_scen=0), "n_scen=0 outside"),
        (dict(n_scen=-3), "n_scen=-3 outside"),
        (dict(n_scen=max_s + 1), f"n_scen={max_s + 1} outside"),
        (dict(n_gas=2), "has no forcing form"),
        (dict(n=0), "n_members"),
        (dict(ld=4), "ld="),
        (dict(ptr=0), "NULL device pointer"),
        (dict(t0=3, t1=2), "step range"),
        (dict(t0=-1), "step range"),
        (dict(t1=5), "step range"),
    ]
    if plan:
        cases += [(dict(t0=2, t1=2), "empty step range")]
    else:
        cases += [(dict(form=2), "form=2"), (dict(form=-1), "form=-1"), (dict(form=_capi.FORM_FUSED, k_steps=-1), "k_steps=-1"),
                  (dict(k_steps=-1), "k_steps=-1")]
    for kw, needle in cases:
        rc = _call(lib, sfx, plan=plan, **kw)
        msg = lib.fiveeq_last_error().decode()
        assert rc == _capi.E_INVALID, (kw, rc, msg)
        assert needle in msg, (kw, msg)


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_valid_arguments_pass_the_checks_with_an_empty_range(sfx):
    """An empty step range is validated and launches nothing: what is valid gets past every check, with K = 0 and fext = NULL,
    with the largest scenario count, in both forms, for both layouts that carry the forcing form."""
    lib = _capi.load()
    for kw in (dict(), dict(n_fext=0, fext=0), dict(n_fext=4), dict(n_scen=lib.fiveeq_max_scenarios()), dict(n_scen=1),
               dict(form=_capi.FORM_FUSED), dict(form=_capi.FORM_FUSED, k_steps=7), dict(n_gas=1)):
        assert _call(lib, sfx, t0=2, t1=2, **kw) == _capi.OK, (kw, lib.fiveeq_last_error())


# ---- ScenarioForcings ------------------------------------------------------------------------------------------------------
def test_scenario_forcings_validates_and_is_read_only():
    x = np.arange(24.0).reshape(2, 4, 3)
    names = ("aerosol", "volcanic", "solar")
    sf = ScenarioForcings(x, names)
    assert (sf.n_scenarios, sf.n_steps, sf.n_categories, sf.names) == (2, 4, 3, names)
    with pytest.raises(ValueError):
        sf.table[0, 0, 0] = 1.0                                   # read-only
    pad = sf.padded()
    assert pad.shape == (2, 4, 4) and pad.dtype == np.float64 and pad.flags["C_CONTIGUOUS"]
    assert np.array_equal(pad[:, :, :3], x) and not pad[:, :, 3].any()
    one = sf.scenario(1)
    assert isinstance(one, ExternalForcings) and one.names == names and np.array_equal(one.table, x[1])
    assert ScenarioForcings(np.zeros((3, 5, 0))).n_categories == 0               # K = 0: gas scales only
    assert ScenarioForcings(np.zeros((3, 5, 0))).padded().shape == (3, 5, 4)
    assert ScenarioForcings(x).names == ("fx0", "fx1", "fx2")
    for bad, needle in ((np.zeros((2, 4, 5)), "at most 4"), (np.zeros((4, 3)), "want \\[S, n_steps, K\\]"),
                        (np.zeros((0, 4, 2)), "want \\[S, n_steps, K\\]"), (np.zeros((2, 0, 2)), "want \\[S, n_steps, K\\]"),
                        (np.zeros((2, 2, 2, 2)), "want \\[S, n_steps, K\\]"), (np.full((1, 1, 1), np.nan), "non-finite"),
                        (np.array([[[np.inf, 0.0]]]), "non-finite")):
        with pytest.raises(ValueError, match=needle):
            ScenarioForcings(bad)
    with pytest.raises(ValueError, match="names for"):
        ScenarioForcings(x, ("a", "b"))
    with pytest.raises(ValueError, match="repeat"):
        ScenarioForcings(x, ("a", "b", "a"))


def test_scenario_forcings_from_a_sequence_of_tables_and_shared():
    a = ExternalForcings(np.linspace(-1.0, 0.0, 10).reshape(5, 2), ("aerosol", "volcanic"))
    b = ExternalForcings(np.linspace(-2.0, 0.5, 10).reshape(5, 2), ("aerosol", "volcanic"))
    sf = ScenarioForcings([a, b])
    assert sf.names == a.names and sf.n_scenarios == 2 and np.array_equal(sf.table, np.stack([a.table, b.table]))
    assert sf.sha256 == ScenarioForcings(np.stack([a.table, b.table]), a.names).sha256
    assert ScenarioForcings((a, b), ("aerosol", "volcanic")).sha256 == sf.sha256
    with pytest.raises(ValueError, match="categories"):
        ScenarioForcings([a, ExternalForcings(b.table, ("aerosol", "solar"))])
    with pytest.raises(ValueError, match="categories"):
        ScenarioForcings([a, ExternalForcings(b.table[:, :1], ("aerosol",))])
    with pytest.raises(ValueError, match="steps"):
        ScenarioForcings([a, ExternalForcings(b.table[:4], b.names)])
    with pytest.raises(ValueError, match="are not the tables'"):
        ScenarioForcings([a, b], ("volcanic", "aerosol"))
    sh = ScenarioForcings.shared(a, 3)
    assert sh.n_scenarios == 3 and sh.names == a.names and all(np.array_equal(sh.table[s], a.table) for s in range(3))
    assert sh.scenario(2).sha256 == a.sha256
    with pytest.raises(ValueError, match="n_scenarios"):
        ScenarioForcings.shared(a, 0)


def test_sha256_changes_with_any_table_byte_or_name():
    x = np.random.default_rng(11).uniform(-2.0, 0.5, (3, 6, 2))
    names = ("aerosol", "volcanic")
    sf = ScenarioForcings(x, names)
    assert len(sf.sha256) == 64 and sf.sha256 == ScenarioForcings(x.copy(), names).sha256
    for idx in ((0, 0, 0), (1, 3, 1), (2, 5, 1)):
        y = x.copy()
        y[idx] = np.nextafter(y[idx], np.inf)                     # one bit of one entry
        assert ScenarioForcings(y, names).sha256 != sf.sha256, idx
    assert ScenarioForcings(x, ("volcanic", "aerosol")).sha256 != sf.sha256
    assert ScenarioForcings(x, ("aerosol", "Volcanic")).sha256 != sf.sha256
    assert ScenarioForcings(x[::-1], names).sha256 != sf.sha256                   # the same tables under other scenarios
    assert ScenarioForcings(x.reshape(2, 9, 2), names).sha256 != sf.sha256        # the same bytes in another shape
    assert ScenarioForcings(x[:1], names).sha256 != ExternalForcings(x[0], names).sha256


def test_from_csvs_reads_one_file_per_scenario(tmp_path):
    years = np.arange(1850.0, 1856.0)
    paths, tables = [], []
    for s in range(3):
        aer = -0.1 * (s + 1) * np.arange(6.0)
        vol = np.where(np.arange(6) == 2 + s, -1.5, 0.0)
        path = tmp_path / f"forcing_{s}.csv"
        lines = ["external forcing, W m-2", "YEARS,SOLAR,AEROSOL,VOLCANIC"]
        lines += [f"{int(y)},0.0,{float(a)!r},{float(v)!r}" for y, a, v in zip(years, aer, vol)]
        path.write_text("\n".join(lines) + "\n")
        paths.append(str(path))
        tables.append(np.stack([aer, vol], 1))
    sf = ScenarioForcings.from_csvs(paths, ("AEROSOL", "VOLCANIC"), years[1:5])
    assert sf.names == ("AEROSOL", "VOLCANIC") and sf.table.shape == (3, 4, 2)
    assert np.array_equal(sf.table, np.stack(tables)[:, 1:5])
    for s in range(3):
        assert sf.scenario(s).sha256 == ExternalForcings.from_csv(paths[s], ("AEROSOL", "VOLCANIC"), years[1:5]).sha256
    with pytest.raises(ValueError, match="not in the file"):
        ScenarioForcings.from_csvs(paths, ("AEROSOL",), [1849.0, 1850.0])
    with pytest.raises(ValueError, match="no scenario files"):
        ScenarioForcings.from_csvs([], ("AEROSOL",), years)
    short = tmp_path / "short.csv"
    short.write_text("YEARS,AEROSOL,VOLCANIC\n1850,0,0\n1851,0,0\n")
    with pytest.raises(ValueError, match="not in the file"):
        ScenarioForcings.from_csvs(paths[:1] + [str(short)], ("AEROSOL", "VOLCANIC"), years)


# ---- the checkpoint ----------------------------------------------------------------------------------------------------------
class _Stub(CheckpointMixin):
    """The attributes load_state_dict() reads before it validates the forcing set and the scenario set."""
    cumE = misfit = observations = R = S = None
    collect_stats = False
    scenario_axis = True
    n_scenarios = 2
    drive_sha256 = "d" * 64

    def __init__(self, forcing, scales):
        self.forcing, self._scales = forcing, scales

    def fscale_sha256(self):
        return None if self.forcing is None else hashlib.sha256(np.asarray(self._scales, dtype=np.float64).tobytes()).hexdigest()


def test_a_scenario_checkpoint_of_another_table_set_or_other_scales_is_refused():
    x = np.linspace(-1.0, 0.0, 20).reshape(2, 5, 2)
    sf = ScenarioForcings(x)
    scales = np.ones((5, 4))
    mine = _Stub(sf, scales)
    state = {"forcing_sha256": sf.sha256, "fscale_sha256": mine.fscale_sha256(), "n_scenarios": 2, "drive_sha256": "d" * 64}
    others = (_Stub(ScenarioForcings(x * 2.0), scales),           # another table set
              _Stub(ScenarioForcings(x[::-1]), scales),            # the same tables under swapped scenarios
              _Stub(sf, scales * 1.5),                            # other scale rows
              _Stub(None, None))                                  # a scenario engine without forcing=
    for other in others:
        with pytest.raises(ValueError, match="forcing set"):
            other.load_state_dict(state)
    plain_scen = {"n_scenarios": 2, "drive_sha256": "d" * 64}
    with pytest.raises(ValueError, match="forcing set"):
        mine.load_state_dict(plain_scen)                          # a checkpoint of a scenario run without forcing=
    with pytest.raises(ValueError, match="scenario set"):
        mine.load_state_dict(dict(state, drive_sha256="e" * 64))  # the same forcing set under other emissions
    with pytest.raises(KeyError, match="'R'"):
        mine.load_state_dict(state)                               # the same sets pass both checks and go on to the state
