"""The scenario axis (ABI v13) without a GPU: the entry points are exported and bound, every bad argument returns
FIVEEQ_E_INVALID on the host (fake pointers are never dereferenced, nothing is launched), the stacked drive table, and the
scenario CSV files."""
import ctypes

import numpy as np
import pytest

from fiveeqscm_amd import _capi, emissions, scenario
from fiveeqscm_amd import params as prm
from fiveeqscm_amd.engine import _is_scenario_set

NEW = ("fiveeq_run_scen_f64", "fiveeq_run_scen_f32", "fiveeq_plan_create_scen_f64", "fiveeq_plan_create_scen_f32",
       "fiveeq_max_scenarios")


def test_the_scenario_entry_points_are_exported_and_bound():
    lib = _capi.load()
    assert _capi.ABI_VERSION == 13 == lib.fiveeq_abi_version()
    for name in NEW:
        assert name in _capi.SIGNATURES and getattr(lib, name) is not None
    assert lib.fiveeq_max_scenarios() == 64
    # the arguments of fiveeq_run_obs_* with n_scen in place of (obs, misfit): 19
    assert len(_capi.SIGNATURES["fiveeq_run_scen_f64"][1]) == len(_capi.SIGNATURES["fiveeq_run_obs_f64"][1]) - 1 == 19


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_every_bad_argument_is_refused_on_the_host(sfx):
    lib = _capi.load()
    run, plan = getattr(lib, f"fiveeq_run_scen_{sfx}"), getattr(lib, f"fiveeq_plan_create_scen_{sfx}")
    m = prm.make_model(prm.default_params("multigas"))
    p = ctypes.c_void_p(0x1000)

    def call(n_scen=2, drive=p, t0=0, t1=4, R=p, S=p, form=_capi.FORM_PER_STEP, k=0, model=m):
        return run(ctypes.byref(model), 8, 8, n_scen, drive, 4, t0, t1, p, p, R, S, None, None, 0, None, form, k, None)

    def err():
        return lib.fiveeq_last_error()

    for n_scen in (0, -1, lib.fiveeq_max_scenarios() + 1):
        assert call(n_scen=n_scen) == _capi.E_INVALID and b"n_scen" in err()
    assert call(drive=None) == _capi.E_INVALID and b"NULL" in err()
    assert call(R=None) == _capi.E_INVALID and b"NULL" in err()
    assert call(S=None) == _capi.E_INVALID and b"NULL" in err()
    assert call(form=2) == _capi.E_INVALID and b"form" in err()
    assert call(form=_capi.FORM_FUSED, k=-1) == _capi.E_INVALID and b"k_steps" in err()
    assert call(t0=-1) == _capi.E_INVALID and b"step range" in err()
    assert call(t1=5) == _capi.E_INVALID and b"step range" in err()
    assert call(t0=3, t1=2) == _capi.E_INVALID and b"step range" in err()
    # an empty range is validated and launches nothing; so is the largest scenario count
    assert call(t0=2, t1=2) == _capi.OK
    assert call(n_scen=lib.fiveeq_max_scenarios(), t0=4, t1=4, form=_capi.FORM_FUSED) == _capi.OK
    bad = prm.make_model(prm.default_params("multigas"))
    bad.dt = -1.0
    assert call(model=bad) == _capi.E_INVALID
    out = ctypes.c_void_p(0x1)

    def mk(n_scen=2, t0=0, t1=4, drive=p):
        return plan(ctypes.byref(m), 8, 8, n_scen, drive, 4, t0, t1, p, p, p, p, None, None, 0, None, ctypes.byref(out))

    assert mk(n_scen=0) == _capi.E_INVALID and out.value is None
    assert mk(n_scen=65) == _capi.E_INVALID and b"n_scen" in err()
    assert mk(drive=None) == _capi.E_INVALID and b"NULL" in err()
    assert mk(t0=1, t1=1) == _capi.E_INVALID and b"empty" in err()
    assert mk(t1=9) == _capi.E_INVALID and b"step range" in err()
    assert plan(ctypes.byref(m), 8, 8, 2, p, 4, 0, 4, p, p, p, p, None, None, 0, None, None) == _capi.E_INVALID


def test_every_layout_takes_the_scenario_forms_on_the_host():
    """All compiled pool layouts get as far as the launch check: an empty range is FIVEEQ_OK for each of them."""
    lib = _capi.load()
    p = ctypes.c_void_p(0x1000)
    for pools in ([1], [2], [3], [4], [1, 1], [4, 1], [4, 4], [1, 1, 1], [4, 1, 1], [4, 4, 1], [4, 4, 4]):
        base = prm.default_params("multigas" if len(pools) == 3 else "co2")
        m = prm.make_model(base)
        m.n_gas = len(pools)
        for g, n in enumerate(pools):
            m.gas[g].n_pools = n
            for i in range(4):
                m.gas[g].a[i], m.gas[g].tau[i] = (1.0, 10.0) if i >= n or m.gas[g].tau[i] <= 0 else (m.gas[g].a[i], m.gas[g].tau[i])
            m.gas[g].g1 = m.gas[g].g1 or 1.0
            m.gas[g].C0 = m.gas[g].C0 or 1.0
            m.gas[g].emis2conc = m.gas[g].emis2conc or 1.0
        for form in (_capi.FORM_PER_STEP, _capi.FORM_FUSED):
            rc = lib.fiveeq_run_scen_f64(ctypes.byref(m), 8, 8, 3, p, 4, 2, 2, p, p, p, p, None, None, 0, None, form, 0, None)
            assert rc == _capi.OK, (pools, lib.fiveeq_last_error())


def test_make_scenario_drive_stacks_per_scenario_tables_with_one_row_map():
    n, G = 40, 3
    base = emissions.rcp_like_emissions(n, G)
    E = np.stack([base, 1.5 * base, 0.5 * base])
    F = np.stack([np.full(n, 0.1), np.zeros(n), np.linspace(0, 1, n)])
    d = emissions.make_scenario_drive(E, F, dt=1.0, output_steps=[3, 7, 39])
    assert d.shape == (3, n, 8)
    for s in range(3):
        np.testing.assert_array_equal(d[s], emissions.make_drive(E[s], F[s], 1.0, [3, 7, 39]))
        np.testing.assert_array_equal(d[s, 1:, 3:6], np.cumsum(E[s], axis=0)[:-1])      # each scenario's own cumulative column
        np.testing.assert_array_equal(d[s, :, 7], d[0, :, 7])                           # one row map
    assert list(np.nonzero(d[0, :, 7] >= 0)[0]) == [3, 7, 39]
    # a sequence of [n_steps, G] arrays and a shared F_ext
    d2 = emissions.make_scenario_drive([E[0], E[1]], np.full(n, 0.2))
    assert d2.shape == (2, n, 8) and (d2[:, :, 6] == 0.2).all()
    assert np.array_equal(d2[1], emissions.make_drive(E[1], np.full(n, 0.2)))


def test_make_scenario_drive_refuses_bad_shapes():
    E = emissions.rcp_like_emissions(20, 3)
    with pytest.raises(ValueError):
        emissions.make_scenario_drive(E)                          # 2-D: one scenario, not a set
    with pytest.raises(ValueError):
        emissions.make_scenario_drive([E, E[:10]])                # scenarios of different lengths
    with pytest.raises(ValueError):
        emissions.make_scenario_drive(np.stack([E, E]), F_ext=np.zeros((3, 20)))
    with pytest.raises(ValueError):
        emissions.make_scenario_drive(np.stack([E, E]), F_ext=np.zeros(19))
    bad = np.stack([E, E])
    bad[1, 3, 0] = np.nan
    with pytest.raises(ValueError):
        emissions.make_scenario_drive(bad)
    # make_drive itself still refuses a 3-D input: no single-scenario call changes meaning
    with pytest.raises(ValueError):
        emissions.make_drive(np.stack([E, E]))


def test_which_emissions_make_a_scenario_engine():
    E = emissions.rcp_like_emissions(20, 3)
    assert _is_scenario_set(np.stack([E, E])) and _is_scenario_set([E, E]) and _is_scenario_set((E,))
    assert not _is_scenario_set(E) and not _is_scenario_set(E[:, 0]) and not _is_scenario_set(E.tolist())
    assert not _is_scenario_set([])


def test_read_emissions_csvs_round_trip_and_refusals(tmp_path):
    n = 30
    years = 1900.0 + np.arange(n)
    base = emissions.rcp_like_emissions(n, 3)
    paths = []
    for i, f in enumerate((1.0, 0.5, 2.0)):
        p = str(tmp_path / f"ssp{i}.csv")
        scenario.write_emissions_csv(p, years, f * base)
        paths.append(p)
    y, E = scenario.read_emissions_csvs(paths)
    assert np.array_equal(y, years) and E.shape == (3, n, 3)
    for i, f in enumerate((1.0, 0.5, 2.0)):
        assert np.array_equal(E[i], f * base)
    other = str(tmp_path / "late.csv")
    scenario.write_emissions_csv(other, years + 1, base)
    with pytest.raises(ValueError, match="years"):
        scenario.read_emissions_csvs(paths + [other])
    short = str(tmp_path / "short.csv")
    scenario.write_emissions_csv(short, years[:-1], base[:-1])
    with pytest.raises(ValueError, match="years"):
        scenario.read_emissions_csvs([paths[0], short])
    co2 = str(tmp_path / "co2.csv")
    scenario.write_emissions_csv(co2, years, base[:, :1], gases=("CO2",))
    with pytest.raises(ValueError, match="CH4"):
        scenario.read_emissions_csvs([paths[0], co2])                # another gas set
    with pytest.raises(ValueError):
        scenario.read_emissions_csvs([])


def test_scenario_summary_csv_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    years = np.array([2030.0, 2050.0, 2100.0])
    names = ["low", "mid", "high"]
    sums = []
    for _ in names:
        pct = np.sort(rng.normal(size=(3, 3)), axis=1)
        sums.append({"count": np.full(3, 17.0), "mean": rng.normal(size=3), "var": rng.random(3), "min": pct[:, 0] - 1,
                     "max": pct[:, 2] + 1, "percentiles": pct})
    path = str(tmp_path / "summary.csv")
    scenario.write_scenario_summary_csv(path, names, years, sums)
    lines = open(path).read().splitlines()
    assert lines[1].split(",") == ["SCENARIO", "YEAR", "COUNT", "MEAN", "STD", "MIN", "P05", "P50", "P95", "MAX"]
    assert len(lines) == 2 + 3 * 3 and lines[2].startswith("low,2030,17,")
    back = scenario.read_scenario_summary_csv(path)
    assert list(back) == names
    for name, s in zip(names, sums):
        y, cols = back[name]
        assert np.array_equal(y, years) and np.array_equal(cols["percentiles"], s["percentiles"])
        assert np.array_equal(cols["mean"], s["mean"]) and np.array_equal(cols["std"], np.sqrt(s["var"]))
        assert cols["levels"] == [5.0, 50.0, 95.0] and np.array_equal(cols["count"], s["count"])
    with pytest.raises(ValueError):
        scenario.write_scenario_summary_csv(path, names[:2], years, sums)
    with pytest.raises(ValueError):
        scenario.write_scenario_summary_csv(path, names, years, [dict(s, percentiles=None) for s in sums])
