"""Which refusal a forward-run call reports when TWO of its arguments are wrong at once, for every family of the C ABI
(include/fiveeq.h): plain, obs (the misfit), scen (the scenario axis), forc (forcing scales) without and with the misfit, and
scen_forc — `run` and `plan_create`, fp64 and fp32.  The checks of a call run in a fixed order and the first that fails is
reported; callers and the other suites match on these texts, so the order is part of the interface.  ORDER below was recorded
from the library as it stood BEFORE the host layer was gathered into one preparation (one check chain per family then): it is
the yardstick for that one chain, not a description of it.  Fake pointers only, nothing is launched: no GPU needed."""
import ctypes
import itertools

import pytest

from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm

# family: (symbol of the run, symbol of the plan, scenario axis?, the arguments the feature adds, as names of _call's keywords)
FAMILIES = {
    "plain": ("run_ksteps", "plan_create", False, ()),                  # (run_ksteps: the plain run that takes a k_steps)
    "obs": ("run_obs", "plan_create_obs", False, ("obs", "misfit")),
    "scen": ("run_scen", "plan_create_scen", True, ()),
    "forc": ("run_forc", "plan_create_forc", False, ("fscale", "fext", "n_fext", "obs", "misfit")),
    "forc_obs": ("run_forc", "plan_create_forc", False, ("fscale", "fext", "n_fext", "obs", "misfit")),
    "scen_forc": ("run_scen_forc", "plan_create_scen_forc", True, ("fscale", "fext", "n_fext")),
}
# what a family's valid call differs in from _call's defaults
DEFAULTS = {"plain": dict(k_steps=1), "forc": dict(obs=0, misfit=0)}

# fault: ({family or "*": the keywords that make it}, {family or "*": what the refusal says})
FAULTS = {
    "n_scen": ({"*": dict(n_scen=0)}, {"*": "n_scen=0 outside 1..64"}),
    "n_scen_min": ({"*": dict(n_scen=-2 ** 31)}, {"*": "n_scen=-2147483648 outside 1..64"}),      # no value of n_scen is a flag
    "n_members": ({"*": dict(n=0)}, {"*": "n_members=0 must be >= 1"}),
    "fscale_null": ({"*": dict(fscale=0)}, {"*": "fscale is NULL"}),
    "fscale_odd": ({"*": dict(fscale=0x2001)}, {"*": "fscale must be"}),
    "lone_obs": ({"*": dict(misfit=0), "forc": dict(obs=0x4000)},
                 {"obs": "NULL misfit pointer", "*": "obs and misfit go together"}),
    "obs_odd": ({"*": dict(obs=0x4001)}, {"*": "obs and misfit must be 8-byte aligned"}),
    "layout": ({"*": dict(n_gas=2)}, {"obs": "pool layout 410 has no misfit form", "*": "pool layout 410 has no forcing form"}),
    "form": ({"*": dict(form=2)}, {"*": "form=2: FIVEEQ_FORM_PER_STEP"}),
    "k_steps": ({"*": dict(k_steps=-1)}, {"*": "k_steps=-1 must be >="}),
    "plan_out": ({"*": dict(plan_out=False)}, {"*": "plan_out is NULL"}),
    "empty": ({"*": dict(t0=2, t1=2)}, {"*": "empty step range for a plan"}),
}

# (family, plan?): the family's faults, the one reported first when two are present coming first
ORDER = {
    ("plain", False): ("n_members", "k_steps"),
    ("plain", True): ("plan_out", "n_members", "empty"),
    ("obs", False): ("n_members", "lone_obs", "obs_odd", "layout", "form", "k_steps"),
    ("obs", True): ("plan_out", "n_members", "lone_obs", "obs_odd", "layout", "empty"),
    ("scen", False): ("n_scen", "n_scen_min", "n_members", "form", "k_steps"),
    ("scen", True): ("n_scen", "n_scen_min", "plan_out", "n_members", "empty"),
    ("forc", False): ("n_members", "fscale_null", "fscale_odd", "layout", "lone_obs", "form", "k_steps"),
    ("forc", True): ("plan_out", "n_members", "fscale_null", "fscale_odd", "layout", "lone_obs", "empty"),
    ("forc_obs", False): ("n_members", "fscale_null", "fscale_odd", "layout", "lone_obs", "obs_odd", "form", "k_steps"),
    ("forc_obs", True): ("plan_out", "n_members", "fscale_null", "fscale_odd", "layout", "lone_obs", "obs_odd", "empty"),
    ("scen_forc", False): ("n_scen", "n_scen_min", "n_members", "fscale_null", "fscale_odd", "layout", "form", "k_steps"),
    ("scen_forc", True): ("n_scen", "n_scen_min", "plan_out", "n_members", "fscale_null", "fscale_odd", "layout", "empty"),
}


def _of(table, family):
    return table.get(family, table["*"])


def _call(lib, family, sfx, plan, *, n_gas=3, n=8, ld=8, n_scen=2, t0=0, t1=4, fscale=0x2000, fext=0x3000, n_fext=2,
          obs=0x4000, misfit=0x5000, form=_capi.FORM_PER_STEP, k_steps=0, plan_out=True):
    """One call of the family's run or plan_create; returns (rc, message, what the call left in *plan_out)."""
    run, create, scen, feature = FAMILIES[family]
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas                              # 2: pools 4 + 1, a compiled layout without the misfit or forcing form
    p, given = ctypes.c_void_p(0x1000), locals()
    args = [ctypes.byref(model), n, ld] + ([n_scen] if scen else []) + [p, 4, t0, t1, p, p, p, p, None, None, 0, None]
    args += [given[k] if k == "n_fext" else ctypes.c_void_p(given[k]) for k in feature]
    out = ctypes.c_void_p(0xDEAD)
    if plan:
        rc = getattr(lib, f"fiveeq_{create}_{sfx}")(*args, ctypes.byref(out) if plan_out else None)
    else:
        tail = [k_steps] if family == "plain" else [form, k_steps]
        rc = getattr(lib, f"fiveeq_{run}_{sfx}")(*args, *tail, None)
    return rc, lib.fiveeq_last_error().decode(), out.value


def _pairs(family, plan):
    """Every two faults of the family that can be made at once (not two values of one argument), the expected winner first."""
    for a, b in itertools.combinations(ORDER[family, plan], 2):
        kw_a, kw_b = _of(FAULTS[a][0], family), _of(FAULTS[b][0], family)
        if not set(kw_a) & set(kw_b):
            yield a, b, {**kw_a, **kw_b}


@pytest.mark.parametrize("plan", [False, True])
@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_of_two_faults_the_earlier_check_is_reported(family, sfx, plan):
    lib = _capi.load()
    base = DEFAULTS.get(family, {})
    # the yardstick's own footing: the valid call passes every check (an empty range launches nothing; a plan refuses it last) ...
    rc, msg, _ = _call(lib, family, sfx, plan, **{**base, "t0": 2, "t1": 2})
    assert "empty step range for a plan" in msg if plan else rc == _capi.OK, (family, rc, msg)
    # ... and each fault alone draws its own text
    for name in ORDER[family, plan]:
        rc, msg, out = _call(lib, family, sfx, plan, **{**base, **_of(FAULTS[name][0], family)})
        assert rc == _capi.E_INVALID and _of(FAULTS[name][1], family) in msg, (family, name, rc, msg)
    seen = 0
    for first, second, kw in _pairs(family, plan):
        rc, msg, out = _call(lib, family, sfx, plan, **{**base, **kw})
        print(f"{family} {sfx} plan={plan}: {first} + {second} -> {msg}")
        assert rc == _capi.E_INVALID, (family, first, second, rc, msg)
        assert _of(FAULTS[first][1], family) in msg, (family, first, second, msg)
        assert _of(FAULTS[second][1], family) not in msg, (family, first, second, msg)
        if plan and "plan_out" not in (first, second):
            assert out is None, (family, first, second)          # a refused plan call leaves *plan_out NULL
        seen += 1
    assert seen
