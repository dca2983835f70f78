"""The single-valued parameter rows of the C ABI (include/fiveeq.h "SINGLE-VALUED PARAMETER ROWS") as far as they go without a
GPU: the symbols are exported and bound, the ABI version and the model size did not move, and every bad argument is refused
with FIVEEQ_E_INVALID and a message before anything is launched (fake pointers only)."""
import ctypes

import pytest

from fiveeqscm_amd import _capi
from fiveeqscm_amd import params as prm

SYMBOLS = [f"fiveeq_{name}_{sfx}" for name in ("uniform_rows", "run_uniform", "plan_create_uniform") for sfx in ("f64", "f32")]


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def test_symbols_exported_and_bound(lib):
    for name in SYMBOLS:
        assert name in _capi.SIGNATURES
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(_capi.SIGNATURES[name][1])
    # the run's arguments are fiveeq_run's plus (mask, values) in front of the stream; the plan's in front of plan_out
    for sfx in ("f64", "f32"):
        run, uni = _capi.SIGNATURES[f"fiveeq_run_{sfx}"][1], _capi.SIGNATURES[f"fiveeq_run_uniform_{sfx}"][1]
        assert uni == run[:-1] + [ctypes.c_uint32, ctypes.c_void_p] + run[-1:]
        plan, uni = _capi.SIGNATURES[f"fiveeq_plan_create_{sfx}"][1], _capi.SIGNATURES[f"fiveeq_plan_create_uniform_{sfx}"][1]
        assert uni == plan[:-1] + [ctypes.c_uint32, ctypes.c_void_p] + plan[-1:]


def test_abi_and_model_size_unchanged(lib):
    assert lib.fiveeq_abi_version() == 13 == _capi.ABI_VERSION
    assert lib.fiveeq_sizeof_model() == 448 == ctypes.sizeof(_capi.Model)


def test_header_declares_them():
    import os
    with open(os.path.join(os.path.dirname(_capi.SOURCES[-1]), "fiveeq.h")) as fh:
        text = fh.read()
    for name in SYMBOLS:
        assert f"int {name}(" in text
    assert "#define FIVEEQ_ABI_VERSION   13" in text


def _run(lib, sfx, plan, mask, values, n_gas=3, n=8):
    model = prm.make_model(prm.default_params("multigas"))
    model.n_gas = n_gas
    p = ctypes.c_void_p(0x1000)
    args = [ctypes.byref(model), n, 8, p, 4, 0, 4, p, p, p, p, None, None, 0, None, mask, values]
    out = ctypes.c_void_p(0xDEAD)
    if plan:
        rc = getattr(lib, f"fiveeq_plan_create_uniform_{sfx}")(*args, ctypes.byref(out))
    else:
        rc = getattr(lib, f"fiveeq_run_uniform_{sfx}")(*args, None)
    return rc, lib.fiveeq_last_error().decode(), out.value


@pytest.mark.parametrize("sfx", ["f64", "f32"])
@pytest.mark.parametrize("plan", [False, True])
def test_run_refusals(lib, sfx, plan):
    vals = ((ctypes.c_double if sfx == "f64" else ctypes.c_float) * 11)()
    # bits at or above 3G + 2: G = 3 -> 11 rows, G = 2 -> 8, G = 1 -> 5
    for n_gas, mask in ((3, 1 << 11), (3, 0x80000000), (3, 0xFFFFFFFF), (2, 1 << 8), (1, 1 << 5)):
        rc, msg, out = _run(lib, sfx, plan, mask, vals, n_gas=n_gas)
        assert rc == _capi.E_INVALID and "uniform mask" in msg and f"above {3 * n_gas + 2}" in msg, (n_gas, mask, msg)
        assert not plan or out is None                      # a refused plan_create leaves NULL
    # ... also with values NULL (the mask is looked at first)
    rc, msg, _ = _run(lib, sfx, plan, 1 << 11, None)
    assert rc == _capi.E_INVALID and "uniform mask" in msg
    # a non-zero mask without values: every bit, every layout (with the form or without it)
    for n_gas, mask in ((3, 1), (3, 0x190), (3, 0x7FF), (2, 0xFF), (1, 0x10)):
        rc, msg, out = _run(lib, sfx, plan, mask, None, n_gas=n_gas)
        assert rc == _capi.E_INVALID and "uniform values is NULL" in msg, (n_gas, mask, msg)
        assert not plan or out is None
    # the base arguments come first
    rc, msg, _ = _run(lib, sfx, plan, 1 << 11, None, n=0)
    assert rc == _capi.E_INVALID and "n_members=0 must be >= 1" in msg


@pytest.mark.parametrize("sfx", ["f64", "f32"])
def test_scan_refusals(lib, sfx):
    fn = getattr(lib, f"fiveeq_uniform_rows_{sfx}")
    mask = ctypes.c_uint32(0xABCD)
    vals = ((ctypes.c_double if sfx == "f64" else ctypes.c_float) * 11)()
    p, m = ctypes.c_void_p(0x1000), ctypes.byref(mask)
    cases = [
        ((0, 8, 9, p, p, m, vals), "n_members=0 must be >= 1"),
        ((9, 8, 9, p, p, m, vals), "ld=8 < n_members=9"),
        ((8, 8, 0, p, p, m, vals), "n_r_rows=0"),
        ((8, 8, 4, p, p, m, vals), "n_r_rows=4"),
        ((8, 8, 12, p, p, m, vals), "n_r_rows=12"),
        ((8, 8, 9, None, p, m, vals), "NULL device pointer"),
        ((8, 8, 9, p, None, m, vals), "NULL device pointer"),
        ((8, 8, 9, ctypes.c_void_p(0x1002), p, m, vals), "aligned"),
        ((8, 8, 9, p, p, None, vals), "NULL output pointer"),
        ((8, 8, 9, p, p, m, None), "NULL output pointer"),
    ]
    for args, text in cases:
        rc = fn(*args, None)
        assert rc == _capi.E_INVALID and text in lib.fiveeq_last_error().decode(), (args[:3], lib.fiveeq_last_error())
    assert mask.value == 0xABCD                             # a refused scan writes nothing
