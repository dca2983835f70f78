"""The helpers the row-pass wrappers share (fiveeqscm_amd/_rowargs.py): pure functions of shapes, strides and host values, so
they run on CPU tensors.  The layout table states, per caller, what the wrappers' own inline expressions decided before the
helper existed (profiles/r23/NOTES.md: how it was filled)."""
import types

import numpy as np
import pytest
import torch

from fiveeqscm_amd import _capi, joint, metrics
from fiveeqscm_amd._rowargs import (bool_mask, dev_rows, drive_table, forcing_tables, int_weights, model_steps, steps_i32,
                                    steps_in_tables, walk_in_place)
from fiveeqscm_amd.forcing import ExternalForcings, ScenarioForcings

N = 5
EXT = {"S": 2, "K": 3, "G": 2}


def _zeros(axes, n=N, **ext):
    return torch.zeros(tuple(ext.get(a, EXT[a]) for a in axes) + (n,), dtype=torch.float64)


def _on(axes, a, s):
    return tuple(s if b == a else slice(None) for b in axes)


def _layouts(axes):
    """name -> view [*axes, members] for the leading axes named (S scenarios, K rows, G gases or quantities)."""
    out = {"contiguous": _zeros(axes), "members 1:4": _zeros(axes)[..., 1:4], "members ::2": _zeros(axes)[..., ::2],
           "N = 1": _zeros(axes, 4)[..., ::4]}
    for a in axes:
        out[f"{a} ::2"] = _zeros(axes, **{a: 2 * EXT[a]})[_on(axes, a, slice(None, None, 2))]
        out[f"{a} expanded"] = _zeros(axes, **{a: 1}).expand(tuple(EXT[b] for b in axes) + (N,))
        out[f"{a} = 1"] = _zeros(axes, **{a: 2})[_on(axes, a, slice(0, 2, 2))]               # one entry, at twice the usual stride
    if "K" in axes:
        out["K = 0"] = _zeros(axes, K=0)
    if "K" in axes and "G" in axes:
        i, j = axes.index("K"), axes.index("G")
        swapped = list(axes)
        swapped[i], swapped[j] = "G", "K"
        out["G transposed"] = _zeros(tuple(swapped)).transpose(i, j)
    if axes == ("S", "K"):
        out["ld = 2 N - 1"] = _zeros(axes, 2 * N - 1)[..., :N]
        out["ld = 2 N"] = _zeros(axes, 2 * N)[..., :N]
        out["S expanded, K = 0"] = _zeros(axes, S=1, K=0).expand(2, 0, N)
        out["S ::2, K = 1"] = _zeros(axes, S=4, K=2)[::2, 0:2:2]
    if axes == ("K",):
        out["N = 0"] = torch.zeros((3, 0), dtype=torch.float64)
        out["K = 1, N = 0"] = torch.zeros((1, 0), dtype=torch.float64)
    return out


_plain = lambda x: walk_in_place(x, x.shape[-1])                                            # noqa: E731
_lead = lambda x: walk_in_place(x, x.shape[-1], always=(0,))                                # noqa: E731
# caller -> (leading axes, the call as the wrapper makes it -> (tensor, strides), layout -> (copied?, strides))
_ROWS_GASES = {                                             # views [3, 2, 5]
    "contiguous": (False, (10, 5)),
    "members 1:4": (False, (10, 5)),                        # strides (10, 5, 1): in place, rows 5 apart per gas
    "members ::2": (True, (6, 3)),
    "N = 1": (False, (8, 4)),                               # strides (8, 4, 4): the member stride is not examined
    "K ::2": (False, (20, 5)),
    "K expanded": (True, (10, 5)),                          # a row stride of 0
    "K = 1": (False, (5, 5)),                               # lies at (20, 5, 1)
    "G ::2": (False, (20, 10)),
    "G expanded": (True, (10, 5)),
    "G = 1": (False, (10, 5)),                              # lies at (10, 10, 1)
    "K = 0": (False, (5, 5)),
    "G transposed": (False, (5, 15)),
}
_ROWS = {                                                   # views [3, 5]
    "contiguous": (False, (5,)),
    "members 1:4": (False, (5,)),
    "members ::2": (True, (3,)),
    "N = 1": (False, (4,)),
    "K ::2": (False, (10,)),
    "K expanded": (True, (5,)),
    "K = 1": (False, (5,)),                                 # lies at (10, 1)
    "K = 0": (False, (5,)),
}
PROFILES = {
    "score": (("K", "G"), _plain, _ROWS_GASES),
    "forcing C": (("K", "G"), _plain, _ROWS_GASES),
    "forcing T": (("K",), _plain, dict(_ROWS, **{"N = 0": (False, (1,)), "K = 1, N = 0": (False, (0,))})),
    "pulse C": (("S", "K", "G"), _lead, {                  # views [2, 3, 2, 5]
        "contiguous": (False, (30, 10, 5)),
        "members 1:4": (False, (30, 10, 5)),
        "members ::2": (True, (18, 6, 3)),
        "N = 1": (False, (24, 8, 4)),
        "S ::2": (False, (60, 10, 5)),
        "S expanded": (True, (30, 10, 5)),
        "S = 1": (False, (60, 10, 5)),                      # the scenario stride as it lies (the wrapper refuses S < 2 anyway)
        "K ::2": (False, (60, 20, 5)),
        "K expanded": (True, (30, 10, 5)),
        "K = 1": (False, (20, 5, 5)),                       # lies at (20, 20, 5, 1)
        "G ::2": (False, (60, 20, 10)),
        "G expanded": (True, (30, 10, 5)),
        "G = 1": (False, (30, 10, 5)),                      # lies at (30, 10, 10, 1)
        "K = 0": (False, (10, 5, 5)),
        "G transposed": (False, (30, 5, 15)),
    }),
    "pulse T": (("S", "K"), _lead, {                       # views [2, 3, 5]
        "contiguous": (False, (15, 5)),
        "members 1:4": (False, (15, 5)),
        "members ::2": (True, (9, 3)),
        "N = 1": (False, (12, 4)),
        "S ::2": (False, (30, 5)),
        "S expanded": (True, (15, 5)),
        "S = 1": (False, (30, 5)),
        "K ::2": (False, (30, 10)),
        "K expanded": (True, (15, 5)),
        "K = 1": (False, (10, 5)),
        "K = 0": (False, (5, 5)),
        "ld = 2 N - 1": (False, (27, 9)),
        "ld = 2 N": (False, (30, 10)),                      # only the metrics mind a wide buffer
        "S expanded, K = 0": (False, (0, 5)),               # (an empty view is its own contiguous copy)
        "S ::2, K = 1": (False, (20, 5)),
    }),
    "pulse fscale": (("G",), _lead, {        # views [2, 5]
        "contiguous": (False, (5,)),
        "members 1:4": (False, (5,)),
        "members ::2": (True, (3,)),
        "N = 1": (False, (4,)),
        "G ::2": (False, (10,)),
        "G expanded": (True, (5,)),
        "G = 1": (False, (10,)),                            # one row of scales reports the stride it lies at
    }),
    "metrics": (("S", "K"), lambda x: (lambda r: (r[0], (r[2], r[1])))(metrics._rows_in_place(x)), {     # (scen_stride, ld)
        "contiguous": (False, (15, 5)),
        "members 1:4": (False, (15, 5)),                    # ld = 5 < 2 * 3
        "members ::2": (True, (9, 3)),
        "N = 1": (True, (3, 1)),                            # ld = 4 >= 2 * 1
        "S ::2": (False, (30, 5)),
        "S expanded": (True, (15, 5)),                      # scenario blocks less than K ld apart
        "S = 1": (False, (15, 5)),                          # K ld, whatever the view says
        "K ::2": (True, (15, 5)),                           # ld = 10 >= 2 N
        "K expanded": (True, (15, 5)),
        "K = 1": (False, (10, 5)),
        "K = 0": (False, (0, 5)),
        "ld = 2 N - 1": (False, (27, 9)),
        "ld = 2 N": (True, (15, 5)),
        "S expanded, K = 0": (False, (0, 5)),
        "S ::2, K = 1": (False, (20, 5)),
    }),
    "joint": (("K",), lambda x: (lambda r: (r[0], (r[1],)))(joint._in_place(x)),
              dict(_ROWS, **{"N = 0": (False, (1,)), "K = 1, N = 0": (False, (1,))})),
}


@pytest.mark.parametrize("caller", list(PROFILES))
def test_walk_in_place_decides_and_reports_what_the_wrappers_did(caller):
    axes, call, want = PROFILES[caller]
    views = _layouts(axes)
    assert set(views) == set(want)
    for name, v in views.items():
        got, strides = call(v)
        assert ((got is not v), strides) == want[name], (caller, name, tuple(v.shape), v.stride())
        assert got is v or (got.is_contiguous() and torch.equal(got, v))
        assert all(isinstance(s, int) for s in strides)


def test_walk_in_place_copies_on_the_callers_word_and_skips_the_callers_axes():
    x = _zeros(("S", "K"))
    got, strides = walk_in_place(x, N, copy=True)
    assert got is x and strides == (15, 5)                        # (a contiguous tensor is its own contiguous copy)
    wide = _zeros(("S", "K"), 7)[..., :N]
    got, strides = walk_in_place(wide, N, copy=True)
    assert got is not wide and strides == (15, 5)
    lone = _zeros(("S", "K"), S=1).expand(2, 3, N)                # first=1: the scenario axis is not judged and not reported
    got, strides = walk_in_place(lone, N, first=1)
    assert got is lone and strides == (5,)


STEP_OPTIONS = {"score": dict(n_steps=40), "forcing": {}, "pulse": dict(increasing=False), "metrics": dict(non_negative=True)}


@pytest.mark.parametrize("caller", list(STEP_OPTIONS))
def test_model_steps_refusals(caller):
    opt = STEP_OPTIONS[caller]
    for K, bad in ((3, [1, 2]), (3, [[1, 2, 3]]), (3, [1.0, 2.0, 3.0]), (0, [1]), (1, 7)):
        with pytest.raises(ValueError, match=f"^steps: want {K} integers, one per row$"):
            model_steps(bad, K, **opt)
    st = model_steps([], 0, **opt)                                # no rows: an empty list is float64 to NumPy, and passes
    assert st.dtype == np.int64 and st.shape == (0,)
    st = model_steps(np.array([3, 4, 9], dtype=np.int32), 3, **opt)
    assert st.dtype == np.int64 and st.tolist() == [3, 4, 9]
    assert model_steps(range(5, 6), 1, **opt).tolist() == [5]
    disorder = ([3, 3, 4], [4, 3, 5])
    if caller == "pulse":                                         # the caller asks for consecutive steps itself
        assert [model_steps(b, 3, **opt).tolist() for b in disorder] == [list(b) for b in disorder]
        assert model_steps([-2, -1, 0], 3, **opt).tolist() == [-2, -1, 0]
    elif caller == "metrics":
        for b in disorder + ([-1, 0, 1], [0, 1, 2 ** 31]):
            with pytest.raises(ValueError, match="^steps: want non-negative, strictly increasing model steps$"):
                model_steps(b, 3, **opt)
        assert model_steps([0, 2 ** 31 - 1], 2, **opt).tolist() == [0, 2 ** 31 - 1]
    else:
        for b in disorder:
            with pytest.raises(ValueError, match="^steps: want strictly increasing model steps$"):
                model_steps(b, 3, **opt)
    if caller == "score":
        for b, text in (([-1, 0, 1], "-1..1"), ([38, 39, 40], "38..40")):
            with pytest.raises(ValueError, match=rf"^steps: {text} outside the tables' steps 0\.\.39$"):
                model_steps(b, 3, **opt)
        assert model_steps([0, 39], 2, **opt).tolist() == [0, 39]
    if caller == "forcing":                                       # no table yet: the range is checked once the drive table stands
        assert model_steps([-1, 0, 50], 3, **opt).tolist() == [-1, 0, 50]


def test_steps_in_tables_and_the_upload():
    steps_in_tables(np.zeros(0, dtype=np.int64), 0)
    steps_in_tables(np.array([0, 9]), 10)
    with pytest.raises(ValueError, match=r"^steps: 0\.\.10 outside the tables' steps 0\.\.9$"):
        steps_in_tables(np.array([0, 10]), 10)
    with pytest.raises(ValueError, match=r"^steps: -3\.\.2 outside the tables' steps 0\.\.9$"):
        steps_in_tables(np.array([-3, 2]), 10)
    up = steps_i32(np.array([1, 5], dtype=np.int64), torch.device("cpu"))
    assert up.dtype == torch.int32 and up.tolist() == [1, 5]


def test_dev_rows_refusals():
    cpu = torch.device("cpu")
    t = torch.zeros((2, 3), dtype=torch.float32)
    for bad in (np.zeros((2, 3), dtype=np.float32), torch.zeros((3, 2), dtype=torch.float32), t.double()):
        with pytest.raises(ValueError, match=r"^q: want a torch.float32 tensor of shape \[2, 3\]$"):
            dev_rows(bad, (2, 3), "q", torch.float32, cpu)
    with pytest.raises(TypeError, match=r"^q must be on the GPU \(got cpu\): there is no CPU path$"):
        dev_rows(t, (2, 3), "q", torch.float32, cpu)


def test_int_weights_and_bool_mask():
    cpu = torch.device("cpu")
    w = torch.tensor([0, 1, 1 << 32], dtype=torch.int64)
    for check in (False, True):
        assert int_weights(w, 3, cpu, check_range=check) is w
        assert int_weights(w[:0], 0, cpu, check_range=check).numel() == 0
        for bad in (w.numpy(), w.to(torch.int32), w[:2], w.reshape(1, 3), torch.empty(3, dtype=torch.int64, device="meta")):
            with pytest.raises(ValueError, match=r"^weights: want an int64 tensor of shape \[3\] on cpu$"):
                int_weights(bad, 3, cpu, check_range=check)
    for bad in (torch.tensor([0, -1, 2]), torch.tensor([0, (1 << 32) + 1, 2])):
        assert int_weights(bad, 3, cpu, check_range=False) is bad             # the range is looked at only where it is asked for
        with pytest.raises(ValueError, match=r"^weights: values outside \[0, 2\^32\]$"):
            int_weights(bad, 3, cpu, check_range=True)
    m = bool_mask([True, False, True], 3, cpu)
    assert m.dtype == torch.bool and m.tolist() == [True, False, True]
    assert bool_mask(np.zeros(0, dtype=bool), 0, cpu).numel() == 0
    for bad in ([1, 0, 1], [True, False], np.ones((1, 3), dtype=bool), torch.ones(3)):
        with pytest.raises(ValueError, match=r"^accepted: want a boolean mask of shape \[3\]$"):
            bool_mask(bad, 3, cpu)


@pytest.mark.parametrize("lead", [(), (2,)])
def test_drive_table_from_host_values(lead):
    cpu, n = torch.device("cpu"), 7
    fe = np.linspace(-1.0, 2.0, n)
    for given in (fe, fe.tolist(), torch.from_numpy(fe)):
        tab = drive_table(given, lead, "F_ext (unused)", torch.float32, cpu)
        assert tab.dtype == torch.float32 and tuple(tab.shape) == lead + (n, _capi.DRIVE_STRIDE)
        want = np.zeros(lead + (n, _capi.DRIVE_STRIDE), dtype=np.float32)
        want[..., 6] = fe.astype(np.float32)
        assert np.array_equal(tab.numpy(), want)
    if lead:
        both = np.stack([fe, 2.0 * fe])
        tab = drive_table(both, lead, "F_ext (unused)", torch.float64, cpu)
        assert np.array_equal(tab[:, :, 6].numpy(), both) and not tab[:, :, :6].any() and not tab[:, :, 7:].any()
        for bad in (np.zeros((3, n)), np.zeros((2, n, 1)), np.float64(1.0)):
            with pytest.raises(ValueError, match=r"^F_ext: want \[n_steps\] or \[2, n_steps\]$"):
                drive_table(bad, lead, "F_ext (unused)", torch.float64, cpu)
    else:                                                         # one scenario: any host shape is read as its values in order
        assert tuple(drive_table(np.zeros((2, n)), lead, "F_ext (unused)", torch.float64, cpu).shape) == (2 * n, _capi.DRIVE_STRIDE)
    # a device table of the pass's rank is taken as it is — once it passes dev_rows, which names it
    table = torch.zeros(lead + (n, _capi.DRIVE_STRIDE), dtype=torch.float64)
    with pytest.raises(TypeError, match=r"^F_ext \(named\) must be on the GPU"):
        drive_table(table, lead, "F_ext (named)", torch.float64, cpu)
    with pytest.raises(ValueError, match=r"^F_ext \(named\): want a torch.float64 tensor of shape \[" + "2, " * len(lead) + r"7, 8\]$"):
        drive_table(table[..., :7], lead, "F_ext (named)", torch.float64, cpu)


@pytest.mark.parametrize("lead", [(), (2,)])
def test_forcing_tables(lead):
    cpu, G, n, n_steps = torch.device("cpu"), 3, 4, 6
    seen = []

    def host_table(X):
        seen.append(X)
        return X if not isinstance(X, np.ndarray) else (ScenarioForcings(X) if lead else ExternalForcings(X))

    def tables(fscale, X):
        return forcing_tables(fscale, X, lead, G, n, n_steps, torch.float64, cpu, together="fscale and X: the caller's sentence",
                              x_name="X (named)", host_table=host_table)
    assert tables(None, None) == (0, None, None) and not seen
    for fscale, X in ((torch.zeros((G, n)), None), (None, np.zeros(lead + (n_steps, 0)))):
        with pytest.raises(ValueError, match="^fscale and X: the caller's sentence$"):
            tables(fscale, X)
    # K from a table object: it shows in the shape asked of fscale, and a good fscale gets as far as the device check
    X = np.arange(float(np.prod(lead + (n_steps, 2)))).reshape(lead + (n_steps, 2))
    with pytest.raises(ValueError, match=r"^fscale: want a torch.float64 tensor of shape \[5, 4\]$"):
        tables(torch.zeros((G, n), dtype=torch.float64), X)
    with pytest.raises(TypeError, match=r"^fscale must be on the GPU \(got cpu\)"):
        tables(torch.zeros((G + 2, n), dtype=torch.float64), X)
    assert len(seen) == 2 and seen[0] is X
    # ... a table object of more categories than the C ABI takes
    wide = types.SimpleNamespace(n_categories=_capi.MAX_FEXT + 1, padded=lambda: np.zeros(lead + (n_steps, _capi.MAX_FEXT)))
    with pytest.raises(ValueError, match=rf"^fscale: 8 rows for 3 gases: want G \+ K rows, K <= {_capi.MAX_FEXT}$"):
        tables(torch.zeros((8, n), dtype=torch.float64), wide)
    # K from fscale's rows when X is a device table: X is named by the caller in its refusals (the rest needs a GPU)
    with pytest.raises(ValueError, match=r"^X \(named\): want a torch.float64 tensor of shape \[" + "2, " * len(lead) + r"6, 4\]$"):
        tables(torch.zeros((G + 1, n), dtype=torch.float64), torch.zeros(lead + (n_steps, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match=r"^X \(named\) must be on the GPU"):
        tables(torch.zeros((G + 1, n), dtype=torch.float64), torch.zeros(lead + (n_steps, _capi.MAX_FEXT), dtype=torch.float64))
