#!/usr/bin/env python3
"""The call trace of the two end-of-run summaries (distributed.gather_summary / gather_weighted_summary): which C-ABI passes
run, in which order and with which sizes, which collectives run with which payloads, and what `stats` and the result hold —
on host rows through the NumPy restatements of the passes (oracle/summary_passes.py, fiveeqscm_amd/_wsummary_host.py), in one
process without a GPU.

    python tools/summary_call_trace.py            # writes tests/golden/summary_call_trace.json

tests/test_summary_call_trace_cpu.py imports record() and compares with the committed fixture, so a change of
distributed.py that moves a pass call, a collective or a `stats` value shows up without a GPU and without a second rank.
Cases: K = 3 rows of 1000 members (row 1 constant, row 2 holds a NaN), unweighted and weighted; alone, with
SELECT_CAND_BYTES lowered (the unweighted summary goes through halves of the rows, the weighted one through row blocks), and
in a one-rank gloo group with force_collectives (the exchange branch: every collective executes), with and without the
lowered bound.
"""
import contextlib
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from fiveeqscm_amd import _wsummary_host  # noqa: E402
from fiveeqscm_amd import distributed as D  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "summary_call_trace.json")
K, N, PCT = 3, 1000, (5.0, 50.0, 95.0)
SPLIT_BYTES = {"unweighted": 100, "weighted": 20_000}      # halves of 1 + 2 rows; row blocks of 2 + 1 rows


class RecordingPasses:
    """In front of a pass object: logs every call as [name, non-pointer arguments] and forwards it."""

    def __init__(self, passes, trace):
        self._passes, self._trace = passes, trace

    def __getattr__(self, name):
        fn = getattr(self._passes, name)

        def logged(*a):
            self._trace.append([name] + [v for v in a if not isinstance(v, ctypes.c_void_p)])
            return fn(*a)
        return logged


@contextlib.contextmanager
def recorded(passes, trace):
    """`passes` behind distributed.py's switch and the three collectives of torch.distributed logged into `trace`."""
    import torch.distributed as dist
    saved = D._lib_and_stream, D._passes_apply
    real = {name: getattr(dist, name) for name in ("all_gather", "all_reduce", "gather")}

    def spy(name):
        def f(*a, **k):
            t = a[1] if name == "all_gather" else a[0]         # the payload: all_gather's first argument is the receive list
            trace.append([name, str(t.dtype), list(t.shape)])
            return real[name](*a, **k)
        return f

    proxy = RecordingPasses(passes, trace)
    D._lib_and_stream = lambda rows: (proxy, _wsummary_host._Check, ctypes, None)
    D._passes_apply = lambda rows: rows.dtype in (torch.float32, torch.float64)
    for name in real:
        setattr(dist, name, spy(name))
    try:
        yield
    finally:
        for name, fn in real.items():
            setattr(dist, name, fn)
        D._lib_and_stream, D._passes_apply = saved


def inputs():
    rng = np.random.default_rng(2024)
    x = rng.normal(1.5, 0.7, size=(K, N))
    x[1] = 2.5
    x[2, 77] = np.nan
    w = rng.integers(1, (1 << 32) + 1, size=N, dtype=np.int64)
    w[rng.uniform(size=N) < 0.5] = 0
    return torch.from_numpy(x), torch.from_numpy(w)


def _plain(v):
    """A result or stats value as JSON holds it: floats by their hex form (bit for bit, NaN included)."""
    if isinstance(v, torch.Tensor):
        return [_plain(e) for e in v.tolist()]
    if isinstance(v, (list, tuple)):
        return [_plain(e) for e in v]
    return float(v).hex() if isinstance(v, float) else v


def one_case(kind, split):
    from oracle.summary_passes import SummaryPasses
    x, w = inputs()
    trace, stats = [], {}
    saved = D.SELECT_CAND_BYTES
    if split:
        D.SELECT_CAND_BYTES = SPLIT_BYTES[kind]
    try:
        if kind == "unweighted":
            with recorded(SummaryPasses(), trace):
                out = D.gather_summary(x, PCT, stats=stats)
        else:
            with recorded(_wsummary_host.WeightedPasses(), trace):
                out = D.gather_weighted_summary(x, w, PCT, stats=stats)
    finally:
        D.SELECT_CAND_BYTES = saved
    return {"trace": trace, "stats": {k: _plain(v) for k, v in stats.items()},
            "result": {k: _plain(v) for k, v in out.items()}}


def record():
    """{case name: {"trace", "stats", "result"}} of the eight cases."""
    import torch.distributed as dist
    cases = {}
    for kind in ("unweighted", "weighted"):
        for split in (False, True):
            cases[f"{kind}{'/split' if split else ''}"] = one_case(kind, split)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("gloo", rank=0, world_size=1, init_method=f"tcp://127.0.0.1:{port}")
    prev = D.force_collectives(True)
    try:
        for kind in ("unweighted", "weighted"):
            for split in (False, True):
                cases[f"{kind}/forced{'/split' if split else ''}"] = one_case(kind, split)
    finally:
        D.force_collectives(prev)
        dist.destroy_process_group()
    return cases


def main():
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "-C", ROOT, "status", "--porcelain", "--", "fiveeqscm_amd", "oracle"], capture_output=True,
                           text=True, check=True).stdout.strip()
    doc = {"header": f"recorded by tools/summary_call_trace.py at commit {commit}{' (modified tree)' if dirty else ''}: the pass calls, "
                     "collectives, stats and results of both summaries; tests/test_summary_call_trace_cpu.py compares with it",
           "cases": record()}
    with open(FIXTURE, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(f"{FIXTURE}: {len(doc['cases'])} cases at {commit}")


if __name__ == "__main__":
    main()
