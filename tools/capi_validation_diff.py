#!/usr/bin/env python3
"""Differential check of the C ABI's host validation between two builds of the library.

    FIVEEQ_ALLOW_STALE_LIB=1 python tools/capi_validation_diff.py PARENT.so NEW.so

For every post-processing entry point (the counting, summary, weighted-summary, resampling, metrics, joint, scoring, forcing-row
and pulse passes, fp64 and fp32) the tool starts from one argument set that would pass validation — fake 0x1000-aligned
device pointers that nothing dereferences, small sizes, a valid model — and issues every single perturbation of every
argument and every pair of perturbations of two different arguments:

    integers   -1, 0, one past each documented limit, 2^31
    pointers   NULL, base + 2, base + 4        (host arrays, which validation reads: NULL only)
    strides    n_members - 1 and its negative, 0

Each call goes to both libraries; (return code, fiveeq_last_error()) must agree byte for byte.  Pairs pin the ORDER of the
checks: with two bad arguments the message names the one checked first.  Every difference is printed and the exit status is
non-zero when there is one.

The unperturbed call is never issued, and the tool refuses to run where a GPU is visible: a call that passes validation
launches a kernel on the fake pointers.  Without a GPU such a call returns the HIP error of the failed launch; those calls
are counted ("reached the launch") and compared like the others, so a check lost on one side shows as a difference.
"""
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 8                                   # members of the base calls (ld = N)
TWO31 = 1 << 31
_next_ptr = [0x10000]


class Arg:
    def __init__(self, name, base, values):
        self.name, self.base, self.values = name, base, values


def I(name, base, *limits):
    """an integer: -1, 0, one past each documented limit, 2^31 (whatever of these is not the base value)"""
    vals = [-1, 0] + [lim + 1 for lim in limits] + [TWO31]
    return Arg(name, base, [v for v in dict.fromkeys(vals) if v != base])


def P(name):
    """a device pointer nothing dereferences: NULL, base + 2, base + 4"""
    _next_ptr[0] += 0x1000
    base = _next_ptr[0]
    return Arg(name, base, [None, base + 2, base + 4])


def H(name, ctype, values):
    """a host array that validation reads: NULL only"""
    arr = (ctype * len(values))(*values)
    return Arg(name, arr, [None])


def S(name, base):
    """a stride in members: n_members - 1 and its negative, and 0"""
    return Arg(name, base, [N - 1, -(N - 1), 0])


def K(name, value):
    """an argument that stays what it is (the stream, a flag, a range end)"""
    return Arg(name, value, [])


def specs(lib, model):
    """entry point -> its arguments in order, for both precisions where it has them"""
    max_scen = lib.fiveeq_max_scenarios()
    both = {}

    def add(name, args, suffixes=("_f64", "_f32")):
        for sfx in suffixes:
            both[f"fiveeq_{name}{sfx}"] = args()

    M = lambda: Arg("model", ctypes.pointer(model), [None])
    rows3 = lambda: [I("n_rows", 3, 65535), I("n_members", N), I("ld", N)]
    add("hist_rows", lambda: rows3() + [P("rows"), K("lo", -1.0), K("hi", 3.0), I("n_bins", 16, 4096), P("hist"), K("stream", None)])
    add("hist_rows_ranged", lambda: rows3() + [P("rows"), P("ranges"), I("n_bins", 16, 4096), P("hist"), K("stream", None)])
    add("hist_bins", lambda: rows3() + [P("bins"), I("n_bins", 16, 4096), P("hist"), K("stream", None)], suffixes=("",))
    add("row_moments", lambda: rows3() + [P("rows"), P("partial"), P("moments"), K("stream", None)])
    add("select_bins", lambda: rows3() + [P("rows"), P("ranges"), I("n_bins", 16, 4096), P("binmask"), P("cand"), I("cap", 4), P("cand_n"),
                                         K("stream", None)])
    add("wrow_moments", lambda: rows3() + [P("rows"), P("weights"), P("partial"), P("moments"), K("stream", None)])
    add("whist_rows_ranged", lambda: rows3() + [P("rows"), P("weights"), P("ranges"), I("n_bins", 16, 4096), P("hist"), K("stream", None)])
    add("wselect_bins", lambda: rows3() + [P("rows"), P("weights"), P("ranges"), I("n_bins", 16, 4096), P("binmask"), P("cand"), P("candw"),
                                          I("cap", 4), P("cand_n"), K("stream", None)])
    add("wscan", lambda: [I("n_members", N), P("weights"), P("partial"), P("cum"), P("flags"), K("stream", None)], suffixes=("",))
    add("resample_pick", lambda: [I("n_members", N), P("cum"), K("c_lo", 0), I("M", N), I("q", 1), I("a", 1), I("s", 1, N - 1), I("b", 1, N - 1),
                                  I("j0", 1, N), I("n_out", 4, N - 1), P("src"), K("stream", None)], suffixes=("",))
    add("gather_rows", lambda: [I("n_rows", 3), I("n_out", N), I("ld_in", N), P("rows_in"), I("ld_out", N), P("rows_out"), P("src"),
                                K("stream", None)])
    add("traj_metrics", lambda: [I("n_scen", 2, max_scen), I("n_rows", 3), I("n_members", N), I("ld", N), P("rows"), I("scen_stride", 3 * N),
                                 P("steps"), I("n_levels", 2, 8), H("levels", ctypes.c_double, [1.5, 2.0] + [0.0] * 6), I("n_windows", 1, 4),
                                 H("windows", ctypes.c_int32, [0, 2] + [0] * 6), P("fmet"), P("imet"), I("first_call", 1), K("stream", None)])
    joint = lambda: [I("n_members", N), I("n_x", 2, 32), I("ld_x", N), P("x"), I("n_y", 2, 32), I("ld_y", N), P("y"), P("weights")]
    add("joint_moments", lambda: joint() + [P("pivots"), P("partial"), P("co"), P("margins"), P("info"), P("nanrows"), K("stream", None)])
    add("cond_sums", lambda: joint() + [I("n_bins", 2, 32), P("edges"), P("pivots"), P("partial"), P("sums"), P("binw"), P("xnan"),
                                       K("stream", None)])
    add("score_rows", lambda: [I("n_q", 2, 4), I("n_rows", 3), I("n_members", N), P("rows"), S("row_stride", N), S("q_stride", 3 * N), P("steps"),
                               P("obs"), I("n_steps", 10), P("misfit"), I("ld_m", N), K("stream", None)])
    add("forcing_rows", lambda: [M(), I("n_rows", 3), I("n_members", N), I("ld", N), P("C_rows"), S("c_row_stride", 3 * N), S("c_gas_stride", N),
                                 P("T_rows"), S("t_row_stride", N), P("steps"), P("drive"), I("n_steps", 10), P("q"), P("fscale"),
                                 I("n_fext", 2, 4), P("fext"), P("F"), P("F_gas"), P("N"), P("H"), I("ld_out", N), P("H_io"), P("S_io"),
                                 P("n_mismatch"), K("stream", None)])
    i32 = ctypes.c_int32
    add("pulse_response", lambda: [M(), I("n_scen", 3), I("n_rows", 3), I("n_members", N), I("ld", N), P("C_rows"), S("c_scen_stride", 9 * N),
                                   S("c_row_stride", 3 * N), S("c_gas_stride", N), P("T_rows"), S("t_scen_stride", 3 * N),
                                   S("t_row_stride", N), P("steps"), P("drive"), I("n_steps", 10), P("fscale"), I("n_fext", 2, 4), P("fext"),
                                   I("base", 0, 2), I("n_pulses", 2, 3), H("pulse_scen", i32, [1, 2, 1]), H("pulse_gas", i32, [0, 1, 2]),
                                   I("n_horizons", 2, 8), H("horizons", i32, [1, 2, 3, 4, 5, 6, 7, 8]), I("row0", 1), P("out"),
                                   I("ld_out", N), P("io"), K("stream", None)])
    return both


def call(lib, name, values):
    rc = getattr(lib, name)(*values)
    return rc, lib.fiveeq_last_error() or b""


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    import torch
    if torch.cuda.is_available():
        sys.exit("capi_validation_diff: a GPU is visible; a call that passes validation would launch on fake pointers. "
                 "Run this where there is none.")
    from fiveeqscm_amd import _capi, params
    libs = [_capi.load(os.path.abspath(p)) for p in sys.argv[1:]]
    model = params.make_model(params.default_params("multigas"))
    calls = launched = 0
    diffs = []
    for name, args in specs(libs[0], model).items():
        base = [a.base for a in args]
        singles = [(i, v) for i, a in enumerate(args) for v in a.values]
        pairs = [(p, q) for p, q in itertools.combinations(singles, 2) if p[0] != q[0]]
        for changes in [(s,) for s in singles] + pairs:
            values = list(base)
            for i, v in changes:
                values[i] = v
            got = [call(lib, name, values) for lib in libs]
            calls += 1
            launched += got[0][0] == _capi.E_HIP and got[1][0] == _capi.E_HIP
            if got[0] != got[1]:
                what = ", ".join(f"{args[i].name}={v if not isinstance(v, int) or abs(v) < 4096 else hex(v)}" for i, v in changes)
                diffs.append(f"{name}({what}):\n    {sys.argv[1]}: {got[0]}\n    {sys.argv[2]}: {got[1]}")
    for d in diffs:
        print(d)
    print(f"capi_validation_diff: {calls} calls compared over {len(specs(libs[0], model))} entry points, {launched} of them reached "
          f"the launch in both libraries, {len(diffs)} differences")
    sys.exit(1 if diffs else 0)


if __name__ == "__main__":
    main()
