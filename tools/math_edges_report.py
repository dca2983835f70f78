#!/usr/bin/env python3
"""Worst ulp error of the device's math primitives per op, precision and family of tests/math_reference.py, with the
argument that produced it: what profiles/r19/math_edges.txt records.  Needs the MI355X.

    python tools/math_edges_report.py > math_edges.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import math_reference as mr
    import test_math_edges_gpu as t
    from fiveeqscm_amd import _capi
    lib = _capi.load()
    print("# device math primitives (fiveeq_math.hpp) through fiveeq_math_probe_*: worst ulp error against the exact value")
    print("# (tests/math_reference.py: mpmath on the structured families, long double / fp64 on 'dense'), and where")
    print("# prec op     family      worst_ulp  cap   x                          got                        exact(rounded to double)")
    for prec in mr.PRECS:
        for op in mr.OPS:
            worst, (x, fam, names, got, want, u) = t.measure(lib, op, prec)
            for name, (uu, xx, gg, ww) in worst.items():
                print(f"{prec}  {op:6s} {name:11s} {uu:9.4f}  {mr.CAPS[prec, op]:<4} {float(xx).hex():26s} {float(gg).hex():26s} {float(ww).hex()}")
            if (prec, op) == ("f32", "log"):
                print(f"{prec}  {op:6s} mean over all points {u[x != 1].mean():.4f} (cap {mr.F32_LOG_MEAN_CAP})")


if __name__ == "__main__":
    main()
