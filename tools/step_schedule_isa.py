#!/usr/bin/env python3
"""Where a per-step kernel's row traffic sits relative to its arithmetic, read from the gfx950 assembly hipcc emits.

    python tools/step_schedule_isa.py FILE.s [LABEL] [kernel-name substring ...]

FILE.s is an assembly written with --save-temps (fiveeq_capi-hip-amdgcn-amd-amdhsa-gfx950.s, see kernel_isa_stats.py).
Default kernels: the fp64 4 + 1 + 1 plain and single-valued-rows kernels, default row policy.  Per kernel: VGPRs, SGPRs,
scratch, waves per SIMD, and one line per EVENT in program order with the index of the instruction it is at:

    load / store     a global_load_* / global_store_* (vector memory; the destination or data registers)
    wait vmcnt(N)    an s_waitcnt that carries a vmcnt field: at most N vector-memory operations stay outstanding behind it
    barrier          the staging s_barrier
    gas g            the compiler-only barrier in front of gas g's arithmetic in member_step() (an empty inline asm, which the
                     assembly marks with ASMSTART / ASMEND)

and a summary line: how many instructions lie between the first and the last store, and the vmcnt values of the waits in
front of each gas body and the thermal step."""
import re
import subprocess
import sys

KERNEL = re.compile(r"^(_Z\w+):\s*; @\1\n(.*?)\.end_amdhsa_kernel", re.S | re.M)
DEFAULT = ("step_kernel<double, 4, 1, 1, false, false, false, false>", "step_uniform_kernel<double, 4, 1, 1, false>")


def events(body):
    """[(instruction index, text)] of the events of one kernel's code, and its instruction count."""
    out, i = [], 0
    gas = 0
    for line in body.split(".section")[0].splitlines():
        if "#ASMSTART" in line:
            out.append((i, f"gas {gas}"))
            gas += 1
            continue
        m = re.match(r"^\s+([a-z]\w+)\s*(.*?)\s*(;.*)?$", line)
        if not m:
            continue
        op, args = m.group(1), m.group(2)
        if op.startswith("global_load"):
            out.append((i, f"load   {op} {args.split(',')[0]}"))
        elif op.startswith("global_store"):
            out.append((i, f"store  {op} {args.split(',')[1].strip()}"))
        elif op.startswith(("global_atomic", "flat_", "buffer_", "scratch_")):
            out.append((i, f"other  {op}"))
        elif op == "s_waitcnt" and "vmcnt" in args:
            out.append((i, "wait   " + re.search(r"vmcnt\(\d+\)", args)[0]))
        elif op == "s_barrier":
            out.append((i, "barrier"))
        i += 1
    return out, i


def report(asm, wanted, label):
    found = [(m.group(1), m.group(2), asm[m.end():m.end() + 4000]) for m in KERNEL.finditer(asm)]
    names = subprocess.run(["c++filt"], input="\n".join(f[0] for f in found), capture_output=True, text=True).stdout.split("\n")
    for (_, body, tail), dem in zip(found, names):
        name = dem.replace("float __vector(2)", "float2v").split("(")[0].replace("void fiveeq::", "")
        if not any(name == w or (w not in DEFAULT and w in name) for w in wanted):
            continue
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body)[1])   # noqa: E731
        after = lambda k: int(re.search(r"; %s: (\d+)" % k, tail)[1])   # noqa: E731
        ev, n_instr = events(body)
        print(f"== {label} {name}")
        print(f"   vgpr {get('next_free_vgpr')} sgpr {get('next_free_sgpr')} scratch {after('ScratchSize')} "
              f"waves/SIMD {after('Occupancy')} instructions {n_instr}")
        for i, text in ev:
            print(f"   {i:5d}  {text}")
        stores = [i for i, t in ev if t.startswith("store")]
        marks = [i for i, t in ev if t.startswith("gas")]
        # the waits that gate each phase: the last one at or before each gas marker's first use is the one behind the marker
        phases = marks + [n_instr]
        gates = []
        for a, b in zip(phases[:-1], phases[1:]):
            gates.append([t.split()[1] for i, t in ev if a <= i < b and t.startswith("wait")])
        print(f"   loads {sum(t.startswith('load') for _, t in ev)} stores {len(stores)}; first store at {stores[0]}, last at "
              f"{stores[-1]}: {stores[-1] - stores[0]} instructions apart; stores ahead of the last gas body's end: "
              f"{sum(s < (marks[-1] if marks else 0) for s in stores)}")
        for g, w in enumerate(gates):
            what = f"gas {g}" + (" and the thermal step" if g == len(gates) - 1 else "")
            print(f"   waits inside {what}: {' '.join(w) or '-'}")
        print()


def main():
    args = sys.argv[1:]
    asm = open(args[0]).read()
    label = args[1] if len(args) > 1 else ""
    report(asm, args[2:] or DEFAULT, label)


if __name__ == "__main__":
    main()
