#!/usr/bin/env python3
"""Static per-kernel facts from the gfx950 assembly hipcc emits: VGPR/SGPR/LDS/scratch and the
instruction mix (VALU by type, SALU, LDS, global).  Runs in the CPU container (cross-compile).

    python tools/kernel_isa_stats.py [substring ...]      # default: the 4+1+1 instantiations
    python tools/kernel_isa_stats.py --digest [FILE.s]    # every kernel: mangled name and sha256 of its assembly
    python tools/kernel_isa_stats.py --compare-forc PARENT.s [NEW.s]   # profiles/r08/forcing_isa.txt
    python tools/kernel_isa_stats.py --compare-scen-forc PARENT.s [NEW.s]   # profiles/r09/scenario_forcing_isa.txt
    python tools/kernel_isa_stats.py --compare-digest PARENT.s [NEW.s]      # profiles/r12/resample_isa.txt

--compare-forc: PARENT.s is the assembly of the commit before the FORC template parameter (step_kernel / fused_kernel gained
it as their last one, default false), NEW.s the tree's (compiled when not given).  Every kernel of PARENT.s is looked up in
NEW.s by its demangled name — with ", false" appended for the two templates — and compared on VGPR, SGPR, LDS, scratch,
occupancy and instruction count; then every FORC = true instantiation is listed beside its FORC = false counterpart.

--compare-scen-forc: the same for the commit before step_scen_kernel gained FORC as its last template parameter (default
false; fused_kernel's parameter list did not change, it gained the SCEN + FORC instantiations): every kernel of PARENT.s
against NEW.s, then every new instantiation beside its SCEN, FORC = false counterpart.

--compare-digest: every kernel of PARENT.s against its namesake in NEW.s by the digest below (the same machine code or not),
then the facts of the kernels only NEW.s has.

--digest hashes each kernel from its `<name>:` label through `.end_amdhsa_kernel` (code and kernel descriptor), with
comments and blank lines dropped and the function-numbered labels (.LBB<n>_, .Lfunc_end<n>) made position-independent:
two builds whose digests all match emit the same machine code for every kernel.  FILE.s is an assembly hipcc wrote with
--save-temps (fiveeq_capi-hip-amdgcn-amd-amdhsa-gfx950.s); without it the tree is compiled first.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


KERNEL = re.compile(r"^(_Z\w+):\s*; @\1\n(.*?)\.end_amdhsa_kernel", re.S | re.M)


def compile_asm():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"), "--save-temps", "-o",
               os.path.join(tmp, "lib.so"), os.path.join(ROOT, "fiveeqscm_amd", "csrc", "fiveeq_capi.hip")]
        cmd += [f"-D{d}" for d in os.environ.get("FIVEEQ_DEFS", "").split() if d]
        subprocess.run(cmd, cwd=tmp, check=True, stderr=subprocess.DEVNULL)
        return open(os.path.join(tmp, "fiveeq_capi-hip-amdgcn-amd-amdhsa-gfx950.s")).read()


def digests(asm):
    """{mangled kernel name: sha256 of its normalised assembly}"""
    out = {}
    for m in KERNEL.finditer(asm):
        lines = (line.split(";")[0].rstrip() for line in m.group(0).splitlines())
        text = "\n".join(line for line in lines if line.strip())
        text = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"\.LBB\d+_", ".LBB_", text))
        out[m.group(1)] = hashlib.sha256(text.encode()).hexdigest()
    return out


def digest(asm):
    for name, h in digests(asm).items():
        print(name, h)


def compare_digest(parent_asm, new_asm):
    old, new = digests(parent_asm), digests(new_asm)
    missing = [n for n in old if n not in new]
    changed = [n for n in old if n in new and new[n] != old[n]]
    for n in missing:
        print("MISSING", n)
    for n in changed:
        print("CHANGED", n)
    added = facts(new_asm)
    known = set(facts(parent_asm))
    fresh = sorted(n for n in added if n not in known)
    print(f"kernels of the parent build compared by digest: {len(old)}; missing: {len(missing)}; changed: {len(changed)}; "
          f"new: {len(fresh)}\n")
    for name in fresh:
        print(name)
        print("   vgpr %3d sgpr %3d lds %5d scratch %d waves/SIMD %d instr %d" % added[name])


def facts(asm):
    """{demangled kernel name without its parameter list: (vgpr, sgpr, lds, scratch, occupancy, instructions)}"""
    found = [(m.group(1), m.group(2), asm[m.end():m.end() + 4000]) for m in KERNEL.finditer(asm)]
    names = subprocess.run(["c++filt"], input="\n".join(f[0] for f in found), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for (_, body, tail), dem in zip(found, names):
        get = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, body)[1])   # noqa: E731
        after = lambda k: int(re.search(r"; %s: (\d+)" % k, tail)[1])   # noqa: E731
        code = body.split(".section")[0]
        key = dem.replace("float __vector(2)", "float2v").split("(")[0].replace("void fiveeq::", "")
        out[key] = (get("next_free_vgpr"), get("next_free_sgpr"), after("LDSByteSize"), after("ScratchSize"), after("Occupancy"),
                    len(re.findall(r"^\s+[a-z]\w+ ", code, re.M)))
    return out


def compare_forc(parent_asm, new_asm):
    old, new = facts(parent_asm), facts(new_asm)
    changed = missing = 0
    for name, f in old.items():
        key = name[:-1] + ", false>" if name.startswith(("step_kernel<", "fused_kernel<")) else name
        if key not in new:
            missing += 1
            print("MISSING", key)
        elif new[key] != f:
            changed += 1
            print("CHANGED", key, f, "->", new[key])
    print(f"pre-existing instantiations compared: {len(old)}; missing: {missing}; changed: {changed}\n")
    line = "   %-7s vgpr %3d sgpr %3d lds %5d scratch %d waves/SIMD %d instr %d"
    for name in sorted(new):
        if name.startswith(("step_kernel<", "fused_kernel<")) and name.endswith(", true>"):
            print(name)
            print(line % (("forc",) + new[name]))
            print(line % (("without",) + new[name[:-len("true>")] + "false>"]))


def compare_scen_forc(parent_asm, new_asm):
    old, new = facts(parent_asm), facts(new_asm)
    changed = missing = 0
    for name, f in old.items():
        key = name[:-1] + ", false>" if name.startswith("step_scen_kernel<") else name
        if key not in new:
            missing += 1
            print("MISSING", key)
        elif new[key] != f:
            changed += 1
            print("CHANGED", key, f, "->", new[key])
    renamed = {(n[:-1] + ", false>" if n.startswith("step_scen_kernel<") else n) for n in old}
    added = sorted(n for n in new if n not in renamed)
    print(f"pre-existing instantiations compared: {len(old)}; missing: {missing}; changed: {changed}; new: {len(added)}\n")
    line = "   %-7s vgpr %3d sgpr %3d lds %5d scratch %d waves/SIMD %d instr %d"
    worse = 0
    for name in added:
        assert name.endswith("true>"), name                    # step_scen_kernel<.., FORC>, fused_kernel<.., SCEN, FORC>
        plain = name[:-len("true>")] + "false>"
        print(name)
        print(line % (("forc",) + new[name]))
        print(line % (("without",) + new[plain]))
        if new[name][3] != 0 or new[name][4] < new[plain][4]:
            worse += 1
            print("   ^^^ scratch, or fewer waves per SIMD than the counterpart")
    print(f"\nnew instantiations with scratch or fewer waves per SIMD than their counterpart: {worse}")


def main():
    if sys.argv[1:2] == ["--compare-scen-forc"]:
        compare_scen_forc(open(sys.argv[2]).read(), open(sys.argv[3]).read() if len(sys.argv) > 3 else compile_asm())
        return
    if sys.argv[1:2] == ["--compare-digest"]:
        compare_digest(open(sys.argv[2]).read(), open(sys.argv[3]).read() if len(sys.argv) > 3 else compile_asm())
        return
    if sys.argv[1:2] == ["--digest"]:
        digest(open(sys.argv[2]).read() if len(sys.argv) > 2 else compile_asm())
        return
    if sys.argv[1:2] == ["--compare-forc"]:
        compare_forc(open(sys.argv[2]).read(), open(sys.argv[3]).read() if len(sys.argv) > 3 else compile_asm())
        return
    want = sys.argv[1:] or ["Li4ELi1ELi1E"]
    asm = compile_asm()
    for m in KERNEL.finditer(asm):
        name, body = m.group(1), m.group(2)
        if not any(w in name for w in want):
            continue
        demangled = subprocess.run(["c++filt", name], capture_output=True,
                                   text=True).stdout.strip().split("(")[0]
        code = body.split(".section")[0]
        get = lambda k: (re.search(r"\.amdhsa_%s (\d+)" % k, body) or [None, "?"])[1]   # noqa: E731
        tail = asm[m.end():m.end() + 4000]
        scratch = (re.search(r"; ScratchSize: (\d+)", tail) or [None, "?"])[1]
        occ = (re.search(r"; Occupancy: (\d+)", tail) or [None, "?"])[1]
        lds = (re.search(r"; LDSByteSize: (\d+)", tail) or [None, "?"])[1]
        cnt = lambda pat: len(re.findall(r"^\s+" + pat, code, re.M))   # noqa: E731
        print(f"{demangled}\n   vgpr {get('next_free_vgpr')} sgpr {get('next_free_sgpr')} lds {lds} scratch {scratch} "
              f"occupancy {occ}\n   VALU {cnt('v_')} (fma_f64 {cnt('v_fma_f64')} mul_f64 {cnt('v_mul_f64')} "
              f"add_f64 {cnt('v_add_f64')} fma_f32 {cnt('v_fma_f32|v_fmac_f32')} pk {cnt('v_pk_')} readlane "
              f"{cnt('v_readlane|v_writelane')}) SALU {cnt('s_')} LDS {cnt('ds_')} global {cnt('global_')} "
              f"waitcnt {cnt('s_waitcnt')}")


if __name__ == "__main__":
    main()
