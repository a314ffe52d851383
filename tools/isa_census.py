"""Per-kernel census of the instruction kinds that three round-6 fixes were about, from the compiled ISA: ds_bpermute
(cross-lane moves through the LDS crossbar: a `__shfl_xor` tree is a chain of them), integer divisions (v_rcp_iflag: one per
32-bit division, a 64-bit one is ~120 instructions around it), float divisions (v_div_scale pairs), dword-sized global loads
(per-element loads of constants) -- for kernels whose workgroups live a few microseconds each of these is on the critical path.
    python tools/isa_census.py [file.hip ...]
Per-`s_barrier` segment (a kernel whose phases are barrier-separated and whose waves all run the same stream: a wave's own
instruction stream is a lower bound on each phase), with the opcode histogram of every segment:
    python tools/isa_census.py --segments KERNEL_SUBSTRING [--top N] file.hip"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "t-deed_amd", "csrc")
PAT = dict(bpermute=r"\bds_bpermute_b32", idiv=r"\bv_rcp_iflag_f32", fdiv=r"\bv_div_scale_f32", ld_dword=r"\bglobal_load_dword\b",
           ld_x4=r"\bglobal_load_dwordx4", mfma=r"\bv_mfma", waitcnt0=r"s_waitcnt vmcnt\(0\)", barrier=r"\bs_barrier")


def compile_isa(f):
    """the device assembly of one source file (release flags)"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S",
                        "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-o", out, f], check=True, capture_output=True)
        return open(out).read()


def kernels(txt):
    """(demangled name, body) of every kernel in an assembly listing"""
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", txt, re.S | re.M):
        name = subprocess.run(["c++filt", "-p", m.group(1)], capture_output=True, text=True).stdout.strip()
        yield re.sub(r"\(anonymous namespace\)::", "", name), m.group(2)


def segments(body):
    """One dict per `s_barrier`-separated stretch of a kernel body, in text order: valu (v_* other than MFMAs), mfma, lds (ds_*),
    vmem (global_* / buffer_*), salu, and `ops`, the opcode histogram.  A static count: a loop body counts once."""
    segs, cur = [], collections.Counter()
    for ln in body.splitlines():
        m = re.match(r"\s+([a-z][a-z0-9_]+)\b", ln)
        if not m:
            continue
        op = m.group(1)
        if op == "s_barrier":
            segs.append(cur)
            cur = collections.Counter()
        else:
            cur[op] += 1
    segs.append(cur)
    out = []
    for c in segs:
        kind = lambda pre, c=c: sum(n for o, n in c.items() if o.startswith(pre))      # noqa: E731
        mfma = kind("v_mfma")
        out.append(dict(valu=kind("v_") - mfma, mfma=mfma, lds=kind("ds_"), vmem=kind("global_") + kind("buffer_"),
                        salu=kind("s_"), ops=c))
    return out


def main():
    args = sys.argv[1:]
    if args and args[0] == "--segments":
        want, args = args[1], args[2:]
        top = 12
        if args and args[0] == "--top":
            top, args = int(args[1]), args[2:]
        for f in args:
            for name, body in kernels(compile_isa(f)):
                if want not in name:
                    continue
                segs = segments(body)
                print(name)
                for i, s in enumerate(segs):
                    hist = ", ".join(f"{o} {n}" for o, n in s["ops"].most_common(top) if o.startswith("v_") and not o.startswith("v_mfma"))
                    print(f"  seg {i:2d}: VALU {s['valu']:5d}  MFMA {s['mfma']:4d}  LDS {s['lds']:4d}  VMEM {s['vmem']:4d}  SALU {s['salu']:5d}   {hist}")
                print(f"  whole : VALU {sum(s['valu'] for s in segs):5d}  MFMA {sum(s['mfma'] for s in segs):4d}  LDS {sum(s['lds'] for s in segs):4d}")
        return
    files = args or [os.path.join(CSRC, f) for f in ("conv.hip", "gsf.hip", "front.hip", "gemm.hip", "bneck.hip", "sgp_gemm.hip",
                                                     "sgp_fused.hip", "misc.hip")]
    print(f"{'kernel':70s} {'lines':>6} " + " ".join(f"{k:>8}" for k in PAT))
    for f in files:
        for name, body in kernels(compile_isa(f)):
            cnt = {k: len(re.findall(p, body)) for k, p in PAT.items()}
            print(f"{name[:70]:70s} {body.count(chr(10)):6d} " + " ".join(f"{cnt[k]:8d}" for k in PAT))


if __name__ == "__main__":
    main()
