"""Is a source change invisible to the device?  Compile a .hip file of csrc/ at a parent revision and in the working tree to
gfx950 assembly (build.py's flags, device only) and compare every kernel symbol's instruction text, comments stripped and the
function index taken out of the local labels.  Per kernel: identical yes / no, VGPRs, scratch, LDS and kernarg bytes on both
sides.  Exit status 1 if a kernel that both sides have differs.  No GPU needed.

    python tools/asm_diff.py conv.hip --parent HEAD --out profiles/NAME.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "t-deed_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-S", "--cuda-device-only"]


def assembly(path):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "a.s")
        subprocess.run([HIPCC, *FLAGS, "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "hip", path, "-o", out], check=True,
                       stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()


def kernels(asm):
    """{kernel as written, e.g. "c1_gconv_mfma_kernel<2, 1>": dict(text, vgpr, scratch, lds, kernarg)}.  text: the instructions
    up to the kernel descriptor, comments stripped, the function index taken out of the local labels, and scalar loads of the
    hidden arguments written relative to their start (they sit behind the explicit arguments, so they move with the list)"""
    body = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\s*\.section\s+\.rodata", asm, re.M | re.S):
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()) for ln in m.group(2).splitlines()]
        body[m.group(1)] = [ln for ln in lines if ln]
    out = {}
    for entry in asm[asm.index("amdhsa.kernels:"):].split("\n  - .agpr_count:")[1:]:
        def field(name):
            return re.search(r"\.%s:\s+(\S+)" % name, entry).group(1)
        hid = re.search(r"\.offset:\s+(\d+)\n\s+\.size:\s+\d+\n\s+\.value_kind:\s+hidden_", entry)
        hid = int(hid.group(1)) if hid else 1 << 30

        def rel(m):
            off = int(m.group(2), 16)
            return m.group(1) + (hex(off) if off < hid else "hidden+" + hex(off - hid))
        sym = field("name")
        name = subprocess.run(["c++filt", sym], check=True, capture_output=True, text=True).stdout.strip()
        name = re.sub(r"^void ", "", name.replace("(anonymous namespace)::", ""))
        out[name[:name.index("(")] if "(" in name else sym] = dict(      # (the symbol, where c++filt gives up)
            text="\n".join(re.sub(r"^(s_load_dword\w* \S+ s\[0:1\], )(0x[0-9a-f]+)$", rel, ln) for ln in body[sym]),
            vgpr=int(field("vgpr_count")), scratch=int(field("private_segment_fixed_size")),
            lds=int(field("group_segment_fixed_size")), kernarg=int(field("kernarg_segment_size")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="a file of t-deed_amd/csrc")
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--out")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPL"), help="applied to the parent's kernel names (a dropped template argument)")
    a = ap.parse_args()
    rel = os.path.relpath(os.path.join(CSRC, a.source), ROOT)
    with tempfile.TemporaryDirectory() as d:
        old = os.path.join(d, a.source)
        with open(old, "w") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{a.parent}:{rel}"], check=True, capture_output=True, text=True).stdout)
        parent, new = kernels(assembly(old)), kernels(assembly(os.path.join(CSRC, a.source)))
    if a.rename:
        parent = {re.sub(a.rename[0], a.rename[1], k): v for k, v in parent.items()}
    keys = ("vgpr", "scratch", "lds", "kernarg")
    table = {}
    for sym in sorted(set(parent) | set(new)):
        p, n = parent.get(sym), new.get(sym)
        table[sym] = {"identical": bool(p and n and p["text"] == n["text"]),
                      "parent": {k: p[k] for k in keys} if p else None, "new": {k: n[k] for k in keys} if n else None}
    differ = [s for s, r in table.items() if not r["identical"]]
    print(f"{len(table)} kernels, {len(table) - len(differ)} identical")
    for s in differ:
        print("  differs:" if table[s]["parent"] and table[s]["new"] else "  one side only:", s, table[s]["parent"], table[s]["new"])
    if a.out:
        with open(a.out, "w") as f:
            rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], check=True, capture_output=True, text=True)
            json.dump({"source": rel, "parent": rev.stdout.strip(), "flags": FLAGS, "kernels": table}, f, indent=1)
            f.write("\n")
    return 1 if any(table[s]["parent"] and table[s]["new"] for s in differ) else 0


if __name__ == "__main__":
    sys.exit(main())
