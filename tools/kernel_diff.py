#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of the engine, kernel by kernel, without a GPU.

    python3 tools/kernel_diff.py BASE NEW [--all]

BASE / NEW: libryd_engine.so (or any file with a .hip_fatbin section), an offload bundle, or
a device code object.  For every kernel: whether the disassembly is identical once addresses
and encodings are stripped; vgpr_count, sgpr_count, scratch and LDS bytes from the code
object's notes; and the mnemonic histograms of three instruction classes (FP64 vector ALU,
LDS, vector memory).  Kernels with identical disassembly are only counted unless --all.
Exit status 1 when the kernel sets differ or a kernel's resources or histograms differ
(a renumbered register or a reordered scalar instruction alone does not fail it).
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
RES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
CLASSES = {"fp64": lambda m: m.startswith("v_") and "_f64" in m,
           "lds": lambda m: m.startswith("ds_"),
           "vmem": lambda m: m.split("_")[0] in ("global", "flat", "buffer", "scratch")}


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, tmp, tag):
    """path -> its gfx950 ELFs: out of the host library's fat binary (one bundle per translation
    unit that holds kernels), out of a bundle, or the file as given."""
    with open(path, "rb") as f:
        magic = f.read(24)
    if magic.startswith(b"\x7fELF") and magic[18:20] != b"\xe0\x00":      # host ELF (not EM_AMDGPU)
        fat = os.path.join(tmp, tag + ".fatbin")
        # (with an output file of its own: without one llvm-objcopy rewrites its input in place)
        tool("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path, os.path.join(tmp, tag + ".copy"))
        path, magic = fat, BUNDLE
    if not magic.startswith(BUNDLE):
        return [path]
    with open(path, "rb") as f:
        data = f.read()
    out, at = [], data.find(BUNDLE)
    while at >= 0:                                                         # the section is the bundles in a row
        nxt = data.find(BUNDLE, at + 1)
        one = os.path.join(tmp, f"{tag}{len(out)}.bundle")
        with open(one, "wb") as f:
            f.write(data[at:nxt if nxt >= 0 else len(data)])
        target = next(t for t in tool("clang-offload-bundler", "--list", "--type=o", "--input=" + one).split()
                      if t.endswith("gfx950"))
        out.append(os.path.join(tmp, f"{tag}{len(out)}.co"))
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=" + target, "--input=" + one,
             "--output=" + out[-1])
        at = nxt
    return out


def merged(dicts):
    out = {}
    for d in dicts:
        out.update(d)
    return out


def kernels(co):
    """{kernel name: {resource: value}} from the AMDGPU metadata note."""
    out, cur = {}, {}
    for line in tool("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"(  - | {4})(\.\w+):\s*(\S+)", line)               # a kernel entry's own keys
        if not m:
            continue
        if m.group(1) == "  - ":                                           # first key of the next entry
            cur = {}
        if m.group(2) in RES:
            cur[m.group(2)] = int(m.group(3))
        if m.group(2) == ".symbol":
            out[m.group(3)[:-len(".kd")]] = cur
    return out


def functions(co):
    """{symbol: [instruction text]} with addresses, encodings and comments stripped."""
    out, cur = {}, None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()
            # a scalar instruction's trailing 32-bit literal may be a distance in the file (the halves
            # of a pc-relative address), which moves with every other kernel's size
            cur.append(re.sub(r"^(s_.* )0x[0-9a-f]{5,8}$", r"\1<lit32>", ins))
    return out


def histogram(insns):
    h = {c: collections.Counter() for c in CLASSES}
    for ins in insns:
        mnem = re.sub(r"_e(32|64)$", "", ins.split(" ")[0])               # the encoding is not the operation
        for c, pred in CLASSES.items():
            if pred(mnem):
                h[c][mnem] += 1
    return h


def short(sym):
    m = re.match(r"_ZN12_GLOBAL__N_1\d+(\w+?)(E?Ev\w*|ENS_\w*)$", sym)
    return m.group(1) if m else sym


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--all", action="store_true", help="list the kernels with identical disassembly too")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        cos = [code_objects(p, tmp, t) for p, t in ((a.base, "base"), (a.new, "new"))]
        kb, kn = [merged(kernels(c) for c in cs) for cs in cos]
        fb, fn = [merged(functions(c) for c in cs) for cs in cos]
    bad = False
    for only, where in ((set(kb) - set(kn), "base"), (set(kn) - set(kb), "new")):
        for s in sorted(only):
            print(f"kernel only in {where}: {s}")
            bad = True
    same = 0
    print(f"{'kernel':60s} {'asm':9s} {'vgpr':>9s} {'sgpr':>9s} {'scratch':>9s} {'lds':>11s}  fp64/lds/vmem")
    for s in sorted(set(kb) & set(kn)):
        ident = fb.get(s) == fn.get(s)
        same += ident
        if ident and not a.all:
            continue
        hb, hn = histogram(fb.get(s, [])), histogram(fn.get(s, []))
        res = [f"{kb[s].get(r)}" if kb[s].get(r) == kn[s].get(r) else f"{kb[s].get(r)}>{kn[s].get(r)}" for r in RES]
        hist = "/".join(str(sum(hb[c].values())) if hb[c] == hn[c] else "DIFF" for c in CLASSES)
        print(f"{short(s):60s} {'identical' if ident else 'differs':9s} {res[0]:>9s} {res[1]:>9s} {res[2]:>9s} "
              f"{res[3]:>11s}  {hist}")
        for c in CLASSES:
            for mnem in sorted(set(hb[c]) | set(hn[c])):
                if hb[c][mnem] != hn[c][mnem]:
                    print(f"    {c}: {mnem} {hb[c][mnem]} > {hn[c][mnem]}")
        # sgpr_count may move with scalar scheduling; the other resources and the histograms may not
        if any(">" in r for r in (res[0], res[2], res[3])) or "DIFF" in hist:
            bad = True
    others = sorted(s for s in set(fb) | set(fn) if s not in kb and s not in kn and fb.get(s) != fn.get(s))
    for s in others:
        print(f"device function differs: {s}")
    print(f"{len(set(kb) & set(kn))} kernels in both builds, {same} with identical disassembly; "
          f"{len(others)} other device functions differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
