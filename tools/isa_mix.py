#!/usr/bin/env python3
"""Instruction mix of one kernel, read from the compiler's assembly (no GPU needed):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -fno-slp-vectorize -S seld_amd/csrc/conv_pool_sb.hip -o cpsb.s
    python3 tools/isa_mix.py cpsb.s 'conv_first_fwd_pool_sbpp_kernel<7, true, false>'

The kernel is named by its mangled symbol, its demangled name or a part of either that fits one symbol only.  The body is cut at every s_barrier
(static order, labels ignored), so a kernel whose loop alternates segments across workgroup barriers shows each segment as one row; the last row is
the whole body.  Classes: mfma, v_pk_*_f32 (packed fp32 VALU), transcendental (exp log rcp rsq sqrt sin cos), other VALU, ds_*, global_load_*,
global_store_*, scratch_* (spills), s_waitcnt, other scalar."""
import re
import shutil
import subprocess
import sys

CLASSES = ("mfma", "pk_f32", "trans", "valu", "ds", "gload", "gstore", "scratch", "waitcnt", "salu")
TRANS = re.compile(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_")


def classify(op):
    if op.startswith(("v_mfma", "v_smfma")):
        return "mfma"
    if op.startswith("v_pk_") and op.endswith("_f32"):
        return "pk_f32"
    if TRANS.match(op):
        return "trans"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_load", "buffer_load", "flat_load")):
        return "gload"
    if op.startswith(("global_store", "buffer_store", "flat_store", "global_atomic")):
        return "gstore"
    if op.startswith("scratch_"):
        return "scratch"
    if op == "s_waitcnt":
        return "waitcnt"
    return "salu" if op.startswith("s_") else None


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return out if len(out) == len(names) else list(names)


def bodies(path):
    """symbol -> instruction mnemonics of its body, in file order"""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and not m.group(1).startswith((".L", "BB")):
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end") or line.lstrip().startswith("s_endpgm"):
                cur = None
                continue
            m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", line)
            if m:
                cur.append(m.group(1))
    return {k: v for k, v in out.items() if v}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    path, want = sys.argv[1], sys.argv[2].replace(" ", "")
    syms = bodies(path)
    names = list(syms)
    hits = [n for n, d in zip(names, demangle(names)) if want == n or want in n or want in d.replace(" ", "")]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} symbols match {sys.argv[2]!r}: " + " ".join(hits[:8]))
    segs, cur = [], dict.fromkeys(CLASSES, 0)
    for op in syms[hits[0]]:
        if op == "s_barrier":
            segs.append(cur)
            cur = dict.fromkeys(CLASSES, 0)
            continue
        c = classify(op)
        if c:
            cur[c] += 1
    segs.append(cur)
    print("segment " + " ".join(f"{c:>8}" for c in CLASSES))
    for i, s in enumerate(segs):
        print(f"{i:>7} " + " ".join(f"{s[c]:>8}" for c in CLASSES))
    print("    all " + " ".join(f"{sum(s[c] for s in segs):>8}" for c in CLASSES))


if __name__ == "__main__":
    main()
