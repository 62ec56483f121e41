#!/usr/bin/env python3
"""Is the device code of two trees the same, kernel by kernel?  (no GPU needed)
usage: scripts/kernels_same.py <other tree's drake_amd/csrc> [this tree's csrc]

Compiles mpm_engine.hip of both with the flags of drake_amd/_build.py plus --cuda-device-only -S, splits the output at the
kernel symbols and compares, per kernel, the instruction text (labels renumbered in order of appearance; comment, .loc,
.file and .cfi lines dropped) and the .amdhsa_* block.  Exit status 1 if a kernel differs or the sets of symbols do.
A host-only refactor must come out with every kernel identical."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from drake_amd import _build  # noqa: E402


def assembly(csrc):
    with tempfile.NamedTemporaryFile(suffix=".s") as f:
        flags = [x for x in _build.FLAGS if x != "-shared"]
        subprocess.run(["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", f.name,
                        os.path.join(csrc, "mpm_engine.hip")], check=True, stderr=subprocess.DEVNULL)
        return open(f.name).read().split("\n")


def kernels(lines):
    """symbol -> (normalised instruction lines, .amdhsa_* lines)"""
    funcs, hsa, cur, inh = {}, {}, None, None
    for ln in lines:
        s = ln.strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            inh = m.group(1)
            hsa[inh] = []
        elif s == ".end_amdhsa_kernel":
            inh = None
        elif inh:
            hsa[inh].append(s)
        elif re.match(r"^\w+:\s*(;.*)?$", ln):
            cur = funcs.setdefault(ln.split(":")[0], [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and s and not re.match(r"^(;|\.loc\b|\.file\b|\.cfi)", s):
            cur.append(re.sub(r"\s*;.*$", "", s))
    out = {}
    for k in hsa:
        labels = {}
        out[k] = ([re.sub(r"\.L[\w$]+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), s)
                   for s in funcs.get(k, [])], hsa[k])
    return out


if __name__ == "__main__":
    a = kernels(assembly(sys.argv[1]))
    b = kernels(assembly(sys.argv[2] if len(sys.argv) > 2 else _build.CSRC))
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    for k in bad:
        print("ONLY IN ONE TREE:" if k not in a or k not in b else "DIFFERS:", k)
    print(f"{len(a)} / {len(b)} kernels, {sum(len(v[0]) for v in a.values())} instruction lines compared, {len(bad)} kernels differ")
    sys.exit(1 if bad else 0)
