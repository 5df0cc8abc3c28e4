#!/usr/bin/env python3
"""Compare two builds' gfx950 assembly listings kernel by kernel: one line per kernel symbol, `equal` or `different`, with the SHA-256 of
each side's text -- everything the listing holds for the kernel: its instructions, its resource symbols, its kernel descriptor
(.amdhsa_kernel block), the compiler's remarks behind it and its entry in the amdhsa.kernels metadata -- after the compiler's local labels
(.LBB<f>_<n>, .Ltmp<n>, .Lfunc_end<n>, ...) have been renumbered in order of first appearance, so that "only the numbers in local labels
differ" compares equal.  A generic text compare: it knows nothing of what the kernels do.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize --cuda-device-only -S -o DIR/bez_step_ws8.s bez_isaacgym_amd/csrc/bez_step_ws8.hip
  python tools/isa_compare.py PARENT_DIR NEW_DIR            (every *.s of PARENT_DIR against the file of the same name in NEW_DIR)

Exit status 1 when a kernel differs or exists on one side only."""
import hashlib
import os
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9_]+|\bBB[0-9]+_[0-9]+")   # (the second form: block names in the compiler's remarks)


def kernels(path):
    """{symbol: text}"""
    lines = open(path).read().split("\n")
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    # the listing's body: a kernel's text runs from its first `.section .text.SYM` line to the next function's (its code, its descriptor
    # in .rodata, its resource symbols, the compiler's remarks); the last one's ends where the module's own trailer starts
    starts, seen = [], set()
    for i, l in enumerate(lines):
        m = re.match(r"\s*\.section\s+\.text\.([^,\s]+),", l)
        if m and m.group(1) not in seen:
            seen.add(m.group(1))
            starts.append((i, m.group(1)))
    end = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdgpu_metadata", l))
    trailer = next(i for i, l in enumerate(lines) if i > starts[-1][0] and re.match(r"\s*\.section\s+\.AMDGPU\.gpr_maximums", l))
    parts = {}
    for (a, n), (b, _) in zip(starts, starts[1:] + [(trailer, None)]):
        if n in names:
            parts[n] = lines[a:b]
    # the metadata: the items of the amdhsa.kernels list
    items = [i for i, l in enumerate(lines) if i > end and l.startswith("  - .")]
    stop = next(i for i, l in enumerate(lines) if i > end and l.startswith("amdhsa.target"))
    for a, b in zip(items, items[1:] + [stop]):
        n = next(m.group(1) for l in lines[a:b] for m in [re.match(r"    \.name:\s+(\S+)", l)] if m)
        parts[n] += lines[a:b]
    out = {}
    for n, ls in parts.items():
        seen = {}
        text = "\n".join(re.sub(r"\s+;", " ;", l.rstrip()) for l in ls)   # (remarks are aligned to a column that moves with a label's length)
        out[n] = LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), text)
    return out


def main(parent, new):
    bad = 0
    for f in sorted(x for x in os.listdir(parent) if x.endswith(".s")):
        a, b = kernels(os.path.join(parent, f)), kernels(os.path.join(new, f))
        for n in sorted(set(a) | set(b)):
            ha, hb = (hashlib.sha256(d[n].encode()).hexdigest()[:16] if n in d else "missing" for d in (a, b))
            bad += ha != hb
            print("%-17s %-9s %s %s %s" % (f[:-2], "equal" if ha == hb else "different", ha, hb, n))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
