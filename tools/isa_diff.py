#!/usr/bin/env python3
"""Are two gfx950 device listings the same code?  For a change that must not
touch the kernels (a header split, a host-side refactor):

  hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -o old/k.s hhmm_m_tayal.hip   (at the parent)
  hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S -o new/k.s hhmm_m_tayal.hip   (with the change)
  python tools/isa_diff.py old/k.s new/k.s

Per kernel symbol it compares the instruction sequence, the .amdhsa_* block
with the kernel's .set lines (registers, LDS, private segment), and the
kernel's entry in the amdhsa.kernels metadata; device functions a kernel
calls (the noinline accurate phases of hhmm_crmath.h) and the data objects
outside the functions are compared too.  Ignored: comments, .file / .loc /
.ident, the per-file __hip_cuid_* symbol, and the numbering of local labels
(.LBB<f>_<n>, .Lfunc_end<f>, ...: renumbered per function in order of first
use, so a function that moved inside the file still compares equal).

Prints "identical: N kernels" (exit 0) or the differing symbols (exit 1).
"""
import re
import sys

SKIP = re.compile(r"\s*\.(file|loc|ident)\b")
LOCAL = re.compile(r"\.L[A-Za-z_$]*\d[\d_]*")
BEGIN = re.compile(r";\s*-- Begin function (\S+)")
END = re.compile(r";\s*-- End function")


def strip_comment(line):
    """the line without its `;` comment (a `;` inside a string stays)"""
    quoted = False
    for i, ch in enumerate(line):
        if ch == '"' and (i == 0 or line[i - 1] != "\\"):
            quoted = not quoted
        elif ch == ";" and not quoted:
            return line[:i].rstrip()
    return line.rstrip()


def canon(lines):
    """comment-free lines with local labels renumbered in order of first use"""
    names = {}
    out = []
    for raw in lines:
        if SKIP.match(raw):
            continue
        ln = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", strip_comment(raw))
        if not ln.strip():
            continue
        ln = LOCAL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), ln)
        out.append(" ".join(ln.split()))
    return out


def parse(path):
    """{symbol: canonical lines} for every function, the kernel names, the
    kernels' metadata entries, and the canonical rest of the file"""
    funcs, meta, rest = {}, {}, []
    cur = None
    in_meta = False
    entry = None
    for raw in open(path).read().split("\n"):
        if raw.strip() == ".amdgpu_metadata":
            in_meta = True
            continue
        if raw.strip() == ".end_amdgpu_metadata":
            in_meta = False
            entry = None
            continue
        if in_meta:
            if raw.startswith("  - "):  # one kernel's entry of amdhsa.kernels
                entry = []
            elif not raw.startswith("    "):
                entry = None
                rest.append(raw)
            if entry is not None:
                entry.append(raw)
                m = re.match(r"\s+\.name:\s+(\S+)", raw)
                if m:
                    meta[m.group(1)] = entry
            continue
        m = BEGIN.search(raw)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        (rest if cur is None else cur).append(raw)
        if END.search(raw):
            cur = None
    kernels = [n for n, body in funcs.items() if any(l.strip().startswith(".amdhsa_kernel ") for l in body)]
    return ({n: canon(b) for n, b in funcs.items()}, kernels, {n: [" ".join(l.split()) for l in e]
                                                               for n, e in meta.items()}, canon(rest))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    fa, ka, ma, ra = parse(sys.argv[1])
    fb, kb, mb, rb = parse(sys.argv[2])
    bad = []
    for n in sorted(set(fa) | set(fb)):
        kind = "kernel" if n in ka or n in kb else "function"
        if n not in fa or n not in fb:
            bad.append(f"{kind} {n}: only in {sys.argv[2] if n in fb else sys.argv[1]}")
        elif fa[n] != fb[n]:
            i = next((i for i, (x, y) in enumerate(zip(fa[n], fb[n])) if x != y), min(len(fa[n]), len(fb[n])))
            what = ".amdhsa_* / .set block" if i < len(fa[n]) and re.match(r"\.(amdhsa_|set )", fa[n][i]) else "code"
            bad.append(f"{kind} {n}: {what} differs at line {i} of {len(fa[n])} / {len(fb[n])}")
        elif ma.get(n) != mb.get(n):
            bad.append(f"{kind} {n}: metadata entry differs")
    if ra != rb:
        bad.append("outside the functions: data objects or directives differ")
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print(f"identical: {len(ka)} kernels")


if __name__ == "__main__":
    main()
