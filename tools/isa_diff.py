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

For a change that moves kernels between files or renames them (several kernel
files folded into one template), the mapped form:

  python tools/isa_diff.py --map syms.map old/a.s old/b.s ... new/k.s

The last listing is the new one.  syms.map has one "OLD NEW" pair of kernel
symbols per line (# starts a comment); OLD is rewritten to NEW wherever it
occurs in the old listings -- the label, .amdhsa_kernel, the .set lines, the
metadata .name / .symbol -- before anything is compared.  Every kernel of the
new listing is compared with its one counterpart among the old listings (code,
.amdhsa_* / .set block, metadata entry), every device function and data
object of the new listing with each namesake in the old listings, and an old
kernel that no new kernel answers to is reported.  The directives outside the
functions and objects (.section, .addrsig_sym, ...) follow the files' layout
and are not compared in this form.  Same output, same exit status.
"""
import re
import sys

SKIP = re.compile(r"\s*\.(file|loc|ident)\b")
LOCAL = re.compile(r"\.L[A-Za-z_$]*\d[\d_]*")
BEGIN = re.compile(r";\s*-- Begin function (\S+)")
END = re.compile(r";\s*-- End function")
SET = re.compile(r"\s*\.set\s+(?:\.L)?([^\s,]+)\.\w+,")
OBJECT = re.compile(r"\s*\.type\s+([^\s,]+),@object")
SIZE = re.compile(r"\s*\.size\s+([^\s,]+),")


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


def split(text):
    """the raw lines of every function by symbol, of the kernels' metadata
    entries by name, and of the rest of the listing"""
    funcs, meta, rest = {}, {}, []
    cur = None
    in_meta = False
    entry = None
    for raw in text.split("\n"):
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
    return funcs, meta, rest


def kernels_of(funcs):
    return [n for n, body in funcs.items() if any(l.strip().startswith(".amdhsa_kernel ") for l in body)]


def parse(path):
    """{symbol: canonical lines} for every function, the kernel names, the
    kernels' metadata entries, and the canonical rest of the file"""
    funcs, meta, rest = split(open(path).read())
    return ({n: canon(b) for n, b in funcs.items()}, kernels_of(funcs),
            {n: [" ".join(l.split()) for l in e] for n, e in meta.items()}, canon(rest))


def parse_symbols(path, rename):
    """the mapped form's view of a listing, after rename(text): per function
    its canonical lines with its .set lines behind them, the kernel names, the
    metadata entries, and per data object its canonical lines"""
    funcs, meta, rest = split(rename(open(path).read()))
    objs, cur = {}, None
    for raw in rest:
        m = SET.match(raw)
        if m and m.group(1) in funcs:
            funcs[m.group(1)].append(raw)
            continue
        m = OBJECT.match(raw)
        if m and not m.group(1).startswith("__hip_cuid"):
            cur = objs.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(raw)
        m = SIZE.match(raw)
        if m and m.group(1) in objs:
            cur = None
    return ({n: canon(b) for n, b in funcs.items()}, kernels_of(funcs),
            {n: [" ".join(l.split()) for l in e] for n, e in meta.items()}, {n: canon(b) for n, b in objs.items()})


def differs(kind, n, a, b, ma, mb):
    """what differs between two bodies (and metadata entries) of symbol n, or None"""
    if a != b:
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        what = ".amdhsa_* / .set block" if i < len(a) and re.match(r"\.(amdhsa_|set )", a[i]) else "code"
        return f"{kind} {n}: {what} differs at line {i} of {len(a)} / {len(b)}"
    if ma != mb:
        return f"{kind} {n}: metadata entry differs"
    return None


def diff_two(old, new):
    fa, ka, ma, ra = parse(old)
    fb, kb, mb, rb = parse(new)
    bad = []
    for n in sorted(set(fa) | set(fb)):
        kind = "kernel" if n in ka or n in kb else "function"
        if n not in fa or n not in fb:
            bad.append(f"{kind} {n}: only in {new if n in fb else old}")
        else:
            bad.append(differs(kind, n, fa[n], fb[n], ma.get(n), mb.get(n)))
    if ra != rb:
        bad.append("outside the functions: data objects or directives differ")
    return [b for b in bad if b], len(ka)


def diff_mapped(map_path, olds, new):
    pairs = [ln.split("#")[0].split() for ln in open(map_path)]
    mp = {p[0]: p[1] for p in pairs if len(p) == 2}
    if len(mp) != sum(1 for p in pairs if p) or len(set(mp.values())) != len(mp):
        sys.exit(f"{map_path}: every line is one 'OLD NEW' pair, no symbol twice")
    # the longest symbol first, and only as a whole symbol (a .kd or .num_vgpr suffix may follow)
    pat = re.compile(r"(?<![\w$])(" + "|".join(map(re.escape, sorted(mp, key=len, reverse=True))) + r")(?![\w$])")
    rename = (lambda text: pat.sub(lambda m: mp[m.group(1)], text)) if mp else (lambda text: text)
    parsed = [(o,) + parse_symbols(o, rename) for o in olds]
    fb, kb, mb, ob = parse_symbols(new, lambda text: text)
    bad = []
    for n in sorted(fb):
        kind = "kernel" if n in kb else "function"
        have = [(o, fa[n], ma.get(n)) for o, fa, ka, ma, oa in parsed if n in fa]
        if not have:
            bad.append(f"{kind} {n}: only in {new}" + (" (no old kernel is mapped to it)" if n in kb else ""))
        elif n in kb and len(have) > 1:
            bad.append(f"kernel {n}: {len(have)} counterparts: " + ", ".join(o for o, _, _ in have))
        for o, body, m in have:
            bad.append(differs(kind, n, body, fb[n], m, mb.get(n)))
    for o, fa, ka, ma, oa in parsed:
        bad += [f"kernel {n}: only in {o} (unmapped, or mapped to no kernel of {new})"
                for n in sorted(ka) if n not in kb]
        bad += [f"data object {n}: differs from {o}" for n in sorted(ob) if n in oa and oa[n] != ob[n]]
    bad += [f"data object {n}: only in {new}" for n in sorted(ob) if not any(n in oa for *_, oa in parsed)]
    return [b for b in bad if b], len(kb)


def main():
    argv = sys.argv[1:]
    if len(argv) == 2 and argv[0] != "--map":
        bad, count = diff_two(*argv)
    elif len(argv) >= 4 and argv[0] == "--map":
        bad, count = diff_mapped(argv[1], argv[2:-1], argv[-1])
    else:
        sys.exit(__doc__)
    if bad:
        print("\n".join(bad))
        sys.exit(1)
    print(f"identical: {count} kernels")


if __name__ == "__main__":
    main()
