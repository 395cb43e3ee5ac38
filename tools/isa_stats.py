#!/usr/bin/env python3
"""Static instruction mix of gfx950 kernels in a hipcc `-S` assembly file.

  hipcc -O3 ... --cuda-device-only -S -o k.s hhmm_io_mix_lo.hip
  python tools/isa_stats.py k.s 'iohmm_mix_kernelILi4ELi4ELb1'

Prints, per matching kernel: total instructions, VALU / SALU / VMEM / LDS
counts, v_readlane / v_writelane (SGPR spills live in VGPR lanes), f64 ops,
s_nop, and the register metadata (vgpr, sgpr spill count).

  python tools/isa_stats.py k.s --loops _ZN4hhmm10vfb_kernelILi2ELi4EEEvNS_7DevArgsE

takes one kernel symbol and prints its resources (VGPRs, AGPRs, scratch, SGPR
spills) and one row per loop: instruction total, SALU without waits, nops and
branches, s_mul_*, 64-bit VALU adds (v_lshl_add_u64, v_add_co / v_addc pairs
counted once), VMEM and LDS.  Loops are the ones hipcc marks in the listing
("Loop Header" / "in Loop: Header=..." on every block).  A loop whose body
chooses between long alternatives -- the backward sweep of the phased kernel
runs either the whole-wave block or the predicated one -- is also split into
its arms: the stretches between the uniform branches (s_branch, s_cbranch_scc*,
s_cbranch_vcc*) that jump forward over at least --arm (default 400)
instructions; arms shorter than that are not listed.  The blocks hipcc moves
to the end of a loop (the lanes-diverged slow paths, each ending in a branch
back) come out as the loop's last arm.
"""
import argparse
import collections
import re


def classify(op):
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        return op.split("_b")[0]
    if op.startswith("v_") and "f64" in op:
        return "valu_f64"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_load") or op.startswith("s_buffer"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_") or op.startswith("scratch_"):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return "other"


def kernels(text):
    """(symbol, body) of every function of the listing."""
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\.Lfunc_end", text, re.S):
        yield m.group(1), m.group(2)


def whole_kernels(text, pat):
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?.*?\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?.*?\.vgpr_count:\s+(\d+)",
                         text):
        meta[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    for name, body in kernels(text):
        if not pat.search(name) or name.startswith("_ZL"):
            continue
        c = collections.Counter()
        for ln in body.split("\n"):
            ln = ln.strip()
            if not ln or ln[0] in ";." or ln.endswith(":"):
                continue
            c[classify(ln.split()[0])] += 1
        sp, vg = meta.get(name, (None, None))
        print(f"{name}: total={sum(c.values())} vgpr={vg} sgpr_spill={sp}")
        print("   ", dict(sorted(c.items(), key=lambda kv: -kv[1])))


# ---- per-loop breakdown ----

COLS = ("instr", "salu", "s_mul", "add64", "vmem", "lds")
UNIFORM_BRANCH = ("s_branch", "s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz")


def tally(ops):
    """The table's columns for a list of opcodes."""
    c = dict.fromkeys(COLS, 0)
    for op in ops:
        c["instr"] += 1
        kind = classify(op)
        if kind == "salu" and not op.startswith(("s_branch", "s_cbranch", "s_barrier", "s_endpgm")):
            c["salu"] += 1
        if op.startswith("s_mul_"):
            c["s_mul"] += 1
        # one 64-bit VALU add: the fused form, or the carry-out half of an add / addc pair
        if op.startswith(("v_lshl_add_u64", "v_add_co_u32", "v_sub_co_u32")):
            c["add64"] += 1
        if kind == "vmem":
            c["vmem"] += 1
        if kind == "lds":
            c["lds"] += 1
    return c


def parse_body(body):
    """[(opcode, operand text, loop header or None)] in listing order and {label: index of its first instruction}."""
    ins, labels = [], {}
    loop = None
    for ln in body.split("\n"):
        s = ln.strip()
        if not s:
            continue
        is_label = re.match(r"(\.LBB\d+_\d+):", s)
        is_block = s.startswith("; %bb.")
        if is_label or is_block:
            if is_label:
                labels[is_label.group(1)] = len(ins)
            m = re.search(r"in Loop: Header=(BB\d+_\d+)", s)
            if m:
                loop = m.group(1)
            elif "Loop Header" in s and is_label:
                loop = is_label.group(1)[2:]
            else:
                loop = None
            continue
        if s[0] in ";." or s.endswith(":"):
            continue
        parts = s.split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else "", loop))
    return ins, labels


def resources(text, sym):
    """The kernel's resource lines of the listing's trailer and metadata."""
    out = {}
    m = re.search(r"\n" + re.escape(sym) + r":.*?\.Lfunc_end\d+:.*?; Kernel info:\n((?:;.*\n)+)", text, re.S)
    trailer = m.group(1) if m else ""
    for key, rx in (("num_vgpr", r"; NumVgprs: (\d+)"), ("num_agpr", r"; NumAgprs: (\d+)"),
                    ("scratch", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"),
                    ("num_sgpr", r"; TotalNumSgprs: (\d+)")):
        mm = re.search(rx, trailer)
        out[key] = int(mm.group(1)) if mm else None
    mm = re.search(r"\.name:\s+" + re.escape(sym) + r"\n(?:.*\n)*?.*?\.sgpr_spill_count:\s+(\d+)", text)
    out["sgpr_spill"] = int(mm.group(1)) if mm else None
    return out


def loop_table(text, sym, arm_min):
    body = dict(kernels(text)).get(sym)
    if body is None:
        raise SystemExit(f"no kernel {sym} in the listing")
    res = resources(text, sym)
    print(sym)
    print("resources: " + " ".join(f"{k}={v}" for k, v in res.items()))
    ins, labels = parse_body(body)
    order, members = [], collections.defaultdict(list)
    for i, (_, _, loop) in enumerate(ins):
        if loop is None:
            continue
        if loop not in members:
            order.append(loop)
        members[loop].append(i)
    head = f"{'loop':<34}" + "".join(f"{c:>8}" for c in COLS)
    print(head)

    def row(name, idx):
        c = tally(ins[i][0] for i in idx)
        print(f"{name:<34}" + "".join(f"{c[k]:>8}" for k in COLS))

    row("whole kernel", range(len(ins)))
    for loop in order:
        idx = members[loop]
        row(f".L{loop}", idx)
        # arms: cut where a uniform branch jumps far, at the branch and at its target
        inside = set(idx)
        cuts = set()
        for i in idx:
            op, arg, _ = ins[i]
            tgt = labels.get(arg.strip())
            if op in UNIFORM_BRANCH and tgt is not None and tgt > i:  # forward: the way back from a cold block is no arm
                span = sum(1 for j in range(i, tgt) if j in inside)
                if span >= arm_min:
                    cuts.add(i + 1)
                    cuts.add(tgt)
        if not cuts:
            continue
        arm, n = [], 0
        for i in idx:
            if i in cuts and arm:
                if len(arm) >= arm_min:
                    n += 1
                    row(f"  arm {n} (instr {arm[0]}..{arm[-1]})", arm)
                arm = []
            arm.append(i)
        if len(arm) >= arm_min:
            row(f"  arm {n + 1} (instr {arm[0]}..{arm[-1]})", arm)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("pattern", nargs="?", default=".", help="regular expression over the kernel symbols")
    ap.add_argument("--loops", metavar="SYMBOL", help="per-loop breakdown of this kernel symbol")
    ap.add_argument("--arm", type=int, default=400, help="least length of a branch that splits a loop into arms")
    a = ap.parse_args()
    text = open(a.listing).read()
    if a.loops:
        loop_table(text, a.loops, a.arm)
    else:
        whole_kernels(text, re.compile(a.pattern))


if __name__ == "__main__":
    main()
