"""CPU: tools/isa_diff.py on hand-written listings -- the mapped form (several
old listings, a map of renamed kernel symbols) says `identical` for the same
code under new names and names the kernel and the part that differs otherwise;
the two-file form is unchanged.  No compiler and no GPU is needed."""
import pathlib
import subprocess
import sys

TOOL = pathlib.Path(__file__).resolve().parent.parent / "tools" / "isa_diff.py"

KERNEL = """\
\t.protected\t{n}                     ; -- Begin function {n}
{n}:                                    ; @{n}
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB{f}_1:
\t{insn}
\ts_cbranch_scc1 .LBB{f}_1
\ts_endpgm
\t.amdhsa_kernel {n}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
                                        ; -- End function
\t.set {n}.num_vgpr, {vgpr}
"""
TABLE = "\t.type\ttab,@object\ntab:\n\t.quad\t0x3ff0000000000000\n\t.size\ttab, 8\n"
META = "  - .name:           {n}\n    .symbol:         {n}.kd\n    .vgpr_count:     {vgpr}\n"


def listing(path, names, first=0, insn="v_add_f64 v[0:1], v[0:1], v[2:3]", vgpr=4, changed=()):
    """a listing with one kernel per name; the kernels in `changed` take insn / vgpr, the others the defaults"""
    ks = [dict(n=n, f=first + i, insn=insn if n in changed else "v_add_f64 v[0:1], v[0:1], v[2:3]",
               vgpr=vgpr if n in changed else 4) for i, n in enumerate(names)]
    path.write_text("\t.text\n" + "".join(KERNEL.format(**k) for k in ks) + TABLE +
                    "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + "".join(META.format(**k) for k in ks) +
                    "...\n\t.end_amdgpu_metadata\n")
    return str(path)


def run(*args):
    r = subprocess.run([sys.executable, str(TOOL), *args], capture_output=True, text=True)
    return r.returncode, r.stdout


def mapped(tmp_path, pairs=("old_a new_a", "old_b new_b"), **new):
    """two old listings of one kernel each against one new listing of both, renamed"""
    m = tmp_path / "syms.map"
    m.write_text("# OLD NEW\n" + "\n".join(pairs) + "\n")
    return run("--map", str(m), listing(tmp_path / "a.s", ["old_a"]), listing(tmp_path / "b.s", ["old_b"], first=7),
               listing(tmp_path / "new.s", ["new_a", "new_b"], **new))


def test_mapped_identical(tmp_path):
    assert mapped(tmp_path) == (0, "identical: 2 kernels\n")


def test_mapped_changed_instruction(tmp_path):
    rc, out = mapped(tmp_path, insn="v_mul_f64 v[0:1], v[0:1], v[2:3]", changed=("new_b",))
    assert rc == 1 and out.startswith("kernel new_b: code differs") and "new_a" not in out, out


def test_mapped_changed_vgprs(tmp_path):
    rc, out = mapped(tmp_path, vgpr=5, changed=("new_a",))
    assert rc == 1 and out.startswith("kernel new_a: .amdhsa_* / .set block differs") and "new_b" not in out, out


def test_mapped_unmapped_old_kernel(tmp_path):
    rc, out = mapped(tmp_path, pairs=("old_a new_a",))
    assert rc == 1 and "kernel old_b: only in" in out and "kernel new_b: only in" in out and "new_a" not in out, out


def test_two_files(tmp_path):
    old = listing(tmp_path / "old.s", ["k_a", "k_b"])
    assert run(old, listing(tmp_path / "same.s", ["k_a", "k_b"], first=3)) == (0, "identical: 2 kernels\n")
    rc, out = run(old, listing(tmp_path / "new.s", ["k_a", "k_b"], vgpr=5, changed=("k_b",)))
    assert rc == 1 and out.startswith("kernel k_b: .amdhsa_* / .set block differs"), out
