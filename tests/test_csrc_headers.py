"""CPU: every header under gsoc17-hhmm_amd/csrc has `#pragma once`, includes
what it names and compiles when it is the only thing included (DESIGN.md
§3.18): a translation unit may then include exactly the headers it uses, and
the compiler-written dependency files of csrc/Makefile are the whole truth.
A host-only syntax pass; nothing is built and no GPU is needed."""
import os
import pathlib
import shutil
import subprocess

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
CSRC = REPO / "gsoc17-hhmm_amd" / "csrc"
HEADERS = sorted(p.name for p in CSRC.glob("*.h"))


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and pathlib.Path(c).exists():
            return c
    return None


HIPCC = _hipcc()


def test_headers_found():
    assert "hhmm_hmm.h" in HEADERS and "hhmm_step.h" in HEADERS and len(HEADERS) >= 20


@pytest.mark.skipif(HIPCC is None, reason="hipcc not installed")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    assert "#pragma once" in (CSRC / header).read_text()
    src = tmp_path / "only.hip"
    src.write_text(f'#include "{header}"\n')
    # -Wno-unused-command-line-argument: the hipcc wrapper adds a link option
    # of its own, which the driver reports as unused under -fsyntax-only; that
    # is about the command line, not the header
    r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only",
                        "-Wno-unused-command-line-argument", f"-I{REPO / 'include'}", f"-I{CSRC}", str(src)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and not r.stdout.strip() and not r.stderr.strip(), r.stdout + r.stderr
