"""csrc/div_recip.h (floor(r / d) through a double reciprocal: the division of every key <-> coordinate conversion of
csrc/prims.hip) compiled for the HOST into a stand-alone program, tests/div_recip_check.cpp, that compares the 32-bit and the
64-bit instantiation with exact integer division at q d - 1, q d and q d + 1 over [0, 2^32) and [0, 2^52), counts how often
each of the two repairs fires and checks that the 32-bit form's product cannot wrap.  No GPU.  With the undefined-behaviour
sanitizer where the compiler has it: a product with the reciprocal that no longer fits the unsigned word is then an error,
not a lucky result."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sparse_amd", "csrc")


def _compilers():
    out = []
    for name in ("c++", "g++", "clang++"):
        path = shutil.which(name)
        if path:
            out.append([path])
    for path in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if path and os.path.exists(path):
            out.append([path, "-x", "c++"])          # host only: the header's qualifiers are empty without the HIP language
    return out


def test_reciprocal_division_against_integer_division_on_the_host(tmp_path):
    compilers = _compilers()
    if not compilers:
        pytest.skip("no host C++ compiler and no hipcc")
    exe = str(tmp_path / "div_recip_check")
    base = ["-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "div_recip_check.cpp"), "-o", exe]
    errors = []
    for cc in compilers:
        for extra in (["-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all"], []):
            r = subprocess.run(cc + extra + base, capture_output=True, text=True)
            if r.returncode == 0:
                break
            errors.append(r.stderr[-2000:])
        if r.returncode == 0:
            break
    assert r.returncode == 0, "\n".join(errors)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout[-4000:], run.stderr[-4000:])
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1].startswith("OK:"), run.stdout[-4000:] + run.stderr[-4000:]
    # what the header's comment says about the two repairs is what the program counted
    counts = re.findall(r"--q repairs (\d+), \+\+q repairs (\d+)", run.stdout)
    assert len(counts) == 2, run.stdout
    assert all(int(down) == 0 for down, _ in counts), "the --q repair fired: the comment in csrc/div_recip.h says it does not"
    assert all(int(up) > 0 for _, up in counts), "the ++q repair never fired: the cases do not reach it"


def test_the_kernels_use_the_header():
    """prims.hip has no second copy of the function that the host program could not see"""
    text = open(os.path.join(CSRC, "prims.hip")).read()
    assert '#include "div_recip.h"' in text
    assert not re.search(r"\bU\s+div_recip\s*\(", text)
