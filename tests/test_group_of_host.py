"""csrc/group_of.h (the group id of a key, k / divisor, in the two forms the grouped reduce uses) compiled for the HOST into
a stand-alone program, tests/group_of_check.cpp, that compares both forms with exact integer division at q d - 1, q d and
q d + 1 over [0, 2^53) and [0, 2^63) and bounds the integer form's correction loops.  No GPU.  With the undefined-behaviour
sanitizer where the compiler has it: a double outside int64's range converted to int64 (what the top 512 keys with divisor 1
did before the estimate was clamped) is then an error, not a lucky result."""
import os
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


def test_group_ids_against_integer_division_on_the_host(tmp_path):
    compilers = _compilers()
    if not compilers:
        pytest.skip("no host C++ compiler and no hipcc")
    exe = str(tmp_path / "group_of_check")
    base = ["-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "group_of_check.cpp"), "-o", exe]
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
