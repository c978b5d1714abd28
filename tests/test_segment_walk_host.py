"""csrc/segment_walk.h (the window walk and the slot rule that the long forms of softmax, attention, the semiring products and
mttkrp share) compiled for the HOST into a stand-alone program, tests/segment_walk_check.cpp, that walks every window of
pointer arrays with every boundary length and asserts: the pieces found are exactly the pieces of the long segments, each
once and at most two per window; seg_slot is injective over them, below 2 nwin, and slot / 2 is the window that found the
piece.  No GPU.  With the undefined-behaviour sanitizer where the compiler has it."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "sparse_amd", "csrc")
OWN = r"\b(?!seg_)\w+_(row_of|seg_of|slot)\s*\("   # a search or a slot rule under a file's own prefix, defined or called
WALKERS = ("softmax.hip", "attention.hip", "attention_grad.hip", "semiring_spmm.hip", "semiring_grad.hip", "mttkrp.hip")


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


def test_window_walk_and_slots_on_the_host(tmp_path):
    compilers = _compilers()
    if not compilers:
        pytest.skip("no host C++ compiler and no hipcc")
    exe = str(tmp_path / "segment_walk_check")
    base = ["-std=c++17", "-O2", "-I", CSRC, os.path.join(HERE, "segment_walk_check.cpp"), "-o", exe]
    errors = []
    for cc in compilers:
        for extra in (["-fsanitize=undefined", "-fno-sanitize-recover=all"], []):
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
    arrays, pieces, two = map(int, re.search(r"OK: (\d+) pointer arrays, (\d+) pieces, (\d+) windows with two", run.stdout).groups())
    assert arrays > 20000 and pieces > arrays and two > 1000, "the cases do not reach what they are meant to reach"


def test_the_kernels_use_the_header():
    """none of the six files has a second copy of the search or of the slot rule that the host program could not see"""
    for name in WALKERS:
        text = open(os.path.join(CSRC, name)).read()
        assert "seg_window_pieces(" in text, name
        assert not re.search(OWN, text), name
    assert not re.search(OWN, open(os.path.join(CSRC, "attention_common.h")).read())
