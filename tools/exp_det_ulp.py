"""The accuracy of exp_det (csrc/exp_det.h) in ulp, measured on the CPU through its NumPy restatement
(tests/softmax_cases.py), which equals the kernel's function bit for bit (tests/test_softmax_gpu.py):

    python tools/exp_det_ulp.py [--n 4000000] [--mp 200000]

float32 against float64 np.exp; float64 against mpmath on --mp arguments and against longdouble np.exp on --n.  The
arguments cover (-underflow, 0] densely, the subnormal results, multiples of ln2 / 2 and the neighbourhood of 0 down to 1e-8.
DESIGN A14 records the output; tests/softmax_cases.py takes U from it, rounded up to the next half ulp."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import softmax_cases as sc  # noqa: E402


def report(name, d, got, want, dtype):
    err = sc.ulp_error(got, want)
    sub = np.abs(want) < np.finfo(dtype).smallest_normal
    i = int(np.argmax(err))
    print(f"{name}: {len(d)} arguments, largest error {err[~sub].max():.4f} ulp (normal results), "
          f"{err[sub].max() if sub.any() else 0:.4f} ulp (subnormal results); worst at d = {d[i]!r}")
    return float(err.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4_000_000)
    ap.add_argument("--mp", type=int, default=200_000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    d = sc.exp_arguments(rng, a.n, np.float32)
    report("float32 vs float64 np.exp", d, sc.exp_det(d, np.float32), np.exp(d.astype(np.float64)), np.float32)
    d = sc.exp_arguments(rng, a.n, np.float64)
    report("float64 vs longdouble np.exp", d, sc.exp_det(d, np.float64), np.exp(d.astype(np.longdouble)), np.float64)
    import mpmath

    d = sc.exp_arguments(rng, a.mp, np.float64)
    with mpmath.workprec(200):
        want = np.array([np.longdouble(mpmath.nstr(mpmath.exp(mpmath.mpf(float(v))), 25)) for v in d], dtype=np.longdouble)
    report("float64 vs mpmath", d, sc.exp_det(d, np.float64), want, np.float64)


if __name__ == "__main__":
    main()
