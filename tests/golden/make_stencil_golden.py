#!/usr/bin/env python
"""Reference side of the grid-stencil tests (tests/test_stencil_objective_gpu.py), computed once and committed.

tests/cpp/stencil_probe.cpp -- a Swift-Hohenberg / plate energy of 3x3 patches on a grid, open or periodic per direction,
through LBFGSSolver (More-Thuente) and LBFGSBSolver (box [-0.25, 0.6]) -- is compiled here against the UNMODIFIED reference
headers with oracle/eigen_shim as Eigen, in a temporary directory outside the repository, twice: with the shim's native
accumulation (-DSHIM_ACC=0) and with its double-double accumulation (-DSHIM_ACC=1).  The two differ only in how the solvers' dot
products are rounded, so the iterations over which they agree are the ones an implementation with yet another summation order
can be held to: for each instance only the leading iterations are recorded over which the two builds have the same counts and
x and f within a tenth of the project's iterate tolerance (TOL[F64] = 1e-10 of tests/test_lbfgs_gpu.py).  An instance left with
fewer than 8 such iterations is refused.  The double-double build's values are stored, with the spread seen, and how many
coordinates end at a bound.  This is the recipe of make_field_golden.py.

    python tests/golden/make_stencil_golden.py [--ref /root/reference]
"""
import argparse
import base64
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "stencil_golden.json")
TOL = 1e-10
# (shape, mask) -> iterations asked of the probe (the fixture stores every x): a torus, a channel (periodic columns), a
# cylinder (periodic rows) and the open plate
INSTANCES = {((6, 8), 3): 12, ((6, 8), 1): 12, ((5, 7), 2): 12, ((6, 7), 0): 12}
C0, LB, UB = 1.0, -0.25, 0.6  # kC0, kLo, kHi of the probe
MIN_ITERATIONS = 8


def run_probe(exe, shape, mask, kmax):
    n = int(np.prod(shape))
    out = subprocess.run([exe] + [str(v) for v in tuple(shape) + (mask, kmax)], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    assert "STENCIL PROBE OK" in out, out[-2000:]
    rows = {"lbfgs": [], "lbfgsb": []}
    for line in out.splitlines():
        w = line.split()
        if w and w[0] in rows:
            assert int(w[1]) == len(rows[w[0]]) + 1 and len(w) == 5 + n
            rows[w[0]].append((int(w[2]), int(w[3]), float(w[4]), np.array([float(v) for v in w[5:]])))
    return rows


def pack(x):
    return base64.b64encode(np.ascontiguousarray(x, "<f8").tobytes()).decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference", help="checkout of the reference (its include/ is used)")
    args = ap.parse_args()
    golden = {"tolerance": TOL, "c0": C0, "instances": []}
    with tempfile.TemporaryDirectory() as d:
        exes = {}
        for acc in (0, 1):
            exes[acc] = os.path.join(d, "stencil_probe_acc%d" % acc)
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DSHIM_ACC=%d" % acc,
                                   "-I", os.path.join(args.ref, "include"), "-I", os.path.join(ROOT, "oracle", "eigen_shim"),
                                   os.path.join(ROOT, "tests", "cpp", "stencil_probe.cpp"), "-o", exes[acc]])
        for (shape, mask), kmax in INSTANCES.items():
            native, dd = run_probe(exes[0], shape, mask, kmax), run_probe(exes[1], shape, mask, kmax)
            name = "%s mask %d" % (" x ".join(str(v) for v in shape), mask)
            for solver in ("lbfgs", "lbfgsb"):
                keep, spread_x, spread_f = 0, 0.0, 0.0
                for a, b in zip(native[solver], dd[solver]):
                    dx, df = float(np.abs(a[3] - b[3]).max()), abs(a[2] - b[2])
                    if a[:2] != b[:2] or dx > TOL / 10 or df > TOL / 10:
                        break
                    keep += 1
                    spread_x, spread_f = max(spread_x, dx), max(spread_f, df)
                rows = dd[solver][:keep]
                at_bound = int(np.sum((rows[-1][3] == LB) | (rows[-1][3] == UB))) if (rows and solver == "lbfgsb") else 0
                print("%s %s: %d of %d iterations agree, spread x %.3g f %.3g, last niter %d, %d coordinates at a bound"
                      % (name, solver, keep, kmax, spread_x, spread_f, rows[-1][0] if rows else 0, at_bound))
                if keep < MIN_ITERATIONS:
                    raise SystemExit("%s %s: only %d iterations agree between the two accumulations: not written"
                                     % (name, solver, keep))
                golden["instances"].append({
                    "solver": solver, "shape": list(shape), "periodic": mask, "m": 6, "lb": LB, "ub": UB,
                    "iterations": keep, "spread_x": spread_x, "spread_f": spread_f, "at_bound": at_bound,
                    "niter": [r[0] for r in rows], "nfev": [r[1] for r in rows], "f": [r[2] for r in rows],
                    "x_f8_base64": [pack(r[3]) for r in rows]})
    with open(OUT, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
