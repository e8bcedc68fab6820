#!/usr/bin/env python
"""Reference side of the periodic-objective tests (tests/test_periodic_objective_gpu.py), computed once and committed.

tests/cpp/periodic_probe.cpp -- the Allen-Cahn energy on a grid or a 3-D array with periodic boundaries through LBFGSSolver
(More-Thuente) and LBFGSBSolver (box [-0.5, 2]) -- is compiled here against the UNMODIFIED reference headers with
oracle/eigen_shim as Eigen, in a temporary directory outside the repository, twice: with the shim's native accumulation
(-DSHIM_ACC=0) and with its double-double accumulation (-DSHIM_ACC=1).  The two differ only in how the solvers' dot products
are rounded, so the iterations over which they agree are the ones an implementation with yet another summation order can be
held to: for each instance only the leading iterations are recorded over which the two builds have the same counts and x and
f within a tenth of the project's iterate tolerance (TOL[F64] = 1e-10 of tests/test_lbfgs_gpu.py).  An instance left with
fewer than 8 such iterations is refused.  The double-double build's values are stored, with the spread seen.  This is the
recipe of make_volume_golden.py.

    python tests/golden/make_periodic_golden.py [--ref /root/reference]
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
OUT = os.path.join(HERE, "periodic_golden.json")
TOL = 1e-10
# (shape, mask) -> iterations asked of the probe (the fixture stores every x): a full torus in 2-D and in 3-D, and a grid that
# is periodic in the column direction only (a channel)
INSTANCES = {((6, 8), 3): 12, ((4, 6, 8), 7): 12, ((6, 8), 1): 12}
C0 = 1.0  # kC0 of the probe
MIN_ITERATIONS = 8


def run_probe(exe, shape, mask, kmax):
    n = int(np.prod(shape))
    shape3 = (0,) * (3 - len(shape)) + tuple(shape)
    out = subprocess.run([exe] + [str(v) for v in shape3] + [str(mask), str(kmax)], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    assert "PERIODIC PROBE OK" in out, out[-2000:]
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
            exes[acc] = os.path.join(d, "periodic_probe_acc%d" % acc)
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DSHIM_ACC=%d" % acc,
                                   "-I", os.path.join(args.ref, "include"), "-I", os.path.join(ROOT, "oracle", "eigen_shim"),
                                   os.path.join(ROOT, "tests", "cpp", "periodic_probe.cpp"), "-o", exes[acc]])
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
                print("%s %s: %d of %d iterations agree, spread x %.3g f %.3g" % (name, solver, keep, kmax, spread_x, spread_f))
                if keep < MIN_ITERATIONS:
                    raise SystemExit("%s %s: only %d iterations agree between the two accumulations: not written"
                                     % (name, solver, keep))
                rows = dd[solver][:keep]
                golden["instances"].append({
                    "solver": solver, "shape": list(shape), "periodic": mask, "m": 6, "lb": -0.5, "ub": 2.0,
                    "iterations": keep, "spread_x": spread_x, "spread_f": spread_f,
                    "niter": [r[0] for r in rows], "nfev": [r[1] for r in rows], "f": [r[2] for r in rows],
                    "x_f8_base64": [pack(r[3]) for r in rows]})
    with open(OUT, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
