"""-m gpu: a genuinely dense instance against the reference (tests/golden/dense_golden.json, written by
tests/golden/make_dense_golden.py from tests/cpp/dense_probe.cpp and the unmodified reference headers): logistic regression
with a ridge at D = 1 under LBFGSSolver and multi-target non-negative least squares at D = 3 under LBFGSBSolver with bounds
active at the start, over a matrix given by a closed formula that the probe and this file share.  Checked from Python
(lbfgspp_amd.DenseLinearObjective) and from a C++ program using DenseLinearObjective<double>; every recorded iteration is
compared, x and f within the fixture's own tolerance, the counts equal."""
import base64
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGISTIC = """
const T m = p0[r] * z[0];
const T e = exp(m > T(0) ? T(0) - m : m);
const T s = (m > T(0) ? e : T(1)) / (T(1) + e);
dz[0] = T(0) - p0[r] * s;
return (m > T(0) ? T(0) : T(0) - m) + log1p(e);"""
RIDGE = """
g[0] = c[0] * x[0];
return T(0.5) * (c[0] * (x[0] * x[0]));"""
SQUARES = """
T q = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    const T u = z[k] - p0[r * D + k];
    dz[k] = u;
    q = q + u * u;
}
return T(0.5) * q;"""


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    core, _ = A.load()
    assert core.lbfgsx_device_count() >= 1, "no GPU visible: these tests must run on the MI355X box"
    return A


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "dense_golden.json")) as f:
        g = json.load(f)
    assert g["tolerance"] == 1e-10 and os.path.getsize(f.name) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "multilinear_golden.json"))
    return g


def _probe_instance(A, inst, k):
    """tests/cpp/dense_probe.cpp: the matrix, the per-row data and start(), operation for operation"""
    R_, F, D = inst["R"], inst["F"], inst["D"]
    r, j = np.arange(R_)[:, None], np.arange(F)[None, :]
    dense = ((31 * r + 17 * j + 3 * r * j) % 13 - 6) / 4.0
    n = F * D
    t = (np.arange(n, dtype=np.float64) + 1.0) / float(n + 1)
    x0 = k["amp"] * ((0.5 - t) * (1.0 + t))
    r = r.reshape(-1)
    if inst["solver"] == "lbfgs":
        y = np.where((5 * r) % 3 == 0, -1.0, 1.0)
        return A.DenseLinearObjective(LOGISTIC, dense, 1, coord_body=RIDGE, data=(y,), scalars=(k["c0"],)), x0
    b = (((11 * r[:, None] + 5 * np.arange(D)[None, :]) % 7 - 3) / 2.0).reshape(-1)
    return A.DenseLinearObjective(SQUARES, dense, D, data=(b,)), x0


@pytest.mark.parametrize("inst", _golden()["instances"], ids=lambda i: "%s-%dx%dx%d" % (i["solver"], i["R"], i["F"], i["D"]))
def test_dense_models_follow_the_reference(A, inst):
    n, tol = inst["n"], 1e-10
    assert inst["iterations"] >= 8 and n == inst["F"] * inst["D"] and inst["D"] == (1 if inst["solver"] == "lbfgs" else 3)
    f, x0 = _probe_instance(A, inst, _golden()["constants"])
    lb, ub = np.zeros(n), np.full(n, np.inf)
    assert np.any(x0 < lb)  # bounds are active at the projected start
    for k in range(1, inst["iterations"] + 1):
        prm = dict(m=inst["m"], epsilon=0, epsilon_rel=0, max_iterations=k)
        x = x0.copy()
        if inst["solver"] == "lbfgs":
            s = A.LBFGSSolver(A.LBFGSParam(**prm), linesearch=A.LS_MORE_THUENTE)
            niter, fx = s.minimize(f, x)
        else:
            s = A.LBFGSBSolver(A.LBFGSBParam(past=0, **prm))
            niter, fx = s.minimize(f, x, lb, ub)
        x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
        assert x_ref.size == n
        dx, df = float(np.abs(x - x_ref).max()), abs(fx - inst["f"][k - 1])
        print("k %d: niter %d nfev %d |dx| %.3g |df| %.3g" % (k, niter, s.last.nfev, dx, df))
        assert (niter, s.last.nfev) == (inst["niter"][k - 1], inst["nfev"][k - 1])
        assert dx <= tol and df <= tol


def test_cpp_dense_linear_objective_follows_the_reference(tmp_path):
    """tests/cpp/dense_probe.cpp with DenseLinearObjective<double> in place of the functor, built with g++ against include/"""
    exe = str(tmp_path / "dense_probe")
    lib = os.path.join(ROOT, "lbfgspp_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DDENSE_PROBE_DEVICE", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "oracle", "eigen_shim"), os.path.join(ROOT, "tests", "cpp", "dense_probe.cpp"),
           "-o", exe, "-L" + lib, "-llbfgsx", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    insts = _golden()["instances"]
    for shape in sorted({(i["R"], i["F"]) for i in insts}):
        mine = [i for i in insts if (i["R"], i["F"]) == shape]
        kmax = max(i["iterations"] for i in mine)
        out = subprocess.run([exe] + [str(v) for v in shape] + [str(kmax)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                             text=True, timeout=300)
        assert out.returncode == 0 and "DENSE PROBE OK" in out.stdout, out.stdout[-2000:]
        rows_ = {}
        for line in out.stdout.splitlines():
            w = line.split()
            if w and w[0] in ("lbfgs", "lbfgsb"):
                rows_[(w[0], int(w[1]))] = (int(w[2]), float(w[4]), np.array([float(v) for v in w[5:]]))
        for inst in mine:
            for k in range(1, inst["iterations"] + 1):
                niter, fx, x = rows_[(inst["solver"], k)]
                x_ref = np.frombuffer(base64.b64decode(inst["x_f8_base64"][k - 1]), "<f8")
                assert niter == inst["niter"][k - 1]
                assert np.abs(x - x_ref).max() <= 1e-10 and abs(fx - inst["f"][k - 1]) <= 1e-10, (inst["solver"], shape, k)
