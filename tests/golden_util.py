"""Shared helpers to replay tests/golden/*.json cases against any implementation."""
import json
import os

import numpy as np

import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))


def load(name="lbfgs_golden.json"):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def unhex(lst):
    return np.array([float.fromhex(v) for v in lst], dtype=np.float64)


def case_inputs(c):
    dtype, n = c["dtype"], c["n"]
    if c["obj"] == O.OBJ_ROSEN:
        x0 = O.rosen_x0(n, c["seed"], dtype) if c["hash_x0"] else np.zeros(n, O.NPDT[dtype])
        a = b = None
    else:
        x0 = np.zeros(n, O.NPDT[dtype])
        a, b = O.quad_problem(n, c["kappa"], 1, dtype)
    return x0, a, b


# ---- tests/cpp/policy10_capi.cpp: the built-in line-search policies through the reference's ten-argument static form
POLICY10_CASES = [(0, (1, 2, 3)), (1, (1, 2, 3)), (2, (3,)), (3, (3,))]   # (policy, conditions): 0 backtracking, 1 bracketing,
POLICY10_TRIALS, POLICY10_NMAX = 300, 20                                     # 2 More-Thuente, 3 Nocedal-Wright


def policy10_trials(policy, conditions):
    """The seeded inputs of test_built_in_policies_offer_the_reference_signature_with_the_reference_results: random descent
    (and a few ascent / degenerate) directions of the extended Rosenbrock function.  Yields (xp, drt, args) with args the
    leading arguments of policy10() (the pointers refer to xp and drt)."""
    import ctypes as C
    rng = np.random.default_rng(1234 + policy)
    for trial in range(POLICY10_TRIALS):
        n = int(rng.choice([2, 6, POLICY10_NMAX]))
        xp = np.where(np.arange(n) % 2 == 1, 1.0, -1.2) + 0.4 * rng.random(n)
        g = np.zeros(n)
        for i in range(0, n, 2):
            t1, t2 = 1.0 - xp[i], 10.0 * (xp[i + 1] - xp[i] ** 2)
            g[i + 1] = 20.0 * t2
            g[i] = -2.0 * (xp[i] * g[i + 1] + t1)
        kind = trial % 10
        drt = -g * (10.0 ** rng.uniform(-4, 1)) + (0.3 * rng.standard_normal(n) * np.abs(g).mean() if kind >= 3 else 0.0)
        if kind == 9:
            drt = g.copy()  # ascent: the policies throw
        step0 = float(10.0 ** rng.uniform(-3, 1)) if kind != 8 else -1.0
        cond = int(conditions[trial % len(conditions)])
        args = (policy, cond, n, xp.ctypes.data_as(C.c_void_p), drt.ctypes.data_as(C.c_void_p), step0, 1e20,
                1e-4, 0.9, 1e-20 if kind != 7 else 1e-3, 1e20 if kind != 6 else 2.0, int(rng.choice([3, 8, 20])))
        yield xp, drt, args


def policy10_lib(path):
    import ctypes as C
    lib = C.CDLL(path)
    lib.policy10.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_double] * 6 + [C.c_int] + [C.c_void_p] * 3
    return lib


def policy10_run(lib, args):
    """(rc, out[4] = step, fx, dg, evaluations, x, grad) of one policy10() call"""
    import ctypes as C
    n = args[2]
    out, x, gr = np.zeros(4), np.zeros(n), np.zeros(n)
    rc = lib.policy10(*args, out.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), gr.ctypes.data_as(C.c_void_p))
    return rc, out, x, gr


# ---- parameter validation: one bad field each (Param.h's checks), the reference's messages in tests/golden/param_messages.json
PARAM_BAD = [dict(m=0), dict(epsilon=-1.0), dict(epsilon_rel=-1.0), dict(past=-1), dict(delta=-1.0), dict(max_iterations=-1),
             dict(max_linesearch=0), dict(min_step=-1.0), dict(max_step=1e-30), dict(ftol=0.0), dict(ftol=0.6),
             dict(wolfe=1e-5), dict(wolfe=1.0)]
