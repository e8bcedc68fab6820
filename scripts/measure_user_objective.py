#!/usr/bin/env python3
"""What a caller-supplied objective costs ("User objectives"): the three measurements of profiles/user_objective.json.

    python scripts/measure_user_objective.py [--out profiles/user_objective.json] [--count 1024] [--n 100000] [--single-n 100000000]

1. lbfgsx_bat_pack / lbfgsx_bat_unpack against the launches they replace (LBFGSX_BAT_POINT / LBFGSX_BAT_GDOT) at cfg5's
   shape: device-event time per launch (lbfgsx_bat_timing), bytes of each launch's own model over that time.
2. problem-iterations/s of the callback batch (torch extended Rosenbrock over the packed rows) beside the built-in batch.
3. wall time per objective evaluation of the single-problem callback path (torch extended Rosenbrock) beside the built-in
   fused trial, n = 1e8 f64.
Needs a GPU; fails without one.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Desc(C.Structure):  # lbfgsx_bat_desc
    _fields_ = [("active", C.c_int), ("mode", C.c_int), ("x_in", C.c_int), ("x_out", C.c_int), ("col_u", C.c_int),
                ("col_w", C.c_int), ("i_num", C.c_int), ("i_den", C.c_int), ("i_num2", C.c_int), ("i_theta", C.c_int),
                ("i_out", C.c_int), ("pad", C.c_float), ("step", C.c_double)]


def rosen_rows(torch):
    def fn(ids, X, G):
        x0, x1 = X[:, 0::2], X[:, 1::2]
        t1 = 1.0 - x0
        t2 = 10.0 * (x1 - x0 * x0)
        g1 = 20.0 * t2
        G[:, 1::2] = g1
        G[:, 0::2] = -2.0 * (x0 * g1 + t1)
        return (t1 * t1 + t2 * t2).sum(dim=1, dtype=torch.float64)
    return fn


def rosen_single(torch):
    def fn(x, g):
        x0, x1 = x[0::2], x[1::2]
        t1 = 1.0 - x0
        t2 = 10.0 * (x1 - x0 * x0)
        g1 = 20.0 * t2
        g[1::2] = g1
        g[0::2] = -2.0 * (x0 * g1 + t1)
        return float((t1 * t1 + t2 * t2).sum())
    return fn


def streaming(core, L, P, n, reps):
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    for name, res, args in (("lbfgsx_bat_create", i32, [C.POINTER(vp), i32, i64, i32, i32, i32]), ("lbfgsx_bat_destroy", None, [vp]),
                            ("lbfgsx_bat_scalar_index", i32, [vp, i32, i32]), ("lbfgsx_bat_launch", i32, [vp, i32, i32, vp, i32, vp]),
                            ("lbfgsx_bat_pack", i32, [vp, vp]), ("lbfgsx_bat_unpack", i32, [vp, vp, vp]), ("lbfgsx_bat_sync", i32, [vp]),
                            ("lbfgsx_bat_timing", i32, [vp, i32]), ("lbfgsx_bat_timing_read", i32, [vp, vp]),
                            ("lbfgsx_bat_gen_rosen_x0", i32, [vp, C.c_uint64])):
        f = getattr(core, name)
        f.restype, f.argtypes = res, args
    bat = vp()
    L.check(core.lbfgsx_bat_create(C.byref(bat), L.F32, n, 1, P, 0))
    desc = (Desc * P)()
    for p in range(P):
        d = desc[p]
        d.active, d.x_in, d.x_out, d.col_u, d.step, d.i_out = 1, 0, 1, p, 0.5, core.lbfgsx_bat_scalar_index(bat, 3, 0)
    L.check(core.lbfgsx_bat_gen_rosen_x0(bat, 1))
    out = np.zeros(P)
    outp = out.ctypes.data_as(vp)
    runs = {"LBFGSX_BAT_POINT": (3, lambda: core.lbfgsx_bat_launch(bat, 4, -1, desc, 0, None)),
            "lbfgsx_bat_pack": (4, lambda: core.lbfgsx_bat_pack(bat, desc)),
            "LBFGSX_BAT_GDOT": (2, lambda: core.lbfgsx_bat_launch(bat, 5, -1, desc, 1, outp)),
            "lbfgsx_bat_unpack": (3, lambda: core.lbfgsx_bat_unpack(bat, desc, outp))}
    res = {}
    t = (C.c_double * 4)()
    for name, (vectors, call) in runs.items():  # warm up every shape first
        L.check(call())
    L.check(core.lbfgsx_bat_sync(bat))
    for rnd in range(2):  # alternate the four, twice
        for name, (vectors, call) in runs.items():
            L.check(core.lbfgsx_bat_timing(bat, 1))
            L.check(core.lbfgsx_bat_timing_read(bat, t))
            for _ in range(reps):
                L.check(call())
            L.check(core.lbfgsx_bat_timing_read(bat, t))
            ms = t[0] / t[1]
            nbytes = vectors * n * 4 * P
            res.setdefault(name, []).append({"ms_per_launch": ms, "model_bytes": nbytes, "GB_per_s": nbytes / ms / 1e6})
    core.lbfgsx_bat_destroy(bat)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "user_objective.json"))
    ap.add_argument("--count", type=int, default=1024)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--single-n", type=int, default=100000000)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    from lbfgspp_amd import batched as B
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_user_objective.py needs a GPU")
    rec = {"device": torch.cuda.get_device_name(0), "shape": {"count": args.count, "n": args.n, "dtype": "f32"}}
    rec["streaming"] = streaming(core, L, args.count, args.n, 20)

    par = A.LBFGSParam(m=10, epsilon=0.0, epsilon_rel=0.0, max_iterations=args.iters)
    rng = np.random.default_rng(1000)
    x0 = (np.where(np.arange(args.n) % 2 == 1, 1.0, -1.2) + 0.4 * rng.random((args.count, args.n))).astype(np.float32)
    x0_dev = torch.as_tensor(x0, device="cuda:0")
    fn = rosen_rows(torch)
    batch = B.LockstepBatch(par, args.n, args.count, dtype=np.float32)
    legs = {"built_in": [], "torch_callback": []}
    for rnd in range(3):  # round 0 warms both up; then alternating
        for name in ("built_in", "torch_callback"):
            t0 = time.perf_counter()
            recs = batch.minimize(first=0, seed_base=1000) if name == "built_in" else batch.minimize_fn(fn, x0_dev)
            dt = time.perf_counter() - t0
            if rnd:
                legs[name].append({"s": dt, "problem_iterations_per_s": float(recs["niter"].sum()) / dt,
                                   "evaluations": int(recs["nfev"].sum()), **batch.stats})
    batch.close()
    rec["batch"] = {"iterations_per_problem": args.iters, "m": 10, **legs}
    del x0_dev
    torch.cuda.empty_cache()

    n1 = args.single_n
    single = {"n": n1, "dtype": "f64", "built_in": [], "torch_callback": []}
    par1 = A.LBFGSParam(m=6, epsilon=0.0, epsilon_rel=0.0, max_iterations=5)
    s = A.LBFGSSolver(par1, linesearch=A.LS_MORE_THUENTE)
    xd = torch.empty(n1, dtype=torch.float64, device="cuda:0")
    start = torch.where(torch.arange(n1, device="cuda:0") % 2 == 1, 1.0, -1.2).double()
    for rnd in range(3):
        for name, f in (("built_in", A.ExtendedRosenbrock()), ("torch_callback", A.DeviceObjective(rosen_single(torch)))):
            xd.copy_(start)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            niter, fx = s.minimize(f, xd)
            dt = time.perf_counter() - t0
            if rnd:
                single[name].append({"s": dt, "niter": niter, "nfev": s.last.nfev, "s_per_evaluation_of_the_whole_solve": dt / s.last.nfev})
    rec["single"] = single
    json.dump(rec, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
