#!/usr/bin/env python3
"""What a periodic grid or volume objective (lbfgspp_amd.PeriodicGridObjective, PeriodicVolumeObjective) costs, in one process on
one device (profiles/periodic_objective.json).

  trial   n ~ 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of the timed calls after warm-up, the tile order alternating as in a search; the legs of a
          context alternate, so every ratio is taken inside one process on one device) of the torus Allen-Cahn energy
            on 10000 x 10000  against (a) GridObjective with the same cell on the same shape (the open form's kernels,
                              unchanged), (b) the built-in ExtendedRosenbrock at that n and (c) a torch callable written with
                              torch.roll (trial point + callable + grad.d: what a DeviceObjective costs per evaluation);
            on 464^3          against VolumeObjective, the built-in and the torch callable in the same way;
          and the half-periodic forms (grid: columns only; volume: rows only) beside them.
  code    VGPRs and scratch of the compiled bodies, from the code object.

    python scripts/measure_periodic_objective.py [--out profiles/periodic_objective.json] [--side 464] [--grid-side 10000]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

C0 = 4.0
STEP = 0.37


def torus_torch(torch, shape):
    """the torus Allen-Cahn energy and its gradient with torch.roll: every lattice edge has the weight 1/2 in total"""
    dims = tuple(range(len(shape)))

    def fn(x, g):
        X = x.view(shape)
        G = g.view(shape)
        u = X * X - 1.0
        G.copy_(C0 * (u * X))
        e = (0.25 * C0) * (u * u)
        for ax in dims:
            d = torch.roll(X, -1, ax) - X
            e = e + 0.5 * (d * d)
            G.sub_(d)
            G.add_(torch.roll(d, 1, ax))
        return float(e.sum())
    return fn


class Bench:
    """one context of n f64 coordinates with random xp and d, ready for trial evaluations"""

    def __init__(self, torch, core, L, n):
        self.torch, self.core, self.L, self.n = torch, core, L, n
        self.h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(self.h), L.F64, n, 1, 0, 0))
        gen = torch.Generator(device="cuda:0").manual_seed(1)
        self.vec(L.VEC_X).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        self.vec(L.VEC_D).copy_(torch.rand(n, dtype=torch.float64, device="cuda:0", generator=gen) - 0.5)
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(self.h))
        self.fx, self.dg = C.c_double(), C.c_double()

    def vec(self, v):
        return self.L.device_tensor(self.core.lbfgsx_vec(self.h, v), (self.n,), np.float64, 0)

    def trial(self, oid):
        t0 = time.perf_counter()
        self.L.check(self.core.lbfgsx_trial(self.h, oid, STEP, C.byref(self.fx), C.byref(self.dg)))
        return (time.perf_counter() - t0) * 1e3

    def callable_trial(self, fn):
        t0 = time.perf_counter()
        self.L.check(self.core.lbfgsx_trial_point(self.h, STEP))
        self.L.check(self.core.lbfgsx_sync(self.h))
        fn(self.vec(self.L.VEC_XT), self.vec(self.L.VEC_GT))
        self.torch.cuda.synchronize()
        self.L.check(self.core.lbfgsx_trial_dg(self.h, C.byref(self.dg)))
        return (time.perf_counter() - t0) * 1e3

    def close(self):
        self.core.lbfgsx_destroy(self.h)
        self.torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "periodic_objective.json"))
    ap.add_argument("--side", type=int, default=464)
    ap.add_argument("--grid-side", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    import periodic_ref as PR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_periodic_objective.py needs a GPU")
    gshape, vshape = (args.grid_side, args.grid_side), (args.side,) * 3
    objs = {"grid": A.GridObjective(PR.ALLENCAHN, shape=gshape, scalars=(C0,)),
            "periodic_grid": A.PeriodicGridObjective(PR.ALLENCAHN, shape=gshape, scalars=(C0,)),
            "volume": A.VolumeObjective(PR.ALLENCAHN3, shape=vshape, scalars=(C0,)),
            "periodic_volume": A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=vshape, scalars=(C0,))}
    cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)

    def bind(b, name, shape, mask=None):
        oid = C.c_int(-1)
        fn = getattr(core, {"grid": "lbfgsx_objective_bind_grid", "volume": "lbfgsx_objective_bind_volume",
                            "periodic_grid": "lbfgsx_objective_bind_grid_periodic",
                            "periodic_volume": "lbfgsx_objective_bind_volume_periodic"}[name])
        extra = () if mask is None else (mask,)
        L.check(fn(b.h, objs[name].compile(), *shape, *extra, None, C.byref(cs), C.byref(oid)))
        return oid.value

    rec = {"device": torch.cuda.get_device_name(0), "code": {k: v.info() for k, v in objs.items()}}
    times = {}

    def run(b, legs):
        """legs: [(name, form or None, mask, callable or None)]; a leg binds its objective, then times its calls; round 0 warms
        every leg up, the legs of a context alternate"""
        for name, *_ in legs:
            times[name] = []
        for rnd in range(args.rounds):
            for name, form, mask, fn in legs:
                if fn is not None:
                    call = lambda: b.callable_trial(fn)
                elif form is None:
                    call = lambda: b.trial(L.OBJ_EXT_ROSENBROCK)
                else:
                    oid = bind(b, form, gshape if "grid" in form else vshape, mask)
                    call = lambda: b.trial(oid)
                ms = [call() for _ in range(args.calls)]
                if rnd:
                    times[name] += ms[2:]

    b = Bench(torch, core, L, gshape[0] * gshape[1])
    run(b, [("built_in_at_grid_n", None, None, None), ("grid_open", "grid", None, None), ("grid_torus", "periodic_grid", 3, None),
            ("grid_columns_periodic", "periodic_grid", 1, None), ("grid_mask_0", "periodic_grid", 0, None),
            ("grid_torch_roll", None, None, torus_torch(torch, gshape))])
    b.close()
    b = Bench(torch, core, L, vshape[0] * vshape[1] * vshape[2])
    run(b, [("built_in_at_volume_n", None, None, None), ("volume_open", "volume", None, None),
            ("volume_torus", "periodic_volume", 7, None), ("volume_rows_periodic", "periodic_volume", 2, None),
            ("volume_mask_0", "periodic_volume", 0, None), ("volume_torch_roll", None, None, torus_torch(torch, vshape))])
    b.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec["trial"] = {"shapes": {"grid": list(gshape), "volume": list(vshape)},
                    "n": {"grid": gshape[0] * gshape[1], "volume": vshape[0] * vshape[1] * vshape[2]},
                    "dtype": "f64", "step": STEP, "timed_calls_per_leg": len(times["grid_open"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "grid_torus_over_open": med["grid_torus"] / med["grid_open"],
                    "volume_torus_over_open": med["volume_torus"] / med["volume_open"],
                    "grid_torus_over_built_in": med["grid_torus"] / med["built_in_at_grid_n"],
                    "volume_torus_over_built_in": med["volume_torus"] / med["built_in_at_volume_n"],
                    "torch_roll_over_grid_torus": med["grid_torch_roll"] / med["grid_torus"],
                    "torch_roll_over_volume_torus": med["volume_torch_roll"] / med["volume_torus"]}
    json.dump(rec, open(args.out, "w"))
    print(json.dumps(rec["trial"]))


if __name__ == "__main__":
    main()
