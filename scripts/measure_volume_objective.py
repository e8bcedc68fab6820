#!/usr/bin/env python3
"""What a volume objective (2x2x2-cell terms on a slab-major 3-D array, lbfgspp_amd.VolumeObjective) costs, in one process on
one device (profiles/volume_objective.json).

  trial   n ~ 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of the 20 timed calls after warm-up, the tile order alternating as in a search) for
          (a) the built-in ExtendedRosenbrock and (b) the grid Allen-Cahn energy on 10000 x 10000, (c) the volume Allen-Cahn
          energy on 464^3 (cols % W == 0: every neighbouring pack is a 16-byte load), (d) the same on 463 x 465 x 465 (element
          loads) and (e) the torch callable of (c) (trial point + callable + grad.d, what a DeviceObjective costs per
          evaluation: what a user with a 3-D field had before this form).
  code    VGPRs and scratch of the compiled bodies, from the code object.

The bytes of one k_volume_trial launch past L2 are a counter run of their own: rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE,
no tracing combined, around this script with --pmc-program, which makes a few lbfgsx_trial calls of the built-in and of (c) and
nothing else; --counters <csv> ... then folds the per-launch figures into the "counters" entry of the file.

    python scripts/measure_volume_objective.py [--out profiles/volume_objective.json] [--side 464]
    rocprofv3 --pmc FETCH_SIZE -d <dir> -o fetch --output-format csv -- python scripts/measure_volume_objective.py --pmc-program
    python scripts/measure_volume_objective.py --counters <dir>/..._counter_collection.csv [...]
"""
import argparse
import csv
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


def allencahn3_torch(torch, shape):
    def fn(x, g):
        X = x.view(shape)
        G = g.view(shape)
        c = [X[ds:shape[0] - 1 + ds, dr:shape[1] - 1 + dr, dc:shape[2] - 1 + dc] for ds in (0, 1) for dr in (0, 1) for dc in (0, 1)]
        a = [c[1] - c[0], c[3] - c[2], c[5] - c[4], c[7] - c[6]]
        b = [c[2] - c[0], c[3] - c[1], c[6] - c[4], c[7] - c[5]]
        e = [c[4] - c[0], c[5] - c[1], c[6] - c[2], c[7] - c[3]]
        u = c[0] * c[0] - 1.0
        g.zero_()
        out = [G[ds:shape[0] - 1 + ds, dr:shape[1] - 1 + dr, dc:shape[2] - 1 + dc] for ds in (0, 1) for dr in (0, 1) for dc in (0, 1)]
        out[0] += -0.25 * (a[0] + b[0] + e[0]) + C0 * (u * c[0])
        out[1] += 0.25 * (a[0] - b[1] - e[1])
        out[2] += 0.25 * (b[0] - a[1] - e[2])
        out[3] += 0.25 * (a[1] + b[1] - e[3])
        out[4] += 0.25 * (e[0] - a[2] - b[2])
        out[5] += 0.25 * (a[2] + e[1] - b[3])
        out[6] += 0.25 * (b[2] + e[2] - a[3])
        out[7] += 0.25 * (a[3] + b[3] + e[3])
        sq = sum(d * d for d in a + b + e)
        return float((0.125 * sq + (0.25 * C0) * (u * u)).sum())
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


def fold_counters(paths):
    """{kernel: {counter: [value per launch]}} of rocprofv3's counter_collection csv files"""
    out = {}
    for path in paths:
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                kernel = "k_volume_trial" if "k_volume_trial" in name else "k_trial_built_in" if "k_trial" in name else None
                if kernel:
                    out.setdefault(kernel, {}).setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_objective.json"))
    ap.add_argument("--side", type=int, default=464)
    ap.add_argument("--grid-side", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pmc-program", action="store_true", help="a few trial calls of the built-in and of the aligned volume, no file")
    ap.add_argument("--counters", nargs="+", metavar="CSV", help="fold rocprofv3 counter files into the counters entry of --out")
    args = ap.parse_args()
    side = args.side
    shapes = {"aligned": (side, side, side), "unaligned": (side - 1, side + 1, side + 1)}
    if args.counters:
        rec = json.load(open(args.out))
        n = side ** 3
        rec["counters"] = {"what": "rocprofv3 --pmc, one counter per run, %d^3 f64 beside the built-in at the same n, per launch as "
                                   "reported (see profiles/grid_objective.json on what FETCH_SIZE reports on gfx950)" % side,
                           "model_bytes": {"read": 16 * n, "written": 16 * n}}
        rec["counters"].update(fold_counters(args.counters))
        vol, blt = rec["counters"].get("k_volume_trial", {}), rec["counters"].get("k_trial_built_in", {})
        if "FETCH_SIZE" in vol and "FETCH_SIZE" in blt:
            rec["counters"]["fetch_over_built_in"] = float(np.median(vol["FETCH_SIZE"]) / np.median(blt["FETCH_SIZE"]))
        json.dump(rec, open(args.out, "w"))
        print(json.dumps({k: v for k, v in rec["counters"].items() if k != "what"}))
        return
    import torch

    import lbfgspp_amd as A
    import grid_ref as GR
    import volume_ref as VR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_volume_objective.py needs a GPU")
    vol = A.VolumeObjective(VR.ALLENCAHN3, shape=shapes["aligned"], scalars=(C0,))
    grid = A.GridObjective(GR.ALLENCAHN, shape=(args.grid_side, args.grid_side), scalars=(C0,))
    cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)

    def bind_volume(b, shape):
        oid = C.c_int(-1)
        L.check(core.lbfgsx_objective_bind_volume(b.h, vol.compile(), *shape, None, C.byref(cs), C.byref(oid)))
        return oid.value

    if args.pmc_program:
        n = side ** 3
        b = Bench(torch, core, L, n)
        for _ in range(2):
            b.trial(L.OBJ_EXT_ROSENBROCK)
        oid = bind_volume(b, shapes["aligned"])
        for _ in range(4):
            b.trial(oid)
        b.close()
        return

    rec = {"device": torch.cuda.get_device_name(0), "code": {"allen_cahn_grid": grid.info(), "allen_cahn_volume": vol.info()}}
    times = {}

    def run(legs):
        """legs: [(name, call)]; round 0 warms every leg up, the legs of a context alternate"""
        for name, _ in legs:
            times[name] = []
        for rnd in range(args.rounds):
            for name, call in legs:
                ms = [call() for _ in range(args.calls)]
                if rnd:
                    times[name] += ms[2:]

    b = Bench(torch, core, L, args.grid_side ** 2)
    oid = C.c_int(-1)
    L.check(core.lbfgsx_objective_bind_grid(b.h, grid.compile(), args.grid_side, args.grid_side, None, C.byref(cs), C.byref(oid)))
    run([("built_in", lambda: b.trial(L.OBJ_EXT_ROSENBROCK)), ("allen_cahn_grid", lambda: b.trial(oid.value))])
    b.close()
    b = Bench(torch, core, L, side ** 3)
    fn = allencahn3_torch(torch, shapes["aligned"])
    vid = bind_volume(b, shapes["aligned"])
    run([("built_in_at_volume_n", lambda: b.trial(L.OBJ_EXT_ROSENBROCK)), ("allen_cahn_volume_aligned", lambda: b.trial(vid)),
         ("torch_callable", lambda: b.callable_trial(fn))])
    b.close()
    del fn
    s = shapes["unaligned"]
    b = Bench(torch, core, L, s[0] * s[1] * s[2])
    vid = bind_volume(b, s)
    run([("allen_cahn_volume_unaligned", lambda: b.trial(vid))])
    b.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec["trial"] = {"shapes": {"grid": [args.grid_side, args.grid_side], **{k: list(v) for k, v in shapes.items()}},
                    "n": {"grid": args.grid_side ** 2, "aligned": side ** 3, "unaligned": s[0] * s[1] * s[2]},
                    "dtype": "f64", "step": STEP, "timed_calls_per_leg": len(times["built_in"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "over_built_in_at_volume_n": {k: med[k] / med["built_in_at_volume_n"] for k in med},
                    "torch_callable_over_volume": med["torch_callable"] / med["allen_cahn_volume_aligned"],
                    "model_streams_of_n_elements": 4}
    json.dump(rec, open(args.out, "w"))
    print(json.dumps(rec["trial"]))


if __name__ == "__main__":
    main()
