#!/usr/bin/env python3
"""What a graph objective (edge terms over an index list, lbfgspp_amd.GraphObjective) costs, in one process on one device
(profiles/graph_objective.json).

  trial   n = 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial: x = xp + step d, f, grad, grad.d; wall clock around the
          synchronous call, median of 20 timed calls after warm-up, the tile order alternating as in a search) for
          (a) the built-in ExtendedRosenbrock, (b) the K = 2 chained Rosenbrock, (c) the same body on the path graph
          (E = n - 1), (d) springs plus a double well on the 4-neighbour lattice 10000 x 10000 as a graph (E = 2 rows cols -
          rows - cols) with natural labels, (e) the same with the nodes relabelled by a fixed random permutation (no locality)
          and (f) the torch callable of (d) (index_select / index_add_; trial point + callable + grad.d, what a
          DeviceObjective costs per evaluation).
  build   the time of lbfgsx_objective_bind_graph (copy, validation, sort, offsets, entries) for the path and the lattice,
          from device-resident edge arrays.
  code    VGPRs and scratch of the compiled bodies, from the code object.

--counter-run LEG makes a few lbfgsx_trial calls of one leg and nothing else: the program for a counter run of its own
(rocprofv3 --pmc FETCH_SIZE, then --pmc WRITE_SIZE, no tracing combined); its figures go into the "counters" entry by hand.

    python scripts/measure_graph_objective.py [--out profiles/graph_objective.json] [--rows 10000] [--cols 10000]
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

CHAINED_ROSEN = """const T u = x[1] - x[0] * x[0];
const T v = T(1) - x[0];
g[1] = T(200) * u;
g[0] = T(-400) * (u * x[0]) - T(2) * v;
return T(100) * (u * u) + v * v;"""
SPRING = """const T d = x[0] - x[1];
g[0] = d;
g[1] = T(0) - d;
return T(0.5) * (d * d);"""
WELL = """const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = (T(4) * k) * (u * x[0]);
return k * (u * u);"""
C0 = 4.0


def lattice_torch(torch, ei, ej):
    ei, ej = ei.long(), ej.long()

    def fn(x, g):
        d = x.index_select(0, ei) - x.index_select(0, ej)
        u = x * x - 1.0
        torch.mul(u * x, C0, out=g)
        g.index_add_(0, ei, d)
        g.index_add_(0, ej, -d)
        return float(0.5 * (d * d).sum() + (0.25 * C0) * (u * u).sum())
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_objective.json"))
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--counter-run", default=None, help="one leg, a few trial calls, nothing written")
    args = ap.parse_args()
    import torch

    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_graph_objective.py needs a GPU")
    rows, cols = args.rows, args.cols
    n = rows * cols
    assert n % 2 == 0, "the built-in extended Rosenbrock leg needs an even n"
    dev = "cuda:0"
    rec = {"device": torch.cuda.get_device_name(0)}
    chain = A.ChainObjective(CHAINED_ROSEN, K=2)
    # compiled through the Python class for info(); bound below through the C ABI with device-resident edges
    path_obj = A.GraphObjective(CHAINED_ROSEN, edges=([0], [1]))
    lat_obj = A.GraphObjective(SPRING, edges=([0], [1]), node_body=WELL)
    rec["code"] = {"chained_rosenbrock": chain.info(), "path_graph": path_obj.info(), "lattice": lat_obj.info()}

    # ---- the edge lists, on the device
    idx = torch.arange(n, dtype=torch.int32, device=dev).view(rows, cols)
    lat_i = torch.cat([idx[:, :-1].reshape(-1), idx[:-1, :].reshape(-1)]).contiguous()
    lat_j = torch.cat([idx[:, 1:].reshape(-1), idx[1:, :].reshape(-1)]).contiguous()
    perm = torch.randperm(n, generator=torch.Generator(device=dev).manual_seed(7), device=dev).to(torch.int32)
    prm_i, prm_j = perm[lat_i.long()].contiguous(), perm[lat_j.long()].contiguous()
    path_i = torch.arange(n - 1, dtype=torch.int32, device=dev)
    path_j = path_i + 1
    del idx
    torch.cuda.synchronize()
    edges = {"path_graph": (path_i, path_j), "lattice_natural": (lat_i, lat_j), "lattice_permuted": (prm_i, prm_j)}

    h = C.c_void_p()
    L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))

    def vec(v):
        return L.device_tensor(core.lbfgsx_vec(h, v), (n,), np.float64, 0)

    gen = torch.Generator(device=dev).manual_seed(1)
    vec(L.VEC_X).copy_(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
    vec(L.VEC_D).copy_(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
    torch.cuda.synchronize()
    L.check(core.lbfgsx_ls_begin(h))
    fx, dg = C.c_double(), C.c_double()
    cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)
    fn = lattice_torch(torch, lat_i, lat_j)
    build_ms = {}

    def setup(leg):
        oid = C.c_int(-1)
        if leg == "built_in":
            return L.OBJ_EXT_ROSENBROCK
        if leg == "torch_callable":
            return -1
        if leg == "chained_rosenbrock":
            L.check(core.lbfgsx_objective_bind(h, chain.compile(), None, None, C.byref(oid)))
            return oid.value
        ei, ej = edges[leg]
        obj = path_obj if leg == "path_graph" else lat_obj
        p = [C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_int32)) for t in (ei, ej)]
        t0 = time.perf_counter()
        L.check(core.lbfgsx_objective_bind_graph(h, obj.compile(), ei.numel(), p[0], p[1], 1, None, C.byref(cs), C.byref(oid)))
        build_ms.setdefault(leg, []).append((time.perf_counter() - t0) * 1e3)
        return oid.value

    def one_call(leg, oid):
        t0 = time.perf_counter()
        if leg == "torch_callable":
            L.check(core.lbfgsx_trial_point(h, 0.37))
            L.check(core.lbfgsx_sync(h))
            fn(vec(L.VEC_XT), vec(L.VEC_GT))
            torch.cuda.synchronize()
            L.check(core.lbfgsx_trial_dg(h, C.byref(dg)))
        else:
            L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
        return (time.perf_counter() - t0) * 1e3

    if args.counter_run:
        oid = setup(args.counter_run)
        for _ in range(4):
            one_call(args.counter_run, oid)
        core.lbfgsx_destroy(h)
        return

    legs = ["built_in", "chained_rosenbrock", "path_graph", "lattice_natural", "lattice_permuted", "torch_callable"]
    times = {leg: [] for leg in legs}
    for rnd in range(args.rounds):  # round 0 warms every leg up
        for leg in legs:
            oid = setup(leg)
            ms = [one_call(leg, oid) for _ in range(args.calls)]
            if rnd:
                times[leg] += ms[2:]
    core.lbfgsx_destroy(h)
    med = {k: float(np.median(v)) for k, v in times.items()}
    E = {k: int(v[0].numel()) for k, v in edges.items()}
    rec["trial"] = {"n": n, "lattice": [rows, cols], "edges": E, "dtype": "f64", "step": 0.37,
                    "timed_calls_per_leg": len(times["built_in"]), "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "over_built_in": {k: med[k] / med["built_in"] for k in med},
                    "torch_callable_over": {k: med["torch_callable"] / med[k] for k in med},
                    "model_bytes": {k: 4 * n * 8 + (n + 1) * 4 + 2 * E[k] * 8 + 2 * 2 * E[k] * 8 for k in E}}
    rec["build"] = {"median_ms": {k: float(np.median(v)) for k, v in build_ms.items()},
                    "all_ms": build_ms, "edges_on_device": True}
    rec["counters"] = None  # FETCH_SIZE / WRITE_SIZE of one k_graph_trial launch: a run of its own (--counter-run), not taken here
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"median_ms": med, "over_built_in": rec["trial"]["over_built_in"], "build_ms": rec["build"]["median_ms"],
                      "vgprs": {k: v["vgprs"] for k, v in rec["code"].items()},
                      "scratch": {k: v["scratch_bytes"] for k, v in rec["code"].items()}}))


if __name__ == "__main__":
    main()
