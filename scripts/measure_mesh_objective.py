#!/usr/bin/env python3
"""What a mesh objective (lbfgspp_amd.MeshObjective) costs, in one process on one device (profiles/mesh_objective.json).

  trial   n ~ 1e8 f64: the time of ONE trial evaluation (lbfgsx_trial; wall clock around the synchronous call, median of 20
          timed calls after warm-up, the tile order alternating) for (a) springs plus a double well on the 10000 x 10000
          lattice through k_graph_trial and (b) the same lattice as a K = 2, D = 1 mesh in the same context -- the same work,
          so (b) / (a) is the number of interest; (c) the triangulated 7071 x 7071 lattice, K = 3, D = 2, the solver tests'
          energy; (d) the tetrahedralised 322^3 lattice, K = 4, D = 3, a volume penalty.
  build   the time of lbfgsx_objective_bind_mesh from a device-resident table.
  code    VGPRs and scratch of the compiled bodies, from the code object.

Every GPU step runs under a time limit of its own (--limit seconds): SIGALRM ends the process, and nothing more is started.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SPRING = """const T d = x[0] - x[1];
g[0] = d;
g[1] = T(0) - d;
return T(0.5) * (d * d);"""
WELL = """const T u = x[0] * x[0] - T(1);
const T k = c[0] * T(0.25);
g[0] = (T(4) * k) * (u * x[0]);
return k * (u * u);"""
C0 = 4.0


class step:
    """a GPU step under its own time limit: SIGALRM's default action ends the process, inside a library call too"""
    limit = 120

    def __init__(self, what):
        self.what = what

    def __enter__(self):
        sys.stderr.write("step: %s (limit %d s)\n" % (self.what, step.limit))
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(step.limit)

    def __exit__(self, *exc):
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_objective.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="scales every lattice's side (1.0: n ~ 1e8)")
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    step.limit = args.limit
    import torch

    import lbfgspp_amd as A
    import mesh_ref as MR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_mesh_objective.py needs a GPU")
    dev = "cuda:0"
    side2, side3, side4 = (max(4, int(round(v * args.scale))) for v in (10000, 7071, 322))
    rec = {"device": torch.cuda.get_device_name(0)}
    graph = A.GraphObjective(SPRING, edges=([0], [1]), node_body=WELL)
    objs = {"lattice_mesh": A.MeshObjective(SPRING, [[0, 1]], 1, node_body=WELL),
            "triangles": A.MeshObjective(MR.TRIANGLE, [[0, 1, 2]], 2, node_body=MR.TIE_NODE),
            "tetrahedra": A.MeshObjective(MR.VOLUME, [[0, 1, 2, 3]], 3)}
    rec["code"] = dict({"lattice_graph": graph.info()}, **{k: v.info() for k, v in objs.items()})
    fx, dg = C.c_double(), C.c_double()
    times, build_ms, shapes = {}, {}, {}

    def timed(h, oid, leg):
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
            ms.append((time.perf_counter() - t0) * 1e3)
        times[leg] = ms[4:]  # the first calls warm up; both tile orders are among the rest

    def context(n, rest, amp):
        h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))
        gen = torch.Generator(device=dev).manual_seed(1)
        x = L.device_tensor(core.lbfgsx_vec(h, L.VEC_X), (n,), np.float64, 0)
        x.copy_(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
        x.mul_(amp)
        if rest is not None:
            x.add_(rest)
        L.device_tensor(core.lbfgsx_vec(h, L.VEC_D), (n,), np.float64, 0).copy_(
            torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(h))
        return h

    def bind_mesh(h, leg, el, ptrs, cs):
        oid = C.c_int(-1)
        t0 = time.perf_counter()
        L.check(core.lbfgsx_objective_bind_mesh(h, objs[leg].compile(), el.shape[0], C.c_void_p(el.data_ptr()), 1, ptrs, cs, C.byref(oid)))
        build_ms[leg] = (time.perf_counter() - t0) * 1e3
        shapes[leg] = {"N": int(el.max().item()) + 1, "E": int(el.shape[0]), "K": int(el.shape[1])}
        return oid.value

    # ---- (a), (b): the 4-neighbour lattice, as a graph and as a K = 2, D = 1 mesh
    with step("lattice: set-up"):
        n = side2 * side2
        idx = torch.arange(n, dtype=torch.int32, device=dev).view(side2, side2)
        ei = torch.cat([idx[:, :-1].reshape(-1), idx[:-1, :].reshape(-1)]).contiguous()
        ej = torch.cat([idx[:, 1:].reshape(-1), idx[1:, :].reshape(-1)]).contiguous()
        el = torch.stack([ei, ej], 1).contiguous()
        del idx
        h = context(n, None, 1.0)
        cs = (C.c_double * 8)(C0, 0, 0, 0, 0, 0, 0, 0)
    with step("lattice as a graph"):
        oid = C.c_int(-1)
        p = [C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_int32)) for t in (ei, ej)]
        t0 = time.perf_counter()
        L.check(core.lbfgsx_objective_bind_graph(h, graph.compile(), ei.numel(), p[0], p[1], 1, None, C.byref(cs), C.byref(oid)))
        build_ms["lattice_graph"] = (time.perf_counter() - t0) * 1e3
        timed(h, oid.value, "lattice_graph")
    with step("lattice as a mesh"):
        timed(h, bind_mesh(h, "lattice_mesh", el, None, C.byref(cs)), "lattice_mesh")
        shapes["lattice_mesh"]["D"] = 1
    with step("lattice: the graph again"):  # the order of the two legs is not what separates them
        L.check(core.lbfgsx_objective_bind_graph(h, graph.compile(), ei.numel(), p[0], p[1], 1, None, C.byref(cs), C.byref(oid)))
        timed(h, oid.value, "lattice_graph_again")
        core.lbfgsx_destroy(h)
        del ei, ej, el

    # ---- (c): triangles, D = 2
    with step("triangles: set-up"):
        ny = nx = side3
        N = ny * nx
        idx = torch.arange(N, dtype=torch.int32, device=dev).view(ny, nx)
        i = idx[:-1, :-1].reshape(-1)
        el = torch.stack([torch.stack([i, i + 1, i + nx + 1], 1), torch.stack([i, i + nx + 1, i + nx], 1)], 1).view(-1, 3).contiguous()
        rest = torch.stack([(idx % nx).double(), (idx // nx).double()], -1).view(-1).contiguous()
        E = el.shape[0]
        odd = (torch.arange(E, device=dev) & 1).double()
        l0, l1, l2 = 1.0 + odd, 1.0 + 0.0 * odd, 2.0 - odd  # (i, i+1, i+nx+1): 1, 1, 2; (i, i+nx+1, i+nx): 2, 1, 1
        del idx, i, odd
        h = context(2 * N, rest, 0.1)
        ptrs = (C.c_void_p * 4)(l0.data_ptr(), l1.data_ptr(), l2.data_ptr(), rest.data_ptr())
        cs = (C.c_double * 8)(2.0, 1.0, 4.0, 0, 0, 0, 0, 0)
    with step("triangles"):
        timed(h, bind_mesh(h, "triangles", el, C.byref(ptrs), C.byref(cs)), "triangles")
        shapes["triangles"]["D"] = 2
        core.lbfgsx_destroy(h)
        del el, rest, l0, l1, l2

    # ---- (d): tetrahedra, D = 3
    with step("tetrahedra: set-up"):
        s = side4
        N = s ** 3
        idx = torch.arange(N, dtype=torch.int32, device=dev).view(s, s, s)
        i = idx[:-1, :-1, :-1].reshape(-1)
        stepv = (1, s, s * s)
        tets = []
        for perm in itertools.permutations(range(3)):
            a, b, c3 = (stepv[q] for q in perm)
            even = perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1))
            cols = [i, i + a, i + a + b, i + a + b + c3] if even else [i, i + a + b, i + a, i + a + b + c3]
            tets.append(torch.stack(cols, 1))
        el = torch.stack(tets, 1).view(-1, 4).contiguous()
        rest = torch.stack([(idx % s).double(), ((idx // s) % s).double(), (idx // (s * s)).double()], -1).view(-1).contiguous()
        vol = torch.ones(el.shape[0], dtype=torch.float64, device=dev)
        del idx, i, tets
        h = context(3 * N, rest, 0.1)
        ptrs = (C.c_void_p * 4)(vol.data_ptr(), None, None, None)
    with step("tetrahedra"):
        timed(h, bind_mesh(h, "tetrahedra", el, C.byref(ptrs), None), "tetrahedra")
        shapes["tetrahedra"]["D"] = 3
        core.lbfgsx_destroy(h)

    med = {k: float(np.median(v)) for k, v in times.items()}

    def model(s):  # the byte model of one trial launch (include/lbfgsx.h)
        K, D, KE = s["K"], s["D"], s["K"] * s["E"]
        return 4 * s["N"] * D * 8 + (s["N"] + 1) * 4 + KE * 4 * K + 2 * KE * (K - 1) * D * 8
    rec["trial"] = {"dtype": "f64", "step": 0.37, "timed_calls_per_leg": args.calls - 4, "shapes": shapes, "median_ms": med,
                    "min_ms": {k: float(np.min(v)) for k, v in times.items()},
                    "mesh_over_graph": med["lattice_mesh"] / min(med["lattice_graph"], med["lattice_graph_again"]),
                    "model_bytes": {k: model(v) for k, v in shapes.items()},
                    "model_gbps": {k: model(v) / med[k] / 1e6 for k, v in shapes.items()}}
    rec["build"] = {"ms": build_ms, "elements_on_device": True}
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"median_ms": med, "mesh_over_graph": rec["trial"]["mesh_over_graph"], "build_ms": build_ms,
                      "model_gbps": rec["trial"]["model_gbps"], "vgprs": {k: v["vgprs"] for k, v in rec["code"].items()}}))


if __name__ == "__main__":
    main()
