#!/usr/bin/env python3
"""What a graph-regularised linear-model objective (lbfgspp_amd.GraphLinearObjective) costs, in one process on one device
(profiles/graph_linear_objective.json).  Recorded, not gated.

  trial   f64, logistic loss + ridge + springs: a random sparse R x n matrix with R = n and --per-row entries per row (columns
          uniform at random: no locality), and the side x side lattice with natural labels as the graph (n = side^2, edges to the
          right and to the lower neighbour).  The time of ONE trial evaluation (lbfgsx_trial: row pass, column pass; wall clock
          around the synchronous call, median of the timed calls after 4 warm-up calls, as many calls as fill --window seconds, the tile order alternating), beside, in the same
          loop so that the three alternate on one device,
            (a) the SUM of a LinearObjective trial on the same matrix (logistic + ridge) and a GraphObjective trial on the same
                graph (springs), each on a context of its own: the existing forms, which stream x, xp, d and g twice;
            (b) the torch callable of the same objective (torch.sparse_csr products, index_select and index_add_), the function
                a DeviceObjective would call.
  build   the time of lbfgsx_objective_bind_linear_graph from device-resident arrays.
  code    VGPRs and scratch of the compiled bodies of the three forms, from the code objects.

Every GPU step runs under a time limit of its own (--limit seconds): SIGALRM ends the process, and nothing more is started.
"""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LAM, KAPPA = 1e-3, 0.05
# springs with one weight c[1] for every edge
SPRINGS = """const T d = x[0] - x[1];
const T w = c[1] * d;
g[0] = w;
g[1] = T(0) - w;
return T(0.5) * (w * d);"""


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_linear_objective.json"))
    ap.add_argument("--sides", default="1000,3162")
    ap.add_argument("--per-row", type=int, default=10)
    ap.add_argument("--calls", type=int, default=16, help="rounds of the three forms at least, the first 4 of them warm-up")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed fused trials at least (a short window times the clock)")
    ap.add_argument("--max-calls", type=int, default=2000)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    step.limit = args.limit
    import torch

    import lbfgspp_amd as A
    import linear_ref as LR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_graph_linear_objective.py needs a GPU")
    dev = "cuda:0"
    one, e1 = ([0, 2], [0, 1], [1.0, 1.0]), ([0], [1])
    fused = A.GraphLinearObjective(LR.LOGISTIC, one, e1, SPRINGS, n=2, coord_body=LR.RIDGE)
    lin = A.LinearObjective(LR.LOGISTIC, one, 2, coord_body=LR.RIDGE)
    gra = A.GraphObjective(SPRINGS, e1)
    rec = {"device": torch.cuda.get_device_name(0), "objective": "logistic + ridge + springs", "dtype": "f64",
           "code": {"linear_graph": fused.info(), "linear": lin.info(), "graph": gra.info()}, "cases": []}
    fx, dg = C.c_double(), C.c_double()
    for side in (int(v) for v in args.sides.split(",")):
        n = R = side * side
        per = args.per_row
        nnz = R * per
        case = {"side": side, "n": n, "R": R, "per_row": per, "nnz": nnz}
        with step("side %d: set-up" % side):
            gen = torch.Generator(device=dev).manual_seed(n + per)
            col = torch.randint(0, n, (R * per,), dtype=torch.int32, device=dev, generator=gen)
            val = torch.randn(R * per, dtype=torch.float64, device=dev, generator=gen) / float(np.sqrt(per))
            rowptr = (torch.arange(R + 1, dtype=torch.int64, device=dev) * per).to(torch.int32)
            y = 1.0 - 2.0 * (torch.rand(R, dtype=torch.float64, device=dev, generator=gen) < 0.5).to(torch.float64)
            node = torch.arange(n, dtype=torch.int32, device=dev)
            right, down = node[(node % side) != side - 1], node[: n - side]
            ei = torch.cat([right, down]).contiguous()
            ej = torch.cat([right + 1, down + side]).contiguous()
            E = case["E"] = int(ei.numel())
            x0 = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
            d0 = torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5
            ctx = {}
            for name in ("linear_graph", "linear", "graph"):
                h = C.c_void_p()
                L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))
                L.device_tensor(core.lbfgsx_vec(h, L.VEC_X), (n,), np.float64, 0).copy_(x0)
                L.device_tensor(core.lbfgsx_vec(h, L.VEC_D), (n,), np.float64, 0).copy_(d0)
                ctx[name] = h
            torch.cuda.synchronize()
            for h in ctx.values():
                L.check(core.lbfgsx_ls_begin(h))
        with step("bind"):
            ptrs = (C.c_void_p * 4)(y.data_ptr(), None, None, None)
            cs = (C.c_double * 8)(LAM, KAPPA, 0, 0, 0, 0, 0, 0)
            oid = {k: C.c_int(-1) for k in ctx}
            t0 = time.perf_counter()
            L.check(core.lbfgsx_objective_bind_linear_graph(ctx["linear_graph"], fused.compile(), R, nnz, rowptr.data_ptr(),
                                                            col.data_ptr(), val.data_ptr(), 1, 0, E, ei.data_ptr(), ej.data_ptr(), 1,
                                                            C.byref(ptrs), C.byref(cs), C.byref(oid["linear_graph"])))
            case["bind_ms"] = (time.perf_counter() - t0) * 1e3
            L.check(core.lbfgsx_objective_bind_linear(ctx["linear"], lin.compile(), R, nnz, rowptr.data_ptr(), col.data_ptr(),
                                                      val.data_ptr(), 1, 0, C.byref(ptrs), C.byref(cs), C.byref(oid["linear"])))
            L.check(core.lbfgsx_objective_bind_graph(ctx["graph"], gra.compile(), E, C.cast(ei.data_ptr(), C.POINTER(C.c_int32)),
                                                     C.cast(ej.data_ptr(), C.POINTER(C.c_int32)), 1, C.byref(ptrs), C.byref(cs),
                                                     C.byref(oid["graph"])))
            info = (C.c_int64 * 8)()
            L.check(core.lbfgsx_objective_linear_topology(ctx["linear_graph"], C.byref(info), None, None, None, None, None, None))
            case.update(lanes=int(info[2]), long_columns=int(info[4]))
        with step("trials, the three forms alternating"):
            ms = {k: [] for k in ctx}
            f = {}
            calls = args.calls
            done = 0
            while done < calls:
                for k, h in ctx.items():
                    t0 = time.perf_counter()
                    L.check(core.lbfgsx_trial(h, oid[k].value, 0.37, C.byref(fx), C.byref(dg)))
                    ms[k].append((time.perf_counter() - t0) * 1e3)
                    f[k] = fx.value
                done += 1
                if done == 4:  # warmed up: as many rounds as make the fused form's timed window --window seconds, at least --calls
                    calls = max(calls, 4 + min(args.max_calls, int(args.window * 1e3 / ms["linear_graph"][-1]) + 1))
            ms = {k: v[4:] for k, v in ms.items()}  # the first calls warm up; both tile orders are among the rest
            case["timed_calls"] = calls - 4
            case["trial_ms"] = {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in ms.items()}
            sep = [a + b for a, b in zip(ms["linear"], ms["graph"])]
            case["separate_ms"] = {"median": float(np.median(sep)), "min": float(np.min(sep))}
            case["fused_over_separate"] = case["trial_ms"]["linear_graph"]["median"] / case["separate_ms"]["median"]
            case["f"] = f  # the fused f is the linear form's (logistic + ridge) plus the graph form's (springs)
            case["f_difference_to_separate"] = f["linear_graph"] - (f["linear"] + f["graph"])
            gt = {k: L.device_tensor(core.lbfgsx_vec(h, L.VEC_GT), (n,), np.float64, 0) for k, h in ctx.items()}
            xt = x0 + 0.37 * d0
            # the separate forms' gradients add up to the fused one but for the order of the sum
            case["max_abs_gradient_difference_to_separate"] = float((gt["linear_graph"] - (gt["linear"] + gt["graph"])).abs().max())
            # the byte model of one fused trial (include/lbfgsx.h): the trial kernel's four streams and the data array, the linear
            # form's terms, the graph form's list terms
            model = 4 * n * 8 + n * 8 + (R + 1) * 4 + (n + 1) * 4 + 2 * nnz * 4 + 2 * nnz * 8 + 3 * nnz * 8 + 4 * R * 8 \
                + (n + 1) * 4 + 2 * E * 8 + 2 * E * 8 * 2
            case["model_bytes"] = model
            case["model_gbps"] = model / case["trial_ms"]["linear_graph"]["median"] / 1e6
        try:
            with step("torch callable"):
                a = torch.sparse_csr_tensor(rowptr, col, val, size=(R, n))
                at = a.t().to_sparse_csr()
                li, lj = ei.long(), ej.long()

                def fn(xv, grad):
                    m = y * (a @ xv)
                    w = -y * torch.sigmoid(-m)
                    grad.copy_(at @ w)
                    grad.add_(xv, alpha=LAM)
                    dd = xv.index_select(0, li) - xv.index_select(0, lj)
                    grad.index_add_(0, li, dd, alpha=KAPPA)
                    grad.index_add_(0, lj, dd, alpha=-KAPPA)
                    return float(torch.nn.functional.softplus(-m).sum() + 0.5 * LAM * (xv @ xv) + 0.5 * KAPPA * (dd @ dd))
                g = torch.empty_like(xt)
                tms = []
                calls = args.calls
                while len(tms) < calls:
                    t0 = time.perf_counter()
                    ft = fn(xt, g)
                    tms.append((time.perf_counter() - t0) * 1e3)
                    if len(tms) == 4:  # the same window as the fused form's
                        calls = max(calls, 4 + min(args.max_calls, int(args.window * 1e3 / tms[-1]) + 1))
                tms = tms[4:]
                case["torch_ms"] = {"median": float(np.median(tms)), "min": float(np.min(tms))}
                case["torch_f"] = ft
                case["torch_over_fused"] = case["torch_ms"]["median"] / case["trial_ms"]["linear_graph"]["median"]
                case["max_abs_gradient_difference_to_torch"] = float((gt["linear_graph"] - g).abs().max())
                del a, at, g, li, lj
        except RuntimeError as e:  # torch could not form or multiply the CSR matrix: recorded, the rest goes on
            if "HIP" in str(e) or "illegal" in str(e):  # a device error is not: nothing more is started
                raise
            case["torch_error"] = str(e)[:300]
        del gt
        for h in ctx.values():
            core.lbfgsx_destroy(h)
        del col, val, rowptr, y, ei, ej, x0, d0, xt
        torch.cuda.empty_cache()
        rec["cases"].append(case)
        sys.stderr.write(json.dumps(case) + "\n")
        json.dump(rec, open(args.out, "w"), indent=1)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps({"cases": [{k: c.get(k) for k in ("n", "E", "per_row", "lanes", "bind_ms", "trial_ms", "separate_ms",
                                                       "fused_over_separate", "torch_ms", "torch_over_fused", "model_gbps")}
                                for c in rec["cases"]],
                      "vgprs": {k: v["vgprs"] for k, v in rec["code"].items()}}))


if __name__ == "__main__":
    main()
