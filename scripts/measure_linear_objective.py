#!/usr/bin/env python3
"""What a linear-model objective (lbfgspp_amd.LinearObjective) costs, in one process on one device
(profiles/linear_objective.json).  Recorded, not gated.

  trial   f64, logistic loss + ridge over a random sparse R x n matrix with R = n: the time of ONE trial evaluation
          (lbfgsx_trial: row pass, long-column launch if any, column pass; wall clock around the synchronous call, median of
          the timed calls after warm-up, the tile order alternating) for n = 1e6 and 1e7, about 10 and about 100 entries per
          row (columns uniform at random: no locality), each without and with a dense intercept column (column 0, a long
          column), beside the torch callable of the same objective (torch.sparse_csr products with A and its stored
          transpose, the function a DeviceObjective would call) on the same device in the same process.
  build   the time of lbfgsx_objective_bind_linear from device-resident arrays.
  code    VGPRs and scratch of the compiled bodies, from the code object.

A case whose entries exceed --max-nnz is not run and is listed under "skipped".  Every GPU step runs under a time limit of
its own (--limit seconds): SIGALRM ends the process, and nothing more is started.
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

LAM = 1e-3


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_objective.json"))
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--per-row", default="10,100")
    ap.add_argument("--max-nnz", type=float, default=1.5e9)
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    step.limit = args.limit
    import torch

    import lbfgspp_amd as A
    import linear_ref as LR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_linear_objective.py needs a GPU")
    dev = "cuda:0"
    obj = A.LinearObjective(LR.LOGISTIC, ([0, 1], [0], [1.0]), 1, coord_body=LR.RIDGE)
    rec = {"device": torch.cuda.get_device_name(0), "code": obj.info(), "objective": "logistic + ridge", "dtype": "f64",
           "cases": [], "skipped": []}
    fx, dg = C.c_double(), C.c_double()
    for n in (int(v) for v in args.sizes.split(",")):
        for per in (int(v) for v in args.per_row.split(",")):
            for intercept in (False, True):
                R = n
                width = per + (1 if intercept else 0)
                nnz = R * width
                case = {"n": n, "R": R, "per_row": per, "intercept": intercept, "nnz": nnz}
                if nnz > args.max_nnz:
                    rec["skipped"].append(case)
                    continue
                with step("n %d per %d intercept %s: set-up" % (n, per, intercept)):
                    gen = torch.Generator(device=dev).manual_seed(n + per)
                    col = torch.randint(1 if intercept else 0, n, (R, width), dtype=torch.int32, device=dev, generator=gen)
                    val = torch.randn(R, width, dtype=torch.float64, device=dev, generator=gen) / float(np.sqrt(width))
                    if intercept:
                        col[:, 0] = 0
                        val[:, 0] = 1.0
                    col, val = col.view(-1).contiguous(), val.view(-1).contiguous()
                    rowptr = (torch.arange(R + 1, dtype=torch.int64, device=dev) * width).to(torch.int32)
                    y = 1.0 - 2.0 * (torch.rand(R, dtype=torch.float64, device=dev, generator=gen) < 0.5).to(torch.float64)
                    assert y.dtype == torch.float64 and y.numel() == R and val.dtype == torch.float64  # what the kernels read
                    h = C.c_void_p()
                    L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))
                    x = L.device_tensor(core.lbfgsx_vec(h, L.VEC_X), (n,), np.float64, 0)
                    d = L.device_tensor(core.lbfgsx_vec(h, L.VEC_D), (n,), np.float64, 0)
                    x.copy_(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
                    d.copy_(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
                    torch.cuda.synchronize()
                    L.check(core.lbfgsx_ls_begin(h))
                with step("bind"):
                    ptrs = (C.c_void_p * 4)(y.data_ptr(), None, None, None)
                    cs = (C.c_double * 8)(LAM, 0, 0, 0, 0, 0, 0, 0)
                    oid = C.c_int(-1)
                    t0 = time.perf_counter()
                    L.check(core.lbfgsx_objective_bind_linear(h, obj.compile(), R, nnz, rowptr.data_ptr(), col.data_ptr(),
                                                              val.data_ptr(), 1, 0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
                    case["bind_ms"] = (time.perf_counter() - t0) * 1e3
                    info = (C.c_int64 * 8)()
                    L.check(core.lbfgsx_objective_linear_topology(h, C.byref(info), None, None, None, None, None, None))
                    case.update(lanes=int(info[2]), chunk=int(info[3]), long_columns=int(info[4]), chunks=int(info[5]))
                with step("trial"):
                    ms = []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        L.check(core.lbfgsx_trial(h, oid.value, 0.37, C.byref(fx), C.byref(dg)))
                        ms.append((time.perf_counter() - t0) * 1e3)
                    ms = ms[4:]  # the first calls warm up; both tile orders are among the rest
                    case["trial_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms))}
                    case["f"] = fx.value
                    # the byte model of one trial (include/lbfgsx.h): the trial kernel's four streams, then linear_model_add
                    model = 4 * n * 8 + n * 8 + (R + 1) * 4 + (n + 1) * 4 + 2 * nnz * 4 + 2 * nnz * 8 + 3 * nnz * 8 + 4 * R * 8 \
                        + 2 * case["chunks"] * 8
                    case["model_bytes"] = model
                    case["model_gbps"] = model / case["trial_ms"]["median"] / 1e6
                try:
                    with step("torch callable"):
                        a = torch.sparse_csr_tensor(rowptr, col, val, size=(R, n))
                        at = a.t().to_sparse_csr()
                        xt = x + 0.37 * d

                        def fn(xv, grad):
                            m = y * (a @ xv)
                            w = -y * torch.sigmoid(-m)
                            grad.copy_(at @ w)
                            grad.add_(xv, alpha=LAM)
                            return float(torch.nn.functional.softplus(-m).sum() + 0.5 * LAM * (xv @ xv))
                        g = torch.empty_like(xt)
                        ms = []
                        for _ in range(args.calls):
                            t0 = time.perf_counter()
                            ft = fn(xt, g)
                            ms.append((time.perf_counter() - t0) * 1e3)
                        ms = ms[4:]
                        case["torch_ms"] = {"median": float(np.median(ms)), "min": float(np.min(ms))}
                        case["torch_f"] = ft
                        case["torch_over_fused"] = case["torch_ms"]["median"] / case["trial_ms"]["median"]
                        gt = L.device_tensor(core.lbfgsx_vec(h, L.VEC_GT), (n,), np.float64, 0)
                        case["max_abs_gradient_difference"] = float((gt - g).abs().max())
                        del a, at, g, xt
                except RuntimeError as e:  # torch could not form or multiply the CSR matrix: recorded, the rest goes on
                    if "HIP" in str(e) or "illegal" in str(e):  # a device error is not: nothing more is started
                        raise
                    case["torch_error"] = str(e)[:300]
                core.lbfgsx_destroy(h)
                del col, val, rowptr, y
                torch.cuda.empty_cache()
                rec["cases"].append(case)
                sys.stderr.write(json.dumps(case) + "\n")
                json.dump(rec, open(args.out, "w"))
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"cases": [{k: c.get(k) for k in ("n", "per_row", "intercept", "lanes", "bind_ms", "trial_ms", "torch_ms",
                                                       "torch_over_fused", "model_gbps")} for c in rec["cases"]],
                      "skipped": rec["skipped"], "vgprs": rec["code"]["vgprs"]}))


if __name__ == "__main__":
    main()
