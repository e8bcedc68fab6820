#!/usr/bin/env python3
"""What a dense linear-model objective (lbfgspp_amd.DenseLinearObjective) costs, in one process on one device
(profiles/dense_objective.json).  Recorded, not gated.  It follows scripts/measure_multilinear_objective.py.

  f64, ONE trial evaluation (lbfgsx_trial: row pass, partial pass, column pass; wall clock around the synchronous call, median
  of 12 timed calls after 4 warm-up calls, the tile order alternating), logistic + ridge at D = 1 and softmax + ridge at
  D = 10, on a random dense matrix held in device memory and used in place, for the shapes
      R = 1e6, F = 1e3;    R = 1e5, F = 1e4;    R = 1e6, F = 64 (the small-F slot mapping of the partial pass).
  Beside it, per shape and objective:
    (a) the torch callable of the same objective with a dense A @ W and A.T @ G (the function a DeviceObjective would call);
    (b) the sparse form (LinearObjective / MultiLinearObjective) on the same matrix as CSR with every entry stored, where
        --sparse-limit allows its nnz (the CSR copy, its transpose and the bind's sort take about 40 bytes per entry);
    (c) the time of streaming 2 R F 8 bytes at the device's stream-copy rate, measured here by a device-to-device copy of a
        2 GiB buffer (read + write counted), and the fraction of that rate the evaluation reaches on its 2 R F 8 bytes of A.
  The split between the row pass and the partial pass comes from a kernel trace taken in a run of its own:
      rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/measure_dense_objective.py --shapes 0 --dense-only --out <file>
  code: VGPRs and scratch of the compiled bodies, from the code object.

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

LAM = 1e-3
SHAPES = ((1000000, 1000), (100000, 10000), (1000000, 64))
LOGISTIC = """
const T m = p0[r] * z[0];
const T e = exp(m > T(0) ? T(0) - m : m);
const T s = (m > T(0) ? e : T(1)) / (T(1) + e);
dz[0] = T(0) - p0[r] * s;
return (m > T(0) ? T(0) : T(0) - m) + log1p(e);"""
SOFTMAX = """
T m = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    m = z[k] > m ? z[k] : m;
T e[D];
T s = T(0);
#pragma unroll
for (int k = 0; k < D; k++)
{
    e[k] = exp(z[k] - m);
    s = s + e[k];
}
const int y = int(p0[r]);
T zy = z[0];
#pragma unroll
for (int k = 1; k < D; k++)
    zy = k == y ? z[k] : zy;
#pragma unroll
for (int k = 0; k < D; k++)
    dz[k] = e[k] / s - (k == y ? T(1) : T(0));
return (log(s) + m) - zy;"""


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_objective.json"))
    ap.add_argument("--shapes", default="0,1,2")
    ap.add_argument("--dense-only", action="store_true")
    ap.add_argument("--sparse-limit", type=int, default=100000000, help="the largest nnz given to the sparse form")
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--limit", type=int, default=120)
    args = ap.parse_args()
    step.limit = args.limit
    import torch

    import lbfgspp_amd as A
    import linear_ref as LR
    import multilinear_ref as MR
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    if core.lbfgsx_device_count() < 1:
        sys.exit("measure_dense_objective.py needs a GPU")
    dev = "cuda:0"
    one_d, one_s = np.ones((1, 1)), ([0, 1], [0], [1.0])
    objs = {1: A.DenseLinearObjective(LOGISTIC, one_d, 1, coord_body=LR.RIDGE),
            10: A.DenseLinearObjective(SOFTMAX, one_d, 10, coord_body=LR.RIDGE)}
    sparse = {1: A.MultiLinearObjective(LOGISTIC, one_s, 1, 1, coord_body=LR.RIDGE),
              10: A.MultiLinearObjective(SOFTMAX, one_s, 1, 10, coord_body=LR.RIDGE)}
    rec = {"device": torch.cuda.get_device_name(0), "dtype": "f64", "timed_calls": args.calls - 4,
           "code": {"logistic D=1": objs[1].info(), "softmax D=10": objs[10].info()}, "cases": []}
    fx, dg = C.c_double(), C.c_double()
    with step("stream copy"):
        src = torch.zeros(1 << 28, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        ms = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        rec["stream_copy_gbps"] = 2 * src.numel() * 8 / float(np.median(ms[2:])) / 1e6
        del src, dst
        torch.cuda.empty_cache()

    def context(n, gen):
        h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))
        x = L.device_tensor(core.lbfgsx_vec(h, L.VEC_X), (n,), np.float64, 0)
        d = L.device_tensor(core.lbfgsx_vec(h, L.VEC_D), (n,), np.float64, 0)
        x.copy_((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5) * 0.1)
        d.copy_((torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5) * 0.1)
        keep = (x.clone(), d.clone())
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(h))
        return h, keep[0], keep[1]

    def trials(h, oid, calls):
        ms = []
        for _ in range(calls):
            t0 = time.perf_counter()
            L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
            ms.append((time.perf_counter() - t0) * 1e3)
        return {"median": float(np.median(ms[4:])), "min": float(np.min(ms[4:]))}

    for k in (int(v) for v in args.shapes.split(",")):
        R, F = SHAPES[k]
        with step("R %d F %d: the matrix" % (R, F)):
            gen = torch.Generator(device=dev).manual_seed(11 + k)
            a = torch.randn(R, F, dtype=torch.float64, device=dev, generator=gen) / float(np.sqrt(F))
            labels = torch.randint(0, 10, (R,), device=dev, generator=gen)
            torch.cuda.synchronize()
        for D in (1, 10):
            n = F * D
            case = {"R": R, "F": F, "D": D, "n": n, "objective": "logistic + ridge" if D == 1 else "softmax + ridge",
                    "A_bytes": R * F * 8}
            y = (1.0 - 2.0 * (labels % 2).to(torch.float64)) if D == 1 else labels.to(torch.float64)
            ptrs = (C.c_void_p * 4)(y.data_ptr(), None, None, None)
            cs = (C.c_double * 8)(LAM, 0, 0, 0, 0, 0, 0, 0)
            with step("dense D %d" % D):
                h, x, d = context(n, gen)
                oid = C.c_int(-1)
                t0 = time.perf_counter()
                L.check(core.lbfgsx_objective_bind_dense(h, objs[D].compile(), R, a.data_ptr(), F, 1, 0, C.byref(ptrs), C.byref(cs),
                                                         C.byref(oid)))
                case["bind_ms"] = (time.perf_counter() - t0) * 1e3
                info = (C.c_int64 * 8)()
                L.check(core.lbfgsx_objective_dense_info(h, C.byref(info)))
                case.update(lanes=int(info[3]), chunk=int(info[4]), chunks=int(info[5]), context_owns_copy=int(info[7]))
                case["trial_ms"] = trials(h, oid.value, args.calls)
                case["f"] = fx.value
                s = 8
                model = 4 * n * s + n * s + 2 * R * F * s + 2 * n * s + 2 * R * D * s + 2 * R * s + 2 * case["chunks"] * n * s
                case["model_bytes"] = model
                case["model_gbps"] = model / case["trial_ms"]["median"] / 1e6
                case["stream_2RF_ms"] = 2 * R * F * 8 / rec["stream_copy_gbps"] / 1e6
                case["fraction_of_stream_copy"] = case["stream_2RF_ms"] / case["trial_ms"]["median"]
                gt = L.device_tensor(core.lbfgsx_vec(h, L.VEC_GT), (n,), np.float64, 0).clone()
            if not args.dense_only:
                with step("torch callable D %d" % D):
                    xt = (x + 0.37 * d).view(F, D)
                    rows = torch.arange(R, device=dev)

                    def fn(xv, grad):
                        z = a @ xv
                        if D == 1:
                            mm = y[:, None] * z
                            v = torch.nn.functional.softplus(-mm)
                            gz = -y[:, None] * torch.sigmoid(-mm)
                            val = v.sum()
                        else:
                            lp = torch.log_softmax(z, dim=1)
                            gz = lp.exp()
                            gz[rows, labels] -= 1.0
                            val = -lp[rows, labels].sum()
                        torch.matmul(a.t(), gz, out=grad)
                        grad.add_(xv, alpha=LAM)
                        return float(val + 0.5 * LAM * (xv * xv).sum())
                    g = torch.empty_like(xt)
                    ms = []
                    for _ in range(args.calls):
                        t0 = time.perf_counter()
                        ft = fn(xt, g)
                        ms.append((time.perf_counter() - t0) * 1e3)
                    case["torch_ms"] = {"median": float(np.median(ms[4:])), "min": float(np.min(ms[4:]))}
                    case["torch_f"] = ft
                    case["torch_over_fused"] = case["torch_ms"]["median"] / case["trial_ms"]["median"]
                    case["max_abs_gradient_difference"] = float((gt - g.view(-1)).abs().max())
                    del g, xt
                if R * F <= args.sparse_limit:
                    with step("sparse form D %d" % D):
                        rowptr = (torch.arange(R + 1, dtype=torch.int64, device=dev) * F).to(torch.int32)
                        col = torch.arange(F, dtype=torch.int32, device=dev).repeat(R)
                        hs = C.c_void_p()
                        L.check(core.lbfgsx_create(C.byref(hs), L.F64, n, 1, 0, 0))
                        L.device_tensor(core.lbfgsx_vec(hs, L.VEC_X), (n,), np.float64, 0).copy_(x)
                        L.device_tensor(core.lbfgsx_vec(hs, L.VEC_D), (n,), np.float64, 0).copy_(d)
                        torch.cuda.synchronize()
                        L.check(core.lbfgsx_ls_begin(hs))
                        oid_s = C.c_int(-1)
                        t0 = time.perf_counter()
                        L.check(core.lbfgsx_objective_bind_linear(hs, sparse[D].compile(), R, R * F, rowptr.data_ptr(), col.data_ptr(),
                                                                  a.data_ptr(), 1, 0, C.byref(ptrs), C.byref(cs), C.byref(oid_s)))
                        case["sparse_bind_ms"] = (time.perf_counter() - t0) * 1e3
                        case["sparse_trial_ms"] = trials(hs, oid_s.value, args.calls)
                        case["sparse_f_equal"] = bool(fx.value == case["f"])
                        case["sparse_over_dense"] = case["sparse_trial_ms"]["median"] / case["trial_ms"]["median"]
                        core.lbfgsx_destroy(hs)
                        del rowptr, col
                else:
                    case["sparse_skipped"] = "nnz = %d exceeds --sparse-limit %d" % (R * F, args.sparse_limit)
            core.lbfgsx_destroy(h)
            torch.cuda.empty_cache()
            rec["cases"].append(case)
            sys.stderr.write(json.dumps(case) + "\n")
            json.dump(rec, open(args.out, "w"))
        del a, labels
        torch.cuda.empty_cache()
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"stream_copy_gbps": rec["stream_copy_gbps"],
                      "cases": [{k: c.get(k) for k in ("R", "F", "D", "lanes", "trial_ms", "torch_ms", "torch_over_fused",
                                                       "sparse_trial_ms", "sparse_over_dense", "fraction_of_stream_copy")}
                                for c in rec["cases"]]}))


if __name__ == "__main__":
    main()
