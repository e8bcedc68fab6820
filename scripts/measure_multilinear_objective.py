#!/usr/bin/env python3
"""What a multi-output linear-model objective (lbfgspp_amd.MultiLinearObjective) costs, in one process on one device
(profiles/multilinear_objective.json).  Recorded, not gated.  It follows scripts/measure_linear_objective.py.

  trial   f64, softmax cross-entropy + ridge with D = 10 outputs over a random sparse R x F matrix, R = 1e6, F = 1e5: the time
          of ONE trial evaluation (lbfgsx_trial: row pass, long-column launch if any, column pass; wall clock around the
          synchronous call, median of the timed calls after warm-up, the tile order alternating) with about 10 and about 100
          entries per row (columns uniform at random: no locality), and with 10 entries and a dense intercept column (column
          0, a long column); the effective bytes per second under the byte model of include/lbfgsx.h; beside it
            * the torch callable of the same objective (torch.sparse_csr @ W, log_softmax, the stored transpose for the
              gradient: the function a DeviceObjective would call) on the same device in the same process, and
            * one trial of the SCALAR form (logistic + ridge, n = F) on the same matrix: D of them are what D independent
              one-output models cost, the ratio recorded is D * scalar / multi;
  d1      at D = 1 the new form (the logistic body in the D-output signature) against the scalar form on the same matrix, the
          runs alternating.
  code    VGPRs and scratch of the compiled bodies, from the code object.

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multilinear_objective.json"))
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=100000)
    ap.add_argument("--outputs", type=int, default=10)
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
        sys.exit("measure_multilinear_objective.py needs a GPU")
    dev = "cuda:0"
    one = ([0, 1], [0], [1.0])
    R, F, D = args.rows, args.features, args.outputs
    multi = A.MultiLinearObjective(SOFTMAX, one, 1, D, coord_body=LR.RIDGE)
    scalar = A.LinearObjective(LR.LOGISTIC, one, 1, coord_body=LR.RIDGE)
    multi1 = A.MultiLinearObjective(MR.scalar_body(LR.LOGISTIC), one, 1, 1, coord_body=LR.RIDGE)
    rec = {"device": torch.cuda.get_device_name(0), "objective": "softmax + ridge", "dtype": "f64", "R": R, "F": F, "D": D,
           "code": {"softmax D=%d" % D: multi.info(), "logistic (scalar form)": scalar.info(), "logistic (D = 1)": multi1.info()},
           "cases": []}
    fx, dg = C.c_double(), C.c_double()

    def context(n, gen, like=None):
        """a context of n unknowns with a random point and direction, or with copies of the pair `like`"""
        h = C.c_void_p()
        L.check(core.lbfgsx_create(C.byref(h), L.F64, n, 1, 0, 0))
        x = L.device_tensor(core.lbfgsx_vec(h, L.VEC_X), (n,), np.float64, 0)
        d = L.device_tensor(core.lbfgsx_vec(h, L.VEC_D), (n,), np.float64, 0)
        x.copy_(like[0] if like else torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
        d.copy_(like[1] if like else torch.rand(n, dtype=torch.float64, device=dev, generator=gen) - 0.5)
        keep = (x.clone(), d.clone())
        torch.cuda.synchronize()
        L.check(core.lbfgsx_ls_begin(h))
        return h, keep[0], keep[1]

    def bind(h, obj, m, data):
        ptrs = (C.c_void_p * 4)(data.data_ptr(), None, None, None)
        cs = (C.c_double * 8)(LAM, 0, 0, 0, 0, 0, 0, 0)
        oid = C.c_int(-1)
        t0 = time.perf_counter()
        L.check(core.lbfgsx_objective_bind_linear(h, obj.compile(), R, m[1].numel(), m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(), 1,
                                                  0, C.byref(ptrs), C.byref(cs), C.byref(oid)))
        ms = (time.perf_counter() - t0) * 1e3
        info = (C.c_int64 * 8)()
        L.check(core.lbfgsx_objective_linear_topology(h, C.byref(info), None, None, None, None, None, None))
        return oid.value, ms, info

    def trials(pairs, calls):
        """[(h, oid)]: the contexts' trials alternating; per context the times after the warm-up calls"""
        ms = [[] for _ in pairs]
        for _ in range(calls):
            for k, (h, oid) in enumerate(pairs):
                t0 = time.perf_counter()
                L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
                ms[k].append((time.perf_counter() - t0) * 1e3)
        return [{"median": float(np.median(v[4:])), "min": float(np.min(v[4:]))} for v in ms]

    for per, intercept in ((10, False), (100, False), (10, True)):
        width = per + (1 if intercept else 0)
        nnz, n = R * width, F * D
        case = {"per_row": per, "intercept": intercept, "nnz": nnz, "n": n}
        with step("per %d intercept %s: set-up" % (per, intercept)):
            gen = torch.Generator(device=dev).manual_seed(per + (7 if intercept else 0))
            col = torch.randint(1 if intercept else 0, F, (R, width), dtype=torch.int32, device=dev, generator=gen)
            val = torch.randn(R, width, dtype=torch.float64, device=dev, generator=gen) / float(np.sqrt(width))
            if intercept:
                col[:, 0] = 0
                val[:, 0] = 1.0
            col, val = col.view(-1).contiguous(), val.view(-1).contiguous()
            rowptr = (torch.arange(R + 1, dtype=torch.int64, device=dev) * width).to(torch.int32)
            m = (rowptr, col, val)
            labels = torch.randint(0, D, (R,), device=dev, generator=gen)
            y = labels.to(torch.float64)
            ypm = 1.0 - 2.0 * (labels % 2).to(torch.float64)
            h, x, d = context(n, gen)
            hs, xs, ds = context(F, gen)
        with step("bind"):
            oid, case["bind_ms"], info = bind(h, multi, m, y)
            case.update(lanes=int(info[2]), chunk=int(info[3]), long_columns=int(info[4]), chunks=int(info[5]))
            assert int(info[6]) == D
            oid_s, case["scalar_bind_ms"], _ = bind(hs, scalar, m, ypm)
        with step("trial"):
            case["trial_ms"], case["scalar_trial_ms"] = trials([(h, oid), (hs, oid_s)], args.calls)
            L.check(core.lbfgsx_trial(h, oid, 0.37, C.byref(fx), C.byref(dg)))
            case["f"] = fx.value
            # the byte model of one trial (include/lbfgsx.h): the trial kernel's four streams and the one data array, then the
            # matrix terms with the gathered values (xp, d, w), w written and read and the chunk partials counted D times
            model = 4 * n * 8 + n * 8 + (R + 1) * 4 + (F + 1) * 4 + 2 * nnz * 4 + 2 * nnz * 8 + 3 * nnz * 8 * D + 2 * R * 8 * D \
                + 2 * R * 8 + 2 * case["chunks"] * 8 * D
            case["model_bytes"] = model
            case["model_gbps"] = model / case["trial_ms"]["median"] / 1e6
            case["d_scalar_over_multi"] = D * case["scalar_trial_ms"]["median"] / case["trial_ms"]["median"]
        try:
            with step("torch callable"):
                a = torch.sparse_csr_tensor(rowptr, col, val, size=(R, F))
                at = a.t().to_sparse_csr()
                xt = (x + 0.37 * d).view(F, D)
                rows = torch.arange(R, device=dev)

                def fn(xv, grad):
                    z = a @ xv
                    lp = torch.log_softmax(z, dim=1)
                    p = lp.exp()
                    p[rows, labels] -= 1.0
                    grad.copy_(at @ p)
                    grad.add_(xv, alpha=LAM)
                    return float(-lp[rows, labels].sum() + 0.5 * LAM * (xv * xv).sum())
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
                case["max_abs_gradient_difference"] = float((gt - g.view(-1)).abs().max())
                del a, at, g, xt
        except RuntimeError as e:  # torch could not form or multiply the CSR matrix: recorded, the rest goes on
            if "HIP" in str(e) or "illegal" in str(e):  # a device error is not: nothing more is started
                raise
            case["torch_error"] = str(e)[:300]
        if per == 10 and not intercept:
            with step("D = 1 against the scalar form"):
                h1, _, _ = context(F, gen, (xs, ds))  # the scalar context's point and direction: f is then the same number
                oid_1, _, info = bind(h1, multi1, m, ypm)
                assert int(info[6]) == 1
                t1, ts = trials([(h1, oid_1), (hs, oid_s)], 2 * args.calls)
                L.check(core.lbfgsx_trial(h1, oid_1, 0.37, C.byref(fx), C.byref(dg)))
                f1 = fx.value
                L.check(core.lbfgsx_trial(hs, oid_s, 0.37, C.byref(fx), C.byref(dg)))
                rec["d1"] = {"per_row": per, "multi_form_ms": t1, "scalar_form_ms": ts, "multi_over_scalar": t1["median"] / ts["median"],
                             "f_multi": f1, "f_scalar": fx.value}
                core.lbfgsx_destroy(h1)
        core.lbfgsx_destroy(h)
        core.lbfgsx_destroy(hs)
        del col, val, rowptr, y, ypm, labels, m
        torch.cuda.empty_cache()
        rec["cases"].append(case)
        sys.stderr.write(json.dumps(case) + "\n")
        json.dump(rec, open(args.out, "w"))
    json.dump(rec, open(args.out, "w"))
    print(json.dumps({"cases": [{k: c.get(k) for k in ("per_row", "intercept", "lanes", "bind_ms", "trial_ms", "scalar_trial_ms",
                                                       "d_scalar_over_multi", "torch_ms", "torch_over_fused", "model_gbps")}
                                for c in rec["cases"]], "d1": rec.get("d1"),
                      "vgprs": {k: v["vgprs"] for k, v in rec["code"].items()}}))


if __name__ == "__main__":
    main()
