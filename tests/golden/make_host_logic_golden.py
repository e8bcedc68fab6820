#!/usr/bin/env python
"""Reference side of two tests of tests/test_host_logic_cpu.py, computed once and committed (test infrastructure).

* policy10_golden.npz -- tests/cpp/policy10_capi.cpp calls the four line-search policies through the reference's ten-argument
  static form.  This script compiles it against the UNMODIFIED reference headers (/root/reference/include, with
  oracle/eigen_shim as Eigen, the flags the test uses), runs the test's seeded trials (tests/golden_util.py: policy10_trials)
  and stores every result: the return code, step / fx / dg / evaluation count, x and grad (zero-padded to POLICY10_NMAX).
  The test compiles the same source against include/ only and compares with this file.
* param_messages.json -- the status and exception text oracle/_ref (make -C oracle ref) answers for each parameter set of
  tests/golden_util.py: PARAM_BAD.

    make -C oracle ref && python tests/golden/make_host_logic_golden.py [--ref /root/reference]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as GU  # noqa: E402
import oracle_lib as O  # noqa: E402

OUT = os.path.join(HERE, "policy10_golden.npz")
MSG_OUT = os.path.join(HERE, "param_messages.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference", help="checkout of the reference (its include/ is used)")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        lib_path = os.path.join(d, "libpolicy10_ref.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off",
                               "-I", os.path.join(args.ref, "include"), "-I", os.path.join(ROOT, "oracle", "eigen_shim"),
                               os.path.join(ROOT, "tests", "cpp", "policy10_capi.cpp"), "-o", lib_path])
        lib = GU.policy10_lib(lib_path)
        arrays = {}
        for policy, conditions in GU.POLICY10_CASES:
            T, N = GU.POLICY10_TRIALS, GU.POLICY10_NMAX
            rc, out = np.zeros(T, np.int32), np.zeros((T, 4))
            x, g = np.zeros((T, N)), np.zeros((T, N))
            for k, (_xp, _drt, a) in enumerate(GU.policy10_trials(policy, conditions)):
                r = GU.policy10_run(lib, a)
                rc[k], out[k] = r[0], r[1]
                x[k, :a[2]], g[k, :a[2]] = r[2], r[3]
            arrays.update({"p%d_rc" % policy: rc, "p%d_out" % policy: out, "p%d_x" % policy: x, "p%d_g" % policy: g})
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    ref = O.Oracle("ref", "dd")
    msgs = []
    for bad in GU.PARAM_BAD:
        _, r = ref.lbfgs(O.F64, O.LS_NW, O.OBJ_ROSEN, np.zeros(4), O.lbfgs_params(**bad))
        msgs.append({"param": bad, "status": r.status, "msg": r.msg.decode()})
    with open(MSG_OUT, "w") as f:
        json.dump(msgs, f, indent=1)
        f.write("\n")
    print("wrote %s" % MSG_OUT)


if __name__ == "__main__":
    main()
