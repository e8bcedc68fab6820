#!/usr/bin/env python3
"""Registers, scratch and occupancy of the kernels on the two kernel frames -- own_frame.cuh: graph, mesh and linear-model
(sparse, multi-output, dense); halo_frame.cuh: chain, grid, volume, the two periodic forms, the grid field form and the grid stencil
form -- in two trees, side by side
(profiles/own_frame_kernel_resources.tsv).  No GPU is needed: the generated sources are compiled for gfx950 here.

Each tree (a built checkout: the parent commit's and this one) is asked, in a process of its own, for the generated
translation unit -- source() -- of
    chain    ASYM2, ASYM3, CHAINED_ROSEN, SECOND_DIFF at their K                 (tests/chain_ref.py)
    grid     ASYM4, ALLENCAHN                                                  (tests/grid_ref.py)
    volume   ASYM8, ALLENCAHN3                                                 (tests/volume_ref.py)
    pgrid    PASYM4, ALLENCAHN; pvolume  PASYM8, ALLENCAHN3                     (tests/periodic_ref.py)
    gfield   FASYM, GL at D = 1, 2, 3                                          (tests/field_ref.py)
    stencil  SASYM9, PLATE                                                     (tests/stencil_ref.py)
    graph    ASYM_EDGE with and without NODE                                   (tests/graph_ref.py)
    mesh     every (K, D) with the bodies tests/test_mesh_objective_cpu.py compiles (tests/mesh_ref.py)
    linear   LOGISTIC with and without RIDGE                                   (tests/linear_ref.py)
    multi    MHINGE at D = 1, 3, 10, 16 with and without RIDGE                 (tests/multilinear_ref.py)
    dense    the same bodies and D over a dense matrix
at f64 and f32.  Each is compiled against its own tree's lbfgspp_amd/csrc with the library's flags,
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -Rpass-analysis=kernel-resource-usage
and the compiler's remarks give VGPRs, scratch bytes per lane and occupancy (waves per SIMD) per kernel.

A case the parent tree does not have (a form it lacks) has no parent figures (-) and is checked for scratch only.

The script fails when a kernel of this tree has scratch or a lower occupancy than the parent's.

    python scripts/measure_own_frame_resources.py --parent <built checkout of the parent commit> [--out profiles/...tsv]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S",
         "-Rpass-analysis=kernel-resource-usage"]


def emit_sources(tree):
    """{case: source} of one tree, by that tree's own library"""
    for p in (tree, os.path.join(tree, "tests")):
        sys.path.insert(0, p)
    import numpy as np

    import chain_ref as CR
    import graph_ref as GR
    import grid_ref as GD
    import linear_ref as LR
    import lbfgspp_amd as A
    import mesh_ref as MR
    import multilinear_ref as ML
    out = {}
    one_edge = (np.array([0]), np.array([1]))
    one_entry = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([1.0]))
    for dname, dtype in (("f64", np.float64), ("f32", np.float32)):
        for name, body, K in (("asym2", CR.ASYM2, 2), ("asym3", CR.ASYM3, 3), ("chained_rosen", CR.CHAINED_ROSEN, 2),
                              ("second_diff", CR.SECOND_DIFF, 3)):
            out["chain/K%d/%s/%s" % (K, name, dname)] = A.ChainObjective(body, K=K).source(dtype)
        for name, body in (("asym4", GD.ASYM4), ("allencahn", GD.ALLENCAHN)):
            out["grid/%s/%s" % (name, dname)] = A.GridObjective(body, shape=(2, 2)).source(dtype)
        if hasattr(A, "VolumeObjective"):
            import volume_ref as VR
            for name, body in (("asym8", VR.ASYM8), ("allencahn3", VR.ALLENCAHN3)):
                out["volume/%s/%s" % (name, dname)] = A.VolumeObjective(body, shape=(2, 2, 2)).source(dtype)
        if hasattr(A, "PeriodicGridObjective"):
            import periodic_ref as PR
            for name, body in (("pasym4", PR.PASYM4), ("allencahn", PR.ALLENCAHN)):
                out["pgrid/%s/%s" % (name, dname)] = A.PeriodicGridObjective(body, shape=(2, 2)).source(dtype)
            for name, body in (("pasym8", PR.PASYM8), ("allencahn3", PR.ALLENCAHN3)):
                out["pvolume/%s/%s" % (name, dname)] = A.PeriodicVolumeObjective(body, shape=(2, 2, 2)).source(dtype)
        if hasattr(A, "GridFieldObjective"):
            import field_ref as FR
            for D in (1, 2, 3):
                for name, body in (("fasym", FR.FASYM), ("gl", FR.GL)):
                    out["gfield/D%d/%s/%s" % (D, name, dname)] = A.GridFieldObjective(body, shape=(2, 2), D=D).source(dtype)
        if hasattr(A, "StencilObjective"):
            import stencil_ref as SR
            for name, body in (("sasym9", SR.SASYM9), ("plate", SR.PLATE)):
                out["stencil/%s/%s" % (name, dname)] = A.StencilObjective(body, shape=(3, 3)).source(dtype)
        for name, node in (("asym+node", GR.NODE), ("asym", None)):
            out["graph/%s/%s" % (name, dname)] = A.GraphObjective(GR.ASYM_EDGE, edges=one_edge, node_body=node).source(dtype)
        for K in (2, 3, 4):
            for D in (1, 2, 3):
                bodies = list(MR.GENERIC_BODIES)
                bodies += {(3, 1): [("triple", MR.ALIAS_I + MR.TRIPLE, None)], (3, 2): [("triangle", MR.TRIANGLE, MR.TIE_NODE)],
                           (4, 3): [("volume", MR.VOLUME, None)]}.get((K, D), [])
                for name, elem, node in bodies:
                    out["mesh/K%dD%d/%s/%s" % (K, D, name, dname)] = A.MeshObjective(elem, MR.strip(K, K), D, node_body=node).source(dtype)
        for name, coord in (("logistic+ridge", LR.RIDGE), ("logistic", None)):
            out["linear/%s/%s" % (name, dname)] = A.LinearObjective(LR.LOGISTIC, one_entry, 1, coord_body=coord).source(dtype)
        for D in (1, 3, 10, 16):
            for name, coord in (("mhinge+ridge", ML.RIDGE), ("mhinge", None)):
                out["multi/D%d/%s/%s" % (D, name, dname)] = A.MultiLinearObjective(ML.MHINGE, one_entry, 1, D,
                                                                                  coord_body=coord).source(dtype)
                out["dense/D%d/%s/%s" % (D, name, dname)] = A.DenseLinearObjective(ML.MHINGE, np.ones((1, 1)), D,
                                                                                  coord_body=coord).source(dtype)
    return out


def kernel_name(mangled):
    m = re.search(r"(\d+)k_", mangled)
    return mangled[m.end(1):m.end(1) + int(m.group(1))] if m else mangled


def resources(job):
    """{kernel: (vgprs, scratch, occupancy)} of one source compiled against one tree's kernel headers"""
    src, csrc = job
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "objective_wrapper.hip")
        with open(path, "w") as f:
            f.write(src)
        r = subprocess.run([HIPCC] + FLAGS + ["-I", csrc, path, "-o", os.path.join(d, "out.s")], stderr=subprocess.PIPE, text=True)
        if r.returncode:
            raise SystemExit(r.stderr[-4000:])
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:.*?\s)?(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = kernel_name(m.group(2))
            out[name] = {}
        elif name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return {k: (v["VGPRs"], v["ScratchSize"], v["Occupancy"]) for k, v in out.items() if k.startswith("k_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "own_frame_kernel_resources.tsv"))
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--emit-sources", metavar="TREE", help="print the sources of TREE as JSON and nothing else")
    args = ap.parse_args()
    if args.emit_sources:
        json.dump(emit_sources(args.emit_sources), sys.stdout)
        return
    if not args.parent:
        ap.error("--parent is required")
    trees = {"parent": os.path.abspath(args.parent), "head": ROOT}
    srcs = {k: json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--emit-sources", t], cwd=t, check=True,
                                         stdout=subprocess.PIPE, text=True).stdout) for k, t in trees.items()}
    assert set(srcs["parent"]) <= set(srcs["head"])
    cases = sorted(srcs["head"])
    jobs = [(srcs[k][c], os.path.join(trees[k], "lbfgspp_amd", "csrc")) for c in cases for k in ("parent", "head") if c in srcs[k]]
    with ThreadPoolExecutor(max_workers=args.jobs) as ex:
        done = iter(list(ex.map(resources, jobs)))
    res = {(c, k): next(done) for c in cases for k in ("parent", "head") if c in srcs[k]}
    bad = []
    with open(args.out, "w") as f:
        f.write("# VGPRs, scratch bytes per lane and occupancy (waves per SIMD) of every chain, grid, volume, periodic, graph, mesh and\n"
                "# linear-model kernel, from the compiler's kernel-resource-usage remarks: the parent commit and this tree's kernels\n"
                "# on own_frame.cuh and halo_frame.cuh, side by side; - where the parent has no such form\n"
                "# (scripts/measure_own_frame_resources.py; case = form/bodies/dtype)\n")
        f.write("case\tkernel\tvgpr_parent\tvgpr_head\tscratch_parent\tscratch_head\toccupancy_parent\toccupancy_head\tsame_source\n")
        for c in cases:
            head = res[c, "head"]
            if c not in srcs["parent"]:
                for k in sorted(head):
                    h = head[k]
                    f.write("%s\t%s\t-\t%d\t-\t%d\t-\t%d\t-\n" % (c, k, h[0], h[1], h[2]))
                    if h[1] != 0:
                        bad.append("%s %s: scratch %d" % (c, k, h[1]))
                continue
            parent = res[c, "parent"]
            assert sorted(parent) == sorted(head), (c, sorted(parent), sorted(head))
            for k in sorted(head):
                p, h = parent[k], head[k]
                f.write("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (c, k, p[0], h[0], p[1], h[1], p[2], h[2],
                                                                    "yes" if srcs["parent"][c] == srcs["head"][c] else "no"))
                if h[1] != 0 or h[2] < p[2]:
                    bad.append("%s %s: scratch %d, occupancy %d against the parent's %d" % (c, k, h[1], h[2], p[2]))
    print("wrote %s: %d cases" % (args.out, len(cases)))
    if bad:
        sys.exit("\n".join(bad))


if __name__ == "__main__":
    main()
