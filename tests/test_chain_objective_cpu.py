"""CPU suite: chain objectives compiled at run time (lbfgspp_amd.ChainObjective, lbfgsx_objective_compile_chain of
include/lbfgsx.h).  Everything here runs without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object
says about its kernels is read from the code object itself."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_chain_eval", "k_chain_trial", "k_chain_b_eval", "k_chain_b_dg_maxstep_trial")


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body,K", [(CR.CHAINED_ROSEN, 2), (CR.SECOND_DIFF, 3), (CR.ASYM2, 2), (CR.ASYM3, 3)],
                         ids=["chained_rosenbrock", "second_difference", "asym2", "asym3"])
def test_both_K_compile_for_both_dtypes_without_scratch(A, body, K, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = A.ChainObjective(body, K=K)
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == K and core.lbfgsx_objective_form(h) == 1
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_chain_kernels(A):
    for body, K in ((CR.CHAINED_ROSEN, 2), (CR.SECOND_DIFF, 3)):
        for dtype in (np.float64, np.float32):
            src = A.ChainObjective(body, K=K).source(dtype)
            assert src.count(body) == 1
            assert '#include "chain_kernels.cuh"' in src and "static constexpr int K = %d;" % K in src
            for k in KERNELS:
                assert "template __global__ void %s<S, ObjChain>" % k in src
            assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
            assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)
    # the term form of the same body is another translation unit
    assert "k_chain_eval" not in A.TermObjective(CR.CHAINED_ROSEN, K=2).source()


def test_compile_error_comes_back_with_body_relative_lines(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    bad = "const T r = x[0];\ng[0] = r;\ng[1] = r\nreturn r * r;"  # line 3 lacks its semicolon
    with pytest.raises(ValueError) as e:
        A.ChainObjective(bad, K=2).compile()
    assert "ChainObjective" in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)
    h = C.c_void_p()
    log = C.create_string_buffer(4096)
    rc = core.lbfgsx_objective_compile_chain(C.byref(h), L.F32, 3, b"T q = undeclared_name;\nreturn q;", log, len(log))
    assert rc == L.E_INVALID and not h.value and b"objective_body:1:" in log.value and b"undeclared_name" in log.value
    # x has K elements: reading x[2] of a K = 2 term is caught by the compiler, not at run time
    assert A.ChainObjective(CR.CHAINED_ROSEN, K=2).info()["scratch_bytes"] == 0  # the process goes on


def test_K_outside_2_and_3_is_refused_by_name(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    for K in (1, 4):
        with pytest.raises(ValueError, match="ChainObjective: K = %d is not supported.*K = 2 or K = 3" % K):
            A.ChainObjective(CR.CHAINED_ROSEN, K=K)
        h = C.c_void_p()
        log = C.create_string_buffer(1024)
        assert core.lbfgsx_objective_compile_chain(C.byref(h), L.F64, K, CR.CHAINED_ROSEN.encode(), log, len(log)) == L.E_INVALID
        assert not h.value and b"K = %d" % K in log.value and b"K = 2 or K = 3" in log.value
        assert core.lbfgsx_objective_source_chain(L.F64, K, CR.CHAINED_ROSEN.encode(), None, 0) == L.E_INVALID
    # the term form keeps its own limit
    assert core.lbfgsx_objective_compile(C.byref(h), L.F64, 3, CR.SECOND_DIFF.encode(), log, len(log)) == L.E_INVALID
    assert b"K = 1 or K = 2" in log.value


def test_body_with_inline_assembly_is_refused(A):
    word = "as" + "m"
    for body in ("%s volatile(\"\");\ng[0] = x[0];\ng[1] = x[1];\nreturn x[0];" % word,
                 "g[0] = x[0]; g[1] = x[1]; __%s__(\"\"); return x[0];" % word):
        with pytest.raises(ValueError, match="inline assembly is not accepted"):
            A.ChainObjective(body, K=2).compile()


def test_pair_and_chain_of_one_body_are_two_cache_entries(A):
    core, _ = A.load()
    body = CR.CHAINED_ROSEN + "\n// cache test"
    pair, chain = A.TermObjective(body, K=2), A.ChainObjective(body, K=2)
    ip, ic = pair.info(), chain.info()
    assert not ip["cache_hit"] and not ic["cache_hit"]
    hp, hc = pair.compile(), chain.compile()
    assert hp.value != hc.value and core.lbfgsx_objective_form(hp) == 0 and core.lbfgsx_objective_form(hc) == 1
    again = A.ChainObjective(body, K=2).info()
    assert again["cache_hit"] and again["compile_ms"] == ic["compile_ms"] and again["vgprs"] == ic["vgprs"]
    assert A.TermObjective(body, K=2).info()["cache_hit"]
    # another K or dtype of the chain form is another entry
    assert not A.ChainObjective(body, K=2).info(np.float32)["cache_hit"]


NEW_SYMBOLS = ["lbfgsx_objective_compile_chain", "lbfgsx_objective_source_chain", "lbfgsx_objective_form"]


def test_new_symbols_are_exported_and_listed(A):
    listed = open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "export.map")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lbfgspp_amd", "liblbfgsx.so")], stdout=subprocess.PIPE,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    for name in NEW_SYMBOLS:
        assert name in exported, "liblbfgsx.so does not export %s" % name
        assert name + ";" in listed, "export.map does not list %s" % name
        assert name + "(" in header
    assert "ChainObjective" in A.__all__


def test_n_below_K_and_other_limits_are_said_before_a_device_is_needed(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="n = 2 is less than K = 3"):
        s.minimize(A.ChainObjective(CR.SECOND_DIFF, K=3, data=(np.ones(2), np.ones(2)), scalars=(1.0,)), np.zeros(2))
    f = A.ChainObjective(CR.CHAINED_ROSEN, K=2)
    res = L.Result()
    x = np.zeros(1)
    rc = sol.lbfgsx_solver_minimize_obj(s._h, f.compile(), 1, None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None,
                                        C.byref(res))
    assert rc == L.E_INVALID and b"n = 1 is less than K = 2" in res.msg
    with pytest.raises(ValueError, match="ChainObjective: 5 data arrays given, at most 4"):
        A.ChainObjective(CR.CHAINED_ROSEN, data=[np.ones(4)] * 5)
    with pytest.raises(ValueError, match="ChainObjective: data\\[0\\] must have 5 elements"):
        s.minimize(A.ChainObjective(CR.ASYM2, data=(np.ones(4),), scalars=CR.ASYM_SCALARS), np.zeros(5))


def test_generated_wrapper_and_kernel_header_name_no_inline_assembly(A):
    """the text generated around a body and the header it includes hold no inline assembly of their own (the word is spelt in
    pieces so that this file does not hold it either)"""
    word = "as" + "m"
    text = A.ChainObjective(CR.SECOND_DIFF, K=3).source() + open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "chain_kernels.cuh")).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", [2, 3, 4, 5, 9, 64])
def test_the_numpy_restatement_follows_the_ownership_rule(dtype, n):
    """chain_grad (vectorised, what the GPU tests compare with) against the rule written as a loop over the coordinates"""
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(dtype)
    p0 = (0.5 + rng.random(n)).astype(dtype)
    cases = [CR.chained_rosen_terms(x), CR.asym2_terms(x, p0)]
    if n >= 3:
        cases += [CR.asym3_terms(x, p0), CR.second_diff_terms(x, p0, p0[::-1].copy(), 0.7)]
    for tg, v in cases:
        K = len(tg)
        assert v.size == n - K + 1 and v.dtype == dtype
        g = CR.chain_grad(tg, n)
        assert g.dtype == dtype and np.array_equal(g, CR.chain_grad_scalar(tg, n))
    # the gradient is the derivative: central differences of the sum of the values, in double
    if dtype == np.float64 and n >= 3:
        tg, v = CR.asym3_terms(x, p0)
        g = CR.chain_grad(tg, n)
        for j in range(n):
            e = np.zeros(n)
            e[j] = 1e-6
            fd = (CR.asym3_terms(x + e, p0)[1].sum() - CR.asym3_terms(x - e, p0)[1].sum()) / 2e-6
            assert abs(fd - g[j]) <= 1e-6 * (1.0 + abs(g[j]))
