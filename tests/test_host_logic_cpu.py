"""-m "not gpu": the pure-host pieces of the drop-in headers, compiled with g++ and driven through a small C
wrapper (tests/cpp/host_logic_capi.cpp): Bunch-Kaufman LDL' (reference BKLDLT.h:390-520), the More-Thuente state
machine (MoreThuente.h:213-615) and parameter validation (Param.h:193-217,352-376).  No GPU, no device library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_util as GU
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# LBFGSX_TEST_SANITIZE=1 (scripts/sanitize_host.sh, with libasan preloaded into the interpreter): the host templates under
# AddressSanitizer + UndefinedBehaviorSanitizer, any finding aborts the test process
SAN = (["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
       if os.environ.get("LBFGSX_TEST_SANITIZE") == "1" else [])


@pytest.fixture(scope="module")
def hl(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hl") / "libhostlogic.so")
    cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off"] + SAN + ["-I", os.path.join(ROOT, "include"),
           os.path.join(HERE, "cpp", "host_logic_capi.cpp"), "-o", out]
    subprocess.check_call(cmd)
    lib = C.CDLL(out)
    lib.hl_bkldlt_solve.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _sym(rng, n, kind):
    A = rng.standard_normal((n, n))
    A = A + A.T
    if kind == "zero_diag":      # forces 2x2 pivots
        np.fill_diagonal(A, 0.0)
    elif kind == "permMinv":     # the L-BFGS-B structure: [[-D, L'], [L, theta S'S]] padded with identity rows
        c = n // 2
        S = rng.standard_normal((50, c))
        Y = S * (1 + rng.random((50, c))) + 0.1 * rng.standard_normal((50, c))
        SY = S.T @ Y
        A = np.zeros((n, n))
        A[:c, :c] = -np.diag(np.diag(SY))
        A[c:2 * c, :c] = np.tril(SY, -1)
        A[:c, c:2 * c] = np.tril(SY, -1).T
        A[c:2 * c, c:2 * c] = 1.7 * (S.T @ S)
        for i in range(2 * c, n):
            A[i, i] = 1.0
    elif kind == "spd":
        A = A @ A.T + n * np.eye(n)
    return A


@pytest.mark.parametrize("kind", ["indefinite", "zero_diag", "permMinv", "spd"])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 12, 20, 40])
def test_bkldlt_solves_symmetric_systems(hl, n, kind):
    if kind == "zero_diag" and n == 1:
        pytest.skip("the 1 x 1 zero matrix is singular")
    rng = np.random.default_rng(100 * n + len(kind))
    A = _sym(rng, n, kind)
    b = rng.standard_normal(n)
    x = np.zeros(n)
    Af = np.asfortranarray(np.tril(A) + np.triu(np.full((n, n), np.nan), 1))  # only the lower triangle may be read
    info = hl.hl_bkldlt_solve(n, Af.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p))
    # n = 1 never enters the elimination loop, so info() keeps its initial NOT_COMPUTED -- same as the reference
    # (BKLDLT.h:407-436); the solve is valid all the same
    assert info == (0 if n > 1 else 1)
    ref = np.linalg.solve(A, b)
    cond = np.linalg.cond(A)
    assert np.abs(x - ref).max() <= 1e-13 * cond * max(1.0, np.abs(ref).max())
    assert np.abs(A @ x - b).max() <= 1e-12 * max(1.0, np.abs(A).max() * np.abs(x).max())


def test_bkldlt_requires_compute(hl):
    assert hl.hl_bkldlt_uncomputed_throws() == 1


PHI = C.CFUNCTYPE(C.c_double, C.c_double, C.POINTER(C.c_double), C.c_void_p)


def _search(hl, fun, step=1.0, step_max=1e20, ftol=1e-4, wolfe=0.9, min_step=1e-20, max_step=1e20, max_ls=20):
    calls = []

    def phi(t, dphi, _):
        f, d = fun(t)
        dphi[0] = d
        calls.append(t)
        return f

    cb = PHI(phi)
    so, fo, do, nf = C.c_double(), C.c_double(), C.c_double(), C.c_int()
    msg = C.create_string_buffer(256)
    hl.hl_more_thuente.argtypes = [PHI, C.c_void_p] + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_double,
                                                                           C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                                           C.POINTER(C.c_double), C.POINTER(C.c_int),
                                                                           C.c_char_p, C.c_int]
    rc = hl.hl_more_thuente(cb, None, ftol, wolfe, min_step, max_step, max_ls, step, step_max, C.byref(so), C.byref(fo),
                            C.byref(do), C.byref(nf), msg, 256)
    return rc, so.value, fo.value, do.value, nf.value, msg.value.decode(), calls


# the six test functions of More & Thuente (1994), table 5.1-5.6 shapes
def _mt1(t, beta=2.0):
    return -t / (t * t + beta), (t * t - beta) / (t * t + beta) ** 2


def _mt2(t, beta=0.004):
    return (t + beta) ** 5 - 2 * (t + beta) ** 4, 5 * (t + beta) ** 4 - 8 * (t + beta) ** 3


def _quad(t):
    return (t - 3.0) ** 2, 2 * (t - 3.0)


@pytest.mark.parametrize("fun", [_mt1, _mt2, _quad], ids=["mt1", "mt2", "quad"])
@pytest.mark.parametrize("step", [1e-3, 0.1, 1.0, 10.0])
@pytest.mark.parametrize("wolfe", [0.9, 0.1])
def test_more_thuente_returns_a_strong_wolfe_point(hl, fun, step, wolfe):
    ftol = 1e-4
    rc, t, f, d, nfev, msg, calls = _search(hl, fun, step=step, ftol=ftol, wolfe=wolfe, max_ls=40)
    assert rc == 0, msg
    f0, d0 = fun(0.0)
    assert (f, d) == fun(t)                       # the reported values belong to the reported step
    assert f <= f0 + ftol * t * d0 + 1e-15        # sufficient decrease
    if nfev < 40:  # with the budget exhausted (1.1x extrapolation from a tiny first step) only decrease is promised
        assert abs(d) <= wolfe * abs(d0) * (1 + 1e-12)  # curvature
    assert 1 <= nfev <= 40 and calls[1] == step   # calls[0] is phi(0); the first trial is the given step


def test_more_thuente_argument_errors(hl):
    rc, *_, msg, _c = _search(hl, _quad, step=-1.0)
    assert rc == 1 and msg == "'step' must be positive"
    rc, *_, msg, _c = _search(hl, _quad, step=2.0, step_max=1.0)
    assert rc == 1 and msg == "'step' exceeds 'step_max'"
    rc, *_, msg, _c = _search(hl, lambda t: ((t + 3.0) ** 2, 2 * (t + 3.0)), step=1.0)
    assert rc == 2 and msg == "the moving direction does not decrease the objective function value"


def test_more_thuente_exhausted_budget_returns_best_point(hl):
    """max_linesearch trials without a Wolfe point: the search hands back the saved best point, never throws
    (reference MoreThuente.h:599-613)."""
    rc, t, f, d, nfev, msg, calls = _search(hl, _mt2, step=1e-3, wolfe=1e-9, max_ls=3)
    assert rc == 0 and nfev <= 4
    assert (f, d) == _mt2(t) and f <= _mt2(0.0)[0]


BAD = GU.PARAM_BAD


def _check(hl, which, **kw):
    d = dict(m=6, epsilon=1e-5, epsilon_rel=1e-5, past=0, delta=0.0, max_iterations=0, linesearch=3, max_linesearch=20,
             min_step=1e-20, max_step=1e20, ftol=1e-4, wolfe=0.9, max_submin=10)
    d.update(kw)
    msg = C.create_string_buffer(256)
    hl.hl_check_param.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                  C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_char_p, C.c_int]
    rc = hl.hl_check_param(which, d["m"], d["epsilon"], d["epsilon_rel"], d["past"], d["delta"], d["max_iterations"],
                           d["linesearch"], d["max_linesearch"], d["min_step"], d["max_step"], d["ftol"], d["wolfe"],
                           d["max_submin"], msg, 256)
    return rc, msg.value.decode()


@pytest.mark.parametrize("bad", BAD, ids=[list(b)[0] + "=" + str(list(b.values())[0]) for b in BAD])
def test_param_validation_messages_match_the_reference(hl, bad):
    """the reference's exception text for each bad parameter: tests/golden/param_messages.json (what oracle/_ref answered,
    tests/golden/make_host_logic_golden.py), and oracle/_ref itself where it is built"""
    rc, msg = _check(hl, 0, **bad)
    assert rc == 1 and msg
    gold = GU.load("param_messages.json")[GU.PARAM_BAD.index(bad)]
    assert gold["param"] == bad and gold["status"] == 1 and gold["msg"] == msg
    if O.available("ref", "dd"):
        p = O.lbfgs_params(**bad)
        _, r = O.Oracle("ref", "dd").lbfgs(O.F64, O.LS_NW, O.OBJ_ROSEN, np.zeros(4), p)
        assert r.status == 1 and r.msg.decode() == msg


def test_param_validation_accepts_defaults_and_checks_lbfgsb_fields(hl):
    assert _check(hl, 0)[0] == 0 and _check(hl, 1)[0] == 0
    assert _check(hl, 0, linesearch=7)[0] == 1
    rc, msg = _check(hl, 1, max_submin=-1)
    assert rc == 1 and "max_submin" in msg



@pytest.mark.parametrize("kind", ["indefinite", "zero_diag", "permMinv", "spd"])
@pytest.mark.parametrize("n", [2, 7, 20, 40])
def test_bkldlt_batched_solve_is_bit_identical_lane_by_lane(hl, n, kind):
    """solve_inplace_batch<4> (used by the sequential Cauchy search for the M w of four break points at once) must give,
    in every lane, exactly the bits of solve_inplace"""
    rng = np.random.default_rng(31 * n + len(kind))
    A = _sym(rng, n, kind)
    Af = np.asfortranarray(np.tril(A) + np.triu(np.full((n, n), np.nan), 1))
    B = rng.standard_normal((4, n))
    B[3] = 0.0  # a padding lane, as at the end of a break-point list
    Xb = np.zeros((4, n))
    hl.hl_bkldlt_solve_batch4.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    hl.hl_bkldlt_solve_batch4(n, Af.ctypes.data_as(C.c_void_p), B.ctypes.data_as(C.c_void_p), Xb.ctypes.data_as(C.c_void_p))
    for k in range(4):
        x = np.zeros(n)
        hl.hl_bkldlt_solve(n, Af.ctypes.data_as(C.c_void_p), np.ascontiguousarray(B[k]).ctypes.data_as(C.c_void_p),
                           x.ctypes.data_as(C.c_void_p))
        assert np.array_equal(x, Xb[k])

# ---- Gram-space recursion (include/LBFGSpp/GramSpace.h): the coefficient form must reproduce BFGSMat::apply_Hv
def _two_loop(S, Y, order, v, a):
    """reference BFGSMat.h:276-302 on explicit vectors; order = pair indices newest -> oldest"""
    q = a * v
    alpha = {}
    for k in order:
        alpha[k] = (S[k] @ q) / (S[k] @ Y[k])
        q = q - alpha[k] * Y[k]
    if order:
        k0 = order[0]
        q = q / ((Y[k0] @ Y[k0]) / (S[k0] @ Y[k0]))
    for k in reversed(order):
        beta = (Y[k] @ q) / (S[k] @ Y[k])
        q = q + (alpha[k] - beta) * S[k]
    return q


@pytest.mark.parametrize("n,m,K,reject", [(50, 6, 0, ()), (50, 6, 1, ()), (50, 6, 4, ()), (50, 6, 6, ()), (50, 6, 15, ()),
                                          (64, 1, 5, ()), (40, 3, 11, (2, 7)), (200, 10, 27, (0, 13)), (30, 24, 30, ())])
def test_gram_space_direction_equals_vector_two_loop(hl, n, m, K, reject):
    rng = np.random.default_rng(7 * n + m + K)
    # a smooth convex model so that s.y > 0: g(x) = A x with SPD diagonal-dominant A
    A = np.diag(1.0 + 9.0 * rng.random(n)) + 0.05 * rng.standard_normal((n, n))
    A = 0.5 * (A + A.T) + n * 0.05 * np.eye(n)
    X = np.cumsum(0.3 * rng.standard_normal((K + 1, n)), axis=0)
    G = X @ A
    S = np.ascontiguousarray(X[1:] - X[:-1])
    Y = G[1:] - G[:-1]
    accept = np.ones(max(K, 1), dtype=np.uint8)
    for k in reject:
        accept[k] = 0
    coef = np.zeros(2 * m)
    cg = C.c_double()
    slots = np.zeros(m, dtype=np.int32)
    hl.hl_gram_space.restype = C.c_int
    ptr = hl.hl_gram_space(n, m, K, S.ctypes.data_as(C.c_void_p), np.ascontiguousarray(G).ctypes.data_as(C.c_void_p),
                           accept.ctypes.data_as(C.c_void_p), coef.ctypes.data_as(C.c_void_p), C.byref(cg),
                           slots.ctypes.data_as(C.c_void_p))
    assert ptr >= 0
    kept = [k for k in range(K) if accept[k]][-m:]           # the pairs still in the history, oldest -> newest
    assert sorted(int(v) for v in slots if v >= 0) == kept   # cyclic slot bookkeeping == BFGSMat::add_correction
    d = cg.value * G[K]
    for j in range(m):
        if slots[j] >= 0:
            d = d + coef[j] * S[slots[j]] + coef[m + j] * Y[slots[j]]
    ref = _two_loop(S, Y, kept[::-1], G[K], -1.0)
    assert np.linalg.norm(d - ref) <= 1e-9 * np.linalg.norm(ref)


def test_sums_over_L_u_U_are_used_by_the_solve_that_follows_their_pass_only(tmp_path):
    """Advisor finding (round 4): W_{L u U}'(-c), left un-rounded by Wtv_lu for the 'W_P'rhs without a pass' identity of
    BFGSMatB::solve_PtBP, must not survive a solve that does not consume it -- a later sweep with an empty L or U never
    calls Wtv_lu, and would have combined the OLD partition's sums with the new partition's Gram.  Host code against a mock of
    the C ABI (tests/cpp/mock_bfgsmat_capi.cpp); the log lists the device entries each sweep's solve called."""
    out = str(tmp_path / "libmockbfgs.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off"] + SAN +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "mock_bfgsmat_capi.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.mock_sweep_sequence.restype = C.c_char_p
    lib.mock_sweep_sequence.argtypes = [C.c_int]
    env = dict(os.environ)
    first, second = [s.split() for s in lib.mock_sweep_sequence(0).decode().split("|")]
    assert "wtv_lu_c" in first and "gram_fused_ex" in first and "solve_sweep_rhs" not in first        # sweep k: the one-pass Gram
    assert "solve_sweep_rhs" not in second, "sweep k + 1 used the sums of sweep k's partition: %r" % second
    assert "wtv_prologue" in second and "gram_fused_dd" in second                                     # complement branch, v row by a pass
    # control: with Wtv_lu right before it the same solve does use the identity (and no v-row pass)
    first, second = [s.split() for s in lib.mock_sweep_sequence(1).decode().split("|")]
    assert "solve_sweep_rhs" in second and "wtv_prologue" not in second, second


@pytest.fixture(scope="module")
def policy10_ours(tmp_path_factory):
    """tests/cpp/policy10_capi.cpp compiled against include/; the same source compiled against the reference's headers was
    run once on the same inputs, its results are tests/golden/policy10_golden.npz (tests/golden/make_host_logic_golden.py)"""
    out = str(tmp_path_factory.mktemp("p10") / "libpolicy10_ours.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off"] + SAN +
                          ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "oracle", "eigen_shim"),
                           os.path.join(HERE, "cpp", "policy10_capi.cpp"), "-o", out])
    return GU.policy10_lib(out)


@pytest.mark.parametrize("policy,conditions", GU.POLICY10_CASES,
                         ids=["backtracking", "bracketing", "more-thuente", "nocedal-wright"])
def test_built_in_policies_offer_the_reference_signature_with_the_reference_results(policy10_ours, policy, conditions):
    """VERDICT r5, missing 2: a program that calls a built-in policy directly through the reference's ten-argument static form
    now compiles -- and gets the reference's result: step, fx, dg, the evaluation count, x, grad and the exception class, on
    random descent (and a few ascent / degenerate) directions of the extended Rosenbrock function"""
    gold = np.load(os.path.join(HERE, "golden", "policy10_golden.npz"))
    seen = set()
    for trial, (_xp, _drt, args) in enumerate(GU.policy10_trials(policy, conditions)):
        n = args[2]
        rc_r, o_r = int(gold["p%d_rc" % policy][trial]), gold["p%d_out" % policy][trial]
        x_r, g_r = gold["p%d_x" % policy][trial, :n], gold["p%d_g" % policy][trial, :n]
        rc_o, o_o, x_o, g_o = GU.policy10_run(policy10_ours, args)
        assert rc_r == rc_o and o_r[3] == o_o[3], (trial, rc_r, rc_o, o_r, o_o)
        seen.add(rc_r)
        # The interpolation formulas of the More-Thuente / Nocedal-Wright machines are algebraically the reference's, not
        # operation for operation (a step may differ in its last bit, x with it): the contract is the north star's 1e-10 on
        # iterates, and identical decisions.  dg is a dot product: the stand-in Eigen's order against a left-to-right loop.
        tol = 0.0 if policy < 2 else 1e-12
        assert np.abs(x_r - x_o).max() <= tol * max(1.0, np.abs(x_r).max()), trial
        assert np.abs(g_r - g_o).max() <= 1e3 * tol * max(1.0, np.abs(g_r).max()), trial
        if rc_r == 0:
            assert abs(o_r[0] - o_o[0]) <= tol * abs(o_r[0]) and abs(o_r[1] - o_o[1]) <= tol * max(1.0, abs(o_r[1])), (trial, o_r, o_o)
            assert abs(o_r[2] - o_o[2]) <= 1e-9 * max(1.0, abs(o_r[2])), (trial, o_r, o_o)
    assert 0 in seen and len(seen) >= 2   # successes and at least one exception class were exercised
