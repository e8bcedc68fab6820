"""CPU suite: tests/subspace_ref.py is proved here before tests/test_subspace_statements_gpu.py relies on it.
  * the vectorised statements equal a scalar transcription of the reference's SubspaceMin.h (:159-172, :194-219, :229-271,
    :276-296) bit for bit on the edge inputs (every tie, one ulp around every bound, infinite bounds, l = u);
  * the fused passes (solve_sweep, lu_sweep) equal the separate statements they stand for;
  * a whole minimisation composed of the statements agrees with the oracle's cauchy_subspace on the instances of
    test_cauchy_and_subspace_match_oracle at that test's tolerance;
  * every case generator's inputs contain every edge class and every set change between two sweeps."""
import numpy as np
import pytest

import subspace_ref as S

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]


def _vecs(n, dt, seed, shift=0, c=3):
    """a host-only case: rows, a history, cF random, edge values in y / lam / mu, sentinels elsewhere"""
    r = S.build_rows(n, dt, seed)
    st = np.where(r["free"], S.ST_FREE, np.where(r["newact"], S.ST_NEWACT, 0)).astype(np.uint8)
    rng = np.random.default_rng([seed, 5])
    li, ui = r["lb"] - r["x0_sweep"], r["ub"] - r["x0_sweep"]
    y, lam, mu = S.edge_values(li, ui, r["free"], dt, shift, seed)
    for k, a in ((S.SV_Y, y), (S.SV_LAM, lam), (S.SV_MU, mu)):
        a[~r["free"]] = S.sentinel(k, n, dt)[~r["free"]]
    V = S.Vecs(dt, x0=r["x0_sweep"], g=r["g"], lb=r["lb"], ub=r["ub"], drt=rng.standard_normal(n), cF=rng.standard_normal(n), y=y,
               yfb=S.sentinel(S.SV_YFB, n, dt), lam=lam, mu=mu, rhs=S.sentinel(S.SV_RHS, n, dt), st=st)
    _, cols = S.history(n, c, dt, seed)
    return V, cols, r


def _same(V, W, what=""):
    for k in S.Vecs.FIELDS:
        assert S.same_bits(getattr(V, k), getattr(W, k)), "%s: %s differs in rows %s" % (what, k, S.diff_rows(getattr(V, k), getattr(W, k))[:8])


# ---------------------------------------------------------------- scalar transcription
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shift", [0, 7])
def test_partition_equals_the_scalar_transcription(dt, shift):
    V, _, r = _vecs(400, dt, 1, shift)
    f = np.nonzero(r["free"])[0]
    vecy, vecl, vecu, lam, mu = V.y[f].copy(), V.li[f], V.ui[f], V.lam[f].copy(), V.mu[f].copy()
    L, U, P = S.scalar_partition(vecy, vecl, vecu, lam, mu)
    W = V.copy()
    nl, nu, np_ = S.partition(W)
    assert (nl, nu, np_) == (len(L), len(U), len(P)) and min(nl, nu, np_) > 0
    assert S.same_bits(W.y[f], vecy) and S.same_bits(W.lam[f], lam) and S.same_bits(W.mu[f], mu)
    for rows, bit in ((L, S.ST_L), (U, S.ST_U), (P, S.ST_P)):
        assert np.array_equal(np.nonzero(W.st & bit)[0], f[rows])
    # nothing else moved: the rows outside the free set, yfb, rhs, cF, drt
    for k in ("y", "lam", "mu"):
        assert S.same_bits(getattr(W, k)[~r["free"]], getattr(V, k)[~r["free"]])
    for k in ("yfb", "rhs", "cF", "drt"):
        assert S.same_bits(getattr(W, k), getattr(V, k))
    assert np.array_equal(W.st[~r["free"]], V.st[~r["free"]])


@pytest.mark.parametrize("dt", DTYPES)
def test_sweeps_equal_the_scalar_transcription(dt):
    """first sweep: :170-172 then :194-219 and :232; a later one: the counts of :271 on the values before, then the same"""
    V, _, r = _vecs(400, dt, 2, 0)
    f = np.nonzero(r["free"])[0]
    T = V.dt
    # first
    vecy, vecl, vecu = V.y[f].copy(), V.li[f], V.ui[f]
    yfb = vecy.copy()
    lam, mu = np.zeros(f.size, T), np.zeros(f.size, T)
    outside = S.scalar_converged([], [], [], vecy, vecl, vecu, lam, mu)[0]
    L, U, P = S.scalar_partition(vecy, vecl, vecu, lam, mu)
    W = V.copy()
    cnt = S.sweep(W, True, None, np.zeros(V.n, T), np.zeros(V.n, T))
    assert cnt == [len(L), len(U), len(P), outside, 0, 0, 0] and outside > 0
    assert S.same_bits(W.y[f], vecy) and S.same_bits(W.yfb[f], yfb) and S.same_bits(W.lam[f], lam) and S.same_bits(W.mu[f], mu)
    assert S.same_bits(W.rhs[f[P]], V.cF[f[P]])
    keep = np.ones(V.n, bool)
    keep[f[P]] = False
    assert S.same_bits(W.rhs[keep], V.rhs[keep]), "rhs changed outside the new P"
    assert S.same_bits(W.yfb[~r["free"]], V.yfb[~r["free"]])
    # a later sweep on the sets the first one made, with new values (another class for every row)
    y2, lam2, mu2 = S.edge_values(V.li, V.ui, r["free"], dt, 7, 3)
    X = W.copy()
    X.y[f], X.lam[f], X.mu[f] = y2[f], lam2[f], mu2[f]
    X.rhs = S.sentinel(S.SV_RHS, V.n, dt, 1)
    vecy, lam, mu = X.y[f].copy(), X.lam[f].copy(), X.mu[f].copy()
    conv = S.scalar_converged(L, U, P, vecy, vecl, vecu, lam, mu)
    L2, U2, P2 = S.scalar_partition(vecy, vecl, vecu, lam, mu)
    Z = X.copy()
    cnt = S.sweep(Z, False)
    assert cnt == [len(L2), len(U2), len(P2), 0, conv[1], conv[2], conv[3]] and min(conv[1:]) > 0
    assert S.check(X) == list(conv)
    assert S.same_bits(Z.y[f], vecy) and S.same_bits(Z.lam[f], lam) and S.same_bits(Z.mu[f], mu)
    assert S.same_bits(Z.rhs[f[P2]], X.cF[f[P2]])
    keep = np.ones(V.n, bool)
    keep[f[P2]] = False
    assert S.same_bits(Z.rhs[keep], X.rhs[keep]) and S.same_bits(Z.yfb, X.yfb)
    assert S.transitions(X.st, Z.st) >= {"L->P", "U->P", "P->L", "P->U", "L->U"}


@pytest.mark.parametrize("dt", DTYPES)
def test_multipliers_and_clamps_equal_the_scalar_transcription(dt):
    V, cols, r = _vecs(300, dt, 4, 0, c=3)
    S.partition(V)
    T = V.dt
    c = 3
    coef = np.random.default_rng(9).standard_normal(2 * c)
    theta = 1.7
    cf = S.coef_t(coef, T, 2 * c)
    W = V.copy()
    S.wcombine(W, cols, S.CB_LAMBDA, S.ST_L, S.VS_DRT, coef, theta)
    S.wcombine(W, cols, S.CB_MU, S.ST_U, S.VS_DRT, coef, theta)
    for i in range(V.n):
        res = S.scalar_multiplier([cols[j][i] for j in range(c)], [cols[c + j][i] for j in range(c)], cf[:c], cf[c:], V.cF[i], T(theta), V.y[i])
        if V.st[i] & S.ST_L:
            assert W.lam[i].tobytes() == res.tobytes()
        else:
            assert W.lam[i].tobytes() == V.lam[i].tobytes()
        if V.st[i] & S.ST_U:
            assert W.mu[i].tobytes() == (-res).tobytes()
        else:
            assert W.mu[i].tobytes() == V.mu[i].tobytes()
    # the plain order differs from the paired one somewhere: the two accumulation orders are not interchangeable
    assert not S.same_bits(S.wacc(cols, coef, T), S.wacc(cols, coef, T, paired=True))
    f = r["free"]
    for op, src in ((S.SO_CLAMP_Y, V.y), (S.SO_CLAMP_FB, V.yfb)):
        W = V.copy()
        W.yfb[f] = S.edge_values(V.li, V.ui, f, dt, 11, 5)[0][f]
        src = W.y if op == S.SO_CLAMP_Y else W.yfb
        want = S.scalar_clamp(src[f], V.li[f], V.ui[f])
        X = W.copy()
        S.sub_op(X, op)
        assert S.same_bits(X.y[f], want) and S.same_bits(X.y[~f], W.y[~f])


@pytest.mark.parametrize("dt", DTYPES)
def test_solve_and_prologue_restatements(dt):
    """y = v / theta + a / theta^2 row by row for every selector; rhs = (rhs + -(W c1)) + -(W c2) row by row"""
    V, cols, r = _vecs(200, dt, 6, 0, c=2)
    S.partition(V)
    T = V.dt
    rng = np.random.default_rng(8)
    coef, c1, c2 = rng.standard_normal(4), rng.standard_normal(4), rng.standard_normal(4)
    theta = 0.3
    th = T(theta)
    rows = V.rows(S.ST_P)
    for sel in range(6):
        W = V.copy()
        S.solve(W, cols, rows, sel, coef, theta)
        W0 = V.copy()
        S.solve(W0, cols, rows, sel, None, theta)
        v = S.vsel(V, sel)
        cf = S.coef_t(coef, T, 4)
        for i in np.nonzero(rows)[0]:
            a = T(0)
            for k in range(4):
                a = a + cols[k][i] * cf[k]
            assert W.y[i].tobytes() == (v[i] / th + a / (th * th)).tobytes()
            assert W0.y[i].tobytes() == (v[i] / th).tobytes()
        assert S.same_bits(W.y[~rows], V.y[~rows])
    for a1, a2 in ((c1, None), (None, c2), (c1, c2)):
        W = V.copy()
        S.gp_rhs(W, cols, rows, a1, a2)
        for i in np.nonzero(rows)[0]:
            rh = V.rhs[i]
            for cc in (a1, a2):
                if cc is not None:
                    cf = S.coef_t(cc, T, 4)
                    a = T(0)
                    for k in range(4):
                        a = a + cols[k][i] * cf[k]
                    rh = rh + (-a)
            assert W.rhs[i].tobytes() == rh.tobytes()
        assert S.same_bits(W.rhs[~rows], V.rhs[~rows])


@pytest.mark.parametrize("dt", DTYPES)
def test_fused_passes_equal_the_separate_statements(dt):
    """lbfgsx_b_solve_sweep(first = 1) = CB_SOLVE over F + the first sweep; (first = 0) + lbfgsx_b_lu_sweep = GP_RHS and CB_SOLVE
    over P, CB_LAMBDA over L, CB_MU over U, then a later sweep over F; the sums of the two calls add up"""
    V, cols, r = _vecs(500, dt, 7, 0, c=3)
    rng = np.random.default_rng(3)
    coef, coef2, coefm, c1, c2 = (0.3 * rng.standard_normal(6) for _ in range(5))
    theta = 1.3
    A = V.copy()
    sums, yd = S.solve_sweep(A, cols, 1, S.VS_NEG_CF, coef, theta)
    B = V.copy()
    S.wcombine(B, cols, S.CB_SOLVE, S.ST_FREE, S.VS_NEG_CF, coef, theta)
    z = np.zeros(V.n, V.dt)
    assert S.sweep(B, True, None, z, z) == sums and yd is None
    _same(A, B, "first")
    A2 = A.copy()
    listed = A.rows(S.ST_L | S.ST_U)
    s1, yd = S.solve_sweep(A2, cols, 0, S.VS_NEG_RHS, coef2, theta, c1, c2)
    s2 = S.lu_sweep(A2, cols, coefm, theta, listed)
    B2 = B.copy()
    S.gp_rhs(B2, cols, B2.rows(S.ST_P), c1, c2)
    S.wcombine(B2, cols, S.CB_SOLVE, S.ST_P, S.VS_NEG_RHS, coef2, theta)
    assert S.same_bits(yd, B2.y)
    S.wcombine(B2, cols, S.CB_LAMBDA, S.ST_L, S.VS_DRT, coefm, theta)
    S.wcombine(B2, cols, S.CB_MU, S.ST_U, S.VS_DRT, coefm, theta)
    tot = S.sweep(B2, False)
    assert [a + b for a, b in zip(s1, s2)] == tot and tot[4] + tot[5] + tot[6] > 0
    _same(A2, B2, "sweep")


# ---------------------------------------------------------------- a whole minimisation against the oracle
def _oracle_instances():
    import test_lbfgsb_gpu as TB
    mark = [m for m in TB.test_cauchy_and_subspace_match_oracle.pytestmark if m.name == "parametrize" and "mode" in m.args[0]][0]
    return TB, list(mark.args[1])


@pytest.mark.parametrize("k", range(6))
def test_whole_minimisation_matches_the_oracle(oracle, k):
    """the instances and the tolerance of test_cauchy_and_subspace_match_oracle (1e-9 max(1, |drt|_inf)), float64"""
    import oracle_lib as O
    if not oracle.supports_lbfgsb:
        pytest.skip("this oracle build has no L-BFGS-B entry points")
    TB, inst = _oracle_instances()
    assert len(inst) == 6
    n, m, npairs, mode = inst[k]
    rng = np.random.default_rng(100 + n + npairs)
    Sm, Ym, x0, g, lb, ub = TB._instance(rng, n, npairs, O.F64, mode)
    ref = oracle.cauchy_subspace(O.F64, m, Sm, Ym, x0, g, lb, ub, max_submin=10)
    free, newact = np.zeros(n, bool), np.zeros(n, bool)
    free[ref["fv"]] = True
    newact[ref["newact"]] = True
    drt, sweeps = S.minimize(F64, Sm, Ym, m, x0, ref["xcp"], g, lb, ub, free, newact, 10)
    scale = max(1.0, float(np.abs(ref["drt"]).max()))
    err = float(np.abs(drt - ref["drt"]).max())
    print("instance %r: %d sweeps, max |drt - oracle| = %.3g (scale %.3g)" % (inst[k], sweeps, err, scale))
    assert err <= 1e-9 * scale


# ---------------------------------------------------------------- coverage of the inputs
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("n", [255, 257, 511, 1025, 4097])
def test_generators_cover_every_edge_class(dt, n):
    """every n >= 255 the GPU file partitions: each edge class is present in the first input and in the shifted one, the two
    sweeps between them make every set change, and every kind of row exists"""
    r = S.build_rows(n, dt, n)
    assert set(np.unique(r["kind"])) == set(range(8))
    assert r["kind"][0] == S.K_FREE and r["kind"][-1] == S.K_FREE, "a dropped head or tail row must show"
    li, ui = r["lb"] - r["x0_sweep"], r["ub"] - r["x0_sweep"]
    assert np.array_equal(li[r["kind"] == S.K_EQ], ui[r["kind"] == S.K_EQ]) and (r["lb"] < r["ub"])[r["free"]].all()
    st = np.where(r["free"], S.ST_FREE, np.where(r["newact"], S.ST_NEWACT, 0)).astype(np.uint8)
    z = np.zeros(n, dt)
    for shift in (0, 7):
        y, lam, mu = S.edge_values(li, ui, r["free"], dt, shift, n)
        assert np.isfinite(y).all() and np.isfinite(lam).all() and np.isfinite(mu).all()
        missing = set(S.EDGE_LABELS) - S.edge_classes(li, ui, r["free"], y, lam, mu)
        assert not missing, "n = %d shift %d: no row of class %s" % (n, shift, sorted(missing))
    V = S.Vecs(dt, x0=r["x0_sweep"], g=r["g"], lb=r["lb"], ub=r["ub"], drt=z, cF=z, y=S.edge_values(li, ui, r["free"], dt, 0, n)[0], yfb=z,
               lam=z, mu=z, rhs=z, st=st)
    S.sweep(V, True, None, z, z)
    W = V.copy()
    y, lam, mu = S.edge_values(li, ui, r["free"], dt, 7, n)
    f = r["free"]
    W.y[f], W.lam[f], W.mu[f] = y[f], lam[f], mu[f]
    S.sweep(W, False)
    assert S.transitions(V.st, W.st) >= {"L->P", "U->P", "P->L", "P->U", "L->U"}


def test_break_points_put_the_rows_where_build_rows_says():
    """Cauchy.h:111-129 with t = 1: break point (x0 - bound) / g is >= 4 or infinite on the free kinds, <= 1 / 2 on the
    newly active ones, 0 on the fixed ones -- far from the crossing threshold 1 in both scalar types"""
    for dt in DTYPES:
        r = S.build_rows(3000, dt, 12)
        g, x0, lb, ub = (r[k].astype(F64) for k in ("g", "x0", "lb", "ub"))
        with np.errstate(divide="ignore", invalid="ignore"):
            brk = np.where(g < 0, (x0 - ub) / g, np.where(g > 0, (x0 - lb) / g, np.inf))
        assert (brk[r["free"]] >= 3.9).all() and (brk[r["newact"]] <= 0.51).all() and (brk[r["newact"]] > 0).all()
        brk[lb == ub] = 0.0
        assert (brk[r["kind"] == S.K_FIXED] == 0).all() and np.array_equal(lb == ub, r["kind"] == S.K_FIXED)
        assert np.array_equal(r["free"] | r["newact"], r["kind"] != S.K_FIXED)


def test_exact_row_counts_for_the_compact_copy():
    for n, nfree in ((6000, 4096), (8192, 7168), (8192, 7169)):
        r = S.build_rows(n, F64, 3, nfree=nfree)
        assert int(r["free"].sum()) == nfree and int(r["newact"].sum()) == n - nfree
    r = S.build_rows(999, F32, 3, free_all=True)
    assert not r["newact"].any()


def test_sentinels_are_distinct_and_finite():
    for dt, n in ((F32, 1 << 21), (F64, 1000)):
        for which in range(6):
            s = S.sentinel(which, n, dt)
            assert np.isfinite(s).all() and np.unique(s).size == n
