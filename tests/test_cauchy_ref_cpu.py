"""CPU suite: tests/cauchy_ref.py is proved here before tests/test_cauchy_statements_gpu.py relies on it.
  * the vectorised build and finish equal a scalar, row-by-row transcription of Cauchy.h:111-129 and :201-206,219-233,265-282
    bit for bit on edge_rows (every class of the issue; with and without the clamp of LBFGSB.h:240), and the inputs do what
    their labels say (a quotient that underflows to a subnormal IS subnormal, and so on);
  * build + order + search + finish agree with the oracle's cauchy_subspace(subspace=False) on the instances of
    test_cauchy_and_subspace_match_oracle: the same sets on every instance.  Without pairs (no M) the search is a fixed
    sequence of IEEE operations and cauchy_ref.whole_search gives the oracle's xcp BIT FOR BIT, in f64 at every hand-over
    point and in f32 for the host form.  With pairs the exact search runs with M = Minv^-1 formed in 400-bit arithmetic, and
    xcp is held to 1e-12 max(1, |xcp|_inf), not to scan_bound, because no bound on the ORACLE's side can be derived from
    outside it: scan_bound covers the device's operations for a given M, while the oracle applies M through the reference's
    Bunch-Kaufman factorisation of Minv at every crossing.  The backward error of that solve is p(k) u (1 + 36 k rho_k) |Minv|
    (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorems 11.3 and 11.4) with the growth factor rho_k of
    the pivots it chose, which it does not report and which a priori is only known to be below 2.57^(k-1), i.e. 1e6 at
    2c = 16; and Minv's entries are the oracle's own rounded sums.  A term built on that would exceed 1e-12 by orders of
    magnitude, so the figure stays, stated as what it is: the tolerance of the existing whole-search comparison;
  * scan_emulate lies inside scan_bound of search_exact for every committed scan case, both chains;
  * each wrong variant of scan_emulate falls outside the bound or moves the exit on at least one committed case;
  * the condition the GPU test depends on: at every group end up to and including the exit, the exact margin exceeds
    cauchy_ref.FACTOR = 4 times the bound on -f'/f''."""
from fractions import Fraction

import numpy as np
import pytest

import cauchy_ref as G
import subspace_ref as S

F64, F32 = np.float64, np.float32
DTYPES = [F64, F32]


# ---------------------------------------------------------------- scalar transcription
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("n", [7, 64, 257, G.EDGE_NEED + 300])
def test_build_equals_the_scalar_transcription(dt, force, n):
    r = G.edge_rows(n, dt, 3)
    x = r["x_out"] if force else r["x"]
    b = G.build(x, r["g"], r["lb"], r["ub"], force)
    xo, brk, d, fv, ordr = G.build_scalar(x, r["g"], r["lb"], r["ub"], force)
    assert G.same_bits(b.x, xo) and G.same_bits(b.brk, brk) and G.same_bits(b.d, d) and G.same_bits(b.xcp, xo)
    assert (b.nfree, b.nord) == (len(fv), len(ordr))
    assert np.array_equal(np.nonzero(b.isord)[0], ordr)
    assert G.same_bits(b.x, r["x"]), "the clamp puts x_out on x"
    if force:
        assert b.moved == min(4, max(0, n - 20))
    # the order: the candidates by (break point, row)
    o = G.order(b.brk)
    want = sorted(ordr, key=lambda i: (b.brk[i], i))
    assert o.tolist() == want
    assert (b.brk >= 0).all(), "inside the box every break point is >= 0"
    keys = G.build(x, r["g"], r["lb"], r["ub"], force).keys
    assert G.same_bits(keys[b.isord], b.brk[b.isord]) and np.isinf(keys[~b.isord]).all()
    for tau in (0.0, float(b.brk[o[0]]) if o.size else 1.0, 0.25, 1e30):
        p = G.prefix(b.brk, tau)
        assert p.tolist() == [i for i in want if b.brk[i] <= dt(tau)]


@pytest.mark.parametrize("dt", DTYPES)
def test_edge_rows_hold_every_class(dt):
    n = G.EDGE_NEED + 300
    r = G.edge_rows(n, dt, 3)
    b = G.build(r["x"], r["g"], r["lb"], r["ub"])
    got = G.edge_classes(r, b)
    for lab, kind in G.EXPECT.items():
        assert got[lab] == {kind}, "%s: break point class %r, expected %s" % (lab, got[lab], kind)
    lo, hi = b.brk[r["label"] == "ulp lo"][0], b.brk[r["label"] == "ulp hi"][0]
    assert np.nextafter(lo, dt(1)) == hi
    for gi, (size, kind) in enumerate(G.GROUPS):
        rows = np.nonzero(r["label"] == "tie%d" % gi)[0]
        assert rows.size == size and len({b.brk[i].tobytes() for i in rows}) == 1, "group %d is not one break point" % gi
        assert (len(set(r["g"][rows].tolist())) == 1) == (kind == "eq")
        assert (np.diff(rows) != 1).any() or size == 2, "a group's rows are scattered"
    # a smaller n keeps the classes that fit
    small = G.edge_rows(30, dt, 3)
    assert set(small["label"]) - {""} >= set(G.SINGLE_LABELS)
    assert np.isfinite(float(b.dd_exact)) and float(b.dd_exact) < float(np.finfo(dt).max)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("crossed_all", [0, 1])
def test_finish_equals_the_scalar_transcription(dt, crossed_all):
    r = G.edge_rows(G.EDGE_NEED + 300, dt, 5)
    b = G.build(r["x"], r["g"], r["lb"], r["ub"])
    tie = float(b.brk[r["label"] == "tie5"][0])
    for tc in (0.0, tie, float(np.nextafter(dt(tie), dt(0))), float(np.nextafter(dt(tie), dt(1))), 1e-42, 1e30):
        for tf in (0.0, 0.1, 0.3):
            f = G.finish(b.brk, b.x, b.d, r["lb"], r["ub"], tc, tf, crossed_all)
            xcp, st = G.finish_scalar(b.brk, b.x, b.d, r["lb"], r["ub"], tc, tf, crossed_all)
            assert G.same_bits(f["xcp"], xcp) and np.array_equal(f["st"], st)
            assert f["nact"] == int((st == G.ST_NEWACT).sum()) and f["nfree"] == int((st == G.ST_FREE).sum())
            with np.errstate(all="ignore"):
                assert G.same_bits(f["drt"], (xcp - b.x).astype(dt))
    # the whole group is inside at its break point and outside one ulp below
    grp = r["label"] == "tie5"
    at = G.finish(b.brk, b.x, b.d, r["lb"], r["ub"], tie, 0.1, 0)["st"][grp]
    below = G.finish(b.brk, b.x, b.d, r["lb"], r["ub"], float(np.nextafter(dt(tie), dt(0))), 0.1, 0)["st"][grp]
    assert (at == G.ST_NEWACT).all() and (below == G.ST_FREE).all()


# ---------------------------------------------------------------- the oracle
def _oracle_instances():
    import test_lbfgsb_gpu as TB
    mark = [m for m in TB.test_cauchy_and_subspace_match_oracle.pytestmark if m.name == "parametrize" and "mode" in m.args[0]][0]
    return TB, list(mark.args[1])


@pytest.mark.parametrize("k", range(6))
def test_search_matches_the_oracle(oracle, k):
    import oracle_lib as O
    if not oracle.supports_lbfgsb:
        pytest.skip("this oracle build has no L-BFGS-B entry points")
    TB, inst = _oracle_instances()
    assert len(inst) == 6
    n, m, npairs, mode = inst[k]
    rng = np.random.default_rng(100 + n + npairs)
    Sm, Ym, x0, g, lb, ub = TB._instance(rng, n, npairs, O.F64, mode)
    ref = oracle.cauchy_subspace(O.F64, m, Sm, Ym, x0, g, lb, ub, subspace=False)
    cols, theta, Minv = S.bfgs_mats(Sm, Ym, m)
    nc2 = len(cols)
    M = np.linalg.inv(Minv) if nc2 else np.zeros((0, 0))
    Mx = M
    if nc2:     # the inverse of these doubles in 400-bit arithmetic, as rationals
        import mpmath
        with mpmath.workprec(400):
            Mm = mpmath.matrix(Minv.tolist()) ** -1
            Mx = [[Fraction(*mpmath.libmp.to_rational(Mm[i, j]._mpf_)) for j in range(nc2)] for i in range(nc2)]
    b = G.build(x0, g, lb, ub)
    o = G.order(b.brk)
    ga = G.gather(o, b.brk, b.x, g, b.d, lb, ub, cols)
    p = np.array([np.dot(c, b.d) for c in cols])
    p[nc2 // 2:] *= theta
    f1 = -float(np.dot(b.d, b.d))
    f2 = -theta * f1 - float(p @ M @ p) if nc2 else -theta * f1
    state = np.concatenate((p, np.zeros(nc2), [f1, f2]))
    crossed_all, e = False, -1
    if o.size and -f1 / f2 >= ga["brk"][0]:
        ex = G.search_exact(ga["brk"], ga["g"], ga["z"], ga["w"], Mx, theta, state, 0.0)
        e = ex["exit"] if ex["exit"] >= 0 else o.size - 1
        crossed_all = ex["exit"] < 0 and b.nfree == 0
        f1, f2 = float(ex["f1"][e]), float(ex["f2"][e])
    il = float(ga["brk"][e]) if e >= 0 else 0.0
    dtm = -f1 / f2 if f2 >= np.finfo(F64).eps else -f1 / np.finfo(F64).eps
    tfinal = il + max(dtm, 0.0)
    f = G.finish(b.brk, b.x, b.d, lb, ub, il, tfinal, crossed_all)
    free, newact = np.zeros(n, bool), np.zeros(n, bool)
    free[ref["fv"]] = True
    newact[ref["newact"]] = True
    print("instance %r: %d of %d crossed" % (inst[k], e + 1, o.size))
    assert np.array_equal(f["st"] == G.ST_NEWACT, newact) and np.array_equal(f["st"] == G.ST_FREE, free)
    # the oracle made them active in the order of the break points; inside a group of ties its sort (std::sort, not stable)
    # leaves any order, the device's is by row
    na = ref["newact"]
    assert (np.diff(b.brk[na]) >= 0).all() and na[np.lexsort((na, b.brk[na]))].tolist() == o[:e + 1].tolist()
    assert np.abs(f["xcp"] - ref["xcp"]).max() <= 1e-12 * max(1.0, np.abs(ref["xcp"]).max())
    if nc2 == 0:
        assert G.same_bits(G.whole_search(x0, g, lb, ub, -1)["xcp"], ref["xcp"]), "without pairs the oracle's xcp is reproducible"


# ---------------------------------------------------------------- emulation, bound, mutations, margins
_CASES = G.scan_cases()
_MEMO = {}


def _solved(cs):
    """(lists, exact search, bound per chain) of a case, computed once"""
    if cs.name not in _MEMO:
        b, o, ga = cs.lists()
        cnt = cs.count
        nxt = ga["brk"][cnt] if o.size > cnt else None
        args = (ga["brk"][:cnt], ga["g"][:cnt], ga["z"][:cnt], ga["w"][:cnt], cs.M, cs.theta, cs.state, cs.t_prev, nxt)
        ex = G.search_exact(*args)
        upto = ex["exit"] if ex["exit"] >= 0 else cnt - 1
        bd = {ch: G.scan_bound(*args, cs.dtype, ex, upto, chain=ch) for ch in ("host", "scan")}
        _MEMO[cs.name] = (b, o, ga, args, ex, upto, bd)
    return _MEMO[cs.name]


def _inside(em, ex, upto, bd):
    """is the emulated state within the bound of the exact one after crossing upto?"""
    if em["exit"] != ex["exit"]:
        return False
    ok = abs(Fraction(em["f1"]) - ex["f1"][upto]) <= bd["f1"] and abs(Fraction(em["f2"]) - ex["f2"][upto]) <= bd["f2"]
    for j in range(len(em["p"])):
        ok = ok and abs(Fraction(float(em["p"][j])) - ex["p"][upto][j]) <= bd["p"][j]
        ok = ok and abs(Fraction(float(em["c"][j])) - ex["c"][upto][j]) <= bd["c"][j]
    return ok


@pytest.mark.parametrize("cs", _CASES, ids=lambda c: c.name)
def test_designed_exit_and_margins(cs):
    """the case does what it was designed to do, and every exit decision is FACTOR x clear of the bound (both chains)"""
    b, o, ga, args, ex, upto, bd = _solved(cs)
    assert o.size == cs.n - 3
    if cs.exit_at is None:      # tieflip: f' is positive inside the first group and negative at its end; the exit comes later
        assert ex["f1"][0] > 0 and ex["f1"][1] < 0 and 0 not in ex["margin"] and ex["margin"][1] > 0 and ex["exit"] > 1
    else:
        assert ex["exit"] == cs.exit_at
    assert len(ex["margin"]) >= 1 or cs.name.startswith("listend")
    for ch in ("host", "scan"):
        if ex["margin"]:
            ratio = G.min_margin_ratio(ex, bd[ch])
            print("%s %s: smallest margin / bound = %.3g" % (cs.name, ch, ratio))
            assert ratio >= G.FACTOR


@pytest.mark.parametrize("chain", ["host", "scan"])
@pytest.mark.parametrize("cs", _CASES, ids=lambda c: c.name)
def test_emulation_lies_inside_the_bound(cs, chain):
    b, o, ga, args, ex, upto, bd = _solved(cs)
    em = G.scan_emulate(*args, cs.dtype, chain=chain)
    assert em["exit"] == ex["exit"]
    assert em["brk"] == ga["brk"][upto]
    assert _inside(em, ex, upto, bd[chain])
    # the bound is not vacuous: it is far below the state it bounds
    assert bd[chain]["f1"] <= 1e-3 * abs(float(ex["f1"][upto])) + 1e-3 and bd[chain]["f2"] <= 1e-3 * abs(float(ex["f2"][upto]))


@pytest.mark.parametrize("mutate", ["theta_s", "drop_p", "drop_tile1", "dt_tprev", "exit_in_tie", "z_wrong"])
def test_wrong_variants_are_caught(mutate):
    caught = []
    for cs in _CASES:
        b, o, ga, args, ex, upto, bd = _solved(cs)
        for chain in ("host", "scan"):
            if mutate == "z_wrong":        # the other bound's distance
                bad = G.gather(o, b.brk, b.x, cs.g, -b.d, cs.lb, cs.ub, cs.cols)["z"][:cs.count]
                em = G.scan_emulate(args[0], args[1], bad, *args[3:], cs.dtype, chain=chain)
            else:
                em = G.scan_emulate(*args, cs.dtype, chain=chain, mutate=mutate)
            if not _inside(em, ex, upto, bd[chain]):
                caught.append((cs.name, chain))
    assert caught, "no committed case notices the variant %s" % mutate
    print("%s: caught by %d of %d runs" % (mutate, len(caught), 2 * len(_CASES)))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("count", [1, 2, 65, 257, 513])
def test_no_pair_scan_is_two_ieee_chains(dt, count):
    """without stored pairs the emulation is the plain statement of Cauchy.h:218,227-228,240 in the chain's type"""
    cs = G.ScanCase("n", dt, 0, count, count // 2, 7, extra=3)
    b, o, ga = cs.lists()
    nxt = ga["brk"][count] if o.size > count else None
    em = G.scan_emulate(ga["brk"][:count], ga["g"][:count], ga["z"][:count], ga["w"][:count], cs.M, cs.theta, cs.state, 0.0, nxt, dt)
    CT = dt
    f1, f2, prev, e = CT(cs.state[0]), CT(cs.state[1]), 0.0, -1
    th = cs.theta
    for k in range(count):
        gk, zk = ga["g"][k], ga["z"][k]
        f1 = f1 + CT(ga["brk"][k] - prev) * f2
        f1 = f1 + CT(gk * gk + th * gk * zk - gk * 0.0)
        f2 = f2 - CT(th * (gk * gk) + 2 * gk * 0.0 + (gk * gk) * 0.0)
        prev = ga["brk"][k]
        dn = CT(ga["brk"][k + 1] - prev)
        if dn > 0 and not (-f1 / f2 >= dn):
            e = k
            break
    assert e == em["exit"] == count // 2
    assert float(f1) == em["f1"] and float(f2) == em["f2"]


def test_whole_search_matches_the_oracle(oracle):
    """the search without pairs, composed of the scalar loop and the emulated device search, against the oracle (float64)"""
    import oracle_lib as O
    if not oracle.supports_lbfgsb:
        pytest.skip("this oracle build has no L-BFGS-B entry points")
    TB, inst = _oracle_instances()
    n, m, npairs, mode = inst[0]
    assert npairs == 0
    rng = np.random.default_rng(100 + n + npairs)
    Sm, Ym, x0, g, lb, ub = TB._instance(rng, n, npairs, O.F64, mode)
    ref = oracle.cauchy_subspace(O.F64, m, Sm, Ym, x0, g, lb, ub, subspace=False)
    free, newact = np.zeros(n, bool), np.zeros(n, bool)
    free[ref["fv"]] = True
    newact[ref["newact"]] = True
    for dev_min in (-1, 0, 300):
        w = G.whole_search(x0, g, lb, ub, dev_min)
        assert w["crossings"] == ref["newact"].size > 300
        assert np.array_equal(w["st"] == G.ST_NEWACT, newact) and np.array_equal(w["st"] == G.ST_FREE, free)
        assert G.same_bits(w["xcp"], ref["xcp"]), "hand-over at %d: xcp differs from the oracle's in rows %s" % (
            dev_min, G.diff_rows(w["xcp"], ref["xcp"])[:8])
    # float: the host form is the reference's own float arithmetic
    Sm, Ym, x0, g, lb, ub = TB._instance(np.random.default_rng(5), 2000, 0, O.F32, "edge")
    ref = oracle.cauchy_subspace(O.F32, m, Sm, Ym, x0, g, lb, ub, subspace=False)
    w = G.whole_search(x0, g, lb, ub, -1)
    assert w["crossings"] == ref["newact"].size > 300 and G.same_bits(w["xcp"], ref["xcp"])


@pytest.mark.parametrize("dt", DTYPES)
def test_whole_search_hand_over_changes_nothing_in_double(dt):
    """in double the device search's chains are the host loop's own operations: any hand-over point gives the same bits; in
    float the per-crossing terms are computed in double first (the library's documented departure), so only the sets agree"""
    r = G.edge_rows(900, dt, 81, extreme=False)
    res = [G.whole_search(r["x"], r["g"], r["lb"], r["ub"], dm) for dm in (-1, 0, 7)]
    assert res[0]["crossings"] > 100
    for q in res[1:]:
        assert q["crossings"] == res[0]["crossings"] and np.array_equal(q["st"], res[0]["st"])
        if dt == F64:
            assert G.same_bits(q["xcp"], res[0]["xcp"])
