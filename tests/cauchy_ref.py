"""Reference of the generalized-Cauchy-point search (Cauchy.h:93-284) as the device states it, for
tests/test_cauchy_statements_gpu.py; proved by tests/test_cauchy_ref_cpu.py.

Element-wise statements (build, finish, gather) are plain numpy in the problem's dtype, one numpy operation per operation of
the kernel (k_cauchy_build / k_b_post_build, k_cauchy_finish, k_cauchy_gather / k_gcp_gather in csrc/lbfgsb_kernels.cuh and
csrc/gcp_scan.cuh; the library is built without contraction, so a * b + c is two roundings there as here).  The order of the
sorts is (break point, row).  The recurrences of the search (gcp_scan.cuh's header, Cauchy.h:183-256) are exact rationals
(search_exact); scan_emulate performs the kernels' own floating-point operations in the kernels' own order; scan_bound bounds
the difference between the two from that order.  Finite inputs apart from infinite bounds: NaN handling is out of scope.

scan_bound: the derivation
--------------------------
u = 2^-53 (every device operation of the search is a double operation, for f32 problems too: the sorted list is gathered into
doubles), uT = the unit roundoff of the host chain's type (2^-53, or 2^-24 when an f32 problem runs the default chain),
gam(k, v) = k v / (1 - k v).  A sum of terms whose longest path has D additions, formed from terms that carry r roundings of
their own, is off its exact value by at most gam(D + r, u) * sum|terms| (Higham, Accuracy and Stability, section 4.2: any
order of summation; the bound only counts the additions a term passes through).

  tile scan   a value of tile t passes through: 6 additions of the Hillis-Steele steps inside its wavefront (offsets 1..32), at
              most 3 of the wave totals left to right plus the addition of that prefix, 1 of the tile offset, and t + 1 of
              k_gcp_tiles' left-to-right chain (the seed is the chain's first term): D(t) = 11 + t + 1.  With T tiles every
              value has D <= DS = 12 + T.
  p           term g * w with w = W (y half) or W * theta (s half, one rounding), product rounded once: r = 2.  The state
              handed back is P[e] + g * w: one more addition.  Ep_k[j] = gam(DS + 3, u) * (|p_in[j]| + sum_{i <= k} |g_i w_ij|)
              bounds both p_{k-1} as stored and p_k as returned (the sums of absolute values are monotone in k).
  c           term dt_k * p_{k-1}: dt_k = brk_k - brk_{k-1} rounded once, the product once, on a p that is itself off by Ep:
              |term - exact| <= dt (2 u + 3 u^2)(|p| + Ep) + dt Ep, and the scan adds gam(DS, u) * (|c_in| + sum|terms|):
              Ec_k[j] = gam(DS, u) * (|c_in[j]| + Sc) + 1.000001 * (2.000001 u Sc + sum_{i <= k} dt_i Ep_i[j]),
              Sc = sum_{i <= k} dt_i (|p_{i-1}[j]| + Ep_i[j]).
  (M w)_i     NC products of M_ij and w_j (w_j carries one rounding) summed left to right: nc2 + 1 roundings on the longest
              path (padding adds exact zeros): |u_i - (M w)_i| <= Eu_i = gam(nc2 + 2, u) * Ua_i,  Ua_i = sum_j |M_ij| |w_j|.
  dots        d = sum_i u_i v_i left to right over nc2 terms, v = c_k, p_{k-1} or w, v off by Ev:
              |d - exact| <= gam(nc2 + 1, u) * sum_i (Ua_i + Eu_i)(|v_i| + Ev_i) + sum_i (Eu_i (|v_i| + Ev_i) + Ua_i Ev_i).
              (|(M w)_i| <= Ua_i is used for the magnitude: looser than the value, never smaller.)
  B_k         theta g^2 + 2 g d_p + g^2 d_w: at most 4 roundings on any term's path:
              EB_k = gam(4, u) * (theta g^2 + 2 |g| (|d_p| + Edp) + g^2 (|d_w| + Edw)) + 2 |g| Edp + g^2 Edw.
  A_k         g^2 + theta g z - g d_c: likewise EA_k = gam(4, u) * (g^2 + theta |g z| + |g| (|d_c| + Edc)) + |g| Edc.
              z is the gathered double of the T-rounded bound - x0, the same number on both sides: no error of its own.
  f''         host chain: f2 <- f2 - CT(B_k), left to right from CT(f2_in): k + 1 subtractions and two conversions:
              Ef2_k = gam(k + 3, uT) * (|f2_in| + sum_{i <= k} (|B_i| + EB_i)) + sum_{i <= k} EB_i.
              scan chain: the same with gam(DS + 1, u): the increments are negated (exact) and summed by the tile scan.
  f'          host chain: f1 <- f1 + CT(dt) * f2; f1 <- f1 + CT(A_k): 2 (k + 1) additions, the product and the conversions
              (of dt, of A_k, of f1_in) at most four roundings more:
              Ef1_k = gam(2 k + 6, uT) * (|f1_in| + sum_{i <= k} (dt_i (|f2_{i-1}| + Ef2_{i-1}) + |A_i| + EA_i))
                      + sum_{i <= k} (dt_i Ef2_{i-1} + EA_i).
              scan chain: increment dt * f2_{k-1} + A_k (3 roundings) summed by the tile scan: gam(DS + 3, u) in place of
              gam(2 k + 6, uT).
  -f'/f''     Eq_k = ((Ef1 + |q| Ef2) / (|f2| - Ef2)) * (1 + 2 uT) + 2 uT (|q| + dnext), q = f'/f'' exact: the division and
              the conversion of the next interval to CT round once each; needs Ef2 < |f2| (asserted).
  calls > 1   a search continued over several calls of lbfgsx_b_cauchy_scan (state_in and t_prev from the call before): a value
              passes through the additions of every call it lives through, each at most 12 + T + 3 with the T of the whole
              range (a call's range has no more tiles), so DS + 3 becomes calls * (15 + T); the host chains go on left to right
              as before and each further call converts the state once more (3 roundings allowed per further call).
All sums of absolute values use the EXACT p, c, f', f'' of search_exact (rounded up into doubles with a factor 1 + 2^-40, which
also covers the double arithmetic of the bound's own evaluation).  No constant is fitted to any device output."""
from fractions import Fraction

import numpy as np

import statement_ref as R

ST_FREE, ST_NEWACT = 1, 2
CV_BRK, CV_DVEC, CV_VALS_OUT = 0, 1, 2
TILE = 256


def _T(dtype):
    return np.dtype(dtype).type


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def diff_rows(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    ui = {4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize]
    return np.nonzero(a.view(ui) != b.view(ui))[0]


# ---------------------------------------------------------------- element-wise statements
def clamp(x, lb, ub):
    """x.cwiseMax(lb).cwiseMin(ub) as the kernels state it (LBFGSB.h:240)"""
    v = np.where(x < lb, lb, x)
    return np.where(ub < v, ub, v)


class Build:
    pass


def build(x, g, lb, ub, force=False):
    """k_cauchy_build's row statement (Cauchy.h:95,111-129): x (clamped when force), brk, d, xcp = x0, the sort keys, the
    counts and the exact d.d"""
    T = x.dtype.type
    assert g.dtype == lb.dtype == ub.dtype == x.dtype
    inf = T(np.inf)
    b = Build()
    b.x = clamp(x, lb, ub) if force else x.copy()
    with np.errstate(all="ignore"):
        tu = (b.x - ub) / g
        tl = (b.x - lb) / g
    b.brk = np.where(lb == ub, T(0), np.where(g < T(0), tu, np.where(g > T(0), tl, inf))).astype(T)
    iszero = b.brk == T(0)
    b.d = np.where(iszero, T(0), -g).astype(T)
    b.xcp = b.x.copy()
    isfree = b.brk == inf
    b.isord = ~isfree & ~iszero
    b.keys = np.where(b.isord, b.brk, inf).astype(T)
    b.nfree, b.nord = int(isfree.sum()), int(b.isord.sum())
    b.dd_exact = R.exact_dot(b.d, b.d)
    b.dd_abs = b.dd_exact
    b.moved = int((~(b.x == x)).sum())
    return b


def build_scalar(x, g, lb, ub, force=False):
    """the same row by row: a transcription of Cauchy.h:111-129 (and LBFGSB.h:240 when force) with numpy scalars"""
    T = x.dtype.type
    n = x.size
    inf = T(np.inf)
    xo, brk, d = x.copy(), np.empty(n, T), np.empty(n, T)
    fv, ordr = [], []
    with np.errstate(all="ignore"):
        for i in range(n):
            if force:
                xo[i] = min(max(xo[i], lb[i]), ub[i]) if not (xo[i] != xo[i]) else xo[i]
            if lb[i] == ub[i]:
                brk[i] = T(0)
            elif g[i] < T(0):
                brk[i] = (xo[i] - ub[i]) / g[i]
            elif g[i] > T(0):
                brk[i] = (xo[i] - lb[i]) / g[i]
            else:
                brk[i] = inf
            iszero = brk[i] == T(0)
            d[i] = T(0) if iszero else -g[i]
            if brk[i] == inf:
                fv.append(i)
            elif not iszero:
                ordr.append(i)
    return xo, brk, d, fv, ordr


def order(brk):
    """the rows with 0 < brk < inf sorted by (brk, row)"""
    rows = np.nonzero((brk != 0) & (brk != np.inf))[0]
    return rows[np.lexsort((rows, brk[rows]))].astype(np.int64)


def prefix(brk, tau):
    """order(brk) restricted to brk <= T(tau)"""
    o = order(brk)
    return o[brk[o] <= brk.dtype.type(tau)]


def gather(o, brk, x0, g, d, lb, ub, cols=()):
    """k_cauchy_gather: brk, g, z = T(bound - x0) with the bound chosen by d > 0, idx and the W rows [y.., s..], as doubles"""
    T = x0.dtype.type
    with np.errstate(all="ignore"):
        z = (np.where(d[o] > T(0), ub[o], lb[o]) - x0[o]).astype(T)
    w = np.stack([np.asarray(c)[o].astype(np.float64) for c in cols], axis=1) if len(cols) else np.zeros((o.size, 0))
    return dict(brk=brk[o].astype(np.float64), g=g[o].astype(np.float64), z=z.astype(np.float64), idx=o.astype(np.int32), w=w)


def finish(brk, x0, d, lb, ub, t_cross, tfinal, crossed_all):
    """k_cauchy_finish's row statement (Cauchy.h:201-206,219-233,265-282)"""
    T = x0.dtype.type
    tc, tf = T(t_cross), T(tfinal)
    zero = brk == T(0)
    act = ~zero & (brk <= tc)
    free = ~zero & ~act
    xcp = x0.copy()
    xcp[act] = np.where(d > T(0), ub, lb)[act]
    if not crossed_all:
        with np.errstate(all="ignore"):
            xcp[free] = (x0 + tf * d).astype(T)[free]
    with np.errstate(all="ignore"):
        drt = (xcp - x0).astype(T)
    st = np.where(act, ST_NEWACT, np.where(free, ST_FREE, 0)).astype(np.uint8)
    return dict(xcp=xcp, drt=drt, st=st, nact=int(act.sum()), nfree=int(free.sum()), newact=np.nonzero(act)[0])


def finish_scalar(brk, x0, d, lb, ub, t_cross, tfinal, crossed_all):
    T = x0.dtype.type
    tc, tf = T(t_cross), T(tfinal)
    xcp, st = x0.copy(), np.zeros(x0.size, np.uint8)
    with np.errstate(all="ignore"):
        for i in range(x0.size):
            if brk[i] == T(0):
                continue
            if brk[i] <= tc:
                xcp[i] = ub[i] if d[i] > T(0) else lb[i]
                st[i] = ST_NEWACT
            else:
                if not crossed_all:
                    xcp[i] = x0[i] + tf * d[i]
                st[i] = ST_FREE
    return xcp, st


# ---------------------------------------------------------------- the exact search
def _F(x):
    return x if isinstance(x, Fraction) else Fraction(float(x))


def search_exact(brk, g, z, w, M, theta, state, t_prev, brk_next=None, stop=True):
    """Cauchy.h:183-256 over the sorted crossings brk[0..count) in exact rationals.  w: count x 2c un-scaled rows [y.., s..];
    M[i][j]: the 2c x 2c matrix; state = [p (2c), c (2c), f', f'']; brk_next: the break point after the range (None at the end
    of the list).  Returns the states after every crossing (lists of Fractions), the margin (-f'/f'') - (brk_{k+1} - brk_k) at
    every group end that has a successor (dict k -> Fraction) and `exit`, the first group end with a negative margin (-1:
    none).  stop: do not walk on behind the exit."""
    count = len(brk)
    nc2 = len(state) // 2 - 1
    nc = nc2 // 2
    th = _F(theta)
    p = [_F(v) for v in state[:nc2]]
    c = [_F(v) for v in state[nc2:2 * nc2]]
    f1, f2 = _F(state[2 * nc2]), _F(state[2 * nc2 + 1])
    Mq = [[_F(M[i][j]) for j in range(nc2)] for i in range(nc2)]
    out = dict(p=[], c=[], f1=[], f2=[], margin={}, exit=-1)
    prev = _F(t_prev)
    for k in range(count):
        bk, gk, zk = _F(brk[k]), _F(g[k]), _F(z[k])
        dt = bk - prev
        assert dt >= 0
        wk = [_F(w[k][j]) * (th if j >= nc else 1) for j in range(nc2)]
        u = [sum(Mq[i][j] * wk[j] for j in range(nc2)) for i in range(nc2)]
        c = [c[j] + dt * p[j] for j in range(nc2)]
        f1 = f1 + dt * f2 + gk * gk + th * gk * zk - gk * sum(u[i] * c[i] for i in range(nc2))
        f2 = f2 - (th * gk * gk + 2 * gk * sum(u[i] * p[i] for i in range(nc2)) + gk * gk * sum(u[i] * wk[i] for i in range(nc2)))
        p = [p[j] + gk * wk[j] for j in range(nc2)]
        prev = bk
        out["p"].append(p)
        out["c"].append(c)
        out["f1"].append(f1)
        out["f2"].append(f2)
        nxt = _F(brk[k + 1]) if k + 1 < count else (None if brk_next is None else _F(brk_next))
        if nxt is not None and nxt > bk:
            assert f2 != 0
            out["margin"][k] = -f1 / f2 - (nxt - bk)
            if out["margin"][k] < 0 and out["exit"] < 0:
                out["exit"] = k
                if stop:
                    break
    return out


# ---------------------------------------------------------------- the kernels' own operations
def _tile_scan(v):
    """block_scan / wave_scan_x + wave_prefix_x over tiles of 256: (wave-inclusive, wave-exclusive, add of the wave, tile total),
    each ntiles x 4 x 64 (add: ntiles x 4, total: ntiles)"""
    count = v.size
    nt = (count + TILE - 1) // TILE
    x = np.zeros(nt * TILE)
    x[:count] = v
    x = x.reshape(nt, 4, 64)
    for off in (1, 2, 4, 8, 16, 32):
        y = x.copy()
        y[..., off:] = x[..., off:] + x[..., :-off]
        x = y
    ex = np.zeros_like(x)
    ex[..., 1:] = x[..., :-1]
    tot = x[..., 63]
    add = np.zeros((nt, 4))
    run = np.zeros(nt)
    for wv in range(4):
        add[:, wv] = run
        run = run + tot[:, wv]
    return x, ex, add, run


def _offsets(ts, init, drop_tile=None):
    """k_gcp_tiles: init + the totals of the tiles before, left to right"""
    ts = np.array(ts, np.float64)
    if drop_tile is not None and drop_tile < ts.size:
        ts[drop_tile] = 0.0
    return np.cumsum(np.concatenate(([init], ts)))[:-1]


def _flat(a, count):
    return a.reshape(-1)[:count]


def scan_emulate(brk, g, z, w, M, theta, state, t_prev, brk_next, dtype, chain="host", mutate=None):
    """lbfgsx_b_cauchy_scan's floating-point operations in the kernels' order (k_gcp_a1 .. k_gcp_extract, gcp_chain_host) in
    numpy f64; the host chain of an f32 problem in float.  Arguments as search_exact (doubles).  mutate: a wrong variant
    for tests/test_cauchy_ref_cpu.py ("theta_s", "drop_p", "drop_tile1", "dt_tprev", "exit_in_tie")."""
    brk, g, z = (np.asarray(a, np.float64) for a in (brk, g, z))
    count = brk.size
    nc2 = len(state) // 2 - 1
    nc = nc2 // 2
    w = np.asarray(w, np.float64).reshape(count, nc2)
    M = np.asarray(M, np.float64).reshape(nc2, nc2)
    tile = np.arange(count) // TILE
    wave = (np.arange(count) % TILE) // 64
    ws = w.copy()
    if mutate != "theta_s":
        ws[:, nc:] = ws[:, nc:] * theta
    dt = np.empty(count)
    dt[0] = brk[0] - t_prev
    dt[1:] = brk[1:] - (t_prev if mutate == "dt_tprev" else brk[:-1])
    pprev, ck = np.zeros((count, nc2)), np.zeros((count, nc2))
    for j in range(nc2):
        a = g * ws[:, j]
        if mutate == "drop_p" and count > 1:
            a[count // 3] = 0.0
        inc, ex, add, tot = _tile_scan(a)
        off = _offsets(tot, state[j], 1 if mutate == "drop_tile1" else None)
        pprev[:, j] = off[tile] + (add[tile, wave] + _flat(ex, count))
        inc, ex, add, tot = _tile_scan(dt * pprev[:, j])
        off = _offsets(tot, state[nc2 + j])
        ck[:, j] = off[tile] + (add[tile, wave] + _flat(inc, count))
    d_c, d_p, d_w = np.zeros(count), np.zeros(count), np.zeros(count)
    for i in range(nc2):
        u = np.zeros(count)
        for j in range(nc2):
            u = u + M[i, j] * ws[:, j]
        d_c = d_c + u * ck[:, i]
        d_p = d_p + u * pprev[:, i]
        d_w = d_w + u * ws[:, i]
    gg = g * g
    A = g * g + theta * g * z - g * d_c
    B = theta * gg + 2 * g * d_p + gg * d_w
    dnext = np.full(count, -1.0)
    dnext[:-1] = brk[1:] - brk[:-1]
    if brk_next is not None:
        dnext[-1] = brk_next - brk[-1]
    f1_in, f2_in = float(state[2 * nc2]), float(state[2 * nc2 + 1])
    e = -1
    if chain == "host":
        CT = np.float32 if np.dtype(dtype) == np.float32 else np.float64
        f1s, f2s = np.empty(count), np.empty(count)
        if CT is np.float64:
            f1, f2 = f1_in, f2_in
            dtl, Al, Bl, dnl = dt.tolist(), A.tolist(), B.tolist(), dnext.tolist()
            with np.errstate(all="ignore"):
                for k in range(count):
                    f1 = f1 + dtl[k] * f2
                    f1 = f1 + Al[k]
                    f2 = f2 - Bl[k]
                    f1s[k], f2s[k] = f1, f2
                    dn = dnl[k]
                    if (dn > 0.0 or (mutate == "exit_in_tie" and dn == 0.0)) and not (_div(-f1, f2) >= dn):
                        e = k
                        break
        else:
            f1, f2 = CT(f1_in), CT(f2_in)
            dtf, Af, Bf, dnf = dt.astype(CT), A.astype(CT), B.astype(CT), dnext.astype(CT)
            with np.errstate(all="ignore"):
                for k in range(count):
                    f1 = f1 + dtf[k] * f2
                    f1 = f1 + Af[k]
                    f2 = f2 - Bf[k]
                    f1s[k], f2s[k] = f1, f2
                    dn = dnf[k]
                    if (dn > 0 or (mutate == "exit_in_tie" and dn == 0)) and not (-f1 / f2 >= dn):
                        e = k
                        break
    else:
        inc, ex, add, tot = _tile_scan(-B)
        off = _offsets(tot, f2_in)
        f2s = off[tile] + (add[tile, wave] + _flat(inc, count))
        f2prev = off[tile] + (add[tile, wave] + _flat(ex, count))
        dfp = dt * f2prev + A
        inc, ex, add, tot = _tile_scan(dfp)
        off = _offsets(tot, f1_in)
        f1s = off[tile] + (add[tile, wave] + _flat(inc, count))
        with np.errstate(all="ignore"):
            ok = (dnext > 0.0) | ((dnext == 0.0) if mutate == "exit_in_tie" else False)
            fail = ok & ~(-f1s / f2s >= dnext)
        hit = np.nonzero(fail)[0]
        e = int(hit[0]) if hit.size else -1
    last = e if e >= 0 else count - 1
    return dict(p=pprev[last] + g[last] * ws[last], c=ck[last].copy(), f1=float(f1s[last]), f2=float(f2s[last]), brk=float(brk[last]),
                exit=e, A=A, B=B, dt=dt)


def _div(a, b):
    """IEEE division of two Python floats (Python raises where IEEE delivers inf or NaN)"""
    return a / b if b != 0.0 else float(np.float64(a) / np.float64(b))


def _gam(k, u):
    return k * u / (1 - k * u)


_UP = 1.0 + 2.0 ** -40


def _up(q):
    """a double not below |q|"""
    return abs(float(q)) * _UP


def scan_bound(brk, g, z, w, M, theta, state, t_prev, brk_next, dtype, exact, upto, chain="host", calls=1):
    """bounds on |device - exact| after crossing `upto` for p, c (arrays of 2c), f', f'' and, per group end k <= upto with a
    successor, on -f'/f'' (dict `q`); `exact` = search_exact's result over at least [0, upto].  See the module docstring."""
    brk, g, z = (np.asarray(a, np.float64) for a in (brk, g, z))
    count = brk.size
    nc2 = len(state) // 2 - 1
    nc = nc2 // 2
    w = np.asarray(w, np.float64).reshape(count, nc2)
    M = np.abs(np.asarray(M, np.float64).reshape(nc2, nc2))
    u = 2.0 ** -53
    uT = 2.0 ** -24 if (np.dtype(dtype) == np.float32 and chain == "host") else u
    DS = calls * (15 + (count + TILE - 1) // TILE) - 3
    extra = 3 * (calls - 1)
    th = abs(float(theta))
    K = upto + 1
    wa = np.abs(w[:K]).copy()
    wa[:, nc:] = wa[:, nc:] * th * (1 + u) * _UP
    ga = np.abs(g[:K])
    dta = np.empty(K)
    dta[0] = brk[0] - t_prev
    dta[1:] = brk[1:K] - brk[:K - 1]
    dta = dta * _UP
    st = np.abs(np.asarray(state, np.float64))
    pex = np.array([[_up(v) for v in row] for row in exact["p"][:K]]).reshape(K, nc2)
    cex = np.array([[_up(v) for v in row] for row in exact["c"][:K]]).reshape(K, nc2)
    pprev = np.vstack([st[:nc2].reshape(1, nc2), pex[:-1]]) if K > 1 else st[:nc2].reshape(1, nc2)
    f1ex = np.array([_up(v) for v in exact["f1"][:K]])
    f2ex = np.array([_up(v) for v in exact["f2"][:K]])
    f2prev = np.concatenate(([st[2 * nc2 + 1]], f2ex[:-1]))
    # p
    Sp = st[:nc2] + np.cumsum(ga[:, None] * wa, axis=0) * _UP
    Ep = _gam(DS + 3, u) * Sp * _UP                                   # K x nc2: p_k returned, and (row k - 1) p_{k-1} stored
    Epprev = np.vstack([np.zeros((1, nc2)) + _gam(DS + 3, u) * st[:nc2], Ep[:-1]]) if K > 1 else np.zeros((1, nc2)) + _gam(DS + 3, u) * st[:nc2]
    # c
    Sc = np.cumsum(dta[:, None] * (pprev + Epprev), axis=0) * _UP
    Ec = (_gam(DS, u) * (st[nc2:2 * nc2] + Sc) + 1.000001 * (2.000001 * u * Sc + np.cumsum(dta[:, None] * Epprev, axis=0))) * _UP
    # (M w), the three dots
    Ua = wa @ M.T * _UP                                                # K x nc2
    Eu = _gam(nc2 + 2, u) * Ua * _UP
    gd = _gam(nc2 + 1, u)

    def dot_err(v, Ev):
        mag = ((Ua + Eu) * (v + Ev)).sum(axis=1)
        return (gd * mag + (Eu * (v + Ev) + Ua * Ev).sum(axis=1)) * _UP, mag * _UP

    Edc, mdc = dot_err(cex, Ec)
    Edp, mdp = dot_err(pprev, Epprev)
    Edw, mdw = dot_err(wa, np.zeros_like(wa))
    gg = ga * ga * _UP
    Babs = (th * gg + 2 * ga * mdp + gg * mdw) * _UP
    EB = (_gam(4, u) * Babs + 2 * ga * Edp + gg * Edw) * _UP
    Aabs = (gg + th * ga * np.abs(z[:K]) + ga * mdc) * _UP
    EA = (_gam(4, u) * Aabs + ga * Edc) * _UP
    ks = np.arange(K)
    if chain == "host":
        g2 = np.array([_gam(k + 3 + extra, uT) for k in ks])
        g1 = np.array([_gam(2 * k + 6 + extra, uT) for k in ks])
    else:
        g2 = np.full(K, _gam(DS + 1, u))
        g1 = np.full(K, _gam(DS + 3, u))
    Ef2 = (g2 * (st[2 * nc2 + 1] + np.cumsum(Babs + EB)) + np.cumsum(EB)) * _UP
    Ef2prev = np.concatenate(([0.0], Ef2[:-1]))
    Ef1 = (g1 * (st[2 * nc2] + np.cumsum(dta * (f2prev + Ef2prev) + Aabs + EA)) + np.cumsum(dta * Ef2prev + EA)) * _UP
    q = {}
    for k in range(K):
        nxt = brk[k + 1] if k + 1 < count else brk_next
        if nxt is None or not nxt > brk[k]:
            continue
        assert Ef2[k] < f2ex[k] / _UP / _UP, "f'' is not resolved at crossing %d" % k
        qa = f1ex[k] / (f2ex[k] / _UP / _UP)
        q[k] = ((Ef1[k] + qa * Ef2[k]) / (f2ex[k] / _UP / _UP - Ef2[k]) * (1 + 2 * uT) + 2 * uT * (qa + (nxt - brk[k]))) * _UP
    return dict(p=Ep[upto], c=Ec[upto], f1=float(Ef1[upto]), f2=float(Ef2[upto]), q=q)


def min_margin_ratio(exact, bound):
    """the smallest |margin| / bound on -f'/f'' over the group ends up to and including the exit"""
    return min(float(abs(exact["margin"][k])) / bound["q"][k] for k in bound["q"] if k in exact["margin"])


# ---------------------------------------------------------------- inputs
def _consts(dtype):
    if np.dtype(dtype) == np.float32:
        return dict(big=1e30, gsmall=1e-10, gbig=1e10, sub=1e-30, zero=2e-38)
    return dict(big=1e250, gsmall=1e-100, gbig=1e65, sub=1e-250, zero=1e-300)


GROUPS = ((2, "eq"), (2, "diff"), (3, "eq"), (3, "diff"), (64, "eq"), (300, "diff"))
SINGLE_LABELS = ("eq g<0", "eq g>0", "eq g=0", "g=+0", "g=-0", "x=lb g>0", "x=ub g<0", "x=lb g<0", "x=ub g>0", "lb=-inf g>0",
                 "lb=-inf g<0", "ub=inf g<0", "ub=inf g>0", "both inf g>0", "both inf g<0", "subnormal", "underflow0", "overflow",
                 "ulp lo", "ulp hi", "out ub 1ulp", "out lb 1ulp", "out ub far", "out lb far")
EDGE_NEED = len(SINGLE_LABELS) + sum(k for k, _ in GROUPS)


def edge_rows(n, dtype, seed, extreme=True):
    """per-row inputs holding every class of the issue (the module docstring of the GPU test lists them): x (inside the box),
    x_out (some rows outside it: only for force), g, lb, ub and `label` (class of the row, "" for the fill).  n >= EDGE_NEED
    holds every class (asserted); a smaller n the singles and the groups that fit.  extreme=False: the three rows whose
    quotient leaves the normal range get ordinary magnitudes instead (a whole search over g = 1e65 next to g = 1 ends at
    its first crossing, where f' = -d.d + g^2 cancels)."""
    T = _T(dtype)
    k = _consts(dtype) if extreme else dict(big=3.0, gsmall=0.7, gbig=1.2, sub=0.01, zero=0.02)
    rng = np.random.default_rng([seed, n, 41])
    inf = np.inf
    t0 = T(0.37)
    rows = [("eq g<0", 0.5, -1.0, 0.5, 0.5), ("eq g>0", 0.5, 1.0, 0.5, 0.5), ("eq g=0", 0.5, 0.0, 0.5, 0.5),
            ("g=+0", 0.2, 0.0, -1.0, 1.0), ("g=-0", 0.2, -0.0, -1.0, 1.0),
            ("x=lb g>0", -1.0, 2.0, -1.0, 1.0), ("x=ub g<0", 1.0, -2.0, -1.0, 1.0),
            ("x=lb g<0", -1.0, -2.0, -1.0, 1.0), ("x=ub g>0", 1.0, 2.0, -1.0, 1.0),
            ("lb=-inf g>0", 0.3, 1.5, -inf, 1.0), ("lb=-inf g<0", 0.3, -1.5, -inf, 1.0),
            ("ub=inf g<0", 0.3, -1.5, -1.0, inf), ("ub=inf g>0", 0.3, 1.5, -1.0, inf),
            ("both inf g>0", 0.3, 1.5, -inf, inf), ("both inf g<0", 0.3, -1.5, -inf, inf),
            ("subnormal", k["sub"], k["gbig"], 0.0, 1.0), ("underflow0", k["zero"], k["gbig"], 0.0, 1.0),
            ("overflow", 0.0, k["gsmall"], -k["big"], 1.0),
            ("ulp lo", t0, 1.0, 0.0, 10.0), ("ulp hi", np.nextafter(t0, T(1)), 1.0, 0.0, 10.0),
            ("out ub 1ulp", 1.0, -2.0, -1.0, 1.0), ("out lb 1ulp", -1.0, -2.0, -1.0, 1.0),
            ("out ub far", 1.0, 2.0, -1.0, 1.0), ("out lb far", -1.0, 2.0, -1.0, 1.0)]
    rows = rows[:n]
    for gi, (size, kind) in enumerate(GROUPS):
        if len(rows) + size > n:
            break
        tb = float(T(0.11 + 0.07 * gi))
        for r in range(size):
            sc = 1.0 if kind == "eq" else (1.0, 2.0, 0.5, 4.0)[r % 4]
            neg = kind == "diff" and r % 3 == 1
            if neg:       # ub = 0, x = -tb sc, g = -sc: brk = (x - 0) / g = tb exactly (sc is a power of two)
                rows.append(("tie%d" % gi, -tb * sc, -sc, -1000.0, 0.0))
            else:
                rows.append(("tie%d" % gi, tb * sc, sc, 0.0, 1000.0))
    ns = len(rows)
    x, g, lb, ub = (np.empty(n, T) for _ in range(4))
    label = np.full(n, "", dtype=object)
    lo = (-1.0 - rng.random(n)).astype(T)
    hi = (1.0 + rng.random(n)).astype(T)
    x[:] = (lo + (hi - lo) * (0.05 + 0.9 * rng.random(n)).astype(T)).astype(T)
    g[:] = rng.standard_normal(n).astype(T)
    g[g == 0] = T(1)
    lb[:], ub[:] = lo, hi
    some = rng.random(n) < 0.1
    lb[some & (g < 0)] = -inf
    ub[some & (g > 0)] = inf
    x[:] = clamp(x, lb, ub)
    where = rng.permutation(n)[:ns]
    for (lab, xv, gv, lv, uv), i in zip(rows, where):
        x[i], g[i], lb[i], ub[i], label[i] = T(xv), T(gv), T(lv), T(uv), lab
    x_out = x.copy()
    for lab, v in (("out ub 1ulp", np.nextafter(T(1), T(2))), ("out lb 1ulp", np.nextafter(T(-1), T(-2))), ("out ub far", T(101)),
                   ("out lb far", T(-101))):
        x_out[label == lab] = v
    if n >= EDGE_NEED:
        assert set(SINGLE_LABELS) | {"tie%d" % i for i in range(len(GROUPS))} <= set(label), "edge_rows: a class is missing"
    assert same_bits(clamp(x_out, lb, ub), x)
    return dict(x=x, x_out=x_out, g=g, lb=lb, ub=ub, label=label)


def edge_classes(r, b):
    """what the build makes of edge_rows' classes: label -> set of (brk class) seen; used to assert that the inputs do what
    their labels say"""
    T = r["x"].dtype.type
    tiny = np.finfo(T).tiny
    out = {}
    for lab in set(r["label"]) - {""}:
        t = b.brk[r["label"] == lab]
        kinds = set()
        for v in t:
            kinds.add("zero" if v == 0 else "inf" if v == np.inf else "sub" if 0 < v < tiny else "pos" if v > 0 else "neg")
        out[lab] = kinds
    return out


EXPECT = {"eq g<0": "zero", "eq g>0": "zero", "eq g=0": "zero", "g=+0": "inf", "g=-0": "inf", "x=lb g>0": "zero", "x=ub g<0": "zero",
          "x=lb g<0": "pos", "x=ub g>0": "pos", "lb=-inf g>0": "inf", "lb=-inf g<0": "pos", "ub=inf g<0": "inf", "ub=inf g>0": "pos",
          "both inf g>0": "inf", "both inf g<0": "inf", "subnormal": "sub", "underflow0": "zero", "overflow": "inf", "ulp lo": "pos",
          "ulp hi": "pos"}


# ---------------------------------------------------------------- scan cases
class ScanCase:
    """rows whose sorted list is a designed sequence of crossings, a history, M, theta and the state the search starts from.
    Break points t_k rise by gaps of about `gap`; after the crossing `exit_at` (when >= 0) the next gap is `jump`, and
    state = [p, c, f' = -F, f'' = F2] has -f'/f'' of order 1 throughout: the search goes on across every small gap and stops
    at the jump.  tie = (start, size): that many consecutive crossings share one break point."""

    def __init__(self, name, dtype, c, count, exit_at, seed, tie=None, extra=0, gap=5e-4, jump=1e3, flip=False):
        T = self.T = _T(dtype)
        self.name, self.dtype, self.c, self.count, self.exit_at = name, np.dtype(dtype), c, count, exit_at
        n = self.n = count + extra + 3
        rng = np.random.default_rng([seed, count, c, 43])
        gaps = gap * (0.5 + rng.random(n))
        if tie:
            gaps[tie[0] + 1:tie[0] + tie[1]] = 0.0
        if exit_at is not None and exit_at >= 0:
            gaps[exit_at + 1] = jump
        t = np.cumsum(gaps)
        t = t.astype(T).astype(np.float64)
        sc = np.array([1.0, 2.0, 0.5, 4.0])[rng.integers(0, 4, n)]      # powers of two: x / g is t exactly
        neg = rng.random(n) < 0.5
        if flip:
            sc[:2], neg[:2] = 1.0, False
        g = np.where(neg, -sc, sc)
        self.g = g.astype(T)
        self.x = (t * g).astype(T)
        assert np.array_equal(self.x.astype(np.float64), t * g), "t g must be exact"
        self.lb = np.where(neg, -1e6, 0.0).astype(T)
        self.ub = np.where(neg, 0.0, 1e6).astype(T)
        # three rows that never enter the list: on a bound, free, and fixed
        self.x[-3:], self.g[-3:], self.lb[-3:], self.ub[-3:] = T(0), (T(1), T(0), T(-1)), (T(0), T(-1), T(0)), (T(1), T(1), T(0))
        perm = rng.permutation(n)                       # scattered rows; ties land in arbitrary row order
        inv = np.argsort(perm)
        for k in ("x", "g", "lb", "ub"):
            setattr(self, k, getattr(self, k)[inv])
        self.pairs = [(0.3 * rng.standard_normal(n).astype(T), 0.3 * rng.standard_normal(n).astype(T)) for _ in range(c)]
        self.cols = [p[1] for p in self.pairs] + [p[0] for p in self.pairs]
        nc2 = 2 * c
        Q = 0.05 * rng.standard_normal((nc2, nc2))
        self.M = (Q + Q.T) / 2 + 0.2 * np.diag(np.where(np.arange(nc2) < c, -1.0, 1.0))
        self.theta = 1.3
        F = 40.0 * count + 1000.0
        self.state = np.concatenate((0.5 * rng.standard_normal(nc2), 0.01 * rng.standard_normal(nc2), [-F, F]))
        self.t_prev = 0.0
        if flip:
            # the first two crossings share a break point; the first lifts f' above zero, the second takes it back below: a
            # search that tested -f'/f'' inside the group would stop at crossing 0
            assert c == 1 and tie == (0, 2)
            r0, r1 = sorted(perm[:2].tolist())
            self.pairs[0][1][[r0, r1]] = T(10), T(-10)
            self.pairs[0][0][[r0, r1]] = T(0)
            self.state = np.array([0.5, -0.25, 10.0, 0.0, -10.0, 100.0])

    def lists(self):
        """the reference's sorted list of the rows: (build, order, gather)"""
        b = build(self.x, self.g, self.lb, self.ub)
        o = order(b.brk)
        return b, o, gather(o, b.brk, b.x, self.g, b.d, self.lb, self.ub, self.cols)

    def Mmat(self):
        """column-major, as lbfgsx_b_cauchy_scan takes it"""
        return np.ascontiguousarray(self.M.T).reshape(-1)


HIST_CS = (1, 2, 4, 5, 7, 8, 10, 12, 16, 20, 24, 32, 40)


def hist_count(c):
    """crossings of a case with c pairs: about 600 (three tiles), fewer where the exact reference would take too long"""
    return 600 if c <= 5 else 530 if c <= 10 else 300 if c <= 16 else 270 if c <= 24 else 260


def scan_cases():
    """the committed cases with stored pairs: every NC class and every placement of the exit, in f64 and in f32"""
    out = []
    for c in HIST_CS:
        n = hist_count(c)
        out.append(ScanCase("c%d" % c, np.float64, c, n, n - 40, 50 + c, extra=20))
    for c in HIST_CS:
        n = hist_count(c)
        out.append(ScanCase("c%d-f32" % c, np.float32, c, n, n - 40, 80 + c, extra=20))
    for dt, sfx in ((np.float64, ""), (np.float32, "-f32")):
        out.append(ScanCase("exit0" + sfx, dt, 2, 300, 0, 101, extra=5))
        out.append(ScanCase("exit255" + sfx, dt, 2, 600, 255, 102, extra=5))
        out.append(ScanCase("exit256" + sfx, dt, 2, 600, 256, 103, extra=5))
        out.append(ScanCase("tie300" + sfx, dt, 1, 600, 399, 104, tie=(100, 300), extra=5))
        out.append(ScanCase("noexit" + sfx, dt, 2, 300, -1, 105, extra=5))
        out.append(ScanCase("listend" + sfx, dt, 2, 300, -1, 106, extra=0))
        out.append(ScanCase("tieflip" + sfx, dt, 1, 40, None, 107, tie=(0, 2), extra=5, flip=True))
    return out


FACTOR = 4       # the exact margin at every group end up to the exit exceeds FACTOR x the bound on -f'/f''


# ---------------------------------------------------------------- a whole search without stored pairs
def whole_search(x, g, lb, ub, dev_min, dd=None):
    """get_cauchy_point (include/LBFGSpp/Cauchy.h, the reference's :140-282) for an empty history, as the library runs it:
    the reference's scalar loop in the problem's type T for the groups that start below sorted position dev_min (all of them
    when dev_min < 0), scan_emulate (default chain) from there on.  d.d enters as the correctly rounded sum the build
    delivers.  Every step is a fixed sequence of IEEE operations, so xcp, the state bytes and the counts are exact
    expectations.  Returns finish()'s dict plus `crossings`."""
    from bounded_sums_ref import stored
    T = x.dtype.type
    b = build(x, g, lb, ub)
    o = order(b.brk)
    ga = gather(o, b.brk, b.x, g, b.d, lb, ub)
    nord, nfree = o.size, b.nfree
    if nfree < 1 and nord < 1:
        out = finish(b.brk, b.x, b.d, lb, ub, 0.0, 0.0, 0)
        out["crossings"] = 0
        return out
    brk, gs, zs = ga["brk"].astype(T), ga["g"].astype(T), ga["z"].astype(T)
    theta, zero = T(1), T(0)
    with np.errstate(all="ignore"):
        fp = -T(stored(b.dd_exact, T) if dd is None else dd)
        fpp = -theta * fp
        dtm = -fp / fpp
        il, bpos, crossings, t_cross, crossed_all = T(0), 0, 0, T(0), False
        iu = T(np.inf) if nord < 1 else brk[0]
        deltat = iu - il
        while dtm >= deltat:
            if dev_min >= 0 and bpos >= dev_min:
                em = scan_emulate(ga["brk"][bpos:], ga["g"][bpos:], ga["z"][bpos:], ga["w"][bpos:], np.zeros((0, 0)), 1.0,
                                  [float(fp), float(fpp)], float(il), None, T)
                done = em["exit"] + 1 if em["exit"] >= 0 else nord - bpos
                crossings += done
                bpos += done
                il = t_cross = T(em["brk"])
                fp, fpp = T(em["f1"]), T(em["f2"])
                dtm = -fp / fpp
                if nfree == 0 and bpos >= nord:
                    crossed_all = True
                break
            e = bpos
            while e < nord and not (brk[e] > iu):
                e += 1
            e -= 1
            if nfree == 0 and e == nord - 1:
                crossed_all, t_cross = True, iu
                crossings += e - bpos + 1
                break
            fp = fp + deltat * fpp
            for i in range(bpos, e + 1):
                gg = gs[i] * gs[i]
                fp = fp + (gg + theta * gs[i] * zs[i] - gs[i] * zero)
                fpp = fpp - (theta * gg + T(2) * gs[i] * zero + gg * zero)
            crossings += e - bpos + 1
            dtm = -fp / fpp
            il = t_cross = iu
            bpos = e + 1
            if bpos >= nord:
                break
            iu = brk[bpos]
            deltat = iu - il
        eps = np.finfo(T).eps
        if fpp < eps:
            dtm = -fp / eps
        tfinal = T(0)
        if not crossed_all:
            dtm = max(dtm, T(0))
            tfinal = il + dtm
    out = finish(b.brk, b.x, b.d, lb, ub, float(t_cross), float(tfinal), crossed_all)
    out["crossings"] = crossings
    return out
