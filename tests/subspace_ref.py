"""numpy restatements of the device side of the L-BFGS-B subspace minimisation (BOXCQP; csrc/lbfgsb_subspace.hip and its
kernels in csrc/lbfgsb_kernels.cuh / lbfgsb_x.cuh), in the context's scalar type, ONE numpy operation per source operation.
The library is built with -ffp-contract=off, so the claim is bit equality for every vector and state byte and exact
equality for every count; the n-length sums (wty, out_l, out_u, negc_dd) are held to bounded_sums_ref (exact sums,
check_rounded / check_pair with dd_bound).  No GPU, no oracle library; tests/test_subspace_ref_cpu.py proves what is here
(a scalar transcription of the reference's SubspaceMin.h, a whole minimisation against the oracle, the coverage of the case
generators), tests/test_subspace_statements_gpu.py uses it.

  Vecs                      the vectors the statements read and write, by row, and the state bytes
  sweep                     sweep_row / sweep_row_v with `first` (k_sub_sweep_begin, the tail of k_solve_sweep, k_lu_sweep)
  partition, check          k_sub_partition, k_sub_check
  sub_op                    the six LBFGSX_SO_* statements
  wacc                      (W coef)(row) in the two accumulation orders of k_wcombine
  wcombine                  the five LBFGSX_CB_* combines
  solve                     y = v / theta + a / theta^2 (v / theta without coefficients), any selector
  gp_rhs                    the LBFGSX_GP_RHS prologue  rhs = (rhs + -(W c1)) + -(W c2)
  solve_sweep, lu_sweep     the fused passes, composed of the statements above in the kernels' order
  minimize                  a whole minimisation composed of these statements (dense numpy solves of the 2c x 2c systems)
  case generators           build_rows (bounds, x0, g per row), edge_values (y, lambda, mu at every tie and one ulp around it)

Coefficients and theta enter as doubles and are converted with T(.) as CoefArg / CoefX do.  Finite inputs only: what the
kernels do with NaN is not restated here."""
import numpy as np

ST_FREE, ST_NEWACT, ST_L, ST_U, ST_P = 1, 2, 4, 8, 16
ST_PART = ST_L | ST_U | ST_P
SV_CF, SV_Y, SV_YFB, SV_LAM, SV_MU, SV_RHS = range(6)
SV_NAMES = ("cF", "y", "yfb", "lam", "mu", "rhs")
VS_DRT, VS_NEG_CF, VS_NEG_RHS, VS_LBOUND, VS_UBOUND, VS_Y = range(6)
CB_LINEAR, CB_SOLVE, CB_RHS_ADD, CB_LAMBDA, CB_MU = range(5)
SO_SAVE_FALLBACK, SO_RHS_INIT, SO_ASSIGN_Y, SO_CLAMP_Y, SO_CLAMP_FB, SO_ASSIGN_FB = range(6)
GP_NONE, GP_RHS, GP_LINEAR = 0, 1, 2


class Vecs:
    """x0, g, lb, ub, drt and the six sub-vectors by row (arrays of the scalar type), st (uint8)"""
    FIELDS = ("x0", "g", "lb", "ub", "drt") + SV_NAMES + ("st",)

    def __init__(self, dt, **kw):
        self.dt = np.dtype(dt).type
        for k in self.FIELDS:
            a = kw[k]
            setattr(self, k, np.array(a, np.uint8 if k == "st" else self.dt))

    def copy(self):
        return Vecs(self.dt, **{k: getattr(self, k) for k in self.FIELDS})

    @property
    def n(self):
        return self.st.size

    @property
    def li(self):
        return self.lb - self.x0   # const T li = b.lb[i] - b.x0[i]

    @property
    def ui(self):
        return self.ub - self.x0

    def rows(self, mask):
        return (self.st & mask) != 0


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def diff_rows(a, b):
    """rows whose bit patterns differ"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    w = a.dtype.itemsize
    return np.nonzero((a.view(np.uint8).reshape(-1, w) != b.view(np.uint8).reshape(-1, w)).any(axis=1))[0]


# ---------------------------------------------------------------- the statements of one sweep
def sweep(V, first, rows=None, lam=None, mu=None, store_mult=True):
    """sweep_row on the free rows among `rows` (None: all): first ? (#outside, yfb = y) : the three convergence counts; then
    the partition with the multipliers lam / mu (None: the stored ones; `first` callers pass zeros), y moved onto the bound,
    rhs = cF on the new P, the multipliers stored when store_mult, the state byte.
    Returns the 7 counts {#L, #U, #P, #F outside (first), #P outside, #L lam < 0, #U mu < 0}."""
    dt = V.dt
    act = V.rows(ST_FREE) if rows is None else (V.rows(ST_FREE) & rows)
    li, ui, y, s = V.li, V.ui, V.y.copy(), V.st.copy()
    lam = V.lam.copy() if lam is None else np.array(lam, dt)
    mu = V.mu.copy() if mu is None else np.array(mu, dt)
    cnt = [0] * 7
    outside = (y < li) | (y > ui)
    if first:
        cnt[3] = int((act & outside).sum())
        V.yfb[act] = y[act]
    else:
        cnt[4] = int((act & ((s & ST_P) != 0) & outside).sum())
        cnt[5] = int((act & ((s & ST_L) != 0) & (lam < dt(0))).sum())
        cnt[6] = int((act & ((s & ST_U) != 0) & (mu < dt(0))).sum())
    toL = act & ((y < li) | ((y == li) & (lam >= dt(0))))
    toU = act & ~toL & ((y > ui) | ((y == ui) & (mu >= dt(0))))
    toP = act & ~toL & ~toU
    V.y[toL] = li[toL]
    mu[toL] = dt(0)
    V.y[toU] = ui[toU]
    lam[toU] = dt(0)
    lam[toP] = dt(0)
    mu[toP] = dt(0)
    V.rhs[toP] = V.cF[toP]
    if store_mult:
        V.lam[act] = lam[act]
        V.mu[act] = mu[act]
    s[act] &= np.uint8(0xFF ^ ST_PART)
    s[toL] |= np.uint8(ST_L)
    s[toU] |= np.uint8(ST_U)
    s[toP] |= np.uint8(ST_P)
    V.st = s
    cnt[0], cnt[1], cnt[2] = int(toL.sum()), int(toU.sum()), int(toP.sum())
    return cnt


def partition(V):
    """k_sub_partition: the partition alone (no rhs, no yfb, the stored multipliers); returns (#L, #U, #P)"""
    dt = V.dt
    act = V.rows(ST_FREE)
    li, ui, y = V.li, V.ui, V.y.copy()
    toL = act & ((y < li) | ((y == li) & (V.lam >= dt(0))))
    toU = act & ~toL & ((y > ui) | ((y == ui) & (V.mu >= dt(0))))
    toP = act & ~toL & ~toU
    V.y[toL] = li[toL]
    V.mu[toL] = dt(0)
    V.y[toU] = ui[toU]
    V.lam[toU] = dt(0)
    V.lam[toP] = dt(0)
    V.mu[toP] = dt(0)
    s = V.st.copy()
    s[act] &= np.uint8(0xFF ^ ST_PART)
    s[toL] |= np.uint8(ST_L)
    s[toU] |= np.uint8(ST_U)
    s[toP] |= np.uint8(ST_P)
    V.st = s
    return int(toL.sum()), int(toU.sum()), int(toP.sum())


def check(V):
    """k_sub_check: {#F outside, #P outside, #L lam < 0, #U mu < 0}; changes nothing"""
    dt = V.dt
    act = V.rows(ST_FREE)
    outside = (V.y < V.li) | (V.y > V.ui)
    return [int((act & outside).sum()), int((act & V.rows(ST_P) & outside).sum()),
            int((act & V.rows(ST_L) & (V.lam < dt(0))).sum()), int((act & V.rows(ST_U) & (V.mu < dt(0))).sum())]


def sub_op(V, op):
    """k_sub_op on the free rows"""
    dt = V.dt
    act = V.rows(ST_FREE)
    if op == SO_SAVE_FALLBACK:
        V.yfb[act] = V.y[act]
        V.lam[act] = dt(0)
        V.mu[act] = dt(0)
    elif op == SO_RHS_INIT:
        p = act & V.rows(ST_P)
        V.rhs[p] = V.cF[p]
    elif op == SO_ASSIGN_Y:
        V.drt[act] = V.y[act]
    elif op in (SO_CLAMP_Y, SO_CLAMP_FB):
        li, ui = V.li, V.ui
        v = (V.y if op == SO_CLAMP_Y else V.yfb).copy()
        v = np.where(v < li, li, v)       # v = (v < li) ? li : v
        v = np.where(ui < v, ui, v)       # v = (ui < v) ? ui : v
        V.y[act] = v[act]
    else:
        V.drt[act] = V.yfb[act]


# ---------------------------------------------------------------- combines
def coef_t(coef, dt, total):
    """T(coef[k]) for k < 2c (CoefArg / CoefX)"""
    dt = np.dtype(dt).type
    return [dt(np.float64(coef[k])) for k in range(total)]


def wacc(cols, coef, dt, paired=False):
    """(W coef)(row) for every row, acc = T(0) first.  cols: logical order [Y slots, S slots].
    plain  : acc = acc + col_k * c_k, k = 0 .. 2c - 1        (CB_LINEAR, CB_SOLVE, CB_RHS_ADD, the solves, GP_RHS)
    paired : acc = acc + (c_j * Y_j + c_{c+j} * S_j), j < c   (CB_LAMBDA, CB_MU, k_lu_sweep)"""
    dt = np.dtype(dt).type
    total = len(cols)
    c = total // 2
    if not total:
        return dt(0)      # no history: the sum stays T(0) on every row
    acc = np.zeros(cols[0].size, dt)
    if coef is None:
        return acc
    cf = coef_t(coef, dt, total)
    if paired:
        for j in range(c):
            acc = acc + (cf[j] * cols[j] + cf[c + j] * cols[c + j])
    else:
        for k in range(total):
            acc = acc + cols[k] * cf[k]
    return acc


def vsel(V, sel):
    if sel == VS_DRT:
        return V.drt.copy()
    if sel == VS_NEG_CF:
        return -V.cF
    if sel == VS_NEG_RHS:
        return -V.rhs
    if sel == VS_LBOUND:
        return V.lb - V.x0
    if sel == VS_UBOUND:
        return V.ub - V.x0
    return V.y.copy()


def solve_values(V, cols, sel, coef, theta):
    """y = v / theta + a / theta^2 (coef None or no columns: v / theta) on every row"""
    dt = V.dt
    th = dt(np.float64(theta))
    th2 = th * th
    v = vsel(V, sel)
    with np.errstate(invalid="ignore", over="ignore"):   # rows outside the mask may hold infinite bounds
        if coef is None or not len(cols):
            return v / th
        return v / th + wacc(cols, coef, dt) / th2


def solve(V, cols, rows, sel, coef, theta):
    y = solve_values(V, cols, sel, coef, theta)
    V.y[rows] = y[rows]


def wcombine(V, cols, mode, mask, sel, coef, theta):
    """k_wcombine<mode> on the rows whose state has a bit of `mask`"""
    dt = V.dt
    rows = V.rows(mask)
    has_w = coef is not None and len(cols) > 0
    th = dt(np.float64(theta))
    if mode == CB_LINEAR:
        new = (dt(-1) * wacc(cols, coef, dt) if has_w else np.zeros(V.n, dt)) + V.g
        V.cF[rows] = new[rows]
    elif mode == CB_SOLVE:
        solve(V, cols, rows, sel, coef if has_w else None, theta)
    elif mode == CB_RHS_ADD:
        new = V.rhs + (-wacc(cols, coef if has_w else None, dt))
        V.rhs[rows] = new[rows]
    else:
        r = (dt(-1) * wacc(cols, coef if has_w else None, dt, paired=True)) + (V.cF + th * V.y)
        if mode == CB_LAMBDA:
            V.lam[rows] = r[rows]
        else:
            V.mu[rows] = (-r)[rows]


def gp_rhs(V, cols, rows, c1, c2):
    """LBFGSX_GP_RHS: rhs = (rhs + -(W c1)) + -(W c2) on `rows`, a NULL coefficient vector skips its term"""
    rh = V.rhs.copy()
    if c1 is not None:
        rh = rh + (-wacc(cols, c1, V.dt))
    if c2 is not None:
        rh = rh + (-wacc(cols, c2, V.dt))
    V.rhs[rows] = rh[rows]


# ---------------------------------------------------------------- the fused passes
def solve_sweep(V, cols, first, sel, coef, theta, c1=None, c2=None):
    """lbfgsx_b_solve_sweep[_rhs]: first: the solve on every free row, then the first sweep's statements; else the rhs updates
    and the solve on the rows of P, then the next sweep's statements on those rows with zero multipliers that are not
    stored.  Returns (sums[7], y as the dots W_F'y see it -- the un-clamped y of the solved rows, None when first)."""
    free = V.rows(ST_FREE)
    rows = free if first else (free & V.rows(ST_P))
    if c1 is not None or c2 is not None:
        gp_rhs(V, cols, rows, c1, c2)
    solve(V, cols, rows, sel, coef, theta)
    ydots = None if first else V.y.copy()
    zeros = np.zeros(V.n, V.dt)
    cnt = sweep(V, bool(first), rows, zeros, zeros, store_mult=bool(first))
    if not first:
        cnt[3] = 0
    return cnt, ydots


def lu_sweep(V, cols, coef, theta, listed):
    """k_lu_sweep over the rows of the index list (`listed`: the L u U of the partition BEFORE the solve that precedes it -- the
    rows that solve moved from P into L or U are not among them): lambda on the rows of L, mu on the rows of U (paired
    order), then the sweep's statements on those rows"""
    dt = V.dt
    rows = listed & V.rows(ST_L | ST_U)
    th = dt(np.float64(theta))
    has_w = coef is not None and len(cols) > 0
    r = (dt(-1) * wacc(cols, coef if has_w else None, dt, paired=True)) + (V.cF + th * V.y)
    lam, mu = V.lam.copy(), V.mu.copy()
    isl, isu = rows & V.rows(ST_L), rows & V.rows(ST_U)
    lam[isl] = r[isl]
    mu[isu] = (-r)[isu]
    return sweep(V, False, rows, lam, mu, store_mult=True)


# ---------------------------------------------------------------- scalar transcription of the reference (SubspaceMin.h)
def scalar_partition(vecy, vecl, vecu, lam, mu):
    """SubspaceMin.h:194-219 on the free rows (arrays over the free set, changed in place); returns the L, U, P index lists"""
    T = vecy.dtype.type
    L, U, P = [], [], []
    for i in range(vecy.size):
        li, ui = vecl[i], vecu[i]
        if (vecy[i] < li) or (vecy[i] == li and lam[i] >= T(0)):
            L.append(i)
            vecy[i] = li
            mu[i] = T(0)
        elif (vecy[i] > ui) or (vecy[i] == ui and mu[i] >= T(0)):
            U.append(i)
            vecy[i] = ui
            lam[i] = T(0)
        else:
            P.append(i)
            lam[i] = T(0)
            mu[i] = T(0)
    return L, U, P


def scalar_converged(L, U, P, vecy, vecl, vecu, lam, mu):
    """:60-108, :162, :271 as counts: (#outside over all, #P outside, #L lam < 0, #U mu < 0)"""
    T = vecy.dtype.type
    out_all = sum(1 for i in range(vecy.size) if vecy[i] < vecl[i] or vecy[i] > vecu[i])
    out_p = sum(1 for i in P if vecy[i] < vecl[i] or vecy[i] > vecu[i])
    return out_all, out_p, sum(1 for i in L if lam[i] < T(0)), sum(1 for i in U if mu[i] < T(0))


def scalar_multiplier(Wrow_y, Wrow_s, cy, cs, cval, theta, yval):
    """:256-258 with apply_PtWMv's paired order (BFGSMat.h:447-457): res = -1 * sum_j (cy_j y_j + cs_j s_j); res += c + theta y"""
    T = type(yval)
    acc = T(0)
    for j in range(len(cy)):
        acc = acc + (cy[j] * Wrow_y[j] + cs[j] * Wrow_s[j])
    return (T(-1) * acc) + (cval + theta * yval)


def scalar_clamp(v, lo, hi):
    """:278, :287 cwiseMax(l).cwiseMin(u): max(v, l) = (v < l) ? l : v, min(., u) = (u < .) ? u : ."""
    out = v.copy()
    for i in range(v.size):
        x = out[i]
        x = lo[i] if x < lo[i] else x
        x = hi[i] if hi[i] < x else x
        out[i] = x
    return out


# ---------------------------------------------------------------- a whole minimisation from the statements
def bfgs_mats(S, Y, m):
    """the compact representation from the pairs (rows of S, Y in the order they were added): the last c = min(npairs, m)
    pairs oldest first, theta = y'y / s'y of the newest, Minv = [[-D, L'], [L, theta S'S]] (BFGSMat.h:101-146), in double"""
    npairs = S.shape[0]
    c = min(npairs, m)
    if c == 0:
        return [], 1.0, np.zeros((0, 0))
    Sc = [np.asarray(S[k], np.float64) for k in range(npairs - c, npairs)]
    Yc = [np.asarray(Y[k], np.float64) for k in range(npairs - c, npairs)]
    theta = float(np.dot(Yc[-1], Yc[-1]) / np.dot(Sc[-1], Yc[-1]))
    Minv = np.zeros((2 * c, 2 * c))
    for i in range(c):
        Minv[i, i] = -np.dot(Sc[i], Yc[i])
        for j in range(c):
            Minv[c + i, c + j] = theta * np.dot(Sc[i], Sc[j])
            if i > j:
                Minv[c + i, j] = Minv[j, c + i] = np.dot(Sc[i], Yc[j])
    return Yc + Sc, theta, Minv


def _wt(cols, v, rows, theta):
    """W_rows' v with W = [Y, theta S]"""
    c = len(cols) // 2
    out = np.array([np.dot(col[rows], v[rows]) for col in cols])
    out[c:] *= theta
    return out


def _to_cols(z, theta):
    """W z = Y z_Y + theta S z_S as coefficients of the columns [Y S]"""
    z = np.array(z, np.float64)
    z[len(z) // 2:] *= theta
    return z


def minimize(dt, S, Y, m, x0, xcp, g, lb, ub, free, newact, maxit):
    """subspace_minimize (SubspaceMin.h:122-302) composed of the statements above; the 2c x 2c systems are solved densely in
    double (numpy) where the product takes its Gram route.  Returns (drt, sweeps run)."""
    dt = np.dtype(dt).type
    n = x0.size
    cols64, theta, Minv = bfgs_mats(S, Y, m)
    cols = [c.astype(dt) for c in cols64]
    total = len(cols)
    st = np.where(free, ST_FREE, np.where(newact, ST_NEWACT, 0)).astype(np.uint8)
    z = np.zeros(n, dt)
    V = Vecs(dt, x0=x0, g=g, lb=lb, ub=ub, drt=np.asarray(xcp, dt) - np.asarray(x0, dt), cF=z, y=z, yfb=z, lam=z, mu=z, rhs=z, st=st)
    if not free.any():
        return V.drt, 0
    M = np.linalg.inv(Minv) if total else None

    def solve_ptbp(rows, sel):
        # BFGSMat.h:525-565: y = v / theta + W_P (Minv - W_P'W_P / theta)^-1 W_P'v / theta^2
        if not total:
            solve(V, cols, rows, sel, None, theta)
            return
        v = vsel(V, sel).astype(np.float64)
        WP = np.array([col[rows] for col in cols64]).T
        WP[:, total // 2:] *= theta
        zc = np.linalg.solve(Minv - WP.T @ WP / theta, WP.T @ v[rows])
        solve(V, cols, rows, sel, _to_cols(zc, theta), theta)

    # :143-156 vecc = -W_F M W_A'(A'd) + g_F
    cf = None
    if total and newact.any():
        cf = _to_cols(M @ _wt(cols64, V.drt.astype(np.float64), newact, theta), theta)
    wcombine(V, cols, CB_LINEAR, ST_FREE, VS_DRT, cf, theta)
    solve_ptbp(free, VS_NEG_CF)                                       # :159
    if check(V)[0] == 0:                                              # :162
        sub_op(V, SO_ASSIGN_Y)
        return V.drt, 0
    k = 0
    first = True
    while k < maxit:
        sweep(V, first, None, z if first else None, z if first else None)   # :170-172 / :194-219, :232
        first = False
        isL, isU, isP = V.rows(ST_L), V.rows(ST_U), V.rows(ST_P)
        if isP.any():
            for rows_q, sel_q in ((isL, VS_LBOUND), (isU, VS_UBOUND)):      # :236-241
                if total and rows_q.any():
                    q = vsel(V, sel_q).astype(np.float64)
                    if np.any(q[rows_q] != 0):
                        wcombine(V, cols, CB_RHS_ADD, ST_P, VS_DRT, _to_cols(M @ _wt(cols64, q, rows_q, theta), theta), theta)
            solve_ptbp(isP, VS_NEG_RHS)                                     # :243
        if isL.any() or isU.any():
            cfm = _to_cols(M @ _wt(cols64, V.y.astype(np.float64), free, theta), theta) if total else None
            if isL.any():
                wcombine(V, cols, CB_LAMBDA, ST_L, VS_DRT, cfm, theta)
            if isU.any():
                wcombine(V, cols, CB_MU, ST_U, VS_DRT, cfm, theta)
        ck = check(V)
        if ck[1] == 0 and ck[2] == 0 and ck[3] == 0:                        # :271
            break
        k += 1
    if k >= maxit:                                                          # :276-296
        eps = float(np.finfo(dt).eps)
        sub_op(V, SO_CLAMP_Y)
        sub_op(V, SO_ASSIGN_Y)
        if float(np.dot(V.drt.astype(np.float64), V.g.astype(np.float64))) <= -eps:
            return V.drt, k
        sub_op(V, SO_CLAMP_FB)
        sub_op(V, SO_ASSIGN_Y)
        if float(np.dot(V.drt.astype(np.float64), V.g.astype(np.float64))) <= -eps:
            return V.drt, k
        sub_op(V, SO_ASSIGN_FB)
        return V.drt, k
    sub_op(V, SO_ASSIGN_Y)
    return V.drt, k + 1


# ---------------------------------------------------------------- case generators
K_FREE, K_FREE0, K_NEWACT, K_FIXED, K_INFL, K_INFU, K_INFB, K_EQ = range(8)
_FREE_KINDS = (K_FREE, K_FREE0, K_INFL, K_INFU, K_INFB, K_EQ)


def build_rows(n, dtype, seed, nfree=None, free_all=False, finite_only=False):
    """Bounds, x0 and g per row such that lbfgsx_b_cauchy_build / _finish(1, 1, 0) / lbfgsx_b_sub_begin put each row in the free
    set or among the newly active rows at will.  x0 is random, lb = x0 - wl, ub = x0 + wu with widths in [0.5, 2).  Kinds:
      K_FREE   |g| = a quarter of the smaller width: break point >= 4, free          K_FREE0  g = 0: free
      K_NEWACT |g| = twice the larger width: break point <= 1 / 2, newly active       K_FIXED  lb = ub = x0, g != 0: in neither set
      K_INFL / K_INFU / K_INFB  lb = -inf / ub = +inf / both: free (|g| as K_FREE)    K_EQ     l == u on a free row, see below
    K_EQ: a row with lb == ub is never free (its break point is 0, Cauchy.h:113), so l == u cannot come from equal bounds.  It
    comes from ADJACENT bounds, lb = x0, ub = the next number above it, g = 0 (free), and an x0 that the caller moves 1024 away
    after the Cauchy search (`x0_sweep`; upload it after lbfgsx_b_sub_begin): lb - x0 and ub - x0 then round to the same number.
    nfree: exactly that many free rows (the compact-copy thresholds); free_all: no other kind than the free ones;
    finite_only: K_FREE in place of the kinds with an infinite bound (every free row can be moved into L u U).
    Returns a dict of arrays in `dtype` and `kind`, `free`, `newact` (what the state bytes must come out as)."""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng([seed, n, 4711])
    u = rng.random(n)
    kind = np.full(n, K_NEWACT, np.int8)
    edges = (0.40, 0.46, 0.52, 0.58, 0.62, 0.70)       # FREE, FREE0, INFL, INFU, INFB, EQ | then NEWACT 0.70..0.95, FIXED
    kind[u < edges[5]] = K_EQ
    kind[u < edges[4]] = K_INFB
    kind[u < edges[3]] = K_INFU
    kind[u < edges[2]] = K_INFL
    kind[u < edges[1]] = K_FREE0
    kind[u < edges[0]] = K_FREE
    kind[u >= 0.95] = K_FIXED
    if free_all:
        kind[u >= edges[5]] = K_FREE
    if finite_only:
        kind[np.isin(kind, (K_INFL, K_INFU, K_INFB))] = K_FREE
    if nfree is not None:
        # keep the mix among the first nfree rows of a permutation, every other row newly active
        perm = rng.permutation(n)
        isfree = np.isin(kind, _FREE_KINDS)
        kind[perm[:nfree][~isfree[perm[:nfree]]]] = K_FREE
        kind[perm[nfree:]] = K_NEWACT
    # the first and the last row are free (kinds swapped, the counts stay): a dropped head or tail row of a pass shows
    for end in (0, n - 1):
        donors = np.nonzero(kind == K_FREE)[0]
        donors = donors[(donors != 0) & (donors != n - 1)]
        if kind[end] != K_FREE and donors.size:
            d = donors[donors.size // 2]
            kind[end], kind[d] = kind[d], kind[end]
    x0 = rng.standard_normal(n).astype(dt)
    wl, wu = 0.5 + 1.5 * rng.random(n), 0.5 + 1.5 * rng.random(n)
    lb, ub = (x0 - wl).astype(dt), (x0 + wu).astype(dt)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    g = sign * 0.25 * np.minimum(wl, wu)
    g = np.where(kind == K_NEWACT, sign * 2.0 * np.maximum(wl, wu), g)
    g[(kind == K_FREE0) | (kind == K_EQ)] = 0.0
    eq = (kind == K_FIXED) | (kind == K_EQ)
    lb[eq] = x0[eq]
    ub[eq] = x0[eq]
    keq = kind == K_EQ
    ub[keq] = np.nextafter(x0[keq], dt(np.inf))
    lb[(kind == K_INFL) | (kind == K_INFB)] = -np.inf
    ub[(kind == K_INFU) | (kind == K_INFB)] = np.inf
    free = np.isin(kind, _FREE_KINDS)
    x0_sweep = x0.copy()
    x0_sweep[keq] = x0[keq] - dt(1024)
    return dict(x0=x0, x0_sweep=x0_sweep, lb=lb, ub=ub, g=g.astype(dt), kind=kind, free=free, newact=kind == K_NEWACT)


def sentinel(which, n, dtype, gen=0):
    """distinct finite values no statement produces: 7 + gen + which / 16 + row / 2 (exact in float32 below 2^19 rows, distinct
    below 2^23)"""
    dt = np.dtype(dtype).type
    return (dt(7 + gen) + dt(which) * dt(0.0625) + np.arange(n, dtype=dt) * dt(0.5)).astype(dt)


NCLASS = 20
EDGE_LABELS = ("y==l lam>0", "y==l lam=+0", "y==l lam=-0", "y==l lam<0", "y==u mu>0", "y==u mu=+0", "y==u mu=-0", "y==u mu<0",
               "l==u==y", "y=l+ulp", "y=l-ulp", "y=u-ulp", "y=u+ulp", "l=-inf", "u=+inf", "y<l", "y>u", "interior")


def edge_values(li, ui, free, dtype, shift=0, seed=0):
    """(y, lam, mu) for every row: on the free rows the class (rank among the free rows + shift) % NCLASS decides --
      0..3   y = l with lam > 0, = +0, = -0, < 0         4..7   y = u with mu > 0, = +0, = -0, < 0
      8, 9   y one ulp inside / outside l                10, 11 y one ulp inside / outside u
      12, 13 y far below l / far above u                 14, 15 interior with both multipliers < 0 / > 0
      16, 17 y = l with lam < 0 and mu < 0 / mu > 0 (on a row with l = u: P / U)
      18, 19 interior
    -- where the bound a class needs is infinite the row gets an interior y.  The other rows hold what the caller fills in.
    A different shift moves every free row to another class: between two sweeps rows go L -> P, U -> P, P -> L, P -> U and
    (l = u rows) L -> U."""
    dt = np.dtype(dtype).type
    n = li.size
    rng = np.random.default_rng([seed, n, shift, 99])
    rank = np.cumsum(free) - 1
    cls = np.where(free, (rank + shift) % NCLASS, -1)
    finl, finu = np.isfinite(li), np.isfinite(ui)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = np.where(finl & finu, li + (ui - li) * dt(0.375), np.where(finl, li + dt(1), np.where(finu, ui - dt(1), dt(0.5))))
    y = mid.astype(dt)
    lam = (rng.standard_normal(n) + 0.01).astype(dt)
    mu = (rng.standard_normal(n) + 0.01).astype(dt)

    def put(arr, rows, vals):
        arr[rows] = np.asarray(vals, dt)[rows] if np.ndim(vals) else dt(vals)

    atl = finl & np.isin(cls, (0, 1, 2, 3, 16, 17))
    put(y, atl, li)
    for k, v in ((0, 1.5), (1, 0.0), (2, -0.0), (3, -0.5), (16, -0.5), (17, -0.5)):
        put(lam, atl & (cls == k), v)
    put(mu, atl & (cls == 3), 0.75)
    put(mu, atl & (cls == 16), -0.5)
    put(mu, atl & (cls == 17), 0.5)
    atu = finu & np.isin(cls, (4, 5, 6, 7))
    put(y, atu, ui)
    for k, v in ((4, 2.0), (5, 0.0), (6, -0.0), (7, -0.25)):
        put(mu, atu & (cls == k), v)
    put(lam, atu, -1.25)                                   # lam < 0: a row with l = u = y is decided by mu
    inf = dt(np.inf)
    put(y, finl & (cls == 8), np.nextafter(li, inf))
    put(y, finl & (cls == 9), np.nextafter(li, -inf))
    put(y, finu & (cls == 10), np.nextafter(ui, -inf))
    put(y, finu & (cls == 11), np.nextafter(ui, inf))
    put(y, finl & (cls == 12), li - dt(3))
    put(y, finu & (cls == 13), ui + dt(3))
    put(lam, cls == 14, -0.5)
    put(mu, cls == 14, -0.5)
    put(lam, cls == 15, 0.5)
    put(mu, cls == 15, 0.5)
    return y, lam, mu


def edge_classes(li, ui, free, y, lam, mu):
    """which of EDGE_LABELS the free rows of an input contain, read from the VALUES (not from the class numbers)"""
    f = free
    sgn = lambda a: np.signbit(a)  # noqa: E731
    has = {}
    has["y==l lam>0"] = (f & (y == li) & (lam > 0)).any()
    has["y==l lam=+0"] = (f & (y == li) & (lam == 0) & ~sgn(lam)).any()
    has["y==l lam=-0"] = (f & (y == li) & (lam == 0) & sgn(lam)).any()
    has["y==l lam<0"] = (f & (y == li) & (lam < 0)).any()
    has["y==u mu>0"] = (f & (y == ui) & (mu > 0)).any()
    has["y==u mu=+0"] = (f & (y == ui) & (mu == 0) & ~sgn(mu)).any()
    has["y==u mu=-0"] = (f & (y == ui) & (mu == 0) & sgn(mu)).any()
    has["y==u mu<0"] = (f & (y == ui) & (mu < 0)).any()
    has["l==u==y"] = (f & (li == ui) & (y == li)).any()
    finl, finu = np.isfinite(li), np.isfinite(ui)
    t = y.dtype.type
    has["y=l+ulp"] = (f & finl & (y == np.nextafter(li, t(np.inf))) & (li != ui)).any()
    has["y=l-ulp"] = (f & finl & (y == np.nextafter(li, t(-np.inf)))).any()
    has["y=u-ulp"] = (f & finu & (y == np.nextafter(ui, t(-np.inf))) & (li != ui)).any()
    has["y=u+ulp"] = (f & finu & (y == np.nextafter(ui, t(np.inf)))).any()
    has["l=-inf"] = (f & ~finl).any()
    has["u=+inf"] = (f & ~finu).any()
    has["y<l"] = (f & (y < li - t(1))).any()
    has["y>u"] = (f & (y > ui + t(1))).any()
    has["interior"] = (f & (y > li) & (y < ui)).any()
    return {k for k, v in has.items() if v}


def transitions(st_before, st_after):
    """the set changes of the free rows between two sweeps, as strings like "L->P" """
    names = {ST_L: "L", ST_U: "U", ST_P: "P"}
    out = set()
    a, b = st_before & ST_PART, st_after & ST_PART
    for x, nx in names.items():
        for y_, ny in names.items():
            if x != y_ and ((a == x) & (b == y_)).any():
                out.add("%s->%s" % (nx, ny))
    return out


def history(n, c, dtype, seed):
    """c pairs (s, y) of independent normal columns; returns (pairs in the order they are added, cols = [Y slots, S slots])"""
    dt = np.dtype(dtype).type
    rng = np.random.default_rng([seed, n, c, 31])
    pairs = [(rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)) for _ in range(c)]
    return pairs, [p[1] for p in pairs] + [p[0] for p in pairs]
