"""Exact references and acceptance criteria for the n-length sums of the bounded (L-BFGS-B) path: the Gram W_P'W_P, the
masked multi-dots W'v / W'd, the dots of add_correction.  No GPU, no oracle library; tests/test_bounded_sums_ref_cpu.py
proves what is here, tests/test_bounded_sums_gpu.py uses it.

The claim under test (csrc/reduce.cuh, include/lbfgsx.h): every such sum is the correctly rounded value of the exact sum,
and the un-rounded (hi, lo) pairs the carried Gram and the complement identity work with are good to far below an ulp.
Exact arithmetic comes from statement_ref (exact_dot, bracket, ulp); what is added here:

  exact_gram / exact_wtv   Fractions of sum_{i in rows} a_i b_i, columns in the ABI's logical order [Y slots, S slots]
  nearest                  the correctly rounded value, ties to even
  dd_bound                 a derived worst-case error of the TwoProd / TwoSum accumulators over ANY summation order
  sum_bound                the same, and 0 where the data prove the accumulator exact (f32 data, v = +-1)
  i8_bound                 the documented error of the integer-MFMA Gram (csrc/gram_i8.cuh), restated
  check_pair               |hi + lo - exact| <= B
  check_rounded            "ok" / "ambiguous-ok" / "wrong": only nearest(exact) passes unless the exact value lies within B
                           of a rounding boundary -- stricter than statement_ref.adjacent, because these kernels claim
                           correct rounding
  gp_linear_ref            the LBFGSX_GP_LINEAR prologue statement, one numpy operation per source operation
  family / build_case      the inputs of the GPU tests, fixed seeds, reproducible without a device

Final stores (read from the kernels, mirrored by the callers of check_rounded through `dtype`):
  * the one-pass Gram family (k_gram_dd + k_gram_finish, kx_gram + kx_gram_finish, k_vrows, kx_rows, k_gram_i8_final) stores
    acc.value() as a double, f32 contexts included: ONE rounding, to double -> dtype = float64;
  * the multi-dot family (k_multidot*, kx_multidot_mask, kx_list1, kx_multidot2*), the blocked k_gram and d.d of
    k_cauchy_build store double(T(acc.value())): for f32 contexts TWO roundings, to double and then to float -> dtype = T.

LBFGSX_GP_RHS is not here: its input vector rhs lives inside the context; tests/subspace_ref.py restates it (gp_rhs) and
tests/test_subspace_statements_gpu.py gives rhs a known value through lbfgsx_b_sub_upload and holds its sums to the criteria
above.
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

import statement_ref as R

ST_FREE, ST_NEWACT = 1, 2  # LBFGSX_ST_FREE, LBFGSX_ST_NEWACT (include/lbfgsx.h)
VS_DRT, VS_LBOUND, VS_UBOUND = 0, 3, 4
GP_NONE, GP_LINEAR = 0, 2


# ---------------------------------------------------------------- exact sums
def _rows(cols, rows):
    if rows is None:
        return list(cols)
    return [np.ascontiguousarray(c[rows]) for c in cols]


def exact_gram(cols, rows=None):
    """packed lower triangle, entry e = i (i + 1) / 2 + j (i >= j): Fraction of sum_{r in rows} cols[i][r] cols[j][r].  `rows`:
    boolean mask, index array or None (every row)."""
    sub = _rows(cols, rows)
    return [R.exact_dot(sub[i], sub[j]) for i in range(len(sub)) for j in range(i + 1)]


def exact_wtv(cols, v, rows=None):
    """[Fraction of sum_{r in rows} cols[k][r] v[r] for every k]"""
    sub = _rows(list(cols) + [v], rows)
    return [R.exact_dot(c, sub[-1]) for c in sub[:-1]]


def abs_gram(cols, rows=None):
    """sum |a_i b_i| of the same entries (exact): what the error bounds are relative to"""
    return exact_gram([np.abs(c) for c in cols], rows)


def abs_wtv(cols, v, rows=None):
    return exact_wtv([np.abs(c) for c in cols], np.abs(v), rows)


# ---------------------------------------------------------------- rounding
def _is_even(x, dtype):
    if np.dtype(dtype) == np.float64:
        return (int(np.float64(x).view(np.int64)) & 1) == 0
    return (int(np.float32(x).view(np.int32)) & 1) == 0


def midpoint(exact, dtype):
    """the rounding boundary of exact's bracket in dtype (None when exact is a dtype value)"""
    lo, hi = R.bracket(exact, dtype)
    if lo == hi:
        return None
    return (Fraction(lo) + Fraction(hi)) / 2


def nearest(exact, dtype):
    """the dtype value nearest to the exact real `exact`, ties to even (as a Python float)"""
    exact = Fraction(exact)
    lo, hi = R.bracket(exact, dtype)
    if lo == hi:
        return lo
    assert math.isfinite(lo) and math.isfinite(hi), "outside dtype's range"
    mid = (Fraction(lo) + Fraction(hi)) / 2
    if exact < mid:
        return lo
    if exact > mid:
        return hi
    return lo if _is_even(lo, dtype) else hi


def stored(exact, dtype):
    """what a kernel that holds the exact sum stores through double(T(acc.value())): nearest double, then (f32) nearest float"""
    d = nearest(exact, np.float64)
    if np.dtype(dtype) == np.float32:
        return float(np.float32(d))
    return d


# ---------------------------------------------------------------- bounds
_U = Fraction(1, 1 << 53)


def dd_bound(nrows, sum_abs):
    """2 (nrows 2^-53)^2 sum|a_i b_i|.

    Worst case of the accumulators of csrc/reduce.cuh over any summation order.  DD::add_prod is Dot2 of Ogita, Rump and
    Oishi (TwoProd by FMA, TwoSum, the error terms added in plain double); DD::merge is the same TwoSum on partial sums with
    the partners' error terms added in plain double and a renormalisation (FastTwoSum, error-free).  Every error-free
    transformation contributes nothing; what is lost are the roundings of the plain additions into `lo`, each at most 2^-53
    of a partial sum of error terms, which are themselves at most 2^-53 of partial sums of |a_i b_i|.  A value passes
    through at most one addition per row of its chain and the tree stages have fewer members than there are rows, so with
    gamma_k = k u / (1 - k u), u = 2^-53, the Dot2 bound gamma_n^2 sum|a_i b_i| (their Proposition 5.5 without the final
    rounding) holds with the chain length bounded by nrows; the factor 2 covers gamma_n against n u for every n < 2^26 and
    the f32 accumulator D1 (exact products, the same compensated sum).  Independent of the launch geometry, loose on purpose;
    one row gives 2^-105 |a b| although TwoProd alone is exact."""
    return 2 * (nrows * _U) ** 2 * Fraction(sum_abs)


def _lowbit_exp(a):
    """smallest exponent of the lowest set bit over the non-zero elements: every element is a multiple of 2^that (None when
    there is no non-zero element)"""
    a = np.asarray(a, np.float64)
    nz = a[a != 0]
    if nz.size == 0:
        return None
    m, e = np.frexp(nz)
    mant = np.abs(np.ldexp(m, 53)).astype(np.int64)   # exact, < 2^53
    low = mant & -mant
    tz = np.frexp(low.astype(np.float64))[1] - 1      # log2 of a power of two
    return int((e.astype(np.int64) - 53 + tz).min())


def sum_bound(nrows, sum_abs, a, b):
    """The bound used for a sum of products of the columns a and b: 0 where the arithmetic proves the accumulator exact,
    dd_bound elsewhere.  Tighter than dd_bound and derived from the data, never from a kernel's output.

    Let every element of a be a multiple of 2^la and every element of b of 2^lb (_lowbit_exp), q = 2^(la + lb).  Every
    product is a multiple of q; so is its rounding p (a multiple of its own ulp >= q when the product has more than 53
    bits) and TwoProd's error term e; so, by induction, are every partial sum `hi`, every TwoSum error term and `lo`, in
    any summation order and through DD::merge / D1::merge.  An error term is at most 2^-53 of a partial sum, i.e. at most
    2^-53 sum|ab|; an e is at most 2^-53 |ab|; only additions of two non-zero operands produce an error term, fewer than
    nrows of them in the chains and the trees together.  So what is added into lo, and lo itself, stays below
    2 nrows 2^-53 sum|ab|, and while that is below 2^53 q every one of those additions is exact: hi + lo IS the exact sum and
    value() = RN(hi + lo) its correct rounding, ties to even.  Hence B = 0 when 2 nrows sum|ab| < 2^106 q.
    That is the case for f32 data (24-bit elements, exact products) and for the bound selectors (v = +-1); there the exact
    sum has few bits below the double ulp and lands ON a rounding boundary in one entry out of eight or so -- with dd_bound
    every such tie would count as ambiguous, with B = 0 the kernels are held to ties-to-even."""
    la, lb = _lowbit_exp(a), _lowbit_exp(b)
    if la is None or lb is None:
        return Fraction(0)
    q = Fraction(2) ** (la + lb)
    if 2 * nrows * Fraction(sum_abs) < (1 << 106) * q:
        return Fraction(0)
    return dd_bound(nrows, sum_abs)


def i8_bound(nrows, cmax_i, cmax_j):
    """nrows 2^-80 cmax_i cmax_j: the error of the integer-MFMA Gram's un-rounded entry (i, j) against the exact sum.

    From csrc/gram_i8.cuh: column k is put on the grid 2^(E_k - 86), where 2^E_k is the power of two above the column's
    largest magnitude over ALL rows (colmax; 2^E_k <= 2 cmax_k), and cut into 11 signed radix-256 digits.
      * truncation: |x - grid(x)| < 2^(E_k - 86), so a product errs by less than 2^E_i 2^(E_j - 86) + 2^E_j 2^(E_i - 86)
        = 2^(E_i + E_j - 85) <= 2^-83 cmax_i cmax_j;
      * of the 121 digit products d_k d'_l 256^(k + l) the 55 with k + l < 10 are dropped: |d d'| <= 2^14 and there are s + 1
        pairs with k + l = s, so they sum to less than 2^14 sum_{s<10} (s + 1) 2^(8 s) < 2^89.4 grid units 2^(E_i + E_j - 172),
        i.e. below 2^(E_i + E_j - 82.6) <= 2^-80.6 cmax_i cmax_j;
    together below 2^-80 cmax_i cmax_j per row; the integer sums add nothing.  The bound is relative to the whole column's
    maximum, masked-out rows included: a masked-out row of magnitude 2^300 would coarsen the grid of every row, which is why
    the i8 cases keep masked-out rows at the scale of the others."""
    return nrows * Fraction(1, 1 << 80) * Fraction(float(cmax_i)) * Fraction(float(cmax_j))


# ---------------------------------------------------------------- criteria
def pair_error(hi, lo, exact):
    return abs(Fraction(float(hi)) + Fraction(float(lo)) - Fraction(exact))


def check_pair(hi, lo, exact, B, what=""):
    """asserts |hi + lo - exact| <= B for an un-rounded double-double sum"""
    assert math.isfinite(float(hi)) and math.isfinite(float(lo)), "%s: (hi, lo) = (%r, %r)" % (what, hi, lo)
    err = pair_error(hi, lo, exact)
    assert err <= B, "%s: (hi, lo) = (%r, %r) is off the exact sum %.20g by %.3g, bound %.3g" % (
        what, float(hi), float(lo), float(exact), float(err), float(B))


def is_ambiguous(exact, B, dtype):
    """the exact value lies within B of the rounding boundary of its bracket: either neighbour is a correct rounding of a
    value that is only known to within B.  For float32 (two roundings) the boundary that matters is the double one.  B = 0
    (sum_bound: the sum is provably exact) leaves no zone."""
    if B == 0:
        return False  # an exactly known sum has one correct rounding, ties to even
    mid = midpoint(exact, np.float64)
    return mid is not None and abs(Fraction(exact) - mid) <= B


def check_rounded(got, exact, B, dtype):
    """"ok": got is the stored value of the exact sum (nearest double; for float32 that double rounded to float).
    "ambiguous-ok": the exact sum lies within B of the midpoint of its double bracket and got comes from one of the two
    bracket values.  "wrong": everything else."""
    got = float(got)
    if not math.isfinite(got):
        return "wrong"
    if got == stored(exact, dtype) and (got != 0.0 or math.copysign(1.0, got) == math.copysign(1.0, stored(exact, dtype))):
        return "ok"
    if is_ambiguous(exact, B, dtype):
        lo, hi = R.bracket(exact, np.float64)
        cands = (lo, hi) if np.dtype(dtype) == np.float64 else (float(np.float32(lo)), float(np.float32(hi)))
        if got in cands:
            return "ambiguous-ok"
    return "wrong"


def judge(gots, exacts, bounds, dtype, cap, what=""):
    """check_rounded over a list of sums; asserts that none is wrong and that at most `cap` are ambiguous (a case with more
    says nothing about rounding and fails as uninformative instead of passing quietly).  Returns the number of ambiguous ones."""
    assert len(gots) == len(exacts) == len(bounds)
    amb = sum(1 for e, b in zip(exacts, bounds) if is_ambiguous(e, b, dtype))
    assert amb <= cap, "%s: %d of %d exact sums lie within their bound of a rounding boundary (cap %d): uninformative input" % (
        what, amb, len(exacts), cap)
    for k, (g, e, b) in enumerate(zip(gots, exacts, bounds)):
        verdict = check_rounded(g, e, b, dtype)
        assert verdict != "wrong", "%s[%d]: got %r, correctly rounded %r (exact %.20g, off by %.3g ulp, bound %.3g ulp)" % (
            what, k, float(g), stored(e, dtype), float(e), float((Fraction(float(g)) - e) / R.ulp(e, dtype)) if math.isfinite(float(g)) else math.nan,
            float(b / R.ulp(e, dtype)))
    return amb


# ---------------------------------------------------------------- a host-side double-double sum (what the mutations start from)
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    """error-free product of two doubles without an FMA: Dekker's, on the Veltkamp halves"""
    p = a * b
    ah, al = R._split(np.float64(a))
    bh, bl = R._split(np.float64(b))
    e = ((float(ah) * float(bh) - p) + float(ah) * float(bl) + float(al) * float(bh)) + float(al) * float(bl)
    return p, e


def dd_dot(a, b, chunks=1, drop_lo_at=None):
    """sum a_i b_i the way reduce.cuh forms it: `chunks` DD::add_prod chains merged left to right with DD::merge; returns
    (hi, lo).  drop_lo_at = k discards the partner's lo at merge k (the mutation "lo lost in a merge stage")."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    parts = []
    for ch in range(chunks):
        hi = lo = 0.0
        for x, y in zip(a[ch::chunks].tolist(), b[ch::chunks].tolist()):
            p, e = two_prod(x, y)
            s, err = two_sum(hi, p)
            lo += err + e
            hi = s
        parts.append((hi, lo))
    hi, lo = parts[0]
    for k, (ohi, olo) in enumerate(parts[1:]):
        if drop_lo_at == k:
            olo = 0.0
        s, err = two_sum(hi, ohi)
        lo += err + olo
        hi = s
        t = hi + lo
        lo = lo - (t - hi)
        hi = t
    return hi, lo


# ---------------------------------------------------------------- the prologue statement
def gp_linear_ref(cols, coef1, g, dt):
    """LBFGSX_GP_LINEAR on every row (the kernels evaluate it on the rows of the mask only): a = 0; a = a + col_j * T(coef_j)
    for the Y columns then the S columns, left to right in plain T; cF = T(-1) * a + g (coef1 NULL: cF = T(0) + g); v = -cF.
    Returns (cF, v)."""
    dt = np.dtype(dt).type
    if coef1 is None:
        cF = dt(0) + g
    else:
        a = np.zeros(g.shape, dt)
        for col, cf in zip(cols, coef1):
            a = a + col * dt(cf)
        cF = dt(-1) * a + g
    return cF, -cF


# ---------------------------------------------------------------- inputs
def family(name, n, ncols, seed, dtype):
    """(columns, base): "pos" = base (1 + 0.5 U(0, 1)) over a common normal base -- every product of two columns has the sign
    of base^2, sum|ab| / |sum ab| = 1; "indep" = independent normal columns, condition ~ sqrt(n); "spread" = "pos" with the
    rows scaled by 10^U(-6, 6).  base is None for "indep"."""
    rng = np.random.default_rng([seed, n, ncols, {"pos": 1, "indep": 2, "spread": 3}[name]])
    dt = np.dtype(dtype).type
    if name == "indep":
        return [rng.standard_normal(n).astype(dt) for _ in range(ncols)], None
    base = rng.standard_normal(n)
    if name == "spread":
        base = base * 10.0 ** rng.uniform(-6.0, 6.0, n)
    return [(base * (1.0 + 0.5 * rng.random(n))).astype(dt) for _ in range(ncols)], base


# family, rows, ring length, pairs added (c = min(npairs, m) are stored at the end), scalar type, mask kind, seed
Case = namedtuple("Case", "family n m npairs dtype mask seed")

K_FREE, K_FREE0, K_NEWACT, K_FIXED, K_INF = 0, 1, 2, 3, 4


def case_id(cs):
    return "%s-n%d-m%d-p%d-%s-%s-s%d" % (cs.family, cs.n, cs.m, cs.npairs, np.dtype(cs.dtype).name, cs.mask, cs.seed)


Built = namedtuple("Built", "case c pairs cols g lb ub kind state xcp drt dvec free newact")


def build_case(cs):
    """The host side of one GPU case.  x0 = 0, lb = -1, ub = 1; |g_i| is 0, about 0.5 or about 2, so that with the crossing
    threshold 1 the break point 1 / |g_i| puts row i in the free set (xcp_i = -g_i) or among the newly active rows
    (xcp_i = +-1) at will.  Mask kinds: "all" (every row free), "none" (no row free), "one@k" (row k free, the others newly
    active), "rand60" (60 % free -- a tenth of them with g = 0 --, 35 % newly active, 5 % with lb = ub = 0: in neither set),
    "rand60inf" (the same with some rows whose bounds are infinite: free whatever g is), "half" (a contiguous-free
    pattern of about half the rows: the compact-copy cases).
    In the "pos" and "spread" families g takes the sign that makes v = xcp - x0 share base's sign, so the v row is as well
    conditioned as the Gram."""
    n, dt = cs.n, np.dtype(cs.dtype).type
    rng = np.random.default_rng([cs.seed, n, cs.m, 77])
    raw, base = family(cs.family, n, 2 * cs.npairs, cs.seed, cs.dtype)
    # pair k = (s_k, y_k): y_k = raw[k], s_k = raw[npairs + k]; storage slot of pair k = k % m, the newest pair wins
    c = min(cs.npairs, cs.m)
    slot_pair = [max(k for k in range(cs.npairs) if k % cs.m == j) for j in range(c)]
    pairs = [(raw[cs.npairs + k], raw[k]) for k in range(cs.npairs)]
    cols = [raw[k] for k in slot_pair] + [raw[cs.npairs + k] for k in slot_pair]
    kind = np.full(n, K_NEWACT, np.int8)
    if cs.mask == "all":
        kind[:] = K_FREE
    elif cs.mask == "none":
        pass
    elif cs.mask.startswith("one@"):
        kind[int(cs.mask[4:]) % n] = K_FREE
    elif cs.mask in ("rand60", "rand60inf"):
        u = rng.random(n)
        kind[u < 0.60] = K_FREE
        kind[u < 0.06] = K_FREE0
        kind[u >= 0.95] = K_FIXED
        if cs.mask == "rand60inf":
            kind[(u >= 0.90) & (u < 0.95)] = K_INF
    elif cs.mask == "half":
        kind[rng.random(n) < 0.5] = K_FREE
    else:
        raise ValueError(cs.mask)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0) if base is None else np.where(base < 0, -1.0, 1.0)
    mag = np.where(kind == K_NEWACT, 1.5 + rng.random(n), 0.25 + 0.5 * rng.random(n))
    mag = np.where(kind == K_INF, 0.25 + 2.0 * rng.random(n), mag)
    mag[kind == K_FREE0] = 0.0
    g = (-sign * mag).astype(dt)          # v = -g has the sign of base
    lb, ub = np.full(n, -1, dt), np.full(n, 1, dt)
    lb[kind == K_FIXED] = 0
    ub[kind == K_FIXED] = 0
    lb[kind == K_INF] = -np.inf
    ub[kind == K_INF] = np.inf
    free = (kind == K_FREE) | (kind == K_FREE0) | (kind == K_INF)
    newact = kind == K_NEWACT
    state = np.where(free, ST_FREE, np.where(newact, ST_NEWACT, 0)).astype(np.uint8)
    # Cauchy.h:111-129: d_i = 0 where the break point is 0 (lb = ub), else -g_i; xcp = x0 + tfinal d on the free rows with
    # tfinal = 1, the bound d points to on the newly active ones, x0 elsewhere
    dvec = np.where(kind == K_FIXED, dt(0), -g).astype(dt)
    x0 = np.zeros(n, dt)
    xcp = np.where(free, x0 + dt(1) * dvec, np.where(newact, np.where(dvec > 0, ub, lb), x0)).astype(dt)
    drt = xcp - x0
    return Built(cs, c, pairs, cols, g, lb, ub, kind, state, xcp, drt, dvec, free, newact)


@functools.lru_cache(maxsize=4)
def built(cs):
    return build_case(cs)


Sums = namedtuple("Sums", "exact bound nrows")  # lists over the entries, and the number of rows summed


def _nrows(n, rows):
    if rows is None:
        return n
    rows = np.asarray(rows)
    return int(np.count_nonzero(rows)) if rows.dtype == bool else int(rows.size)


def _abs_dot(a, b, exact):
    """sum |a_i b_i|: the exact sum itself where no product is negative (the "pos" and "spread" families), else computed"""
    if exact >= 0 and not ((a < 0) != (b < 0))[(a != 0) & (b != 0)].any():
        return exact
    return R.exact_dot(np.abs(a), np.abs(b))


def gram_sums(cols, rows, i8_cmax=None):
    """exact packed Gram over `rows` with sum_bound (or, with the column maxima, i8_bound) per entry"""
    nrows = _nrows(len(cols[0]), rows)
    sub = _rows(cols, rows)
    t = len(sub)
    ex = exact_gram(sub)
    if i8_cmax is not None:
        bd = [i8_bound(nrows, i8_cmax[i], i8_cmax[j]) for i in range(t) for j in range(i + 1)]
    else:
        bd = [sum_bound(nrows, _abs_dot(sub[i], sub[j], ex[i * (i + 1) // 2 + j]), sub[i], sub[j]) for i in range(t) for j in range(i + 1)]
    return Sums(ex, bd, nrows)


def wtv_sums(cols, v, rows):
    """exact W'v over `rows` with sum_bound per entry"""
    nrows = _nrows(len(v), rows)
    sub = _rows(list(cols) + [v], rows)
    ex = exact_wtv(sub[:-1], sub[-1])
    bd = [sum_bound(nrows, _abs_dot(sub[k], sub[-1], ex[k]), sub[k], sub[-1]) for k in range(len(sub) - 1)]
    return Sums(ex, bd, nrows)


def cap_for(family_name, nentries, well_conditioned=True):
    """how many ambiguous entries a case may have and still say something: none where every product has one sign, one in
    twenty where the terms cancel ("indep", and any v that does not follow base's sign)"""
    return 0 if (family_name in ("pos", "spread") and well_conditioned) else nentries // 20


# ---------------------------------------------------------------- the cases of tests/test_bounded_sums_gpu.py
F64, F32 = np.float64, np.float32
ROW_NS = [1, 63, 64, 65, 129, 255, 257, 4095, 4097, 20011]
HISTORY_CS = [1, 4, 5, 7, 8, 10, 11, 13, 14, 15, 16, 20, 40]
N_HIST = 1501   # 24 batches of 64 rows, 6 blocks, a tail of 29 rows: every history length at one small row count

ROW_CASES = [Case("pos", n, c, c, F64, "rand60" if n >= 63 else "all", 1) for c in (2, 10) for n in ROW_NS]
LONG_CASES = [Case("pos", 300001, 4, 4, F64, "rand60", 2), Case("pos", 70001, 15, 15, F64, "rand60", 2)]
HISTORY_CASES = [Case("pos", N_HIST, c, c, F64, "rand60", 3) for c in HISTORY_CS]
WRAP_CASES = [Case("pos", N_HIST, m, m + 3, F64, "rand60", 4) for m in (5, 10)]
MASK_CASES = ([Case("pos", 321, 3, 3, F64, mk, 5) for mk in ("all", "none", "one@0", "one@63", "one@64", "one@320", "rand60inf")])
COMPACT_CASES = [Case("pos", 20011, 10, 10, F64, "half", 6), Case("pos", 20011, 3, 3, F64, "half", 6)]
HUGE_CASE = Case("pos", 4097, 4, 4, F64, "rand60", 7)      # masked-out rows of magnitude 2^300
FAMILY_CASES = [Case(f, 20011, c, c, F64, "rand60", 8) for f in ("spread", "indep") for c in (4, 10, 15)]
F32_CASES = [Case("pos", n, c, c, F32, "rand60", 9) for c in (2, 10, 20) for n in (65, 4097, 20011)]
NOSPLIT_CASES = [Case("pos", N_HIST, c, c, F64, "rand60", 3) for c in HISTORY_CS if c <= 15] + [
    Case("pos", 20011, 10, 10, F32, "rand60", 9)]
I8_CASES = [Case("pos", N_HIST, c, c, F64, "rand60", 3) for c in HISTORY_CS if 2 * c <= 30] + [
    Case("spread", 20011, 10, 10, F64, "rand60", 8), Case("indep", 20011, 15, 15, F64, "rand60", 8)]
I8_FLUSH_CASE = Case("pos", 8_000_003, 1, 1, F64, "all", 10)
CARRIED_CASES = [Case("pos", 20011, 6, 6, F64, "half", 11)]


def all_cases():
    seen, out = set(), []
    for cs in (ROW_CASES + LONG_CASES + HISTORY_CASES + WRAP_CASES + MASK_CASES + COMPACT_CASES + [HUGE_CASE] + FAMILY_CASES +
               F32_CASES + NOSPLIT_CASES + I8_CASES + [I8_FLUSH_CASE] + CARRIED_CASES):
        if cs not in seen:
            seen.add(cs)
            out.append(cs)
    return out


@functools.lru_cache(maxsize=None)
def case_sums(cs, mask):
    """(gram, wtv): the exact sums and dd bounds of the 2c x 2c Gram and of the v row (v = drt = xcp - x0) of case `cs` over the
    rows whose state has a bit of `mask` (0: every row).  Computed once per case and shared: the CPU preconditions and every
    GPU test of the case read the same objects and leave them unchanged."""
    bt = built(cs)
    if mask == 0 or (mask == ST_FREE and bt.free.all()):
        if mask != 0:
            return case_sums(cs, 0)
        rows = None
    else:
        rows = (bt.state & mask) != 0
    return gram_sums(bt.cols, rows), wtv_sums(bt.cols, bt.drt, rows)
