"""Python mirror of the reference's solver API over the native MI355X path.

Names, argument meaning and error behaviour follow yixuan/LBFGSpp:
  LBFGSParam / LBFGSBParam   -- reference include/LBFGSpp/Param.h:67-219, 224-377 (same fields and defaults)
  LBFGSSolver(param, linesearch).minimize(f, x)  -> (niter, fx)      reference include/LBFGS.h:78-173
  LBFGSBSolver(param).minimize(f, x, lb, ub)     -> (niter, fx)      reference include/LBFGSB.h:116-262
Exceptions: std::invalid_argument -> ValueError, std::logic_error -> ArithmeticError,
std::runtime_error -> RuntimeError (same messages).  `f` is a built-in device objective
(`DiagQuadratic(a, b)`, `ExtendedRosenbrock()`), the caller's own term compiled into the same kernels (`TermObjective(body)`,
`ChainObjective(body)` for terms that overlap, `GridObjective(body, shape)` for 2x2-cell terms on a grid, `VolumeObjective(body, shape)` for 2x2x2-cell terms on a 3-D array,
`PeriodicGridObjective(body, shape, periodic)` and `PeriodicVolumeObjective(body, shape, periodic)` for those two with wrap-around cells,
`GridFieldObjective(body, shape, D, periodic)` for a grid whose nodes carry D unknowns,
`StencilObjective(body, shape, periodic)` for 3x3-node terms on a grid, or
`GraphObjective(edge_body, edges)` for edge terms over an index list,
`MeshObjective(elem_body, elements, dim)` for K-node elements with vector unknowns, or
`LinearObjective(row_body, (rowptr, col, val), n)` for a linear model over a sparse matrix, or
`GraphLinearObjective(row_body, (rowptr, col, val), (ei, ej), edge_body, n)` for one with an edge term over a graph on its weights, or
`MultiLinearObjective(row_body, (rowptr, col, val), features, outputs)` for one with several outputs per row, or
`DenseLinearObjective(row_body, matrix, outputs)` for one over a dense matrix)
or the caller's own callable, `DeviceObjective(fn)`: fn(x, grad) -> float on torch
tensors that alias the library's device vectors.  All O(n) work of the solver runs in the HIP library, Python only passes
pointers.  There is no CPU fallback: without the built extension or a GPU these calls raise.
"""
import ctypes as C
import math

import numpy as np

from . import _lib as L

_NP = {L.F64: np.float64, L.F32: np.float32}


class LBFGSParam:
    """Reference Param.h:168-184 defaults."""

    def __init__(self, **kw):
        self.m = 6
        self.epsilon = 1e-5
        self.epsilon_rel = 1e-5
        self.past = 0
        self.delta = 0.0
        self.max_iterations = 0
        self.linesearch = 3  # LBFGS_LINESEARCH_BACKTRACKING_STRONG_WOLFE
        self.max_linesearch = 20
        self.min_step = 1e-20
        self.max_step = 1e20
        self.ftol = 1e-4
        self.wolfe = 0.9
        self.max_submin = 10
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def _c(self):
        return L.Params(m=self.m, epsilon=self.epsilon, epsilon_rel=self.epsilon_rel, past=self.past,
                        delta=self.delta, max_iterations=self.max_iterations, linesearch=self.linesearch,
                        max_linesearch=self.max_linesearch, min_step=self.min_step, max_step=self.max_step,
                        ftol=self.ftol, wolfe=self.wolfe, max_submin=self.max_submin)


class LBFGSBParam(LBFGSParam):
    """Reference Param.h:327-343 defaults (past = 1, delta = 1e-10, max_submin = 10)."""

    def __init__(self, **kw):
        super().__init__(**{**dict(past=1, delta=1e-10), **kw})


class DiagQuadratic:
    """f(x) = 0.5*||a.*x - b||^2 ; a, b host arrays, or None when generated on the device."""
    objective = L.OBJ_DIAG_QUAD

    def __init__(self, a=None, b=None):
        self.a, self.b = a, b


class ExtendedRosenbrock:
    """sum over pairs (1-x0)^2 + 100 (x1-x0^2)^2 in the reference's example form."""
    objective = L.OBJ_EXT_ROSENBROCK
    a = b = None


class DeviceObjective:
    """The caller's objective on device memory: fn(x, grad) -> float.  x and grad are 1-D torch tensors that ALIAS the
    solver's own device vectors (no copy; on the solver's device, of its dtype): fn fills grad in place and returns f(x).
    They are valid during the call only.  An exception raised by fn ends the minimisation and reaches the caller of
    minimize() as itself (solver.last.status == LBFGSX_E_USER); a non-finite value is left to the line search, as in the
    reference.  Usable wherever DiagQuadratic / ExtendedRosenbrock are."""

    def __init__(self, fn):
        if not callable(fn):
            raise TypeError("DeviceObjective: fn must be callable as fn(x, grad) -> float")
        L.require_torch("DeviceObjective")
        self.fn = fn

    @classmethod
    def from_autograd(cls, loss):
        """fn built from a scalar-valued torch function of x: the gradient comes from torch.autograd.grad."""
        if not callable(loss):
            raise TypeError("DeviceObjective.from_autograd: loss must be callable as loss(x) -> scalar tensor")
        torch = L.require_torch("DeviceObjective.from_autograd")

        def fn(x, grad):
            with torch.enable_grad():
                xv = x.detach().requires_grad_(True)
                f = loss(xv)
                (g,) = torch.autograd.grad(f, xv)
            grad.copy_(g)
            return float(f.detach())
        return cls(fn)


class TermObjective:
    """An objective that is a sum of terms over K consecutive coordinates (K = 1 or 2), given as HIP/C++ text for ONE term
    and compiled at run time into the fused kernels the built-in objectives use (include/lbfgsx.h, "term objectives").
    The body sees T (scalar type), const T x[K], T g[K] (to fill), int64_t i (index of x[0]), const T* p0..p3 (`data`) and
    T c[8] (`scalars`) and returns the term's value; f is the sum of the returned values.

        rosen = TermObjective("const T t1 = T(1) - x[0]; const T t2 = T(10) * (x[1] - x[0] * x[0]);"
                              "g[1] = T(20) * t2; g[0] = T(-2) * (x[0] * g[1] + t1); return t1 * t1 + t2 * t2;", K=2)

    data: up to four per-coordinate arrays of n elements -- numpy arrays (copied to the device at every minimise) or torch
    tensors on the solver's device (used in place); scalars: up to eight numbers.  Both may be replaced between minimises
    (set_data / set_scalars): the compiled code is kept.  Usable wherever ExtendedRosenbrock / DeviceObjective are, except
    with the Gram-space recursion, row shards and the lock-step batch.  A body that does not compile raises ValueError with
    the compiler's log (line numbers count from the body's first line)."""
    MAX_DATA, MAX_SCALARS = 4, 8
    # what ChainObjective replaces: the name in messages, the K accepted, the two entry points of the library
    _NAME, _KS, _K_RULE = "TermObjective", (1, 2), "a term reads K = 1 or K = 2 consecutive coordinates"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile", "lbfgsx_objective_source"

    def __init__(self, body, K=1, data=(), scalars=()):
        if K not in self._KS:
            raise ValueError("%s: K = %r is not supported: %s" % (self._NAME, K, self._K_RULE))
        self.body, self.K = str(body), int(K)
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    def set_data(self, *data):
        if len(data) > self.MAX_DATA:
            raise ValueError("%s: %d data arrays given, at most %d (p0..p3) are supported" % (self._NAME, len(data), self.MAX_DATA))
        self.data = tuple(data)

    def set_scalars(self, *scalars):
        if len(scalars) > self.MAX_SCALARS:
            raise ValueError("%s: %d scalars given, at most %d (c[0..7]) are supported"
                             % (self._NAME, len(scalars), self.MAX_SCALARS))
        self.scalars = tuple(float(v) for v in scalars)

    def source(self, dtype=np.float64):
        """The translation unit the library generates around the body."""
        core, _ = L.load()
        dt = L.F64 if np.dtype(dtype) == np.float64 else L.F32
        source = getattr(core, self._SOURCE)
        need = source(dt, *self._form_args(), self.body.encode(), None, 0)
        L.check(min(need, 0))
        buf = C.create_string_buffer(int(need))
        source(dt, *self._form_args(), self.body.encode(), buf, need)
        return buf.value.decode()

    def compile(self, dtype=np.float64):
        """Compile for gfx950 (no device needed) or fetch from the process-wide cache; returns the handle."""
        core, _ = L.load()
        dt = L.F64 if np.dtype(dtype) == np.float64 else L.F32
        if dt not in self._h:
            h = C.c_void_p()
            log = C.create_string_buffer(1 << 16)
            rc = getattr(core, self._COMPILE)(C.byref(h), dt, *self._form_args(), self.body.encode(), log, len(log))
            if rc == L.E_INVALID:
                raise ValueError("%s: the body does not compile\n" % self._NAME + log.value.decode(errors="replace"))
            L.check(rc, log.value.decode(errors="replace"))
            self._h[dt] = h
        return self._h[dt]

    def info(self, dtype=np.float64):
        """{vgprs, scratch_bytes, cache_hit, compile_ms, scratch_by_kernel} of the compiled code object."""
        core, _ = L.load()
        arr = (C.c_longlong * 8)()
        L.check(core.lbfgsx_objective_info(self.compile(dtype), C.byref(arr)))
        return {"vgprs": arr[0], "scratch_bytes": arr[1], "cache_hit": bool(arr[2]), "compile_ms": arr[3],
                "scratch_by_kernel": dict(zip(("k_eval", "k_trial", "k_b_eval", "k_b_dg_maxstep_trial"), list(arr)[4:8]))}

    def _form_args(self):
        """what the form's compile and source entry points take between dtype and body"""
        return (self.K,)

    def _check_n(self, n):
        if n % self.K:
            raise ValueError("TermObjective: n = %d is not a multiple of K = %d" % (n, self.K))

    def _data_sizes(self, n):
        """the element counts a data array may have"""
        return (n,)

    def __del__(self):
        try:
            core, _ = L.load()
            for h in self._h.values():
                core.lbfgsx_objective_destroy(h)
            self._h = {}
        except Exception:
            pass


class ChainObjective(TermObjective):
    """An objective whose terms OVERLAP: f(x) = sum over t = 0 .. n-K of phi(x[t], .., x[t+K-1]; t) with K = 2 or 3, one term
    starting at every coordinate -- the chained Rosenbrock function, difference regularisers, nearest-neighbour energies
    (include/lbfgsx.h, "chain objectives").  The body is a TermObjective's: it sees T, const T x[K], T g[K] (the term's K
    partial derivatives, to fill), int64_t i (index of x[0]), p0..p3 and c[8], may read p0[i] .. p0[i+K-1], and returns the
    term's value.  grad[j] is the sum of the g_t[j-t] of the terms that cover j, in ascending t.

        chained = ChainObjective("const T u = x[1] - x[0] * x[0]; const T v = T(1) - x[0]; g[1] = T(200) * u;"
                                 "g[0] = T(-400) * (u * x[0]) - T(2) * v; return T(100) * (u * u) + v * v;", K=2)

    Any n >= K.  data, scalars, set_data, set_scalars, source, compile and info as for a TermObjective (scratch_by_kernel
    names the four kernels by their counterparts); usable wherever one is, refused where one is."""
    _NAME, _KS, _K_RULE = "ChainObjective", (2, 3), "a chain term reads K = 2 or K = 3 consecutive coordinates"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_chain", "lbfgsx_objective_source_chain"

    def __init__(self, body, K=2, data=(), scalars=()):
        super().__init__(body, K, data, scalars)

    def _check_n(self, n):
        if n < self.K:
            raise ValueError("ChainObjective: n = %d is less than K = %d: there is no term" % (n, self.K))


class _LatticeObjective(TermObjective):
    """What the six forms on a regular array share: a shape of one extent per axis, each at least _MIN; for a form with a
    mask (_MASKED) the axes that wrap; for the field form D unknowns per node; and the solver's entry point (_ENTRY), which
    takes the shape and the mask.  A class states these as attributes and keeps its own signature."""
    _AXES, _MIN, _EXTENT_RULE = ("rows", "cols"), 2, "a grid has at least 2 rows and 2 columns"
    _MASKED = False       # periodic is taken, as a tuple of flags per axis
    _MASK_NUMBER = False  # ... or as the mask itself
    _HAS_D = False        # D is taken: it goes to the compiler and multiplies into n
    _CELL, _ENTRY = 4, None

    def _lattice_init(self, body, shape, data, scalars, periodic=None, D=None):
        try:
            shape = tuple(int(v) for v in shape)
            if len(shape) != len(self._AXES):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("%s: shape must be (%s)" % (self._NAME, ", ".join(self._AXES))) from None
        if min(shape) < self._MIN:
            raise ValueError("%s: shape = %s: %s" % (self._NAME, self._shape_text(shape), self._EXTENT_RULE))
        self.shape = shape
        if self._HAS_D:
            if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or D not in (1, 2, 3):
                raise ValueError("%s: D = %r is not supported: a node has D = 1, 2 or 3 unknowns" % (self._NAME, D))
            self.D = int(D)
        if self._MASKED:
            if self._MASK_NUMBER and isinstance(periodic, (int, np.integer)) and not isinstance(periodic, (bool, np.bool_)):
                if not 0 <= periodic <= 3:
                    raise ValueError("%s: periodic = %d: the mask has bit 0 for the column direction and bit 1 for the "
                                     "row direction (0 .. 3)" % (self._NAME, periodic))
                self.periodic = int(periodic)
            else:
                self.periodic = _periodic_mask(self._NAME, periodic, self._AXES)
        self.body, self.K = str(body), self._CELL
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    @staticmethod
    def _shape_text(shape):
        return "(%s)" % ", ".join("%d" % v for v in shape)

    def _form_args(self):
        return (self.D,) if self._HAS_D else ()

    def _check_n(self, n):
        D = self.D if self._HAS_D else 1
        if math.prod(self.shape) * D != n:
            raise ValueError("%s: shape = %s%s does not multiply to n = %d"
                             % (self._NAME, self._shape_text(self.shape), ", D = %d" % D if self._HAS_D else "", n))

    def _entry_args(self):
        """what the solver's entry point takes between the handle and the data"""
        return self.shape + ((self.periodic,) if self._MASKED else ())


class GridObjective(_LatticeObjective):
    """An objective on a 2-D grid: x is a row-major rows x cols array (flattened, n = rows*cols, rows >= 2, cols >= 2) and
    f(x) = sum over the (rows-1)(cols-1) cells of phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c) -- the MINPACK-2 energies
    (a cell covers both triangles of their discretisation), smoothness terms of image problems, membrane and Allen-Cahn
    energies (include/lbfgsx.h, "grid objectives").  The body is the text of ONE CELL: it sees T, const T x[4] in the order
    above, T g[4] (the cell's four partial derivatives, to fill), int64_t i (the flat index of x[0], row*cols + col),
    int64_t row, col, rows, cols, p0..p3 and c[8], may read p0[i], p0[i+1], p0[i+cols] and p0[i+cols+1], and returns the
    cell's value.  grad[r,c] is g[3] of cell (r-1,c-1) + g[2] of cell (r-1,c) + g[1] of cell (r,c-1) + g[0] of cell (r,c),
    those that exist, in this order.

        membrane = GridObjective("const T a = x[1] - x[0]; const T b = x[2] - x[0];"
                                 "g[0] = T(0) - a - b; g[1] = a; g[2] = b; g[3] = T(0);"
                                 "return T(0.5) * (a * a + b * b);", shape=(rows, cols))

    A per-node term is written inside the body: node (row, col) goes to the cell that starts there, and the cells of the last
    row and column of cells pick up the nodes no cell starts at (row + 2 == rows, col + 2 == cols).  A denoiser with data p0
    and fidelity weight c[0] appends this to the membrane body in place of its return:

        T v = T(0.5) * (a * a + b * b);
        const bool lastc = col + 2 == cols, lastr = row + 2 == rows;
        const T r0 = x[0] - p0[i];
        g[0] = g[0] + c[0] * r0;  v = v + T(0.5) * (c[0] * (r0 * r0));
        if (lastc) { const T r1 = x[1] - p0[i + 1];  g[1] = g[1] + c[0] * r1;  v = v + T(0.5) * (c[0] * (r1 * r1)); }
        if (lastr) { const T r2 = x[2] - p0[i + cols];  g[2] = g[2] + c[0] * r2;  v = v + T(0.5) * (c[0] * (r2 * r2)); }
        if (lastr && lastc) { const T r3 = x[3] - p0[i + cols + 1];  g[3] = g[3] + c[0] * r3;  v = v + T(0.5) * (c[0] * (r3 * r3)); }
        return v;

    data, scalars, set_data, set_scalars, source, compile and info as for a TermObjective (scratch_by_kernel names the four
    kernels by their counterparts); usable wherever a ChainObjective is, refused where one is.  minimize raises ValueError
    when rows*cols != len(x)."""
    _NAME = "GridObjective"
    _COMPILE, _SOURCE, _ENTRY = "lbfgsx_objective_compile_grid", "lbfgsx_objective_source_grid", "lbfgsx_solver_minimize_grid"

    def __init__(self, body, shape, data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars)


class VolumeObjective(_LatticeObjective):
    """An objective on a 3-D array: x is a slab-major slabs x rows x cols array (flattened, n = slabs*rows*cols, every extent
    >= 2; node (s, r, c) has flat index (s*rows + r)*cols + c) and f(x) = sum over the (slabs-1)(rows-1)(cols-1) cells of
    phi(x[8]; s, r, c) with x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc] -- volumetric denoising, 3-D phase-field and Allen-Cahn
    energies, tomographic volumes under bounds, obstacle problems in 3-D (include/lbfgsx.h, "volume objectives").  The body is
    the text of ONE CELL: it sees T, const T x[8], T g[8] (the cell's eight partial derivatives, to fill), int64_t i (the flat
    index of x[0]), int64_t slab, row, col, slabs, rows, cols, p0..p3 and c[8], may read p0 at the cell's eight corners
    (p0[i + dc + dr*cols + ds*rows*cols]), and returns the cell's value.  grad[s,r,c] is g[7] of cell (s-1,r-1,c-1) + g[6] of
    (s-1,r-1,c) + g[5] of (s-1,r,c-1) + g[4] of (s-1,r,c) + g[3] of (s,r-1,c-1) + g[2] of (s,r-1,c) + g[1] of (s,r,c-1) + g[0] of
    (s,r,c), those that exist, in this order.

        dirichlet = VolumeObjective("const T a = x[1] - x[0]; const T b = x[2] - x[0]; const T e = x[4] - x[0];"
                                    "for (int k = 0; k < 8; k++) g[k] = T(0);"
                                    "g[0] = (T(0) - a - b) - e; g[1] = a; g[2] = b; g[4] = e;"
                                    "return T(0.5) * ((a * a + b * b) + e * e);", shape=(slabs, rows, cols))

    A per-node term is written inside the body as for a GridObjective: node (slab, row, col) goes to the cell that starts
    there, and the last layer of cells in each direction picks up the nodes no cell starts at -- the cell adds the node term of
    its corner (ds, dr, dc) iff (ds == 0 or slab + 2 == slabs) and (dr == 0 or row + 2 == rows) and (dc == 0 or
    col + 2 == cols), with the matching addition to g[4*ds + 2*dr + dc]; every node is then counted once.

    data, scalars, set_data, set_scalars, source, compile and info as for a TermObjective (scratch_by_kernel names the four
    kernels by their counterparts); usable wherever a GridObjective is, refused where one is.  minimize raises ValueError
    when slabs*rows*cols != len(x)."""
    _NAME = "VolumeObjective"
    _COMPILE, _SOURCE, _ENTRY = "lbfgsx_objective_compile_volume", "lbfgsx_objective_source_volume", "lbfgsx_solver_minimize_volume"
    _AXES, _EXTENT_RULE, _CELL = ("slabs", "rows", "cols"), "a volume has at least 2 slabs, 2 rows and 2 columns", 8

    def __init__(self, body, shape, data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars)


def _periodic_mask(name, periodic, axes):
    """the mask of a periodic form from its tuple of flags, outermost axis first: bit 0 the column direction"""
    try:
        flags = tuple(periodic)
    except TypeError:
        flags = ()
    if len(flags) != len(axes):
        raise ValueError("%s: periodic must have one flag per axis, (%s)" % (name, ", ".join(axes)))
    for v in flags:
        if not isinstance(v, (bool, np.bool_)) and not (isinstance(v, (int, np.integer)) and v in (0, 1)):
            raise ValueError("%s: periodic = %r: a flag is True or False" % (name, periodic))
    return sum(1 << k for k, v in enumerate(reversed(flags)) if v)


class PeriodicGridObjective(_LatticeObjective):
    """A GridObjective with wrap-around cells (include/lbfgsx.h, "periodic grid and volume objectives"): periodic = (rows,
    cols) says which directions wrap.  Cell (r, c) has the corners x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1] with + modulo the
    extent and exists iff (c < cols-1 or the columns wrap) and (r < rows-1 or the rows wrap); with periodic = (False, False)
    this is a GridObjective.  The body sees what a GridObjective's sees, plus const int64_t j[4], the flat indices of its four
    corners (j[0] == i), and int periodic (bit 0: columns, bit 1: rows).  It reads data as p0[j[k]]: p0[i + 1] and
    p0[i + cols] are wrong at a seam.  grad[r,c] is g[3] of cell (r-1,c-1) + g[2] of (r-1,c) + g[1] of (r,c-1) + g[0] of
    (r,c) with - modulo the extent on a periodic axis, those that exist, in this order.

        torus = PeriodicGridObjective("const T a = x[1] - x[0]; const T b = x[2] - x[0];"
                                      "g[0] = T(0) - a - b; g[1] = a; g[2] = b; g[3] = T(0);"
                                      "return T(0.5) * (a * a + b * b);", shape=(rows, cols))

    A per-node term goes to the cell that starts at the node; on an open axis the last layer of cells picks up the nodes no
    cell starts at (if (!(periodic & 1) && col + 2 == cols) ...), on a periodic axis there is nothing to pick up.  Everything
    else as for a GridObjective; usable wherever one is, refused where one is."""
    _NAME, _MASKED = "PeriodicGridObjective", True
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_grid_periodic", "lbfgsx_objective_source_grid_periodic"
    _ENTRY = "lbfgsx_solver_minimize_grid_periodic"

    def __init__(self, body, shape, periodic=(True, True), data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars, periodic)


class PeriodicVolumeObjective(_LatticeObjective):
    """A VolumeObjective with wrap-around cells: periodic = (slabs, rows, cols) says which directions wrap.  Cell (s, r, c) has
    the corners x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc] with + modulo the extent and exists iff, per axis, its origin is not
    in the last layer or the axis wraps; with no axis periodic this is a VolumeObjective.  The body sees what a
    VolumeObjective's sees, plus const int64_t j[8], the flat indices of its eight corners (j[0] == i), and int periodic (bit
    0: columns, bit 1: rows, bit 2: slabs); it reads data as p0[j[k]].  The gradient's order is the VolumeObjective's, with
    wrapped indices.  Everything else as for a VolumeObjective; usable wherever one is, refused where one is."""
    _NAME, _MASKED = "PeriodicVolumeObjective", True
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_volume_periodic", "lbfgsx_objective_source_volume_periodic"
    _ENTRY = "lbfgsx_solver_minimize_volume_periodic"
    _AXES, _EXTENT_RULE, _CELL = VolumeObjective._AXES, VolumeObjective._EXTENT_RULE, 8

    def __init__(self, body, shape, periodic=(True, True, True), data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars, periodic)


class GridFieldObjective(_LatticeObjective):
    """A PeriodicGridObjective whose nodes carry D = 1, 2 or 3 unknowns (include/lbfgsx.h, "grid field objectives"): complex
    Ginzburg-Landau lattices, Heisenberg films, optical flow and 2-D elasticity, multi-channel image models.  x is node-major,
    x[(r*cols + c)*D + d], n = rows*cols*D; periodic = (rows, cols) says which directions wrap, (False, False) is the open
    grid.  The body is the text of one cell and sees T, constexpr int D, const T x[4*D] and T g[4*D] (x[k*D + d]: unknown d of
    corner k, the corners in a GridObjective's order), int64_t i, row, col, const int64_t j[4] (the NODE indices of the
    corners, j[0] == i: the flat coordinate of x[k*D + d] is j[k]*D + d), rows, cols, int periodic, p0..p3 and c[8].  For every
    d, grad[(r,c), d] is g[3*D+d] of cell (r-1,c-1) + g[2*D+d] of (r-1,c) + g[D+d] of (r,c-1) + g[d] of (r,c) with - modulo the
    extent on a periodic axis, those that exist, in this order.  At D = 1 the text of a PeriodicGridObjective compiles unchanged.

        gl = GridFieldObjective("T v = T(0); for (int d = 0; d < D; d++) { const T a = x[D + d] - x[d], b = x[2 * D + d] - x[d];"
                                " g[d] = T(0) - a - b; g[D + d] = a; g[2 * D + d] = b; g[3 * D + d] = T(0);"
                                " v += T(0.5) * (a * a + b * b); } return v;", shape=(rows, cols), D=2, periodic=(True, True))

    Everything else as for a PeriodicGridObjective; usable wherever one is, refused where one is."""
    _NAME, _MASKED, _HAS_D = "GridFieldObjective", True, True
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_grid_field", "lbfgsx_objective_source_grid_field"
    _ENTRY = "lbfgsx_solver_minimize_grid_field"

    def __init__(self, body, shape, D, periodic=(False, False), data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars, periodic, D)


class StencilObjective(_LatticeObjective):
    """An objective of 3x3-node terms on a 2-D grid (include/lbfgsx.h, "grid stencil objectives"): energies that need a second
    difference at a node -- plate bending and thin-plate splines, sum (Laplace u)^2, Swift-Hohenberg and phase-field-crystal
    functionals, second-order TV priors, 3x3 clique priors, anything on a 9-point stencil.  x is a row-major rows x cols array
    (flattened, n = rows*cols, rows >= 3, cols >= 3).  periodic is the mask of a PeriodicGridObjective as a number, bit 0 the
    columns and bit 1 the rows (0 = the open grid, 3 = the torus), or its tuple of flags (rows, cols).  Patch (r, c) has the
    nodes x[3*dr + dc] = x[r+dr, c+dc], dr, dc = 0, 1, 2, with + modulo the extent (its centre is x[4]) and exists iff
    (c < cols-2 or the columns wrap) and (r < rows-2 or the rows wrap).  The body is the text of ONE PATCH: it sees T,
    const T x[9], T g[9] (the patch's nine partial derivatives, to fill), int64_t i, row, col (those of x[0]), const int64_t
    j[9] (the flat indices of the nine nodes, j[0] == i), rows, cols, int periodic, p0..p3 and c[8], reads data as p0[j[k]],
    and returns the patch's value.  grad[r,c] is the sum of g[3*dr + dc] of patch (r-dr, c-dc) over dr = 2, 1, 0 (outer) and
    dc = 2, 1, 0 (inner) with - modulo the extent on a periodic axis, those that exist, in this order.

        plate = StencilObjective("const T l = (((x[1] + x[3]) + x[5]) + x[7]) - T(4) * x[4];"
                                 "for (int k = 0; k < 9; k++) g[k] = T(0);"
                                 "g[1] = l; g[3] = l; g[5] = l; g[7] = l; g[4] = T(-4) * l;"
                                 "return T(0.5) * (l * l);", shape=(rows, cols), periodic=3)

    A per-node term is written inside the body: the patch adds the term of its node (dr, dc) iff (dr == 0 or (the rows do not
    wrap and row + 3 == rows)) and (dc == 0 or (the columns do not wrap and col + 3 == cols)); every node is then counted
    once.  Everything else as for a PeriodicGridObjective; usable wherever one is, refused where one is."""
    _NAME, _MASKED, _MASK_NUMBER = "StencilObjective", True, True
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_grid_stencil", "lbfgsx_objective_source_grid_stencil"
    _ENTRY = "lbfgsx_solver_minimize_grid_stencil"
    _MIN, _EXTENT_RULE, _CELL = 3, "a 3x3 patch needs at least 3 rows and 3 columns", 9

    def __init__(self, body, shape, periodic=0, data=(), scalars=()):
        self._lattice_init(body, shape, data, scalars, periodic)


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


class GraphObjective(TermObjective):
    """An objective on a graph: x has one coordinate per node, the E edges are (ei[e], ej[e]), and
    f(x) = sum over nodes v of psi(x[v]; v) + sum over edges e of phi(x[ei[e]], x[ej[e]]; e) -- spring and finite-element
    energies on an unstructured mesh, graph-Laplacian regularisers, XY and synchronisation energies, pairwise-comparison
    losses (include/lbfgsx.h, "graph objectives").  edge_body sees T, const T x[2] (x at ei[e] and at ej[e], in the edge's own
    orientation), T g[2] (to fill), int64_t e, i, j (the edge's index and its two nodes), p0..p3 and c[8] and returns the
    edge's value; node_body (optional) sees T, const T x[1], T g[1], int64_t i, p0..p3 and c[8] and returns the node's value.
    grad[v] is the node term's g[0], then the g_e[side] of the edges incident to v in ascending e.

        springs = GraphObjective("const T d = x[0] - x[1]; const T w = p0[e] * d; g[0] = w; g[1] = T(0) - w;"
                                 "return T(0.5) * (w * d);", edges=(ei, ej), data=(weights,),
                                 node_body="const T r = x[0] - p1[i]; g[0] = r; return T(0.5) * (r * r);")

    edges: two integer numpy arrays or torch tensors of equal length E >= 1; they are range-checked and converted to int32 on
    the host here, and copied, validated (0 <= index < n, ei[e] != ej[e]) and turned into the incidence list on the device at
    every minimise.  Each data[k] has n (per node) or E (per edge) elements.  set_data, set_scalars, source, compile and info
    as for a TermObjective; usable wherever a GridObjective is, refused where one is."""
    _NAME = "GraphObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_graph", "lbfgsx_objective_source_graph"

    def __init__(self, edge_body, edges, node_body=None, data=(), scalars=()):
        try:
            ei, ej = edges
        except (TypeError, ValueError):
            raise ValueError("GraphObjective: edges must be a pair (ei, ej) of integer arrays") from None
        self.ei, self.ej = self._indices(ei, "ei"), self._indices(ej, "ej")
        if self.ei.size != self.ej.size:
            raise ValueError("GraphObjective: ei has %d elements and ej has %d: one pair per edge" % (self.ei.size, self.ej.size))
        if self.ei.size < 1:
            raise ValueError("GraphObjective: E = 0: a graph objective has at least one edge")
        self.E = int(self.ei.size)
        self.body, self.K = str(edge_body), 2
        self.node_body = None if not node_body else str(node_body)
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    @staticmethod
    def _indices(a, name):
        if _is_torch(a):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("GraphObjective: %s must be a 1-D integer array, not %s with %d dimensions" % (name, a.dtype, a.ndim))
        if a.size:
            lo, hi = int(a.min()), int(a.max())
            for v in (lo, hi):
                if v < -2 ** 31 or v > 2 ** 31 - 1:
                    raise ValueError("GraphObjective: %s holds %d, which does not fit a 32-bit node index" % (name, v))
        return np.ascontiguousarray(a, np.int32)

    def _form_args(self):
        return (self.node_body.encode() if self.node_body else None,)

    def _check_n(self, n):
        if n > 2 ** 31 - 1:
            raise ValueError("GraphObjective: n = %d exceeds 2^31 - 1: node indices are int32" % n)

    def _data_sizes(self, n):
        return (n, self.E)


class MeshObjective(TermObjective):
    """An objective on a mesh: N nodes with D = dim unknowns each (x node-major, x[v*D + d], n = N*D), E elements of K nodes
    each as an (E, K) connectivity table, K in {2, 3, 4}, D in {1, 2, 3}, and
    f(x) = sum over nodes v of psi(x_v; v) + sum over elements e of phi(x at the K nodes of e; e) (include/lbfgsx.h, "mesh
    objectives").  elem_body sees T, K, D, const T x[K*D] (x[k*D + d]: unknown d of the node in slot k), T g[K*D] (to fill),
    int64_t e, const int64_t v[K], p0..p3 and c[8] and returns the element's value; node_body (optional) sees T, D,
    const T x[D], T g[D], int64_t i, p0..p3, c[8].  grad[v*D + d] is the node term's g[d], then the g_e[slot*D + d] of the
    elements that contain v in ascending e.

        springs = MeshObjective("T s = T(0); for (int d = 0; d < D; d++) { const T u = x[d] - x[D + d]; s = s + u * u; }"
                                "const T r = s - p0[e];"
                                "for (int d = 0; d < D; d++) { const T u = x[d] - x[D + d]; g[d] = r * u; g[D + d] = T(0) - r * u; }"
                                "return T(0.25) * (r * r);", elements=pairs, dim=3, data=(rest2,))

    elements is range-checked and converted to int32 here, and copied, validated (0 <= index < N, pairwise distinct within an
    element) and turned into the incidence list on the device at every minimise.  Each data[k] has n, N or E elements.
    Otherwise a GraphObjective's interface; usable wherever one is, refused where one is."""
    _NAME = "MeshObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_mesh", "lbfgsx_objective_source_mesh"

    def __init__(self, elem_body, elements, dim, node_body=None, data=(), scalars=()):
        a = elements
        if _is_torch(a):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("MeshObjective: elements must be an (E, K) integer array, not one of shape %r" % (a.shape,))
        if a.dtype.kind not in "iu":
            raise ValueError("MeshObjective: elements must be an (E, K) integer array, not one of dtype %s" % a.dtype)
        if a.shape[1] not in (2, 3, 4):
            raise ValueError("MeshObjective: K = %d is not supported: an element has K = 2, 3 or 4 nodes" % a.shape[1])
        if a.shape[0] < 1:
            raise ValueError("MeshObjective: E = 0: a mesh objective has at least one element")
        for v in (int(a.min()), int(a.max())):
            if v < -2 ** 31 or v > 2 ** 31 - 1:
                raise ValueError("MeshObjective: elements holds %d, which does not fit a 32-bit node index" % v)
        if a.shape[0] > 2 ** 30 - 1:
            raise ValueError("MeshObjective: E = %d exceeds 2^30 - 1" % a.shape[0])
        if dim not in (1, 2, 3):
            raise ValueError("MeshObjective: dim = %r is not supported: a node has D = 1, 2 or 3 unknowns" % (dim,))
        self.elements = np.ascontiguousarray(a, np.int32)
        self.E, self.K, self.D = int(a.shape[0]), int(a.shape[1]), int(dim)
        self.body = str(elem_body)
        self.node_body = None if not node_body else str(node_body)
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    def _form_args(self):
        return (self.K, self.D, self.node_body.encode() if self.node_body else None)

    def _check_n(self, n):
        if n % self.D:
            raise ValueError("MeshObjective: n = %d is not a multiple of D = %d: x holds D unknowns per node" % (n, self.D))
        if n > 2 ** 31 - 1:
            raise ValueError("MeshObjective: n = %d exceeds 2^31 - 1: node indices are int32" % n)

    def _data_sizes(self, n):
        return (n, n // self.D, self.E)


class LinearObjective(TermObjective):
    """A linear model fitted to data: x are the n weights, row r of the sparse R x n matrix A is one sample, and
    f(x) = sum over coordinates j of psi(x[j]; j) + sum over rows r of phi(z_r; r) with z = A x -- logistic regression, least
    squares, non-negative least squares under LBFGSBSolver, Poisson and Huber regression, L2-loss SVMs (include/lbfgsx.h,
    "linear-model objectives").  row_body sees T, const T z, T& dz (to assign: phi'(z)), int64_t r, p0..p3 and c[8] and returns
    phi(z); coord_body (optional) is a GraphObjective's node body: T, const T x[1], T g[1], int64_t i, p0..p3, c[8], returns
    psi.  grad[j] is the coordinate term's g[0], then val * phi'(z_r) over the entries of column j in ascending r.

        svm = LinearObjective("const T m = T(1) - p0[r] * z; const T h = m > T(0) ? m : T(0);"
                              "dz = T(-2) * (p0[r] * h); return h * h;", (rowptr, col, val), n, data=(labels,), scalars=(1e-3,),
                              coord_body="g[0] = c[0] * x[0]; return T(0.5) * (c[0] * (x[0] * x[0]));")

    The matrix is CSR: rowptr (R+1), col (nnz) and val (nnz), three numpy arrays (range-checked and converted to int32 and
    the solver's dtype on the host) or three torch tensors on the solver's device (int32, int32 and the solver's dtype: used
    from device memory).  They are copied, validated (rowptr starts at 0, does not decrease, ends at nnz; 0 <= col < n) and
    transposed on the device at every minimise.  lanes: the lanes that share a row in the row pass, 0 = by the library's rule,
    otherwise a power of two <= 64.  Each data[k] has n (per weight) or R (per sample) elements.  Otherwise a
    GraphObjective's interface; usable wherever one is, refused where one is."""
    _NAME = "LinearObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_linear", "lbfgsx_objective_source_linear"

    def __init__(self, row_body, matrix, n, coord_body=None, data=(), scalars=(), lanes=0):
        try:
            rowptr, col, val = matrix
        except (TypeError, ValueError):
            raise ValueError("LinearObjective: matrix must be a triple (rowptr, col, val) of CSR arrays") from None
        self.n = int(n)
        if self.n < 1 or self.n > 2 ** 31 - 1:
            raise ValueError("LinearObjective: n = %d: a linear model has 1 .. 2^31 - 1 weights" % self.n)
        if lanes not in (0, 1, 2, 4, 8, 16, 32, 64):
            raise ValueError("LinearObjective: lanes = %r: the lanes that share a row are 0 (by the rule) or a power of two in "
                             "1..64" % (lanes,))
        self.lanes = int(lanes)
        self.on_device = all(_is_torch(a) and a.is_cuda for a in (rowptr, col, val))
        if self.on_device:
            torch = L.require_torch("LinearObjective with a matrix on the device")
            for a, name in ((rowptr, "rowptr"), (col, "col")):
                if a.dim() != 1 or a.dtype != torch.int32 or not a.is_contiguous():
                    raise ValueError("LinearObjective: %s on the device must be a contiguous 1-D int32 tensor" % name)
            if val.dim() != 1 or val.dtype not in (torch.float32, torch.float64) or not val.is_contiguous():
                raise ValueError("LinearObjective: val on the device must be a contiguous 1-D float32 or float64 tensor")
            self.rowptr, self.col, self.val = rowptr, col, val
            sizes = (int(rowptr.numel()), int(col.numel()), int(val.numel()))
        else:
            self.rowptr, self.col = self._indices(rowptr, "rowptr"), self._indices(col, "col")
            v = val.detach().cpu().numpy() if _is_torch(val) else np.asarray(val)
            if v.ndim != 1 or v.dtype.kind not in "fiu":
                raise ValueError("LinearObjective: val must be a 1-D array of numbers, not %s with %d dimensions" % (v.dtype, v.ndim))
            self.val = np.ascontiguousarray(v, np.float64 if v.dtype != np.float32 else np.float32)
            sizes = (self.rowptr.size, self.col.size, self.val.size)
        self.R, self.nnz = sizes[0] - 1, sizes[1]
        if self.R < 1:
            raise ValueError("LinearObjective: rowptr has %d elements: a matrix has at least one row (R + 1 >= 2)" % sizes[0])
        if self.nnz < 1:
            raise ValueError("LinearObjective: nnz = 0: a matrix has at least one entry")
        if sizes[2] != self.nnz:
            raise ValueError("LinearObjective: col has %d elements and val has %d: one pair per entry" % (self.nnz, sizes[2]))
        if not self.on_device:
            if int(self.rowptr[0]) != 0 or int(self.rowptr[-1]) != self.nnz:
                raise ValueError("LinearObjective: rowptr[0] = %d and rowptr[R] = %d: rowptr starts at 0 and ends at nnz = %d"
                                 % (int(self.rowptr[0]), int(self.rowptr[-1]), self.nnz))
        self.body, self.K = str(row_body), 1
        self.coord_body = None if not coord_body else str(coord_body)
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    @staticmethod
    def _indices(a, name):
        if _is_torch(a):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
            raise ValueError("LinearObjective: %s must be a 1-D integer array, not %s with %d dimensions" % (name, a.dtype, a.ndim))
        if a.size:
            for v in (int(a.min()), int(a.max())):
                if v < -2 ** 31 or v > 2 ** 31 - 1:
                    raise ValueError("LinearObjective: %s holds %d, which does not fit 32 bits" % (name, v))
        return np.ascontiguousarray(a, np.int32)

    def _form_args(self):
        return (self.coord_body.encode() if self.coord_body else None,)

    def _check_n(self, n):
        if n != self.n:
            raise ValueError("LinearObjective: the matrix has n = %d columns and x has %d elements" % (self.n, n))

    def _data_sizes(self, n):
        return (n, self.R)

    def _matrix_args(self, solver):
        """(rowptr, col, val as addresses, on_device, what to keep alive) for a solver of the given dtype and device"""
        np_dt = _NP[solver.dtype]
        if self.on_device:
            torch = L.require_torch("LinearObjective with a matrix on the device")
            want = torch.float64 if solver.dtype == L.F64 else torch.float32
            val = self.val if self.val.dtype == want else self.val.to(want)
            for a in (self.rowptr, self.col, val):
                if a.device.index != solver.device:
                    raise ValueError("LinearObjective: the matrix must be on cuda:%d" % solver.device)
            torch.cuda.current_stream().synchronize()  # the arrays are complete when the library reads them
            return self.rowptr.data_ptr(), self.col.data_ptr(), val.data_ptr(), 1, (val,)
        val = np.ascontiguousarray(self.val, np_dt)
        return self.rowptr.ctypes.data, self.col.ctypes.data, val.ctypes.data, 0, (val,)


class GraphLinearObjective(LinearObjective):
    """A linear model with a coupling term over a graph on its weights: x are the n weights, A is a sparse R x n CSR matrix,
    the E edges are (ei[e], ej[e]), and
    f(x) = sum over coordinates j of psi(x[j]; j) + sum over edges e of rho(x[ei[e]], x[ej[e]]; e) + sum over rows r of
    phi(z_r; r) with z = A x -- tomographic and deblurring reconstruction with a smoothness or smoothed-TV prior under
    non-negativity (LBFGSBSolver), Poisson or logistic regression with a GMRF / ICAR prior on a latent field, Laplacian-
    regularised least squares, fused and graph-trend regression (include/lbfgsx.h, "graph-regularised linear-model
    objectives").  row_body and coord_body are a LinearObjective's, edge_body is a GraphObjective's (T, const T x[2], T g[2],
    int64_t e, i, j); the three share p0..p3 and c[8].  grad[j] is the coordinate term's g[0], then the g_e[side] of the edges
    incident to j in ascending e, then val * phi'(z_r) over the entries of column j in ascending r.

        smooth = GraphLinearObjective("const T u = z - p0[r]; dz = u; return T(0.5) * (u * u);", (rowptr, col, val), (ei, ej),
                                      "const T d = x[0] - x[1]; const T w = c[0] * d; g[0] = w; g[1] = T(0) - w;"
                                      "return T(0.5) * (w * d);", n=n, data=(b,), scalars=(lam,))

    matrix as for a LinearObjective, edges as for a GraphObjective (E >= 1, so n >= 2); both are copied, validated and turned
    into the transposed matrix and the incidence list on the device at every minimise.  Each data[k] has n, E or R elements.
    Otherwise a LinearObjective's interface; usable wherever one is, refused where one is."""
    _NAME = "GraphLinearObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_linear_graph", "lbfgsx_objective_source_linear_graph"

    def __init__(self, row_body, matrix, edges, edge_body, n, coord_body=None, lanes=0, data=(), scalars=()):
        try:
            ei, ej = edges
        except (TypeError, ValueError):
            raise ValueError("GraphLinearObjective: edges must be a pair (ei, ej) of integer arrays") from None
        # the matrix and the index arrays are checked as the two parent forms check them, in their words
        self.ei, self.ej = GraphObjective._indices(ei, "ei"), GraphObjective._indices(ej, "ej")
        super().__init__(row_body, matrix, n, coord_body, data, scalars, lanes)
        if self.ei.size != self.ej.size:
            raise ValueError("GraphLinearObjective: ei has %d elements and ej has %d: one pair per edge" % (self.ei.size, self.ej.size))
        if self.ei.size < 1:
            raise ValueError("GraphLinearObjective: E = 0: a graph-regularised linear model has at least one edge")
        self.E = int(self.ei.size)
        if self.n < 2:
            raise ValueError("GraphLinearObjective: n = %d: an edge joins two different coordinates (n >= 2)" % self.n)
        self.edge_body = str(edge_body)

    def _form_args(self):
        return (self.coord_body.encode() if self.coord_body else None, self.edge_body.encode())

    def _data_sizes(self, n):
        return (n, self.E, self.R)


class MultiLinearObjective(LinearObjective):
    """A linear model with D = outputs values per sample: x holds an F x D weight matrix, feature-major (x[j*D + c],
    n = features * outputs), A is a sparse R x F CSR matrix, Z = A X, and
    f(x) = sum over coordinates i of psi(x[i]; i) + sum over rows r of phi(Z[r, 0..D); r) -- multinomial (softmax) logistic
    regression, multi-class SVMs, multi-target least squares, non-negative matrix regression under LBFGSBSolver
    (include/lbfgsx.h, "multi-output linear-model objectives").  row_body sees T, constexpr int D, const T z[D], T dz[D] (to
    fill with dphi/dz_c), int64_t r, p0..p3 and c[8] and returns phi; coord_body (optional) is a LinearObjective's, per
    coordinate i = j*D + c (D is visible).  grad[j*D + c] is the coordinate term's g[0], then val * dz_r[c] over the entries of
    column j in ascending r.

        lsq = MultiLinearObjective("T s = T(0);\n#pragma unroll\nfor (int c = 0; c < D; c++) {"
                                   " dz[c] = z[c] - p0[r * D + c]; s = s + dz[c] * dz[c]; } return T(0.5) * s;",
                                   (rowptr, col, val), features=F, outputs=3, data=(targets.ravel(),))

    1 <= outputs <= 16.  The matrix is a LinearObjective's with 0 <= col < features.  Each data[k] has n, features, R or
    R * D elements (an R x D table of targets, p0[r * D + c]).  Otherwise a
    LinearObjective's interface; usable wherever one is, refused where one is."""
    _NAME = "MultiLinearObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_linear_multi", "lbfgsx_objective_source_linear_multi"

    def __init__(self, row_body, matrix, features, outputs, coord_body=None, data=(), scalars=(), lanes=0):
        self.D, self.F = int(outputs), int(features)
        if self.D < 1 or self.D > 16:
            raise ValueError("MultiLinearObjective: D = %d is not supported: a row has D = 1 .. 16 outputs" % self.D)
        if self.F < 1:
            raise ValueError("MultiLinearObjective: features = %d: a model has at least one feature" % self.F)
        super().__init__(row_body, matrix, self.F * self.D, coord_body, data, scalars, lanes)

    def _form_args(self):
        return (self.D, self.coord_body.encode() if self.coord_body else None)

    def _check_n(self, n):
        if n % self.D:
            raise ValueError("MultiLinearObjective: n = %d is not a multiple of D = %d: x holds the D weights of each feature"
                             % (n, self.D))
        if n != self.n:
            raise ValueError("MultiLinearObjective: the model has n = %d * %d = %d weights and x has %d elements"
                             % (self.F, self.D, self.n, n))

    def _data_sizes(self, n):
        return (n, self.F, self.R, self.R * self.D)


class DenseLinearObjective(TermObjective):
    """The multi-output linear model over a DENSE matrix: x holds an F x D weight matrix, feature-major (x[j*D + c],
    n = F * outputs), A is a dense R x F matrix, Z = A X, and
    f(x) = sum over coordinates i of psi(x[i]; i) + sum over rows r of phi(Z[r, 0..D); r) -- logistic, softmax, Poisson and
    least-squares regression on tabular features, non-negative least squares under LBFGSBSolver (include/lbfgsx.h, "dense
    linear-model objectives").  The bodies are a MultiLinearObjective's: row_body sees T, constexpr int D, const T z[D],
    T dz[D] (to fill), int64_t r, p0..p3 and c[8] and returns phi (outputs = 1: z[0] and dz[0]); coord_body (optional) sees
    const T x[1], T g[1], int64_t i.

        logit = DenseLinearObjective("const T m = p0[r] * z[0]; const T e = exp(T(0) - m);"
                                     "dz[0] = T(0) - p0[r] * (e / (T(1) + e)); return log(T(1) + e);",
                                     A, data=(labels,), scalars=(1e-3,),
                                     coord_body="g[0] = c[0] * x[0]; return T(0.5) * (c[0] * (x[0] * x[0]));")

    matrix: a 2-D numpy array (converted to the solver's dtype and copied to the device at every minimise), or a 2-D torch
    tensor on the solver's device with unit column stride, of the solver's dtype, which is used IN PLACE with lda = its row
    stride: it is not copied, and stays alive and unchanged while a minimise runs.  1 <= outputs <= 16.  lanes: the lanes that
    share a row in the row pass, 0 = by the library's rule, otherwise a power of two <= 64.  Each data[k] has n, F, R or R * D
    elements.  Otherwise a MultiLinearObjective's interface; usable wherever one is, refused where one is."""
    _NAME = "DenseLinearObjective"
    _COMPILE, _SOURCE = "lbfgsx_objective_compile_dense", "lbfgsx_objective_source_dense"

    def __init__(self, row_body, matrix, outputs=1, coord_body=None, data=(), scalars=(), lanes=0):
        self.D = int(outputs)
        if self.D < 1 or self.D > 16:
            raise ValueError("DenseLinearObjective: D = %d is not supported: a row has D = 1 .. 16 outputs" % self.D)
        if lanes not in (0, 1, 2, 4, 8, 16, 32, 64):
            raise ValueError("DenseLinearObjective: lanes = %r: the lanes that share a row are 0 (by the rule) or a power of two "
                             "in 1..64" % (lanes,))
        self.lanes = int(lanes)
        self.on_device = _is_torch(matrix) and matrix.is_cuda
        if self.on_device:
            torch = L.require_torch("DenseLinearObjective with a matrix on the device")
            if matrix.dim() != 2:
                raise ValueError("DenseLinearObjective: matrix on the device must be a 2-D tensor, not one of %d dimensions"
                                 % matrix.dim())
            if matrix.dtype not in (torch.float32, torch.float64):
                raise ValueError("DenseLinearObjective: matrix on the device has dtype %s: it must be float32 or float64, the "
                                 "solver's" % matrix.dtype)
            if matrix.shape[0] >= 1 and matrix.shape[1] >= 1 and (
                    (matrix.shape[1] > 1 and matrix.stride(1) != 1) or (matrix.shape[0] > 1 and matrix.stride(0) < matrix.shape[1])):
                raise ValueError("DenseLinearObjective: matrix on the device has strides (%d, %d): it must be row-major with unit "
                                 "column stride and a row stride >= its %d columns" % (matrix.stride(0), matrix.stride(1),
                                                                                     matrix.shape[1]))
            self.matrix = matrix
            self.lda = int(matrix.stride(0)) if matrix.shape[0] > 1 else int(matrix.shape[1])
        else:
            a = matrix.detach().cpu().numpy() if _is_torch(matrix) else np.asarray(matrix)
            if a.ndim != 2 or a.dtype.kind not in "fiu":
                raise ValueError("DenseLinearObjective: matrix must be a 2-D array of numbers, not %s with %d dimensions"
                                 % (a.dtype, a.ndim))
            self.matrix = np.ascontiguousarray(a, np.float64 if a.dtype != np.float32 else np.float32)
            self.lda = int(a.shape[1])
        self.R, self.F = int(self.matrix.shape[0]), int(self.matrix.shape[1])
        if self.R < 1 or self.F < 1:
            raise ValueError("DenseLinearObjective: matrix has shape (%d, %d): a model has at least one row and one feature"
                             % (self.R, self.F))
        self.n = self.F * self.D
        self.body, self.K = str(row_body), 1
        self.coord_body = None if not coord_body else str(coord_body)
        self._h = {}
        self.set_data(*data)
        self.set_scalars(*scalars)

    def _form_args(self):
        return (self.D, self.coord_body.encode() if self.coord_body else None)

    def _check_n(self, n):
        if n % self.D:
            raise ValueError("DenseLinearObjective: n = %d is not a multiple of D = %d: x holds the D weights of each feature"
                             % (n, self.D))
        if n != self.n:
            raise ValueError("DenseLinearObjective: the model has n = %d * %d = %d weights and x has %d elements"
                             % (self.F, self.D, self.n, n))

    def _data_sizes(self, n):
        return (n, self.F, self.R, self.R * self.D)

    def _matrix_args(self, solver):
        """(A as an address, lda, on_device, what to keep alive) for a solver of the given dtype and device"""
        if self.on_device:
            torch = L.require_torch("DenseLinearObjective with a matrix on the device")
            want = torch.float64 if solver.dtype == L.F64 else torch.float32
            if self.matrix.dtype != want:
                raise ValueError("DenseLinearObjective: matrix on the device has dtype %s and the solver %s: a device matrix is "
                                 "used in place, not converted" % (self.matrix.dtype, want))
            if self.matrix.device.index != solver.device:
                raise ValueError("DenseLinearObjective: the matrix must be on cuda:%d" % solver.device)
            torch.cuda.current_stream().synchronize()  # the matrix is complete when the library reads it
            return self.matrix.data_ptr(), self.lda, 1, (self.matrix,)
        a = np.ascontiguousarray(self.matrix, _NP[solver.dtype])
        return a.ctypes.data, self.lda, 0, (a,)


class TraceBuffer:
    """Per-evaluation record (fx and x[::stride]) for the parity tests."""

    def __init__(self, n, cap=512, stride=1, with_x=True):
        self.nsamp = (n + stride - 1) // stride
        self.fx = np.zeros(cap, dtype=np.float64)
        self.xs = np.zeros((cap, self.nsamp), dtype=np.float64) if with_x else None
        pd = C.POINTER(C.c_double)
        self.c = L.Trace(cap=cap, count=0, fx=self.fx.ctypes.data_as(pd), stride=stride, nsamp=self.nsamp,
                         xs=self.xs.ctypes.data_as(pd) if with_x else None)

    @property
    def count(self):
        return self.c.count


class Result:
    def __init__(self, r):
        self.niter, self.nfev, self.fx, self.gnorm = r.niter, r.nfev, r.fx, r.gnorm
        self.status, self.msg = r.status, r.msg.decode()


class _SolverBase:
    _algo = L.ALGO_LBFGS

    def __init__(self, param, linesearch=L.LS_NOCEDAL_WRIGHT, dtype=np.float64, device=0):
        self._core, self._sol = L.load()
        self.dtype = L.F64 if np.dtype(dtype) == np.float64 else L.F32
        self.device = int(device)
        self.param = param
        self._h = C.c_void_p()
        cp = param._c()
        rc = self._sol.lbfgsx_solver_create(C.byref(self._h), self._algo, self.dtype, linesearch, C.byref(cp), device)
        L.check(rc, self._sol.lbfgsx_solver_create_error().decode())
        self.last = None

    def __del__(self):
        try:
            if self._h:
                self._sol.lbfgsx_solver_destroy(self._h)
                self._h = None
        except Exception:
            pass

    close = __del__

    def prepare(self, n):
        """Allocate the device state for dimension n; returns the low-level context handle."""
        rc = self._sol.lbfgsx_solver_prepare(self._h, n)
        L.check(rc)
        return C.c_void_p(self._sol.lbfgsx_solver_ctx(self._h))

    def set_iteration_hook(self, fn):
        """fn(k) is called on the host after iteration k produced the next search direction (None to clear)."""
        self._hook = L.ITER_HOOK((lambda k, _u: fn(k)) if fn else 0)
        L.check(self._sol.lbfgsx_solver_set_iteration_hook(self._h, self._hook, None))

    def set_recursion(self, form):
        """Extension: L.RECURSION_VECTOR (bit-parity two-loop, default) or L.RECURSION_GRAM_SPACE (coefficient-space
        recursion over [S, Y, g]: about half the HBM traffic, equal to the vector form only up to rounding)."""
        L.check(self._sol.lbfgsx_solver_set_recursion(self._h, int(form)), "set_recursion: unknown form, or not an L-BFGS solver")

    def set_direction_scale(self, a):
        """Extension, for tests of the line searches' entry check: the directions computed from now on are a * H * grad
        (-1 is the method, +1 an ascent direction)."""
        L.check(self._sol.lbfgsx_solver_set_direction_scale(self._h, float(a)), "set_direction_scale: not an L-BFGS solver")

    def set_reducer(self, fn):
        """Extension, row-sharded runs: fn(values) receives a float64 numpy view of a small array and must replace it by
        its sum over all ranks (an all-reduce).  None switches back.  Gram-space recursion only."""
        if fn is None:
            self._red = L.ALLREDUCE(0)
        else:
            def cb(ptr, count, _user):
                fn(np.ctypeslib.as_array(ptr, shape=(count,)))
            self._red = L.ALLREDUCE(cb)
        L.check(self._sol.lbfgsx_solver_set_allreduce(self._h, self._red, None), "set_reducer: not an L-BFGS solver")

    def set_devices(self, devices):
        """Extension: minimize(f, x) row-shards the ONE problem over these GPUs of the node from this process (one host
        thread + context per device; the driver's sums cross the devices through the library's RCCL all-reduce).
        [] switches back."""
        devs = [int(d) for d in (devices or [])]
        arr = (C.c_int * max(len(devs), 1))(*devs)
        L.check(self._sol.lbfgsx_solver_set_devices(self._h, arr, len(devs)), "set_devices: not an L-BFGS solver")

    def set_native_reducer(self, comm, local_rank=0):
        """Extension, row-sharded runs: the reducer is the library's own all-reduce over `comm` (lbfgsx_comm_create_*),
        called from C without passing through Python."""
        core, _ = L.load()
        hook = C.cast(core.lbfgsx_comm_allreduce_hook, L.ALLREDUCE)
        L.check(self._sol.lbfgsx_solver_set_allreduce(self._h, hook, C.c_void_p(core.lbfgsx_comm_hook_arg(comm, local_rank))),
                "set_reducer: not an L-BFGS solver")

    @property
    def ctx(self):
        return C.c_void_p(self._sol.lbfgsx_solver_ctx(self._h))

    def _ptr(self, arr):
        if arr is None:
            return None
        assert arr.dtype == _NP[self.dtype] and arr.flags["C_CONTIGUOUS"]
        return arr.ctypes.data_as(C.c_void_p)

    def _vec(self, which, n):
        """torch view of a named device vector of the prepared state (valid until the next call into the solver)"""
        return L.device_tensor(self._core.lbfgsx_vec(self.ctx, which), (n,), _NP[self.dtype], self.device)

    def _minimize_device(self, f, x, bounds, trace):
        """x (and bounds) as torch tensors on the solver's device: placed in the resident state, solved there, x updated in
        place.  When minimize raises, x keeps its start point."""
        torch = L.require_torch("minimize with a torch x")
        n = x.numel()
        want = torch.float64 if self.dtype == L.F64 else torch.float32
        if x.dim() != 1 or x.dtype != want or not x.is_cuda or x.device.index != self.device:
            raise ValueError("x must be a 1-D %s tensor on cuda:%d" % (want, self.device))
        self.prepare(n)
        with torch.cuda.device(self.device):
            self._vec(L.VEC_X, n).copy_(x)
            for which, v in bounds:
                v = torch.as_tensor(v, dtype=want)
                if v.numel() != n:
                    raise ValueError("'lb' and 'ub' must have the same size as 'x'")
                self._vec(which, n).copy_(v.reshape(n))
            torch.cuda.current_stream().synchronize()
            r = self._minimize(f, n, None, None, None, trace)
            x.copy_(self._vec(L.VEC_X, n))
            torch.cuda.current_stream().synchronize()
        return r.niter, r.fx

    def _minimize_fn(self, f, n, x, lb, ub, trace):
        torch = L.require_torch("DeviceObjective")
        raised = []

        def cb(_user, xp, gp, nn, fxp):
            try:
                with torch.cuda.device(self.device):
                    xt = L.device_tensor(xp, (nn,), _NP[self.dtype], self.device)
                    gt = L.device_tensor(gp, (nn,), _NP[self.dtype], self.device)
                    fxp[0] = float(f.fn(xt, gt))
                    torch.cuda.current_stream().synchronize()  # grad is complete when the library reads it
                return 0
            except BaseException as e:  # re-raised below, after the C call has unwound
                raised.append(e)
                return 1

        res = L.Result()
        rc = self._sol.lbfgsx_solver_minimize_fn(self._h, n, L.OBJECTIVE_FN(cb), None, self._ptr(x), self._ptr(lb),
                                                 self._ptr(ub), C.byref(trace.c) if trace else None, C.byref(res))
        self.last = Result(res)
        if raised:
            raise raised[0]
        L.check(rc, self.last.msg)
        return self.last

    def _minimize_obj(self, f, n, x, lb, ub, trace):
        np_dt = _NP[self.dtype]
        f._check_n(n)
        h = f.compile(np_dt)
        ptrs = (C.c_void_p * 4)()
        counts = (C.c_int64 * 4)()
        sizes = f._data_sizes(n)
        what = " or ".join("%d" % v for v in sizes)
        keep, mask = [], 0
        for k, d in enumerate(f.data):
            if d is None:
                continue
            if _is_torch(d):
                torch = L.require_torch("%s with torch data" % f._NAME)
                want = torch.float64 if self.dtype == L.F64 else torch.float32
                if d.dim() != 1 or d.numel() not in sizes or d.dtype != want or not d.is_cuda or d.device.index != self.device \
                        or not d.is_contiguous():
                    raise ValueError("%s: data[%d] must be a contiguous 1-D %s tensor of %s elements on cuda:%d"
                                     % (f._NAME, k, want, what, self.device))
                ptrs[k] = d.data_ptr()
                keep.append(d)
            else:
                a = np.ascontiguousarray(d, np_dt)
                if a.ndim != 1 or a.size not in sizes:
                    raise ValueError("%s: data[%d] must have %s elements" % (f._NAME, k, what))
                ptrs[k] = a.ctypes.data
                counts[k] = a.size
                mask |= 1 << k
                keep.append(a)  # the converted copy, not d: its address is what the library reads
        cs = (C.c_double * 8)(*(f.scalars + (0.0,) * (8 - len(f.scalars))))
        res = L.Result()
        if any(_is_torch(d) for d in f.data):
            torch.cuda.current_stream().synchronize()  # the data arrays are complete when the library reads them
        tail = (C.byref(ptrs), mask, C.byref(cs), self._ptr(x), self._ptr(lb), self._ptr(ub), C.byref(trace.c) if trace else None,
                C.byref(res))
        if isinstance(f, GraphLinearObjective):
            rp, cp, vp, on_dev, keep_m = f._matrix_args(self)
            rc = self._sol.lbfgsx_solver_minimize_linear_graph(self._h, h, n, f.R, f.nnz, rp, cp, vp, on_dev, f.lanes, f.E,
                                                               f.ei.ctypes.data, f.ej.ctypes.data, 0, tail[0], mask,
                                                               C.byref(counts), *tail[2:])
            del keep_m
        elif isinstance(f, DenseLinearObjective):
            ap, lda, on_dev, keep_m = f._matrix_args(self)
            rc = self._sol.lbfgsx_solver_minimize_dense(self._h, h, n, f.R, ap, lda, on_dev, f.lanes, tail[0], mask,
                                                        C.byref(counts), *tail[2:])
            del keep_m
        elif isinstance(f, LinearObjective):
            rp, cp, vp, on_dev, keep_m = f._matrix_args(self)
            rc = self._sol.lbfgsx_solver_minimize_linear(self._h, h, n, f.R, f.nnz, rp, cp, vp, on_dev, f.lanes, tail[0], mask,
                                                         C.byref(counts), *tail[2:])
            del keep_m
        elif isinstance(f, MeshObjective):
            rc = self._sol.lbfgsx_solver_minimize_mesh(self._h, h, n, f.E, f.elements.ctypes.data_as(C.POINTER(C.c_int32)), 0,
                                                       tail[0], mask, C.byref(counts), *tail[2:])
        elif isinstance(f, GraphObjective):
            rc = self._sol.lbfgsx_solver_minimize_graph(self._h, h, n, f.E, f.ei.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        f.ej.ctypes.data_as(C.POINTER(C.c_int32)), 0, tail[0], mask,
                                                        C.byref(counts), *tail[2:])
        elif isinstance(f, _LatticeObjective):
            rc = getattr(self._sol, f._ENTRY)(self._h, h, *f._entry_args(), *tail)
        else:
            rc = self._sol.lbfgsx_solver_minimize_obj(self._h, h, n, *tail)
        del keep
        self.last = Result(res)
        L.check(rc, self.last.msg)
        return self.last

    def bound_data(self):
        """The four device pointers of the term objective bound to this solver's context (0 = unused)."""
        arr = (C.c_void_p * 4)()
        L.check(self._core.lbfgsx_objective_bound(self.ctx, C.byref(arr)))
        return [int(v or 0) for v in arr]

    def _minimize(self, f, n, x, lb, ub, trace):
        if isinstance(f, DeviceObjective):
            return self._minimize_fn(f, n, x, lb, ub, trace)
        if isinstance(f, TermObjective):
            return self._minimize_obj(f, n, x, lb, ub, trace)
        if not hasattr(f, "objective"):
            raise TypeError("f must be DiagQuadratic, ExtendedRosenbrock, TermObjective(body), ChainObjective(body), "
                            "GridObjective(body, shape), VolumeObjective(body, shape), PeriodicGridObjective(body, shape, periodic), "
                            "PeriodicVolumeObjective(body, shape, periodic), GridFieldObjective(body, shape, D, periodic), StencilObjective(body, shape, periodic), GraphObjective(edge_body, edges), MeshObjective(elem_body, elements, dim), "
                            "LinearObjective(row_body, matrix, n), GraphLinearObjective(row_body, matrix, edges, edge_body, n), "
                            "MultiLinearObjective(row_body, matrix, features, outputs), "
                            "DenseLinearObjective(row_body, matrix, outputs) or DeviceObjective(fn)")
        res = L.Result()
        a = None if f.a is None else np.ascontiguousarray(f.a, _NP[self.dtype])
        b = None if f.b is None else np.ascontiguousarray(f.b, _NP[self.dtype])
        rc = self._sol.lbfgsx_solver_minimize(self._h, f.objective, n, self._ptr(a), self._ptr(b), self._ptr(x),
                                              self._ptr(lb), self._ptr(ub), C.byref(trace.c) if trace else None,
                                              C.byref(res))
        self.last = Result(res)
        L.check(rc, self.last.msg)
        return self.last


class LBFGSSolver(_SolverBase):
    """LBFGSSolver<Scalar, LineSearch> (reference LBFGS.h:20-23)."""
    _algo = L.ALGO_LBFGS

    def minimize(self, f, x, trace=None):
        """x: numpy vector, or a torch tensor on the solver's device, updated in place.  Returns (niter, fx) like
        minimize(f, x, fx)."""
        if _is_torch(x):
            return self._minimize_device(f, x, (), trace)
        xx = np.ascontiguousarray(x, _NP[self.dtype])
        r = self._minimize(f, xx.size, xx, None, None, trace)
        if xx is not x:
            x[...] = xx
        return r.niter, r.fx

    def minimize_resident(self, f, n, trace=None):
        """Start point already in LBFGSX_VEC_X of the device state (see prepare()); result stays there."""
        r = self._minimize(f, n, None, None, None, trace)
        return r.niter, r.fx

    def final_grad_norm(self):
        return self.last.gnorm

    def final_approx_hessians(self, n):
        """(final_approx_hessian(), final_approx_inverse_hessian()) as dense n x n arrays (small n only)."""
        B = np.zeros((n, n), order="F")
        H = np.zeros((n, n), order="F")
        L.check(self._sol.lbfgsx_solver_hessians(self._h, B.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)))
        return B, H


class LBFGSBSolver(_SolverBase):
    """LBFGSBSolver<Scalar> with LineSearchMoreThuente (reference LBFGSB.h:21-23)."""
    _algo = L.ALGO_LBFGSB

    def __init__(self, param, dtype=np.float64, device=0):
        super().__init__(param, linesearch=L.LS_MORE_THUENTE, dtype=dtype, device=device)

    def minimize(self, f, x, lb, ub, trace=None):
        """minimize(f, x, fx, lb, ub): x updated in place; raises ValueError when lb/ub sizes differ from x."""
        dt = _NP[self.dtype]
        if _is_torch(x):
            return self._minimize_device(f, x, ((L.VEC_LB, lb), (L.VEC_UB, ub)), trace)
        xx = np.ascontiguousarray(x, dt)
        lbv, ubv = np.ascontiguousarray(lb, dt), np.ascontiguousarray(ub, dt)
        if lbv.size != xx.size or ubv.size != xx.size:
            raise ValueError("'lb' and 'ub' must have the same size as 'x'")
        r = self._minimize(f, xx.size, xx, lbv, ubv, trace)
        if xx is not x:
            x[...] = xx
        return r.niter, r.fx

    def minimize_resident(self, f, n, trace=None):
        """x0, lb, ub already in VEC_X / VEC_LB / VEC_UB of the device state (see prepare())."""
        r = self._minimize(f, n, None, None, None, trace)
        return r.niter, r.fx

    def final_grad_norm(self):
        return self.last.gnorm

    def stats(self):
        arr = (C.c_longlong * 8)()
        L.check(self._sol.lbfgsx_solver_stats(self._h, C.byref(arr)))
        keys = ("gcp_crossings", "submin_sweeps", "submin_calls", "submin_unconverged", "resets", "gcp_build_us",
                "gcp_fetch_us", "gcp_total_us")
        d = dict(zip(keys, list(arr)))
        arr2 = (C.c_longlong * 8)()
        L.check(self._sol.lbfgsx_solver_stats2(self._h, C.byref(arr2)))
        d.update(zip(("gcp_dev_crossings", "gcp_sort_fallbacks", "gcp_partial_sorts", "submin_us", "linesearch_us",
                      "correction_us", "submin_fused_sweeps", "gram_carried"), list(arr2)[:8]))
        arr3 = (C.c_longlong * 8)()
        L.check(self._sol.lbfgsx_solver_stats3(self._h, C.byref(arr3)))
        d.update(zip(("gcp_searches", "gcp_nord", "gcp_sorted", "rhs_identities"), list(arr3)[:4]))
        return d
