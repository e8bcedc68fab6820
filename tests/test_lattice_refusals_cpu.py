"""CPU suite: what the six objective forms on a regular array (grid, volume, periodic grid, periodic volume, grid field, grid
stencil) refuse, and in which words.  One table, the complete message of every refusal written out: the entry points of the
solver library (lbfgsx_solver_minimize_*: no device needed), those of the core library (lbfgsx_objective_bind_*: on a context,
so on a device) and the Python classes.  The messages are part of the interface; this file is what keeps them from drifting
between the forms."""
import ctypes as C

import numpy as np
import pytest

GRID_EXTENT = "a grid has at least 2 rows and 2 columns (rows >= 2, cols >= 2)"
VOLUME_EXTENT = "a volume has at least 2 slabs, 2 rows and 2 columns (slabs >= 2, rows >= 2, cols >= 2)"
STENCIL_EXTENT = "a 3x3 patch needs at least 3 rows and 3 columns (rows >= 3, cols >= 3)"
MASK2 = "the mask has bit 0 for the column direction and bit 1 for the row direction (0 .. 3)"
MASK3 = "the mask has bit 0 for the column, bit 1 for the row and bit 2 for the slab direction (0 .. 7)"
CELL4 = "for (int k = 0; k < 4; k++) g[k] = x[0]; return x[0];"
CELL8 = "for (int k = 0; k < 8; k++) g[k] = x[0]; return x[0];"

# per form: the Python class and what it is built with; `good`, a shape (and mask) of `n` coordinates; the refused shapes with
# the complete message of the solver's entry point and of the bind call (None: that call has no such refusal)
FORMS = [
    dict(key="grid", cls="GridObjective", body=CELL4, kw={}, good=(3, 4), n=12, mask_hi=None, other="volume",
         too_small=[((1, 12), "grid objective: rows = 1, cols = 12: " + GRID_EXTENT),
                    ((12, 1), "grid objective: rows = 12, cols = 1: " + GRID_EXTENT),
                    ((-3, -4), "grid objective: rows = -3, cols = -4: " + GRID_EXTENT)],
         overflow=[((2 ** 40, 2 ** 40), "grid objective: rows = 1099511627776, cols = 1099511627776: rows*cols overflows",
                    "grid objective: rows = 1099511627776, cols = 1099511627776 does not multiply to n = 12")],
         product=((3, 5), "grid objective: rows = 3, cols = 5 does not multiply to n = 12"),
         wrong=("lbfgsx_solver_minimize_grid: the handle is not a grid objective (lbfgsx_objective_compile_grid)",
                "lbfgsx_objective_bind_grid: the handle is a %s, not a grid objective (lbfgsx_objective_compile_grid)"),
         dtype="lbfgsx_solver_minimize_grid: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_grid: invalid argument",
         unshaped=("a grid objective is minimised with its shape: lbfgsx_solver_minimize_grid",
                   "a grid objective is bound with its shape: lbfgsx_objective_bind_grid"),
         py_small=((1, 5), "GridObjective: shape = (1, 5): a grid has at least 2 rows and 2 columns"),
         py_product="GridObjective: shape = (3, 4) does not multiply to n = 13", py_shape=None),
    dict(key="volume", cls="VolumeObjective", body=CELL8, kw={}, good=(2, 3, 4), n=24, mask_hi=None, other="grid_periodic",
         too_small=[((1, 6, 4), "volume objective: slabs = 1, rows = 6, cols = 4: " + VOLUME_EXTENT),
                    ((6, 4, 1), "volume objective: slabs = 6, rows = 4, cols = 1: " + VOLUME_EXTENT),
                    ((-2, -3, -4), "volume objective: slabs = -2, rows = -3, cols = -4: " + VOLUME_EXTENT)],
         overflow=[((2 ** 30, 2 ** 30, 2 ** 30),
                    "volume objective: slabs = 1073741824, rows = 1073741824, cols = 1073741824: slabs*rows*cols overflows",
                    "volume objective: slabs = 1073741824, rows = 1073741824, cols = 1073741824 does not multiply to n = 24"),
                   ((2, 2 ** 40, 2 ** 40),
                    "volume objective: slabs = 2, rows = 1099511627776, cols = 1099511627776: slabs*rows*cols overflows",
                    "volume objective: slabs = 2, rows = 1099511627776, cols = 1099511627776 does not multiply to n = 24")],
         product=((2, 3, 5), "volume objective: slabs = 2, rows = 3, cols = 5 does not multiply to n = 24"),
         wrong=("lbfgsx_solver_minimize_volume: the handle is not a volume objective (lbfgsx_objective_compile_volume)",
                "lbfgsx_objective_bind_volume: the handle is a %s, not a volume objective (lbfgsx_objective_compile_volume)"),
         dtype="lbfgsx_solver_minimize_volume: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_volume: invalid argument",
         unshaped=("a volume objective is minimised with its shape: lbfgsx_solver_minimize_volume",
                   "a volume objective is bound with its shape: lbfgsx_objective_bind_volume"),
         py_small=((2, 1, 5), "VolumeObjective: shape = (2, 1, 5): a volume has at least 2 slabs, 2 rows and 2 columns"),
         py_product="VolumeObjective: shape = (2, 3, 4) does not multiply to n = 25",
         py_shape="VolumeObjective: shape must be (slabs, rows, cols)"),
    dict(key="grid_periodic", cls="PeriodicGridObjective", body=CELL4, kw={}, good=(4, 6), n=24, mask_hi=3, other="volume_periodic",
         too_small=[((1, 24), "periodic grid objective: rows = 1, cols = 24: " + GRID_EXTENT),
                    ((24, 1), "periodic grid objective: rows = 24, cols = 1: " + GRID_EXTENT),
                    ((-4, -6), "periodic grid objective: rows = -4, cols = -6: " + GRID_EXTENT)],
         overflow=[((2 ** 40, 2 ** 40),
                    "periodic grid objective: rows = 1099511627776, cols = 1099511627776: rows*cols overflows",
                    "periodic grid objective: rows = 1099511627776, cols = 1099511627776 does not multiply to n = 24")],
         product=((4, 5), "periodic grid objective: rows = 4, cols = 5 does not multiply to n = 24"),
         mask=[(4, "periodic grid objective: periodic = 4: " + MASK2), (-1, "periodic grid objective: periodic = -1: " + MASK2)],
         wrong=("lbfgsx_solver_minimize_grid_periodic: the handle is not a periodic grid objective "
                "(lbfgsx_objective_compile_grid_periodic)",
                "lbfgsx_objective_bind_grid_periodic: the handle is a %s, not a periodic grid objective "
                "(lbfgsx_objective_compile_grid_periodic)"),
         dtype="lbfgsx_solver_minimize_grid_periodic: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_grid_periodic: invalid argument",
         unshaped=("a periodic grid objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_periodic",
                   "a periodic grid objective is bound with its shape and mask: lbfgsx_objective_bind_grid_periodic"),
         py_small=((5, 1), "PeriodicGridObjective: shape = (5, 1): a grid has at least 2 rows and 2 columns"),
         py_product="PeriodicGridObjective: shape = (4, 6) does not multiply to n = 25",
         py_shape="PeriodicGridObjective: shape must be (rows, cols)"),
    dict(key="volume_periodic", cls="PeriodicVolumeObjective", body=CELL8, kw={}, good=(2, 3, 4), n=24, mask_hi=7, other="grid_field",
         too_small=[((1, 6, 4), "periodic volume objective: slabs = 1, rows = 6, cols = 4: " + VOLUME_EXTENT),
                    ((6, 4, 1), "periodic volume objective: slabs = 6, rows = 4, cols = 1: " + VOLUME_EXTENT),
                    ((-2, -3, -4), "periodic volume objective: slabs = -2, rows = -3, cols = -4: " + VOLUME_EXTENT)],
         overflow=[((2 ** 30, 2 ** 30, 2 ** 30),
                    "periodic volume objective: slabs = 1073741824, rows = 1073741824, cols = 1073741824: slabs*rows*cols overflows",
                    "periodic volume objective: slabs = 1073741824, rows = 1073741824, cols = 1073741824 does not multiply to "
                    "n = 24")],
         product=((2, 3, 5), "periodic volume objective: slabs = 2, rows = 3, cols = 5 does not multiply to n = 24"),
         mask=[(8, "periodic volume objective: periodic = 8: " + MASK3), (-1, "periodic volume objective: periodic = -1: " + MASK3)],
         wrong=("lbfgsx_solver_minimize_volume_periodic: the handle is not a periodic volume objective "
                "(lbfgsx_objective_compile_volume_periodic)",
                "lbfgsx_objective_bind_volume_periodic: the handle is a %s, not a periodic volume objective "
                "(lbfgsx_objective_compile_volume_periodic)"),
         dtype="lbfgsx_solver_minimize_volume_periodic: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_volume_periodic: invalid argument",
         unshaped=("a periodic volume objective is minimised with its shape and mask: lbfgsx_solver_minimize_volume_periodic",
                   "a periodic volume objective is bound with its shape and mask: lbfgsx_objective_bind_volume_periodic"),
         py_small=((2, 3, 0), "PeriodicVolumeObjective: shape = (2, 3, 0): a volume has at least 2 slabs, 2 rows and 2 columns"),
         py_product="PeriodicVolumeObjective: shape = (2, 3, 4) does not multiply to n = 25",
         py_shape="PeriodicVolumeObjective: shape must be (slabs, rows, cols)"),
    dict(key="grid_field", cls="GridFieldObjective", body="for (int k = 0; k < 4 * D; k++) g[k] = x[0]; return x[0];", kw={"D": 2},
         good=(4, 6), n=48, mask_hi=3, other="grid_stencil",
         too_small=[((1, 24), "grid field objective: rows = 1, cols = 24, D = 2: " + GRID_EXTENT),
                    ((24, 1), "grid field objective: rows = 24, cols = 1, D = 2: " + GRID_EXTENT),
                    ((-4, -6), "grid field objective: rows = -4, cols = -6, D = 2: " + GRID_EXTENT)],
         overflow=[((2 ** 40, 2 ** 40),
                    "grid field objective: rows = 1099511627776, cols = 1099511627776, D = 2: rows*cols*D overflows",
                    "grid field objective: rows = 1099511627776, cols = 1099511627776, D = 2 does not multiply to n = 48"),
                   ((2 ** 31, 2 ** 31),  # rows*cols = 2^62 fits, times D = 2 does not
                    "grid field objective: rows = 2147483648, cols = 2147483648, D = 2: rows*cols*D overflows",
                    "grid field objective: rows = 2147483648, cols = 2147483648, D = 2 does not multiply to n = 48")],
         product=((8, 6), "grid field objective: rows = 8, cols = 6, D = 2 does not multiply to n = 48"),
         mask=[(4, "grid field objective: periodic = 4: " + MASK2), (-1, "grid field objective: periodic = -1: " + MASK2)],
         wrong=("lbfgsx_solver_minimize_grid_field: the handle is not a grid field objective (lbfgsx_objective_compile_grid_field)",
                "lbfgsx_objective_bind_grid_field: the handle is a %s, not a grid field objective "
                "(lbfgsx_objective_compile_grid_field)"),
         dtype="lbfgsx_solver_minimize_grid_field: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_grid_field: invalid argument",
         unshaped=("a grid field objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_field",
                   "a grid field objective is bound with its shape, mask and D: lbfgsx_objective_bind_grid_field"),
         py_small=((1, 1), "GridFieldObjective: shape = (1, 1): a grid has at least 2 rows and 2 columns"),
         py_product="GridFieldObjective: shape = (4, 6), D = 2 does not multiply to n = 49",
         py_shape="GridFieldObjective: shape must be (rows, cols)"),
    dict(key="grid_stencil", cls="StencilObjective", body="for (int k = 0; k < 9; k++) g[k] = x[0]; return x[0];", kw={},
         good=(4, 6), n=24, mask_hi=3, other="grid",
         too_small=[((2, 12), "grid stencil objective: rows = 2, cols = 12: " + STENCIL_EXTENT),
                    ((12, 2), "grid stencil objective: rows = 12, cols = 2: " + STENCIL_EXTENT),
                    ((-4, -6), "grid stencil objective: rows = -4, cols = -6: " + STENCIL_EXTENT)],
         overflow=[((2 ** 40, 2 ** 40),
                    "grid stencil objective: rows = 1099511627776, cols = 1099511627776: rows*cols overflows",
                    "grid stencil objective: rows = 1099511627776, cols = 1099511627776 does not multiply to n = 24")],
         product=((4, 5), "grid stencil objective: rows = 4, cols = 5 does not multiply to n = 24"),
         mask=[(4, "grid stencil objective: periodic = 4: " + MASK2), (-1, "grid stencil objective: periodic = -1: " + MASK2)],
         wrong=("lbfgsx_solver_minimize_grid_stencil: the handle is not a grid stencil objective "
                "(lbfgsx_objective_compile_grid_stencil)",
                "lbfgsx_objective_bind_grid_stencil: the handle is a %s, not a grid stencil objective "
                "(lbfgsx_objective_compile_grid_stencil)"),
         dtype="lbfgsx_solver_minimize_grid_stencil: the objective was compiled for the other dtype",
         null="lbfgsx_solver_minimize_grid_stencil: invalid argument",
         unshaped=("a grid stencil objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_stencil",
                   "a grid stencil objective is bound with its shape and mask: lbfgsx_objective_bind_grid_stencil"),
         py_small=((2, 9), "StencilObjective: shape = (2, 9): a 3x3 patch needs at least 3 rows and 3 columns"),
         py_product="StencilObjective: shape = (4, 6) does not multiply to n = 25",
         py_shape="StencilObjective: shape must be (rows, cols)"),
]
BY_KEY = {f["key"]: f for f in FORMS}
NOUN = {"grid": "grid objective", "volume": "volume objective", "grid_periodic": "periodic grid objective",
        "volume_periodic": "periodic volume objective", "grid_field": "grid field objective",
        "grid_stencil": "grid stencil objective", "chain": "chain objective"}
IDS = [f["key"] for f in FORMS]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


@pytest.fixture(scope="module")
def objects(A):
    """one object of every form (and a chain objective): they own the handles, so they live as long as the module's tests"""
    out = {f["key"]: getattr(A, f["cls"])(f["body"], shape=f["good"], **f["kw"]) for f in FORMS}
    out["chain"] = A.ChainObjective("g[0] = x[1]; g[1] = x[0]; return x[0] * x[1];", K=2)
    return out


def _args(f, shape, mask=0):
    """a form's arguments between the handle and the data pointers"""
    return tuple(shape) + ((mask,) if f["mask_hi"] is not None else ())


def _solve(A, s, f, h, shape, mask=0):
    from lbfgspp_amd import _lib as L
    _, sol = A.load()
    x = np.zeros(f["n"])
    res = L.Result()
    rc = getattr(sol, "lbfgsx_solver_minimize_" + f["key"])(s._h, h, *_args(f, shape, mask), None, 0, None,
                                                            x.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res))
    return rc, res.msg.decode()


@pytest.mark.parametrize("f", FORMS, ids=IDS)
def test_the_solver_entry_points_refuse_in_these_words(A, objects, f):
    """extents, then overflow, then the mask, after the handle's form and dtype: no device is needed for any of it"""
    from lbfgspp_amd import _lib as L
    _, sol = A.load()
    s = A.LBFGSSolver(A.LBFGSParam())
    h = objects[f["key"]].compile()
    for shape, msg in f["too_small"]:
        assert _solve(A, s, f, h, shape) == (L.E_INVALID, msg)
    for shape, msg, _ in f["overflow"]:
        assert _solve(A, s, f, h, shape) == (L.E_INVALID, msg)
    for mask, msg in f.get("mask", []):
        assert _solve(A, s, f, h, f["good"], mask) == (L.E_INVALID, msg)
    if f["mask_hi"] is not None:
        # the order: a shape that is refused is refused before the mask is looked at
        assert _solve(A, s, f, h, f["too_small"][0][0], -1) == (L.E_INVALID, f["too_small"][0][1])
        assert _solve(A, s, f, h, f["overflow"][0][0], f["mask_hi"] + 1) == (L.E_INVALID, f["overflow"][0][1])
    # another form's handle, in both directions; a chain handle; the form before the dtype, the dtype before the shape
    g = BY_KEY[f["other"]]
    assert _solve(A, s, f, objects[g["key"]].compile(), f["good"]) == (L.E_INVALID, f["wrong"][0])
    assert _solve(A, s, g, h, g["good"]) == (L.E_INVALID, g["wrong"][0])
    assert _solve(A, s, f, objects["chain"].compile(), f["good"]) == (L.E_INVALID, f["wrong"][0])
    assert _solve(A, s, f, objects[g["key"]].compile(np.float32), f["good"]) == (L.E_INVALID, f["wrong"][0])
    assert _solve(A, s, f, objects[f["key"]].compile(np.float32), f["too_small"][0][0]) == (L.E_INVALID, f["dtype"])
    assert _solve(A, s, f, None, f["good"]) == (L.E_INVALID, f["null"])
    # the call without a shape names the one with it
    x = np.zeros(f["n"])
    res = L.Result()
    rc = sol.lbfgsx_solver_minimize_obj(s._h, h, f["n"], None, 0, None, x.ctypes.data_as(C.c_void_p), None, None, None, C.byref(res))
    assert (rc, res.msg.decode()) == (L.E_INVALID, f["unshaped"][0])
    # a request with nothing wrong gets as far as the device
    rc, msg = _solve(A, s, f, h, f["good"], f["mask_hi"] or 0)
    if A.load()[0].lbfgsx_device_count() <= 0:
        assert (rc, msg) == (L.E_NOGPU, "lbfgsx_solver_minimize_%s: no HIP device available (this library has no CPU fallback)"
                             % f["key"])
    else:
        assert rc == 0, msg


@pytest.mark.parametrize("f", FORMS, ids=IDS)
def test_the_python_classes_refuse_in_these_words(A, f):
    cls = getattr(A, f["cls"])
    shape, msg = f["py_small"]
    with pytest.raises(ValueError) as e:
        cls(f["body"], shape=shape, **f["kw"])
    assert str(e.value) == msg
    if f["py_shape"]:
        for bad in (f["good"] + (2,), f["good"][:-1], 7, ("a", "b", "c")[:len(f["good"])]):
            with pytest.raises(ValueError) as e:
                cls(f["body"], shape=bad, **f["kw"])
            assert str(e.value) == f["py_shape"]
    with pytest.raises(ValueError) as e:
        A.LBFGSSolver(A.LBFGSParam()).minimize(cls(f["body"], shape=f["good"], **f["kw"]), np.zeros(f["n"] + 1))
    assert str(e.value) == f["py_product"]
    if f["mask_hi"] is not None:
        axes = ("slabs", "rows", "cols")[-len(f["good"]):]
        with pytest.raises(ValueError) as e:
            cls(f["body"], shape=f["good"], periodic=(True,) * (len(axes) + 1), **f["kw"])
        assert str(e.value) == "%s: periodic must have one flag per axis, (%s)" % (f["cls"], ", ".join(axes))
        with pytest.raises(ValueError) as e:
            cls(f["body"], shape=f["good"], periodic=(2,) * len(axes), **f["kw"])
        assert str(e.value) == "%s: periodic = %r: a flag is True or False" % (f["cls"], (2,) * len(axes))
        ok = cls(f["body"], shape=f["good"], periodic=(True,) + (False,) * (len(axes) - 1), **f["kw"])
        assert ok.periodic == 1 << (len(axes) - 1) and ok.shape == f["good"]


def test_the_python_classes_refuse_d_and_a_numeric_mask_in_these_words(A):
    f, g = BY_KEY["grid_field"], BY_KEY["grid_stencil"]
    for D in (0, 4, True, 2.0):
        with pytest.raises(ValueError) as e:
            A.GridFieldObjective(f["body"], shape=f["good"], D=D)
        assert str(e.value) == "GridFieldObjective: D = %r is not supported: a node has D = 1, 2 or 3 unknowns" % (D,)
    for mask in (4, -1):
        with pytest.raises(ValueError) as e:
            A.StencilObjective(g["body"], shape=g["good"], periodic=mask)
        assert str(e.value) == "StencilObjective: periodic = %d: " % mask + MASK2
    assert A.StencilObjective(g["body"], shape=g["good"], periodic=2).periodic == 2
    # the shape is refused before D and the mask are looked at
    with pytest.raises(ValueError) as e:
        A.GridFieldObjective(f["body"], shape=(1, 1), D=7, periodic=(True,))
    assert str(e.value) == f["py_small"][1]
    with pytest.raises(ValueError) as e:
        A.StencilObjective(g["body"], shape=(2, 9), periodic=9)
    assert str(e.value) == g["py_small"][1]


def _context(A, n, dtype=None):
    """a context of n coordinates, or None where there is no device to make one on"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64 if dtype is None else dtype, n, 3, 0, 0)
    if core.lbfgsx_device_count() <= 0:
        assert rc != 0 and not ctx.value
        return None
    assert rc == 0
    return ctx


@pytest.mark.parametrize("f", FORMS, ids=IDS)
def test_the_bind_calls_refuse_in_these_words(A, objects, f):
    """the handle's form, then the extents, then the product, then the mask, then the dtype.  A context needs a device: without
    one the refusals are those of the solver's entry points above and this test only checks that no context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = _context(A, f["n"])
    if ctx is None:
        return
    oid = C.c_int(-1)

    def bind(form, h, shape, mask=0):
        rc = getattr(core, "lbfgsx_objective_bind_" + form["key"])(ctx, h, *_args(form, shape, mask), None, None, C.byref(oid))
        return rc, (L.last_error() if rc else "")
    try:
        h = objects[f["key"]].compile()
        for shape, msg in f["too_small"]:
            assert bind(f, h, shape) == (L.E_INVALID, msg)
        for shape, _, msg in f["overflow"]:
            assert bind(f, h, shape) == (L.E_INVALID, msg)
        assert bind(f, h, f["product"][0]) == (L.E_INVALID, f["product"][1])
        for mask, msg in f.get("mask", []):
            assert bind(f, h, f["good"], mask) == (L.E_INVALID, msg)
        if f["mask_hi"] is not None:
            assert bind(f, h, f["too_small"][0][0], -1) == (L.E_INVALID, f["too_small"][0][1])
            assert bind(f, h, f["product"][0], f["mask_hi"] + 1) == (L.E_INVALID, f["product"][1])
        g = BY_KEY[f["other"]]
        assert bind(f, objects[g["key"]].compile(), f["good"]) == (L.E_INVALID, f["wrong"][1] % NOUN[g["key"]])
        assert bind(g, h, g["good"]) == (L.E_INVALID, g["wrong"][1] % NOUN[f["key"]])
        assert bind(f, objects["chain"].compile(), f["good"]) == (L.E_INVALID, f["wrong"][1] % NOUN["chain"])
        h32 = objects[f["key"]].compile(np.float32)
        assert bind(f, h32, f["good"]) == (L.E_INVALID, "lbfgsx_objective_bind: the objective was compiled for the other dtype")
        assert bind(f, h32, f["product"][0]) == (L.E_INVALID, f["product"][1])  # the shape before the dtype
        assert core.lbfgsx_objective_bind(ctx, h, None, None, C.byref(oid)) == L.E_INVALID
        assert L.last_error() == f["unshaped"][1]
        assert bind(f, h, f["good"], f["mask_hi"] or 0) == (0, "") and oid.value == L.OBJ_BOUND
    finally:
        core.lbfgsx_destroy(ctx)


def test_shape_shape3_and_periodic_answer_for_these_forms(A, objects):
    """lbfgsx_objective_shape: the four forms on a grid; _shape3: the two on a volume; _periodic: the four with a mask; no other
    form, and no context without an objective"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    answers = {"grid": (True, False, False), "volume": (False, True, False), "grid_periodic": (True, False, True),
               "volume_periodic": (False, True, True), "grid_field": (True, False, True), "grid_stencil": (True, False, True),
               "chain": (False, False, False), "term": (False, False, False), "graph": (False, False, False), None: (False, False, False)}
    refusals = ("lbfgsx_objective_shape: no grid objective is bound to this context",
                "lbfgsx_objective_shape3: no volume objective is bound to this context",
                "lbfgsx_objective_periodic: no periodic grid or volume objective is bound to this context")
    term = A.TermObjective("g[0] = x[0]; return x[0];", K=1)
    graph = A.GraphObjective("g[0] = x[1]; g[1] = x[0]; return x[0] * x[1];", edges=([0, 1], [1, 2]))
    for key, want in answers.items():
        f = BY_KEY.get(key)
        ctx = _context(A, f["n"] if f else 12)
        if ctx is None:
            return
        oid = C.c_int(-1)
        try:
            if f:
                mask = f["mask_hi"] or 0
                rc = getattr(core, "lbfgsx_objective_bind_" + key)(ctx, objects[key].compile(), *_args(f, f["good"], mask), None, None,
                                                                   C.byref(oid))
            elif key == "graph":
                ei, ej = np.array([0, 1], np.int32), np.array([1, 2], np.int32)
                rc = core.lbfgsx_objective_bind_graph(ctx, graph.compile(), 2, ei.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      ej.ctypes.data_as(C.POINTER(C.c_int32)), 0, None, None, C.byref(oid))
            elif key:
                rc = core.lbfgsx_objective_bind(ctx, (objects["chain"] if key == "chain" else term).compile(), None, None, C.byref(oid))
            else:
                rc = 0
            assert rc == 0, L.last_error()
            r, c, s3, r3, c3 = (C.c_int64(-1) for _ in range(5))
            m = C.c_int(-1)
            for k, call in enumerate((lambda: core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)),
                                      lambda: core.lbfgsx_objective_shape3(ctx, C.byref(s3), C.byref(r3), C.byref(c3)),
                                      lambda: core.lbfgsx_objective_periodic(ctx, C.byref(m)))):
                rc = call()
                assert (rc == 0) == want[k], (key, k)
                if rc:
                    assert rc == L.E_INVALID and L.last_error() == refusals[k]
            assert (r.value, c.value) == (f["good"] if want[0] else (-1, -1))
            assert (s3.value, r3.value, c3.value) == (f["good"] if want[1] else (-1, -1, -1))
            assert m.value == (mask if want[2] else -1)
        finally:
            core.lbfgsx_destroy(ctx)
