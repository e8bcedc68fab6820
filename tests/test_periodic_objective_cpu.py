"""CPU suite: periodic grid and volume objectives compiled at run time (lbfgspp_amd.PeriodicGridObjective,
PeriodicVolumeObjective; lbfgsx_objective_compile_grid_periodic and _volume_periodic of include/lbfgsx.h).  Everything here runs
without a GPU: hipRTC compiles for the fixed target gfx950, and what the code object says about its kernels is read from the
code object itself."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import grid_ref as GR
import periodic_ref as PR
import volume_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID_KERNELS = ("k_pgrid_eval", "k_pgrid_trial", "k_pgrid_b_eval", "k_pgrid_b_dg_maxstep_trial")
VOLUME_KERNELS = ("k_pvolume_eval", "k_pvolume_trial", "k_pvolume_b_eval", "k_pvolume_b_dg_maxstep_trial")
SHAPES2 = [(2, 2), (2, 3), (3, 2), (3, 5), (5, 3), (5, 5)]
SHAPES3 = [(2, 2, 2), (2, 3, 5), (3, 2, 2), (5, 2, 3), (3, 5, 2)]
CASES = [(s, m) for s in SHAPES2 for m in range(4)] + [(s, m) for s in SHAPES3 for m in range(8)]


@pytest.fixture(scope="module")
def A():
    import lbfgspp_amd as A
    A.load()
    return A


def _instance(shape, dtype):
    rng = np.random.default_rng(sum(1000 ** k * e for k, e in enumerate(shape)) + 17)
    n = int(np.prod(shape))
    return rng.standard_normal(n).astype(dtype), (0.5 + rng.random(n)).astype(dtype)


def _terms(name, x, shape, p0):
    if len(shape) == 2:
        return PR.pasym4_terms(x, shape, p0) if name == "asym" else PR.allencahn_terms(x, shape, 0.75)
    return PR.pasym8_terms(x, shape, p0) if name == "asym" else PR.allencahn3_terms(x, shape, 0.75)


# ---------------------------------------------------------------- the numpy restatement
def _asym_cell(dt, xs, ws, pos):
    """one cell of PASYM4 / PASYM8 in scalar arithmetic of dtype dt, operation for operation"""
    if len(xs) == 4:
        c0, c1 = (dt(v) for v in GR.ASYM_SCALARS)
        s = dt(dt(dt(dt(ws[0] * xs[0]) + dt(dt(2) * dt(ws[1] * xs[1]))) + dt(dt(3) * dt(ws[2] * xs[2]))) + dt(dt(5) * dt(ws[3] * xs[3])))
        q = dt(s + dt(dt(dt(pos[0]) * c0) + dt(dt(pos[1]) * c1)))
        w = (1, 2, 3, 5)
    else:
        c0, c1, c2 = (dt(v) for v in VR.ASYM_SCALARS)
        s0 = dt(dt(dt(dt(ws[0] * xs[0]) + dt(dt(2) * dt(ws[1] * xs[1]))) + dt(dt(3) * dt(ws[2] * xs[2]))) + dt(dt(5) * dt(ws[3] * xs[3])))
        s1 = dt(dt(dt(dt(dt(7) * dt(ws[4] * xs[4])) + dt(dt(11) * dt(ws[5] * xs[5]))) + dt(dt(13) * dt(ws[6] * xs[6]))) +
                dt(dt(17) * dt(ws[7] * xs[7])))
        q = dt(dt(s0 + s1) + dt(dt(dt(dt(pos[0]) * c0) + dt(dt(pos[1]) * c1)) + dt(dt(pos[2]) * c2)))
        w = VR.WEIGHTS
    g = [dt(ws[0] * q)] + [dt(dt(wk) * dt(ws[k] * q)) for k, wk in enumerate(w) if k]
    return g, dt(dt(0.5) * dt(q * q))


def _corner_index(shape, origin):
    out = []
    for off in PR.offsets(len(shape)):
        flat = 0
        for ext, o, d in zip(shape, origin, off):
            flat = flat * ext + (o + d) % ext
        out.append(flat)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape,mask", CASES)
def test_the_restatement_is_the_scalar_loop_bit_for_bit(shape, mask, dtype):
    """the terms cell by cell with wrapped corner indices, the gradient node by node by the rule of include/lbfgsx.h, and every
    existing cell counted once per slot and no other cell at all"""
    x, p0 = _instance(shape, dtype)
    dt = np.dtype(dtype).type
    tg, v = _terms("asym", x, shape, p0)
    ex = PR.exists(shape, mask)
    for origin in itertools.product(*(range(e) for e in shape)):
        idx = _corner_index(shape, origin)
        g, val = _asym_cell(dt, [x[k] for k in idx], [p0[k] for k in idx], origin)
        assert val.tobytes() == v[origin].tobytes()
        assert [a.tobytes() for a in g] == [t[origin].tobytes() for t in tg]
        want = all(o < e - 1 or PR.axis_periodic(shape, mask, ax) for ax, (o, e) in enumerate(zip(origin, shape)))
        assert bool(ex[origin]) == want
    for name in ("asym", "allencahn"):
        tg, v = _terms(name, x, shape, p0)
        assert v.dtype == dtype and all(a.dtype == dtype and a.shape == tuple(shape) for a in tg)
        grad = PR.periodic_grad(tg, shape, mask)
        loop, used = PR.periodic_grad_scalar(tg, shape, mask)
        assert grad.dtype == dtype and grad.tobytes() == loop.tobytes()
        assert np.array_equal(used, np.broadcast_to(ex[..., None], used.shape).astype(np.int64))


@pytest.mark.parametrize("shape,mask", [(s, m) for s, m in CASES if s in ((3, 5), (2, 3, 5))])
def test_the_gradient_is_the_derivative_of_the_sum_of_the_existing_cells(shape, mask):
    x, p0 = _instance(shape, np.float64)
    n = x.size
    for name in ("asym", "allencahn"):
        grad = PR.periodic_grad(_terms(name, x, shape, p0)[0], shape, mask)
        for k in range(n):
            e = np.zeros(n)
            e[k] = 1e-6
            fd = (PR.value_exact(_terms(name, x + e, shape, p0)[1], shape, mask) -
                  PR.value_exact(_terms(name, x - e, shape, p0)[1], shape, mask)) / 2e-6
            assert abs(fd - grad[k]) <= 1e-6 * (1.0 + abs(grad[k]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_with_the_mask_zero_the_restatement_is_the_open_forms(dtype):
    for shape in SHAPES2:
        x, p0 = _instance(shape, dtype)
        for mine, theirs in ((PR.pasym4_terms(x, shape, p0), GR.asym4_terms(x, *shape, p0)),
                             (PR.allencahn_terms(x, shape, 0.75), GR.allencahn_terms(x, *shape, 0.75))):
            assert PR.periodic_grad(mine[0], shape, 0).tobytes() == GR.grid_grad(theirs[0], *shape).tobytes()
            assert PR.values(mine[1], shape, 0).tobytes() == theirs[1].reshape(-1).tobytes()
    for shape in SHAPES3:
        x, p0 = _instance(shape, dtype)
        for mine, theirs in ((PR.pasym8_terms(x, shape, p0), VR.asym8_terms(x, *shape, p0)),
                             (PR.allencahn3_terms(x, shape, 0.75), VR.allencahn3_terms(x, *shape, 0.75))):
            assert PR.periodic_grad(mine[0], shape, 0).tobytes() == VR.volume_grad(theirs[0], *shape).tobytes()
            assert PR.values(mine[1], shape, 0).tobytes() == theirs[1].reshape(-1).tobytes()


@pytest.mark.parametrize("shape", [(3, 5), (5, 2), (2, 3, 5), (3, 2, 4)])
def test_on_a_torus_rolling_x_and_p0_rolls_the_gradient(shape):
    """with a body that ignores position (the scalars zero) the rule is translation-invariant on a full torus, bit for bit"""
    full = 2 ** len(shape) - 1
    x, p0 = _instance(shape, np.float64)
    zeros = (0.0,) * len(shape)
    terms = PR.pasym4_terms if len(shape) == 2 else PR.pasym8_terms
    g = PR.periodic_grad(terms(x, shape, p0, zeros)[0], shape, full).reshape(shape)
    axes = tuple(range(len(shape)))
    for shift in itertools.product(*(range(e) for e in shape)):
        xr = np.roll(x.reshape(shape), shift, axes).reshape(-1)
        pr = np.roll(p0.reshape(shape), shift, axes).reshape(-1)
        gr = PR.periodic_grad(terms(xr, shape, pr, zeros)[0], shape, full).reshape(shape)
        assert gr.tobytes() == np.roll(g, shift, axes).tobytes()


# ---------------------------------------------------------------- compilation
def _objective(A, body, volume, **kw):
    if volume:
        return A.PeriodicVolumeObjective(body, shape=kw.pop("shape", (3, 4, 5)), **kw)
    return A.PeriodicGridObjective(body, shape=kw.pop("shape", (4, 5)), **kw)


BODIES = [(PR.PASYM4, False), (PR.ALLENCAHN, False), (PR.PASYM8, True), (PR.ALLENCAHN3, True)]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("body,volume", BODIES, ids=["asym4", "allencahn", "asym8", "allencahn3"])
def test_both_bodies_compile_for_both_dtypes_without_scratch(A, body, volume, dtype):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    f = _objective(A, body, volume)
    info = f.info(dtype)
    print(info)
    assert info["scratch_bytes"] == 0 and all(v == 0 for v in info["scratch_by_kernel"].values())
    assert 0 < info["vgprs"] <= 512 and info["compile_ms"] > 0
    h = f.compile(dtype)
    assert core.lbfgsx_objective_K(h) == (8 if volume else 4) and core.lbfgsx_objective_form(h) == (11 if volume else 10)
    assert core.lbfgsx_objective_dtype(h) == (L.F64 if dtype == np.float64 else L.F32)


def test_generated_source_holds_the_body_once_and_the_new_kernels(A):
    for body, volume in BODIES:
        for dtype in (np.float64, np.float32):
            src = _objective(A, body, volume).source(dtype)
            assert src.count(body) == 1
            if volume:
                assert '#include "periodic_volume_kernels.cuh"' in src and "int64_t slabs, rows, cols;" in src
                assert ("term(const T (&x)[8], T (&g)[8], int64_t i, int64_t slab, int64_t row, int64_t col, "
                        "const int64_t (&j)[8]) const") in src
                assert "struct ObjVolumePeriodic" in src and "static constexpr int K = 8;" in src
            else:
                assert '#include "periodic_grid_kernels.cuh"' in src and "int64_t rows, cols;" in src
                assert "term(const T (&x)[4], T (&g)[4], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const" in src
                assert "struct ObjGridPeriodic" in src and "static constexpr int K = 4;" in src
            assert "int periodic, pad_;" in src
            for k in (VOLUME_KERNELS if volume else GRID_KERNELS):
                assert "template __global__ void %s<S, %s>" % (k, "ObjVolumePeriodic" if volume else "ObjGridPeriodic") in src
            assert src.count("template __global__") == 4
            assert "__global__ void __launch_bounds__" not in src  # the kernels are included, not restated
            assert ("typedef double term_scalar_t" in src) == (dtype == np.float64)


def test_the_open_forms_sources_name_none_of_the_new_kernels(A):
    for src in (A.GridObjective(GR.ALLENCAHN, shape=(2, 2)).source(), A.VolumeObjective(VR.ALLENCAHN3, shape=(2, 2, 2)).source()):
        assert "pgrid" not in src and "pvolume" not in src and "periodic" not in src.lower()


def test_grid_periodic_and_volume_periodic_of_one_text_are_two_cache_entries(A):
    core, _ = A.load()
    # a text that is valid as either: as a volume cell its g[4..7] stay unset, which this test never runs
    body = "g[0] = x[0]; g[1] = x[1]; g[2] = x[2]; g[3] = x[3]; return x[0] * x[3];\n// cache test of the periodic forms"
    grid, vol = A.PeriodicGridObjective(body, shape=(2, 2)), A.PeriodicVolumeObjective(body, shape=(2, 2, 2))
    ig, iv = grid.info(), vol.info()
    assert not ig["cache_hit"] and not iv["cache_hit"]
    hg, hv = grid.compile(), vol.compile()
    assert hg.value != hv.value and core.lbfgsx_objective_form(hg) == 10 and core.lbfgsx_objective_form(hv) == 11
    # neither the shape nor the mask is part of the key
    again = A.PeriodicVolumeObjective(body, shape=(7, 9, 3), periodic=(False, True, False)).info()
    assert again["cache_hit"] and again["compile_ms"] == iv["compile_ms"] and again["vgprs"] == iv["vgprs"]
    assert A.PeriodicGridObjective(body, shape=(3, 3), periodic=(True, False)).info()["cache_hit"]
    assert not A.GridObjective(body, shape=(3, 3)).info()["cache_hit"]  # the open form of the same text is another entry
    assert not A.PeriodicGridObjective(body, shape=(2, 2)).info(np.float32)["cache_hit"]


def test_the_mask_of_the_python_classes(A):
    assert A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3)).periodic == 3
    assert A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3), periodic=(True, False)).periodic == 2
    assert A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3), periodic=(False, True)).periodic == 1
    assert A.PeriodicVolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 2)).periodic == 7
    assert A.PeriodicVolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 2), periodic=(True, False, False)).periodic == 4
    assert A.PeriodicVolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 2), periodic=(False, False, True)).periodic == 1
    with pytest.raises(ValueError, match="periodic must have one flag per axis, \\(rows, cols\\)"):
        A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3), periodic=(True, True, True))
    with pytest.raises(ValueError, match="periodic must have one flag per axis, \\(slabs, rows, cols\\)"):
        A.PeriodicVolumeObjective(VR.ALLENCAHN3, shape=(2, 3, 2), periodic=True)
    for bad in ("ab", (True, 2), (None, False), (1.0, 0.0)):
        with pytest.raises(ValueError, match="PeriodicGridObjective: periodic = .*: a flag is True or False"):
            A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3), periodic=bad)
    assert A.PeriodicGridObjective(GR.ALLENCAHN, shape=(2, 3), periodic=(1, np.bool_(False))).periodic == 2


# ---------------------------------------------------------------- refusals
def test_body_with_inline_assembly_or_nothing_is_refused(A):
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    word = "as" + "m"
    fill = "for (int k = 0; k < 4; k++) g[k] = x[0];"
    for volume in (False, True):
        for body in ("%s volatile(\"\");\n%s\nreturn x[0];" % (word, fill), "%s __%s__(\"\"); return x[0];" % (fill, word)):
            with pytest.raises(ValueError, match="inline assembly is not accepted"):
                _objective(A, body, volume).compile()
    h = C.c_void_p()
    log = C.create_string_buffer(1024)
    for suffix, name, body in (("grid_periodic", b"periodic grid objective", PR.ALLENCAHN),
                               ("volume_periodic", b"periodic volume objective", PR.ALLENCAHN3)):
        compile_, source = getattr(core, "lbfgsx_objective_compile_" + suffix), getattr(core, "lbfgsx_objective_source_" + suffix)
        for empty in (b"", None):
            assert compile_(C.byref(h), L.F64, empty, log, len(log)) == L.E_INVALID
            assert not h.value and name + b": empty body" in log.value
            assert source(L.F64, empty, None, 0) == L.E_INVALID
        assert compile_(C.byref(h), 7, body.encode(), log, len(log)) == L.E_INVALID
        assert b"unknown dtype" in log.value


def test_compile_error_comes_back_with_body_relative_lines(A):
    bad = "const T r = x[0];\nfor (int k = 0; k < 4; k++) g[k] = r;\ng[3] = r\nreturn r * r;"  # line 3 lacks its semicolon
    for volume, name in ((False, "PeriodicGridObjective"), (True, "PeriodicVolumeObjective")):
        with pytest.raises(ValueError) as e:
            _objective(A, bad, volume).compile()
        assert name in str(e.value) and "objective_body:3:" in str(e.value) and "error" in str(e.value)


def test_shapes_and_masks_that_are_refused_by_value(A):
    from lbfgspp_amd import _lib as L
    core, sol = A.load()
    for shape in ((1, 6), (6, 1), (0, 0)):
        with pytest.raises(ValueError, match="PeriodicGridObjective: shape = \\(%d, %d\\): a grid has at least 2 rows and 2 columns"
                                             % shape):
            A.PeriodicGridObjective(PR.ALLENCAHN, shape=shape)
    for shape in ((1, 6, 2), (6, 1, 2), (2, 6, 1)):
        with pytest.raises(ValueError, match="PeriodicVolumeObjective: shape = \\(%d, %d, %d\\): a volume has at least 2 slabs" % shape):
            A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=shape)
    with pytest.raises(ValueError, match="shape must be \\(slabs, rows, cols\\)"):
        A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=(4, 4))
    with pytest.raises(ValueError, match="shape must be \\(rows, cols\\)"):
        A.PeriodicGridObjective(PR.ALLENCAHN, shape=(4, 4, 4))
    s = A.LBFGSSolver(A.LBFGSParam())
    with pytest.raises(ValueError, match="PeriodicGridObjective: shape = \\(3, 5\\) does not multiply to n = 16"):
        s.minimize(A.PeriodicGridObjective(PR.ALLENCAHN, shape=(3, 5), scalars=(1.0,)), np.zeros(16))
    with pytest.raises(ValueError, match="PeriodicVolumeObjective: shape = \\(2, 3, 5\\) does not multiply to n = 31"):
        s.minimize(A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=(2, 3, 5), scalars=(1.0,)), np.zeros(31))
    # the C entry points of the solver say the same before a device is needed
    fg, fv = A.PeriodicGridObjective(PR.ALLENCAHN, shape=(2, 2)), A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=(2, 2, 2))
    hg, hv = fg.compile(), fv.compile()  # the handles live as long as their objects
    x = np.zeros(12)
    xp = x.ctypes.data_as(C.c_void_p)
    res = L.Result()
    for rows, cols, mask, what in ((1, 12, 3, b"rows = 1, cols = 12"), (12, 1, 3, b"rows = 12, cols = 1"), (-3, -4, 0, b"rows = -3, cols = -4"),
                                   (2 ** 40, 2 ** 40, 1, b"overflows"), (3, 4, 4, b"periodic = 4"), (3, 4, -1, b"periodic = -1")):
        rc = sol.lbfgsx_solver_minimize_grid_periodic(s._h, hg, rows, cols, mask, None, 0, None, xp, None, None, None, C.byref(res))
        assert rc == L.E_INVALID and what in res.msg and b"periodic grid objective: " in res.msg, res.msg
    for slabs, rows, cols, mask, what in ((1, 6, 2, 7, b"slabs = 1, rows = 6, cols = 2"), (6, 1, 2, 7, b"slabs = 6, rows = 1, cols = 2"),
                                          (2, 6, 1, 7, b"slabs = 2, rows = 6, cols = 1"), (2 ** 30, 2 ** 30, 2 ** 30, 0, b"overflows"),
                                          (2, 3, 2, 8, b"periodic = 8"), (2, 3, 2, -2, b"periodic = -2")):
        rc = sol.lbfgsx_solver_minimize_volume_periodic(s._h, hv, slabs, rows, cols, mask, None, 0, None, xp, None, None, None,
                                                        C.byref(res))
        assert rc == L.E_INVALID and what in res.msg and b"periodic volume objective: " in res.msg, res.msg
    # lbfgsx_solver_minimize_obj carries no shape; every shaped entry point refuses another form
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hg, 12, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"a periodic grid objective is minimised with its shape and mask: lbfgsx_solver_minimize_grid_periodic" in res.msg
    rc = sol.lbfgsx_solver_minimize_obj(s._h, hv, 12, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"lbfgsx_solver_minimize_volume_periodic" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid(s._h, hg, 3, 4, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a grid objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_volume(s._h, hv, 2, 3, 2, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a volume objective" in res.msg
    open_grid = A.GridObjective(GR.ALLENCAHN, shape=(2, 2))
    rc = sol.lbfgsx_solver_minimize_grid_periodic(s._h, open_grid.compile(), 3, 4, 3, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a periodic grid objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_volume_periodic(s._h, hg, 2, 3, 2, 7, None, 0, None, xp, None, None, None, C.byref(res))
    assert rc == L.E_INVALID and b"not a periodic volume objective" in res.msg
    rc = sol.lbfgsx_solver_minimize_grid_periodic(s._h, fg.compile(np.float32), 3, 4, 3, None, 0, None, xp, None, None, None,
                                                  C.byref(res))
    assert rc == L.E_INVALID and b"the other dtype" in res.msg
    with pytest.raises(ValueError, match="PeriodicGridObjective: data\\[0\\] must have 12 elements"):
        s.minimize(A.PeriodicGridObjective(PR.PASYM4, shape=(3, 4), data=(np.ones(8),), scalars=GR.ASYM_SCALARS), np.zeros(12))


def test_binding_refusals_name_the_values(A):
    """the bind calls on a context: the context needs a device, so without one the refusals are those of the solver's entry
    points above and this test only checks that no context can be made"""
    from lbfgspp_amd import _lib as L
    core, _ = A.load()
    ctx = C.c_void_p()
    rc = core.lbfgsx_create(C.byref(ctx), L.F64, 24, 3, 0, 0)
    if core.lbfgsx_device_count() <= 0:
        assert rc != 0 and not ctx.value
        return
    assert rc == 0
    try:
        fg, fv = A.PeriodicGridObjective(PR.ALLENCAHN, shape=(4, 6)), A.PeriodicVolumeObjective(PR.ALLENCAHN3, shape=(2, 3, 4))
        fo = A.GridObjective(GR.ALLENCAHN, shape=(4, 6))
        hg, hv, ho = fg.compile(), fv.compile(), fo.compile()
        oid = C.c_int(-1)
        for h, args, what in ((hg, (1, 24, 3), "rows = 1, cols = 24"), (hg, (24, 1, 3), "rows = 24, cols = 1"),
                              (hg, (4, 5, 3), "rows = 4, cols = 5 does not multiply to n = 24"),
                              (hg, (2 ** 40, 2 ** 40, 3), "does not multiply to n = 24"), (hg, (4, 6, 4), "periodic = 4"),
                              (hg, (4, 6, -1), "periodic = -1"), (ho, (4, 6, 3), "grid objective, not a periodic grid"),
                              (hv, (4, 6, 3), "periodic volume objective, not a periodic grid")):
            assert core.lbfgsx_objective_bind_grid_periodic(ctx, h, *args, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        for h, args, what in ((hv, (1, 6, 4, 7), "slabs = 1, rows = 6, cols = 4"), (hv, (6, 4, 1, 7), "slabs = 6, rows = 4, cols = 1"),
                              (hv, (2, 3, 5, 7), "slabs = 2, rows = 3, cols = 5 does not multiply to n = 24"),
                              (hv, (2, 3, 4, 8), "periodic = 8"), (hg, (2, 3, 4, 7), "periodic grid objective, not a periodic volume")):
            assert core.lbfgsx_objective_bind_volume_periodic(ctx, h, *args, None, None, C.byref(oid)) == L.E_INVALID
            assert what in L.last_error(), L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hg, None, None, C.byref(oid)) == L.E_INVALID
        assert "a periodic grid objective is bound with its shape and mask: lbfgsx_objective_bind_grid_periodic" in L.last_error()
        assert core.lbfgsx_objective_bind(ctx, hv, None, None, C.byref(oid)) == L.E_INVALID
        assert "lbfgsx_objective_bind_volume_periodic" in L.last_error()
        assert core.lbfgsx_objective_bind_grid(ctx, hg, 4, 6, None, None, C.byref(oid)) == L.E_INVALID
        assert "periodic grid objective, not a grid" in L.last_error()
        assert core.lbfgsx_objective_bind_volume(ctx, hv, 2, 3, 4, None, None, C.byref(oid)) == L.E_INVALID
        assert "periodic volume objective, not a volume" in L.last_error()
        m = C.c_int(-1)
        s, r, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == L.E_INVALID  # nothing bound yet
        assert core.lbfgsx_objective_bind_grid_periodic(ctx, hg, 4, 6, 2, None, None, C.byref(oid)) == 0 and oid.value == L.OBJ_BOUND
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == 0 and m.value == 2
        assert core.lbfgsx_objective_shape(ctx, C.byref(r), C.byref(c)) == 0 and (r.value, c.value) == (4, 6)
        assert core.lbfgsx_objective_shape3(ctx, C.byref(s), C.byref(r), C.byref(c)) == L.E_INVALID
        assert core.lbfgsx_objective_bind_volume_periodic(ctx, hv, 2, 3, 4, 5, None, None, C.byref(oid)) == 0
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == 0 and m.value == 5
        assert core.lbfgsx_objective_shape3(ctx, C.byref(s), C.byref(r), C.byref(c)) == 0
        assert (s.value, r.value, c.value) == (2, 3, 4)
        assert core.lbfgsx_objective_bind_grid(ctx, ho, 4, 6, None, None, C.byref(oid)) == 0  # an open form: no mask to read
        assert core.lbfgsx_objective_periodic(ctx, C.byref(m)) == L.E_INVALID
        assert core.lbfgsx_objective_bind_grid_periodic(ctx, fg.compile(np.float32), 4, 6, 3, None, None, C.byref(oid)) == L.E_INVALID
        assert "the other dtype" in L.last_error()
    finally:
        core.lbfgsx_destroy(ctx)


NEW_CORE = ["lbfgsx_objective_compile_grid_periodic", "lbfgsx_objective_source_grid_periodic", "lbfgsx_objective_bind_grid_periodic",
            "lbfgsx_objective_compile_volume_periodic", "lbfgsx_objective_source_volume_periodic",
            "lbfgsx_objective_bind_volume_periodic", "lbfgsx_objective_periodic"]
NEW_SOLVER = ["lbfgsx_solver_minimize_grid_periodic", "lbfgsx_solver_minimize_volume_periodic"]


def test_new_symbols_are_exported_and_declared(A):
    listed = open(os.path.join(ROOT, "lbfgspp_amd", "csrc", "export.map")).read()

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "lbfgspp_amd", lib)], stdout=subprocess.PIPE,
                             text=True, check=True).stdout
        return {line.split()[-1] for line in out.splitlines() if line.strip()}
    for names, lib, header in ((NEW_CORE, "liblbfgsx.so", "lbfgsx.h"), (NEW_SOLVER, "liblbfgsx_solver.so", "lbfgsx_solver.h")):
        have, text = exported(lib), open(os.path.join(ROOT, "include", header)).read()
        for name in names:
            assert name in have, "%s does not export %s" % (lib, name)
            assert name + ";" in listed, "export.map does not list %s" % name
            assert name + "(" in text, "%s does not declare %s" % (header, name)
    text = open(os.path.join(ROOT, "include", "lbfgsx.h")).read()
    assert "LBFGSX_FORM_GRID_PERIODIC = 10" in text and "LBFGSX_FORM_VOLUME_PERIODIC = 11" in text
    for name in ("PeriodicGridObjective", "PeriodicVolumeObjective"):
        assert name in A.__all__ and issubclass(getattr(A, name), A.TermObjective)
    device_h = open(os.path.join(ROOT, "include", "LBFGSpp", "Device.h")).read()
    assert "class PeriodicGridObjective : public TermObjective<Scalar>" in device_h
    assert "class PeriodicVolumeObjective : public TermObjective<Scalar>" in device_h


def test_generated_wrappers_and_kernel_headers_name_no_inline_assembly(A):
    """the text generated around a body and the headers it includes hold no inline assembly of their own (the word is spelt in
    pieces so that this file does not hold it either)"""
    word = "as" + "m"
    text = _objective(A, PR.ALLENCAHN, False).source() + _objective(A, PR.ALLENCAHN3, True).source()
    for name in ("periodic_grid_kernels.cuh", "periodic_volume_kernels.cuh"):
        text += open(os.path.join(ROOT, "lbfgspp_amd", "csrc", name)).read()
    assert word + "(" not in text and word + " volatile" not in text and "__" + word not in text
