"""CPU suite: the caller-supplied objective through the C ABI and the Python package -- what can be said without a GPU.
The entry points exist with the documented prototypes, LBFGSX_E_USER is a new code beside the unchanged old ones, nothing
falls back to a CPU path or calls the callback when there is no device, and the Python wrappers reject bad arguments before
any native call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    import lbfgspp_amd as A
    return A.load()


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_entry_points_are_exported_with_the_documented_prototypes(libs):
    core, sol = libs
    for name in ("lbfgsx_solver_minimize_fn", "lbfgsx_lockstep_minimize_fn"):
        assert hasattr(sol, name), "liblbfgsx_solver.so does not export %s" % name
    for name in ("lbfgsx_bat_pack", "lbfgsx_bat_unpack", "lbfgsx_bat_packed", "lbfgsx_bat_set_x0", "lbfgsx_bat_device_push"):
        assert hasattr(core, name), "liblbfgsx.so does not export %s" % name
    h = _header("lbfgsx_solver.h")
    assert ("typedef int (*lbfgsx_objective_fn)(void* user, const void* x_dev, void* grad_dev, int64_t n, double* fx);") in h
    assert ("int lbfgsx_solver_minimize_fn(lbfgsx_solver* s, int64_t n, lbfgsx_objective_fn fn, void* user, void* x, "
            "const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);") in h
    assert ("typedef int (*lbfgsx_batch_objective_fn)(void* user, int nact, const int64_t* ids, const void* X, void* G, "
            "int64_t ld, double* fx);") in h
    assert ("int lbfgsx_lockstep_minimize_fn(lbfgsx_lockstep* h, const void* x0, lbfgsx_batch_objective_fn eval, void* user, "
            "lbfgsx_batch_item* out, void* x_out, double stats[8], char* errbuf, int errlen);") in h


def test_user_status_code_is_new_and_the_old_ones_keep_their_values():
    from lbfgspp_amd import _lib as L
    h = _header("lbfgsx.h")
    codes = dict((k, int(v)) for k, v in re.findall(r"(LBFGSX_(?:OK|E_[A-Z]+)) = (-?\d+)", h))
    assert codes == {"LBFGSX_OK": 0, "LBFGSX_E_INVALID": -1, "LBFGSX_E_LOGIC": -2, "LBFGSX_E_RUNTIME": -3, "LBFGSX_E_HIP": -4,
                     "LBFGSX_E_NOGPU": -5, "LBFGSX_E_USER": -6}
    assert (L.E_INVALID, L.E_LOGIC, L.E_RUNTIME, L.E_HIP, L.E_NOGPU, L.E_USER) == (-1, -2, -3, -4, -5, -6)


def test_without_a_gpu_both_entry_points_answer_nogpu_and_never_call_back(libs):
    """same stance as test_abi_cpu.py: no CPU path; with a GPU this test is a no-op"""
    core, sol = libs
    if core.lbfgsx_device_count() > 0:
        pytest.skip("GPU present")
    import lbfgspp_amd as A
    from lbfgspp_amd import _lib as L
    calls = []

    def single(_u, _x, _g, _n, _fx):
        calls.append("single")
        return 0

    def batch(_u, _nact, _ids, _X, _G, _ld, _fx):
        calls.append("batch")
        return 0

    for algo_solver in (A.LBFGSSolver(A.LBFGSParam()), A.LBFGSBSolver(A.LBFGSBParam())):
        res = L.Result()
        x = np.zeros(10)
        rc = sol.lbfgsx_solver_minimize_fn(algo_solver._h, 10, L.OBJECTIVE_FN(single), None, x.ctypes.data_as(C.c_void_p),
                                           x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), None, C.byref(res))
        assert rc == L.E_NOGPU and res.status == L.E_NOGPU and b"no HIP device" in res.msg
    # the batch: no handle can be created, and the entry point itself says why
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    cp = A.LBFGSParam()._c()
    assert sol.lbfgsx_lockstep_create(C.byref(h), L.F32, L.LS_MORE_THUENTE, C.byref(cp), 64, 2, 0, 0, err, 256) != 0
    assert b"no HIP device" in err.value and not h
    items = (L.BatchItem * 2)()
    x0 = np.zeros((2, 64), np.float32)
    rc = sol.lbfgsx_lockstep_minimize_fn(None, x0.ctypes.data_as(C.c_void_p), L.BATCH_OBJECTIVE_FN(batch), None, items, None,
                                         None, err, 256)
    assert rc == L.E_NOGPU and b"no HIP device" in err.value
    # ... and through the Python wrappers
    with pytest.raises(RuntimeError, match="no HIP device"):
        A.LBFGSSolver(A.LBFGSParam()).minimize(A.DeviceObjective(lambda x, g: calls.append("py") or 0.0), np.zeros(10))
    assert calls == []


def test_python_wrappers_reject_bad_arguments_before_any_native_call():
    import lbfgspp_amd as A
    from lbfgspp_amd import batched as B
    with pytest.raises(TypeError, match="callable"):
        A.DeviceObjective(3.0)
    with pytest.raises(TypeError, match="callable"):
        A.DeviceObjective.from_autograd(None)
    s = A.LBFGSSolver(A.LBFGSParam())
    s._sol = None  # any native call from here on would raise AttributeError instead
    with pytest.raises(TypeError, match="DeviceObjective"):
        s.minimize(lambda x, g: 0.0, np.zeros(4))
    batch = object.__new__(B.LockstepBatch)  # (a real one needs a device)
    batch.n, batch.count, batch.dtype, batch.device, batch._h, batch._sol = 8, 3, np.dtype(np.float32), 0, None, None
    with pytest.raises(TypeError, match="callable"):
        batch.minimize_fn(None, np.zeros((3, 8), np.float32))
    for bad in (np.zeros((3, 7), np.float32), np.zeros((2, 8), np.float32), np.zeros(24, np.float32), [0.0] * 24):
        with pytest.raises(ValueError, match=r"shape \(count, n\)"):
            batch.minimize_fn(lambda ids, X, G: None, bad)
