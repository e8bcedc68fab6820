"""ctypes bindings of liblbfgsx.so / liblbfgsx_solver.so (the product path: native HIP only)."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))

F64, F32 = 0, 1
OBJ_DIAG_QUAD, OBJ_EXT_ROSENBROCK = 0, 1
OBJ_BOUND = 64  # the term objective bound to a context (lbfgsx_objective_bind)
LS_NOCEDAL_WRIGHT, LS_MORE_THUENTE, LS_BACKTRACKING, LS_BRACKETING = 0, 1, 2, 3
ALGO_LBFGS, ALGO_LBFGSB = 0, 1
RECURSION_VECTOR, RECURSION_GRAM_SPACE, RECURSION_GRAM_SPACE_F32H = 0, 1, 2
FLAG_BOUNDED = 1
(VEC_X, VEC_G, VEC_XP, VEC_GP, VEC_D, VEC_XT, VEC_GT, VEC_A, VEC_B, VEC_LB, VEC_UB, VEC_XCP) = range(12)
E_INVALID, E_LOGIC, E_RUNTIME, E_HIP, E_NOGPU, E_USER = -1, -2, -3, -4, -5, -6


class Params(C.Structure):
    _fields_ = [("m", C.c_int), ("epsilon", C.c_double), ("epsilon_rel", C.c_double), ("past", C.c_int),
                ("delta", C.c_double), ("max_iterations", C.c_int), ("linesearch", C.c_int),
                ("max_linesearch", C.c_int), ("min_step", C.c_double), ("max_step", C.c_double),
                ("ftol", C.c_double), ("wolfe", C.c_double), ("max_submin", C.c_int)]


class Result(C.Structure):
    _fields_ = [("niter", C.c_int), ("nfev", C.c_int), ("fx", C.c_double), ("gnorm", C.c_double),
                ("status", C.c_int), ("msg", C.c_char * 200)]


class BatchItem(C.Structure):
    _fields_ = [("niter", C.c_int), ("nfev", C.c_int), ("status", C.c_int), ("fx", C.c_double), ("gnorm", C.c_double)]


class Trace(C.Structure):
    _fields_ = [("cap", C.c_int), ("count", C.c_int), ("fx", C.POINTER(C.c_double)), ("stride", C.c_int64),
                ("nsamp", C.c_int64), ("xs", C.POINTER(C.c_double))]


ITER_HOOK = C.CFUNCTYPE(None, C.c_int, C.c_void_p)
ALLREDUCE = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int, C.c_void_p)
# lbfgsx_objective_fn / lbfgsx_batch_objective_fn (include/lbfgsx_solver.h)
OBJECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_double))
BATCH_OBJECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_int64,
                                 C.POINTER(C.c_double))

_core = None
_solver = None


class NativeLibraryMissing(RuntimeError):
    pass


def load():
    """Load both native libraries.  Fails loudly when they are missing: there is no fallback path."""
    global _core, _solver
    if _core is not None:
        return _core, _solver
    try:
        # When torch is (or will be) in the process its bundled HIP runtime (soname libamdhip64.so.7) must be
        # the one and only runtime, so it has to be loaded before ours resolves the same soname.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover
        pass
    p_core = os.path.join(HERE, "liblbfgsx.so")
    p_sol = os.path.join(HERE, "liblbfgsx_solver.so")
    for p in (p_core, p_sol):
        if not os.path.exists(p):
            raise NativeLibraryMissing(
                "%s not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')" % p)
    core = C.CDLL(p_core)
    sol = C.CDLL(p_sol)
    vp, i64, dbl, i32 = C.c_void_p, C.c_int64, C.c_double, C.c_int
    pd = C.POINTER(C.c_double)

    def sig(lib, name, res, *args):
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = list(args)
        return f

    sig(core, "lbfgsx_last_error", C.c_char_p)
    sig(core, "lbfgsx_version", C.c_char_p)
    sig(core, "lbfgsx_device_count", i32)
    sig(core, "lbfgsx_create", i32, C.POINTER(vp), i32, i64, i32, i32, i32)
    sig(core, "lbfgsx_destroy", None, vp)
    sig(core, "lbfgsx_set_stream", i32, vp, vp)
    sig(core, "lbfgsx_sync", i32, vp)
    sig(core, "lbfgsx_n", i64, vp)
    sig(core, "lbfgsx_vec", vp, vp, i32)
    sig(core, "lbfgsx_upload", i32, vp, i32, vp)
    sig(core, "lbfgsx_download", i32, vp, i32, vp)
    sig(core, "lbfgsx_gather", i32, vp, i32, i64, pd)
    sig(core, "lbfgsx_gen_diag_quad", i32, vp, dbl, C.c_uint64)
    sig(core, "lbfgsx_gen_rosen_x0", i32, vp, C.c_uint64)
    sig(core, "lbfgsx_fill", i32, vp, i32, dbl)
    sig(core, "lbfgsx_bfgs_reset", i32, vp)
    sig(core, "lbfgsx_bfgs_ncorr", i32, vp)
    sig(core, "lbfgsx_bfgs_theta", dbl, vp)
    sig(core, "lbfgsx_bfgs_add_correction_host", i32, vp, vp, vp)
    sig(core, "lbfgsx_bfgs_download_history", i32, vp, vp, vp, C.POINTER(i32), C.POINTER(i32), pd)
    sig(core, "lbfgsx_bfgs_download_dots", i32, vp, pd, i32)
    sig(core, "lbfgsx_apply_Hv", i32, vp, i32, dbl, pd)
    sig(core, "lbfgsx_eval", i32, vp, i32, pd, pd, pd)
    sig(core, "lbfgsx_norms", i32, vp, pd, pd)
    sig(core, "lbfgsx_ls_begin", i32, vp)
    sig(core, "lbfgsx_trial", i32, vp, i32, dbl, pd, pd)
    sig(core, "lbfgsx_trial_point", i32, vp, dbl)
    sig(core, "lbfgsx_trial_dg", i32, vp, pd)
    sig(core, "lbfgsx_ls_keep_trial_as_lo", i32, vp)
    sig(core, "lbfgsx_ls_end", i32, vp, i32)
    sig(core, "lbfgsx_post_linesearch", i32, vp, pd, pd, pd, pd)
    sig(core, "lbfgsx_commit_correction", i32, vp)
    sig(core, "lbfgsx_gs_post_linesearch", i32, vp, pd, pd, pd, pd)
    sig(core, "lbfgsx_gs_set_history_dtype", i32, vp, i32)
    sig(core, "lbfgsx_gs_direction", i32, vp, pd, dbl, pd)
    sig(core, "lbfgsx_timing_enable", i32, vp, i32)
    sig(core, "lbfgsx_timing_read", i32, vp, pd, C.POINTER(i64), pd, C.POINTER(i64))
    sig(core, "lbfgsx_stream_probe", i32, vp, i32, pd, pd)
    sig(core, "lbfgsx_selftest_reduce", i32, vp, i32, i32, i32, pd)
    sig(core, "lbfgsx_post_linesearch_spec", i32, vp, dbl, pd, pd, pd, pd)
    sig(core, "lbfgsx_rccl_allgather_records", i32, C.POINTER(i32), i32, vp, i64, i64, C.POINTER(vp))
    sig(core, "lbfgsx_device_download", i32, i32, vp, i64, vp)
    sig(core, "lbfgsx_device_free", None, i32, vp)
    sig(core, "lbfgsx_spec_counts", i32, vp, C.POINTER(i64 * 3))
    sig(core, "lbfgsx_ls_post_in_trial", i32, vp, dbl)
    sig(core, "lbfgsx_post_in_trial_counts", i32, vp, C.POINTER(i64 * 4))
    sig(core, "lbfgsx_last_in_trial_request", i32, vp, i32)
    sig(core, "lbfgsx_apply_Hv_pending", i32, vp, i32, dbl, pd, C.POINTER(i32))
    sig(core, "lbfgsx_trial_first", i32, vp, i32, dbl, pd, pd, pd)
    sig(core, "lbfgsx_last_in_trial_counts", i32, vp, C.POINTER(i64 * 4))
    sig(core, "lbfgsx_counters", i32, C.POINTER(i64 * 3), i32)
    sig(core, "lbfgsx_counters_ex", i32, C.POINTER(i64 * 8), i32)
    sig(core, "lbfgsx_poll_counts", i32, vp, C.POINTER(i64 * 2))
    sig(core, "lbfgsx_poll_counts_ex", i32, vp, C.POINTER(i64 * 4))
    sig(core, "lbfgsx_b_compact_vec_counts", i32, C.POINTER(i64 * 4), i32)
    sig(core, "lbfgsx_b_reserve", i32, vp)
    sig(core, "lbfgsx_device", i32, vp)
    sig(core, "lbfgsx_persist_counts", i32, vp, C.POINTER(i64 * 4))
    sig(core, "lbfgsx_debug_persist_fault", i32, vp)

    sig(sol, "lbfgsx_solver_create", i32, C.POINTER(vp), i32, i32, i32, C.POINTER(Params), i32)
    sig(sol, "lbfgsx_solver_create_error", C.c_char_p)
    sig(sol, "lbfgsx_solver_destroy", None, vp)
    sig(sol, "lbfgsx_solver_prepare", i32, vp, i64)
    sig(sol, "lbfgsx_solver_ctx", vp, vp)
    sig(sol, "lbfgsx_solver_set_recursion", i32, vp, i32)
    sig(sol, "lbfgsx_solver_set_direction_scale", i32, vp, dbl)
    sig(sol, "lbfgsx_solver_set_allreduce", i32, vp, ALLREDUCE, vp)
    sig(sol, "lbfgsx_solver_set_devices", i32, vp, C.POINTER(i32), i32)
    sig(core, "lbfgsx_comm_unique_id", i32, C.c_char_p)
    sig(core, "lbfgsx_comm_create_rank", i32, C.POINTER(vp), i32, i32, i32, C.c_char_p)
    sig(core, "lbfgsx_comm_create_local", i32, C.POINTER(vp), C.POINTER(i32), i32)
    sig(core, "lbfgsx_comm_allreduce_sum", i32, vp, i32, pd, i32)
    sig(core, "lbfgsx_comm_abort", i32, vp)
    sig(core, "lbfgsx_comm_abort_from", i32, vp, i32)
    sig(core, "lbfgsx_comm_first_abort", i32, vp)
    sig(core, "lbfgsx_b_gram_pairs_max", i32, vp)
    sig(core, "lbfgsx_b_post_linesearch_build", i32, vp, dbl, pd, pd, pd, pd)
    sig(core, "lbfgsx_b_post_build_counts", i32, C.POINTER(i64 * 2), i32)
    sig(core, "lbfgsx_b_psel_counts", i32, C.POINTER(i64 * 1), i32)
    sig(core, "lbfgsx_b_dg_maxstep_trial", i32, vp, i32, dbl, pd, pd)
    sig(core, "lbfgsx_b_solve_sweep_rhs", i32, vp, i32, i32, pd, dbl, pd, pd, pd, C.POINTER(i64 * 7))
    sig(core, "lbfgsx_b_solve_sweep_rhs_ready", i32, vp)
    sig(core, "lbfgsx_b_gram_last_vrow_dd", i32, vp, pd)
    sig(core, "lbfgsx_b_wtv_lu_c", i32, vp, pd, C.POINTER(i64), pd, C.POINTER(i64), pd)
    sig(core, "lbfgsx_b_trial_ahead_counts", i32, vp, C.POINTER(i64 * 2))
    sig(core, "lbfgsx_b_sub_download", i32, vp, i32, vp)
    sig(core, "lbfgsx_b_sub_upload", i32, vp, i32, vp)
    sig(core, "lbfgsx_b_lu_list_download", i32, vp, vp, i64, C.POINTER(i64))
    sig(core, "lbfgsx_b_cauchy_download", i32, vp, i32, vp)
    sig(core, "lbfgsx_comm_info", i32, vp, C.POINTER(i32 * 4))
    sig(core, "lbfgsx_comm_calls", i64, vp, i32)
    sig(core, "lbfgsx_comm_hook_arg", vp, vp, i32)
    sig(core, "lbfgsx_comm_destroy", None, vp)
    sig(core, "lbfgsx_set_shard", i32, vp, i64, i64)
    sig(sol, "lbfgsx_solver_set_iteration_hook", i32, vp, ITER_HOOK, vp)
    sig(sol, "lbfgsx_batch_minimize", i32, i32, i32, i32, C.POINTER(Params), i32, i64, i64, i64, C.c_uint64, i32, i32,
        C.POINTER(BatchItem))
    sig(sol, "lbfgsx_batch_minimize_lockstep", i32, i32, C.POINTER(Params), i64, i64, i32, C.c_uint64, i32,
        C.POINTER(BatchItem), vp, C.c_char_p, i32)
    sig(sol, "lbfgsx_batch_minimize_lockstep_multi", i32, i32, C.POINTER(Params), i64, i64, i32, C.c_uint64,
        C.POINTER(i32), i32, C.POINTER(BatchItem), vp, C.c_char_p, i32)
    sig(sol, "lbfgsx_batch_minimize_lockstep_ex", i32, i32, i32, i32, dbl, C.POINTER(Params), i64, i64, i32, C.c_uint64,
        C.POINTER(i32), i32, C.POINTER(BatchItem), vp, C.c_char_p, i32)
    sig(sol, "lbfgsx_lockstep_create", i32, C.POINTER(vp), i32, i32, C.POINTER(Params), i64, i32, i32, i32, C.c_char_p, i32)
    sig(sol, "lbfgsx_lockstep_minimize", i32, vp, i32, dbl, C.c_uint64, i64, C.POINTER(BatchItem), vp, C.POINTER(dbl * 8),
        C.c_char_p, i32)
    sig(sol, "lbfgsx_lockstep_destroy", None, vp)
    sig(sol, "lbfgsx_lockstep_set_timing", i32, vp, i32)
    sig(sol, "lbfgsx_solver_hessians", i32, vp, vp, vp)
    sig(sol, "lbfgsx_solver_stats", i32, vp, C.POINTER(C.c_longlong * 8))
    sig(sol, "lbfgsx_solver_stats2", i32, vp, C.POINTER(C.c_longlong * 8))
    sig(sol, "lbfgsx_solver_stats3", i32, vp, C.POINTER(C.c_longlong * 8))
    sig(sol, "lbfgsx_solver_minimize", i32, vp, i32, i64, vp, vp, vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    sig(sol, "lbfgsx_solver_minimize_fn", i32, vp, i64, OBJECTIVE_FN, vp, vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    sig(sol, "lbfgsx_lockstep_minimize_fn", i32, vp, vp, BATCH_OBJECTIVE_FN, vp, C.POINTER(BatchItem), vp, C.POINTER(dbl * 8),
        C.c_char_p, i32)
    # term objectives compiled at run time
    sig(core, "lbfgsx_objective_compile", i32, C.POINTER(vp), i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_destroy", None, vp)
    sig(core, "lbfgsx_objective_source", C.c_longlong, i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_info", i32, vp, C.POINTER(C.c_longlong * 8))
    sig(core, "lbfgsx_objective_compile_chain", i32, C.POINTER(vp), i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_chain", C.c_longlong, i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_form", i32, vp)
    sig(core, "lbfgsx_objective_K", i32, vp)
    sig(core, "lbfgsx_objective_dtype", i32, vp)
    sig(core, "lbfgsx_objective_bind", i32, vp, vp, C.POINTER(vp * 4), C.POINTER(dbl * 8), C.POINTER(i32))
    sig(core, "lbfgsx_objective_upload", i32, vp, i32, vp, C.POINTER(vp))
    sig(core, "lbfgsx_objective_bound", i32, vp, C.POINTER(vp * 4))
    sig(sol, "lbfgsx_solver_minimize_obj", i32, vp, vp, i64, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp, vp,
        C.POINTER(Trace), C.POINTER(Result))
    # grid objectives: the shape travels with the binding
    sig(core, "lbfgsx_objective_compile_grid", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_grid", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_grid", i32, vp, vp, i64, i64, C.POINTER(vp * 4), C.POINTER(dbl * 8), C.POINTER(i32))
    sig(core, "lbfgsx_objective_shape", i32, vp, C.POINTER(i64), C.POINTER(i64))
    sig(sol, "lbfgsx_solver_minimize_grid", i32, vp, vp, i64, i64, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp, vp,
        C.POINTER(Trace), C.POINTER(Result))
    # volume objectives: the grid's calls with one more extent
    sig(core, "lbfgsx_objective_compile_volume", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_volume", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_volume", i32, vp, vp, i64, i64, i64, C.POINTER(vp * 4), C.POINTER(dbl * 8), C.POINTER(i32))
    sig(core, "lbfgsx_objective_shape3", i32, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64))
    sig(sol, "lbfgsx_solver_minimize_volume", i32, vp, vp, i64, i64, i64, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp, vp,
        C.POINTER(Trace), C.POINTER(Result))
    # periodic grid and volume objectives: the open forms' calls with a mask after the shape
    sig(core, "lbfgsx_objective_compile_grid_periodic", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_grid_periodic", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_grid_periodic", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(core, "lbfgsx_objective_compile_volume_periodic", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_volume_periodic", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_volume_periodic", i32, vp, vp, i64, i64, i64, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(core, "lbfgsx_objective_periodic", i32, vp, C.POINTER(i32))
    sig(sol, "lbfgsx_solver_minimize_grid_periodic", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp,
        vp, C.POINTER(Trace), C.POINTER(Result))
    sig(sol, "lbfgsx_solver_minimize_volume_periodic", i32, vp, vp, i64, i64, i64, i32, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8),
        vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    # grid field objectives: the periodic grid form's calls with D at compile time
    sig(core, "lbfgsx_objective_compile_grid_field", i32, C.POINTER(vp), i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_grid_field", C.c_longlong, i32, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_grid_field", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(core, "lbfgsx_objective_D", i32, vp)
    sig(sol, "lbfgsx_solver_minimize_grid_field", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp,
        vp, C.POINTER(Trace), C.POINTER(Result))
    # grid stencil objectives: the periodic grid form's calls with a body of nine nodes
    sig(core, "lbfgsx_objective_compile_grid_stencil", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_grid_stencil", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_grid_stencil", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(sol, "lbfgsx_solver_minimize_grid_stencil", i32, vp, vp, i64, i64, i32, C.POINTER(vp * 4), i32, C.POINTER(dbl * 8), vp, vp,
        vp, C.POINTER(Trace), C.POINTER(Result))
    # graph objectives: two bodies; the edges travel with the binding
    i32p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    sig(core, "lbfgsx_objective_compile_graph", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_graph", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_graph", i32, vp, vp, i64, i32p, i32p, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(core, "lbfgsx_objective_topology", i32, vp, C.POINTER(i64), u32p, i32p, u32p)
    sig(core, "lbfgsx_objective_upload_count", i32, vp, i32, vp, i64, C.POINTER(vp))
    sig(sol, "lbfgsx_solver_minimize_graph", i32, vp, vp, i64, i64, i32p, i32p, i32, C.POINTER(vp * 4), i32, C.POINTER(i64 * 4),
        C.POINTER(dbl * 8), vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    # mesh objectives: K nodes per element, D unknowns per node; the connectivity table travels with the binding
    sig(core, "lbfgsx_objective_compile_mesh", i32, C.POINTER(vp), i32, i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_mesh", C.c_longlong, i32, i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_mesh", i32, vp, vp, i64, vp, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8), C.POINTER(i32))
    sig(core, "lbfgsx_objective_mesh_topology", i32, vp, C.POINTER(i64), u32p, u32p)
    sig(core, "lbfgsx_objective_dim", i32, vp)
    sig(sol, "lbfgsx_solver_minimize_mesh", i32, vp, vp, i64, i64, i32p, i32, C.POINTER(vp * 4), i32, C.POINTER(i64 * 4),
        C.POINTER(dbl * 8), vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    # linear-model objectives: two bodies; the CSR matrix travels with the binding
    sig(core, "lbfgsx_objective_compile_linear", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_linear", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_compile_linear_multi", i32, C.POINTER(vp), i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_linear_multi", C.c_longlong, i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_linear", i32, vp, vp, i64, i64, vp, vp, vp, i32, i32, C.POINTER(vp * 4),
        C.POINTER(dbl * 8), C.POINTER(i32))
    sig(core, "lbfgsx_objective_linear_topology", i32, vp, C.POINTER(i64 * 8), u32p, i32p, u32p, i32p, u32p, u32p)
    sig(sol, "lbfgsx_solver_minimize_linear", i32, vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, C.POINTER(vp * 4), i32,
        C.POINTER(i64 * 4), C.POINTER(dbl * 8), vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    # graph-regularised linear-model objectives: three bodies; the CSR matrix and the edges travel with the binding
    sig(core, "lbfgsx_objective_compile_linear_graph", i32, C.POINTER(vp), i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
        C.c_size_t)
    sig(core, "lbfgsx_objective_source_linear_graph", C.c_longlong, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_linear_graph", i32, vp, vp, i64, i64, vp, vp, vp, i32, i32, i64, vp, vp, i32,
        C.POINTER(vp * 4), C.POINTER(dbl * 8), C.POINTER(i32))
    sig(sol, "lbfgsx_solver_minimize_linear_graph", i32, vp, vp, i64, i64, i64, vp, vp, vp, i32, i32, i64, vp, vp, i32,
        C.POINTER(vp * 4), i32, C.POINTER(i64 * 4), C.POINTER(dbl * 8), vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    # dense linear-model objectives: the multi-output form's bodies; the dense matrix travels with the binding
    sig(core, "lbfgsx_objective_compile_dense", i32, C.POINTER(vp), i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_source_dense", C.c_longlong, i32, i32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t)
    sig(core, "lbfgsx_objective_bind_dense", i32, vp, vp, i64, vp, i64, i32, i32, C.POINTER(vp * 4), C.POINTER(dbl * 8),
        C.POINTER(i32))
    sig(core, "lbfgsx_objective_dense_info", i32, vp, C.POINTER(i64 * 8))
    sig(core, "lbfgsx_objective_dense_read", i32, vp, vp, vp, vp)
    sig(sol, "lbfgsx_solver_minimize_dense", i32, vp, vp, i64, i64, vp, i64, i32, i32, C.POINTER(vp * 4), i32,
        C.POINTER(i64 * 4), C.POINTER(dbl * 8), vp, vp, vp, C.POINTER(Trace), C.POINTER(Result))
    _core, _solver = core, sol
    return core, sol


def last_error():
    core, _ = load()
    return core.lbfgsx_last_error().decode()


_EXC = {E_INVALID: ValueError, E_LOGIC: ArithmeticError, E_RUNTIME: RuntimeError, E_HIP: RuntimeError,
        E_NOGPU: RuntimeError, E_USER: RuntimeError}


def check(rc, msg=None):
    if rc != 0:
        raise _EXC.get(rc, RuntimeError)(msg if msg is not None else last_error())


def require_torch(who):
    """torch, for the entry points that hand device memory to a Python callable as tensors."""
    try:
        import torch
    except ImportError as e:
        raise ImportError("%s needs PyTorch (ROCm build): its callable receives torch tensors that alias the library's "
                          "device vectors" % who) from e
    return torch


class _DeviceMemory:
    """Device memory the library owns, described through __cuda_array_interface__ (torch on ROCm reads it)."""

    def __init__(self, ptr, shape, np_dtype, strides):
        import numpy as np
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(np_dtype).str, "data": (int(ptr), False),
                                         "version": 2, "strides": strides}


def device_tensor(ptr, shape, np_dtype, device, row_stride=None):
    """A torch tensor that ALIASES `ptr` (no copy): shape (n,) or (rows, n) with rows `row_stride` elements apart.  The
    memory stays the library's; the tensor must not outlive the call it was made for."""
    import numpy as np
    torch = require_torch("device_tensor")
    esz = np.dtype(np_dtype).itemsize
    strides = None if row_stride is None else (int(row_stride) * esz, esz)
    return torch.as_tensor(_DeviceMemory(ptr, shape, np_dtype, strides), device=torch.device("cuda", int(device)))
