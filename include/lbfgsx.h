/* include/lbfgsx.h -- C ABI of the MI355X-native L-BFGS / L-BFGS-B hot path (liblbfgsx.so).
 *
 * The reference (yixuan/LBFGSpp) is header-only C++ with no FFI seam; the seam this library replaces is
 * the set of BFGSMat / line-search / Cauchy / SubspaceMin call sites inside its drivers:
 *   LBFGS.h:43,91-92,121-123,127,130,137,159-165      (reset, eval, copies, line search, s/y, apply_Hv)
 *   LBFGSB.h:128-138,154,174-179,203-206,235-250      (projection, proj. gradient, max step, GCP, subspace)
 * Every function below cites the reference statement(s) it executes on the device.  The drop-in C++ API
 * (include/LBFGS.h, include/LBFGSB.h: LBFGSpp::LBFGSSolver / LBFGSBSolver / LBFGSParam) keeps all scalar
 * control flow on the host and calls only this C ABI, so user code is compiled by a plain C++ compiler.
 *
 * Conventions: plain pointers and sizes only; every call returns 0 on success or a negative LBFGSX_E_* code
 * (message via lbfgsx_last_error()); scalar results are written to caller-provided doubles (values are
 * computed in the context's scalar type and widened exactly); calls are synchronous w.r.t. the returned
 * scalars but all device work is enqueued on the context's HIP stream.  A context is single-owner and bound
 * to one device; distinct contexts are independent.
 */
#ifndef LBFGSX_H
#define LBFGSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lbfgsx_ctx lbfgsx_ctx;

enum { LBFGSX_F64 = 0, LBFGSX_F32 = 1 };
enum { LBFGSX_OBJ_NONE = -1, LBFGSX_OBJ_DIAG_QUAD = 0, LBFGSX_OBJ_EXT_ROSENBROCK = 1,
       LBFGSX_OBJ_BOUND = 64 /* the term objective bound to the context (lbfgsx_objective_bind below) */ };
enum
{
    LBFGSX_OK = 0,
    LBFGSX_E_INVALID = -1, /* -> std::invalid_argument */
    LBFGSX_E_LOGIC = -2,   /* -> std::logic_error */
    LBFGSX_E_RUNTIME = -3, /* -> std::runtime_error */
    LBFGSX_E_HIP = -4,     /* HIP runtime failure (message holds hipGetErrorString) */
    LBFGSX_E_NOGPU = -5,   /* no usable device: the product never falls back to a CPU path */
    LBFGSX_E_USER = -6     /* a caller-supplied objective callback returned non-zero (include/lbfgsx_solver.h) */
};
/* flags for lbfgsx_create */
enum { LBFGSX_FLAG_BOUNDED = 1 /* allocate the L-BFGS-B work set (lb, ub, xcp, masks, sort buffers) */ };

/* named device vectors of a context (length n, element type = context dtype) */
enum
{
    LBFGSX_VEC_X = 0,     /* current iterate (after a line search: the accepted point)          */
    LBFGSX_VEC_G = 1,     /* gradient at X                                                       */
    LBFGSX_VEC_XP = 2,    /* iterate at the start of the line search (m_xp, LBFGS.h:121)         */
    LBFGSX_VEC_GP = 3,    /* gradient at XP (m_gradp, LBFGS.h:122)                               */
    LBFGSX_VEC_D = 4,     /* search direction (m_drt)                                            */
    LBFGSX_VEC_XT = 5,    /* line-search trial point                                             */
    LBFGSX_VEC_GT = 6,    /* gradient at the trial point                                         */
    LBFGSX_VEC_A = 7,     /* objective data (diag quadratic: a)                                  */
    LBFGSX_VEC_B = 8,     /* objective data (diag quadratic: b)                                  */
    LBFGSX_VEC_LB = 9,    /* lower bounds (BOUNDED contexts)                                     */
    LBFGSX_VEC_UB = 10,   /* upper bounds                                                        */
    LBFGSX_VEC_XCP = 11   /* generalized Cauchy point                                            */
};

const char* lbfgsx_last_error(void);
const char* lbfgsx_version(void);
int lbfgsx_device_count(void);

/* ---- context ---------------------------------------------------------------------------------------
 * replaces LBFGSSolver::reset / BFGSMat::reset (LBFGS.h:40-50, BFGSMat.h:61-78): allocates x/g work
 * vectors and the (m+1)-column S and Y stores (column-contiguous, column stride padded to 64 elements). */
int lbfgsx_create(lbfgsx_ctx** out, int dtype, int64_t n, int m, int device, int flags);
void lbfgsx_destroy(lbfgsx_ctx* c);
int lbfgsx_set_stream(lbfgsx_ctx* c, void* hip_stream); /* adopt an external hipStream_t (e.g. torch's) */
int lbfgsx_sync(lbfgsx_ctx* c);
int64_t lbfgsx_n(const lbfgsx_ctx* c);
/* device pointer of a named vector (valid until the next call that rotates buffers) */
void* lbfgsx_vec(lbfgsx_ctx* c, int which);
int lbfgsx_upload(lbfgsx_ctx* c, int which, const void* host);   /* host -> device, n elements */
int lbfgsx_download(lbfgsx_ctx* c, int which, void* host);       /* device -> host, n elements */
int lbfgsx_gather(lbfgsx_ctx* c, int which, int64_t stride, double* host); /* host[k] = vec[k*stride] */

/* ---- synthetic problems generated on the device from a counter hash */
/* This context holds rows [offset, offset + n) of a problem of n_global rows (row-sharded runs, include/LBFGS.h
 * set_reducer): the generators below then produce exactly that slice of the unsharded data.  Default: 0, n. */
int lbfgsx_set_shard(lbfgsx_ctx* c, int64_t offset, int64_t n_global);
int lbfgsx_gen_diag_quad(lbfgsx_ctx* c, double kappa, uint64_t seed); /* fills A, B */
int lbfgsx_gen_rosen_x0(lbfgsx_ctx* c, uint64_t seed);                /* fills X    */
int lbfgsx_fill(lbfgsx_ctx* c, int which, double value);

/* ---- BFGSMat ----------------------------------------------------------------------------------------*/
/* BFGSMat::reset (BFGSMat.h:61-78): theta = 1, ncorr = 0, ptr = m */
int lbfgsx_bfgs_reset(lbfgsx_ctx* c);
int lbfgsx_bfgs_ncorr(const lbfgsx_ctx* c);
double lbfgsx_bfgs_theta(const lbfgsx_ctx* c);
/* BFGSMat::add_correction (BFGSMat.h:81-97) from host-provided s, y (testing / generic callers) */
int lbfgsx_bfgs_add_correction_host(lbfgsx_ctx* c, const void* s, const void* y);
/* same, but only stages the pair in the spare column (s.y and y.y returned); lbfgsx_commit_correction adds it */
int lbfgsx_bfgs_stage_correction_host(lbfgsx_ctx* c, const void* s, const void* y, double* sy, double* yy);
/* storage-slot order copy of the history for the dense debugging getters (BFGSMat::get_Bmat / get_Hmat,
 * BFGSMat.h:150-271): S_out, Y_out receive ncorr columns of n elements (column j = storage slot j); ptr as in
 * BFGSMat.h:42-48.  Meant for small n only. */
int lbfgsx_bfgs_download_history(lbfgsx_ctx* c, void* S_out, void* Y_out, int* ncorr, int* ptr, double* theta);
/* BFGSMat::apply_Hv (BFGSMat.h:276-302): D = a * H * v where v is a named vector; also returns
 * dg = v . D fused into the last pass: G . D when v == LBFGSX_VEC_G (LBFGS.h:123 of the next iteration).  For any other
 * vector it is the dot with that vector, in the step launches and in the persistent launch alike. */
int lbfgsx_apply_Hv(lbfgsx_ctx* c, int v_which, double a, double* dg);
/* inspection entry: the dots of the recursion as the last product left them, out[k] = sc[dot(k)] widened to double, k < count
 * (1 <= count <= 2m + 1).  With c pairs stored a product leaves 2c + 1 of them: out[i] = s_i . q of the first loop (i < c,
 * columns newest -> oldest, BFGSMat.h:288), out[c + t] = y_i . q of the second loop (t < c, i = c-1-t, :298) and out[2c] = v . D.
 * Every form stores them: the step launches, the persistent launch, the fused post form (out[0] by its step 0) and the launch
 * from the gradient (out[0] by the post-form trial before it).  The call reads; it settles no step that is still owed and
 * invalidates nothing.  A launch that ended one step early (lbfgsx_last_in_trial_request below) leaves out[2c] unset -- the
 * slot keeps what an earlier product stored there -- until the step has run: a step launch (lbfgsx_download, lbfgsx_vec, a
 * second trial, ...) stores it there, and so does a first trial that forms the step in its own pass (lbfgsx_trial_first),
 * besides returning it in *dg_init.  Every post-form trial (lbfgsx_ls_post_in_trial) rewrites out[0]: it holds the first dot
 * of the NEXT product from then on; out[1 .. 2c] stay the last product's until the next launch. */
int lbfgsx_bfgs_download_dots(lbfgsx_ctx* c, double* out, int count);

/* ---- L-BFGS driver statements ------------------------------------------------------------------------*/
/* fx = f(x, grad); gnorm = grad.norm(); x.norm()   (LBFGS.h:91-92,100) with a built-in objective */
int lbfgsx_eval(lbfgsx_ctx* c, int objective, double* fx, double* gnorm2, double* xnorm2);
/* reductions only, for user (device-functor) objectives that filled G themselves */
int lbfgsx_norms(lbfgsx_ctx* c, double* gnorm2, double* xnorm2);
/* xp = x; gradp = grad (LBFGS.h:121-122) by buffer rotation; x_lo/grad_lo alias them
 * (LineSearchMoreThuente.h:393, LineSearchNocedalWright.h:128) */
int lbfgsx_ls_begin(lbfgsx_ctx* c);
/* x = xp + step*drt; fx = f(x, grad); dg = grad.dot(drt)
 * (LineSearchMoreThuente.h:412-414; LineSearchNocedalWright.h:146-148,219-221) */
int lbfgsx_trial(lbfgsx_ctx* c, int objective, double step, double* fx, double* dg);
/* device-functor path: XT = xp + step*drt only; then the caller fills GT; then lbfgsx_trial_dg */
int lbfgsx_trial_point(lbfgsx_ctx* c, double step);
int lbfgsx_trial_dg(lbfgsx_ctx* c, double* dg);
/* x_lo.swap(x); grad_lo.swap(grad)  (LineSearchMoreThuente.h:534-535,553-554; NocedalWright.h:172-173,254-255) */
int lbfgsx_ls_keep_trial_as_lo(lbfgsx_ctx* c);
/* end of the search: the accepted point is the last trial (use_lo = 0) or the saved _lo point
 * (use_lo = 1: LineSearchMoreThuente.h:612-613, NocedalWright.h:191-192,274-275) */
int lbfgsx_ls_end(lbfgsx_ctx* c, int use_lo);
/* gnorm, x.norm(), s = x - xp, y = grad - gradp, s.y, y.y  (LBFGS.h:130,137,159-161) in one pass;
 * s and y land in the spare history column */
int lbfgsx_post_linesearch(lbfgsx_ctx* c, double* gnorm2, double* xnorm2, double* sy, double* yy);
/* BFGSMat::add_correction of the pair just formed (BFGSMat.h:81-97): index rotation only */
int lbfgsx_commit_correction(lbfgsx_ctx* c);
/* lbfgsx_post_linesearch with the next statement of the driver folded in when the pair turns out usable:
 *     s, y, the four sums (LBFGS.h:130,137,159-161)   and, speculatively,   drt = a * H * grad  (LBFGS.h:165)
 * for the history "stored pairs + the pair just formed" -- as step 0 and steps 1..2c of ONE persistent launch: the first
 * step of the recursion needs exactly grad and the new s, which the post pass holds in registers (2n elements fewer per
 * iteration, one launch less).  The kernel applies the driver's test s.y > eps y.y (LBFGS.h:161) itself and stops after
 * the post statements when it fails.  The caller proceeds exactly as after lbfgsx_post_linesearch: convergence tests,
 * lbfgsx_commit_correction if the pair is accepted, lbfgsx_apply_Hv(LBFGSX_VEC_G, a) -- which returns the direction
 * already computed when the speculation applies (same history, same gradient, same a) and computes it otherwise.
 * Falls back to lbfgsx_post_linesearch when the persistent kernel is unavailable (LBFGSX_PERSIST=0, LBFGSX_FUSE_POST=0,
 * m > 128, another persistent launch in flight on the device).  Bit-identical results either way. */
int lbfgsx_post_linesearch_spec(lbfgsx_ctx* c, double a, double* gnorm2, double* xnorm2, double* sy, double* yy);
/* instrumentation: {fused launches, directions taken over by lbfgsx_apply_Hv, pairs rejected by the kernel} */
int lbfgsx_spec_counts(const lbfgsx_ctx* c, int64_t out[3]);
/* Post form of the first trial.  To be called right after lbfgsx_ls_begin by a driver that will run
 * lbfgsx_post_linesearch_spec(c, a, ...) after the search (include/LBFGS.h with the vector recursion and no reducer).  The
 * search's first lbfgsx_trial may then run the statements that follow an accepted search in its own pass: s = x - xp and
 * y = grad - gradp into the spare history column, g.g, x.x, s.y, y.y (LBFGS.h:130,137,159-161) and the first dot of the
 * recursion on the new gradient, s.(a grad) (BFGSMat.h:283-288) -- 7n elements instead of the trial's 4n, and when that
 * trial is accepted lbfgsx_post_linesearch_spec returns its sums without a pass of its own and launches the recursion from
 * the gradient (no step 0: 11.0n instead of 14.6n elements around an accepted first trial at n = 1e8, m = 10).  A rejected
 * first trial has moved 3n elements for nothing, so the context uses the form only when the previous search accepted its
 * first trial, the history is non-empty, the objective goes through k_trial (a built-in one or a bound term objective; the
 * chain, grid, graph, mesh and linear-model objectives keep the plain form) and the context is not a row shard; a search
 * whose post-form trial is rejected goes on with plain trials and today's fused launch.  Same statements on the same
 * operands: bit-identical results.  LBFGSX_POST_IN_TRIAL=0 (read when the context is created) switches the form off. */
int lbfgsx_ls_post_in_trial(lbfgsx_ctx* c, double a);
/* instrumentation: {post-form trials issued, of which accepted, persistent launches that started from the gradient,
 * 1 if the form is enabled for this context} */
int lbfgsx_post_in_trial_counts(const lbfgsx_ctx* c, int64_t out[4]);
/* Last step of the recursion in the first trial.  After an accepted post-form first trial the product's persistent launch
 * writes d, and the next search's first trial -- a post-form one again -- reads it straight back, along with the gradient the
 * last step has just reduced against.  A driver that can do without grad.d until its first trial has come back says so once
 * per context with lbfgsx_last_in_trial_request(c, 1).  The launch that lbfgsx_post_linesearch_spec starts from the gradient
 * then ends with step 2c-1, and
 *   lbfgsx_apply_Hv_pending  is lbfgsx_apply_Hv, except that with *pending = 1 it returns no grad.d (NaN): D holds the vector
 *                            before the last update;
 *   lbfgsx_trial_first       is lbfgsx_trial, except that a first post-form trial of a built-in objective forms
 *                            d = q + (alpha_0 - beta) s_0 (BFGSMat.h:298-299) in its own pass, without storing it, and returns
 *                            *dg_init = grad.d with fx and dg: 8.12n instead of 10.88n elements around that kernel boundary
 *                            at n = 1e8.  *dg_init is NaN when no step was pending.
 * The caller checks the sign of dg_init itself (the reference does so before its first trial; the trial has then written
 * only the trial buffer).  Every other entry point that reads D or replaces a vector the step reads -- lbfgsx_download,
 * lbfgsx_vec, lbfgsx_trial, the second trial of a search, lbfgsx_apply_Hv, ... -- first runs the step as the step launches have
 * it (k_twoloop), which leaves D and grad.d as the full launch does: same bits either way.  Only the built-in objectives
 * have the form; a bounded context never defers.  LBFGSX_LAST_IN_TRIAL=0 (read when the context is created) switches it off. */
int lbfgsx_last_in_trial_request(lbfgsx_ctx* c, int on);
int lbfgsx_apply_Hv_pending(lbfgsx_ctx* c, int v_which, double a, double* dg, int* pending);
int lbfgsx_trial_first(lbfgsx_ctx* c, int objective, double step, double* fx, double* dg, double* dg_init);
/* instrumentation: {launches that ended one step early, steps run by a first trial, steps run on their own ahead of another
 * reader of D, 1 if the form is enabled for this context} */
int lbfgsx_last_in_trial_counts(const lbfgsx_ctx* c, int64_t out[4]);
/* ---- term objectives compiled at run time -------------------------------------------------------------------------
 * An objective that is a sum of terms over K consecutive coordinates (K = 1 or 2), evaluated INSIDE the fused kernels like
 * the two built-in ones.  `body` is HIP/C++ text for one term: statements that see
 *     T (the scalar type), const T x[K], T g[K] (to fill), int64_t i (index of x[0]),
 *     const T* p0..p3 (per-coordinate data arrays of n elements, device memory of the caller), T c[8] (scalars)
 * and return the term's value; f is the sum of the returned values (the order-independent sum of the built-in objectives).
 * No shared memory, no synchronisation, no other coordinates, no inline assembly.  The library wraps the body into the
 * objective struct the kernel templates take, compiles k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial for it with
 * hipRTC for gfx950 (-O3 -ffp-contract=off: the build's own floating-point contract, no device needed), and caches the
 * result per process by (form, body, K, dtype); "chain objectives" below are the other form.  A body that does not compile:
 * LBFGSX_E_INVALID, the compiler's log in `log`
 * (line numbers count from the first line of the body, file name "objective_body").
 * lbfgsx_objective_source: the generated translation unit (returns the length needed, text truncated to len).
 * lbfgsx_objective_info: out = {VGPRs (largest of the four kernels), scratch bytes (largest), 1 if this handle was served
 * from the cache, compile time in ms, scratch bytes of k_eval, k_trial, k_b_eval, k_b_dg_maxstep_trial}, read from the
 * code object.
 * lbfgsx_objective_bind: loads the code object on the context's device (once per device) and binds the objective with its
 * data arrays p[0..3] (device pointers; NULL = unused) and scalars c[0..7] to the context; n must be a multiple of K.  *id
 * receives LBFGSX_OBJ_BOUND, the value that lbfgsx_eval, lbfgsx_trial, lbfgsx_b_eval and lbfgsx_b_dg_maxstep_trial then take
 * for `objective`; they launch the loaded kernels with the grid, arguments and workspace of the built-in launch.  obj = NULL
 * unbinds.  The binding holds the cached code, not the handle: the handle may be destroyed while bound.
 * lbfgsx_objective_upload copies a host array of n elements into a buffer the context owns for `slot` and returns its device
 * address in *dev, to be passed to lbfgsx_objective_bind like any other device array.
 * A body that contains the word asm is refused (LBFGSX_E_INVALID): inline assembly is not part of the contract.
 * Lifetime: a compiled (body, K, dtype) and the modules loaded from it stay until the process ends -- there is no eviction,
 * so a program that generates bodies without bound grows by a code object (tens of KB) and a module per body.
 * LBFGSX_KERNEL_DIR (environment): the directory of lbfgs_kernels.cuh / lbfgsb_kernels.cuh / reduce.cuh for a library that
 * was installed apart from them; by default csrc/ next to the library.
 * lbfgsx_objective_bound: the four data pointers currently bound.  No reference counterpart (the reference's objectives
 * are host functors). */
typedef struct lbfgsx_objective lbfgsx_objective;
int lbfgsx_objective_compile(lbfgsx_objective** out, int dtype, int K, const char* body, char* log, size_t log_len);
void lbfgsx_objective_destroy(lbfgsx_objective* obj);
long long lbfgsx_objective_source(int dtype, int K, const char* body, char* out, size_t len);
int lbfgsx_objective_info(const lbfgsx_objective* obj, long long out[8]);
int lbfgsx_objective_K(const lbfgsx_objective* obj);
int lbfgsx_objective_dtype(const lbfgsx_objective* obj);
int lbfgsx_objective_bind(lbfgsx_ctx* c, const lbfgsx_objective* obj, const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_upload(lbfgsx_ctx* c, int slot, const void* host, void** dev);
int lbfgsx_objective_bound(const lbfgsx_ctx* c, const void* p[4]);
/* ---- chain objectives: overlapping terms ------------------------------------------------------------------------------
 * f(x) = sum over t = 0 .. n-K of phi(x[t], .., x[t+K-1]; t) with K = 2 or 3: ONE TERM STARTS AT EVERY COORDINATE, so
 * neighbouring terms overlap -- the chained Rosenbrock function, first- and second-difference regularisers, any nearest-
 * neighbour energy.  `body` is what a term objective's is: it sees T, const T x[K], T g[K] (the term's K partial derivatives,
 * to fill), int64_t i (the index of x[0]), p0..p3, c[8] and returns the term's value.  It may read p0[i] .. p0[i+K-1]: a term
 * that does not lie inside [0, n) is never evaluated.
 * Semantics (a numpy restatement with one operation per source operation is bit-exact):
 *   grad[j] = the sum of g_t[j-t] over the terms t = max(0, j-K+1) .. min(j, n-K), in ascending t, started from the first
 *             contribution (no leading 0 +);
 *   f       = the order-independent (compensated) sum of the terms' values, each added once, by the thread that owns the
 *             coordinate the term starts at;
 *   one rounding per source operation, no contraction.
 * lbfgsx_objective_compile_chain wraps the body for the four kernels of csrc/chain_kernels.cuh -- the counterparts of k_eval,
 * k_trial, k_b_eval and k_b_dg_maxstep_trial with the same arguments, grids, tiles and reductions, so the byte model is the
 * built-in's (the halo of a pack comes from the neighbouring lanes) -- and caches by (form, body, K, dtype): the same body as
 * a term objective and as a chain objective are two entries.  K outside {2, 3}: LBFGSX_E_INVALID.  The handle carries its
 * form (lbfgsx_objective_form: LBFGSX_FORM_TERM or LBFGSX_FORM_CHAIN); lbfgsx_objective_bind, lbfgsx_objective_info,
 * lbfgsx_solver_minimize_obj and the four evaluation entry points take it like a term objective's.  Binding to a context
 * with n < K is refused (any n >= K is accepted: n need not be a multiple of anything).  The compile log, the refusal of
 * asm and the line numbers are those of lbfgsx_objective_compile. */
enum { LBFGSX_FORM_TERM = 0, LBFGSX_FORM_CHAIN = 1, LBFGSX_FORM_GRID = 2, LBFGSX_FORM_GRAPH = 3, LBFGSX_FORM_MESH = 4, LBFGSX_FORM_LINEAR = 5,
       LBFGSX_FORM_LINEAR_MULTI = 6, LBFGSX_FORM_DENSE = 7, LBFGSX_FORM_LINEAR_GRAPH = 8, LBFGSX_FORM_VOLUME = 9,
       LBFGSX_FORM_GRID_PERIODIC = 10, LBFGSX_FORM_VOLUME_PERIODIC = 11, LBFGSX_FORM_GRID_FIELD = 12,
       LBFGSX_FORM_GRID_STENCIL = 13 };
int lbfgsx_objective_compile_chain(lbfgsx_objective** out, int dtype, int K, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_chain(int dtype, int K, const char* body, char* out, size_t len);
int lbfgsx_objective_form(const lbfgsx_objective* obj);
/* ---- grid objectives: 2x2-cell terms on a row-major grid ----------------------------------------------------------------
 * x is a row-major rows x cols array, n = rows*cols, rows >= 2, cols >= 2, and
 *     f(x) = sum over cells (r, c), 0 <= r < rows-1, 0 <= c < cols-1, of phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c)
 * -- the MINPACK-2 energies (a cell covers both triangles of their discretisation), smoothness terms of image problems,
 * membrane and Allen-Cahn energies.  `body` is the text of ONE CELL: it sees T, const T x[4] in the order above, T g[4] (the
 * cell's four partial derivatives, to fill), int64_t i (the flat index of x[0], row*cols + col), int64_t row, col, rows, cols,
 * p0..p3 and c[8], and returns the cell's value.  It may read p0[i], p0[i+1], p0[i+cols] and p0[i+cols+1]: a cell that does
 * not exist is never evaluated.  A per-node term (a data-fidelity term, say) is written inside the body: node (row, col)
 * goes to the cell that starts there, and the cells of the last row and column of cells pick up the nodes nobody starts at,
 *     T v = ...cell...;  v += node(x[0], i);                      if (col + 2 == cols) v += node(x[1], i + 1);
 *     if (row + 2 == rows) { v += node(x[2], i + cols);           if (col + 2 == cols) v += node(x[3], i + cols + 1); }
 * with the matching additions to g[0..3].
 * Semantics (a numpy restatement with one operation per source operation is bit-exact):
 *   grad[r,c] = g[3] of cell (r-1, c-1) + g[2] of cell (r-1, c) + g[1] of cell (r, c-1) + g[0] of cell (r, c): the cells that
 *               exist, in this order (ascending flat index of the cell's origin), started from the first (no leading 0 +);
 *   f         = the order-independent (compensated) sum of the cells' values, each added once, by the thread that owns the
 *               cell's origin;
 *   one rounding per source operation, no contraction.
 * lbfgsx_objective_compile_grid wraps the body for the four kernels of csrc/grid_kernels.cuh -- the counterparts of k_eval,
 * k_trial, k_b_eval and k_b_dg_maxstep_trial with the same arguments, grids and reductions; the rows above and below a
 * thread's pack are re-read through the caches -- and caches by (form, body, K, dtype) with K = 4 (lbfgsx_objective_K).  The
 * handle's form is LBFGSX_FORM_GRID.  lbfgsx_objective_bind_grid binds it with the grid's shape; it refuses (LBFGSX_E_INVALID,
 * the values named) a handle of another form, rows < 2, cols < 2 and rows*cols != n.  lbfgsx_objective_bind refuses a grid
 * handle.  lbfgsx_objective_shape reads the bound shape back.  lbfgsx_objective_info, lbfgsx_objective_upload and the four
 * evaluation entry points take it like a term objective's; the compile log, the refusal of asm and the line numbers are
 * those of lbfgsx_objective_compile. */
int lbfgsx_objective_compile_grid(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_grid(int dtype, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_grid(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, const void* const p[4],
                               const double cs[8], int* id);
int lbfgsx_objective_shape(const lbfgsx_ctx* c, int64_t* rows, int64_t* cols);
/* ---- volume objectives: 2x2x2-cell terms on a slab-major 3-D array --------------------------------------------------------
 * x is a slab-major slabs x rows x cols array, n = slabs*rows*cols, all three extents >= 2; node (s, r, c) has flat index
 * (s*rows + r)*cols + c, and
 *     f(x) = sum over cells (s, r, c), 0 <= s < slabs-1, 0 <= r < rows-1, 0 <= c < cols-1, of phi(x[8]; s, r, c),
 *     x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc]              (slots 0..3 are the grid form's, on slab s)
 * -- volumetric denoising and deblurring, 3-D phase-field and Allen-Cahn energies, tomographic volumes, minimal-surface and
 * obstacle problems in 3-D.  `body` is the text of ONE CELL: it sees T, const T x[8] in the order above, T g[8] (the cell's
 * eight partial derivatives, to fill), int64_t i (the flat index of x[0]), int64_t slab, row, col, slabs, rows, cols, p0..p3
 * and c[8], and returns the cell's value.  It may read p0 at the eight corners, p0[i + dc + dr*cols + ds*rows*cols]: a cell
 * that does not exist is never evaluated, and no index outside [0, n) is loaded.  A per-node term is written inside the
 * body as for a grid: node (slab, row, col) goes to the cell that starts there, and the last layer of cells in each direction
 * picks up the nodes no cell starts at -- corner (ds, dr, dc) of a cell is added by it iff
 *     (ds == 0 || slab + 2 == slabs) && (dr == 0 || row + 2 == rows) && (dc == 0 || col + 2 == cols),
 *     e.g.  v += node(x[0], i);   if (col + 2 == cols) v += node(x[1], i + 1);
 *           if (slab + 2 == slabs && row + 2 == rows) v += node(x[6], i + (rows + 1)*cols);   ...
 * with the matching additions to g[0..7]: every node is then counted exactly once.
 * Semantics (a numpy restatement with one operation per source operation is bit-exact):
 *   grad[s,r,c] = g[7] of cell (s-1, r-1, c-1) + g[6] of (s-1, r-1, c) + g[5] of (s-1, r, c-1) + g[4] of (s-1, r, c) +
 *                 g[3] of (s, r-1, c-1) + g[2] of (s, r-1, c) + g[1] of (s, r, c-1) + g[0] of (s, r, c): the cells that exist,
 *                 in this order (ascending flat index of the cell's origin), started from the first (no leading 0 +);
 *   f           = the order-independent (compensated) sum of the cells' values, each added once, by the thread that owns the
 *                 cell's origin;
 *   one rounding per source operation, no contraction, no floating-point atomic.
 * lbfgsx_objective_compile_volume wraps the body for the four kernels of csrc/volume_kernels.cuh -- the counterparts of
 * k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial with the same arguments, grids and reductions; the eight packs a row
 * or a slab away from a thread's pack are re-read through the caches, and the form adds nothing to the byte model -- and
 * caches by (form, body, K, dtype) with K = 8: the same text as a grid and as a volume objective are two entries, and the
 * shape is not part of the key.  The handle's form is LBFGSX_FORM_VOLUME.  lbfgsx_objective_bind_volume binds it with the
 * shape; it refuses (LBFGSX_E_INVALID, the values named) a handle of another form, an extent < 2, and a product that is not
 * n or overflows.  lbfgsx_objective_bind and lbfgsx_objective_bind_grid refuse a volume handle.  lbfgsx_objective_shape3
 * reads the bound shape back (lbfgsx_objective_shape speaks of grid objectives only).  lbfgsx_objective_info,
 * lbfgsx_objective_upload and the four evaluation entry points take it like a term objective's; the compile log, the refusal
 * of asm and the line numbers are those of lbfgsx_objective_compile. */
int lbfgsx_objective_compile_volume(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_volume(int dtype, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_volume(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                 const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_shape3(const lbfgsx_ctx* c, int64_t* slabs, int64_t* rows, int64_t* cols);
/* ---- periodic grid and volume objectives: wrap-around cells --------------------------------------------------------------
 * The grid and the volume form with periodic boundaries in the directions of a mask `periodic`: bit 0 the column direction,
 * bit 1 the row direction, bit 2 (a volume only) the slab direction -- Allen-Cahn, Cahn-Hilliard and phase-field energies on a
 * torus, XY, rotor and Ginzburg-Landau lattices, micromagnetic boxes, channels and cylinders (periodic in one direction,
 * walled in the other), circular-convolution image models.
 *   Periodic grid.  x is a row-major rows x cols array, n = rows*cols, rows >= 2, cols >= 2.  Cell (r, c) has the corners
 *     x[r, c], x[r, c(+)1], x[r(+)1, c], x[r(+)1, c(+)1] in the grid form's slot order, (+) modulo the extent, and exists iff
 *     (c < cols-1 or bit 0) and (r < rows-1 or bit 1).  With the mask 0 this is exactly the grid form.
 *     grad[r,c] = g[3] of cell (r(-)1, c(-)1) + g[2] of (r(-)1, c) + g[1] of (r, c(-)1) + g[0] of (r, c): the cells that exist, in
 *     this fixed order, started from the first (no leading 0 +); on a periodic axis (-) wraps, on an open axis a negative index
 *     means the cell does not exist.  Away from the seams this is the grid form's order; on a torus it is translation-invariant.
 *   Periodic volume.  The same on the slab-major slabs x rows x cols array, eight corners in the volume form's slot order,
 *     x[4*ds + 2*dr + dc] = x[s(+)ds, r(+)dr, c(+)dc], and the volume form's order of the eight cells of a node with wrapped
 *     indices.
 *   f = the order-independent (compensated) sum of the existing cells' values, each added once, by the owner of the cell's
 *     origin.  One rounding per source operation, no contraction, no floating-point atomic.  In the trial kernels every corner
 *     value is xp + step*d, never a read of the x the launch writes.
 * `body` sees what the grid or the volume body sees, plus const int64_t j[4] (j[8] for a volume), the flat indices of its
 * corners with j[0] == i, and int periodic.  It may read p0[j[k]]; the i + 1 and i + cols arithmetic of the open forms is
 * wrong at a seam.  A per-node term goes to the cell that starts at the node; on an open axis the last layer of cells picks
 * up the nodes no cell starts at, as described above, and on a periodic axis there is nothing to pick up:
 *     if (!(periodic & 1) && col + 2 == cols) v += node(x[1], j[1]);
 * lbfgsx_objective_compile_grid_periodic and _volume_periodic wrap the body for the four kernels of
 * csrc/periodic_grid_kernels.cuh and csrc/periodic_volume_kernels.cuh (same arguments, grids and reductions as the open
 * forms') and cache by (form, body, K, dtype): the shape and the mask are not part of the key.  The forms are
 * LBFGSX_FORM_GRID_PERIODIC and LBFGSX_FORM_VOLUME_PERIODIC.  The bind calls refuse (LBFGSX_E_INVALID, the values named) a
 * handle of another form, an extent < 2, a product that is not n or overflows, and a mask with bits outside the form's
 * directions; every other bind call refuses these handles.  lbfgsx_objective_shape and lbfgsx_objective_shape3 read the
 * bound shape back, lbfgsx_objective_periodic the bound mask. */
int lbfgsx_objective_compile_grid_periodic(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_grid_periodic(int dtype, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_grid_periodic(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                        const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_compile_volume_periodic(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_volume_periodic(int dtype, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_volume_periodic(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                          int periodic, const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_periodic(const lbfgsx_ctx* c, int* mask);
/* ---- grid field objectives: D unknowns per node of a grid ---------------------------------------------------------------------
 * The periodic grid form with nodes that carry D = 1, 2 or 3 unknowns: complex Ginzburg-Landau lattices (2), micromagnetic and
 * Heisenberg films (3), optical flow and 2-D elasticity (2), colour and multi-channel image models with vectorial TV (3),
 * multi-phase fields.
 *   Layout.  x is node-major, as for a mesh objective: x[(r*cols + c)*D + d] is unknown d of node (r, c); n = rows*cols*D,
 *     rows >= 2, cols >= 2.
 *   Mask.  `periodic` is the periodic grid form's: bit 0 the column direction, bit 1 the row direction, 0 = open.  Cell
 *     existence and the wrapped corners are exactly those of "periodic grid and volume objectives" above.
 *   Body.  The text of one cell; the generated method is
 *       T term(const T (&x)[4 * D], T (&g)[4 * D], int64_t i, int64_t row, int64_t col, const int64_t (&j)[4]) const
 *     x and g are slot-major like the mesh form's: x[k*D + d] is unknown d of corner k, in the grid form's corner order.  i is
 *     the NODE index of corner 0 and j[k] are the node indices of the corners, j[0] == i; the flat coordinate of unknown d of
 *     corner k is j[k]*D + d (data per coordinate: p0[j[k]*D + d]; data per node: p0[j[k]]).  The body also sees constexpr int D,
 *     rows, cols, periodic, p0..p3 and c[8].  At D = 1 this is the periodic grid form's signature: one text compiles in both.
 *   Gradient.  For every d, grad[(r,c), d] = g[3*D+d] of cell (r(-)1, c(-)1) + g[2*D+d] of (r(-)1, c) + g[D+d] of (r, c(-)1) +
 *     g[d] of (r, c): the cells that exist, in this fixed order, started from the first (no leading 0 +); (-) wraps on a
 *     periodic axis.
 *   f = the order-independent (compensated) sum of the existing cells' values, each added once, by the owner of the cell's
 *     origin.  One rounding per source operation, no contraction, no floating-point atomic.  In the trial kernels every corner
 *     value is xp + step*d, never a read of the x the launch writes.  No index outside [0, n) is loaded.
 * lbfgsx_objective_compile_grid_field wraps the body for the four kernels of csrc/grid_field_kernels.cuh (same arguments, grids
 * and reductions as the periodic grid form's; a thread owns W = 16/sizeof(T) nodes, D aligned 16-byte packs) and caches by
 * (form, body, dtype, D): the shape and the mask are not part of the key.  The form is LBFGSX_FORM_GRID_FIELD.  D outside
 * 1 .. 3 is refused ("D = # is not supported: a node has D = 1, 2 or 3 unknowns").  lbfgsx_objective_bind_grid_field refuses
 * (LBFGSX_E_INVALID, the values named) a handle of another form, an extent < 2, rows*cols*D that is not n or overflows, and a
 * mask with bits above 3; every other bind call refuses this handle, lbfgsx_objective_bind saying that it is bound with its
 * shape, mask and D.  lbfgsx_objective_shape and lbfgsx_objective_periodic read the bound shape and mask back,
 * lbfgsx_objective_D the handle's D; lbfgsx_objective_K is 4. */
int lbfgsx_objective_compile_grid_field(lbfgsx_objective** out, int dtype, int D, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_grid_field(int dtype, int D, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_grid_field(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                     const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_D(const lbfgsx_objective* obj);
/* ---- grid stencil objectives: 3x3-node terms on a row-major grid ------------------------------------------------------------
 * One term per 3x3 block of nodes, open or periodic per direction: energies that need a second difference at a node -- plate
 * bending and thin-plate splines, sum (Laplace u)^2 and the Hessian-Frobenius norm with its u_xy term, Swift-Hohenberg and
 * phase-field-crystal functionals, second-order TV and TGV-type image priors, 3x3 clique priors (Fields of Experts), Willmore
 * and Helfrich energies in the Monge gauge, anything on a 9-point stencil.
 *   Layout.  x is a row-major rows x cols array, n = rows*cols, rows >= 3 and cols >= 3, so that the three nodes of a patch
 *     along an axis are distinct on a periodic axis too.
 *   Mask.  `periodic` is the periodic grid form's: bit 0 the column direction, bit 1 the row direction, 0 = open.
 *   Patch.  Patch (r, c) has the nodes x[3*dr + dc] = x[r(+)dr, c(+)dc], dr, dc in {0, 1, 2}, (+) modulo the extent; its centre
 *     is slot 4.  It exists iff (c < cols-2 or bit 0) and (r < rows-2 or bit 1).
 *   Body.  The text of one patch; the generated method is
 *       T term(const T (&x)[9], T (&g)[9], int64_t i, int64_t row, int64_t col, const int64_t (&j)[9]) const
 *     i, row and col are those of slot 0; j[k] are the flat indices of the nine nodes, j[0] == i.  The body also sees rows, cols,
 *     periodic, p0..p3 and c[8].  It may read p0[j[k]]; a patch that does not exist is never evaluated and no index outside
 *     [0, n) is loaded.
 *   Gradient.  grad[r,c] = the sum of g[3*dr + dc] of patch (r(-)dr, c(-)dc) over dr = 2, 1, 0 (outer) and dc = 2, 1, 0 (inner):
 *     g[8] of (r(-)2, c(-)2) + g[7] of (r(-)2, c(-)1) + g[6] of (r(-)2, c) + g[5] of (r(-)1, c(-)2) + .. + g[0] of (r, c) -- the
 *     patches that exist, in this fixed order, started from the first (no leading 0 +).  (-) wraps on a periodic axis; on an
 *     open axis a negative origin means the patch does not exist.  On a torus the order is translation-invariant.
 *   f = the order-independent (compensated) sum of the existing patches' values, each added once, by the owner of the patch's
 *     origin.  One rounding per source operation, no contraction, no floating-point atomic.  In the trial kernels every window
 *     value is xp + step*d, never a read of the x the launch writes.
 *   Per-node terms.  A per-node term is written inside the body.  The term of the node in slot (dr, dc) is added by a patch iff
 *       (dr == 0 || (!(periodic & 2) && row + 3 == rows)) && (dc == 0 || (!(periodic & 1) && col + 3 == cols)):
 *     node (row, col) goes to the patch that starts there; on an open axis the last layer of patches picks up the two layers
 *     of nodes no patch starts at, and on a periodic axis there is nothing to pick up.  Every node is then counted exactly
 *     once.  A term on the CENTRE of every patch (a double well on x[4], say) is another sum: over the patches, not the nodes.
 * lbfgsx_objective_compile_grid_stencil wraps the body for the four kernels of csrc/grid_stencil_kernels.cuh (same arguments,
 * grids, reductions, out[] layout and completion signal as the periodic grid form's; the packs one and two rows away from a
 * thread's pack are re-read through the caches) and caches by (form, body, K, dtype) with K = 9 (lbfgsx_objective_K): the
 * shape and the mask are not part of the key, and the same text as a periodic grid and as a grid stencil objective are two
 * entries.  The form is LBFGSX_FORM_GRID_STENCIL.  lbfgsx_objective_bind_grid_stencil refuses (LBFGSX_E_INVALID, the values
 * named) a handle of another form, an extent < 3, rows*cols that is not n or overflows, and a mask with bits above 3; every
 * other bind call refuses this handle, lbfgsx_objective_bind saying that it is bound with its shape and mask.
 * lbfgsx_objective_shape and lbfgsx_objective_periodic read the bound shape and mask back. */
int lbfgsx_objective_compile_grid_stencil(lbfgsx_objective** out, int dtype, const char* body, char* log, size_t log_len);
long long lbfgsx_objective_source_grid_stencil(int dtype, const char* body, char* out, size_t len);
int lbfgsx_objective_bind_grid_stencil(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                       const void* const p[4], const double cs[8], int* id);
/* ---- graph objectives: edge terms over an index list ---------------------------------------------------------------------
 * x has n coordinates, the NODES; the caller gives E edges as two int32 arrays ei[E], ej[E], and
 *     f(x) = sum over nodes v of psi(x[v]; v)  +  sum over edges e of phi(x[ei[e]], x[ej[e]]; e)
 * -- spring and finite-element energies on an unstructured mesh, graph-Laplacian regularisers, XY and synchronisation
 * energies, pairwise-comparison losses, any smoothness term on a graph.  Both terms are HIP/C++ text:
 *   edge_body sees T, const T x[2] (x[0] = x at ei[e], x[1] = x at ej[e], always in the edge's own orientation), T g[2] (the
 *             two partial derivatives, to fill), int64_t e, i, j (the edge's index and its two node indices), p0..p3 and
 *             c[8]; it returns the edge's value;
 *   node_body (NULL or empty: no node term) sees T, const T x[1], T g[1], int64_t i, p0..p3 and c[8]; it returns the node's
 *             value.
 * The data arrays are raw device pointers the bodies index themselves (p0[e] per edge, p1[i] per node): the library does
 * not know their lengths.
 * Semantics (a numpy restatement with one operation per source operation is bit-exact):
 *   grad[v] = psi's g[0] if there is a node body, then the contributions g_e[side] of the edges incident to v in ASCENDING
 *             EDGE INDEX e (a duplicate edge or an edge listed in both directions contributes once per listing); the sum
 *             starts from the first contribution (no leading 0 +); a node with no contribution gets +0;
 *   f       = the order-independent (compensated) sum the other forms use: each node value added once, by the node's owner,
 *             each edge value added once, by the thread that owns ei[e];
 *   one rounding per source operation, no contraction.
 * Determinism comes from the mapping; no floating-point atomic is used.  The thread that owns v evaluates every edge
 * incident to v and keeps its own side's partial derivative, so an edge's term is evaluated twice, once from each end, on
 * identical inputs by the same instructions: both evaluations have the same bits.  (The alternative, storing every
 * contribution and summing per destination in a second pass, costs a second launch and 2E more stores; the recomputation
 * keeps the single fused launch every form has.)
 * lbfgsx_objective_compile_graph wraps the bodies for the four kernels of csrc/graph_kernels.cuh -- the counterparts of
 * k_eval, k_trial, k_b_eval and k_b_dg_maxstep_trial with the same arguments, grids and reductions -- and caches by (form,
 * both bodies, dtype); lbfgsx_objective_K returns 2 and the form is LBFGSX_FORM_GRAPH.  The word asm in either body is
 * refused; the compile log counts lines per body (file names "edge_body" and "node_body").
 * lbfgsx_objective_bind_graph copies ei / ej (host pointers, or device pointers when edges_on_device != 0; a later change of
 * the caller's arrays has no effect) and builds, on the device, the incidence list the context owns (csrc/graph_topology.hip):
 * uint32 off[n+1] and, for node v, the entries off[v] .. off[v+1]-1 in ascending e, each 8 bytes {int32 other end,
 * uint32 (e << 1) | side}.  VALIDATION COMES FIRST: an edge with an index outside [0, n) or with ei[e] == ej[e] makes the
 * call return LBFGSX_E_INVALID with the smallest such e, its i and j, n and the number of offending edges in the message,
 * and leaves no graph objective bound -- no evaluation kernel is ever launched on an index that was not checked.  Also
 * refused, the values named: a handle of another form, E < 1, E > 2^31 - 1, n > 2^31 - 1.  The list is rebuilt at every
 * bind; nothing is cached by pointer.  lbfgsx_objective_bind refuses a graph handle.
 * lbfgsx_objective_topology copies the built list to host arrays (off: n+1, other and edge_side: 2E elements; any may be
 * NULL) and stores E.  lbfgsx_objective_upload_count is lbfgsx_objective_upload for an array of `count` elements (per-edge
 * data has E, not n).
 * Byte model of one launch (lbfgsx_counters_ex): the built-in's streams plus (n+1)*4 bytes of offsets, 2E*8 bytes of entries
 * and 2E*sizeof(T) bytes of gathered values (twice that in the trial kernels, which gather xp and d).  Each gathered value
 * is counted once; the sectors actually fetched for it are not.
 * Measured (profiles/graph_objective.json; one trial evaluation at n = 1e8 f64): built-in 0.575 ms, the
 * path graph 1.10 ms, the 10000 x 10000 lattice as a graph (E = 2e8) 2.32 ms with natural labels and 16.5 ms with randomly
 * relabelled nodes, its torch callable (natural labels) 10.8 ms; building the list 15 to 30 ms.
 * Not built: an edge-parallel or chunked mapping for strongly skewed degrees (a node's list is walked by one thread),
 * reordering of the nodes for locality, the lock-step batch.  Vector unknowns per node and terms over more than two nodes
 * are the mesh form's (below). */
int lbfgsx_objective_compile_graph(lbfgsx_objective** out, int dtype, const char* node_body, const char* edge_body, char* log,
                                   size_t log_len);
long long lbfgsx_objective_source_graph(int dtype, const char* node_body, const char* edge_body, char* out, size_t len);
int lbfgsx_objective_bind_graph(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t E, const int32_t* ei, const int32_t* ej,
                                int edges_on_device, const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_topology(lbfgsx_ctx* c, int64_t* E, uint32_t* off, int32_t* other, uint32_t* edge_side);
int lbfgsx_objective_upload_count(lbfgsx_ctx* c, int slot, const void* host, int64_t count, void** dev);
/* ---- mesh objectives: K-node elements, D unknowns per node ---------------------------------------------------------------
 * N nodes with D unknowns each, D in {1, 2, 3}; x is node-major, x[v*D + d], n = N*D.  E elements of K nodes each, K in
 * {2, 3, 4}, as one int32 array elems[E*K], row-major (a connectivity table), and
 *     f(x) = sum over nodes v of psi(x_v; v)  +  sum over elements e of phi(x at the K nodes of e; e)
 * -- springs in space, triangle and tetrahedron energies, FEM elasticity, mesh smoothing.  Both terms are HIP/C++ text:
 *   elem_body sees T, constexpr int K, D, const T x[K*D] (slot-major: x[k*D + d] is unknown d of the node in slot k, in the
 *             element's own slot order), T g[K*D] (to fill), int64_t e, const int64_t v[K] (the node indices in slot
 *             order), p0..p3 and c[8]; it returns the element's value;
 *   node_body (NULL or empty: none) sees T, D, const T x[D], T g[D], int64_t i, p0..p3, c[8]; it returns the node's value.
 * The data arrays are raw device pointers the bodies index themselves (p0[e], p1[i], p2[i*D + d]).
 * Semantics (a numpy restatement with one operation per source operation is bit-exact):
 *   grad[v*D + d] = psi's g[d] if there is a node body, then g_e[slot*D + d] of the elements that contain v in ASCENDING
 *             ELEMENT INDEX e (an element's nodes are pairwise distinct; an element listed twice contributes twice); the
 *             sum starts from the first contribution (no leading 0 +); a node with no contribution gets +0;
 *   f       = the order-independent (compensated) sum the other forms use: a node's value added once, by the node's
 *             owner, an element's once, by the owner of the node in slot 0;
 *   one rounding per source operation, no contraction.
 * The thread that owns v evaluates every element that contains v and keeps the partials of v's slot, so an element's term
 * is evaluated K times on identical inputs by the same instructions: the same bits, no floating-point atomic.  The price of
 * the single fused launch with a reproducible sum is K times the arithmetic and K*(K-1)*D gathered values per element.
 * (Storing the K*D contributions once and summing per destination in a second pass evaluates each body once but costs a
 * second launch, K*D*E stores and as many gathered loads.)
 * lbfgsx_objective_compile_mesh wraps the bodies for the four kernels of csrc/mesh_kernels.cuh, the counterparts of the
 * graph form's, and caches by (form, both bodies, K, D, dtype); lbfgsx_objective_K returns K, lbfgsx_objective_dim D (1 for
 * the other forms), the form is LBFGSX_FORM_MESH.  K or D out of range and the word asm in a body are refused with the
 * value named; the compile log counts lines per body ("elem_body", "node_body").
 * lbfgsx_objective_bind_mesh copies elems (host, or device when elems_on_device != 0) and builds on the device the list the
 * context owns (csrc/mesh_topology.hip): uint32 off[N+1] and, for node v, the entries off[v] .. off[v+1]-1 in ascending e,
 * each K 32-bit words: (e << 2) | slot, then the element's other nodes in ascending slot order.  VALIDATION COMES FIRST: an
 * index outside [0, N) or two equal indices in an element return LBFGSX_E_INVALID with the smallest such e, its K indices,
 * N and the number of offenders, and leave no objective bound.  Also refused, the values named: a handle of another form,
 * E < 1, E > 2^30 - 1, n not a multiple of D, n > 2^31 - 1.  Rebuilt at every bind; nothing is cached by pointer.
 * lbfgsx_objective_bind and lbfgsx_objective_bind_graph refuse a mesh handle.  lbfgsx_objective_mesh_topology copies the
 * list to host arrays (off: N+1, words: K*E*K elements; either may be NULL) and stores E.
 * Byte model of one launch: the built-in's streams plus (N+1)*4 bytes of offsets, K*E*4K of entries and
 * K*E*(K-1)*D*sizeof(T) of gathered values (twice that in the trial kernels).  Registers, measurements: DESIGN.md section 1.
 * Not built: K > 4 or D > 3, mixed element types, a chunked or element-parallel mapping for hubs, node reordering, the
 * lock-step batch, a bench.py leg. */
int lbfgsx_objective_compile_mesh(lbfgsx_objective** out, int dtype, int K, int D, const char* node_body, const char* elem_body,
                                  char* log, size_t log_len);
long long lbfgsx_objective_source_mesh(int dtype, int K, int D, const char* node_body, const char* elem_body, char* out, size_t len);
int lbfgsx_objective_bind_mesh(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t E, const int32_t* elems, int elems_on_device,
                               const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_mesh_topology(lbfgsx_ctx* c, int64_t* E, uint32_t* off, uint32_t* words);
int lbfgsx_objective_dim(const lbfgsx_objective* obj);
/* ---- linear-model objectives: sparse-matrix terms phi(a_r . x) ------------------------------------------------------------
 * x has n coordinates, the WEIGHTS; the caller gives a sparse R x n matrix A in CSR (int32 rowptr[R+1], int32 col[nnz],
 * T val[nnz]; row r is one SAMPLE), and
 *     f(x) = sum over coordinates j of psi(x[j]; j)  +  sum over rows r of phi(z_r; r),      z = A x
 * -- logistic regression, least squares, non-negative least squares under L-BFGS-B, Poisson and Huber regression, L2-loss
 * SVMs.  A row couples as many coordinates as it has entries.  Both terms are HIP/C++ text:
 *   row_body   sees T, const T z (the row's product with x), T& dz (to assign: phi'(z)), int64_t r, p0..p3 and c[8]; it
 *              returns phi(z).  Per-row data is indexed by the body, p0[r] (lbfgsx_objective_upload_count, count = R);
 *   coord_body (NULL or empty: none) is a graph objective's node body: T, const T x[1], T g[1], int64_t i, p0..p3, c[8];
 *              it returns psi.
 * Semantics (a numpy restatement with one operation per source operation is bit-exact; tests/linear_ref.py):
 *   z_r     L lanes share a row, L a power of two in 1..64.  Lane l takes the row's entries k0+l, k0+l+L, .. in ascending
 *           order: s_l = val[k]*x[col[k]] for its first entry, s_l = s_l + val[k]*x[col[k]] after it; a lane with no entry
 *           holds +0.  Then s_l = s_l + s_{l+h} for l < h, h = L/2, L/4, .., 1, and z_r = s_0.  A row's entries are taken in
 *           the caller's order, duplicate (r, c) entries contribute twice, an empty row has z = +0 and still has its phi.
 *           L is fixed at bind: the largest power of two <= max(1, nnz / R) (integer division), at most 64, so that a row of
 *           average length gives a lane one or two entries; the bind call's `lanes` forces it (0: by the rule);
 *   grad[j] psi's g[0] if there is a coordinate body, then val*w[r], w[r] = phi'(z_r), over the entries of column j in
 *           ascending r and within one r in the caller's order (a stable sort of the CSR entries by column), started from
 *           the first contribution; a column with none gets +0.  A column with more than C = 4096 entries is LONG (an
 *           intercept column has R): it is cut into chunks of C consecutive entries; chunk b's partial is formed by 256
 *           threads, thread t summing the products of the chunk's entries t, t+256, .. in ascending order from its first
 *           (+0 if none), then s_t = s_t + s_{t+h} for t < h, h = 128 .. 1, the partial being thread 0's value; grad[j] is
 *           psi's g[0], then the chunk partials in ascending b, started from the first contribution;
 *   f       the order-independent (compensated) sum the other forms use, over all psi and all phi values;
 *   one rounding per source operation, no contraction.
 * An evaluation is two launches on one stream with no host wait between them (csrc/linear_kernels.cuh): the ROW pass
 * (k_lin_rows; k_lin_rows_trial gathers xp[c] + step*d[c], the statement c's owner executes, never the x being written)
 * writes w[R] and v[R] = phi(z_r) into vectors the context owns, the COLUMN pass (k_lin_eval, k_lin_trial, k_lin_b_eval,
 * k_lin_b_dg_maxstep_trial: the arguments, tile order, reductions and completion word of the other forms' kernels) forms
 * the gradient per owned coordinate and adds v to f.  Its grid covers the longer of n and R.  A matrix with a long column
 * has a third launch between them, k_lin_long_cols (one block per chunk, precompiled in the library).  No float atomic.
 * The row pass and the column walk are written once, for D outputs per row (lin_rows over an entry source, lin_coord); this
 * form is their D = 1, and the multi-output and the dense form below use the same code.
 * lbfgsx_objective_compile_linear caches by (form, both bodies, dtype); the form is LBFGSX_FORM_LINEAR, lbfgsx_objective_K
 * returns 1.  The word asm in either body is refused; the compile log counts lines per body ("row_body", "coord_body").
 * lbfgsx_objective_info's maxima cover all six kernels.
 * lbfgsx_objective_bind_linear copies the three arrays (host pointers, or device pointers when matrix_on_device != 0; a
 * later change of the caller's arrays has no effect) and builds on the device what the context owns
 * (csrc/linear_topology.hip): the transposed list (uint32 colptr[n+1]; per entry its row, value and CSR position) by a
 * stable radix sort, and the table of long columns and their chunks.  The bind issues 6 launches.  VALIDATION COMES FIRST,
 * in the bind's first launch, the only one of a refused bind: rowptr[0] = 0, rowptr non-decreasing, rowptr[R] = nnz, every
 * col in [0, n).  An offender returns LBFGSX_E_INVALID with the first offending position, its value, n (or R and nnz) and the
 * number of offenders in the message and leaves no objective bound.  Also refused, the values named: a handle of another
 * form, R < 1, nnz < 1, R, nnz or n above 2^31 - 1, lanes not 0 or a power of two <= 64.  Rebuilt at every bind; nothing is
 * cached by pointer.  The other bind calls refuse a linear-model handle.
 * lbfgsx_objective_linear_topology reads the list back: info = {R, nnz, L, C, long columns, chunks, 0, 0}; colptr (n+1),
 * trow and tpos (nnz each: the row of a transposed entry and the CSR position it came from), long_col (long columns,
 * ascending), long_chunk (long columns + 1: the first chunk of each), chunk (2 per chunk: first and past-the-last entry).
 * Any pointer may be NULL.
 * Byte model of one evaluation (lbfgsx_counters_ex): the built-in's streams plus, for both passes, the offsets (R+1 and n+1
 * words), 2 nnz indices, 2 nnz values and the gathered values once each (nnz of x, or of xp and d in a trial, and nnz of w),
 * w and v written and read, the chunk partials written and read.
 * Not built: reusing z = A xp and A d across the trials of one line search (which would make every trial after the first
 * O(R)), column reordering, the lock-step batch, a bench.py leg.  (Several outputs per row are the next section's form, a
 * dense matrix the one after it.)  Measurements: DESIGN.md section 1. */
int lbfgsx_objective_compile_linear(lbfgsx_objective** out, int dtype, const char* coord_body, const char* row_body, char* log,
                                    size_t log_len);
long long lbfgsx_objective_source_linear(int dtype, const char* coord_body, const char* row_body, char* out, size_t len);
int lbfgsx_objective_bind_linear(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, int64_t nnz, const int32_t* rowptr,
                                 const int32_t* col, const void* val, int matrix_on_device, int lanes, const void* const p[4],
                                 const double cs[8], int* id);
int lbfgsx_objective_linear_topology(lbfgsx_ctx* c, int64_t info[8], uint32_t* colptr, int32_t* trow, uint32_t* tpos,
                                     int32_t* long_col, uint32_t* long_chunk, uint32_t* chunk);
/* ---- multi-output linear-model objectives: D outputs per row, phi(a_r . X) ---------------------------------------------------
 * x holds an F x D WEIGHT MATRIX X, feature-major: x[j*D + c], n = F*D.  A is the caller's sparse R x F CSR matrix and
 *     Z = A X  (R x D),      f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r)
 * -- multinomial (softmax) logistic regression, multi-class SVMs, multi-target least squares, non-negative matrix regression
 * under L-BFGS-B.  D is a compile-time constant of the generated struct, 1 <= D <= 16 ("D = # is not supported: a row has
 * D = 1 .. 16 outputs").
 *   row_body   sees T, constexpr int D, const T z[D], T dz[D] (to fill with dphi/dz_c), int64_t r, p0..p3 and c[8]; it
 *              returns phi.  Loops over D unroll fully with #pragma unroll;
 *   coord_body (NULL or empty: none) is the scalar form's, per coordinate i = j*D + c: const T x[1], T g[1], int64_t i; D is
 *              visible, so the body can recover j = i / D and c = i % D.
 * Semantics (bit-exact numpy restatement: tests/multilinear_ref.py): Z[r, c] is the scalar form's row sum for each c on its
 * own (lane l: s_l[c] = val[k]*x[col[k]*D + c] for its first entry, s_l[c] = s_l[c] + .. after it, +0 without one; then the
 * halvings; L by the same rule from nnz / R, or `lanes`).  grad[j*D + c] is psi's g[0] if there is a coordinate body, then
 * tval[q]*w[trow[q]*D + c], w[r*D + c] = dz[c], over column j's transposed entries in ascending q, started from the first
 * contribution, +0 without any.  A column with more than C = 4096 entries is long, as in the scalar form: per chunk b and
 * output c the partial part[b*D + c] is formed by the scalar form's 256-thread rule over w[trow[q]*D + c], and the owner adds
 * a column's partials in ascending b.  f, roundings and the trial's gather of xp[i] + step*d[i]: the scalar form's.
 * Kernels (csrc/linear_multi_kernels.cuh; the bodies are the scalar form's, csrc/linear_kernels.cuh, with D from the
 * generated struct): the row pass k_linm_rows / k_linm_rows_trial (L lanes per row, D accumulators per lane, 16-byte loads of
 * a feature's weight row when D*sizeof(T) is a multiple of 16, D cross-lane moves per halving, no LDS, no atomic), the column
 * pass k_linm_eval, k_linm_trial, k_linm_b_eval, k_linm_b_dg_maxstep_trial (a thread owns one 16-byte pack of consecutive
 * coordinates; coordinate i walks the list of feature i / D, so a pack may straddle two features), and the scalar form's
 * k_lin_long_cols with one block per (chunk, output), precompiled, the third launch only when the matrix has a long column.
 * lbfgsx_objective_compile_linear_multi caches by (form, both bodies, dtype, D); the form is LBFGSX_FORM_LINEAR_MULTI,
 * lbfgsx_objective_K returns 1 and lbfgsx_objective_dim D.  The handle is bound with lbfgsx_objective_bind_linear (and minimised
 * with lbfgsx_solver_minimize_linear), which accept a handle of either linear form; for this one they refuse n % D != 0 with
 * both values named, validate col against F = n / D, size w to R*D and the chunk partials to chunks*D, and
 * lbfgsx_objective_linear_topology reports D in info[6] (0 for the scalar form) with colptr of F + 1 elements.  Every other
 * bind call refuses the handle, as they refuse a scalar one; so do the Gram-space recursion, row shards and the lock-step batch.
 * Byte model of one evaluation: the scalar form's with every count of gathered x, xp, d and w, of w written and read and of
 * the chunk partials multiplied by D; offsets (R+1 and F+1 words), indices and matrix values are counted once.  The D
 * coordinates of a feature read its entries again; those re-reads are cache hits and are not modelled.
 * Not built: D > 16, reusing Z across a line search's trials, mixed per-row output counts, the lock-step batch, a
 * bench.py leg.  (A dense matrix is the next section's form.)  Registers, measurements: DESIGN.md section 1. */
int lbfgsx_objective_compile_linear_multi(lbfgsx_objective** out, int dtype, int D, const char* coord_body, const char* row_body,
                                          char* log, size_t log_len);
long long lbfgsx_objective_source_linear_multi(int dtype, int D, const char* coord_body, const char* row_body, char* out,
                                               size_t len);
/* ---- dense linear-model objectives: the multi-output form over a dense row-major matrix ---------------------------------------
 * x holds an F x D weight matrix X, feature-major (x[j*D + c], n = F*D), A is the caller's DENSE R x F matrix, row-major with a
 * row stride of lda >= F elements, of the solver's dtype, and
 *     Z = A X  (R x D),      f(x) = sum over coordinates i of psi(x[i]; i)  +  sum over rows r of phi(Z[r, 0..D); r)
 * -- logistic, softmax, Poisson and least-squares regression on tabular features, NNLS under L-BFGS-B.  1 <= D <= 16 ("D = #
 * is not supported: a row has D = 1 .. 16 outputs").  The bodies are exactly the multi-output form's: row_body sees T,
 * constexpr int D, const T z[D], T dz[D], int64_t r, p0..p3, c[8] and returns phi; coord_body (NULL or empty: none) sees
 * const T x[1], T g[1], int64_t i.  D = 1 is the scalar model, written z[0] / dz[0]; there is no scalar-signature form.
 * Semantics (bit-exact numpy restatement: tests/dense_ref.py; one rounding per source operation, no contraction):
 *   Z[r, c]   the sparse forms' row rule on the dense row: L lanes share a row, lane l takes columns l, l+L, .. in ascending
 *             order, s_l[c] = A[r,k]*x[k*D + c] for its first column and s_l[c] = s_l[c] + .. after it, +0 without one; then
 *             s_l = s_l + s_{l+h} for l < h, h = L/2 .. 1, and Z[r, c] = s_0[c].  L is the largest power of two <= F, at most
 *             64 (the sparse rule with nnz / R = F), or `lanes`.  The same matrix given to the sparse forms as CSR with every
 *             entry stored, and the same lanes, gives the same bits in z, w, v and f.
 *   grad      rows are cut into chunks of C = 256 consecutive rows (the last one shorter); part[b*n + j*D + c] is the sum over
 *             the rows r of chunk b, in ascending r, of A[r,j]*w[r*D + c], w[r*D + c] = dz[c], started from the first
 *             product; grad[j*D + c] is psi's g[0] if there is a coordinate body, then the partials in ascending b, started
 *             from the first contribution.  C is part of the semantics, a constant (never data-dependent), reported in info[4].
 *   f         the order-independent compensated sum of the other forms over all psi and phi values.
 *   trial     the weight used is xp[i] + step*d[i], the statement i's owner executes, never a read of the x the launch writes.
 * Kernels (csrc/linear_dense_kernels.cuh), three launches per evaluation on one stream, no host wait: the row pass
 * k_dense_rows / k_dense_rows_trial (the sparse forms' row pass with the dense row as its entry source: kBlock / L rows per
 * block step, the lanes of a row read consecutive elements, D accumulators per lane, cross-lane halvings, no LDS, no atomic),
 * the partial pass k_dense_partials (A read a second time,
 * column-wise without a strided access: a thread owns a 16-byte pack of consecutive columns and walks the C rows of a chunk
 * with W*D accumulators; small F packs several chunks into a block) and the column pass k_dense_eval, k_dense_trial,
 * k_dense_b_eval, k_dense_b_dg_maxstep_trial (a thread owns a 16-byte pack of coordinates and adds their partials).
 * k_dense_partials holds no caller text but is instantiated in the generated unit, which keeps D a compile-time constant.
 * lbfgsx_objective_compile_dense caches by (form, both bodies, dtype, D); the form is LBFGSX_FORM_DENSE, lbfgsx_objective_K
 * returns 1 and lbfgsx_objective_dim D.
 * lbfgsx_objective_bind_dense: F = n / D.  A HOST matrix (a_on_device = 0) is copied to the device compactly; the context owns
 * the copy and frees it with the other forms' lists.  A DEVICE matrix is used IN PLACE and is NOT copied: the caller keeps it
 * alive and unchanged while the objective is bound (a second copy is what would make dense data infeasible).  Refused with
 * LBFGSX_E_INVALID, the values named, nothing bound, no launch: a handle of another form, R < 1, A null, n % D != 0, lda < F,
 * R or F above 2^31 - 1, lanes not 0 or a power of two <= 64.  Every other bind call refuses a dense handle, and this one
 * theirs; lbfgsx_solver_minimize_obj and _linear refuse it; so do the Gram-space recursion, row shards and the lock-step batch.
 * lbfgsx_objective_dense_info: info = {R, F, D, L, C, chunks, lda, 1 if the context owns a copy of A}.
 * lbfgsx_objective_dense_read: w (R*D), v (R) and part (chunks*n) of the last evaluation, host arrays, any of them NULL.
 * Byte model of one evaluation (lbfgsx_counters_ex), with s = sizeof(T): the built-in's streams, plus 2 R F s for A (read by
 * the row pass and by the partial pass), n s of weights for the row pass (2 n s in a trial), R D s of w written and R D s
 * read, R s of v written and R s read, chunks n s of partials written and the same read.  The row pass's re-reads of x and
 * the partial pass's re-reads of w are served by the caches and are not modelled.  Launches per evaluation: 3; per bind: the
 * upload only.
 * Not built: a single-sweep kernel that forms Z and A^T w from one read of A, reuse of A xp and A d across a line search's
 * trials, the matrix cores (no default path runs an MFMA, and the bit contract forbids reordering the sums), D > 16,
 * column-major A, mixed dense + sparse blocks, the lock-step batch, a bench.py leg.  Registers, measurements: DESIGN.md
 * section 1. */
int lbfgsx_objective_compile_dense(lbfgsx_objective** out, int dtype, int D, const char* coord_body, const char* row_body, char* log,
                                   size_t log_len);
long long lbfgsx_objective_source_dense(int dtype, int D, const char* coord_body, const char* row_body, char* out, size_t len);
int lbfgsx_objective_bind_dense(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, const void* A, int64_t lda, int a_on_device,
                                int lanes, const void* const p[4], const double cs[8], int* id);
int lbfgsx_objective_dense_info(lbfgsx_ctx* c, int64_t info[8]);
int lbfgsx_objective_dense_read(lbfgsx_ctx* c, void* w, void* v, void* part);
/* ---- graph-regularised linear-model objectives: edge terms in the linear column pass ------------------------------------------
 * The scalar linear-model form with a coupling term over a graph on its coordinates: x has n coordinates, A is a sparse R x n
 * CSR matrix, the E edges are (ei[e], ej[e]) with 0 <= ei[e], ej[e] < n, ei[e] != ej[e], and
 *     f(x) = sum over coordinates j of psi(x[j]; j)  +  sum over edges e of rho(x[ei[e]], x[ej[e]]; e)
 *            +  sum over rows r of phi(z_r; r),      z = A x
 * -- tomographic and deblurring reconstruction with a smoothness or smoothed-TV prior under non-negativity (L-BFGS-B),
 * Poisson or logistic regression with a GMRF / ICAR prior on a latent field, Laplacian-regularised least squares, fused and
 * graph-trend regression with a Huber penalty on differences, network-coupled GLMs.  Three bodies of HIP/C++ text:
 *   row_body   a linear-model objective's: T, const T z, T& dz, int64_t r, p0..p3, c[8]; returns phi(z);
 *   edge_body  a graph objective's: T, const T x[2] (x at ei[e] and at ej[e]), T g[2], int64_t e, i, j, p0..p3, c[8]; returns rho;
 *   coord_body (NULL or empty: none) T, const T x[1], T g[1], int64_t i, p0..p3, c[8]; returns psi.
 * The three bodies share the four data arrays and the eight scalars: a data array has n, E or R elements, as the body that
 * indexes it needs (lbfgsx_objective_upload_count).
 * Semantics (tests/graph_linear_ref.py is the bit-exact numpy restatement):
 *   z_r, w[r], v[r], L, long columns, chunks and C = 4096 are exactly the linear-model form's;
 *   grad[j] in this order, started from the first contribution (no leading 0 +; +0 if there is none): psi's g[0] if there is
 *           a coordinate body; g_e[side] of j's incidence entries in ascending e (the graph form's rule: an edge is evaluated
 *           from both ends on identical inputs, so both evaluations have the same bits); the matrix contributions exactly as
 *           the linear-model form adds them, tval[q]*w[trow[q]] in ascending q or a long column's chunk partials in ascending b;
 *   f       the order-independent (compensated) sum over every psi value, every edge value (added by the owner of end 0) and
 *           every v[r];
 *   in the trial kernels every gathered value, an edge's other end or a row's x[col], is xp[u] + step*d[u], never a read of
 *   the x the launch writes; one rounding per source operation, no contraction.
 * An evaluation is the linear-model form's launches (csrc/linear_graph_kernels.cuh): the row pass k_lin_rows /
 * k_lin_rows_trial instantiated for this form's struct, k_lin_long_cols when the matrix has a long column, then the column
 * pass k_ling_eval, k_ling_trial, k_ling_b_eval or k_ling_b_dg_maxstep_trial, whose node runs the coordinate term, then the
 * node's edges (graph_walk), then its column (the rest of lin_coord) into one running sum: x, xp, d, g, lb and ub are streamed once
 * for both terms.  2 launches per evaluation, 3 with a long column.  No LDS, no float atomic.
 * lbfgsx_objective_compile_linear_graph caches by (form, three bodies, dtype); the form is LBFGSX_FORM_LINEAR_GRAPH,
 * lbfgsx_objective_K returns 1.  The word asm in any body is refused; the compile log counts lines per body ("coord_body",
 * "edge_body", "row_body").  lbfgsx_objective_info's maxima cover all six kernels.
 * lbfgsx_objective_bind_linear_graph builds both lists on the device: the incidence list of lbfgsx_objective_bind_graph
 * (5 launches), then the transposed matrix of lbfgsx_objective_bind_linear (6 launches) beside it.  Each build validates its
 * indices in its first launch; an offender in either list returns LBFGSX_E_INVALID with the first offending edge or
 * position named, as those two calls name it, and leaves no objective bound and no list on the context (an offending edge: 1
 * launch; an offending matrix: the 5 of the edges and 1).  Also refused, the values named: a handle of another form, E < 1,
 * R < 1, nnz < 1, E, R, nnz or n above 2^31 - 1, lanes not 0 or a power of two <= 64.  The other bind calls refuse the handle
 * as they refuse every form that is not theirs: lbfgsx_objective_bind with "a graph-regularised linear-model objective is bound
 * with its matrix and edges: lbfgsx_objective_bind_linear_graph"; lbfgsx_objective_bind_linear, _bind_graph, _bind_mesh, _bind_grid
 * and _bind_dense with "<the call>: the handle is a graph-regularised linear-model objective, not a <that call's form>".
 * lbfgsx_objective_topology and lbfgsx_objective_linear_topology both read back from a context bound this way.
 * Byte model of one evaluation: the linear-model form's plus the graph form's list terms (n+1 offsets, 2E entries of 8
 * bytes, 2E gathered values, of x or of xp and d).
 * Not built: D > 1 outputs per row, the dense matrix, mesh elements in place of edges, the lock-step batch, a bench.py leg.
 * Registers, measurements: DESIGN.md section 1. */
int lbfgsx_objective_compile_linear_graph(lbfgsx_objective** out, int dtype, const char* coord_body, const char* edge_body,
                                          const char* row_body, char* log, size_t log_len);
long long lbfgsx_objective_source_linear_graph(int dtype, const char* coord_body, const char* edge_body, const char* row_body,
                                               char* out, size_t len);
int lbfgsx_objective_bind_linear_graph(lbfgsx_ctx* c, const lbfgsx_objective* obj, int64_t R, int64_t nnz, const int32_t* rowptr,
                                       const int32_t* col, const void* val, int matrix_on_device, int lanes, int64_t E,
                                       const int32_t* ei, const int32_t* ej, int edges_on_device, const void* const p[4],
                                       const double cs[8], int* id);
/* Every entry point of this ABI makes the context's device current for its own duration and restores the caller's
 * afterwards.  Code that launches its OWN kernels on the context's vectors (a device functor, lbfgsx_vec) must run with
 * that device current too: lbfgsx_device tells which one it is, lbfgsx_device_push makes it current for the calling
 * thread (returning the previous one in *prev), lbfgsx_device_pop restores.  The drop-in solvers bracket every call of a
 * device functor with the pair (LBFGSpp/Device.h, Evaluator::call_user). */
int lbfgsx_device(const lbfgsx_ctx* c);
int lbfgsx_device_push(const lbfgsx_ctx* c, int* prev);
int lbfgsx_device_pop(int prev);
/* The persistent launch survives a device it does not own: a meeting point that waits longer than 100 ms flags the launch,
 * the product is redone with the 2c+1 step launches (bit-identical), which the context keeps for 8 products before it tries
 * the persistent form again; every further time-out quadruples that pause, a clean persistent launch resets it.
 * out = {persistent launches, time-outs, products left of the current pause, products computed with step launches}. */
int lbfgsx_persist_counts(const lbfgsx_ctx* c, int64_t out[4]);
/* test hook: sets the failure word the next persistent launch of this context will find (as if a meeting point had timed
 * out); that launch does nothing and the host takes the recovery path above */
int lbfgsx_debug_persist_fault(lbfgsx_ctx* c);
/* instrumentation, process-wide: {kernel launches, stream synchronisations, asynchronous copies} issued by the library
 * since load (or the last call with reset != 0).  bench.py divides them by the iterations of its L-BFGS-B leg. */
int lbfgsx_counters(int64_t out[3], int reset);
/* the same three and the byte model of the L-BFGS-B path as built: out[3] = bytes the launches of the path had to move for
 * the rows and columns they were launched over (columns x rows of the compact copy of the free rows + the vectors each
 * pass reads and writes per row, gathers at 64-byte sectors; DESIGN.md section 5 lists the per-kernel terms), out[4] =
 * passes over the compact copy, out[5] = rows those passes walked, out[6..7] = 0.  bench.py's cfg4 roofline fraction is
 * out[3] of its window / time / HBM peak.  No reference counterpart (instrumentation). */
int lbfgsx_counters_ex(int64_t out[8], int reset);
/* Polled completion (contexts with mapped outputs, i.e. L-BFGS-B ones; LBFGSX_POLL=0 switches it off): the last block of a
 * kernel whose results the host reads next stores a sequence number in host-mapped memory after the results, and the host
 * polls that word instead of waiting for the stream (which returns ~9 us after the kernel's end).  out = {waits served by
 * polling, waits that timed out (50 ms) and fell back to the stream wait -- a kernel that failed to signal} */
int lbfgsx_poll_counts(const lbfgsx_ctx* c, int64_t out[2]);
/* The same with the reasons polling was given up: out = {waits, time-outs, time-outs that said "polling cannot work here"
 * (the word still unset after the stream drained, or the stream wait returned at once because the kernel had ended long
 * before its store became visible), 1 if this context now waits for its stream instead of polling (after two of those)} */
int lbfgsx_poll_counts_ex(const lbfgsx_ctx* c, int64_t out[4]);
/* Tracing: the drop-in solvers bracket their phases -- iteration, line search, post + apply_Hv, the
 * generalized Cauchy point, the subspace minimisation, a lock-step iteration of the batch -- with these calls.  With
 * LBFGSX_ROCTX=1 they become ROCTx ranges (roctxRangePushA / roctxRangePop, the marker library loaded with dlopen), which
 * `rocprofv3 --marker-trace --kernel-trace` shows beside the kernels; otherwise they cost one branch.  `name` must be a string
 * with static storage duration.  No reference counterpart (the reference has no tracing). */
void lbfgsx_range_push(const char* name);
void lbfgsx_range_pop(void);

/* ---- Gram-space ("vector-free") form of the recursion: opt-in, outside the bit-parity contract ----
 * BFGSMat::apply_Hv (BFGSMat.h:276-302) only combines the 2c+1 vectors [S, Y, g]; with their Gram matrix kept on the
 * host (include/LBFGSpp/GramSpace.h) an iteration needs two passes over the history instead of 2c+1 dependent ones.
 * Supported for m <= 24 (LBFGSX_E_INVALID otherwise). */
/* lbfgsx_post_linesearch (LBFGS.h:130,137,159-161; s, y into the spare column) plus, in the same pass, the Gram rows
 * of the new pair and of the new gradient.  scal = {g.g, x.x, s.y, y.y, s.s, g.s, g.y}; for the logical slots
 * j < lbfgsx_bfgs_ncorr(): sdots[j] = S_j.s, sdots[m+j] = Y_j.s, gdots[j] = S_j.g, gdots[m+j] = Y_j.g (arrays of 2m).
 * Sums accumulate in f64 (fixed reduction order).  ydots (2m doubles, may be NULL) receives S_j.y, Y_j.y when the
 * history is kept in f32 (below) -- there the dots are taken from the rounded, stored y; with a native history the caller
 * derives them as differences of the gradient dots and ydots is left untouched. */
int lbfgsx_gs_post_linesearch(lbfgsx_ctx* c, double scal[7], double* sdots, double* gdots, double* ydots);
/* Mixed-precision history: dtype = LBFGSX_F32 on an f64 context makes the Gram-space entry points keep
 * S and Y as float (half the history traffic and memory; x, g, d and all sums stay f64).  Only with an empty history
 * (after lbfgsx_bfgs_reset); dtype = the context's own type switches back.  While it is on, the vector-form entry points
 * that touch the history (lbfgsx_apply_Hv with pairs stored, lbfgsx_post_linesearch, the history getters) return
 * LBFGSX_E_LOGIC. */
int lbfgsx_gs_set_history_dtype(lbfgsx_ctx* c, int dtype);
/* D = coef_g * G + sum_{j < ncorr} coef[j] * S_j + coef[m+j] * Y_j (logical slots); *dg = G . D  (LBFGS.h:123) */
int lbfgsx_gs_direction(lbfgsx_ctx* c, const double* coef, double coef_g, double* dg);

/* ---- L-BFGS-B device operators (contexts created with LBFGSX_FLAG_BOUNDED) ------------------------------
 * Index sets of the reference (fv_set, newact_set, BOXCQP's L/U/P: std::vector<int>) are a per-coordinate
 * state byte on the device; every operator streams the column-contiguous S/Y once and applies the mask. */
enum /* state-byte masks */
{
    LBFGSX_ST_FREE = 1, LBFGSX_ST_NEWACT = 2, LBFGSX_ST_L = 4, LBFGSX_ST_U = 8, LBFGSX_ST_P = 16
};
enum /* vectors formed on the fly inside masked operators */
{
    LBFGSX_VS_DRT = 0,      /* drt = xcp - x0                 (SubspaceMin.h:130)   */
    LBFGSX_VS_NEG_CF = 1,   /* -vecc                          (SubspaceMin.h:159)   */
    LBFGSX_VS_NEG_RHS = 2,  /* -rhs                           (SubspaceMin.h:243)   */
    LBFGSX_VS_LBOUND = 3,   /* vecl = lb - x0                 (SubspaceMin.h:153)   */
    LBFGSX_VS_UBOUND = 4,   /* vecu = ub - x0                 (SubspaceMin.h:154)   */
    LBFGSX_VS_Y = 5         /* vecy                                                   */
};
enum /* lbfgsx_b_wcombine modes: element-wise epilogue around (W_mask * coef)(i) */
{
    LBFGSX_CB_LINEAR = 0,   /* vecc = -W_F M (W'AA'd) + g_F   (BFGSMat.h:521 + SubspaceMin.h:155)        */
    LBFGSX_CB_SOLVE = 1,    /* vecy = v/theta + W_P coef/theta^2   (BFGSMat.h:535,564)                    */
    LBFGSX_CB_RHS_ADD = 2,  /* rhs += -W_P coef               (BFGSMat.h:592 + SubspaceMin.h:236-241)    */
    LBFGSX_CB_LAMBDA = 3,   /* lambda_L = -W_L coef + vecc_L + theta*vecy_L   (SubspaceMin.h:256-258)    */
    LBFGSX_CB_MU = 4        /* mu_U = -( -W_U coef + vecc_U + theta*vecy_U )  (SubspaceMin.h:265-267)    */
};
enum /* lbfgsx_b_sub_op */
{
    LBFGSX_SO_SAVE_FALLBACK = 0, LBFGSX_SO_RHS_INIT = 1, LBFGSX_SO_ASSIGN_Y = 2, LBFGSX_SO_CLAMP_Y = 3,
    LBFGSX_SO_CLAMP_FB = 4, LBFGSX_SO_ASSIGN_FB = 5
};
/* force_bounds: x = x.cwiseMax(lb).cwiseMin(ub)  (LBFGSB.h:55-58,128,240) */
int lbfgsx_b_force_bounds(lbfgsx_ctx* c);
/* the same statement where the generalized-Cauchy-point build follows at once (LBFGSB.h:240-241): nothing is launched,
 * the build's own pass -- which reads x, lb and ub anyway -- clamps on the way (a coordinate already inside its bounds
 * costs no store).  Any other entry of the bounded path called in between runs the statement first.  Same x, same bits. */
int lbfgsx_b_force_bounds_deferred(lbfgsx_ctx* c);
/* fx = f(x,grad); ||P(x-g,l,u)-x||_inf; x.x   (LBFGSB.h:137-138,146) */
int lbfgsx_b_eval(lbfgsx_ctx* c, int objective, double* fx, double* projgnorm, double* xnorm2);
/* the two reductions alone, for objectives evaluated by the caller (device / host functors) */
int lbfgsx_b_norms(lbfgsx_ctx* c, double* projgnorm, double* xnorm2);
/* dg = grad.dot(drt); step_max = max_step_size(x,drt,lb,ub)   (LBFGSB.h:68-86,176-179,195-196) */
int lbfgsx_b_dg_maxstep(lbfgsx_ctx* c, double* dg, double* step_max);
/* the same, and in the same pass the line search's first trial at step0 (the caller's min(1, max_step): LBFGSB.h:200-203 start
 * the search at min(1, step_max)): x_trial = xp + step0 * drt, f and grad there, grad.drt (LineSearchMoreThuente.h:261-262) --
 * kept inside the context and handed to the next lbfgsx_trial() iff it asks for this objective at exactly this step; any other
 * call drops them.  Built-in objectives on contexts with mapped outputs; everything else, LBFGSX_TRIAL_AHEAD=0 and the four
 * iterations after an unused trial behave as lbfgsx_b_dg_maxstep.  To be called right after lbfgsx_ls_begin. */
int lbfgsx_b_dg_maxstep_trial(lbfgsx_ctx* c, int objective, double step0, double* dg, double* step_max);
/* instrumentation: {trials evaluated ahead, of which the line search used} */
int lbfgsx_b_trial_ahead_counts(const lbfgsx_ctx* c, int64_t out[2]);
/* after the line search: proj_grad_norm, x.x, s, y (into the spare column), s.y, y.y  (LBFGSB.h:206,213,235-237) */
int lbfgsx_b_post_linesearch(lbfgsx_ctx* c, double* projgnorm, double* xnorm2, double* sy, double* yy);
/* the same, and in the same pass over x and g the element-wise part of the Cauchy search that follows when the iteration goes
 * on (Cauchy.h:95,111-129; what lbfgsx_b_cauchy_build_partial(c, tau, ...) launches first): that call then finds its
 * break points, d, xcp = x0 and counts ready -- provided nothing has moved x since, the threshold is the same and the
 * deferred x = clamp(x) (LBFGSB.h:240) has nothing to move; otherwise it runs its own pass.  LBFGSX_POST_BUILD=0, contexts
 * without mapped outputs and the integer Gram keep the two passes.  (Replaces nothing new in the reference: LBFGSB.h:206-241
 * in one sweep over the vectors instead of two.) */
int lbfgsx_b_post_linesearch_build(lbfgsx_ctx* c, double tau, double* projgnorm, double* xnorm2, double* sy, double* yy);
/* instrumentation, process-wide: {passes of lbfgsx_b_post_linesearch_build that carried the Cauchy half, Cauchy searches that
 * used it} */
int lbfgsx_b_post_build_counts(int64_t out[2], int reset);
/* Instrumentation of the short partial sort (round 5; no reference counterpart): out[0] = candidate lists of <= 4096 rows
 * (the break points below the search's threshold, Cauchy.h:183-199) ordered by one block (k_psel_sort_small) instead of three
 * launches.  LBFGSX_PSEL_SMALL=0 switches the one-block form off. */
int lbfgsx_b_psel_counts(int64_t out[1], int reset);
/* add_correction tail: sdots[j] = S_j.s_new, ydots[j] = Y_j.s_new for slots j < ncorr  (BFGSMat.h:111,138) */
int lbfgsx_b_correction_dots(lbfgsx_ctx* c, double* sdots, double* ydots);
/* ask the next lbfgsx_b_cauchy_build* to take those dots in the pass that computes W'd (Cauchy.h:152) -- the same 2c
 * columns, one read instead of two; lbfgsx_b_correction_dots then returns them without a launch.  Same sums, same
 * bits.  Without a following build (or with 4c > 40 reductions) lbfgsx_b_correction_dots computes them as before. */
int lbfgsx_b_correction_dots_defer(lbfgsx_ctx* c);
/* GCP build: break points, vecd, xcp = x0, radix sort of the finite positive break points; returns the counts
 * of free (brk = inf) and ordered coordinates, d.d, and the raw W'd dots [Y'd, S'd]  (Cauchy.h:93-133,152-154) */
int lbfgsx_b_cauchy_build(lbfgsx_ctx* c, int64_t* nfree, int64_t* nord, double* dd, double* wtd);
/* sorted break points [first, first+count): brk, g, z = bound - x0, index, W row [y_0..y_{c-1}, s_0..s_{c-1}]
 * for the sequential piecewise-quadratic scan kept on the host (Cauchy.h:183-256) */
int lbfgsx_b_cauchy_chunk(lbfgsx_ctx* c, int64_t first, int64_t count, double* brk, double* g, double* z, int* idx,
                          double* wrows);
/* lbfgsx_b_cauchy_build with a PARTIAL sort: only the candidates whose break point is <= tau are compacted (in
 * index order) and sorted -- in steady state a search crosses 10^2..10^3 of the ~n/2 candidates, so sorting all of
 * them (8 radix passes over n pairs) is the largest item of the build.  *nsorted = length of the sorted prefix
 * (== *nord when tau <= 0 or not finite: full sort).  Every break point <= tau is in the prefix, so the search is
 * exact as long as it stops before tau; the caller falls back to lbfgsx_b_cauchy_sort_full otherwise. */
int lbfgsx_b_cauchy_build_partial(lbfgsx_ctx* c, double tau, int64_t* nfree, int64_t* nord, int64_t* nsorted, double* dd,
                                  double* wtd);
int lbfgsx_b_cauchy_sort_full(lbfgsx_ctx* c);
/* Device form of the break-point search (reference Cauchy.h:183-256) over sorted positions [first, first+count) of
 * the list produced by lbfgsx_b_cauchy_build: three dependent prefix sums (p; c and f''; f') and a min-index exit
 * test, see lbfgspp_amd/csrc/gcp_scan.cuh.  Mmat: explicit 2c x 2c matrix of apply_Mv (BFGSMat.h:361-376), column
 * major; state_in = [p (2c), c (2c), f', f'']; t_prev = break point of the last crossing already processed (0 at
 * the start).  On return *exit_at = sorted index of the group end at which the search stops (-1: not inside this
 * range) and state_out = [p, c, f', f'', brk] after that crossing (after the last crossing of the range when -1).
 * 2c <= 80 (every m an L-BFGS-B context accepts); f32 problems are gathered into doubles and searched in double.
 * The order-sensitive scalar recurrences f', f'' and the exit test run in the reference's left-to-right order on the
 * host over per-crossing terms produced by the device (LBFGSX_GCP_CHAIN=scan: as tree-order prefix sums on the device). */
int lbfgsx_b_cauchy_scan(lbfgsx_ctx* ctx, int64_t first, int64_t count, int64_t nord, const double* Mmat, double theta,
                         double t_prev, const double* state_in, int64_t* exit_at, double* state_out);
/* xcp and the free / newly-active sets from the crossing threshold (Cauchy.h:201-206,219-233,265-282) */
int lbfgsx_b_cauchy_finish(lbfgsx_ctx* c, double t_cross, double tfinal, int crossed_all, int64_t* nact, int64_t* nfree);
/* Inspection entry (tests/test_cauchy_statements_gpu.py): copy one vector of the Cauchy search to the host -- the break points
 * or vecd (n elements of the context's scalar type), or the row numbers the last sort delivered (n int; only the first
 * nsorted of them mean anything).  Reads only: no pending statement is run, no flag of the context changes.
 * LBFGSX_E_INVALID for an unknown selector, a null pointer or a context that is not bounded. */
enum { LBFGSX_CV_BRK = 0, LBFGSX_CV_DVEC = 1, LBFGSX_CV_VALS_OUT = 2 };
int lbfgsx_b_cauchy_download(lbfgsx_ctx* c, int which, void* host);
/* drt = xcp - x0 (SubspaceMin.h:130) */
int lbfgsx_b_sub_begin(lbfgsx_ctx* c);
/* raw masked W'v: out[0..c) = Y_j.v, out[c..2c) = S_j.v over coordinates whose state has `mask` bits
 * (apply_Wtv / apply_WtPv, BFGSMat.h:315-320,382-430); nnz = non-zero entries of v inside the mask */
int lbfgsx_b_wtv(lbfgsx_ctx* c, int vsel, int mask, double* out, int64_t* nnz);
/* masked Gram of [Y_P, S_P] (2c x 2c, row-major, symmetric) for solve_PtBP (BFGSMat.h:543-556) */
int lbfgsx_b_gram(lbfgsx_ctx* c, int mask, double* gram);
/* the same Gram plus W_P'v (v = on-the-fly vector `vsel`, or -1) in ONE pass over the 2c columns: correctly rounded
 * double-double sums (the default kernels), or the exact integer-MFMA form with LBFGSX_GRAM=i8.  (Rounds 1-3 had a plain
 * f64 MFMA form behind this entry, LBFGSX_GRAM=mfma: ~1 ulp per entry, not exact, removed in round 4.)  Returns
 * LBFGSX_E_INVALID when the one-pass form does not apply -- callers then use lbfgsx_b_gram + lbfgsx_b_wtv. */
int lbfgsx_b_gram_fused(lbfgsx_ctx* c, int mask, int vsel, double* gram, double* wtv);
/* The same with the combine statement that produces v fused in as a prologue (one pass instead of two or three):
 *   LBFGSX_GP_RHS     rhs = (rhs + -(W_mask coef1)) + -(W_mask coef2), then v = -rhs   (two apply_PtBQv, BFGSMat.h:570-594;
 *                     a NULL coefficient vector skips its term)
 *   LBFGSX_GP_LINEAR  cF = -1 * (W_mask coef1) + g (coef1 NULL: cF = g), then v = -cF (compute_FtBAb, BFGSMat.h:486-522)
 * coef*: 2c doubles, logical order [Y slots, S slots] as for lbfgsx_b_wcombine.  Default Gram kernel only. */
enum { LBFGSX_GP_NONE = 0, LBFGSX_GP_RHS = 1, LBFGSX_GP_LINEAR = 2 };
int lbfgsx_b_gram_fused_ex(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                           double* gram, double* wtv);
/* The same pass that additionally returns the UN-ROUNDED double-double sums of the 2c x 2c block: gram_dd[2 e],
 * gram_dd[2 e + 1] = (hi, lo) of entry e = i (i + 1) / 2 + j (i >= j), 2c (2c + 1) doubles.  They let the caller form
 * the Gram of a subset through the complement identity  W_P'W_P = W_F'W_F - W_{F\P}'W_{F\P}: both sums are accurate to
 * ~2^-100 of sum |terms| in practice -- provably, and asserted against exact sums by tests/test_bounded_sums_gpu.py, to
 * 2 (k 2^-53)^2 sum |terms| over k rows (2^-69 at k = 3e5) --, so their difference rounds to the same double as the direct
 * sum unless that lies as close to a rounding boundary -- and in a BOXCQP sweep the complement
 * L u U holds 10^1..10^3 rows against |P| ~ n/2.  gram and wtv may be NULL.  Default Gram kernel only. */
int lbfgsx_b_gram_fused_dd(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                           double* gram, double* wtv, double* gram_dd);
/* The v row of lbfgsx_b_gram_fused_ex alone: the prologue statement on the rows of `mask`, then the raw masked
 * multi-dot wtv = [Y_mask'v, S_mask'v] -- the Gram kernel with one pair per lane instead of all of them. 1 <= 2c <= 30. */
int lbfgsx_b_wtv_prologue(lbfgsx_ctx* c, int mask, int vsel_id, int prologue, const double* coef1, const double* coef2,
                          double* wtv);
/* lbfgsx_b_wcombine(LBFGSX_CB_SOLVE, pmask, vsel, coef, theta) fused with the raw masked multi-dot
 * wty = [Y_F' y, S_F' y] over `fmask` (pmask must be a subset of fmask): the solve result of solve_PtBP
 * (BFGSMat.h:564) and the W_F' y the multipliers need (SubspaceMin.h:249-254, apply_WtPv BFGSMat.h:382-430) in one
 * pass.  coef may be NULL (y = v/theta).  1 <= 2c <= 32, LBFGSX_E_INVALID otherwise. */
int lbfgsx_b_solve_wty(lbfgsx_ctx* c, int pmask, int vsel, const double* coef, double theta, int fmask, double* wty);
/* masked combine with element-wise epilogue, see LBFGSX_CB_*; coef = NULL means "W term absent" */
int lbfgsx_b_wcombine(lbfgsx_ctx* c, int mode, int mask, int vsel, const double* coef, double theta);
/* BOXCQP partition of the free set into L/U/P with the value/multiplier updates (SubspaceMin.h:194-219) */
int lbfgsx_b_sub_partition(lbfgsx_ctx* c, int64_t* nL, int64_t* nU, int64_t* nP);
/* counts = {#F outside [l,u], #P outside [l,u], #L with lambda<0, #U with mu<0}  (SubspaceMin.h:60-108) */
int lbfgsx_b_sub_check(lbfgsx_ctx* c, int64_t counts[4]);
/* the element-wise statements between two BOXCQP solves in ONE pass: first != 0: LBFGSX_SO_SAVE_FALLBACK
 * (SubspaceMin.h:170-172) with counts[0] = #F outside [l,u] (the in_bounds test of the first solve, :162; when it is 0
 * the pass has moved no value of y), else the counts[1..3] of lbfgsx_b_sub_check on the current values; then
 * lbfgsx_b_sub_partition (:194-219) and LBFGSX_SO_RHS_INIT (:232).  Bit for bit the calls it replaces. */
int lbfgsx_b_sub_sweep_begin(lbfgsx_ctx* c, int first, int64_t* nL, int64_t* nU, int64_t* nP, int64_t counts[4]);
/* lbfgsx_b_wtv(LBFGSX_VS_LBOUND, LBFGSX_ST_L) and lbfgsx_b_wtv(LBFGSX_VS_UBOUND, LBFGSX_ST_U) -- the inner products of the two
 * apply_PtBQv statements of a BOXCQP sweep (SubspaceMin.h:236-241, BFGSMat.h:570-594) -- in one launch over the index list of
 * L u U.  LBFGSX_E_INVALID when there is no list or 2c is outside 1..80 (LBFGSX_SPLIT=0: 1..24): call lbfgsx_b_wtv per set. */
int lbfgsx_b_wtv_lu(lbfgsx_ctx* c, double* out_l, int64_t* nnz_l, double* out_u, int64_t* nnz_u);
/* the same, plus negc_dd[2 k], [2 k + 1] = the un-rounded (hi, lo) sum of column k of W_{L u U}'(-c) (c = vecc of
 * SubspaceMin.h on the rows of L u U); negc_dd[0] = NaN when this context cannot deliver it (LBFGSX_RHS_IDENTITY=0, no
 * split-row kernels, no mapped outputs) */
int lbfgsx_b_wtv_lu_c(lbfgsx_ctx* c, double* out_l, int64_t* nnz_l, double* out_u, int64_t* nnz_u, double* negc_dd);
/* ---- pieces of the carried Gram of the free set (BFGSMatB::solve_PtBP): W_F'W_F of one iteration from that of the one
 * before -- the entries of the columns add_correction replaced computed afresh, the others corrected by the outer products
 * of the rows that entered or left F.  All sums un-rounded double-doubles (hi, lo).
 *
 * lbfgsx_b_free_delta: the rows whose membership of F (LBFGSX_ST_FREE) differs from what it was at the previous call (the
 * first call: from the empty set) are put on two lists, their sizes returned (-1: more rows than the list
 * holds -- n / 64 of them, at least 2^14 and at most 2^20 -- so it is not usable); the remembered set becomes the current one. */
int lbfgsx_b_free_delta(lbfgsx_ctx* c, int64_t* n_enter, int64_t* n_leave);
/* the 2c x 2c Gram of [Y S] over the rows of one of those lists (0: entered, 1: left), packed lower triangle
 * e = i (i + 1) / 2 + j as lbfgsx_b_gram_fused_dd returns it; LBFGSX_E_INVALID for an empty or overflowed list */
int lbfgsx_b_gram_list_dd(lbfgsx_ctx* c, int which, double* gram_dd);
/* selected entries of [Y_P S_P v]'[Y_P S_P v] in one pass with the prologue of lbfgsx_b_gram_fused_ex: entry e is the
 * product of the columns pair_i[e], pair_j[e] (0..2c-1: Y slots then S slots; 2c: v), at most lbfgsx_b_gram_pairs_max()
 * of them; out_dd[2 e], out_dd[2 e + 1] = (hi, lo).  Writes the compact copy of the free rows
 * under the conditions of lbfgsx_b_set_compaction. */
int lbfgsx_b_gram_pairs_dd(lbfgsx_ctx* c, int mask, int vsel, int prologue, const double* coef1, const double* coef2,
                           int npairs, const int* pair_i, const int* pair_j, int refresh_slot, double* out_dd);
/* how many entries one lbfgsx_b_gram_pairs_dd call serves with the current history: 3 (2c + 1) -- the v row and the rows of
 * two columns, whatever 2c <= 80 is (kernels of csrc/lbfgsb_x.cuh) -- or, with LBFGSX_SPLIT=0, the 64 of the round-3
 * one-entry-per-lane kernel while 2c + 1 <= 31; 0: the call is not available for this history */
int lbfgsx_b_gram_pairs_max(lbfgsx_ctx* c);
/* the un-rounded (hi, lo) sums of the v row W_P'v of the one-pass Gram this context ran last (lbfgsx_b_gram_fused_dd with a
 * vector selector, not a list): out_dd[2 k], [2 k + 1] for column k < 2c.
 * LBFGSX_E_INVALID when there is none.  BFGSMatB::solve_PtBP keeps W_F'(-c) of a first solve that took the full pass, so
 * that its sweeps can form W_P' rhs on the host (see lbfgsx_b_solve_sweep_rhs). */
int lbfgsx_b_gram_last_vrow_dd(lbfgsx_ctx* c, double* out_dd);
/* refresh_slot >= -1: the caller vouches that since the previous subspace minimisation the history changed in at most the
 * storage slot `refresh_slot` (-1: not at all) and that lbfgsx_b_free_delta has been called for the current free set.  The
 * pass may then read the compact copy of the free rows it KEPT from that minimisation (rows that entered F were appended by
 * lbfgsx_b_free_delta, rows that left are skipped through their state byte) and only rewrites the two columns of that slot
 * in it, instead of reading every row of the 2c columns through the mask and writing the copy afresh.  -2: never. */
/* Hint for the subspace minimisation that lbfgsx_b_sub_begin has just opened (which clears it): BOXCQP sweeps are expected,
 * so the full Gram pass of the first solve (lbfgsx_b_gram_fused_dd over LBFGSX_ST_FREE) may also write a compact copy of the
 * free rows of [Y S], and the passes of the sweeps (lbfgsx_b_wtv_prologue, lbfgsx_b_solve_sweep, the complement Grams) then
 * read that copy instead of fetching all n rows through the state-byte mask.  Same sums (double-double), same bits; only
 * taken when the free set leaves out at least an eighth of the rows.  LBFGSX_COMPACT_FREE=0 disables it.  The copy is
 * valid until the next lbfgsx_b_sub_begin / lbfgsx_b_cauchy_finish; the history must not change in between. */
int lbfgsx_b_set_compaction(lbfgsx_ctx* c, int enable);
/* Compact vectors (round 3).  While lbfgsx_b_solve_sweep / _lu_sweep / _wtv_lu / _wtv_prologue and the L u U complement of
 * lbfgsx_b_gram_fused_dd sweep over the compact copy, vecy, yfallback, lambda, mu, rhs, c_F, l - x0, u - x0 and the
 * partition bits of the free rows (SubspaceMin.h:159-268) sit at the rows' POSITIONS in the copy (contiguous) instead of at
 * the rows; lbfgsx_b_sub_op(LBFGSX_SO_ASSIGN_Y) assigns the result from there, any other entry of the bounded path first
 * puts them back at their rows.  Same statements on the same values: no bit changes.  LBFGSX_COMPACT_VEC=0 keeps the
 * vectors at their rows.
 * The kept copy also serves the Cauchy search (round 3): p = W'd (Cauchy.h:152) and the deferred dots of add_correction
 * (BFGSMat.h:111,138) are sums over the rows where d or s_new is not zero -- the positions of the copy plus a short list of
 * other rows that lbfgsx_b_cauchy_build* writes on its way -- instead of over all n rows (LBFGSX_WTD_COMPACT=0: all rows).
 * Instrumentation, process-wide: out = {minimisations that ran on compact vectors, times they were put back before the
 * result was assigned, Cauchy searches whose W'd came from the copy, Grams over index lists that were launched behind the
 * pass before them and cost no round trip of their own (LBFGSX_SYNC_MERGE=0: none)}. */
int lbfgsx_b_compact_vec_counts(int64_t out[4], int reset);
/* Setup: allocates now what the bounded path allocates on first use -- the buffers of the device break-point search, of the
 * partial sort and of the free-set delta, the compact copy of the free rows and its vectors -- so that a solve on a prepared
 * context (LBFGSBSolver::prepare_resident) contains no allocation.  Optional: without it the first iterations allocate
 * (a few milliseconds at n = 10^7).  The optional work sets are skipped silently when there is no room for them. */
int lbfgsx_b_reserve(lbfgsx_ctx* c);
/* A BOXCQP solve and the statements of lbfgsx_b_sub_sweep_begin on the rows it writes, in ONE pass (the solve's row of W is
 * in registers; the sweep's pass over n rows disappears).  Bit for bit lbfgsx_b_wcombine(LBFGSX_CB_SOLVE) /
 * lbfgsx_b_solve_wty followed by lbfgsx_b_sub_sweep_begin.
 *   first != 0: y = v/theta + (W coef)/theta^2 on every free row (SubspaceMin.h:159), then the first sweep's statements;
 *               sums = {#L, #U, #P, #F outside, 0, 0, 0}; wty is not written.
 *   first == 0: y on the rows of P (:243) and wty = W_F'y as lbfgsx_b_solve_wty, then the next sweep's statements on the
 *               rows of P (their multipliers are zero); sums = {#L, #U, #P, 0, #P outside, 0, 0} over those rows.  The
 *               rows of the old L and U follow in lbfgsx_b_lu_sweep, which needs the multipliers' coefficients the caller
 *               derives from wty; the totals are the sums of the two calls.  Needs the index list of L u U that the
 *               previous sweep kept (small sets).
 * vsel: the selector of the ONE vector v solved for (LBFGSX_VS_NEG_CF, LBFGSX_VS_NEG_RHS, ...); LBFGSX_VS_LBOUND / _UBOUND
 * (the bound vectors of lbfgsx_b_wtv_lu) are refused.
 * LBFGSX_E_INVALID when the fused form does not apply here (2c > 80, no list, LBFGSX_SWEEP_SOLVE_FUSE=0, a bound selector):
 * nothing has been changed, run the separate calls.
 * After LBFGSX_SO_ASSIGN_Y has run on live compact vectors the partition bits (LBFGSX_ST_P / _L / _U) of the state byte
 * are not written back (only the free / active bits are read afterwards): lbfgsx_b_download_state returns them undefined. */
int lbfgsx_b_solve_sweep(lbfgsx_ctx* c, int first, int vsel, const double* coef, double theta, double* wty, int64_t sums[7]);
/* the same with the two rhs updates that precede a sweep's solve (SubspaceMin.h:236-241; the LBFGSX_GP_RHS prologue of
 * lbfgsx_b_wtv_prologue with these coefficients) evaluated by the solve's own pass on the W rows it holds: first = 0 and
 * vsel = LBFGSX_VS_NEG_RHS only, split-row kernels only.  The caller then needs W_P'(-rhs) from elsewhere -- BFGSMatB::solve_PtBP
 * forms it from sums it holds (W_F'(-c), W_{L u U}'(-c) of lbfgsx_b_wtv_lu_c, the Gram of the complement identity) -- and the pass
 * over P that lbfgsx_b_wtv_prologue makes for it is saved.  _ready: 1 when this context can do it now. */
int lbfgsx_b_solve_sweep_rhs(lbfgsx_ctx* c, int first, int vsel, const double* coef, double theta, const double* rhs_c1,
                             const double* rhs_c2, double* wty, int64_t sums[7]);
int lbfgsx_b_solve_sweep_rhs_ready(lbfgsx_ctx* c);
/* completes lbfgsx_b_solve_sweep(first == 0): lambda on the rows of L, mu on the rows of U (SubspaceMin.h:256-267, the two
 * lbfgsx_b_wcombine calls) and the sweep's statements on those rows, walking the index list;
 * sums = {#L, #U, #P, 0, 0, #L with lambda < 0, #U with mu < 0} over those rows */
int lbfgsx_b_lu_sweep(lbfgsx_ctx* c, const double* coef, double theta, int64_t sums[7]);
/* element-wise statements of SubspaceMin.h selected by LBFGSX_SO_* */
int lbfgsx_b_sub_op(lbfgsx_ctx* c, int op);
/* copy the per-coordinate state byte (LBFGSX_ST_* bits) to the host: n bytes */
int lbfgsx_b_download_state(lbfgsx_ctx* c, unsigned char* host);
/* Inspection entries (tests/test_subspace_statements_gpu.py): copy one vector of the subspace minimisation -- n elements of
 * the context's scalar type -- to or from the host.  Like any other entry of the bounded path they first put live compact
 * vectors back at their rows.  LBFGSX_E_INVALID for an unknown selector, a null pointer or a context that is not bounded. */
enum { LBFGSX_SV_CF = 0, LBFGSX_SV_Y = 1, LBFGSX_SV_YFB = 2, LBFGSX_SV_LAM = 3, LBFGSX_SV_MU = 4, LBFGSX_SV_RHS = 5 };
int lbfgsx_b_sub_download(lbfgsx_ctx* c, int which, void* host);
int lbfgsx_b_sub_upload(lbfgsx_ctx* c, int which, const void* host);
/* the current index list of L u U (rows in arrival order): *count entries copied to rows[0..cap); *count = -1 and nothing
 * copied when the context holds no valid list; LBFGSX_E_INVALID when cap is too small.  Changes nothing: the list, a pending
 * lbfgsx_b_lu_sweep and live compact vectors stay as they are, so it may be called between lbfgsx_b_solve_sweep(first = 0)
 * and lbfgsx_b_lu_sweep. */
int lbfgsx_b_lu_list_download(lbfgsx_ctx* c, int* rows, int64_t cap, int64_t* count);
/* drt.dot(g) (SubspaceMin.h:281,289) */
int lbfgsx_b_dot_drt_g(lbfgsx_ctx* c, double* dg);
/* drt = xcp - x [, drt.normalize()]  (LBFGSB.h:163-164,191) */
int lbfgsx_b_dir_from_xcp(lbfgsx_ctx* c, int normalize);

/* ---- lock-step batch (BASELINE.json cfg5) ------------------------------------------------------------
 * P independent problems of equal dimension advance together: one kernel launch per reference statement for the
 * whole batch, grid = (chunks, problems), per-problem scalars / reduction workspace / buffer roles / history ring.
 * The host (include/LBFGSBatched.h) keeps one line-search state machine per problem and fills one descriptor per
 * problem and launch.  No reference counterpart (the reference solves one problem per call); per problem the
 * arithmetic is that of LBFGS.h:78-173 with LineSearchMoreThuente. */
typedef struct lbfgsx_batch lbfgsx_batch;
typedef struct
{
    int active;   /* 0: this problem sits out of the launch */
    int mode;     /* two-loop step kind: 0 INIT q=a*g, 1 SUB q-=alpha*y, 2 SUBDIV (q-alpha*y)/theta, 3 ADD q+=(alpha-beta)*s */
    int x_in;     /* point index (0..2): xp for a trial / post, the current point for eval / two-loop */
    int x_out;    /* point index written by a trial; the accepted point for post */
    int col_u;    /* physical history column of the update vector (post: the spare column to fill) */
    int col_w;    /* physical history column of the dot product, -1 = gradient at x_in */
    int i_num, i_den, i_num2, i_theta, i_out; /* indices into the problem's scalar table */
    float pad;
    double step;  /* trial step, or the scale a of the two-loop INIT */
} lbfgsx_bat_desc;
enum
{
    LBFGSX_BAT_EVAL = 0, LBFGSX_BAT_TRIAL = 1, LBFGSX_BAT_POST = 2, LBFGSX_BAT_TWOLOOP = 3,
    /* a user objective evaluated by the caller over the whole batch: the trial point alone (x_out = x_in + step * drt),
     * then -- after the caller's kernels have written f and grad of every active problem -- grad(x_out) . drt, or, after
     * the first evaluation, grad . grad and x . x at x_in */
    LBFGSX_BAT_POINT = 4, LBFGSX_BAT_GDOT = 5, LBFGSX_BAT_NORMS = 6
};
/* per-problem description of a whole apply_Hv (BFGSMat.h:276-302): d = -H grad(x_in), with the history columns
 * pcol[0..ncorr) newest -> oldest (physical column ids) */
typedef struct
{
    int active;
    int x_in;   /* which of the 3 points holds the gradient */
    int ncorr;
    int pcol[32];
} lbfgsx_bat_hvdesc;
/* per-problem description of a whole lock-step iteration (lbfgsx_bat_iterate) */
enum
{
    LBFGSX_BAT_IT_POST = 1,      /* the statements after a finished line search first (xp -> cur, pair into column `spare`) */
    LBFGSX_BAT_IT_POST_ONLY = 2, /* ... and nothing else: the caller already knows that this problem stops */
    LBFGSX_BAT_IT_TRIAL = 4,     /* the first trial of the next line search last (built-in objectives only) */
    LBFGSX_BAT_IT_TRIAL_ONLY = 8 /* nothing but a further trial of a search that goes on: x_trial = x(xp) + step * drt (drt as
                                  * the launch that opened the search left it), results 5 and 6.  Lets problems at different
                                  * points of their iteration share the launch */
};
#define LBFGSX_BAT_NRES 8        /* doubles per problem in the result table of a launch */
typedef struct
{
    int active;
    int flags;    /* LBFGSX_BAT_IT_* */
    int cur;      /* point (0..2) holding the accepted iterate and its gradient */
    int xp;       /* POST: the point the finished line search started from */
    int trial;    /* TRIAL: the point that receives cur + step * drt and the gradient there */
    int ncorr;    /* pairs stored BEFORE this launch */
    int spare;    /* POST: physical column that receives (s, y) */
    int pad;
    double step;  /* TRIAL: the step */
    int pcol[32]; /* physical columns of the stored pairs, newest -> oldest */
} lbfgsx_bat_itdesc;
/* history lengths: the reference puts no upper bound on m (Param.h:350-376); here
 *   LBFGSX_MAX_M_BOUNDED  an L-BFGS-B context passes the 2c coefficients of a W product in kernel arguments (80 slots) and keeps
 *                         the host's 2c-vectors in arrays of that size: lbfgsx_create(LBFGSX_FLAG_BOUNDED) refuses m > 40
 *                         (tests/test_lbfgsb_gpu.py: trajectories at m = 40, the refusal at 41);
 *   LBFGSX_MAX_M_BATCH    the lock-step batch's descriptors carry 32 column ids: lbfgsx_bat_create refuses m > 31;
 * unconstrained L-BFGS contexts take any m (the persistent one-launch recursion describes up to 128 pairs, beyond that the
 * step launches run). */
#define LBFGSX_MAX_M_BOUNDED 40
#define LBFGSX_MAX_M_BATCH 31
int lbfgsx_bat_create(lbfgsx_batch** out, int dtype, int64_t n, int m, int nproblems, int device);
void lbfgsx_bat_destroy(lbfgsx_batch* c);
/* a created batch made ready for another set of problems of the same shape (scalars and counters cleared, nothing
 * re-allocated): what lets a caller keep the ~(2m+9) n P elements of one batch alive across minimisations */
int lbfgsx_bat_reset(lbfgsx_batch* c);
/* index of a scalar inside a problem's table: kind 0 = ys[col], 1 = theta[col], 2 = two-loop dot k, 3 = output k */
int lbfgsx_bat_scalar_index(const lbfgsx_batch* c, int kind, int k);
/* x0 of problem p (point 0) = extended-Rosenbrock start for seed seed0 + p */
int lbfgsx_bat_gen_rosen_x0(lbfgsx_batch* c, uint64_t seed0);
/* the diagonal quadratics of seeds seed0 + p (a, b as lbfgsx_gen_diag_quad makes them for one problem) and x0 = 0 */
int lbfgsx_bat_gen_diag_quad(lbfgsx_batch* c, double kappa, uint64_t seed0);
/* device pointers into the batch for code that evaluates its own objective: kind 0 = x, 1 = grad of `point` (0..2) of
 * `problem`, 2 = its search direction; consecutive problems of one point lie lbfgsx_bat_ld() elements apart.  The
 * caller's kernels must be ordered after the library's on lbfgsx_bat_stream() (launch there, or synchronise). */
void* lbfgsx_bat_vec(lbfgsx_batch* c, int kind, int point, int problem);
int64_t lbfgsx_bat_ld(const lbfgsx_batch* c);
void* lbfgsx_bat_stream(lbfgsx_batch* c);
/* one launch for the whole batch; desc = P descriptors; then out[p*nout + k] = scalar (desc[p].i_out + k) */
int lbfgsx_bat_launch(lbfgsx_batch* c, int kind, int objective, const lbfgsx_bat_desc* desc, int nout, double* out);
/* The whole two-loop recursion of every active problem in ONE launch: one 256-thread block per problem keeps its q
 * vector in registers across the 2c+1 steps (block-level reductions only, no grid synchronisation), so the history
 * is read once and q never travels: (4c+2) n elements instead of (8c+1) n.  Same element-wise arithmetic and
 * order-independent reductions as the step kernels, hence bit-identical results.  The final dot (grad . d) lands in
 * scalar dot(2*ncorr) of each problem, as after the step-wise sequence.  Applicable when the vector fits the block's
 * registers (n a multiple of the 16-byte vector width and n <= 256 * 98 * width: 100352 floats / 50176 doubles);
 * LBFGSX_E_INVALID otherwise -- the caller then issues the LBFGSX_BAT_TWOLOOP steps. */
int lbfgsx_bat_apply_Hv(lbfgsx_batch* c, const lbfgsx_bat_hvdesc* desc);
/* ONE launch per lock-step iteration: for every active problem, one 256-thread block runs
 *   [POST]   s = x - xp, y = grad - gradp into the spare column; grad.grad, x.x, s.y, y.y      (LBFGS.h:130,137,159-161)
 *            and decides add_correction's test s.y > eps * y.y itself (LBFGS.h:161, BFGSMat.h:83-97)
 *   always   drt = -H grad by the two-loop recursion over the history that results (BFGSMat.h:276-302), the direction
 *            held in registers / LDS from the first statement to the last; grad . drt
 *   [TRIAL]  x_trial = x + step * drt, f and grad there, grad_trial . drt   (LineSearchMoreThuente.h:412-414,
 *            LineSearchNocedalWright.h:146-148) -- the first trial of the next line search, whose step the caller knows
 * with the element-wise arithmetic and the order-independent sums of the statement-wise launches, hence the same bits.
 * out[p * LBFGSX_BAT_NRES + k], k = 0..6: grad.grad, x.x, s.y, y.y (POST), grad.drt, f_trial, grad_trial.drt (TRIAL).
 * The caller's host logic stays the reference's: it reads the sums, applies the stopping tests (a problem that stops has
 * had its direction and trial computed in vain, nothing else), rotates the ring when s.y > eps * y.y, and feeds the trial to the
 * line search it starts.  A problem longer than one block's registers hold (100 352 floats / 50 176 doubles) is split over
 * 2..16 consecutive blocks, each with its share of the direction resident, and the blocks exchange their partial sums at every
 * step (n up to 1 605 632 floats / 802 816 doubles, a multiple of the 16-byte vector width; m <= 31): lbfgsx_bat_iterate_ok.
 * LBFGSX_E_INVALID otherwise -- the caller then issues the statement-wise launches.  LBFGSX_E_RUNTIME: the blocks of a split
 * problem were not resident together within 100 ms (something else held the CUs); no sums are returned -- a part that gives up
 * stops publishing and sets the launch's error word, its siblings give up on seeing it, the reporting part checks the word
 * (environment LBFGSX_BAT_DEBUG_XCH_FAULT=k at lbfgsx_bat_create: the k-th such launch of the batch behaves like that). */
int lbfgsx_bat_iterate(lbfgsx_batch* c, int objective, const lbfgsx_bat_itdesc* desc, double* out);
int lbfgsx_bat_iterate_ok(const lbfgsx_batch* c);
/* instrumentation: enable != 0 brackets every launch of the batch with a pair of events; lbfgsx_bat_timing_read waits for
 * the stream and returns {sum of the launches' durations in ms, launches, host waits, waits that timed out} since the
 * last read */
int lbfgsx_bat_timing(lbfgsx_batch* c, int enable);
int lbfgsx_bat_timing_read(lbfgsx_batch* c, double out[4]);
/* out[p] = scalar idx[p] of problem p */
int lbfgsx_bat_fetch(lbfgsx_batch* c, const int* idx, double* out);
int lbfgsx_bat_download_x(lbfgsx_batch* c, int p, int point, void* host);
int lbfgsx_bat_sync(lbfgsx_batch* c);
/* ---- a user objective that sees the batch as ONE packed array (lbfgsx_lockstep_minimize_fn, include/lbfgsx_solver.h) ----
 * The trial of problem p lives in its own point slot (desc[p].x_out), a different one per problem, so the rows of the
 * evaluating problems are neither adjacent nor in one slot.  These two launches replace LBFGSX_BAT_POINT and LBFGSX_BAT_GDOT
 * around the caller's evaluation and keep a packed copy: row k (lbfgsx_bat_ld() elements apart) of lbfgsx_bat_packed(c, 0)
 * holds the trial point of the k-th evaluating problem, row k of lbfgsx_bat_packed(c, 1) receives its gradient.
 *   lbfgsx_bat_pack    for every active p: x(x_out) = x(x_in) + step * drt, written to the point slot AND to packed row
 *                      desc[p].col_u in the same pass (one read of xp and of drt, two writes): 4 n elements per problem
 *   lbfgsx_bat_unpack  for every active p: packed gradient row desc[p].col_u -> gradient slot of x_out, and grad . drt
 *                      formed in that pass (one read of the row and of drt, one write: 3 n elements); out[p] = that sum,
 *                      the bits LBFGSX_BAT_GDOT returns for the same gradient (same accumulators, csrc/reduce.cuh)
 * Both refuse a descriptor table whose active entries name a point outside 0..2, x_in == x_out, a row outside 0..P-1, one
 * row twice or a scalar index outside the table (LBFGSX_E_INVALID, nothing launched).  lbfgsx_bat_packed allocates the two
 * arrays on first use (2 P ld elements) and returns NULL when it cannot.  lbfgsx_bat_set_x0 places P start points (src:
 * P x n elements, row-major, host or device memory) in point 0.  lbfgsx_bat_device_push makes the batch's device current
 * for the calling thread as lbfgsx_device_push does for a context (undo with lbfgsx_device_pop). */
void* lbfgsx_bat_packed(lbfgsx_batch* c, int kind);
int lbfgsx_bat_pack(lbfgsx_batch* c, const lbfgsx_bat_desc* desc);
int lbfgsx_bat_unpack(lbfgsx_batch* c, const lbfgsx_bat_desc* desc, double* out);
int lbfgsx_bat_set_x0(lbfgsx_batch* c, const void* src);
int lbfgsx_bat_device_push(const lbfgsx_batch* c, int* prev);

/* ---- the exchange step of the batched mode over RCCL --------------------------------------
 * After a batch has been sharded over the GPUs of a node (lbfgsx_batch_minimize_lockstep_multi in lbfgsx_solver.h, or one
 * process per GPU) the only data that crosses devices are the per-problem result records.  This call leaves ALL `count`
 * records (rec_bytes each, in problem-id order, given in host memory as the solver returned them) on EVERY listed device:
 * device r contributes its contiguous block, one grouped ncclAllGather over xGMI moves the blocks, dev_out[r] receives a
 * device buffer on devices[r] (release it with lbfgsx_device_free).  One rank per GPU: a device listed twice is refused.
 * RCCL is loaded with dlopen on first use.  No reference counterpart (the reference solves one problem per call). */
int lbfgsx_rccl_allgather_records(const int* devices, int ndev, const void* records, int64_t count, int64_t rec_bytes,
                                  void** dev_out);
/* ---- the sum over the row shards of ONE problem, natively over RCCL --------------------------------
 * A problem whose rows are spread over several GPUs (lbfgsx_set_shard) needs every n-length sum of the driver -- the
 * reference's fx, grad.dot(drt), grad.norm(), x.norm(), s.y, y.y (LBFGS.h:92,123,130,161) and the 6m + 7 sums of the
 * Gram-space pass -- added over the shards before any scalar logic runs.  lbfgsx_comm_allreduce_sum does that for one
 * rank's small bundle of doubles (<= 512): device buffer, ONE ncclAllReduce(sum, f64) over xGMI on the rank's stream,
 * result back in `buf`; every rank gets the same bits.  Communicators:
 *   lbfgsx_comm_create_local  all ranks in THIS process, one host thread per device (ncclCommInitAll).  A device listed
 *                             twice cannot be two RCCL ranks: the sums are then formed in host memory, in rank order,
 *                             behind a barrier (the emulation a one-GPU box runs; lbfgsx_comm_info tells which);
 *   lbfgsx_comm_create_rank   one rank of a multi-process communicator (ncclCommInitRank; the id comes from
 *                             lbfgsx_comm_unique_id on one rank and travels through the caller's launcher).
 * Every rank must make the same sequence of calls (as with any collective).  lbfgsx_comm_abort releases ranks that wait
 * for one that failed.  RCCL is loaded with dlopen on first use.  No reference counterpart. */
typedef struct lbfgsx_comm lbfgsx_comm;
int lbfgsx_comm_unique_id(unsigned char id[128]);
int lbfgsx_comm_create_rank(lbfgsx_comm** out, int device, int rank, int nranks, const unsigned char id[128]);
int lbfgsx_comm_create_local(lbfgsx_comm** out, const int* devices, int ndev);
int lbfgsx_comm_allreduce_sum(lbfgsx_comm* comm, int local_rank, double* buf, int count);
int lbfgsx_comm_abort(lbfgsx_comm* comm);
/* the same, remembering WHICH local rank failed first (the one whose error is the root cause; the others then fail with
 * "aborted by another rank"): lbfgsx_comm_first_abort returns it, -1 when nobody called lbfgsx_comm_abort_from.  A rank of
 * another PROCESS that dies cannot call either: the surviving ranks leave their wait through RCCL's asynchronous error or
 * after LBFGSX_COMM_TIMEOUT_S seconds (default 300) and abort their own communicator. */
int lbfgsx_comm_abort_from(lbfgsx_comm* comm, int local_rank);
int lbfgsx_comm_first_abort(const lbfgsx_comm* comm);
/* info = {ranks, ranks driven by this process, 1 when RCCL carries the sums (0: host emulation), RCCL version code} */
int lbfgsx_comm_info(const lbfgsx_comm* comm, int info[4]);
int64_t lbfgsx_comm_calls(const lbfgsx_comm* comm, int local_rank);
/* the all-reduce as the callback LBFGSSolver::set_reducer / lbfgsx_solver_set_allreduce take: pass
 * lbfgsx_comm_allreduce_hook with user = lbfgsx_comm_hook_arg(comm, local_rank) (owned by the communicator) */
void* lbfgsx_comm_hook_arg(lbfgsx_comm* comm, int local_rank);
void lbfgsx_comm_allreduce_hook(double* buf, int count, void* hook_arg);
void lbfgsx_comm_destroy(lbfgsx_comm* comm);
int lbfgsx_device_download(int device, const void* dev_ptr, int64_t bytes, void* host);
void lbfgsx_device_free(int device, void* dev_ptr);

/* ---- instrumentation ----------------------------------------------------------------------------------*/
/* average duration (ms) of the two-loop step kernels since the last reset, measured with HIP events on
 * the context's stream; count = number of timed launches.  on = 2: one event pair per apply_Hv only (the step launches
 * then run back to back, without an event between them) and the per-step figures are that time / (2c+1) */
int lbfgsx_timing_enable(lbfgsx_ctx* c, int on);
int lbfgsx_timing_read(lbfgsx_ctx* c, double* twoloop_ms_total, int64_t* twoloop_launches,
                       double* applyhv_ms_total, int64_t* applyhv_calls);
/* number of apply_Hv calls of this context served by the persistent one-launch kernel (k_twoloop_persist: the
 * whole recursion in one launch of occupancy x CUs blocks with part of q resident on the CUs).  It is used when
 * m <= 128 and LBFGSX_PERSIST != 0, one such kernel per device at a time within the process (a per-device lock taken
 * for the launch; a context that finds it taken issues its 2c+1 step launches for that call, as does one whose launch
 * timed out because another process shares the GPU).  Results are bit-identical either way. */
int64_t lbfgsx_persistent_launches(const lbfgsx_ctx* c);
/* of the apply_Hv calls timed since lbfgsx_timing_enable, how many were persistent launches that also carried the post
 * statements (lbfgsx_post_linesearch_spec): their algorithmic bytes are (8c+1) n for the product plus 6n - 2n for K3 */
int64_t lbfgsx_timing_fused_launches(const lbfgsx_ctx* c);
/* elements of q (= the direction vector, BFGSMat.h:283-301 `res`) that a persistent launch of this context keeps in the
 * registers / LDS of the CUs for the whole recursion: that share of q's traffic never reaches HBM (0: not available) */
int64_t lbfgsx_persistent_resident_elems(const lbfgsx_ctx* c);
/* Diagnostic: runs the grid-wide reduction every kernel of the path ends in (csrc/reduce.cuh) on `nred` sums of known small
 * integers over `grid` blocks of 256 threads; out[r] = the total of sum r, which the caller checks against the closed
 * form: sum over g < 256 grid of (r + 1)(1 + g mod 7) + (block(g) mod 3) + (1000003 r mod 17).  nred in {1 2 3 5 7 8 9 25 31
 * 33 40 50 56}; f32_accumulators != 0 uses the accumulator type of f32 contexts. */
int lbfgsx_selftest_reduce(lbfgsx_ctx* c, int nred, int grid, int f32_accumulators, double* out);
/* STREAM-style device bandwidth probe on this context's vectors: copy (XT = X) and triad, GB/s */
int lbfgsx_stream_probe(lbfgsx_ctx* c, int reps, double* copy_gbs, double* triad_gbs);

#ifdef __cplusplus
}
#endif
#endif /* LBFGSX_H */
