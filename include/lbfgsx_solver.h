/* include/lbfgsx_solver.h -- C ABI of liblbfgsx_solver.so: the drop-in C++ solvers (include/LBFGS.h,
 * include/LBFGSB.h) instantiated for the built-in device objectives and for a caller-supplied objective on device
 * memory (lbfgsx_solver_minimize_fn, lbfgsx_lockstep_minimize_fn), for callers without a C++ compiler
 * (ctypes / cgo / JNI ...).  Mirrors LBFGSSolver<T, LineSearch>::minimize (reference LBFGS.h:78-173) and
 * LBFGSBSolver<T>::minimize (reference LBFGSB.h:116-262): same parameters (LBFGSParam / LBFGSBParam fields),
 * same return value (iteration count), exceptions mapped to status codes + message.
 */
#ifndef LBFGSX_SOLVER_H
#define LBFGSX_SOLVER_H

#include <stdint.h>

#include "lbfgsx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    LBFGSX_LS_NOCEDAL_WRIGHT = 0,
    LBFGSX_LS_MORE_THUENTE = 1,
    LBFGSX_LS_BACKTRACKING = 2,
    LBFGSX_LS_BRACKETING = 3
};
enum { LBFGSX_ALGO_LBFGS = 0, LBFGSX_ALGO_LBFGSB = 1 };

/* LBFGSParam / LBFGSBParam fields (reference Param.h:79-161, 236-320); doubles are cast to the scalar type */
typedef struct
{
    int m;
    double epsilon, epsilon_rel;
    int past;
    double delta;
    int max_iterations;
    int linesearch;
    int max_linesearch;
    double min_step, max_step, ftol, wolfe;
    int max_submin;
} lbfgsx_params;

typedef struct
{
    int niter;    /* minimize() return value */
    int nfev;     /* objective evaluations */
    double fx;    /* final objective value */
    double gnorm; /* final_grad_norm() */
    int status;   /* 0, or LBFGSX_E_* of the exception the reference API would have thrown */
    char msg[200];
} lbfgsx_result;

/* optional per-evaluation trace (parity testing): fx[k] and x[0::stride] at the k-th objective evaluation */
typedef struct
{
    int cap;
    int count;
    double* fx;
    int64_t stride;
    int64_t nsamp;
    double* xs;
} lbfgsx_trace;

typedef struct lbfgsx_solver lbfgsx_solver;

/* constructor of LBFGSSolver / LBFGSBSolver: validates the parameters (check_param) */
int lbfgsx_solver_create(lbfgsx_solver** out, int algo, int dtype, int linesearch, const lbfgsx_params* p, int device);
const char* lbfgsx_solver_create_error(void); /* message of a failed lbfgsx_solver_create */
void lbfgsx_solver_destroy(lbfgsx_solver* s);
/* allocate device state for dimension n and expose it (to generate / upload resident inputs) */
int lbfgsx_solver_prepare(lbfgsx_solver* s, int64_t n);
lbfgsx_ctx* lbfgsx_solver_ctx(lbfgsx_solver* s);
/* progress hook: fn(k, user) runs on the host after iteration k has produced the next search direction */
int lbfgsx_solver_set_iteration_hook(lbfgsx_solver* s, void (*fn)(int, void*), void* user);
/* LBFGSSolver::set_recursion (extension): 0 = vector two-loop (bit-parity path, default), 1 = Gram-space form
 * (include/LBFGSpp/GramSpace.h), 2 = Gram-space form with an f32 history (f64 solvers only).  LBFGSX_E_INVALID for
 * L-BFGS-B solvers. */
int lbfgsx_solver_set_recursion(lbfgsx_solver* s, int form);
/* LBFGSSolver::set_direction_scale (extension, for tests of the line searches' entry check): the directions computed from
 * now on are a * H * grad; -1 is the method, +1 gives an ascent direction.  LBFGSX_E_INVALID for L-BFGS-B solvers. */
int lbfgsx_solver_set_direction_scale(lbfgsx_solver* s, double a);
/* LBFGSSolver::set_reducer (extension, row-sharded runs): fn(values, count, user) must sum `values` over all ranks in
 * place (an all-reduce); NULL switches back.  L-BFGS solvers with the Gram-space recursion only. */
int lbfgsx_solver_set_allreduce(lbfgsx_solver* s, void (*fn)(double*, int, void*), void* user);
/* LBFGSSolver::set_devices (extension): the next lbfgsx_solver_minimize with a host x row-shards the ONE problem over the
 * listed GPUs of this node -- one host thread + context per device, the driver's sums through lbfgsx_comm_allreduce_sum
 * (RCCL; include/lbfgsx.h).  ndev = 0 switches back.  L-BFGS solvers only. */
int lbfgsx_solver_set_devices(lbfgsx_solver* s, const int* devices, int ndev);
/* test entry: Cauchy::get_cauchy_point + SubspaceMin::subspace_minimize of the drop-in headers on a history of
 * npairs host-provided corrections; counts = {|newact|, |free|, crossings, BOXCQP sweeps} */
int lbfgsx_test_cauchy_subspace(int dtype, int64_t n, int m, int npairs, const void* S, const void* Y, const void* x0,
                                const void* g, const void* lb, const void* ub, int max_submin, void* xcp, double* vecc,
                                unsigned char* state, void* drt, long long counts[4], char* errbuf, int errlen);
/* final_approx_hessian() / final_approx_inverse_hessian() of the last L-BFGS minimize() (reference LBFGS.h:192-197):
 * column-major n x n doubles; small n only */
int lbfgsx_solver_hessians(lbfgsx_solver* s, double* B, double* H);
/* L-BFGS-B instrumentation of the last minimize(): {GCP break points crossed, BOXCQP sweeps, subspace calls,
 * unconverged subspace calls, BFGS resets, 0, 0, 0} */
int lbfgsx_solver_stats(lbfgsx_solver* s, long long out[8]);
/* more of the same: {GCP crossings handled by the device search, partial sorts that had to be redone in full,
 * searches served by a partial sort, subspace us, line-search us, add_correction us, 0, 0} */
int lbfgsx_solver_stats2(lbfgsx_solver* s, long long out[8]);
/* and: {GCP searches, sum of their finite positive break points (the reference's |ord|, Cauchy.h:132-133), sum of the
 * break points actually sorted, 0, 0, 0, 0, 0} */
int lbfgsx_solver_stats3(lbfgsx_solver* s, long long out[8]);
/* minimize(): objective = LBFGSX_OBJ_*; a/b host arrays or NULL (resident); x host in/out or NULL (resident:
 * start point in LBFGSX_VEC_X, result left there); lb/ub host arrays or NULL (resident), L-BFGS-B only */
int lbfgsx_solver_minimize(lbfgsx_solver* s, int objective, int64_t n, const void* a, const void* b, void* x,
                           const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* A caller-supplied objective on device memory.  fn(user, x_dev, grad_dev, n, fx): x_dev and grad_dev are the context's
 * own device vectors of n elements of the solver's dtype (no staging copy; which named vector they are changes from call to
 * call); the callback writes grad f(x) to grad_dev and f(x) to *fx and returns 0, or non-zero to end the minimisation.
 * It is what a C++ device functor gets (LBFGSpp/Device.h, Evaluator::call_user): the library has drained its stream and made
 * the context's device current for the calling thread before the call, so the callback may use any stream; its work must be
 * complete when it returns (the solver's next kernel reads grad_dev).  It runs on the thread that called minimize.
 * lbfgsx_solver_minimize_fn: x, lb, ub, trace and out as lbfgsx_solver_minimize; every algorithm, line search and dtype the
 * solver was created with -- the same templates with one more functor.  A non-zero return ends the call with status
 * LBFGSX_E_USER, out->nfev = the number of calls made (the failing one included), the message naming it, and x left as an
 * exception of a C++ device functor leaves it: the trial point if the running line search had written one, else the current
 * iterate.  A non-finite *fx is not an abort: the line searches' own checks meet it, with the reference's messages.
 * Extensions: lbfgsx_solver_set_recursion applies to a callback as to a built-in objective; after lbfgsx_solver_set_devices
 * (row shards: each evaluates its own rows of a built-in objective) the call is refused with LBFGSX_E_INVALID.
 * Without a GPU: LBFGSX_E_NOGPU, the callback is never called. */
typedef int (*lbfgsx_objective_fn)(void* user, const void* x_dev, void* grad_dev, int64_t n, double* fx);
int lbfgsx_solver_minimize_fn(lbfgsx_solver* s, int64_t n, lbfgsx_objective_fn fn, void* user, void* x, const void* lb,
                              const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* A term objective compiled at run time (include/lbfgsx.h, lbfgsx_objective_compile) through the solver: the objective is
 * bound to the solver's context and the templates run as for a built-in objective -- every fused launch (the trial pass, and
 * for L-BFGS-B the dg / max-step / first-trial pass), every line search, both dtypes, with the launches a built-in objective
 * gets.  p[0..3]: the per-coordinate data arrays, n elements of
 * the solver's dtype each or NULL -- device memory of the caller used in place, or, for the slots whose bit is set in host_mask,
 * host arrays copied to the device first; c[0..7]: the scalars (NULL = zeros).  x, lb, ub, trace and out as
 * lbfgsx_solver_minimize.  n must be a multiple of the objective's K (LBFGSX_E_INVALID).  Refused with LBFGSX_E_INVALID after
 * lbfgsx_solver_set_recursion(1 | 2) or lbfgsx_solver_set_devices / _set_allreduce.  Without a GPU: LBFGSX_E_NOGPU. */
int lbfgsx_solver_minimize_obj(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, const void* const p[4], int host_mask,
                               const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                               lbfgsx_result* out);
/* lbfgsx_solver_minimize_obj for a grid objective (include/lbfgsx.h, lbfgsx_objective_compile_grid): x is a row-major
 * rows x cols array, n = rows*cols.  rows < 2, cols < 2 and a handle of another form are refused with LBFGSX_E_INVALID;
 * lbfgsx_solver_minimize_obj refuses a grid handle (it carries no shape). */
int lbfgsx_solver_minimize_grid(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, const void* const p[4],
                                int host_mask, const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                lbfgsx_result* out);
/* lbfgsx_solver_minimize_obj for a volume objective (include/lbfgsx.h, lbfgsx_objective_compile_volume): x is a slab-major
 * slabs x rows x cols array, n = slabs*rows*cols.  An extent < 2, a product that overflows and a handle of another form are
 * refused with LBFGSX_E_INVALID; lbfgsx_solver_minimize_obj refuses a volume handle (it carries no shape). */
int lbfgsx_solver_minimize_volume(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                  const void* const p[4], int host_mask, const double c[8], void* x, const void* lb, const void* ub,
                                  lbfgsx_trace* trace, lbfgsx_result* out);
/* lbfgsx_solver_minimize_grid and lbfgsx_solver_minimize_volume for the periodic forms (include/lbfgsx.h,
 * lbfgsx_objective_compile_grid_periodic and _volume_periodic): periodic is the mask, bit 0 the column, bit 1 the row, bit 2
 * the slab direction.  An extent < 2, a product that overflows, a mask with other bits and a handle of another form are refused
 * with LBFGSX_E_INVALID; lbfgsx_solver_minimize_obj refuses these handles (they carry no shape). */
int lbfgsx_solver_minimize_grid_periodic(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                         const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                         const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
int lbfgsx_solver_minimize_volume_periodic(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t slabs, int64_t rows, int64_t cols,
                                           int periodic, const void* const p[4], int host_mask, const double c[8], void* x,
                                           const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* lbfgsx_solver_minimize_grid_periodic for a grid field objective (include/lbfgsx.h, lbfgsx_objective_compile_grid_field): x has
 * rows*cols*D coordinates, D the handle's.  An extent < 2, a product that overflows, a mask above 3 and a handle of another form
 * are refused with LBFGSX_E_INVALID; lbfgsx_solver_minimize_obj refuses this handle (it carries no shape). */
int lbfgsx_solver_minimize_grid_field(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                      const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                      const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* lbfgsx_solver_minimize_grid_periodic for a grid stencil objective (include/lbfgsx.h, lbfgsx_objective_compile_grid_stencil): x
 * is a row-major rows x cols array.  An extent < 3, a product that overflows, a mask above 3 and a handle of another form are
 * refused with LBFGSX_E_INVALID; lbfgsx_solver_minimize_obj refuses this handle (it carries no shape). */
int lbfgsx_solver_minimize_grid_stencil(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t rows, int64_t cols, int periodic,
                                        const void* const p[4], int host_mask, const double c[8], void* x, const void* lb,
                                        const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* lbfgsx_solver_minimize_obj for a graph objective (include/lbfgsx.h, lbfgsx_objective_compile_graph): x has n nodes, the E
 * edges are (ei[e], ej[e]), host arrays or device arrays (edges_on_device != 0).  counts[k] is the number of elements of
 * p[k] where host_mask says it is a host array (n or E; NULL: n for all).  A handle of another form is refused with
 * LBFGSX_E_INVALID, as are the edge lists lbfgsx_objective_bind_graph refuses; lbfgsx_solver_minimize_obj refuses a graph
 * handle (it carries no edges). */
int lbfgsx_solver_minimize_graph(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t E, const int32_t* ei,
                                 const int32_t* ej, int edges_on_device, const void* const p[4], int host_mask,
                                 const int64_t counts[4], const double c[8], void* x, const void* lb, const void* ub,
                                 lbfgsx_trace* trace, lbfgsx_result* out);
/* lbfgsx_solver_minimize_obj for a mesh objective (include/lbfgsx.h, lbfgsx_objective_compile_mesh): x has n = N*D unknowns,
 * node-major; elems[E*K] is the connectivity table, a host array or a device array (elems_on_device != 0).  counts[k] is the
 * number of elements of p[k] where host_mask says it is a host array (n, N or E; NULL: n for all).  A handle of another
 * form, E < 1 and n not a multiple of D are refused with LBFGSX_E_INVALID before a device is needed, as are the tables
 * lbfgsx_objective_bind_mesh refuses; lbfgsx_solver_minimize_obj and lbfgsx_solver_minimize_graph refuse a mesh handle. */
/* lbfgsx_solver_minimize_obj for a linear-model objective (include/lbfgsx.h, lbfgsx_objective_compile_linear): x has n
 * weights, the R x n matrix is rowptr / col / val in CSR, host arrays or device arrays (matrix_on_device != 0); lanes as
 * for lbfgsx_objective_bind_linear.  counts[k]: the elements of p[k] where host_mask says it is a host array (n or R; NULL:
 * n for all).  A handle of another form is refused with LBFGSX_E_INVALID, as are the matrices lbfgsx_objective_bind_linear
 * refuses; lbfgsx_solver_minimize_obj refuses a linear-model handle (it carries no matrix).  A multi-output handle
 * (lbfgsx_objective_compile_linear_multi, D outputs per row) is taken here too: x holds the F x D weight matrix, n = F*D, the
 * matrix is R x F, and n not a multiple of D is refused with both values named before a device is needed. */
int lbfgsx_solver_minimize_linear(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, int64_t nnz,
                                  const int32_t* rowptr, const int32_t* col, const void* val, int matrix_on_device, int lanes,
                                  const void* const p[4], int host_mask, const int64_t counts[4], const double c[8], void* x,
                                  const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
/* The same for a dense linear-model objective (lbfgsx_objective_compile_dense, include/lbfgsx.h "dense linear-model
 * objectives"): x holds the F x D weight matrix, n = F*D, A is R x F, row-major with a row stride of lda >= F elements of the
 * solver's dtype, a host array (copied) or a device array used in place (a_on_device != 0); lanes and counts as for
 * lbfgsx_solver_minimize_linear (a data array has n, F, R or R*D elements).  A handle of another form, n not a multiple of D
 * (both named), R < 1, A null and lda < F are refused with LBFGSX_E_INVALID before a device is needed;
 * lbfgsx_solver_minimize_obj and lbfgsx_solver_minimize_linear refuse a dense handle. */
int lbfgsx_solver_minimize_dense(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, const void* A, int64_t lda,
                                 int a_on_device, int lanes, const void* const p[4], int host_mask, const int64_t counts[4],
                                 const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                 lbfgsx_result* out);
/* The same for a graph-regularised linear-model objective (lbfgsx_objective_compile_linear_graph, include/lbfgsx.h
 * "graph-regularised linear-model objectives"): the matrix as for lbfgsx_solver_minimize_linear, the E edges as for
 * lbfgsx_solver_minimize_graph, each host arrays or device arrays by its own flag; a data array has n, E or R elements.  A
 * handle of another form, E < 1, R < 1 and nnz < 1 are refused with LBFGSX_E_INVALID before a device is needed, as are the
 * edges and matrices lbfgsx_objective_bind_linear_graph refuses; every other minimise entry refuses the handle. */
int lbfgsx_solver_minimize_linear_graph(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t R, int64_t nnz,
                                        const int32_t* rowptr, const int32_t* col, const void* val, int matrix_on_device,
                                        int lanes, int64_t E, const int32_t* ei, const int32_t* ej, int edges_on_device,
                                        const void* const p[4], int host_mask, const int64_t counts[4], const double c[8],
                                        void* x, const void* lb, const void* ub, lbfgsx_trace* trace, lbfgsx_result* out);
int lbfgsx_solver_minimize_mesh(lbfgsx_solver* s, const lbfgsx_objective* obj, int64_t n, int64_t E, const int32_t* elems,
                                int elems_on_device, const void* const p[4], int host_mask, const int64_t counts[4],
                                const double c[8], void* x, const void* lb, const void* ub, lbfgsx_trace* trace,
                                lbfgsx_result* out);

/* ---- batched mode (BASELINE.json cfg5): many independent minimisations on one GPU ------------------------
 * Problem `id` is the extended Rosenbrock (or diag quadratic) instance generated on the device from seed
 * `seed_base + id`.  `nthreads` host workers each own one solver/context/stream and pull
 * problem ids from a shared counter, so up to `nthreads` problems are resident and overlap on the GPU; there is
 * no reference counterpart (the reference solves one problem per call).  One process per GPU shards a larger
 * batch by giving each rank its own [first, first+count) range: no inter-GPU traffic on the critical path. */
typedef struct
{
    int niter, nfev, status;
    double fx, gnorm;
} lbfgsx_batch_item;
int lbfgsx_batch_minimize(int algo, int dtype, int linesearch, const lbfgsx_params* p, int objective, int64_t n,
                          int64_t first, int64_t count, uint64_t seed_base, int device, int nthreads,
                          lbfgsx_batch_item* out);
/* lock-step variant (include/LBFGSBatched.h): all `count` problems resident at once and advanced together, one
 * kernel launch per statement for the whole batch; L-BFGS + LineSearchMoreThuente + extended Rosenbrock (the general
 * form below takes the line search and the objective).
 * x_out (optional): count*n scalars receiving the final iterates. */
int lbfgsx_batch_minimize_lockstep(int dtype, const lbfgsx_params* p, int64_t n, int64_t first, int count,
                                   uint64_t seed_base, int device, lbfgsx_batch_item* out, void* x_out, char* errbuf,
                                   int errlen);
/* The same over several GPUs of one node from one process (BASELINE.json cfg5 "sharded over 8 x MI355X"):
 * devices[r] (r < ndev) solves the r-th contiguous, balanced block of the `count` problem ids in its own lock-step
 * batch on its own host thread; no data crosses between devices, the records (and x_out) are gathered in host memory in
 * problem-id order.  A device id may repeat.  Records are bit-identical to the single-device call. */
int lbfgsx_batch_minimize_lockstep_multi(int dtype, const lbfgsx_params* p, int64_t n, int64_t first, int count,
                                         uint64_t seed_base, const int* devices, int ndev, lbfgsx_batch_item* out,
                                         void* x_out, char* errbuf, int errlen);
/* The general form: the line search the reference's solver takes as its template parameter (LBFGS.h:20-21) -- the two
 * policies that exist as state machines, LBFGSX_LS_MORE_THUENTE and LBFGSX_LS_NOCEDAL_WRIGHT -- and the built-in
 * objective: LBFGSX_OBJ_EXT_ROSENBROCK (start points of seed seed_base + id) or LBFGSX_OBJ_DIAG_QUAD (a, b of
 * lbfgsx_gen_diag_quad(kappa, seed_base + id), x0 = 0).  Every problem follows the trajectory of the single-problem solver
 * with that policy, bit for bit.  (A user objective on device memory: lbfgsx_lockstep_minimize_fn below, or from C++
 * LBFGSBatchedSolver::minimize(BatchFunctor / BatchPackedFunctor, ...) in include/LBFGSBatched.h.) */
int lbfgsx_batch_minimize_lockstep_ex(int dtype, int linesearch, int objective, double kappa, const lbfgsx_params* p, int64_t n,
                                      int64_t first, int count, uint64_t seed_base, const int* devices, int ndev,
                                      lbfgsx_batch_item* out, void* x_out, char* errbuf, int errlen);

/* A lock-step batch kept alive across minimisations: `count` problems of dimension n resident on `device` (about
 * (2m + 9) n count scalars of HBM, allocated here once).  Every lbfgsx_lockstep_minimize solves the problems of ids
 * [first, first + count) of seed_base from their start points again -- what a service that solves batch after batch of the
 * same shape calls, and what bench.py times (the allocation of ~12 GB is setup, not solve).  timing != 0: events around
 * every launch; stats = {lock-step iterations, 1 if the one-launch-per-iteration form ran, sum of the launches'
 * durations in ms (timing), launches, host waits, waits that timed out, 0, 0}.  No reference counterpart. */
typedef struct lbfgsx_lockstep lbfgsx_lockstep;
int lbfgsx_lockstep_create(lbfgsx_lockstep** out, int dtype, int linesearch, const lbfgsx_params* p, int64_t n, int count,
                           int device, int timing, char* errbuf, int errlen);
int lbfgsx_lockstep_minimize(lbfgsx_lockstep* h, int objective, double kappa, uint64_t seed_base, int64_t first,
                             lbfgsx_batch_item* out, void* x_out, double stats[8], char* errbuf, int errlen);
/* The batch for a caller-supplied objective that sees the evaluating problems as ONE array.  x0: count x n start points of
 * the handle's dtype, row-major, host or device memory (read before the call returns).
 * eval(user, nact, ids, X, G, ld, fx): X and G are packed device arrays, row k (ld elements apart, k < nact) belonging to problem
 * ids[k] (ascending); the callback writes grad f(X row k) to G row k and f to fx[k] (host) and returns 0, or non-zero to fail
 * the call.  Problems that have converged, failed or do not evaluate in this lock-step turn are not in the list.  The stream
 * and device contract is lbfgsx_objective_fn's.  The first call carries all count problems.  Around every further call the
 * library runs lbfgsx_bat_pack and lbfgsx_bat_unpack (include/lbfgsx.h); the statements after a line search and the recursion
 * stay in the one launch per lock-step iteration where that form applies, its in-kernel first trial does not (it cannot host a
 * callback).  Every member follows the trajectory of lbfgsx_solver_minimize_fn on its own problem with the same per-row
 * arithmetic.  stats as lbfgsx_lockstep_minimize, plus stats[6] = calls of eval.  A non-zero return: LBFGSX_E_USER, out
 * undefined, the handle stays usable.  Without a GPU (no handle can exist): LBFGSX_E_NOGPU. */
typedef int (*lbfgsx_batch_objective_fn)(void* user, int nact, const int64_t* ids, const void* X, void* G, int64_t ld,
                                         double* fx);
int lbfgsx_lockstep_minimize_fn(lbfgsx_lockstep* h, const void* x0, lbfgsx_batch_objective_fn eval, void* user,
                                lbfgsx_batch_item* out, void* x_out, double stats[8], char* errbuf, int errlen);
int lbfgsx_lockstep_set_timing(lbfgsx_lockstep* h, int on);  /* for the minimisations that follow */
void lbfgsx_lockstep_destroy(lbfgsx_lockstep* h);

#ifdef __cplusplus
}
#endif
#endif
