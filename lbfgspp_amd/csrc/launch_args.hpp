// lbfgspp_amd/csrc/launch_args.hpp -- grid and arguments of the four launches that evaluate an objective (k_eval, k_trial,
// k_b_eval, k_b_dg_maxstep_trial), worked out once for both forms of the launch: the built-in instantiations
// (hipLaunchKernelGGL in lbfgsx.hip / lbfgsb_linesearch.hip) and the instantiations compiled at run time for a term objective
// (hipModuleLaunchKernel, jit_objective.hip).  The members are the kernels' arguments in order, the objective left out.
#pragma once
#include <cstddef>

#include "ctx.hpp"

namespace lbfgsx {

template <class T>
struct EvalLaunch
{
    int grid;
    const T* x;
    T* g;
    int64_t n;
    RedWs ws;
    T* out;
};
template <class T>
inline EvalLaunch<T> eval_launch(lbfgsx_ctx* c)
{
    return {c->grid_for(c->n), static_cast<const T*>(c->xb[c->cur]), static_cast<T*>(c->gb[c->cur]), c->n, c->ws,
            c->out_slot<T>()};
}

template <class T>
struct TrialLaunch
{
    int grid;
    const T *xp, *d;
    T step;
    T *x, *g;
    int64_t n;
    RedWs ws;
    T* out;
    int rev;
};
// obj_vectors: n-vectors of its own the objective reads (byte model of the counters)
template <class T>
inline TrialLaunch<T> trial_launch(lbfgsx_ctx* c, T step, int obj_vectors)
{
    const int rev = (c->tl_step++ & 1u) ? 1 : 0;
    poll_arm(c);
    // byte model (counters, L-BFGS-B legs): xp and d read, x and grad written, + the objective's own vectors
    model_add(double(c->n) * sizeof(T) * (4 + obj_vectors));
    return {c->grid_for(c->n), static_cast<const T*>(c->xb[c->xp]), static_cast<const T*>(c->d), step,
            static_cast<T*>(c->xb[c->trial]), static_cast<T*>(c->gb[c->trial]), c->n, c->ws, c->out_slot<T>(), rev};
}

template <class T>
struct BEvalLaunch
{
    int grid;
    const T* x;
    T* g;
    const T *lb, *ub;
    int64_t n;
    RedWs ws;
    T* out;
};
template <class T>
inline BEvalLaunch<T> b_eval_launch(lbfgsx_ctx* c)
{
    return {c->grid_for(c->n), static_cast<const T*>(c->xb[c->cur]), static_cast<T*>(c->gb[c->cur]),
            static_cast<const T*>(c->lb), static_cast<const T*>(c->ub), c->n, c->ws, c->out_slot<T>()};
}

template <class T>
struct DgTrialLaunch
{
    int grid;
    const T *xp, *g0, *d, *lb, *ub;
    T step;
    T *x, *g;
    int64_t n;
    RedWs ws;
    T* out;
    int rev;
};
template <class T>
inline DgTrialLaunch<T> dg_maxstep_trial_launch(lbfgsx_ctx* c, T step, int obj_vectors)
{
    const int rev = (c->tl_step & 1u) ? 1 : 0;  // the order the trial launch it stands for would have taken
    poll_arm(c);
    // byte model: xp, g, d, lb, ub read, x and grad written, + the objective's own vectors (a, b of the quadratic)
    model_add(double(c->n) * sizeof(T) * (7 + obj_vectors));
    return {c->grid_for(c->n), static_cast<const T*>(c->xb[c->xp]), static_cast<const T*>(c->gb[c->cur]),
            static_cast<const T*>(c->d), static_cast<const T*>(c->lb), static_cast<const T*>(c->ub), step,
            static_cast<T*>(c->xb[c->trial]), static_cast<T*>(c->gb[c->trial]), c->n, c->ws, c->out_slot<T>(), rev};
}

// ---- a term objective bound to the context (lbfgsx_objective_bind, jit_objective.hip)
enum { JIT_K_EVAL = 0, JIT_K_TRIAL = 1, JIT_K_B_EVAL = 2, JIT_K_B_DG_MAXSTEP_TRIAL = 3, JIT_NKERNELS = 4 };
// a linear-model objective has two more, the row passes that precede its four column-pass kernels (linear_kernels.cuh)
enum { JIT_K_LIN_ROWS = 4, JIT_K_LIN_ROWS_TRIAL = 5 };
// a term objective has one more, the post form of k_trial (lbfgs_kernels.cuh: k_trial_post); the forms with kernels of their own
// (chain, grid, graph, mesh, linear) have none
enum { JIT_K_TRIAL_POST = 6 };
// a dense linear-model objective has its row passes in slots 4 and 5 and one more, the partial pass between them and the
// column pass (linear_dense_kernels.cuh: k_dense_partials)
enum { JIT_K_DENSE_PARTIALS = 7, JIT_NSLOTS = 8 };
// the by-value kernel argument: layout of the generated struct ObjTerm (four data pointers, eight scalars of type T)
template <class T>
struct TermArgs
{
    const T* p[4];
    T c[8];
};
template <class T>
inline TermArgs<T> term_args(const lbfgsx_ctx* c)
{
    TermArgs<T> a;
    for (int j = 0; j < 4; j++)
        a.p[j] = static_cast<const T*>(c->term_p[j]);
    for (int j = 0; j < 8; j++)
        a.c[j] = T(c->term_c[j]);
    return a;
}
// the by-value arguments of the lattice forms' kernels, one struct per layout the generator writes (jit_objective.hip,
// kForms[..].members: TermArgs' members, then the int64_t extents, then for a form with a mask int periodic, pad_):
//   GridArgs          ObjGrid
//   VolumeArgs        ObjVolume
//   MaskedGridArgs    ObjGridPeriodic, ObjGridField (D is a constant of the struct), ObjGridStencil
//   MaskedVolumeArgs  ObjVolumePeriodic
template <class T>
struct GridArgs
{
    TermArgs<T> t;
    int64_t rows, cols;
};
template <class T>
struct VolumeArgs
{
    TermArgs<T> t;
    int64_t slabs, rows, cols;
};
template <class T>
struct MaskedGridArgs
{
    TermArgs<T> t;
    int64_t rows, cols;
    int32_t periodic, pad_;
};
template <class T>
struct MaskedVolumeArgs
{
    TermArgs<T> t;
    int64_t slabs, rows, cols;
    int32_t periodic, pad_;
};
// a member that moved would corrupt a kernel's arguments without a word: the extents follow TermArgs directly, 8 bytes each,
// the mask follows them, and nothing else is in the struct
template <class T>
constexpr bool lattice_layouts_hold()
{
    constexpr size_t t = sizeof(TermArgs<T>);
    return t == 4 * sizeof(const T*) + 8 * sizeof(T) && t % 8 == 0 && offsetof(GridArgs<T>, t) == 0 &&
           offsetof(GridArgs<T>, rows) == t && offsetof(GridArgs<T>, cols) == t + 8 && sizeof(GridArgs<T>) == t + 16 &&
           offsetof(VolumeArgs<T>, slabs) == t && offsetof(VolumeArgs<T>, rows) == t + 8 && offsetof(VolumeArgs<T>, cols) == t + 16 &&
           sizeof(VolumeArgs<T>) == t + 24 && offsetof(MaskedGridArgs<T>, rows) == t && offsetof(MaskedGridArgs<T>, cols) == t + 8 &&
           offsetof(MaskedGridArgs<T>, periodic) == t + 16 && offsetof(MaskedGridArgs<T>, pad_) == t + 20 &&
           sizeof(MaskedGridArgs<T>) == t + 24 && offsetof(MaskedVolumeArgs<T>, slabs) == t &&
           offsetof(MaskedVolumeArgs<T>, rows) == t + 8 && offsetof(MaskedVolumeArgs<T>, cols) == t + 16 &&
           offsetof(MaskedVolumeArgs<T>, periodic) == t + 24 && offsetof(MaskedVolumeArgs<T>, pad_) == t + 28 &&
           sizeof(MaskedVolumeArgs<T>) == t + 32;
}
static_assert(lattice_layouts_hold<double>() && lattice_layouts_hold<float>(),
              "a lattice form's argument struct no longer has the layout of the struct generated for its kernels");
// the by-value argument of a graph objective's kernels: layout of the generated struct ObjGraph (TermArgs, then the
// context's incidence list: uint32 off[n+1], 8-byte entries inc[2E] (graph_entry.hpp), and E)
struct GraphEntry;
template <class T>
struct GraphArgs
{
    TermArgs<T> t;
    const uint32_t* off;
    const GraphEntry* inc;
    int64_t E;
};
// the by-value argument of a mesh objective's kernels: layout of the generated struct ObjMesh (TermArgs, then the context's
// incidence list: uint32 off[N+1], K*E entries of K 32-bit words (mesh_topology.hip), the E elements and the N nodes)
template <class T>
struct MeshArgs
{
    TermArgs<T> t;
    const uint32_t* off;
    const uint32_t* inc;
    int64_t E, N;
};
// the by-value argument of a linear-model objective's kernels: layout of the generated struct ObjLinear (TermArgs, then the
// context's copy of the CSR arrays, the transposed list, the row pass's outputs and the long columns' chunk table:
// ctx.hpp LinearTopo, linear_topology.hip)
template <class T>
struct LinearArgs
{
    TermArgs<T> t;
    const int32_t* rowptr;
    const int32_t* col;
    const T* val;
    const uint32_t* colptr;
    const int32_t* trow;
    const T* tval;
    T* w;
    T* v;
    const T* part;
    const int32_t* long_col;
    const uint32_t* long_chunk;
    int64_t R, nnz;
    int32_t L, C, nlong, pad_;
};
template <class T>
inline LinearArgs<T> linear_args(const lbfgsx_ctx* c, const TermArgs<T>& t)
{
    const lbfgsx_ctx::LinearTopo& l = c->lin;
    return {t,
            static_cast<const int32_t*>(l.rowptr),
            static_cast<const int32_t*>(l.col),
            static_cast<const T*>(l.val),
            static_cast<const uint32_t*>(l.colptr),
            static_cast<const int32_t*>(l.trow),
            static_cast<const T*>(l.tval),
            static_cast<T*>(l.w),
            static_cast<T*>(l.v),
            static_cast<const T*>(l.part),
            static_cast<const int32_t*>(l.long_col),
            static_cast<const uint32_t*>(l.long_chunk),
            l.R,
            l.nnz,
            l.L,
            l.C,
            l.nlong,
            0};
}
// the by-value argument of a dense linear-model objective's kernels: layout of the generated struct ObjDense (TermArgs, then
// the matrix -- the caller's device array or the context's copy of a host one --, the row pass's outputs and the chunk
// partials: ctx.hpp DenseTopo, dense_topology.hip)
template <class T>
struct DenseArgs
{
    TermArgs<T> t;
    const T* A;
    T* w;
    T* v;
    T* part;
    int64_t R, F, lda, chunks;
    int32_t L, C, pad0_, pad1_;
};
template <class T>
inline DenseArgs<T> dense_args(const lbfgsx_ctx* c, const TermArgs<T>& t)
{
    const lbfgsx_ctx::DenseTopo& d = c->dense;
    return {t, static_cast<const T*>(d.A), static_cast<T*>(d.w), static_cast<T*>(d.v), static_cast<T*>(d.part), d.R, d.F, d.lda,
            d.chunks, d.L, d.C, 0, 0};
}
// the by-value argument of a graph-regularised linear-model objective's kernels: layout of the generated struct
// ObjLinearGraph (LinearArgs, then the context's incidence list as in GraphArgs)
template <class T>
struct LinearGraphArgs
{
    LinearArgs<T> l;
    const uint32_t* off;
    const GraphEntry* inc;
    int64_t E;
};
// the two forms that lbfgsx_objective_bind_linear binds: a linear-model objective and a multi-output one
inline bool form_is_linear(int form) { return form == LBFGSX_FORM_LINEAR || form == LBFGSX_FORM_LINEAR_MULTI; }
// the forms whose evaluation is a row pass over a CSR matrix and a column walk: those two and the graph-regularised one
inline bool form_has_csr(int form) { return form_is_linear(form) || form == LBFGSX_FORM_LINEAR_GRAPH; }
// the objective argument of the bound handle's kernels, by its form: &term for a term or chain objective, &grid, &volume,
// &mgrid or &mvolume for a lattice one by its layout (above), &graph for a graph one, &mesh for a mesh one, &linear for a
// linear-model one of either form, &dense for a dense one, &linear_graph for a graph-regularised linear-model one
template <class T>
struct BoundArgs
{
    TermArgs<T> term;
    GridArgs<T> grid;
    VolumeArgs<T> volume;
    MaskedGridArgs<T> mgrid;
    MaskedVolumeArgs<T> mvolume;
    GraphArgs<T> graph;
    MeshArgs<T> mesh;
    LinearArgs<T> linear;
    DenseArgs<T> dense;
    LinearGraphArgs<T> linear_graph;
    void* ptr;
    explicit BoundArgs(const lbfgsx_ctx* c)
        : term(term_args<T>(c)),
          grid{term, c->term_rows, c->term_cols},
          volume{term, c->term_slabs, c->term_rows, c->term_cols},
          mgrid{term, c->term_rows, c->term_cols, c->term_periodic, 0},
          mvolume{term, c->term_slabs, c->term_rows, c->term_cols, c->term_periodic, 0},
          graph{term, static_cast<const uint32_t*>(c->graph_off), static_cast<const GraphEntry*>(c->graph_inc), c->graph_E},
          mesh{term, static_cast<const uint32_t*>(c->graph_off), static_cast<const uint32_t*>(c->graph_inc), c->graph_E,
               c->mesh_D ? c->n / c->mesh_D : 0},
          linear(linear_args<T>(c, term)),
          dense(dense_args<T>(c, term)),
          linear_graph{linear, static_cast<const uint32_t*>(c->graph_off), static_cast<const GraphEntry*>(c->graph_inc), c->graph_E}
    {
        switch (c->term_form)
        {
        case LBFGSX_FORM_GRID: ptr = &grid; break;
        case LBFGSX_FORM_VOLUME: ptr = &volume; break;
        case LBFGSX_FORM_GRID_PERIODIC:
        case LBFGSX_FORM_GRID_FIELD:
        case LBFGSX_FORM_GRID_STENCIL: ptr = &mgrid; break;
        case LBFGSX_FORM_VOLUME_PERIODIC: ptr = &mvolume; break;
        case LBFGSX_FORM_GRAPH: ptr = &graph; break;
        case LBFGSX_FORM_MESH: ptr = &mesh; break;
        case LBFGSX_FORM_LINEAR:
        case LBFGSX_FORM_LINEAR_MULTI: ptr = &linear; break;
        case LBFGSX_FORM_DENSE: ptr = &dense; break;
        case LBFGSX_FORM_LINEAR_GRAPH: ptr = &linear_graph; break;
        default: ptr = &term;
        }
    }
    BoundArgs(const BoundArgs&) = delete;
};
// what the bound objective's lists add to the byte model, by its form; nothing for a term, chain, grid or volume objective.
// vectors_gathered: 1 in an evaluation, 2 in a trial, which gathers xp and d -- the values, not the sectors fetched for them.
//   graph   one launch: the offsets, the 2E entries of 8 bytes, and every gathered value once
//   mesh    one launch: (N+1)*4 bytes of offsets, K*E entries of 4K bytes, and (K-1)*D gathered values per entry
//   linear  one evaluation (row pass, long-column launch, column pass): the offsets (rowptr, colptr), the indices (col, trow)
//           and the values (val, tval) of both passes, every gathered value once (the row pass gathers vectors_gathered
//           vectors, the column pass gathers w), w and v written and read, the chunk partials written and read
//   multi-output linear  the same with every gathered value of x, xp, d and w, w written and read and the chunk partials
//           counted D times (F + 1 column offsets); offsets, indices and matrix values once: the D coordinates of a feature
//           read the same entries again, which are cache hits and are not modelled
//   dense linear  one evaluation (row pass, partial pass, column pass): A twice (2 R F values), the weights the row pass
//           reads (n values per vector gathered), w written and read (R*D each), v written and read (R each), the chunk
//           partials written and read (chunks*n each).  The row pass's re-reads of x by the rows of a block and the partial
//           pass's re-reads of w by the threads of a chunk are served by the caches and are not modelled
//   graph-regularised linear  the linear form's terms plus the graph form's list terms (its offsets, entries and gathered other
//           ends): the column pass walks both lists
// A trial launch adds it at its call site; an evaluation adds only a linear-model objective's, in linear_pre_eval.
template <class T>
inline void objective_model_add(const lbfgsx_ctx* c, int vectors_gathered)
{
    const double esz = sizeof(T), vg = vectors_gathered;
    if (c->term_form == LBFGSX_FORM_GRAPH || c->term_form == LBFGSX_FORM_LINEAR_GRAPH)
        model_add(double(c->n + 1) * 4 + double(2 * c->graph_E) * 8 + double(2 * c->graph_E) * esz * vg);
    if (c->term_form == LBFGSX_FORM_MESH)
    {
        const double K = c->mesh_K, D = c->mesh_D, KE = K * double(c->graph_E);
        model_add(double(c->n / c->mesh_D + 1) * 4 + KE * 4 * K + KE * (K - 1) * D * esz * vg);
    }
    else if (form_has_csr(c->term_form))
    {
        const double R = double(c->lin.R), nnz = double(c->lin.nnz), D = c->lin.D ? c->lin.D : 1;
        model_add((R + 1) * 4 + (double(c->n) / D + 1) * 4 + 2 * nnz * 4 + 2 * nnz * esz + nnz * esz * (vg + 1) * D +
                  2 * R * esz * D + 2 * R * esz + 2 * double(c->lin.nchunks) * esz * D);
    }
    else if (c->term_form == LBFGSX_FORM_DENSE)
    {
        const double R = double(c->dense.R), F = double(c->dense.F), D = c->dense.D, n = double(c->n);
        model_add(2 * R * F * esz + n * esz * vg + 2 * R * D * esz + 2 * R * esz + 2 * double(c->dense.chunks) * n * esz);
    }
}
// graph_topology.hip: the incidence list of the context (ctx.hpp: graph_off, graph_inc, graph_E).  build validates the
// indices first and leaves the context without a list when an edge offends (LBFGSX_E_INVALID, the edge named)
int graph_topology_build(lbfgsx_ctx* c, const int32_t* ei, const int32_t* ej, int64_t E, int on_device);
int graph_topology_read(lbfgsx_ctx* c, uint32_t* off, int32_t* other, uint32_t* edge_side);
void graph_topology_free(lbfgsx_ctx* c);
// mesh_topology.hip: the same for a mesh objective's elems[E*K], into the same fields of the context (freed by
// graph_topology_free).  words: K*E*K uint32, off: N+1
int mesh_topology_build(lbfgsx_ctx* c, int K, int D, const int32_t* elems, int64_t E, int on_device);
int mesh_topology_read(lbfgsx_ctx* c, uint32_t* off, uint32_t* words);
// linear_topology.hip: the matrix of a linear-model objective (ctx.hpp: lin).  build validates the caller's CSR arrays
// first and leaves the context without a matrix when one offends (LBFGSX_E_INVALID, the position named); lanes: 0 = by the
// rule (linear_lanes_rule), otherwise the lanes per row.  long_launch: the launch between the two passes, none when the
// matrix has no long column.  D: the outputs per row of a multi-output objective (the matrix then has n / D columns), 0 for
// the scalar form.  beside_graph: the incidence list the context holds stays (lbfgsx_objective_bind_linear_graph builds it first);
// otherwise every other form's list is freed first
constexpr int kLinearChunk = 4096;  // C: a column with more entries is long and is summed in chunks of C by k_lin_long_cols
int linear_lanes_rule(int64_t R, int64_t nnz);
int linear_topology_build(lbfgsx_ctx* c, int64_t R, int64_t nnz, const int32_t* rowptr, const int32_t* col, const void* val,
                          int on_device, int lanes, int D = 0, bool beside_graph = false);
int linear_topology_read(lbfgsx_ctx* c, uint32_t* colptr, int32_t* trow, uint32_t* tpos, int32_t* long_col, uint32_t* long_chunk,
                         uint32_t* chunk);
void linear_topology_free(lbfgsx_ctx* c);
int linear_long_launch(lbfgsx_ctx* c);
// dense_topology.hip: the matrix of a dense linear-model objective (ctx.hpp: dense).  A host matrix is copied, compactly
// (lda = F), into an array the context owns; a device matrix is used in place.  lanes: 0 = by the rule (the largest power of
// two <= F, at most 64: linear_lanes_rule with nnz / R = F).  read: w (R*D), v (R), part (chunks*n), any of them null
constexpr int kDenseChunk = 256;  // C: the consecutive rows whose products one partial sums
int dense_topology_build(lbfgsx_ctx* c, int64_t R, int D, const void* A, int64_t lda, int on_device, int lanes);
int dense_topology_read(lbfgsx_ctx* c, void* w, void* v, void* part);
void dense_topology_free(lbfgsx_ctx* c);
inline bool term_bound(const lbfgsx_ctx* c, int objective) { return objective == LBFGSX_OBJ_BOUND && c->term != nullptr; }
// one launch of loaded kernel `which` of the bound objective on the context's stream, block of kBlock threads; params as
// hipModuleLaunchKernel takes them (one pointer per kernel argument)
int jit_launch(lbfgsx_ctx* c, int which, int grid, void** params);

// ---- a linear-model objective's launches ahead of its column pass, on the same stream with no host wait in between: the
// row pass (k_lin_rows over x, or k_lin_rows_trial over xp + step*d), then the long-column launch if the matrix has a long
// column.  A dense linear-model objective's: the row pass, then the partial pass.  Nothing for the other forms.
inline int linear_rows_grid(int64_t R, int L)
{
    const int64_t rpb = kBlock / L, b = (R + rpb - 1) / rpb;
    return int(b < 1 ? 1 : (b > kGridCap ? kGridCap : b));
}
inline int linear_rows_grid(const lbfgsx_ctx* c)
{
    return c->term_form == LBFGSX_FORM_DENSE ? linear_rows_grid(c->dense.R, c->dense.L) : linear_rows_grid(c->lin.R, c->lin.L);
}
// the blocks of k_dense_partials: one per work item (kBlock / S chunks x S packs of W columns, S = the next power of two >=
// the packs of a row, at most kBlock: linear_dense_kernels.cuh), which the kernel strides over past the cap
constexpr int64_t kDensePartialGridCap = 1 << 20;
inline int dense_partials_grid(const lbfgsx_ctx* c)
{
    const int64_t W = 16 / c->esz, packs = (c->dense.F + W - 1) / W;
    int64_t S = 1;
    while (S < kBlock && S < packs)
        S *= 2;
    const int64_t cpb = kBlock / S, items = ((c->dense.chunks + cpb - 1) / cpb) * ((packs + S - 1) / S);
    return int(items > kDensePartialGridCap ? kDensePartialGridCap : items);
}
// the column pass strides over v[R] as well as over the n coordinates: its grid covers the longer of the two
inline int linear_col_grid(const lbfgsx_ctx* c, int grid)
{
    if (!form_has_csr(c->term_form) && c->term_form != LBFGSX_FORM_DENSE)
        return grid;
    const int gr = c->grid_for(c->term_form == LBFGSX_FORM_DENSE ? c->dense.R : c->lin.R);
    return gr > grid ? gr : grid;
}
// what follows a row pass ahead of the column pass
template <class T>
inline int linear_mid_launch(lbfgsx_ctx* c, BoundArgs<T>& obj)
{
    if (c->term_form != LBFGSX_FORM_DENSE)
        return linear_long_launch(c);
    void* params[] = {obj.ptr};
    return jit_launch(c, JIT_K_DENSE_PARTIALS, dense_partials_grid(c), params);
}
template <class T>
inline int linear_pre_eval(lbfgsx_ctx* c, BoundArgs<T>& obj, const T* x)
{
    if (!form_has_csr(c->term_form) && c->term_form != LBFGSX_FORM_DENSE)
        return LBFGSX_OK;
    objective_model_add<T>(c, 1);
    void* params[] = {&x, obj.ptr};
    const int rc = jit_launch(c, JIT_K_LIN_ROWS, linear_rows_grid(c), params);
    return rc ? rc : linear_mid_launch<T>(c, obj);
}
template <class T>
inline int linear_pre_trial(lbfgsx_ctx* c, BoundArgs<T>& obj, const T* xp, const T* d, T step)
{
    if (!form_has_csr(c->term_form) && c->term_form != LBFGSX_FORM_DENSE)
        return LBFGSX_OK;
    void* params[] = {&xp, &d, &step, obj.ptr};
    const int rc = jit_launch(c, JIT_K_LIN_ROWS_TRIAL, linear_rows_grid(c), params);
    return rc ? rc : linear_mid_launch<T>(c, obj);
}

}  // namespace lbfgsx
