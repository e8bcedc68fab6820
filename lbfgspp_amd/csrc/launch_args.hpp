// lbfgspp_amd/csrc/launch_args.hpp -- grid and arguments of the four launches that evaluate an objective (k_eval, k_trial,
// k_b_eval, k_b_dg_maxstep_trial), worked out once for both forms of the launch: the built-in instantiations
// (hipLaunchKernelGGL in lbfgsx.hip / lbfgsb_linesearch.hip) and the instantiations compiled at run time for a term objective
// (hipModuleLaunchKernel, jit_objective.hip).  The members are the kernels' arguments in order, the objective left out.
#pragma once
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
// the by-value argument of a grid objective's kernels: layout of the generated struct ObjGrid (TermArgs, then the shape)
template <class T>
struct GridArgs
{
    TermArgs<T> t;
    int64_t rows, cols;
};
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
// the objective argument of the bound handle's kernels, by its form: &term for a term or chain objective, &grid for a grid
// one, &graph for a graph one, &mesh for a mesh one
template <class T>
struct BoundArgs
{
    TermArgs<T> term;
    GridArgs<T> grid;
    GraphArgs<T> graph;
    MeshArgs<T> mesh;
    void* ptr;
    explicit BoundArgs(const lbfgsx_ctx* c)
        : term(term_args<T>(c)),
          grid{term, c->term_rows, c->term_cols},
          graph{term, static_cast<const uint32_t*>(c->graph_off), static_cast<const GraphEntry*>(c->graph_inc), c->graph_E},
          mesh{term, static_cast<const uint32_t*>(c->graph_off), static_cast<const uint32_t*>(c->graph_inc), c->graph_E,
               c->mesh_D ? c->n / c->mesh_D : 0}
    {
        ptr = (c->term_form == LBFGSX_FORM_GRID)    ? static_cast<void*>(&grid)
              : (c->term_form == LBFGSX_FORM_GRAPH) ? static_cast<void*>(&graph)
              : (c->term_form == LBFGSX_FORM_MESH)  ? static_cast<void*>(&mesh)
                                                    : static_cast<void*>(&term);
    }
    BoundArgs(const BoundArgs&) = delete;
};
// what a graph objective adds to the byte model of one launch of its kernels: the offsets, the entries, and every gathered
// value once (vectors_gathered: 1 in the evaluation kernels, 2 in the trial kernels, which gather xp and d) -- the values,
// not the sectors that are fetched for them.  Nothing for the other forms.
template <class T>
inline void graph_model_add(const lbfgsx_ctx* c, int vectors_gathered)
{
    if (c->term_form == LBFGSX_FORM_GRAPH)
        model_add(double(c->n + 1) * 4 + double(2 * c->graph_E) * 8 + double(2 * c->graph_E) * sizeof(T) * vectors_gathered);
}
// what a mesh objective adds: (N+1)*4 bytes of offsets, K*E entries of 4K bytes, and (K-1)*D gathered values per entry
template <class T>
inline void mesh_model_add(const lbfgsx_ctx* c, int vectors_gathered)
{
    if (c->term_form == LBFGSX_FORM_MESH)
    {
        const double K = c->mesh_K, D = c->mesh_D, KE = K * double(c->graph_E);
        model_add(double(c->n / c->mesh_D + 1) * 4 + KE * 4 * K + KE * (K - 1) * D * sizeof(T) * vectors_gathered);
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
inline bool term_bound(const lbfgsx_ctx* c, int objective) { return objective == LBFGSX_OBJ_BOUND && c->term != nullptr; }
// one launch of loaded kernel `which` of the bound objective on the context's stream, block of kBlock threads; params as
// hipModuleLaunchKernel takes them (one pointer per kernel argument)
int jit_launch(lbfgsx_ctx* c, int which, int grid, void** params);

}  // namespace lbfgsx
