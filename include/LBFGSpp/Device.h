// include/LBFGSpp/Device.h -- C++ face of the C ABI (include/lbfgsx.h) used by the drop-in solvers.
//
// The reference keeps x, grad, drt, xp, gradp and the BFGS history in host Eigen members
// (LBFGS.h:29-36, BFGSMat.h:35-52).  Here they live in HBM inside one `DeviceState`; the solver and
// line-search templates hold only scalars.  Compiled by any C++17 host compiler; links -llbfgsx.
#ifndef LBFGSX_DROPIN_DEVICE_H
#define LBFGSX_DROPIN_DEVICE_H

#include <cmath>
#include <cstdint>
#include <functional>
#include <initializer_list>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../lbfgsx.h"

namespace LBFGSpp {

namespace detail {
// C status -> the exception type the reference would have thrown (SURVEY.md 8(b) "Errors")
inline void check(int rc)
{
    if (rc == LBFGSX_OK)
        return;
    const std::string msg = lbfgsx_last_error();
    switch (rc)
    {
    case LBFGSX_E_INVALID: throw std::invalid_argument(msg);
    case LBFGSX_E_LOGIC: throw std::logic_error(msg);
    default: throw std::runtime_error(msg);
    }
}
// a phase of the solver as a trace range (lbfgsx_range_push / _pop: ROCTx ranges under LBFGSX_ROCTX=1, else one branch)
struct Range
{
    explicit Range(const char* name) { lbfgsx_range_push(name); }
    ~Range() { lbfgsx_range_pop(); }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};
template <typename Scalar> struct dtype_of;
template <> struct dtype_of<double> { static constexpr int value = LBFGSX_F64; };
template <> struct dtype_of<float> { static constexpr int value = LBFGSX_F32; };
}  // namespace detail

// What a caller-supplied objective throws to end the minimisation (the C ABI's callbacks return non-zero: LBFGSX_E_USER).
// It leaves minimize() like any exception of a device functor: x as Evaluator::trial_written decides.
struct UserAbort : std::runtime_error
{
    using std::runtime_error::runtime_error;
};

// A non-owning handle on a device-resident vector, handed to device functors.
template <typename Scalar>
class DeviceVector
{
    Scalar* m_p;
    std::int64_t m_n;

public:
    DeviceVector(Scalar* p, std::int64_t n) : m_p(p), m_n(n) {}
    Scalar* data() const { return m_p; }
    std::int64_t size() const { return m_n; }
};

// Built-in objectives evaluated inside the fused kernels (K0/K2).  `a`/`b` are host arrays of length n
// (copied to the device by minimize()), or null when the data is already resident / generated on device.
template <typename Scalar>
struct BuiltinObjective
{
    int id;
    const Scalar* a;
    const Scalar* b;
    explicit BuiltinObjective(int id_, const Scalar* a_ = nullptr, const Scalar* b_ = nullptr) : id(id_), a(a_), b(b_) {}
};
template <typename Scalar>
inline BuiltinObjective<Scalar> DiagQuadratic(const Scalar* a = nullptr, const Scalar* b = nullptr)
{
    return BuiltinObjective<Scalar>(LBFGSX_OBJ_DIAG_QUAD, a, b);
}
template <typename Scalar>
inline BuiltinObjective<Scalar> ExtendedRosenbrock()
{
    return BuiltinObjective<Scalar>(LBFGSX_OBJ_EXT_ROSENBROCK);
}

// An objective that is a sum of terms over K consecutive coordinates, given as device code for ONE term and compiled at
// run time into the fused kernels (include/lbfgsx.h, "term objectives"): the solvers take every path they take for a
// built-in objective.  body sees T, const T x[K], T g[K], int64_t i, const T* p0..p3, T c[8] and returns the term's value.
//     TermObjective<double> f(2, "const T t1 = T(1) - x[0]; ... return t1 * t1 + t2 * t2;");
//     f.data(p0_dev, p1_dev).scalars({0.5});      solver.minimize(f, x, fx);
// data(): device arrays of n elements owned by the caller; host_data(slot, ptr): a host array the solver copies to the device
// at every minimize().  The constructor throws std::invalid_argument with the compiler's log when the body does not
// compile.  Not for the Gram-space recursion or row-sharded runs (refused), nor the lock-step batch.
template <typename Scalar>
class TermObjective
{
    lbfgsx_objective* m_h = nullptr;
    bool m_own = false;
    const Scalar* m_p[4] = {nullptr, nullptr, nullptr, nullptr};
    const Scalar* m_host[4] = {nullptr, nullptr, nullptr, nullptr};
    double m_c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int m_lattice = LBFGSX_FORM_TERM;     // the form a class on a regular array declares (set_lattice): which call binds it
    std::int64_t m_slabs = 0, m_rows = 0, m_cols = 0;  // its extents (m_slabs: a form on three axes) ...
    int m_periodic = 0;                                // ... and mask (a form that has one)
    std::int64_t m_E = 0;                // a GraphObjective's edges; 0: the handle is bound without any
    const std::int32_t *m_ei = nullptr, *m_ej = nullptr;
    bool m_edges_dev = false;
    const std::int32_t* m_elems = nullptr;  // a MeshObjective's connectivity table of m_E rows; null: bound without one
    std::int64_t m_count[4] = {0, 0, 0, 0};  // elements of m_host[k]; 0: n
    // a LinearObjective's CSR matrix; m_rowptr null: bound without one
    std::int64_t m_R = 0, m_nnz = 0;
    const std::int32_t *m_rowptr = nullptr, *m_col = nullptr;
    const Scalar* m_val = nullptr;
    bool m_matrix_dev = false;
    int m_lanes = 0;
    // a DenseLinearObjective's matrix (m_R rows, m_matrix_dev, m_lanes as above); m_A null: bound without one
    const Scalar* m_A = nullptr;
    std::int64_t m_lda = 0;
    bool m_dense = false;

    TermObjective(const TermObjective&) = delete;
    TermObjective& operator=(const TermObjective&) = delete;

public:
    int id = LBFGSX_OBJ_NONE;  // LBFGSX_OBJ_BOUND once bound to a solver's context (Evaluator::prepare)

    TermObjective(int K, const std::string& body) : TermObjective(LBFGSX_FORM_TERM, K, body, "TermObjective: ") {}
    // a handle compiled elsewhere (lbfgsx_objective_compile); it stays the caller's
    explicit TermObjective(const lbfgsx_objective* compiled) : m_h(const_cast<lbfgsx_objective*>(compiled)) {}

protected:
    // node: a GraphObjective's or MeshObjective's node body (empty: none); D: a MeshObjective's unknowns per node; edge: a
    // GraphLinearObjective's edge body
    TermObjective(int form, int K, const std::string& body, const char* who, const std::string& node = std::string(), int D = 1,
                  const std::string& edge = std::string())
    {
        std::vector<char> log(16384, '\0');
        const int dt = detail::dtype_of<Scalar>::value;
        const int rc = (form == LBFGSX_FORM_LINEAR_GRAPH) ? lbfgsx_objective_compile_linear_graph(&m_h, dt, node.c_str(), edge.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_DENSE) ? lbfgsx_objective_compile_dense(&m_h, dt, D, node.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_LINEAR_MULTI) ? lbfgsx_objective_compile_linear_multi(&m_h, dt, D, node.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_LINEAR)  ? lbfgsx_objective_compile_linear(&m_h, dt, node.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_MESH)  ? lbfgsx_objective_compile_mesh(&m_h, dt, K, D, node.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_GRAPH) ? lbfgsx_objective_compile_graph(&m_h, dt, node.c_str(), body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_GRID_STENCIL) ? lbfgsx_objective_compile_grid_stencil(&m_h, dt, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_GRID_FIELD) ? lbfgsx_objective_compile_grid_field(&m_h, dt, D, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_VOLUME_PERIODIC) ? lbfgsx_objective_compile_volume_periodic(&m_h, dt, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_GRID_PERIODIC) ? lbfgsx_objective_compile_grid_periodic(&m_h, dt, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_VOLUME) ? lbfgsx_objective_compile_volume(&m_h, dt, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_GRID)  ? lbfgsx_objective_compile_grid(&m_h, dt, body.c_str(), log.data(), log.size())
                       : (form == LBFGSX_FORM_CHAIN) ? lbfgsx_objective_compile_chain(&m_h, dt, K, body.c_str(), log.data(), log.size())
                                                     : lbfgsx_objective_compile(&m_h, dt, K, body.c_str(), log.data(), log.size());
        if (rc == LBFGSX_E_INVALID)
            throw std::invalid_argument(std::string(who) + log.data());
        if (rc != LBFGSX_OK)
            throw std::runtime_error(std::string(who) + log.data());
        m_own = true;
    }
    // form: the LBFGSX_FORM_* of the class (not of the handle: a handle of another form is refused by the form's bind call);
    // slabs = 0 on two axes, periodic = 0 for a form without a mask
    void set_lattice(int form, std::int64_t slabs, std::int64_t rows, std::int64_t cols, int periodic)
    {
        m_lattice = form;
        m_slabs = slabs;
        m_rows = rows;
        m_cols = cols;
        m_periodic = periodic;
    }
    void set_elements(std::int64_t E, const std::int32_t* elems, bool on_device)
    {
        m_E = E;
        m_elems = elems;
        m_edges_dev = on_device;
    }
    void set_matrix(std::int64_t R, std::int64_t nnz, const std::int32_t* rowptr, const std::int32_t* col, const Scalar* val,
                    bool on_device, int lanes)
    {
        m_R = R;
        m_nnz = nnz;
        m_rowptr = rowptr;
        m_col = col;
        m_val = val;
        m_matrix_dev = on_device;
        m_lanes = lanes;
    }
    void set_dense(std::int64_t R, const Scalar* A, std::int64_t lda, bool on_device, int lanes)
    {
        m_dense = true;
        m_R = R;
        m_A = A;
        m_lda = lda;
        m_matrix_dev = on_device;
        m_lanes = lanes;
    }
    void set_edges(std::int64_t E, const std::int32_t* ei, const std::int32_t* ej, bool on_device)
    {
        m_E = E;
        m_ei = ei;
        m_ej = ej;
        m_edges_dev = on_device;
    }

public:
    ~TermObjective()
    {
        if (m_own)
            lbfgsx_objective_destroy(m_h);
    }
    TermObjective& data(const Scalar* p0, const Scalar* p1 = nullptr, const Scalar* p2 = nullptr, const Scalar* p3 = nullptr)
    {
        m_p[0] = p0;
        m_p[1] = p1;
        m_p[2] = p2;
        m_p[3] = p3;
        return *this;
    }
    TermObjective& host_data(int slot, const Scalar* host)
    {
        if (slot < 0 || slot >= 4)
            throw std::invalid_argument("TermObjective: a term objective has at most four data arrays (slots 0..3)");
        m_host[slot] = host;
        m_count[slot] = 0;
        return *this;
    }
    // a host array of `count` elements (a GraphObjective's per-edge data has E, not n)
    TermObjective& host_data(int slot, const Scalar* host, std::int64_t count)
    {
        host_data(slot, host);
        m_count[slot] = count;
        return *this;
    }
    TermObjective& scalars(std::initializer_list<double> c) { return scalars(c.begin(), int(c.size())); }
    TermObjective& scalars(const double* c, int count)
    {
        if (count > 8)
            throw std::invalid_argument("TermObjective: a term objective has at most eight scalars");
        for (int k = 0; k < 8; k++)
            m_c[k] = (k < count) ? c[k] : 0.0;
        return *this;
    }
    const lbfgsx_objective* handle() const { return m_h; }
    // copy the host arrays, bind to the context: `id` is what the fused entry points take from here on
    void bind(lbfgsx_ctx* c)
    {
        const void* p[4];
        for (int k = 0; k < 4; k++)
        {
            p[k] = m_p[k];
            if (m_host[k])
            {
                void* dev = nullptr;
                if (m_count[k])
                    detail::check(lbfgsx_objective_upload_count(c, k, m_host[k], m_count[k], &dev));
                else
                    detail::check(lbfgsx_objective_upload(c, k, m_host[k], &dev));
                p[k] = dev;
            }
        }
        if (m_dense)
            detail::check(lbfgsx_objective_bind_dense(c, m_h, m_R, m_A, m_lda, m_matrix_dev ? 1 : 0, m_lanes, p, m_c, &id));
        else if ((m_rowptr || m_R || m_nnz) && (m_E || m_ei || m_ej))
            detail::check(lbfgsx_objective_bind_linear_graph(c, m_h, m_R, m_nnz, m_rowptr, m_col, m_val, m_matrix_dev ? 1 : 0, m_lanes,
                                                             m_E, m_ei, m_ej, m_edges_dev ? 1 : 0, p, m_c, &id));
        else if (m_rowptr || m_R || m_nnz)
            detail::check(lbfgsx_objective_bind_linear(c, m_h, m_R, m_nnz, m_rowptr, m_col, m_val, m_matrix_dev ? 1 : 0, m_lanes, p,
                                                       m_c, &id));
        else if (m_elems)
            detail::check(lbfgsx_objective_bind_mesh(c, m_h, m_E, m_elems, m_edges_dev ? 1 : 0, p, m_c, &id));
        else if (m_E || m_ei || m_ej)
            detail::check(lbfgsx_objective_bind_graph(c, m_h, m_E, m_ei, m_ej, m_edges_dev ? 1 : 0, p, m_c, &id));
        else
            detail::check(bind_lattice(c, p));
    }

private:
    // the bind call of the form the class declares; a GridObjective of 0 x 0 is bound as a class without a shape is
    int bind_lattice(lbfgsx_ctx* c, const void* const p[4])
    {
        switch (m_lattice)
        {
        case LBFGSX_FORM_GRID_FIELD: return lbfgsx_objective_bind_grid_field(c, m_h, m_rows, m_cols, m_periodic, p, m_c, &id);
        case LBFGSX_FORM_GRID_STENCIL: return lbfgsx_objective_bind_grid_stencil(c, m_h, m_rows, m_cols, m_periodic, p, m_c, &id);
        case LBFGSX_FORM_VOLUME_PERIODIC:
            return lbfgsx_objective_bind_volume_periodic(c, m_h, m_slabs, m_rows, m_cols, m_periodic, p, m_c, &id);
        case LBFGSX_FORM_GRID_PERIODIC: return lbfgsx_objective_bind_grid_periodic(c, m_h, m_rows, m_cols, m_periodic, p, m_c, &id);
        case LBFGSX_FORM_VOLUME: return lbfgsx_objective_bind_volume(c, m_h, m_slabs, m_rows, m_cols, p, m_c, &id);
        case LBFGSX_FORM_GRID:
            if (m_rows || m_cols)
                return lbfgsx_objective_bind_grid(c, m_h, m_rows, m_cols, p, m_c, &id);
            break;
        default: break;
        }
        return lbfgsx_objective_bind(c, m_h, p, m_c, &id);
    }
};

// An objective whose terms OVERLAP: f(x) = sum over t = 0 .. n-K of phi(x[t], .., x[t+K-1]; t), K = 2 or 3, one term starting
// at every coordinate (include/lbfgsx.h, "chain objectives").  The body is a TermObjective's; data, scalars and binding too.
//     ChainObjective<double> f(2, "const T u = x[1] - x[0] * x[0]; const T v = T(1) - x[0]; g[1] = T(200) * u;"
//                                 "g[0] = T(-400) * (u * x[0]) - T(2) * v; return T(100) * (u * u) + v * v;");   // chained Rosenbrock
// Accepted by LBFGSSolver::minimize and LBFGSBSolver::minimize wherever a TermObjective is, refused where it is.
template <typename Scalar>
class ChainObjective : public TermObjective<Scalar>
{
public:
    ChainObjective(int K, const std::string& body) : TermObjective<Scalar>(LBFGSX_FORM_CHAIN, K, body, "ChainObjective: ") {}
    // a handle compiled elsewhere (lbfgsx_objective_compile_chain); it stays the caller's
    explicit ChainObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
};

// An objective on a row-major rows x cols grid, x of rows*cols elements: f(x) = the sum over the (rows-1)(cols-1) cells of
// phi(x[r,c], x[r,c+1], x[r+1,c], x[r+1,c+1]; r, c) (include/lbfgsx.h, "grid objectives").  The body is the text of one cell:
// it sees T, const T x[4], T g[4], int64_t i (= row*cols + col), row, col, rows, cols, p0..p3 and c[8].
//     GridObjective<double> f(rows, cols, "const T a = x[1] - x[0]; const T b = x[2] - x[0]; g[1] = a; g[2] = b; g[3] = T(0);"
//                                         "g[0] = -a - b; return T(0.5) * (a * a + b * b);");
// data, scalars and binding are a TermObjective's.  Accepted by LBFGSSolver::minimize and LBFGSBSolver::minimize wherever a
// ChainObjective is, refused where it is; x.size() != rows*cols throws std::invalid_argument.
template <typename Scalar>
class GridObjective : public TermObjective<Scalar>
{
public:
    GridObjective(std::int64_t rows, std::int64_t cols, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_GRID, 4, body, "GridObjective: ")
    {
        this->set_lattice(LBFGSX_FORM_GRID, 0, rows, cols, 0);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_grid); it stays the caller's
    GridObjective(const lbfgsx_objective* compiled, std::int64_t rows, std::int64_t cols) : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_GRID, 0, rows, cols, 0);
    }
};

// An objective on a slab-major slabs x rows x cols array, x of slabs*rows*cols elements: f(x) = the sum over the
// (slabs-1)(rows-1)(cols-1) cells of phi(x[8]; s, r, c), x[4*ds + 2*dr + dc] = x[s+ds, r+dr, c+dc] (include/lbfgsx.h, "volume
// objectives").  The body is the text of one cell: it sees T, const T x[8], T g[8], int64_t i (= (slab*rows + row)*cols + col),
// slab, row, col, slabs, rows, cols, p0..p3 and c[8].
//     VolumeObjective<double> f(slabs, rows, cols, "const T a = x[1] - x[0]; const T b = x[2] - x[0]; const T e = x[4] - x[0];"
//         "for (int k = 0; k < 8; k++) g[k] = T(0); g[1] = a; g[2] = b; g[4] = e; g[0] = (-a - b) - e;"
//         "return T(0.5) * ((a * a + b * b) + e * e);");
// data, scalars and binding are a TermObjective's.  Accepted by LBFGSSolver::minimize and LBFGSBSolver::minimize wherever a
// GridObjective is, refused where it is; an extent < 2 or x.size() != slabs*rows*cols throws std::invalid_argument.
template <typename Scalar>
class VolumeObjective : public TermObjective<Scalar>
{
public:
    VolumeObjective(std::int64_t slabs, std::int64_t rows, std::int64_t cols, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_VOLUME, 8, body, "VolumeObjective: ")
    {
        this->set_lattice(LBFGSX_FORM_VOLUME, slabs, rows, cols, 0);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_volume); it stays the caller's
    VolumeObjective(const lbfgsx_objective* compiled, std::int64_t slabs, std::int64_t rows, std::int64_t cols)
        : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_VOLUME, slabs, rows, cols, 0);
    }
};

// A GridObjective with wrap-around cells (include/lbfgsx.h, "periodic grid and volume objectives"): periodic has bit 0 for the
// column direction and bit 1 for the row direction; cell (r, c) exists iff (c < cols-1 or bit 0) and (r < rows-1 or bit 1) and
// its corners are taken modulo the extents.  The body sees what a GridObjective's sees, and const int64_t j[4], the flat
// indices of its four corners (j[0] == i; read p0[j[k]], not p0[i + 1]: that is wrong at a seam), and int periodic.
//     PeriodicGridObjective<double> f(rows, cols, 3, "const T a = x[1] - x[0]; const T b = x[2] - x[0]; g[1] = a; g[2] = b;"
//                                                    "g[3] = T(0); g[0] = -a - b; return T(0.5) * (a * a + b * b);");
// Accepted and refused where a GridObjective is; a mask outside 0 .. 3 throws std::invalid_argument at minimize(), its value named.
template <typename Scalar>
class PeriodicGridObjective : public TermObjective<Scalar>
{
public:
    PeriodicGridObjective(std::int64_t rows, std::int64_t cols, int periodic, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_GRID_PERIODIC, 4, body, "PeriodicGridObjective: ")
    {
        this->set_lattice(LBFGSX_FORM_GRID_PERIODIC, 0, rows, cols, periodic);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_grid_periodic); it stays the caller's
    PeriodicGridObjective(const lbfgsx_objective* compiled, std::int64_t rows, std::int64_t cols, int periodic)
        : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_GRID_PERIODIC, 0, rows, cols, periodic);
    }
};

// A PeriodicGridObjective whose nodes carry D = 1, 2 or 3 unknowns (include/lbfgsx.h, "grid field objectives"): x is node-major,
// x[(r*cols + c)*D + d], n = rows*cols*D; periodic is the PeriodicGridObjective's mask, 0 = open.  The body is the text of one
// cell and sees T, constexpr int D, const T x[4*D] and T g[4*D] (x[k*D + d]: unknown d of corner k), int64_t i, row, col and
// const int64_t j[4] (NODE indices, j[0] == i; the flat coordinate of x[k*D + d] is j[k]*D + d), rows, cols, periodic, p0..p3
// and c[8].  At D = 1 the text of a PeriodicGridObjective compiles unchanged.
// Accepted and refused where a PeriodicGridObjective is; D outside 1 .. 3 throws std::invalid_argument at construction, a mask
// outside 0 .. 3 or a shape that does not multiply to n at minimize(), the values named.
template <typename Scalar>
class GridFieldObjective : public TermObjective<Scalar>
{
public:
    GridFieldObjective(std::int64_t rows, std::int64_t cols, int D, int periodic, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_GRID_FIELD, 4, body, "GridFieldObjective: ", std::string(), D)
    {
        this->set_lattice(LBFGSX_FORM_GRID_FIELD, 0, rows, cols, periodic);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_grid_field); it stays the caller's
    GridFieldObjective(const lbfgsx_objective* compiled, std::int64_t rows, std::int64_t cols, int periodic)
        : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_GRID_FIELD, 0, rows, cols, periodic);
    }
};

// An objective of 3x3-node terms on a row-major rows x cols grid, open or periodic per direction (include/lbfgsx.h, "grid
// stencil objectives"): rows >= 3, cols >= 3, periodic is the PeriodicGridObjective's mask, 0 = open.  Patch (r, c) has the nodes
// x[3*dr + dc] = x[r+dr, c+dc], dr, dc = 0, 1, 2, modulo the extents (its centre is x[4]), and exists iff (c < cols-2 or bit 0)
// and (r < rows-2 or bit 1).  The body is the text of one patch and sees T, const T x[9], T g[9], int64_t i, row, col (those of
// x[0]), const int64_t j[9] (the flat indices of the nine nodes, j[0] == i), rows, cols, periodic, p0..p3 and c[8].
//     StencilObjective<double> f(rows, cols, 3, "const T l = (((x[1] + x[3]) + x[5]) + x[7]) - T(4) * x[4];"
//         "for (int k = 0; k < 9; k++) g[k] = T(0); g[1] = l; g[3] = l; g[5] = l; g[7] = l; g[4] = T(-4) * l;"
//         "return T(0.5) * (l * l);");                                                        // sum (Laplace u)^2 / 2 on a torus
// Accepted and refused where a PeriodicGridObjective is; an extent < 3, a mask outside 0 .. 3 or a shape that does not multiply
// to n throws std::invalid_argument at minimize(), the values named.
template <typename Scalar>
class StencilObjective : public TermObjective<Scalar>
{
public:
    StencilObjective(std::int64_t rows, std::int64_t cols, int periodic, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_GRID_STENCIL, 9, body, "StencilObjective: ")
    {
        this->set_lattice(LBFGSX_FORM_GRID_STENCIL, 0, rows, cols, periodic);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_grid_stencil); it stays the caller's
    StencilObjective(const lbfgsx_objective* compiled, std::int64_t rows, std::int64_t cols, int periodic)
        : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_GRID_STENCIL, 0, rows, cols, periodic);
    }
};

// A VolumeObjective with wrap-around cells: periodic has bit 0 for the column, bit 1 for the row and bit 2 for the slab
// direction.  The body sees what a VolumeObjective's sees, and const int64_t j[8], the flat indices of its eight corners, and
// int periodic.  Accepted and refused where a VolumeObjective is; a mask outside 0 .. 7 throws std::invalid_argument at minimize(), its value named.
template <typename Scalar>
class PeriodicVolumeObjective : public TermObjective<Scalar>
{
public:
    PeriodicVolumeObjective(std::int64_t slabs, std::int64_t rows, std::int64_t cols, int periodic, const std::string& body)
        : TermObjective<Scalar>(LBFGSX_FORM_VOLUME_PERIODIC, 8, body, "PeriodicVolumeObjective: ")
    {
        this->set_lattice(LBFGSX_FORM_VOLUME_PERIODIC, slabs, rows, cols, periodic);
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_volume_periodic); it stays the caller's
    PeriodicVolumeObjective(const lbfgsx_objective* compiled, std::int64_t slabs, std::int64_t rows, std::int64_t cols, int periodic)
        : TermObjective<Scalar>(compiled)
    {
        this->set_lattice(LBFGSX_FORM_VOLUME_PERIODIC, slabs, rows, cols, periodic);
    }
};

// An objective on a graph: x has one coordinate per node and f(x) = sum over nodes v of psi(x[v]; v) + sum over the E edges
// of phi(x[ei[e]], x[ej[e]]; e) (include/lbfgsx.h, "graph objectives").  The edge body sees T, const T x[2] (the values at
// ei[e] and ej[e]), T g[2], int64_t e, i, j, p0..p3 and c[8]; the node body (optional) sees T, const T x[1], T g[1], int64_t i,
// p0..p3 and c[8].
//     GraphObjective<double> f("const T w = p0[e] * (x[0] - x[1]); g[0] = w; g[1] = T(0) - w; return T(0.5) * (w * (x[0] - x[1]));");
//     f.edges(E, ei, ej).host_data(0, weights, E);      solver.minimize(f, x, fx);
// edges(): int32 arrays of E elements on the host (or on the device: on_device = true) that stay valid until minimize()
// returns; the solver's context copies and validates them at every minimize() (a self-loop or an index outside [0, n) throws
// std::invalid_argument with the edge named).  data, scalars and binding are a TermObjective's.  Accepted by
// LBFGSSolver::minimize and LBFGSBSolver::minimize wherever a GridObjective is, refused where it is.
template <typename Scalar>
class GraphObjective : public TermObjective<Scalar>
{
public:
    explicit GraphObjective(const std::string& edge_body, const std::string& node_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_GRAPH, 2, edge_body, "GraphObjective: ", node_body)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_graph); it stays the caller's
    explicit GraphObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    GraphObjective& edges(std::int64_t E, const std::int32_t* ei, const std::int32_t* ej, bool on_device = false)
    {
        this->set_edges(E, ei, ej, on_device);
        return *this;
    }
};

// An objective on a mesh: N nodes with D unknowns each (x node-major, n = N*D), E elements of K nodes each, K in {2, 3, 4},
// D in {1, 2, 3} (include/lbfgsx.h, "mesh objectives").  The element body sees T, K, D, const T x[K*D] (x[k*D + d]: unknown d
// of the node in slot k), T g[K*D], int64_t e, const int64_t v[K], p0..p3 and c[8]; the node body (optional) sees T, D,
// const T x[D], T g[D], int64_t i, p0..p3 and c[8].
//     MeshObjective<double> f(3, 2, triangle_body);
//     f.elements(E, tris).host_data(0, rest_area, E);      solver.minimize(f, x, fx);
// elements(): an int32 array of E*K elements, row-major, on the host (or the device) that stays valid until minimize()
// returns; it is copied and validated at every minimize() (std::invalid_argument with the element named).  Otherwise a
// GraphObjective's interface; accepted wherever one is, refused where it is.
template <typename Scalar>
class MeshObjective : public TermObjective<Scalar>
{
public:
    MeshObjective(int K, int D, const std::string& elem_body, const std::string& node_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_MESH, K, elem_body, "MeshObjective: ", node_body, D)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_mesh); it stays the caller's
    explicit MeshObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    MeshObjective& elements(std::int64_t E, const std::int32_t* elems, bool on_device = false)
    {
        this->set_elements(E, elems, on_device);
        return *this;
    }
};

// A linear model fitted to data: f(x) = sum over coordinates j of psi(x[j]; j) + sum over the R rows of phi(z_r; r), z = A x,
// A sparse R x n in CSR (include/lbfgsx.h, "linear-model objectives").  The row body sees T, const T z, T& dz (to assign:
// phi'(z)), int64_t r, p0..p3 and c[8] and returns phi(z); the coordinate body (optional) is a GraphObjective's node body.
//     LinearObjective<double> f("const T m = T(1) - p0[r] * z; const T h = m > T(0) ? m : T(0);"
//                               "dz = T(-2) * (p0[r] * h); return h * h;", "g[0] = c[0] * x[0]; return T(0.5) * (c[0] * (x[0] * x[0]));");
//     f.matrix(R, nnz, rowptr, col, val).host_data(0, labels, R).scalars({1e-3});      solver.minimize(f, x, fx);
// matrix(): int32 rowptr[R+1], col[nnz] and Scalar val[nnz] on the host (or on the device: on_device = true) that stay valid
// until minimize() returns; the solver's context copies and validates them at every minimize() (a malformed rowptr or a
// column outside [0, n) throws std::invalid_argument with the position named).  lanes: the lanes that share a row, 0 = by the
// library's rule.  Otherwise a GraphObjective's interface; accepted wherever one is, refused where it is.
template <typename Scalar>
class LinearObjective : public TermObjective<Scalar>
{
public:
    explicit LinearObjective(const std::string& row_body, const std::string& coord_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_LINEAR, 1, row_body, "LinearObjective: ", coord_body)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_linear); it stays the caller's
    explicit LinearObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    LinearObjective& matrix(std::int64_t R, std::int64_t nnz, const std::int32_t* rowptr, const std::int32_t* col, const Scalar* val,
                            bool on_device = false, int lanes = 0)
    {
        this->set_matrix(R, nnz, rowptr, col, val, on_device, lanes);
        return *this;
    }
};

// A linear model with a coupling term over a graph on its weights: f(x) = sum over coordinates j of psi(x[j]; j) + sum over the
// E edges of rho(x[ei[e]], x[ej[e]]; e) + sum over the R rows of phi(z_r; r), z = A x (include/lbfgsx.h, "graph-regularised
// linear-model objectives") -- reconstruction with a smoothness prior under bounds, regression with a GMRF prior, Laplacian-
// regularised least squares.  The row and coordinate bodies are a LinearObjective's, the edge body a GraphObjective's; the three
// share p0..p3 and c[8], so a data array has n, E or R elements.
//     GraphLinearObjective<double> f("const T u = z - p0[r]; dz = u; return T(0.5) * (u * u);",
//                                    "const T d = x[0] - x[1]; const T w = c[0] * d; g[0] = w; g[1] = T(0) - w; return T(0.5) * (w * d);");
//     f.matrix(R, nnz, rowptr, col, val).edges(E, ei, ej).host_data(0, b, R).scalars({lambda});      solver.minimize(f, x, fx, lb, ub);
// matrix() is a LinearObjective's and edges() a GraphObjective's, with their validation at every minimize().  Accepted wherever
// a LinearObjective is, refused where it is.
template <typename Scalar>
class GraphLinearObjective : public TermObjective<Scalar>
{
public:
    GraphLinearObjective(const std::string& row_body, const std::string& edge_body, const std::string& coord_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_LINEAR_GRAPH, 1, row_body, "GraphLinearObjective: ", coord_body, 1, edge_body)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_linear_graph); it stays the caller's
    explicit GraphLinearObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    GraphLinearObjective& matrix(std::int64_t R, std::int64_t nnz, const std::int32_t* rowptr, const std::int32_t* col,
                                 const Scalar* val, bool on_device = false, int lanes = 0)
    {
        this->set_matrix(R, nnz, rowptr, col, val, on_device, lanes);
        return *this;
    }
    GraphLinearObjective& edges(std::int64_t E, const std::int32_t* ei, const std::int32_t* ej, bool on_device = false)
    {
        this->set_edges(E, ei, ej, on_device);
        return *this;
    }
};

// A linear model with D outputs per sample: x holds an F x D weight matrix, feature-major (x[j*D + c], n = F*D), A is a sparse
// R x F CSR matrix, Z = A X and f(x) = sum over coordinates i of psi(x[i]; i) + sum over rows r of phi(Z[r, 0..D); r)
// (include/lbfgsx.h, "multi-output linear-model objectives"): softmax regression, multi-class SVMs, multi-target least
// squares.  D = 1 .. 16.  The row body sees T, D, const T z[D], T dz[D] (to fill), int64_t r, p0..p3 and c[8] and returns phi;
// the coordinate body (optional) is a LinearObjective's, per coordinate i = j*D + c.
//     MultiLinearObjective<double> f(3, "T s = T(0);\n#pragma unroll\nfor (int c = 0; c < D; c++) { dz[c] = z[c] - p0[r * D + c];"
//                                       " s = s + dz[c] * dz[c]; } return T(0.5) * s;");
//     f.matrix(R, nnz, rowptr, col, val).host_data(0, targets, R * 3);      solver.minimize(f, x, fx);
// matrix(): a LinearObjective's, with col in [0, F); x.size() not a multiple of D throws std::invalid_argument.  Accepted
// wherever a LinearObjective is, refused where it is.
template <typename Scalar>
class MultiLinearObjective : public TermObjective<Scalar>
{
public:
    MultiLinearObjective(int D, const std::string& row_body, const std::string& coord_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_LINEAR_MULTI, 1, row_body, "MultiLinearObjective: ", coord_body, D)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_linear_multi); it stays the caller's
    explicit MultiLinearObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    MultiLinearObjective& matrix(std::int64_t R, std::int64_t nnz, const std::int32_t* rowptr, const std::int32_t* col,
                                 const Scalar* val, bool on_device = false, int lanes = 0)
    {
        this->set_matrix(R, nnz, rowptr, col, val, on_device, lanes);
        return *this;
    }
};

// The multi-output linear model over a DENSE matrix: x holds an F x D weight matrix, feature-major (x[j*D + c], n = F*D), A is
// R x F, row-major with a row stride of lda >= F elements, Z = A X and f(x) = sum over coordinates i of psi(x[i]; i) + sum over
// rows r of phi(Z[r, 0..D); r) (include/lbfgsx.h, "dense linear-model objectives"): logistic, softmax, Poisson and
// least-squares regression on tabular features, NNLS under LBFGSBSolver.  D = 1 .. 16; the bodies are a
// MultiLinearObjective's (D = 1: z[0], dz[0]).
//     DenseLinearObjective<double> f(1, "const T m = p0[r] * z[0]; ... return ...;", "g[0] = c[0] * x[0]; return T(0.5) * (c[0] * (x[0] * x[0]));");
//     f.matrix(R, A, F).host_data(0, labels, R).scalars({1e-3});      solver.minimize(f, x, fx);
// matrix(): a host array, copied to the device at every minimize(), or a device array (on_device = true) that is used in
// place, NOT copied: it stays alive and unchanged until minimize() returns.  lda < x.size() / D, R < 1 and x.size() not a
// multiple of D throw std::invalid_argument.  Accepted wherever a MultiLinearObjective is, refused where it is.
template <typename Scalar>
class DenseLinearObjective : public TermObjective<Scalar>
{
public:
    DenseLinearObjective(int D, const std::string& row_body, const std::string& coord_body = std::string())
        : TermObjective<Scalar>(LBFGSX_FORM_DENSE, 1, row_body, "DenseLinearObjective: ", coord_body, D)
    {
    }
    // a handle compiled elsewhere (lbfgsx_objective_compile_dense); it stays the caller's
    explicit DenseLinearObjective(const lbfgsx_objective* compiled) : TermObjective<Scalar>(compiled) {}
    DenseLinearObjective& matrix(std::int64_t R, const Scalar* A, std::int64_t lda, bool on_device = false, int lanes = 0)
    {
        this->set_dense(R, A, lda, on_device, lanes);
        return *this;
    }
};

namespace detail {
// the objectives compiled at run time into the fused kernels: a TermObjective, a ChainObjective, a GridObjective, a
// VolumeObjective, a GraphObjective, a MeshObjective, a LinearObjective, a GraphLinearObjective, a MultiLinearObjective or a DenseLinearObjective
template <typename Scalar, typename Foo>
struct is_compiled_objective
{
    typedef typename std::decay<Foo>::type F;
    static constexpr bool value = std::is_same<F, TermObjective<Scalar> >::value || std::is_same<F, ChainObjective<Scalar> >::value ||
                                  std::is_same<F, GridObjective<Scalar> >::value || std::is_same<F, GraphObjective<Scalar> >::value ||
                                  std::is_same<F, VolumeObjective<Scalar> >::value ||
                                  std::is_same<F, PeriodicGridObjective<Scalar> >::value ||
                                  std::is_same<F, PeriodicVolumeObjective<Scalar> >::value ||
                                  std::is_same<F, GridFieldObjective<Scalar> >::value ||
                                  std::is_same<F, StencilObjective<Scalar> >::value ||
                                  std::is_same<F, MeshObjective<Scalar> >::value || std::is_same<F, LinearObjective<Scalar> >::value ||
                                  std::is_same<F, MultiLinearObjective<Scalar> >::value ||
                                  std::is_same<F, GraphLinearObjective<Scalar> >::value ||
                                  std::is_same<F, DenseLinearObjective<Scalar> >::value;
};
}  // namespace detail

template <typename Scalar>
class DeviceState
{
    lbfgsx_ctx* m_c = nullptr;
    std::int64_t m_n = 0;
    int m_m = 0, m_flags = 0, m_device = 0;

    DeviceState(const DeviceState&) = delete;
    DeviceState& operator=(const DeviceState&) = delete;

public:
    DeviceState() {}
    ~DeviceState() { release(); }
    void release()
    {
        if (m_c)
            lbfgsx_destroy(m_c);
        m_c = nullptr;
    }
    // (re)allocate for dimension n and history m; keeps the allocation when nothing changed
    void ensure(std::int64_t n, int m, int flags = 0, int device = 0)
    {
        if (m_c && n == m_n && m == m_m && flags == m_flags && device == m_device)
            return;
        release();
        detail::check(lbfgsx_create(&m_c, detail::dtype_of<Scalar>::value, n, m, device, flags));
        m_n = n;
        m_m = m;
        m_flags = flags;
        m_device = device;
    }
    lbfgsx_ctx* ctx() const { return m_c; }
    std::int64_t size() const { return m_n; }
    int m() const { return m_m; }
    DeviceVector<Scalar> vec(int which) const
    {
        return DeviceVector<Scalar>(static_cast<Scalar*>(lbfgsx_vec(m_c, which)), m_n);
    }
    void upload(int which, const Scalar* host) { detail::check(lbfgsx_upload(m_c, which, host)); }
    void download(int which, Scalar* host) const { detail::check(lbfgsx_download(m_c, which, host)); }
    void sync() const { detail::check(lbfgsx_sync(m_c)); }
};

namespace detail {

// Uniform view of the four kinds of objective `Foo` the solvers accept:
//   BuiltinObjective<Scalar>                              -> fused device kernels
//   TermObjective<Scalar>, ChainObjective<Scalar>, GridObjective<Scalar>, VolumeObjective<Scalar>, GraphObjective<Scalar>,
//   MeshObjective<Scalar>
//                                                         -> the same kernels, compiled at run time
//   Scalar f(const DeviceVector<Scalar>& x, DeviceVector<Scalar>& grad)   -> user device functor
//   Scalar f(const Vec& x, Vec& grad) with host vectors   -> staged through host memory (compatibility)
template <typename Scalar, typename Foo, typename HostVec>
class Evaluator
{
    Foo& m_f;
    DeviceState<Scalar>& m_s;
    HostVec m_hx, m_hg;  // staging for host functors only
    int m_nfev = 0;

    static constexpr bool is_term = is_compiled_objective<Scalar, Foo>::value;
    // evaluated inside the fused kernels under an objective id: the two built-in ones and a bound term objective
    static constexpr bool is_builtin = is_term || std::is_same<typename std::decay<Foo>::type, BuiltinObjective<Scalar> >::value;
    // A functor that accepts the caller's host vectors is a host functor even if it would also accept device vectors
    // (a generic `template <class V> operator()(const V&, V&)` or `[](const auto& x, auto& g)` satisfies both traits;
    // handing it raw HBM pointers to dereference on the host would crash).  Device functors name DeviceVector.
    static constexpr bool is_host = !is_builtin && std::is_invocable<Foo&, const HostVec&, HostVec&>::value;
    static constexpr bool is_device =
        !is_host && std::is_invocable<Foo&, const DeviceVector<Scalar>&, DeviceVector<Scalar>&>::value;

    // evaluate the user functor at (xwhich) writing (gwhich); returns fx
    Scalar call_user(int xwhich, int gwhich)
    {
        if constexpr (is_builtin)
        {
            return Scalar(0);
        }
        else if constexpr (is_device)
        {
            // The point was produced by a kernel on the context's (non-blocking) stream: drain it, so the functor may
            // use any stream of its own.  The functor returns f as a host scalar, i.e. its own work is complete when it
            // returns and the solver's next kernel may read the gradient it wrote.
            m_s.sync();
            DeviceVector<Scalar> x = m_s.vec(xwhich), g = m_s.vec(gwhich);
            // the functor launches its own kernels on x and g: they live on the context's device, which need not be the
            // calling thread's current one (set_device(k), several solvers per thread) -- make it current for the call
            struct Current
            {
                int prev = -1;
                explicit Current(lbfgsx_ctx* c) { check(lbfgsx_device_push(c, &prev)); }
                ~Current() { (void) lbfgsx_device_pop(prev); }
            } current(m_s.ctx());
            const Scalar fx = m_f(static_cast<const DeviceVector<Scalar>&>(x), g);
            return fx;
        }
        else
        {
            if (std::int64_t(m_hx.size()) != m_s.size())
            {
                m_hx.resize(m_s.size());
                m_hg.resize(m_s.size());
            }
            m_s.download(xwhich, m_hx.data());
            const Scalar fx = m_f(static_cast<const HostVec&>(m_hx), m_hg);
            m_s.upload(gwhich, m_hg.data());
            return fx;
        }
    }

public:
    std::function<void(int, Scalar)> on_eval;  // (evaluation index, fx) -- parity tracing hook
    // Row-sharded runs (LBFGSSolver::set_reducer): every bundle of n-length sums a statement returns is summed over
    // the shards (an all-reduce) before any scalar logic sees it, so all ranks take identical decisions.
    std::function<void(double*, int)> reduce;
    // has the line search in progress written a trial point (x = xp + step * drt) yet?  A search that throws afterwards
    // leaves that point in the caller's x, as the reference's policies do; one that throws at its entry checks, or an
    // exception from anywhere else, leaves the current iterate there.  The solver clears it before every search.
    bool trial_written = false;

    Evaluator(Foo& f, DeviceState<Scalar>& s) : m_f(f), m_s(s) {}
    // the id of a built-in or bound term objective (the fused kernels know it), -1 for a functor
    int builtin_id() const
    {
        if constexpr (is_builtin)
            return m_f.id;
        else
            return -1;
    }
    int nfev() const { return m_nfev; }

    void prepare()
    {
        if constexpr (is_term)
            m_f.bind(m_s.ctx());
        else if constexpr (is_builtin)
        {
            if (m_f.a) m_s.upload(LBFGSX_VEC_A, m_f.a);
            if (m_f.b) m_s.upload(LBFGSX_VEC_B, m_f.b);
        }
    }
    // fx = f(x, grad); |grad|^2; |x|^2     (LBFGS.h:91-92,100)
    void initial(Scalar& fx, Scalar& gnorm2, Scalar& xnorm2)
    {
        double r0 = 0, r1 = 0, r2 = 0;
        if constexpr (is_builtin)
        {
            check(lbfgsx_eval(m_s.ctx(), m_f.id, &r0, &r1, &r2));
        }
        else
        {
            r0 = double(call_user(LBFGSX_VEC_X, LBFGSX_VEC_G));
            check(lbfgsx_norms(m_s.ctx(), &r1, &r2));
        }
        if (reduce)
        {
            double r[3] = {r0, r1, r2};
            reduce(r, 3);
            r0 = r[0];
            r1 = r[1];
            r2 = r[2];
        }
        fx = Scalar(r0);
        gnorm2 = Scalar(r1);
        xnorm2 = Scalar(r2);
        if (on_eval) on_eval(m_nfev, fx);
        m_nfev++;
    }
    // fx = f(x, grad); ||P(x-g,l,u)-x||_inf; |x|^2     (LBFGSB.h:137-138,146)
    void initial_bounded(Scalar& fx, Scalar& projgnorm, Scalar& xnorm2)
    {
        double r0 = 0, r1 = 0, r2 = 0;
        if constexpr (is_builtin)
        {
            check(lbfgsx_b_eval(m_s.ctx(), m_f.id, &r0, &r1, &r2));
        }
        else
        {
            r0 = double(call_user(LBFGSX_VEC_X, LBFGSX_VEC_G));
            check(lbfgsx_b_norms(m_s.ctx(), &r1, &r2));
        }
        fx = Scalar(r0);
        projgnorm = Scalar(r1);
        xnorm2 = Scalar(r2);
        if (on_eval) on_eval(m_nfev, fx);
        m_nfev++;
    }
    // x = xp + step*drt; fx = f(x, grad); dg = grad.dot(drt)
    void trial(Scalar step, Scalar& fx, Scalar& dg)
    {
        double r0 = 0, r1 = 0;
        if constexpr (is_builtin)
        {
            check(lbfgsx_trial(m_s.ctx(), m_f.id, double(step), &r0, &r1));
            trial_written = true;
        }
        else
        {
            check(lbfgsx_trial_point(m_s.ctx(), double(step)));
            trial_written = true;
            r0 = double(call_user(LBFGSX_VEC_XT, LBFGSX_VEC_GT));
            check(lbfgsx_trial_dg(m_s.ctx(), &r1));
        }
        if (reduce)
        {
            double r[2] = {r0, r1};
            reduce(r, 2);
            r0 = r[0];
            r1 = r[1];
        }
        fx = Scalar(r0);
        dg = Scalar(r1);
        if (on_eval) on_eval(m_nfev, fx);
        m_nfev++;
    }
    // ---- grad.dot(drt) from the first trial (lbfgsx.h: lbfgsx_last_in_trial_request).  The solver sets dg_pending when the
    // product that precedes a search returned no grad.d; a policy whose device form knows the protocol (its constant
    // takes_pending_dg) clears it and calls first_trial instead of trial for its first step: dg_init = grad.dot(drt) at xp comes
    // back with fx and dg.  When dg_init >= 0 -- the entry check the policy could not make earlier -- nothing has happened as
    // far as the caller can tell: the evaluation is not counted, no trial point is reported written (the pass wrote the trial
    // buffer only), fx and dg are not assigned.
    bool dg_pending = false;
    bool first_trial(Scalar step, Scalar& fx, Scalar& dg, Scalar& dg_init)
    {
        double r0 = 0, r1 = 0, r2 = 0;
        if constexpr (is_builtin)
            check(lbfgsx_trial_first(m_s.ctx(), m_f.id, double(step), &r0, &r1, &r2));
        else  // the solver asks for the protocol with a built-in objective only (LBFGS.h)
            throw std::logic_error("grad.dot(drt) is pending for an objective evaluated outside the fused kernels");
        dg_init = Scalar(r2);
        if (dg_init >= Scalar(0))
            return false;
        trial_written = true;
        fx = Scalar(r0);
        dg = Scalar(r1);
        if (on_eval) on_eval(m_nfev, fx);
        m_nfev++;
        return true;
    }
    // ---- compatibility path of detail::run_line_search (LBFGSpp/Interop.h): a line-search policy with the reference's
    // signature drives the search on host vectors.  fx = f(x, grad) at a host point, whatever kind of objective Foo is.
    template <typename Vec>
    Scalar eval_host_point(const Vec& x, Vec& grad)
    {
        Scalar fx;
        if constexpr (is_builtin)
        {
            // the point goes into the trial buffer, which becomes the current one for the evaluation kernel
            m_s.upload(LBFGSX_VEC_XT, x.data());
            check(lbfgsx_ls_end(m_s.ctx(), 0));
            double r0 = 0;
            check(lbfgsx_eval(m_s.ctx(), m_f.id, &r0, nullptr, nullptr));
            m_s.download(LBFGSX_VEC_G, grad.data());
            fx = Scalar(r0);
        }
        else if constexpr (is_device)
        {
            m_s.upload(LBFGSX_VEC_XT, x.data());
            fx = call_user(LBFGSX_VEC_XT, LBFGSX_VEC_GT);
            m_s.download(LBFGSX_VEC_GT, grad.data());
        }
        else
            fx = m_f(x, grad);
        if (on_eval) on_eval(m_nfev, fx);
        m_nfev++;
        return fx;
    }
    // the point the policy settled on becomes the accepted one (x, grad of LBFGS.h:127 after the search)
    template <typename Vec>
    void finish_host_point(const Vec& x, const Vec& grad)
    {
        m_s.upload(LBFGSX_VEC_XT, x.data());
        m_s.upload(LBFGSX_VEC_GT, grad.data());
        check(lbfgsx_ls_end(m_s.ctx(), 0));
    }
    // x_lo.swap(x); grad_lo.swap(grad)
    void keep_trial_as_lo() { check(lbfgsx_ls_keep_trial_as_lo(m_s.ctx())); }
    // accepted point = last trial (use_lo = false) or the saved _lo point
    void finish(bool use_lo) { check(lbfgsx_ls_end(m_s.ctx(), use_lo ? 1 : 0)); }
    DeviceState<Scalar>& state() { return m_s; }
};

}  // namespace detail
}  // namespace LBFGSpp

#endif  // LBFGSX_DROPIN_DEVICE_H
