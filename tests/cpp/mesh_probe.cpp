// tests/cpp/mesh_probe.cpp -- a polynomial triangle energy on a triangulated lattice, K = 3 nodes per element, D = 2
// unknowns per node (positions in the plane):
//     f(x) = sum over triangles e of 1/4 ((|a|^2 - l0_e)^2 + (|b|^2 - l1_e)^2 + (|c|^2 - l2_e)^2) + c0/2 (a x b - c1)^2
//          + sum over nodes v of c2/2 |x_v - rest_v|^2,
// a, b, c the triangle's three edge vectors (0->1, 1->2, 2->0), l0..l2 their squared rest lengths, a x b the doubled signed
// area and c1 its rest value, through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with a box that
// becomes active, iterate by iterate.  The mesh: rows x cols nodes, node r*cols + c at rest position (c, r); each cell
// (r, c) with i = r*cols + c gives the triangles (i, i+1, i+cols+1) and (i, i+cols+1, i+cols), cells in row-major order.
// The start is the rest mesh under a smooth perturbation.
//
// One source, two builds:
//   * plain:              a host functor, compiled against the headers on the include path -- the reference's with
//                         oracle/eigen_shim as Eigen for the fixture (tests/golden/make_mesh_golden.py);
//   * -DMESH_PROBE_DEVICE a MeshObjective<double> with the same two terms, compiled against include/ and run on the GPU
//                         (tests/test_mesh_objective_gpu.py).
// The functor states both terms operation by operation as the bodies do and adds the contributions to grad[v*2 + d] in the
// order of include/lbfgsx.h (the node term, then the elements that contain v in ascending e); f is summed with a compensated
// accumulator, so its value does not depend on the order of the terms.
//
//     mesh_probe <rows> <cols> <max iterations recorded>
// prints, for each solver, one line per k = 1 .. max:  <solver> <k> <niter> <nfev> <f> <x[0]> .. <x[n-1]>   (%.17g),
// the state after a run with max_iterations = k (the solvers are deterministic, so run k+1 repeats run k and goes on).
#include <Eigen/Core>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <utility>
#include <vector>

#include <LBFGS.h>
#include <LBFGSB.h>

using namespace LBFGSpp;
typedef Eigen::Matrix<double, Eigen::Dynamic, 1> Vector;

static const double kC0 = 2.0;    // weight of the area term
static const double kC1 = 1.0;    // doubled signed area of a rest triangle
static const double kC2 = 4.0;    // stiffness of the tie to the rest position
static const double kAmp = 0.05;  // amplitude of the start's perturbation
static const double kLo = -0.02;  // the box of the L-BFGS-B runs, relative to the rest mesh's extent in each direction
static const double kHi = 0.03;

static const char* const kElemBody =
    "const T ax = x[2] - x[0], ay = x[3] - x[1];\n"
    "const T bx = x[4] - x[2], by = x[5] - x[3];\n"
    "const T cx = x[0] - x[4], cy = x[1] - x[5];\n"
    "const T ra = (ax * ax + ay * ay) - p0[e];\n"
    "const T rb = (bx * bx + by * by) - p1[e];\n"
    "const T rc = (cx * cx + cy * cy) - p2[e];\n"
    "const T ar = (ax * by - ay * bx) - c[1];\n"
    "const T wa = c[0] * ar;\n"
    "g[0] = (rc * cx - ra * ax) - wa * by;\n"
    "g[1] = (rc * cy - ra * ay) + wa * bx;\n"
    "g[2] = (ra * ax - rb * bx) - wa * cy;\n"
    "g[3] = (ra * ay - rb * by) + wa * cx;\n"
    "g[4] = (rb * bx - rc * cx) - wa * ay;\n"
    "g[5] = (rb * by - rc * cy) + wa * ax;\n"
    "return T(0.25) * ((ra * ra + rb * rb) + rc * rc) + T(0.5) * (wa * ar);";
static const char* const kNodeBody =
    "T s = T(0);\n"
    "for (int d = 0; d < D; d++)\n"
    "{\n"
    "    const T r = x[d] - p3[i * D + d];\n"
    "    const T k = c[2] * r;\n"
    "    g[d] = k;\n"
    "    s = s + T(0.5) * (k * r);\n"
    "}\n"
    "return s;";

struct Mesh
{
    int rows, cols, N;
    std::vector<std::int32_t> el;         // E x 3
    std::vector<double> l0, l1, l2, rest;  // per element; rest: N x 2
    Mesh(int rows_, int cols_) : rows(rows_), cols(cols_), N(rows_ * cols_)
    {
        for (int r = 0; r + 1 < rows; r++)
            for (int c = 0; c + 1 < cols; c++)
            {
                const int i = r * cols + c;
                const int t[2][3] = {{i, i + 1, i + cols + 1}, {i, i + cols + 1, i + cols}};
                for (int k = 0; k < 2; k++)
                    for (int j = 0; j < 3; j++)
                        el.push_back(t[k][j]);
            }
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                rest.push_back(double(c));
                rest.push_back(double(r));
            }
        for (size_t e = 0; e < el.size() / 3; e++)
        {
            double len[3];
            for (int j = 0; j < 3; j++)
            {
                const int u = el[3 * e + j], v = el[3 * e + (j + 1) % 3];
                const double dx = rest[2 * v] - rest[2 * u], dy = rest[2 * v + 1] - rest[2 * u + 1];
                len[j] = dx * dx + dy * dy;
            }
            l0.push_back(len[0]);
            l1.push_back(len[1]);
            l2.push_back(len[2]);
        }
    }
    std::int64_t E() const { return std::int64_t(el.size() / 3); }
};

struct TriangleEnergy
{
    const Mesh& M;
    int calls = 0;
    std::vector<std::vector<std::pair<int, int> > > inc;  // per node: (e, slot), ascending e
    std::vector<double> tg;                               // E x 6
    explicit TriangleEnergy(const Mesh& m) : M(m), inc(size_t(m.N))
    {
        for (std::int64_t e = 0; e < M.E(); e++)
            for (int k = 0; k < 3; k++)
                inc[size_t(M.el[3 * e + k])].push_back(std::make_pair(int(e), k));
    }
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every term
        auto add = [&](double val) {
            const double s = hi + val;
            const double bb = s - hi;
            lo += (hi - (s - bb)) + (val - bb);
            hi = s;
        };
        tg.resize(size_t(M.E()) * 6);
        for (std::int64_t e = 0; e < M.E(); e++)
        {
            double X[6];
            for (int k = 0; k < 3; k++)
                for (int d = 0; d < 2; d++)
                    X[2 * k + d] = x[2 * M.el[3 * e + k] + d];
            const double ax = X[2] - X[0], ay = X[3] - X[1];
            const double bx = X[4] - X[2], by = X[5] - X[3];
            const double cx = X[0] - X[4], cy = X[1] - X[5];
            const double ra = (ax * ax + ay * ay) - M.l0[size_t(e)];
            const double rb = (bx * bx + by * by) - M.l1[size_t(e)];
            const double rc = (cx * cx + cy * cy) - M.l2[size_t(e)];
            const double ar = (ax * by - ay * bx) - kC1;
            const double wa = kC0 * ar;
            double* g = &tg[size_t(e) * 6];
            g[0] = (rc * cx - ra * ax) - wa * by;
            g[1] = (rc * cy - ra * ay) + wa * bx;
            g[2] = (ra * ax - rb * bx) - wa * cy;
            g[3] = (ra * ay - rb * by) + wa * cx;
            g[4] = (rb * bx - rc * cx) - wa * ay;
            g[5] = (rb * by - rc * cy) + wa * ax;
            add(0.25 * ((ra * ra + rb * rb) + rc * rc) + 0.5 * (wa * ar));
        }
        for (int v = 0; v < M.N; v++)
        {
            double acc[2], s = 0.0;
            for (int d = 0; d < 2; d++)
            {
                const double r = x[2 * v + d] - M.rest[size_t(2 * v + d)];
                const double k = kC2 * r;
                acc[d] = k;
                s = s + 0.5 * (k * r);
            }
            add(s);
            for (const std::pair<int, int>& en : inc[size_t(v)])
                for (int d = 0; d < 2; d++)
                    acc[d] = acc[d] + tg[size_t(en.first) * 6 + size_t(en.second) * 2 + size_t(d)];
            grad[2 * v] = acc[0];
            grad[2 * v + 1] = acc[1];
        }
        return hi + lo;
    }
};

// the rest mesh under a smooth perturbation, no two unknowns alike; divisions, products and sums only, so that the test's
// numpy restatement gives the same doubles
static Vector start(const Mesh& M)
{
    Vector x(2 * M.N);
    for (int v = 0; v < M.N; v++)
    {
        const double t = double(v + 1) / double(M.N + 1);
        const double bump = (12.0 * ((t * (1.0 - t)) * (0.5 - t))) * (1.0 + 0.5 * t);
        x[2 * v] = M.rest[size_t(2 * v)] + kAmp * bump;
        x[2 * v + 1] = M.rest[size_t(2 * v + 1)] + (kAmp * 0.5) * (bump * (1.0 - t));
    }
    return x;
}

static void emit(const char* solver, int k, int niter, int nfev, double fx, const Vector& x)
{
    std::printf("%s %d %d %d %.17g", solver, k, niter, nfev, fx);
    for (int i = 0; i < int(x.size()); i++)
        std::printf(" %.17g", x[i]);
    std::printf("\n");
}

#ifdef MESH_PROBE_DEVICE
static void setup(MeshObjective<double>& f, const Mesh& M)
{
    f.elements(M.E(), M.el.data());
    f.host_data(0, M.l0.data(), M.E());
    f.host_data(1, M.l1.data(), M.E());
    f.host_data(2, M.l2.data(), M.E());
    f.host_data(3, M.rest.data(), std::int64_t(M.rest.size()));
    f.scalars({kC0, kC1, kC2});
}
#endif

int main(int argc, char** argv)
{
    if (argc < 4)
    {
        std::fprintf(stderr, "usage: mesh_probe <rows> <cols> <iterations>\n");
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), kmax = std::atoi(argv[3]);
    const Mesh M(rows, cols);
    const int n = 2 * M.N;
    try
    {
        for (int k = 1; k <= kmax; k++)
        {
            LBFGSParam<double> param;
            param.m = 6;
            param.epsilon = 0;
            param.epsilon_rel = 0;
            param.max_iterations = k;
            LBFGSSolver<double, LineSearchMoreThuente> solver(param);
            Vector x = start(M);
            double fx = 0;
#ifdef MESH_PROBE_DEVICE
            MeshObjective<double> f(3, 2, kElemBody, kNodeBody);
            setup(f, M);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            TriangleEnergy f(M);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, f.calls, fx, x);
#endif
        }
        for (int k = 1; k <= kmax; k++)
        {
            LBFGSBParam<double> param;
            param.m = 6;
            param.epsilon = 0;
            param.epsilon_rel = 0;
            param.past = 0;
            param.max_iterations = k;
            LBFGSBSolver<double> solver(param);
            Vector x = start(M), lb(n), ub(n);
            for (int i = 0; i < n; i++)
            {
                lb[i] = M.rest[size_t(i)] + kLo;
                ub[i] = M.rest[size_t(i)] + kHi;
            }
            double fx = 0;
#ifdef MESH_PROBE_DEVICE
            MeshObjective<double> f(3, 2, kElemBody, kNodeBody);
            setup(f, M);
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            TriangleEnergy f(M);
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, f.calls, fx, x);
#endif
        }
    }
    catch (const std::exception& e)
    {
        std::printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    std::printf("MESH PROBE OK\n");
    return 0;
}
