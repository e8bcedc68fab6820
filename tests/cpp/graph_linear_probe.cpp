// tests/cpp/graph_linear_probe.cpp -- two graph-regularised linear models over one sparse R x n matrix A, z = A x, and one graph
// on the n coordinates:
//     squared hinge + ridge + quartic coupling
//         f(x) = sum over rows r of max(0, 1 - y_r z_r)^2 + sum over j of c0/2 x_j^2 + sum over edges e of c1/4 (x_i - x_j)^4
//         through LBFGSSolver with the More-Thuente search,
//     non-negative least squares with a quadratic smoothness term
//         f(x) = sum over rows r of 1/2 (z_r - b_r)^2 + sum over edges e of c1/2 (x_i - x_j)^2,  0 <= x
//         through LBFGSBSolver from a start with negative entries (bounds active at the start),
// iterate by iterate.  The matrix is tests/cpp/linear_probe.cpp's: row r has kPer entries, entry j in column
// (7 r + 3 j j + j) mod n with value (((31 r + 17 j) mod 13) - 6) / 4; y_r = -1 where 5 r mod 3 = 0 and +1 elsewhere;
// b_r = ((11 r mod 7) - 3) / 2.  The graph is tests/cpp/graph_probe.cpp's: for t = 0 .. n-1 the edge (t, (t+1) mod n), then,
// when t mod 3 = 0 and u = (7 t + 3) mod n differs from t, the chord (u, t).  Integers and exact quotients only, no
// transcendental function, so that the test's numpy restatement gives the same doubles.
//
// One source, two builds:
//   * plain:                      a host functor, compiled against the headers on the include path -- the reference's with
//                                 oracle/eigen_shim as Eigen for the fixture (tests/golden/make_graph_linear_golden.py);
//   * -DGRAPH_LINEAR_PROBE_DEVICE a GraphLinearObjective<double> with the same bodies, compiled against include/ and run on
//                                 the GPU (tests/test_graph_linear_objective_gpu.py).
// The functor states the terms operation by operation as the bodies do and sums in the order of include/lbfgsx.h: a row's
// products over L lanes (L by the library's rule) and the halving; per coordinate the coordinate term, then its edges in
// ascending e, then its column's contributions in ascending CSR position; f is summed with a compensated accumulator, so its
// value does not depend on the order of the terms.
//
//     graph_linear_probe <R> <n> <max iterations recorded>
// prints, for each solver, one line per k = 1 .. max:  <solver> <k> <niter> <nfev> <f> <x[0]> .. <x[n-1]>   (%.17g),
// the state after a run with max_iterations = k (the solvers are deterministic, so run k+1 repeats run k and goes on).
#include <Eigen/Core>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <limits>
#include <vector>

#include <LBFGS.h>
#include <LBFGSB.h>

using namespace LBFGSpp;
typedef Eigen::Matrix<double, Eigen::Dynamic, 1> Vector;

static const int kPer = 5;        // entries per row
static const double kC0 = 0.5;    // the ridge weight of the hinge model
static const double kC1 = 0.75;   // the weight of the edge term
static const double kAmp = 0.3;   // amplitude of the start

static const char* const kHingeBody =
    "const T m = T(1) - p0[r] * z;\n"
    "const T h = m > T(0) ? m : T(0);\n"
    "dz = T(-2) * (p0[r] * h);\n"
    "return h * h;";
static const char* const kRidgeBody =
    "g[0] = c[0] * x[0];\n"
    "return T(0.5) * (c[0] * (x[0] * x[0]));";
static const char* const kQuarticEdge =
    "const T d = x[0] - x[1];\n"
    "const T q = c[1] * ((d * d) * d);\n"
    "g[0] = q;\n"
    "g[1] = T(0) - q;\n"
    "return T(0.25) * (q * d);";
static const char* const kSmoothEdge =
    "const T d = x[0] - x[1];\n"
    "const T q = c[1] * d;\n"
    "g[0] = q;\n"
    "g[1] = T(0) - q;\n"
    "return T(0.5) * (q * d);";
static const char* const kSquareBody =
    "const T u = z - p0[r];\n"
    "dz = u;\n"
    "return T(0.5) * (u * u);";

struct Matrix
{
    int R, n, L;
    std::vector<std::int32_t> rowptr, col;
    std::vector<double> val, y, b;
    std::vector<std::vector<int> > byCol;  // per column: CSR positions, ascending
    std::vector<std::int32_t> ei, ej;      // the graph on the columns
    std::vector<std::vector<int> > byNode; // per node: 2 e + side of its incidence entries, ascending e
    Matrix(int R_, int n_) : R(R_), n(n_), byCol(size_t(n_)), byNode(size_t(n_))
    {
        for (int t = 0; t < n; t++)
        {
            ei.push_back(t);
            ej.push_back((t + 1) % n);
            const int u = (7 * t + 3) % n;
            if (t % 3 == 0 && u != t)
            {
                ei.push_back(u);
                ej.push_back(t);
            }
        }
        for (size_t e = 0; e < ei.size(); e++)
        {
            byNode[size_t(ei[e])].push_back(int(2 * e));
            byNode[size_t(ej[e])].push_back(int(2 * e + 1));
        }
        rowptr.push_back(0);
        for (int r = 0; r < R; r++)
        {
            for (int j = 0; j < kPer; j++)
            {
                col.push_back(std::int32_t((7 * r + 3 * j * j + j) % n));
                val.push_back(double((31 * r + 17 * j) % 13 - 6) / 4.0);
            }
            rowptr.push_back(std::int32_t(col.size()));
            y.push_back((5 * r) % 3 == 0 ? -1.0 : 1.0);
            b.push_back(double((11 * r) % 7 - 3) / 2.0);
        }
        for (size_t k = 0; k < col.size(); k++)
            byCol[size_t(col[k])].push_back(int(k));
        // the library's rule: the largest power of two <= max(1, nnz / R), at most 64
        L = 1;
        while (L < 64 && 2 * L <= int(col.size()) / R)
            L *= 2;
    }
    std::int64_t nnz() const { return std::int64_t(col.size()); }
    std::int64_t E() const { return std::int64_t(ei.size()); }
    int rowOf(int k) const { return k / kPer; }
};

struct LinearModel
{
    const Matrix& M;
    const bool hinge;  // the hinge model with its ridge and the quartic coupling, or least squares with the quadratic one
    int calls = 0;
    std::vector<double> w;
    LinearModel(const Matrix& m, bool hinge_) : M(m), hinge(hinge_), w(size_t(m.R)) {}
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every term
        auto add = [&](double v) {
            const double s = hi + v;
            const double bb = s - hi;
            lo += (hi - (s - bb)) + (v - bb);
            hi = s;
        };
        std::vector<double> s(size_t(M.L));
        std::vector<char> has(size_t(M.L));
        for (int r = 0; r < M.R; r++)
        {
            for (int l = 0; l < M.L; l++)
            {
                s[size_t(l)] = 0.0;
                has[size_t(l)] = 0;
            }
            for (int k = M.rowptr[size_t(r)]; k < M.rowptr[size_t(r) + 1]; k++)
            {
                const int l = (k - M.rowptr[size_t(r)]) % M.L;
                const double prod = M.val[size_t(k)] * x[M.col[size_t(k)]];
                s[size_t(l)] = has[size_t(l)] ? s[size_t(l)] + prod : prod;
                has[size_t(l)] = 1;
            }
            for (int h = M.L / 2; h >= 1; h /= 2)
                for (int l = 0; l < h; l++)
                    s[size_t(l)] = s[size_t(l)] + s[size_t(l + h)];
            const double z = s[0];
            if (hinge)
            {
                const double m = 1.0 - M.y[size_t(r)] * z;
                const double h = m > 0.0 ? m : 0.0;
                w[size_t(r)] = -2.0 * (M.y[size_t(r)] * h);
                add(h * h);
            }
            else
            {
                const double u = z - M.b[size_t(r)];
                w[size_t(r)] = u;
                add(0.5 * (u * u));
            }
        }
        for (int j = 0; j < M.n; j++)
        {
            double g = 0.0;
            bool any = false;
            if (hinge)
            {
                g = kC0 * x[j];
                any = true;
                add(0.5 * (kC0 * (x[j] * x[j])));
            }
            for (int es : M.byNode[size_t(j)])
            {
                // the edge's term from this end, on (x[ei[e]], x[ej[e]]) as from the other end
                const int e = es >> 1;
                const double d = x[M.ei[size_t(e)]] - x[M.ej[size_t(e)]];
                const double q = hinge ? kC1 * ((d * d) * d) : kC1 * d;
                const double mine = (es & 1) ? 0.0 - q : q;
                g = any ? g + mine : mine;
                any = true;
                if (!(es & 1))
                    add(hinge ? 0.25 * (q * d) : 0.5 * (q * d));
            }
            for (int k : M.byCol[size_t(j)])
            {
                const double prod = M.val[size_t(k)] * w[size_t(M.rowOf(k))];
                g = any ? g + prod : prod;
                any = true;
            }
            grad[j] = g;
        }
        return hi + lo;
    }
};

// no two weights alike, some negative; divisions, products and sums only
static Vector start(const Matrix& M)
{
    Vector x(M.n);
    for (int i = 0; i < M.n; i++)
    {
        const double t = double(i + 1) / double(M.n + 1);
        x[i] = kAmp * ((0.5 - t) * (1.0 + t));
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

#ifdef GRAPH_LINEAR_PROBE_DEVICE
static void setup(GraphLinearObjective<double>& f, const Matrix& M, const std::vector<double>& perRow)
{
    f.matrix(M.R, M.nnz(), M.rowptr.data(), M.col.data(), M.val.data());
    f.edges(M.E(), M.ei.data(), M.ej.data());
    f.host_data(0, perRow.data(), M.R);
    f.scalars({kC0, kC1});
}
#endif

int main(int argc, char** argv)
{
    if (argc < 4)
    {
        std::fprintf(stderr, "usage: graph_linear_probe <R> <n> <iterations>\n");
        return 2;
    }
    const int R = std::atoi(argv[1]), n = std::atoi(argv[2]), kmax = std::atoi(argv[3]);
    const Matrix M(R, n);
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
#ifdef GRAPH_LINEAR_PROBE_DEVICE
            GraphLinearObjective<double> f(kHingeBody, kQuarticEdge, kRidgeBody);
            setup(f, M, M.y);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            LinearModel f(M, true);
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
            Vector x = start(M), lb = Vector::Constant(n, 0.0), ub = Vector::Constant(n, std::numeric_limits<double>::infinity());
            double fx = 0;
#ifdef GRAPH_LINEAR_PROBE_DEVICE
            GraphLinearObjective<double> f(kSquareBody, kSmoothEdge);
            setup(f, M, M.b);
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            LinearModel f(M, false);
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
    std::printf("GRAPH LINEAR PROBE OK\n");
    return 0;
}
