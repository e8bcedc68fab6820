// tests/cpp/graph_probe.cpp -- a double-well energy on a ring with chords
//     f(x) = sum over nodes of c0/4 (x^2 - 1)^2  +  sum over edges e = (i, j) of 1/2 (w_e (x_i - x_j)) (x_i - x_j),
// w_e = 1 + 0.25 (e mod 5), through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with the box
// [-0.6, 0.8], iterate by iterate.  The edges, generated for t = 0 .. n-1 in this order: (t, (t+1) mod n), then, when
// t mod 3 = 0 and u = (7t + 3) mod n differs from t, the chord (u, t).
//
// One source, two builds:
//   * plain:               a host functor, compiled against the headers on the include path -- the reference's with
//                          oracle/eigen_shim as Eigen for the fixture (tests/golden/make_graph_golden.py);
//   * -DGRAPH_PROBE_DEVICE a GraphObjective<double> with the same two terms, compiled against include/ and run on the GPU
//                          (tests/test_graph_objective_gpu.py).
// The functor states both terms operation by operation as the bodies do and adds the contributions to grad[v] in the order
// of include/lbfgsx.h (the node term, then the incident edges in ascending e); f is summed with a compensated accumulator,
// so its value does not depend on the order of the terms.
//
//     graph_probe <n> <max iterations recorded>
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

static const double kC0 = 1.0;

static const char* const kEdgeBody =
    "const T d = x[0] - x[1];\n"
    "const T w = p0[e] * d;\n"
    "g[0] = w;\n"
    "g[1] = T(0) - w;\n"
    "return T(0.5) * (w * d);";
static const char* const kNodeBody =
    "const T u = x[0] * x[0] - T(1);\n"
    "const T k = c[0] * T(0.25);\n"
    "g[0] = (T(4) * k) * (u * x[0]);\n"
    "return k * (u * u);";

struct Graph
{
    int n;
    std::vector<std::int32_t> ei, ej;
    std::vector<double> w;
    explicit Graph(int n_) : n(n_)
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
            w.push_back(1.0 + 0.25 * double(e % 5));
    }
};

struct DoubleWell
{
    const Graph& G;
    int calls = 0;
    std::vector<std::vector<std::pair<int, int> > > inc;  // per node: (e, side), ascending e
    std::vector<double> tg[2];
    explicit DoubleWell(const Graph& g) : G(g), inc(size_t(g.n))
    {
        for (size_t e = 0; e < G.ei.size(); e++)
        {
            inc[size_t(G.ei[e])].push_back(std::make_pair(int(e), 0));
            inc[size_t(G.ej[e])].push_back(std::make_pair(int(e), 1));
        }
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
        tg[0].resize(G.ei.size());
        tg[1].resize(G.ei.size());
        for (size_t e = 0; e < G.ei.size(); e++)
        {
            const double d = x[G.ei[e]] - x[G.ej[e]];
            const double w = G.w[e] * d;
            tg[0][e] = w;
            tg[1][e] = 0.0 - w;
            add(0.5 * (w * d));
        }
        for (int v = 0; v < G.n; v++)
        {
            const double u = x[v] * x[v] - 1.0;
            const double k = kC0 * 0.25;
            double acc = (4.0 * k) * (u * x[v]);
            add(k * (u * u));
            for (const std::pair<int, int>& en : inc[size_t(v)])
                acc = acc + tg[en.second][size_t(en.first)];
            grad[v] = acc;
        }
        return hi + lo;
    }
};

// a smooth odd-ish profile scaled into the box, no two nodes alike (equal break points of the Cauchy search would be ties);
// divisions, products and sums only, so that the test's numpy restatement gives the same doubles
static Vector start(int n)
{
    Vector x(n);
    for (int v = 0; v < n; v++)
    {
        const double t = double(v + 1) / double(n + 1);
        x[v] = -0.1 + (12.0 * ((t * (1.0 - t)) * (0.5 - t))) * (1.0 + 0.5 * t);
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

int main(int argc, char** argv)
{
    if (argc < 3)
    {
        std::fprintf(stderr, "usage: graph_probe <n> <iterations>\n");
        return 2;
    }
    const int n = std::atoi(argv[1]), kmax = std::atoi(argv[2]);
    const Graph G(n);
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
            Vector x = start(n);
            double fx = 0;
#ifdef GRAPH_PROBE_DEVICE
            GraphObjective<double> f(kEdgeBody, kNodeBody);
            f.edges(std::int64_t(G.ei.size()), G.ei.data(), G.ej.data());
            f.host_data(0, G.w.data(), std::int64_t(G.w.size()));
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            DoubleWell f(G);
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
            Vector x = start(n), lb = Vector::Constant(n, -0.6), ub = Vector::Constant(n, 0.8);
            double fx = 0;
#ifdef GRAPH_PROBE_DEVICE
            GraphObjective<double> f(kEdgeBody, kNodeBody);
            f.edges(std::int64_t(G.ei.size()), G.ei.data(), G.ej.data());
            f.host_data(0, G.w.data(), std::int64_t(G.w.size()));
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            DoubleWell f(G);
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
    std::printf("GRAPH PROBE OK\n");
    return 0;
}
