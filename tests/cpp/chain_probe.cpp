// tests/cpp/chain_probe.cpp -- the chained Rosenbrock function
//     f(x) = sum over t = 0 .. n-2 of 100 (x[t+1] - x[t]^2)^2 + (1 - x[t])^2
// through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with the box [-0.5, 2], iterate by iterate.
//
// One source, two builds:
//   * plain:               a host functor, compiled against the headers on the include path -- the reference's with
//                          oracle/eigen_shim as Eigen for the fixture (tests/golden/make_chain_golden.py);
//   * -DCHAIN_PROBE_DEVICE a ChainObjective<double> with the same term, compiled against include/ and run on the GPU
//                          (tests/test_chain_objective_gpu.py).
// The functor states the term operation by operation as the body does and adds the contributions to grad[j] in ascending t;
// f is summed with a compensated accumulator, so its value does not depend on the order of the terms.
//
//     chain_probe <n> <max iterations recorded>
// prints, for each solver, one line per k = 1 .. max:  <solver> <k> <niter> <nfev> <f> <x[0]> .. <x[n-1]>   (%.17g),
// the state after a run with max_iterations = k (the solvers are deterministic, so run k+1 repeats run k and goes on).
#include <Eigen/Core>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>

#include <LBFGS.h>
#include <LBFGSB.h>

using namespace LBFGSpp;
typedef Eigen::Matrix<double, Eigen::Dynamic, 1> Vector;

static const char* const kBody =
    "const T u = x[1] - x[0] * x[0];\n"
    "const T v = T(1) - x[0];\n"
    "g[1] = T(200) * u;\n"
    "g[0] = T(-400) * (u * x[0]) - T(2) * v;\n"
    "return T(100) * (u * u) + v * v;";

struct ChainedRosenbrock
{
    int n, calls = 0;
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every term
        double from_prev = 0.0;     // g[1] of the term that starts one coordinate earlier
        for (int t = 0; t < n; t++)
        {
            if (t + 1 < n)
            {
                const double u = x[t + 1] - x[t] * x[t];
                const double v = 1.0 - x[t];
                const double g1 = 200.0 * u;
                const double g0 = -400.0 * (u * x[t]) - 2.0 * v;
                const double val = 100.0 * (u * u) + v * v;
                grad[t] = (t > 0) ? from_prev + g0 : g0;
                from_prev = g1;
                const double s = hi + val;
                const double bb = s - hi;
                lo += (hi - (s - bb)) + (val - bb);
                hi = s;
            }
            else
                grad[t] = from_prev;
        }
        return hi + lo;
    }
};

static Vector start(int n)
{
    Vector x(n);
    for (int i = 0; i < n; i++)
    {
        // in [-0.4, 0), no two alike (equal break points of the Cauchy search would be ties); f stays small enough for an
        // absolute tolerance on it
        const double t = double(i) * 0.61803398874989485;
        x[i] = -0.4 + 0.4 * (t - std::floor(t));
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
        std::fprintf(stderr, "usage: chain_probe <n> <iterations>\n");
        return 2;
    }
    const int n = std::atoi(argv[1]), kmax = std::atoi(argv[2]);
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
#ifdef CHAIN_PROBE_DEVICE
            ChainObjective<double> f(2, kBody);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            ChainedRosenbrock f{n};
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
            Vector x = start(n), lb = Vector::Constant(n, -0.5), ub = Vector::Constant(n, 2.0);
            double fx = 0;
#ifdef CHAIN_PROBE_DEVICE
            ChainObjective<double> f(2, kBody);
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            ChainedRosenbrock f{n};
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
    std::printf("CHAIN PROBE OK\n");
    return 0;
}
