// tests/cpp/stencil_probe.cpp -- a Swift-Hohenberg / plate energy on a rows x cols grid, open or periodic in the directions of a
// mask (bit 0 columns, bit 1 rows), one term per 3x3 patch of nodes:
//     f(x) = sum over the patches that exist of 1/2 (x1 + x3 + x5 + x7 - 4 x4)^2 + c0/4 (x4^2 - 1)^2,
// x[3*dr + dc] the node (r+dr, c+dc) of the patch with origin (r, c), taken modulo the extents (x4 is the patch's centre),
// through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with the box [-0.25, 0.6], iterate by iterate.
//
// One source, two builds:
//   * plain:                  host functor, compiled against the headers on the include path -- the reference's with
//                             oracle/eigen_shim as Eigen for the fixture (tests/golden/make_stencil_golden.py);
//   * -DSTENCIL_PROBE_DEVICE  a StencilObjective<double> with the same patch, compiled against include/ and run on the GPU
//                             (tests/test_stencil_objective_gpu.py).
// The functor states the patch operation by operation as the body does and adds the contributions to a node's gradient in the
// order of include/lbfgsx.h (the patches at node - (dr, dc), dr = 2, 1, 0 outer and dc = 2, 1, 0 inner, wrapped, those that
// exist); f is summed with a compensated accumulator, so its value does not depend on the order of the patches.
//
//     stencil_probe <rows> <cols> <mask> <max iterations recorded>
// prints, for each solver, one line per k = 1 .. max:  <solver> <k> <niter> <nfev> <f> <x[0]> .. <x[n-1]>   (%.17g),
// the state after a run with max_iterations = k (the solvers are deterministic, so run k+1 repeats run k and goes on).
#include <Eigen/Core>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include <LBFGS.h>
#include <LBFGSB.h>

using namespace LBFGSpp;
typedef Eigen::Matrix<double, Eigen::Dynamic, 1> Vector;

static const double kC0 = 1.0, kLo = -0.25, kHi = 0.6;

static const char* const kBody =
    "const T l = (((x[1] + x[3]) + x[5]) + x[7]) - T(4) * x[4];\n"
    "const T u = x[4] * x[4] - T(1);\n"
    "const T kw = c[0] * T(0.25);\n"
    "g[0] = T(0);\n"
    "g[2] = T(0);\n"
    "g[6] = T(0);\n"
    "g[8] = T(0);\n"
    "g[1] = l;\n"
    "g[3] = l;\n"
    "g[5] = l;\n"
    "g[7] = l;\n"
    "g[4] = T(-4) * l + (T(4) * kw) * (u * x[4]);\n"
    "return T(0.5) * (l * l) + kw * (u * u);";

struct Plate
{
    int rows, cols, mask, calls = 0;
    std::vector<double> tg;  // [patch][9]
    std::vector<char> ex;
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const int N = rows * cols;
        const bool pc = (mask & 1) != 0, pr = (mask & 2) != 0;
        tg.assign(size_t(N) * 9, 0.0);
        ex.assign(size_t(N), 0);
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every patch
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                if (!((c + 2 < cols || pc) && (r + 2 < rows || pr)))
                    continue;
                const int t = r * cols + c;
                double xs[9];
                for (int dr = 0; dr < 3; dr++)
                    for (int dc = 0; dc < 3; dc++)
                        xs[3 * dr + dc] = x[((r + dr) % rows) * cols + (c + dc) % cols];
                ex[t] = 1;
                double* g = &tg[size_t(t) * 9];
                const double l = (((xs[1] + xs[3]) + xs[5]) + xs[7]) - 4.0 * xs[4];
                const double u = xs[4] * xs[4] - 1.0;
                const double kw = kC0 * 0.25;
                g[0] = g[2] = g[6] = g[8] = 0.0;
                g[1] = g[3] = g[5] = g[7] = l;
                g[4] = -4.0 * l + (4.0 * kw) * (u * xs[4]);
                const double val = 0.5 * (l * l) + kw * (u * u);
                const double sum = hi + val;
                const double bb = sum - hi;
                lo += (hi - (sum - bb)) + (val - bb);
                hi = sum;
            }
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                double acc = 0.0;
                bool has = false;
                for (int dr = 2; dr >= 0; dr--)
                    for (int dc = 2; dc >= 0; dc--)  // the patch at node - (dr, dc): the node is its slot 3*dr + dc
                    {
                        int pr0 = r - dr, pc0 = c - dc;
                        if ((pr0 < 0 && !pr) || (pc0 < 0 && !pc))
                            continue;
                        pr0 = (pr0 + rows) % rows;
                        pc0 = (pc0 + cols) % cols;
                        const int t = pr0 * cols + pc0;
                        if (ex[t])
                        {
                            const double v = tg[size_t(t) * 9 + 3 * dr + dc];
                            acc = has ? acc + v : v;
                            has = true;
                        }
                    }
                grad[r * cols + c] = acc;
            }
        return hi + lo;
    }
};

// a smooth bump, no two coordinates alike (equal break points of the Cauchy search would be ties); divisions, products and
// sums only, so that the test's numpy restatement gives the same doubles
static Vector start(int rows, int cols)
{
    Vector x(rows * cols);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++)
        {
            const double tr = double(r + 1) / double(rows + 1), tc = double(c + 1) / double(cols + 1);
            const double bump = (tr * (1.0 - tr)) * (tc * (1.0 - tc));
            x[r * cols + c] = -0.3 + (16.0 * bump) * ((1.0 + 0.5 * tr) + 0.25 * tc);
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

template <class Solver, class... Bounds>
static int run(Solver& solver, int rows, int cols, int mask, Vector& x, double& fx, int& nfev, Bounds&... bounds)
{
#ifdef STENCIL_PROBE_DEVICE
    nfev = -1;
    StencilObjective<double> f(rows, cols, mask, kBody);
    f.scalars({kC0});
    return solver.minimize(f, x, fx, bounds...);
#else
    (void) kBody;
    Plate f{rows, cols, mask};
    const int niter = solver.minimize(f, x, fx, bounds...);
    nfev = f.calls;
    return niter;
#endif
}

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: stencil_probe <rows> <cols> <mask> <iterations>\n");
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), mask = std::atoi(argv[3]), kmax = std::atoi(argv[4]);
    const int n = rows * cols;
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
            Vector x = start(rows, cols);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, rows, cols, mask, x, fx, nfev);
            emit("lbfgs", k, niter, nfev, fx, x);
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
            Vector x = start(rows, cols), lb = Vector::Constant(n, kLo), ub = Vector::Constant(n, kHi);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, rows, cols, mask, x, fx, nfev, lb, ub);
            emit("lbfgsb", k, niter, nfev, fx, x);
        }
    }
    catch (const std::exception& e)
    {
        std::printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    std::printf("STENCIL PROBE OK\n");
    return 0;
}
