// tests/cpp/field_probe.cpp -- the Ginzburg-Landau energy of a field of D unknowns per node on a rows x cols grid, open or
// periodic in the directions of a mask (bit 0 columns, bit 1 rows), x node-major: x[(r*cols + c)*D + d]
//     f(x) = sum over the cells that exist of 1/4 sum_d ((a^2 + b^2) + (e^2 + h^2)) + c0/4 (sum_d x0_d^2 - 1)^2,
// a, b, e, h the differences x1-x0, x2-x0, x3-x2, x3-x1 of component d along the cell's edges, a cell's corners taken modulo the
// extents, through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with the box [-0.25, 0.6], iterate by
// iterate.
//
// One source, two builds:
//   * plain:                host functor, compiled against the headers on the include path -- the reference's with
//                           oracle/eigen_shim as Eigen for the fixture (tests/golden/make_field_golden.py);
//   * -DFIELD_PROBE_DEVICE  a GridFieldObjective<double> with the same cell, compiled against include/ and run on the GPU
//                           (tests/test_field_objective_gpu.py).
// The functor states the cell operation by operation as the body does and adds the contributions to a node's gradient in the
// order of include/lbfgsx.h (the cells at node - (1,1) .. node, wrapped, those that exist); f is summed with a compensated
// accumulator, so its value does not depend on the order of the cells.
//
//     field_probe <rows> <cols> <D> <mask> <max iterations recorded>
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
    "T ss = T(0);\n"
    "#pragma unroll\n"
    "for (int d = 0; d < D; d++)\n"
    "    ss = ss + x[d] * x[d];\n"
    "const T u = ss - T(1);\n"
    "const T k = c[0] * T(0.25);\n"
    "T v = T(0);\n"
    "#pragma unroll\n"
    "for (int d = 0; d < D; d++)\n"
    "{\n"
    "    const T a = x[D + d] - x[d];\n"
    "    const T b = x[2 * D + d] - x[d];\n"
    "    const T e = x[3 * D + d] - x[2 * D + d];\n"
    "    const T h = x[3 * D + d] - x[D + d];\n"
    "    g[d] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[d]);\n"
    "    g[D + d] = T(0.5) * (a - h);\n"
    "    g[2 * D + d] = T(0.5) * (b - e);\n"
    "    g[3 * D + d] = T(0.5) * (e + h);\n"
    "    v = v + ((a * a + b * b) + (e * e + h * h));\n"
    "}\n"
    "return T(0.25) * v + k * (u * u);";

struct GinzburgLandau
{
    int rows, cols, D, mask, calls = 0;
    std::vector<double> tg;  // [cell][4*D]
    std::vector<char> ex;
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const int N = rows * cols;
        const bool pc = (mask & 1) != 0, pr = (mask & 2) != 0;
        tg.assign(size_t(N) * 4 * D, 0.0);
        ex.assign(size_t(N), 0);
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every cell
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                if (!((c + 1 < cols || pc) && (r + 1 < rows || pr)))
                    continue;
                const int t = r * cols + c, r1 = (r + 1) % rows, c1 = (c + 1) % cols;
                const int j[4] = {t, r * cols + c1, r1 * cols + c, r1 * cols + c1};
                ex[t] = 1;
                double* g = &tg[size_t(t) * 4 * D];
                double ss = 0.0;
                for (int d = 0; d < D; d++)
                    ss = ss + x[j[0] * D + d] * x[j[0] * D + d];
                const double u = ss - 1.0;
                const double k = kC0 * 0.25;
                double v = 0.0;
                for (int d = 0; d < D; d++)
                {
                    const double x0 = x[j[0] * D + d], x1 = x[j[1] * D + d], x2 = x[j[2] * D + d], x3 = x[j[3] * D + d];
                    const double a = x1 - x0, b = x2 - x0, e = x3 - x2, h = x3 - x1;
                    g[d] = -0.5 * (a + b) + (4.0 * k) * (u * x0);
                    g[D + d] = 0.5 * (a - h);
                    g[2 * D + d] = 0.5 * (b - e);
                    g[3 * D + d] = 0.5 * (e + h);
                    v = v + ((a * a + b * b) + (e * e + h * h));
                }
                const double val = 0.25 * v + k * (u * u);
                const double sum = hi + val;
                const double bb = sum - hi;
                lo += (hi - (sum - bb)) + (val - bb);
                hi = sum;
            }
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
                for (int d = 0; d < D; d++)
                {
                    double acc = 0.0;
                    bool has = false;
                    for (int q = 0; q < 4; q++)  // the cells at node - (1,1) .. node: the node is their corner 3 - q
                    {
                        int cr = r - ((q & 2) ? 0 : 1), cc = c - ((q & 1) ? 0 : 1);
                        if ((cr < 0 && !pr) || (cc < 0 && !pc))
                            continue;
                        cr = (cr + rows) % rows;
                        cc = (cc + cols) % cols;
                        const int t = cr * cols + cc;
                        if (ex[t])
                        {
                            const double v = tg[size_t(t) * 4 * D + (3 - q) * D + d];
                            acc = has ? acc + v : v;
                            has = true;
                        }
                    }
                    grad[(r * cols + c) * D + d] = acc;
                }
        return hi + lo;
    }
};

// a smooth bump per component, no two coordinates alike (equal break points of the Cauchy search would be ties); divisions,
// products and sums only, so that the test's numpy restatement gives the same doubles
static Vector start(int rows, int cols, int D)
{
    Vector x(rows * cols * D);
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++)
            for (int d = 0; d < D; d++)
            {
                const double tr = double(r + 1) / double(rows + 1), tc = double(c + 1) / double(cols + 1),
                             td = double(d + 1) / double(D + 1);
                const double bump = (tr * (1.0 - tr)) * (tc * (1.0 - tc));
                x[(r * cols + c) * D + d] = -0.3 + ((16.0 * bump) * (((1.0 + 0.5 * tr) + 0.25 * tc) + 0.125 * td)) * (1.0 - 0.5 * td);
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
static int run(Solver& solver, int rows, int cols, int D, int mask, Vector& x, double& fx, int& nfev, Bounds&... bounds)
{
#ifdef FIELD_PROBE_DEVICE
    nfev = -1;
    GridFieldObjective<double> f(rows, cols, D, mask, kBody);
    f.scalars({kC0});
    return solver.minimize(f, x, fx, bounds...);
#else
    (void) kBody;
    GinzburgLandau f{rows, cols, D, mask};
    const int niter = solver.minimize(f, x, fx, bounds...);
    nfev = f.calls;
    return niter;
#endif
}

int main(int argc, char** argv)
{
    if (argc < 6)
    {
        std::fprintf(stderr, "usage: field_probe <rows> <cols> <D> <mask> <iterations>\n");
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), D = std::atoi(argv[3]), mask = std::atoi(argv[4]),
              kmax = std::atoi(argv[5]);
    const int n = rows * cols * D;
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
            Vector x = start(rows, cols, D);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, rows, cols, D, mask, x, fx, nfev);
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
            Vector x = start(rows, cols, D), lb = Vector::Constant(n, kLo), ub = Vector::Constant(n, kHi);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, rows, cols, D, mask, x, fx, nfev, lb, ub);
            emit("lbfgsb", k, niter, nfev, fx, x);
        }
    }
    catch (const std::exception& e)
    {
        std::printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    std::printf("FIELD PROBE OK\n");
    return 0;
}
