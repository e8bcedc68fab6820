// tests/cpp/grid_probe.cpp -- the Allen-Cahn energy on a rows x cols grid
//     f(x) = sum over cells of 1/4 ((x1-x0)^2 + (x2-x0)^2 + (x3-x2)^2 + (x3-x1)^2) + c0/4 (x0^2 - 1)^2,
// x0..x3 the cell's nodes (r,c), (r,c+1), (r+1,c), (r+1,c+1), through LBFGSSolver with the More-Thuente search and through
// LBFGSBSolver with the box [-0.5, 2], iterate by iterate.
//
// One source, two builds:
//   * plain:              a host functor, compiled against the headers on the include path -- the reference's with
//                         oracle/eigen_shim as Eigen for the fixture (tests/golden/make_grid_golden.py);
//   * -DGRID_PROBE_DEVICE a GridObjective<double> with the same cell, compiled against include/ and run on the GPU
//                         (tests/test_grid_objective_gpu.py).
// The functor states the cell operation by operation as the body does and adds the contributions to grad[r,c] in the order
// of include/lbfgsx.h (cells (r-1,c-1), (r-1,c), (r,c-1), (r,c)); f is summed with a compensated accumulator, so its value
// does not depend on the order of the cells.
//
//     grid_probe <rows> <cols> <max iterations recorded>
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

static const double kC0 = 1.0;

static const char* const kBody =
    "const T a = x[1] - x[0];\n"
    "const T b = x[2] - x[0];\n"
    "const T e = x[3] - x[2];\n"
    "const T h = x[3] - x[1];\n"
    "const T u = x[0] * x[0] - T(1);\n"
    "const T k = c[0] * T(0.25);\n"
    "g[0] = T(-0.5) * (a + b) + (T(4) * k) * (u * x[0]);\n"
    "g[1] = T(0.5) * (a - h);\n"
    "g[2] = T(0.5) * (b - e);\n"
    "g[3] = T(0.5) * (e + h);\n"
    "return T(0.25) * ((a * a + b * b) + (e * e + h * h)) + k * (u * u);";

struct AllenCahn
{
    int rows, cols, calls = 0;
    std::vector<double> tg[4];
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const int cw = cols - 1;
        for (int j = 0; j < 4; j++)
            tg[j].resize(size_t(rows - 1) * cw);
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every cell
        for (int r = 0; r + 1 < rows; r++)
            for (int c = 0; c + 1 < cols; c++)
            {
                const int i = r * cols + c;
                const double x0 = x[i], x1 = x[i + 1], x2 = x[i + cols], x3 = x[i + cols + 1];
                const double a = x1 - x0;
                const double b = x2 - x0;
                const double e = x3 - x2;
                const double h = x3 - x1;
                const double u = x0 * x0 - 1.0;
                const double k = kC0 * 0.25;
                tg[0][r * cw + c] = -0.5 * (a + b) + (4.0 * k) * (u * x0);
                tg[1][r * cw + c] = 0.5 * (a - h);
                tg[2][r * cw + c] = 0.5 * (b - e);
                tg[3][r * cw + c] = 0.5 * (e + h);
                const double val = 0.25 * ((a * a + b * b) + (e * e + h * h)) + k * (u * u);
                const double s = hi + val;
                const double bb = s - hi;
                lo += (hi - (s - bb)) + (val - bb);
                hi = s;
            }
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                double acc = 0.0;
                bool has = false;
                for (int q = 0; q < 4; q++)  // cells (r-1,c-1), (r-1,c), (r,c-1), (r,c): the node is their corner 3 - q
                {
                    const int cr = r - (q < 2 ? 1 : 0), cc = c - ((q & 1) ? 0 : 1);
                    if (cr >= 0 && cc >= 0 && cr < rows - 1 && cc < cols - 1)
                    {
                        const double v = tg[3 - q][cr * cw + cc];
                        acc = has ? acc + v : v;
                        has = true;
                    }
                }
                grad[r * cols + c] = acc;
            }
        return hi + lo;
    }
};

// a smooth bump scaled into the box, no two nodes alike (equal break points of the Cauchy search would be ties); divisions,
// products and sums only, so that the test's numpy restatement gives the same doubles
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

int main(int argc, char** argv)
{
    if (argc < 4)
    {
        std::fprintf(stderr, "usage: grid_probe <rows> <cols> <iterations>\n");
        return 2;
    }
    const int rows = std::atoi(argv[1]), cols = std::atoi(argv[2]), kmax = std::atoi(argv[3]);
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
#ifdef GRID_PROBE_DEVICE
            GridObjective<double> f(rows, cols, kBody);
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            AllenCahn f{rows, cols};
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
            Vector x = start(rows, cols), lb = Vector::Constant(n, -0.5), ub = Vector::Constant(n, 2.0);
            double fx = 0;
#ifdef GRID_PROBE_DEVICE
            GridObjective<double> f(rows, cols, kBody);
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            AllenCahn f{rows, cols};
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
    std::printf("GRID PROBE OK\n");
    return 0;
}
