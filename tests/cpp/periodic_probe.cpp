// tests/cpp/periodic_probe.cpp -- the Allen-Cahn energy on a rows x cols grid or a slabs x rows x cols array with periodic
// boundaries in the directions of a mask (bit 0 columns, bit 1 rows, bit 2 slabs)
//     grid:    f(x) = sum over the cells that exist of 1/4 (the four squared differences along the cell's edges) + c0/4 (x0^2 - 1)^2
//     volume:  f(x) = sum over the cells that exist of 1/8 (the twelve squared differences) + c0/4 (x0^2 - 1)^2,
// a cell's corners taken modulo the extents, through LBFGSSolver with the More-Thuente search and through LBFGSBSolver with the
// box [-0.5, 2], iterate by iterate.
//
// One source, two builds:
//   * plain:                  host functors, compiled against the headers on the include path -- the reference's with
//                             oracle/eigen_shim as Eigen for the fixture (tests/golden/make_periodic_golden.py);
//   * -DPERIODIC_PROBE_DEVICE a PeriodicGridObjective<double> or PeriodicVolumeObjective<double> with the same cell, compiled
//                             against include/ and run on the GPU (tests/test_periodic_objective_gpu.py).
// The functors state the cell operation by operation as the bodies do and add the contributions to a node's gradient in the
// order of include/lbfgsx.h (the cells at node - (1,1,1) .. node, wrapped, those that exist); f is summed with a compensated
// accumulator, so its value does not depend on the order of the cells.
//
//     periodic_probe <slabs, 0 for a grid> <rows> <cols> <mask> <max iterations recorded>
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

static const char* const kBody2 =
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

static const char* const kBody3 =
    "const T a0 = x[1] - x[0], a1 = x[3] - x[2], a2 = x[5] - x[4], a3 = x[7] - x[6];\n"
    "const T b0 = x[2] - x[0], b1 = x[3] - x[1], b2 = x[6] - x[4], b3 = x[7] - x[5];\n"
    "const T e0 = x[4] - x[0], e1 = x[5] - x[1], e2 = x[6] - x[2], e3 = x[7] - x[3];\n"
    "const T u = x[0] * x[0] - T(1);\n"
    "const T k = c[0] * T(0.25);\n"
    "g[0] = T(-0.25) * ((a0 + b0) + e0) + (T(4) * k) * (u * x[0]);\n"
    "g[1] = T(0.25) * ((a0 - b1) - e1);\n"
    "g[2] = T(0.25) * ((b0 - a1) - e2);\n"
    "g[3] = T(0.25) * ((a1 + b1) - e3);\n"
    "g[4] = T(0.25) * ((e0 - a2) - b2);\n"
    "g[5] = T(0.25) * ((a2 + e1) - b3);\n"
    "g[6] = T(0.25) * ((b2 + e2) - a3);\n"
    "g[7] = T(0.25) * ((a3 + b3) + e3);\n"
    "const T sa = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);\n"
    "const T sb = (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);\n"
    "const T se = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);\n"
    "return T(0.125) * ((sa + sb) + se) + k * (u * u);";

// the Allen-Cahn energy of both forms: a grid is run as one slab whose slab direction holds no second layer (K = 4 corners)
struct AllenCahnPeriodic
{
    int slabs, rows, cols, mask, calls = 0;  // slabs = 0: a grid
    std::vector<double> tg[8];
    std::vector<char> ex;
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const bool grid = slabs == 0;
        const int S = grid ? 1 : slabs, K = grid ? 4 : 8, n = S * rows * cols;
        const bool pc = (mask & 1) != 0, pr = (mask & 2) != 0, ps = (mask & 4) != 0;
        for (int j = 0; j < K; j++)
            tg[j].assign(size_t(n), 0.0);
        ex.assign(size_t(n), 0);
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every cell
        for (int s = 0; s < S; s++)
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++)
                {
                    if (!((c + 1 < cols || pc) && (r + 1 < rows || pr) && (grid || s + 1 < slabs || ps)))
                        continue;
                    const int t = (s * rows + r) * cols + c;
                    const int s1 = (s + 1) % S, r1 = (r + 1) % rows, c1 = (c + 1) % cols;
                    ex[t] = 1;
                    const double x0 = x[(s * rows + r) * cols + c], x1 = x[(s * rows + r) * cols + c1];
                    const double x2 = x[(s * rows + r1) * cols + c], x3 = x[(s * rows + r1) * cols + c1];
                    const double k = kC0 * 0.25;
                    const double u = x0 * x0 - 1.0;
                    double val;
                    if (grid)
                    {
                        const double a = x1 - x0, b = x2 - x0, e = x3 - x2, h = x3 - x1;
                        tg[0][t] = -0.5 * (a + b) + (4.0 * k) * (u * x0);
                        tg[1][t] = 0.5 * (a - h);
                        tg[2][t] = 0.5 * (b - e);
                        tg[3][t] = 0.5 * (e + h);
                        val = 0.25 * ((a * a + b * b) + (e * e + h * h)) + k * (u * u);
                    }
                    else
                    {
                        const double x4 = x[(s1 * rows + r) * cols + c], x5 = x[(s1 * rows + r) * cols + c1];
                        const double x6 = x[(s1 * rows + r1) * cols + c], x7 = x[(s1 * rows + r1) * cols + c1];
                        const double a0 = x1 - x0, a1 = x3 - x2, a2 = x5 - x4, a3 = x7 - x6;
                        const double b0 = x2 - x0, b1 = x3 - x1, b2 = x6 - x4, b3 = x7 - x5;
                        const double e0 = x4 - x0, e1 = x5 - x1, e2 = x6 - x2, e3 = x7 - x3;
                        tg[0][t] = -0.25 * ((a0 + b0) + e0) + (4.0 * k) * (u * x0);
                        tg[1][t] = 0.25 * ((a0 - b1) - e1);
                        tg[2][t] = 0.25 * ((b0 - a1) - e2);
                        tg[3][t] = 0.25 * ((a1 + b1) - e3);
                        tg[4][t] = 0.25 * ((e0 - a2) - b2);
                        tg[5][t] = 0.25 * ((a2 + e1) - b3);
                        tg[6][t] = 0.25 * ((b2 + e2) - a3);
                        tg[7][t] = 0.25 * ((a3 + b3) + e3);
                        const double sa = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                        const double sb = (b0 * b0 + b1 * b1) + (b2 * b2 + b3 * b3);
                        const double se = (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
                        val = 0.125 * ((sa + sb) + se) + k * (u * u);
                    }
                    const double sum = hi + val;
                    const double bb = sum - hi;
                    lo += (hi - (sum - bb)) + (val - bb);
                    hi = sum;
                }
        for (int s = 0; s < S; s++)
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++)
                {
                    double acc = 0.0;
                    bool has = false;
                    for (int q = 0; q < K; q++)  // the cells at node - (1,1,1) .. node: the node is their corner K-1 - q
                    {
                        int cs = s - ((grid || (q & 4)) ? 0 : 1), cr = r - ((q & 2) ? 0 : 1), cc = c - ((q & 1) ? 0 : 1);
                        if ((cs < 0 && !ps) || (cr < 0 && !pr) || (cc < 0 && !pc))
                            continue;
                        cs = (cs + S) % S;
                        cr = (cr + rows) % rows;
                        cc = (cc + cols) % cols;
                        const int t = (cs * rows + cr) * cols + cc;
                        if (ex[t])
                        {
                            const double v = tg[K - 1 - q][t];
                            acc = has ? acc + v : v;
                            has = true;
                        }
                    }
                    grad[(s * rows + r) * cols + c] = acc;
                }
        return hi + lo;
    }
};

// a smooth bump scaled into the box, no two nodes alike (equal break points of the Cauchy search would be ties); divisions,
// products and sums only, so that the test's numpy restatement gives the same doubles.  A grid is the single slab of a
// one-slab array: ts = 1/2
static Vector start(int slabs, int rows, int cols)
{
    const int S = slabs ? slabs : 1;
    Vector x(S * rows * cols);
    for (int s = 0; s < S; s++)
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                const double ts = double(s + 1) / double(S + 1), tr = double(r + 1) / double(rows + 1),
                             tc = double(c + 1) / double(cols + 1);
                const double bump = ((ts * (1.0 - ts)) * (tr * (1.0 - tr))) * (tc * (1.0 - tc));
                x[(s * rows + r) * cols + c] = -0.3 + (64.0 * bump) * (((1.0 + 0.5 * tr) + 0.25 * tc) + 0.125 * ts);
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
static int run(Solver& solver, int slabs, int rows, int cols, int mask, Vector& x, double& fx, int& nfev, Bounds&... bounds)
{
#ifdef PERIODIC_PROBE_DEVICE
    nfev = -1;
    if (slabs == 0)
    {
        PeriodicGridObjective<double> f(rows, cols, mask, kBody2);
        f.scalars({kC0});
        return solver.minimize(f, x, fx, bounds...);
    }
    PeriodicVolumeObjective<double> f(slabs, rows, cols, mask, kBody3);
    f.scalars({kC0});
    return solver.minimize(f, x, fx, bounds...);
#else
    (void) kBody2;
    (void) kBody3;
    AllenCahnPeriodic f{slabs, rows, cols, mask};
    const int niter = solver.minimize(f, x, fx, bounds...);
    nfev = f.calls;
    return niter;
#endif
}

int main(int argc, char** argv)
{
    if (argc < 6)
    {
        std::fprintf(stderr, "usage: periodic_probe <slabs, 0 for a grid> <rows> <cols> <mask> <iterations>\n");
        return 2;
    }
    const int slabs = std::atoi(argv[1]), rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), mask = std::atoi(argv[4]),
              kmax = std::atoi(argv[5]);
    const int n = (slabs ? slabs : 1) * rows * cols;
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
            Vector x = start(slabs, rows, cols);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, slabs, rows, cols, mask, x, fx, nfev);
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
            Vector x = start(slabs, rows, cols), lb = Vector::Constant(n, -0.5), ub = Vector::Constant(n, 2.0);
            double fx = 0;
            int nfev = 0;
            const int niter = run(solver, slabs, rows, cols, mask, x, fx, nfev, lb, ub);
            emit("lbfgsb", k, niter, nfev, fx, x);
        }
    }
    catch (const std::exception& e)
    {
        std::printf("EXCEPTION %s\n", e.what());
        return 1;
    }
    std::printf("PERIODIC PROBE OK\n");
    return 0;
}
