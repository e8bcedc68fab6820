// tests/cpp/volume_probe.cpp -- the Allen-Cahn energy on a slabs x rows x cols array
//     f(x) = sum over cells of 1/8 (the twelve squared differences along the cell's edges) + c0/4 (x0^2 - 1)^2,
// x[4*ds + 2*dr + dc] the cell's node (s+ds, r+dr, c+dc), through LBFGSSolver with the More-Thuente search and through
// LBFGSBSolver with the box [-0.5, 2], iterate by iterate.
//
// One source, two builds:
//   * plain:                a host functor, compiled against the headers on the include path -- the reference's with
//                           oracle/eigen_shim as Eigen for the fixture (tests/golden/make_volume_golden.py);
//   * -DVOLUME_PROBE_DEVICE a VolumeObjective<double> with the same cell, compiled against include/ and run on the GPU
//                           (tests/test_volume_objective_gpu.py).
// The functor states the cell operation by operation as the body does and adds the contributions to grad[s,r,c] in the order
// of include/lbfgsx.h (cells (s-1,r-1,c-1) .. (s,r,c), ascending origin); f is summed with a compensated accumulator, so its
// value does not depend on the order of the cells.
//
//     volume_probe <slabs> <rows> <cols> <max iterations recorded>
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

struct AllenCahn3
{
    int slabs, rows, cols, calls = 0;
    std::vector<double> tg[8];
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const int cw = cols - 1, rw = rows - 1, rc = rows * cols;
        for (int j = 0; j < 8; j++)
            tg[j].resize(size_t(slabs - 1) * rw * cw);
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every cell
        for (int s = 0; s + 1 < slabs; s++)
            for (int r = 0; r + 1 < rows; r++)
                for (int c = 0; c + 1 < cols; c++)
                {
                    const int i = (s * rows + r) * cols + c, t = (s * rw + r) * cw + c;
                    const double x0 = x[i], x1 = x[i + 1], x2 = x[i + cols], x3 = x[i + cols + 1];
                    const double x4 = x[i + rc], x5 = x[i + rc + 1], x6 = x[i + rc + cols], x7 = x[i + rc + cols + 1];
                    const double a0 = x1 - x0, a1 = x3 - x2, a2 = x5 - x4, a3 = x7 - x6;
                    const double b0 = x2 - x0, b1 = x3 - x1, b2 = x6 - x4, b3 = x7 - x5;
                    const double e0 = x4 - x0, e1 = x5 - x1, e2 = x6 - x2, e3 = x7 - x3;
                    const double u = x0 * x0 - 1.0;
                    const double k = kC0 * 0.25;
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
                    const double val = 0.125 * ((sa + sb) + se) + k * (u * u);
                    const double sum = hi + val;
                    const double bb = sum - hi;
                    lo += (hi - (sum - bb)) + (val - bb);
                    hi = sum;
                }
        for (int s = 0; s < slabs; s++)
            for (int r = 0; r < rows; r++)
                for (int c = 0; c < cols; c++)
                {
                    double acc = 0.0;
                    bool has = false;
                    for (int q = 0; q < 8; q++)  // cells (s-1,r-1,c-1) .. (s,r,c): the node is their corner 7 - q
                    {
                        const int cs = s - ((q & 4) ? 0 : 1), cr = r - ((q & 2) ? 0 : 1), cc = c - ((q & 1) ? 0 : 1);
                        if (cs >= 0 && cr >= 0 && cc >= 0 && cs < slabs - 1 && cr < rows - 1 && cc < cols - 1)
                        {
                            const double v = tg[7 - q][(cs * rw + cr) * cw + cc];
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
// products and sums only, so that the test's numpy restatement gives the same doubles
static Vector start(int slabs, int rows, int cols)
{
    Vector x(slabs * rows * cols);
    for (int s = 0; s < slabs; s++)
        for (int r = 0; r < rows; r++)
            for (int c = 0; c < cols; c++)
            {
                const double ts = double(s + 1) / double(slabs + 1), tr = double(r + 1) / double(rows + 1),
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

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: volume_probe <slabs> <rows> <cols> <iterations>\n");
        return 2;
    }
    const int slabs = std::atoi(argv[1]), rows = std::atoi(argv[2]), cols = std::atoi(argv[3]), kmax = std::atoi(argv[4]);
    const int n = slabs * rows * cols;
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
#ifdef VOLUME_PROBE_DEVICE
            VolumeObjective<double> f(slabs, rows, cols, kBody);
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            AllenCahn3 f{slabs, rows, cols};
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
            Vector x = start(slabs, rows, cols), lb = Vector::Constant(n, -0.5), ub = Vector::Constant(n, 2.0);
            double fx = 0;
#ifdef VOLUME_PROBE_DEVICE
            VolumeObjective<double> f(slabs, rows, cols, kBody);
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            AllenCahn3 f{slabs, rows, cols};
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
    std::printf("VOLUME PROBE OK\n");
    return 0;
}
