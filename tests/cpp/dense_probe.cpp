// tests/cpp/dense_probe.cpp -- two linear models over one DENSE R x F matrix A, Z = A X, x the F x D matrix X feature-major
// (x[j*D + c], n = F*D):
//     logistic regression + ridge, D = 1   f(x) = sum over rows r of log(1 + exp(-y_r Z[r,0])) + sum over i of c0/2 x_i^2
//                                          through LBFGSSolver with the More-Thuente search,
//     multi-target non-negative least squares, D = 3   f(x) = sum over rows r of 1/2 sum_c (Z[r,c] - b[r,c])^2,  0 <= x
//                                          through LBFGSBSolver from a start with negative entries (bounds active at the start),
// iterate by iterate.  Every entry of the matrix is stored: A[r,j] = (((31 r + 17 j + 3 r j) mod 13) - 6) / 4;
// y_r = -1 if 5 r mod 3 == 0 else 1; b[r,c] = (((11 r + 5 c) mod 7) - 3) / 2.  Integers and exact quotients only, so that the
// test's numpy restatement gives the same doubles.
//
// One source, two builds:
//   * plain:                a host functor, compiled against the headers on the include path -- the reference's with
//                           oracle/eigen_shim as Eigen for the fixture (tests/golden/make_dense_golden.py);
//   * -DDENSE_PROBE_DEVICE  a DenseLinearObjective<double> with the same bodies, compiled against include/ and run on the GPU
//                           (tests/test_dense_golden_gpu.py).
// The functor states the terms operation by operation as the bodies do and sums in the order of include/lbfgsx.h: per output a
// row's products over L lanes (L the largest power of two <= F, at most 64) and the halving; the partial sums of A^T w over
// chunks of 256 rows, added in ascending chunk after the coordinate's own term; f is summed with a compensated accumulator, so
// its value does not depend on the order of the terms.
//
//     dense_probe <R> <F> <max iterations recorded>
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

static const double kC0 = 0.5;    // the ridge weight of the logistic model
static const double kAmp = 0.3;   // amplitude of the start
static const int kChunk = 256;    // C: rows per partial sum
static const int kOutputs = 3;    // D of the least-squares model

static const char* const kLogisticBody =
    "const T m = p0[r] * z[0];\n"
    "const T e = exp(m > T(0) ? T(0) - m : m);\n"
    "const T s = (m > T(0) ? e : T(1)) / (T(1) + e);\n"
    "dz[0] = T(0) - p0[r] * s;\n"
    "return (m > T(0) ? T(0) : T(0) - m) + log1p(e);";
static const char* const kRidgeBody =
    "g[0] = c[0] * x[0];\n"
    "return T(0.5) * (c[0] * (x[0] * x[0]));";
static const char* const kSquaresBody =
    "T q = T(0);\n"
    "#pragma unroll\n"
    "for (int k = 0; k < D; k++)\n"
    "{\n"
    "    const T u = z[k] - p0[r * D + k];\n"
    "    dz[k] = u;\n"
    "    q = q + u * u;\n"
    "}\n"
    "return T(0.5) * q;";

struct Matrix
{
    int R, F, L;
    std::vector<double> a, y, b;  // a: R x F row-major; y: R; b: R x kOutputs
    Matrix(int R_, int F_) : R(R_), F(F_)
    {
        for (int r = 0; r < R; r++)
        {
            for (int j = 0; j < F; j++)
                a.push_back(double((31 * r + 17 * j + 3 * r * j) % 13 - 6) / 4.0);
            y.push_back((5 * r) % 3 == 0 ? -1.0 : 1.0);
            for (int c = 0; c < kOutputs; c++)
                b.push_back(double((11 * r + 5 * c) % 7 - 3) / 2.0);
        }
        L = 1;
        while (L < 64 && 2 * L <= F)
            L *= 2;
    }
};

struct DenseModel
{
    const Matrix& M;
    const int D;
    const bool logistic;  // the logistic model with its ridge (D = 1), or plain least squares
    int calls = 0;
    std::vector<double> w;
    DenseModel(const Matrix& m, int D_, bool logistic_) : M(m), D(D_), logistic(logistic_), w(size_t(m.R) * size_t(D_)) {}
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
        const size_t Ds = size_t(D);
        std::vector<double> s(size_t(M.L)), z(Ds), dz(Ds);
        for (int r = 0; r < M.R; r++)
        {
            for (int c = 0; c < D; c++)
            {
                for (int l = 0; l < M.L; l++)
                    s[size_t(l)] = 0.0;
                for (int k = 0; k < M.F; k++)
                {
                    const int l = k % M.L;
                    const double prod = M.a[size_t(r) * size_t(M.F) + size_t(k)] * x[k * D + c];
                    s[size_t(l)] = k < M.L ? prod : s[size_t(l)] + prod;
                }
                for (int h = M.L / 2; h >= 1; h /= 2)
                    for (int l = 0; l < h; l++)
                        s[size_t(l)] = s[size_t(l)] + s[size_t(l + h)];
                z[size_t(c)] = s[0];
            }
            if (logistic)
            {
                const double yr = M.y[size_t(r)];
                const double m = yr * z[0];
                const double e = std::exp(m > 0.0 ? 0.0 - m : m);
                const double sg = (m > 0.0 ? e : 1.0) / (1.0 + e);
                dz[0] = 0.0 - yr * sg;
                add((m > 0.0 ? 0.0 : 0.0 - m) + std::log1p(e));
            }
            else
            {
                double q = 0.0;
                for (int k = 0; k < D; k++)
                {
                    const double u = z[size_t(k)] - M.b[size_t(r) * size_t(kOutputs) + size_t(k)];
                    dz[size_t(k)] = u;
                    q = q + u * u;
                }
                add(0.5 * q);
            }
            for (int k = 0; k < D; k++)
                w[size_t(r) * Ds + size_t(k)] = dz[size_t(k)];
        }
        const int n = M.F * D;
        for (int i = 0; i < n; i++)
        {
            const int j = i / D, c = i % D;
            double g = 0.0;
            bool any = false;
            if (logistic)
            {
                g = kC0 * x[i];
                any = true;
                add(0.5 * (kC0 * (x[i] * x[i])));
            }
            for (int r0 = 0; r0 < M.R; r0 += kChunk)
            {
                double part = 0.0;
                for (int r = r0; r < M.R && r < r0 + kChunk; r++)
                {
                    const double prod = M.a[size_t(r) * size_t(M.F) + size_t(j)] * w[size_t(r) * Ds + size_t(c)];
                    part = r == r0 ? prod : part + prod;
                }
                g = any ? g + part : part;
                any = true;
            }
            grad[i] = g;
        }
        return hi + lo;
    }
};

// no two weights alike, some negative; divisions, products and sums only
static Vector start(int n)
{
    Vector x(n);
    for (int i = 0; i < n; i++)
    {
        const double t = double(i + 1) / double(n + 1);
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

int main(int argc, char** argv)
{
    if (argc < 4)
    {
        std::fprintf(stderr, "usage: dense_probe <R> <F> <iterations>\n");
        return 2;
    }
    const int R = std::atoi(argv[1]), F = std::atoi(argv[2]), kmax = std::atoi(argv[3]);
    const Matrix M(R, F);
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
            Vector x = start(F);
            double fx = 0;
#ifdef DENSE_PROBE_DEVICE
            DenseLinearObjective<double> f(1, kLogisticBody, kRidgeBody);
            f.matrix(R, M.a.data(), F);
            f.host_data(0, M.y.data(), std::int64_t(M.y.size()));
            f.scalars({kC0});
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            DenseModel f(M, 1, true);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, f.calls, fx, x);
#endif
        }
        const int n = F * kOutputs;
        for (int k = 1; k <= kmax; k++)
        {
            LBFGSBParam<double> param;
            param.m = 6;
            param.epsilon = 0;
            param.epsilon_rel = 0;
            param.past = 0;
            param.max_iterations = k;
            LBFGSBSolver<double> solver(param);
            Vector x = start(n), lb = Vector::Constant(n, 0.0), ub = Vector::Constant(n, std::numeric_limits<double>::infinity());
            double fx = 0;
#ifdef DENSE_PROBE_DEVICE
            DenseLinearObjective<double> f(kOutputs, kSquaresBody);
            f.matrix(R, M.a.data(), F);
            f.host_data(0, M.b.data(), std::int64_t(M.b.size()));
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            DenseModel f(M, kOutputs, false);
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
    std::printf("DENSE PROBE OK\n");
    return 0;
}
