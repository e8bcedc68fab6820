// tests/cpp/multilinear_probe.cpp -- two linear models with D outputs per row over one sparse R x F matrix A, Z = A X, x the
// F x D matrix X feature-major (x[j*D + c], n = F*D):
//     multi-class squared hinge + ridge   f(x) = sum over rows r of sum_{c != y_r} max(0, (1 + Z[r,c]) - Z[r,y_r])^2
//                                                + sum over i of c0/2 x_i^2      through LBFGSSolver with the More-Thuente search,
//     multi-target non-negative least squares  f(x) = sum over rows r of 1/2 sum_c (Z[r,c] - b[r,c])^2,  0 <= x
//                             through LBFGSBSolver from a start with negative entries (bounds active at the start),
// iterate by iterate.  The matrix is tests/cpp/linear_probe.cpp's: row r has kPer entries, entry j in column
// (7 r + 3 j j + j) mod F (two entries of a row may share a column: both count) with value (((31 r + 17 j) mod 13) - 6) / 4;
// y_r = 5 r mod D; b[r,c] = (((11 r + 5 c) mod 7) - 3) / 2.  Integers and exact quotients only, so that the test's numpy
// restatement gives the same doubles.
//
// One source, two builds:
//   * plain:                     a host functor, compiled against the headers on the include path -- the reference's with
//                                oracle/eigen_shim as Eigen for the fixture (tests/golden/make_multilinear_golden.py);
//   * -DMULTILINEAR_PROBE_DEVICE a MultiLinearObjective<double> with the same bodies, compiled against include/ and run on the
//                                GPU (tests/test_multilinear_objective_gpu.py).
// The functor states the terms operation by operation as the bodies do and sums in the order of include/lbfgsx.h: per output a
// row's products over L lanes (L by the library's rule) and the halving, a coordinate's contributions after its own term in
// ascending CSR position; f is summed with a compensated accumulator, so its value does not depend on the order of the terms.
//
//     multilinear_probe <R> <F> <D> <max iterations recorded>
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
static const double kAmp = 0.3;   // amplitude of the start

static const char* const kHingeBody =
    "const int y = int(p0[r]);\n"
    "T zy = z[0];\n"
    "#pragma unroll\n"
    "for (int k = 1; k < D; k++)\n"
    "    zy = k == y ? z[k] : zy;\n"
    "T v = T(0), sd = T(0);\n"
    "#pragma unroll\n"
    "for (int k = 0; k < D; k++)\n"
    "{\n"
    "    const T m = (T(1) + z[k]) - zy;\n"
    "    const T h = (k != y && m > T(0)) ? m : T(0);\n"
    "    const T h2 = T(2) * h;\n"
    "    dz[k] = h2;\n"
    "    v = v + h * h;\n"
    "    sd = sd + h2;\n"
    "}\n"
    "#pragma unroll\n"
    "for (int k = 0; k < D; k++)\n"
    "    dz[k] = k == y ? T(0) - sd : dz[k];\n"
    "return v;";
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
    int R, F, D, L;
    std::vector<std::int32_t> rowptr, col;
    std::vector<double> val, y, b;
    std::vector<std::vector<int> > byCol;  // per column: CSR positions, ascending
    Matrix(int R_, int F_, int D_) : R(R_), F(F_), D(D_), byCol(size_t(F_))
    {
        rowptr.push_back(0);
        for (int r = 0; r < R; r++)
        {
            for (int j = 0; j < kPer; j++)
            {
                col.push_back(std::int32_t((7 * r + 3 * j * j + j) % F));
                val.push_back(double((31 * r + 17 * j) % 13 - 6) / 4.0);
            }
            rowptr.push_back(std::int32_t(col.size()));
            y.push_back(double((5 * r) % D));
            for (int c = 0; c < D; c++)
                b.push_back(double((11 * r + 5 * c) % 7 - 3) / 2.0);
        }
        for (size_t k = 0; k < col.size(); k++)
            byCol[size_t(col[k])].push_back(int(k));
        // the library's rule: the largest power of two <= max(1, nnz / R), at most 64
        L = 1;
        while (L < 64 && 2 * L <= int(col.size()) / R)
            L *= 2;
    }
    int n() const { return F * D; }
    std::int64_t nnz() const { return std::int64_t(col.size()); }
    int rowOf(int k) const { return k / kPer; }
};

struct MultiLinearModel
{
    const Matrix& M;
    const bool hinge;  // the hinge model with its ridge, or plain least squares
    int calls = 0;
    std::vector<double> w;
    MultiLinearModel(const Matrix& m, bool hinge_) : M(m), hinge(hinge_), w(size_t(m.R) * size_t(m.D)) {}
    double operator()(const Vector& x, Vector& grad)
    {
        calls++;
        const int D = M.D;
        double hi = 0.0, lo = 0.0;  // f = hi + lo: TwoSum of every term
        auto add = [&](double v) {
            const double s = hi + v;
            const double bb = s - hi;
            lo += (hi - (s - bb)) + (v - bb);
            hi = s;
        };
        const size_t Ds = size_t(D);
        std::vector<double> s(size_t(M.L)), z(Ds), dz(Ds);
        std::vector<char> has(size_t(M.L));
        for (int r = 0; r < M.R; r++)
        {
            for (int c = 0; c < D; c++)
            {
                for (int l = 0; l < M.L; l++)
                {
                    s[size_t(l)] = 0.0;
                    has[size_t(l)] = 0;
                }
                for (int k = M.rowptr[size_t(r)]; k < M.rowptr[size_t(r) + 1]; k++)
                {
                    const int l = (k - M.rowptr[size_t(r)]) % M.L;
                    const double prod = M.val[size_t(k)] * x[M.col[size_t(k)] * D + c];
                    s[size_t(l)] = has[size_t(l)] ? s[size_t(l)] + prod : prod;
                    has[size_t(l)] = 1;
                }
                for (int h = M.L / 2; h >= 1; h /= 2)
                    for (int l = 0; l < h; l++)
                        s[size_t(l)] = s[size_t(l)] + s[size_t(l + h)];
                z[size_t(c)] = s[0];
            }
            if (hinge)
            {
                const int y = int(M.y[size_t(r)]);
                const double zy = z[size_t(y)];
                double v = 0.0, sd = 0.0;
                for (int k = 0; k < D; k++)
                {
                    const double m = (1.0 + z[size_t(k)]) - zy;
                    const double h = (k != y && m > 0.0) ? m : 0.0;
                    const double h2 = 2.0 * h;
                    dz[size_t(k)] = h2;
                    v = v + h * h;
                    sd = sd + h2;
                }
                dz[size_t(y)] = 0.0 - sd;
                add(v);
            }
            else
            {
                double q = 0.0;
                for (int k = 0; k < D; k++)
                {
                    const double u = z[size_t(k)] - M.b[size_t(r) * size_t(D) + size_t(k)];
                    dz[size_t(k)] = u;
                    q = q + u * u;
                }
                add(0.5 * q);
            }
            for (int k = 0; k < D; k++)
                w[size_t(r) * size_t(D) + size_t(k)] = dz[size_t(k)];
        }
        for (int i = 0; i < M.n(); i++)
        {
            const int j = i / D, c = i % D;
            double g = 0.0;
            bool any = false;
            if (hinge)
            {
                g = kC0 * x[i];
                any = true;
                add(0.5 * (kC0 * (x[i] * x[i])));
            }
            for (int k : M.byCol[size_t(j)])
            {
                const double prod = M.val[size_t(k)] * w[size_t(M.rowOf(k)) * size_t(D) + size_t(c)];
                g = any ? g + prod : prod;
                any = true;
            }
            grad[i] = g;
        }
        return hi + lo;
    }
};

// no two weights alike, some negative; divisions, products and sums only
static Vector start(const Matrix& M)
{
    const int n = M.n();
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

#ifdef MULTILINEAR_PROBE_DEVICE
static void setup(MultiLinearObjective<double>& f, const Matrix& M, const std::vector<double>& data)
{
    f.matrix(M.R, M.nnz(), M.rowptr.data(), M.col.data(), M.val.data());
    f.host_data(0, data.data(), std::int64_t(data.size()));
    f.scalars({kC0});
}
#endif

int main(int argc, char** argv)
{
    if (argc < 5)
    {
        std::fprintf(stderr, "usage: multilinear_probe <R> <F> <D> <iterations>\n");
        return 2;
    }
    const int R = std::atoi(argv[1]), F = std::atoi(argv[2]), D = std::atoi(argv[3]), kmax = std::atoi(argv[4]);
    const Matrix M(R, F, D);
    const int n = M.n();
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
#ifdef MULTILINEAR_PROBE_DEVICE
            MultiLinearObjective<double> f(D, kHingeBody, kRidgeBody);
            setup(f, M, M.y);
            const int niter = solver.minimize(f, x, fx);
            emit("lbfgs", k, niter, -1, fx, x);
#else
            MultiLinearModel f(M, true);
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
#ifdef MULTILINEAR_PROBE_DEVICE
            MultiLinearObjective<double> f(D, kSquaresBody);
            setup(f, M, M.b);
            const int niter = solver.minimize(f, x, fx, lb, ub);
            emit("lbfgsb", k, niter, -1, fx, x);
#else
            MultiLinearModel f(M, false);
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
    std::printf("MULTILINEAR PROBE OK\n");
    return 0;
}
