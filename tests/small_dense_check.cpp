// Properties of arm-spmv_amd/csrc/small_dense.hpp (the small dense symmetric problems of spmv_lobpcg, on the host).
// Compiled and run by tests/test_small_dense.py, once plainly and once with -fsanitize=address,undefined; prints one summary line.
// Orders 1..8, 15, 16, 17, 47, 48, 49, 96, 144.  Matrices: random symmetric, the identity, repeated eigenvalues, a graded diagonal
// (1 .. 1e12, bare and under small couplings), and for the generalised problem a GB that is nearly singular.  With eps = 2^-52,
// ||.|| the largest absolute row sum and B(A) = 64 order eps ||A||:
//   * jacobi_eigh:       ||A V - V W||_max <= B(A), ||V^T V - I||_max <= B(I), the values ascending;
//   * cholesky_first_pivot_below: the first pivot below a threshold, by cholesky_lower's own sums (the threshold at the smallest pivot
//                        and one ulp above it), G left alone
//   * cholesky_lower:    L L^T = G to B(G), the upper triangle cleared, the reported pivot EQUAL to the smallest one of a second
//                        factorisation written out here (the same sums in the same order), and the factor's own diagonal squared agrees;
//   * tri_inverse_lower: L Li = I to B(I) cond(L);
//   * generalised_eigh:  ||C^T GB C - I||_max <= B(I) cond(GB) and ||C^T GA C - Theta||_max <= B(GA') cond(GB), theta ascending, where
//                        GA' is GA in GB's unit-diagonal scaling and cond(GB) = 1 / (the reported smallest pivot): the pivots of a
//                        unit-diagonal matrix are at most 1 and their smallest bounds 1 / lambda_min from below.
// The sums of the checks themselves are taken in long double.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "small_dense.hpp"

using namespace spmv::dense;
typedef long double ld;

static uint64_t g_state = 0x243F6A8885A308D3ull;
static double   rnd()  // [-1, 1)
{
    g_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_state;
    z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-52 - 1.0;
}

static const double kEps = 0x1.0p-52;
static long long    bad = 0, checked = 0;
static double       worst = 0.0;  // the largest error / bound seen

static double norm_inf(int n, const std::vector<double>& A)
{
    double m = 0.0;
    for (int i = 0; i < n; ++i)
    {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += std::fabs(A[(size_t)i * n + j]);
        m = std::fmax(m, s);
    }
    return m;
}

static void expect(bool ok, const char* what, int n, double err, double bound)
{
    ++checked;
    if (bound > 0.0) worst = std::fmax(worst, err / bound);
    if (!ok)
    {
        ++bad;
        std::printf("  FAIL %s at order %d: %.3e against %.3e\n", what, n, err, bound);
    }
}

// Q: a random orthogonal matrix as a product of n reflections
static std::vector<double> random_orthogonal(int n)
{
    std::vector<double> Q((size_t)n * n, 0.0), v(n);
    for (int i = 0; i < n; ++i) Q[(size_t)i * n + i] = 1.0;
    for (int r = 0; r < n; ++r)
    {
        ld vv = 0;
        for (int i = 0; i < n; ++i)
        {
            v[i] = rnd();
            vv += (ld)v[i] * v[i];
        }
        if (vv == 0) continue;
        for (int j = 0; j < n; ++j)
        {
            ld d = 0;
            for (int i = 0; i < n; ++i) d += (ld)v[i] * Q[(size_t)i * n + j];
            const double f = (double)(2 * d / vv);
            for (int i = 0; i < n; ++i) Q[(size_t)i * n + j] -= f * v[i];
        }
    }
    return Q;
}

// Q diag(w) Q^T, exactly symmetric
static std::vector<double> with_spectrum(int n, const std::vector<double>& w)
{
    const std::vector<double> Q = random_orthogonal(n);
    std::vector<double>       A((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
        {
            ld s = 0;
            for (int k = 0; k < n; ++k) s += (ld)Q[(size_t)i * n + k] * w[k] * Q[(size_t)j * n + k];
            A[(size_t)i * n + j] = A[(size_t)j * n + i] = (double)s;
        }
    return A;
}

static void check_eigh(int n, const std::vector<double>& A, const char* what)
{
    std::vector<double> W((size_t)n * n), V((size_t)n * n), w(n);
    W = A;
    const bool ok = jacobi_eigh(n, W.data(), V.data(), w.data());
    expect(ok, what, n, 0, 0);
    if (!ok) return;
    const double bA = 64.0 * n * kEps * norm_inf(n, A), bI = 64.0 * n * kEps;
    double       e_res = 0.0, e_orth = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            ld r = 0, o = 0;
            for (int k = 0; k < n; ++k)
            {
                r += (ld)A[(size_t)i * n + k] * V[(size_t)k * n + j];
                o += (ld)V[(size_t)k * n + i] * V[(size_t)k * n + j];
            }
            r -= (ld)V[(size_t)i * n + j] * w[j];
            o -= i == j ? 1 : 0;
            e_res  = std::fmax(e_res, (double)fabsl(r));
            e_orth = std::fmax(e_orth, (double)fabsl(o));
        }
    expect(e_res <= bA, what, n, e_res, bA);
    expect(e_orth <= bI, "orthonormal vectors", n, e_orth, bI);
    bool asc = true;
    for (int i = 1; i < n; ++i) asc = asc && w[i - 1] <= w[i];
    expect(asc, "ascending values", n, 0, 0);
}

// the same factorisation written out again: the pivots of G in cholesky_lower's own sums
static double pivots_again(int n, std::vector<double> G)
{
    double smallest = INFINITY;
    for (int j = 0; j < n; ++j)
    {
        double d = G[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d = std::fma(-G[(size_t)j * n + k], G[(size_t)j * n + k], d);
        smallest = std::fmin(smallest, d);
        if (!(d > 0.0)) break;
        const double ljj     = std::sqrt(d);
        G[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i)
        {
            double t = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t = std::fma(-G[(size_t)i * n + k], G[(size_t)j * n + k], t);
            G[(size_t)i * n + j] = t / ljj;
        }
    }
    return smallest;
}

static void check_cholesky(int n, const std::vector<double>& G, double cond)
{
    std::vector<double> L = G, Li((size_t)n * n);
    double              piv = -1.0;
    const bool          ok  = cholesky_lower(n, L.data(), &piv);
    expect(ok, "cholesky of a positive definite matrix", n, 0, 0);
    if (!ok) return;
    expect(piv == pivots_again(n, G), "the reported pivot is the smallest one", n, piv - pivots_again(n, G), 0);
    double dmin = INFINITY;
    for (int i = 0; i < n; ++i) dmin = std::fmin(dmin, L[(size_t)i * n + i] * L[(size_t)i * n + i]);
    expect(std::fabs(dmin - piv) <= 4 * kEps * piv, "the pivot is the factor's smallest squared diagonal entry", n, std::fabs(dmin - piv), 4 * kEps * piv);
    const double bG = 64.0 * n * kEps * norm_inf(n, G);
    double       e = 0.0, up = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            ld s = 0;
            for (int k = 0; k < n; ++k) s += (ld)L[(size_t)i * n + k] * L[(size_t)j * n + k];
            e = std::fmax(e, (double)fabsl(s - G[(size_t)i * n + j]));
            if (j > i) up = std::fmax(up, std::fabs(L[(size_t)i * n + j]));
        }
    expect(e <= bG, "L L^T = G", n, e, bG);
    expect(up == 0.0, "upper triangle cleared", n, up, 0);
    tri_inverse_lower(n, L.data(), Li.data());
    double ei = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            ld s = 0;
            for (int k = 0; k < n; ++k) s += (ld)L[(size_t)i * n + k] * Li[(size_t)k * n + j];
            ei = std::fmax(ei, (double)fabsl(s - (i == j ? 1 : 0)));
        }
    expect(ei <= 64.0 * n * kEps * cond, "L Li = I", n, ei, 64.0 * n * kEps * cond);
}

static void check_generalised(int n, const std::vector<double>& GA, const std::vector<double>& GB, const char* what)
{
    std::vector<double> theta(n), C((size_t)n * n);
    double              piv = 0.0;
    const bool          ok  = generalised_eigh(n, GA.data(), GB.data(), theta.data(), C.data(), &piv);
    expect(ok, what, n, 0, 0);
    if (!ok) return;
    expect(piv > 0.0 && piv <= 1.0 + 4 * kEps, "pivot of the scaled GB in (0, 1]", n, piv, 0);
    const double        cond = 1.0 / piv;
    std::vector<double> GAs((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            GAs[(size_t)i * n + j] = GA[(size_t)i * n + j] / std::sqrt(GB[(size_t)i * n + i] * GB[(size_t)j * n + j]);
    const double bI = 64.0 * n * kEps * cond, bA = 64.0 * n * kEps * norm_inf(n, GAs) * cond;
    // T1 = GB C, T2 = GA C in long double; then C^T T
    std::vector<ld> T1((size_t)n * n), T2((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            ld a = 0, b = 0;
            for (int k = 0; k < n; ++k)
            {
                b += (ld)GB[(size_t)i * n + k] * C[(size_t)k * n + j];
                a += (ld)GA[(size_t)i * n + k] * C[(size_t)k * n + j];
            }
            T1[(size_t)i * n + j] = b;
            T2[(size_t)i * n + j] = a;
        }
    double eb = 0.0, ea = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            ld a = 0, b = 0;
            for (int k = 0; k < n; ++k)
            {
                b += (ld)C[(size_t)k * n + i] * T1[(size_t)k * n + j];
                a += (ld)C[(size_t)k * n + i] * T2[(size_t)k * n + j];
            }
            eb = std::fmax(eb, (double)fabsl(b - (i == j ? 1 : 0)));
            ea = std::fmax(ea, (double)fabsl(a - (i == j ? (ld)theta[i] : 0)));
        }
    expect(eb <= bI, "C^T GB C = I", n, eb, bI);
    expect(ea <= bA, "C^T GA C = Theta", n, ea, bA);
    bool asc = true;
    for (int i = 1; i < n; ++i) asc = asc && theta[i - 1] <= theta[i];
    expect(asc, "ascending theta", n, 0, 0);
}

int main()
{
    const int orders[] = {1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 47, 48, 49, 96, 144};
    int       norders  = 0;
    for (int n : orders)
    {
        ++norders;
        const size_t        nn = (size_t)n * n;
        std::vector<double> A(nn), I(nn, 0.0), w(n);
        // random symmetric
        for (int i = 0; i < n; ++i)
            for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = rnd();
        check_eigh(n, A, "random symmetric");
        for (int i = 0; i < n; ++i) I[(size_t)i * n + i] = 1.0;
        check_eigh(n, I, "identity");
        // repeated eigenvalues: three distinct values
        for (int i = 0; i < n; ++i) w[i] = (double)(i % 3) - 1.0;
        check_eigh(n, with_spectrum(n, w), "repeated eigenvalues");
        // graded diagonal 1 .. 1e12: bare, and under couplings of the size of the smaller diagonal entry's root
        std::vector<double> D(nn, 0.0), Dc(nn, 0.0);
        for (int i = 0; i < n; ++i) w[i] = n == 1 ? 1.0 : std::pow(10.0, 12.0 * i / (n - 1));
        for (int i = 0; i < n; ++i) D[(size_t)i * n + i] = Dc[(size_t)i * n + i] = w[i];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j) Dc[(size_t)i * n + j] = Dc[(size_t)j * n + i] = 0.25 * rnd() * std::sqrt(w[j]) / n;
        check_eigh(n, D, "graded diagonal");
        check_eigh(n, Dc, "graded diagonal with couplings");
        // Cholesky: well conditioned, then nearly singular (cond 1e8)
        for (int i = 0; i < n; ++i) w[i] = 1.0 + 0.5 * rnd();
        check_cholesky(n, with_spectrum(n, w), 4.0);
        for (int i = 0; i < n; ++i) w[i] = n == 1 ? 1.0 : std::pow(10.0, -8.0 * i / (n - 1));
        const std::vector<double> Gs = with_spectrum(n, w);
        check_cholesky(n, Gs, 1e8);
        // the generalised problem: GB = identity, well conditioned, nearly singular
        check_generalised(n, A, I, "generalised, GB = I");
        for (int i = 0; i < n; ++i) w[i] = 1.0 + 0.5 * rnd();
        check_generalised(n, A, with_spectrum(n, w), "generalised, GB well conditioned");
        check_generalised(n, A, Gs, "generalised, GB nearly singular");
        check_generalised(n, Dc, Gs, "generalised, graded GA, GB nearly singular");
    }
    // refusals: an indefinite GB, a matrix with a NaN, orders out of range
    {
        std::vector<double> G = {1.0, 2.0, 2.0, 1.0}, L = G, th(2), C(4), N = {1.0, NAN, NAN, 1.0}, V(4);
        double              piv = 1.0;
        expect(!cholesky_lower(2, L.data(), &piv) && piv == -3.0, "an indefinite matrix is refused with its pivot", 2, piv + 3.0, 0);
        expect(!generalised_eigh(2, G.data(), G.data(), th.data(), C.data(), &piv), "an indefinite GB is refused", 2, 0, 0);
        expect(cholesky_first_pivot_below(2, G.data(), 0.0) == 1 && G[1] == 2.0, "the first pivot that is not positive, G left alone", 2, 0, 0);
        // three unit columns, the third at an angle of 1e-4 to the second: pivots 1, 1, about 1e-8
        const double        s = 1e-4, c = std::sqrt(1.0 - s * s);
        std::vector<double> D = {1.0, 0.0, 0.0, 0.0, 1.0, c, 0.0, c, 1.0};
        expect(cholesky_first_pivot_below(3, D.data(), 1e-6) == 2 && cholesky_first_pivot_below(3, D.data(), 1e-9) == -1, "the first pivot below a threshold", 3,
               0, 0);
        std::vector<double> Dl = D;
        expect(cholesky_lower(3, Dl.data(), &piv) && cholesky_first_pivot_below(3, D.data(), piv) == -1 &&
                   cholesky_first_pivot_below(3, D.data(), std::nextafter(piv, 1.0)) == 2,
               "the pivots are cholesky_lower's own", 3, 0, 0);
        expect(cholesky_first_pivot_below(0, D.data(), 1.0) == -1 && cholesky_first_pivot_below(kMaxOrder + 1, D.data(), 1.0) == -1, "orders out of range", 0, 0, 0);
        expect(!jacobi_eigh(2, N.data(), V.data(), th.data()), "a NaN is refused", 2, 0, 0);
        expect(!jacobi_eigh(0, N.data(), V.data(), th.data()) && !jacobi_eigh(kMaxOrder + 1, N.data(), V.data(), th.data()), "orders out of range", 0, 0, 0);
    }
    std::printf("small_dense: %d orders up to %d, %lld checks, worst error / bound %.3g, %lld violations\n", norders, kMaxOrder, checked, worst, bad);
    return bad ? 1 : 0;
}
