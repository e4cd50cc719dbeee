// small_dense.hpp — the small dense symmetric problems of a block eigensolver, on the host: header only, no device code, no library.
// spmv_lobpcg (solver_lobpcg.hip) forms Gram matrices of order up to 3 k = 48 on the device and solves them here; the routines take
// any order up to kMaxOrder.  Every matrix is row-major with leading dimension n.  tests/small_dense_check.cpp holds them to their bounds.
//
//   jacobi_eigh       A = V diag(w) V^T by cyclic Jacobi rotations (Rutishauser's arrangement: the diagonal is kept as a sum of
//                     corrections, a rotation whose off-diagonal entry is below rounding of both diagonal entries is set to zero
//                     instead); w ascending, the columns of V orthonormal.  Jacobi is as accurate on a graded diagonal as on a flat one.
//   cholesky_lower    G = L L^T in place (the lower triangle; the upper one is cleared), with the smallest PIVOT: the diagonal entry
//                     g_ii - sum_k l_ik^2 BEFORE its square root.  On a Gram matrix with unit diagonal that is the squared sine of the
//                     angle between column i and the span of the columns before it.
//   tri_inverse_lower L^-1 of a lower triangle
//   generalised_eigh  GA c = theta GB c for symmetric GA and positive definite GB: GB is scaled to unit diagonal (D = diag(GB)^-1/2),
//                     factored (D GB D = L L^T), M = L^-1 (D GA D) L^-T goes through jacobi_eigh, C = D L^-T Z.  C^T GB C = I and
//                     C^T GA C = diag(theta), theta ascending.  The smallest pivot of the scaled GB is reported: the caller's measure
//                     of how close the basis is to losing rank.
#pragma once

#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace spmv
{
namespace dense
{
constexpr int kMaxOrder  = 144;
constexpr int kMaxSweeps = 60;  // cyclic Jacobi converges quadratically: 6 to 10 sweeps at these orders

// A (n x n, symmetric; its upper triangle is read and destroyed) = V diag(w) V^T.  false: n out of range, or A is not finite
inline bool jacobi_eigh(int n, double* A, double* V, double* w)
{
    if (n < 1 || n > kMaxOrder) return false;
    std::vector<double> b(n), z(n, 0.0);
    for (int i = 0; i < n; ++i)
    {
        for (int j = 0; j < n; ++j) V[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
        b[i] = w[i] = A[(size_t)i * n + i];
    }
    auto rot = [&](double* M, size_t ij, size_t kl, double s, double tau) {
        const double g = M[ij], h = M[kl];
        M[ij] = g - s * (h + g * tau);
        M[kl] = h + s * (g - h * tau);
    };
    bool done = false;
    for (int sweep = 1; sweep <= kMaxSweeps && !done; ++sweep)
    {
        double sm = 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) sm += std::fabs(A[(size_t)p * n + q]);
        if (!std::isfinite(sm)) return false;
        if (sm == 0.0)
        {
            done = true;
            break;
        }
        const double tresh = sweep < 4 ? 0.2 * sm / ((double)n * n) : 0.0;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q)
            {
                const size_t pq = (size_t)p * n + q;
                const double apq = A[pq], g = 100.0 * std::fabs(apq);
                if (sweep > 4 && std::fabs(w[p]) + g == std::fabs(w[p]) && std::fabs(w[q]) + g == std::fabs(w[q]))
                    A[pq] = 0.0;
                else if (std::fabs(apq) > tresh)
                {
                    double h = w[q] - w[p], t;
                    if (std::fabs(h) + g == std::fabs(h))
                        t = apq / h;
                    else
                    {
                        const double theta = 0.5 * h / apq;
                        t                  = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                        if (theta < 0.0) t = -t;
                    }
                    const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c);
                    h = t * apq;
                    z[p] -= h;
                    z[q] += h;
                    w[p] -= h;
                    w[q] += h;
                    A[pq] = 0.0;
                    for (int j = 0; j < p; ++j) rot(A, (size_t)j * n + p, (size_t)j * n + q, s, tau);
                    for (int j = p + 1; j < q; ++j) rot(A, (size_t)p * n + j, (size_t)j * n + q, s, tau);
                    for (int j = q + 1; j < n; ++j) rot(A, (size_t)p * n + j, (size_t)q * n + j, s, tau);
                    for (int j = 0; j < n; ++j) rot(V, (size_t)j * n + p, (size_t)j * n + q, s, tau);
                }
            }
        for (int i = 0; i < n; ++i)
        {
            b[i] += z[i];
            w[i] = b[i];
            z[i] = 0.0;
        }
    }
    // ascending, by selection: the vectors move with their values
    for (int i = 0; i < n - 1; ++i)
    {
        int m = i;
        for (int j = i + 1; j < n; ++j)
            if (w[j] < w[m]) m = j;
        if (m == i) continue;
        std::swap(w[i], w[m]);
        for (int r = 0; r < n; ++r) std::swap(V[(size_t)r * n + i], V[(size_t)r * n + m]);
    }
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(w[i])) return false;
    return true;
}

// G = L L^T in place; *min_pivot: the smallest g_ii - sum_k l_ik^2 met (of the pivots up to a failure, that one included).
// false: n out of range, or a pivot that is not positive and finite (G is then partly overwritten)
inline bool cholesky_lower(int n, double* G, double* min_pivot)
{
    if (n < 1 || n > kMaxOrder) return false;
    double smallest = INFINITY;
    for (int j = 0; j < n; ++j)
    {
        double d = G[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d = std::fma(-G[(size_t)j * n + k], G[(size_t)j * n + k], d);
        if (!(d >= smallest)) smallest = d;  // (a NaN pivot is reported as such)
        if (!(d > 0.0) || !std::isfinite(d))
        {
            *min_pivot = smallest;
            return false;
        }
        const double ljj    = std::sqrt(d);
        G[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i)
        {
            double t = G[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t = std::fma(-G[(size_t)i * n + k], G[(size_t)j * n + k], t);
            G[(size_t)i * n + j] = t / ljj;
        }
        for (int i = 0; i < j; ++i) G[(size_t)i * n + j] = 0.0;
    }
    *min_pivot = smallest;
    return true;
}

// The first j whose pivot - cholesky_lower's, by the same sums - is below `threshold` or not positive and finite; -1: there is none
// (or n is out of range).  G is not written.  On a Gram matrix with unit diagonal: the first column that depends on those before it.
inline int cholesky_first_pivot_below(int n, const double* G, double threshold)
{
    if (n < 1 || n > kMaxOrder) return -1;
    std::vector<double> L(G, G + (size_t)n * n);
    for (int j = 0; j < n; ++j)
    {
        double d = L[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d = std::fma(-L[(size_t)j * n + k], L[(size_t)j * n + k], d);
        if (!(d > 0.0) || !std::isfinite(d) || d < threshold) return j;
        const double ljj    = std::sqrt(d);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i)
        {
            double t = L[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) t = std::fma(-L[(size_t)i * n + k], L[(size_t)j * n + k], t);
            L[(size_t)i * n + j] = t / ljj;
        }
    }
    return -1;
}

// Li = L^-1 of a lower triangle with a non-zero diagonal (column by column, forward substitution)
inline void tri_inverse_lower(int n, const double* L, double* Li)
{
    for (int j = 0; j < n; ++j)
    {
        for (int i = 0; i < j; ++i) Li[(size_t)i * n + j] = 0.0;
        Li[(size_t)j * n + j] = 1.0 / L[(size_t)j * n + j];
        for (int i = j + 1; i < n; ++i)
        {
            double t = 0.0;
            for (int k = j; k < i; ++k) t = std::fma(-L[(size_t)i * n + k], Li[(size_t)k * n + j], t);
            Li[(size_t)i * n + j] = t / L[(size_t)i * n + i];
        }
    }
}

// GA c = theta GB c: theta[n] ascending, column j of C (n x n) its vector, C^T GB C = I.  *min_pivot: of GB scaled to unit diagonal.
// false: n out of range, GB is not positive definite (to rounding), or something is not finite; theta and C are then undefined
inline bool generalised_eigh(int n, const double* GA, const double* GB, double* theta, double* C, double* min_pivot)
{
    *min_pivot = 0.0;
    if (n < 1 || n > kMaxOrder) return false;
    const size_t        nn = (size_t)n * n;
    std::vector<double> d(n), L(nn), Li(nn), T(nn), M(nn), Z(nn);
    for (int i = 0; i < n; ++i)
    {
        const double g = GB[(size_t)i * n + i];
        if (!(g > 0.0) || !std::isfinite(g))
        {
            *min_pivot = g;
            return false;
        }
        d[i] = 1.0 / std::sqrt(g);
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) L[(size_t)i * n + j] = i == j ? 1.0 : d[i] * GB[(size_t)i * n + j] * d[j];
    if (!cholesky_lower(n, L.data(), min_pivot)) return false;
    tri_inverse_lower(n, L.data(), Li.data());
    // T = Li (D GA D);  M = T Li^T, both triangles from the same sums
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            double t = 0.0;
            for (int k = 0; k <= i; ++k) t = std::fma(Li[(size_t)i * n + k], d[k] * GA[(size_t)k * n + j] * d[j], t);
            T[(size_t)i * n + j] = t;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j)
        {
            double t = 0.0;
            for (int k = 0; k <= j; ++k) t = std::fma(T[(size_t)i * n + k], Li[(size_t)j * n + k], t);
            M[(size_t)i * n + j] = t;
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
        {
            // (T Li^T is symmetric up to rounding: the mean of its two triangles)
            double u = 0.0;
            for (int k = 0; k <= i; ++k) u = std::fma(T[(size_t)j * n + k], Li[(size_t)i * n + k], u);
            const double m = 0.5 * (M[(size_t)i * n + j] + u);
            M[(size_t)i * n + j] = M[(size_t)j * n + i] = m;
        }
    if (!jacobi_eigh(n, M.data(), Z.data(), theta)) return false;
    // C = D Li^T Z
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
        {
            double t = 0.0;
            for (int k = i; k < n; ++k) t = std::fma(Li[(size_t)k * n + i], Z[(size_t)k * n + j], t);
            C[(size_t)i * n + j] = d[i] * t;
            if (!std::isfinite(C[(size_t)i * n + j])) return false;
        }
    return true;
}
}  // namespace dense
}  // namespace spmv
