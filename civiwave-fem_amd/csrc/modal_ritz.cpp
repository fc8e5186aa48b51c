// modal_ritz.cpp -- the Rayleigh-Ritz step of the subspace iteration (modal.cpp) on the host: the q x q
// generalised symmetric eigenproblem Kr Q = Mr Q Theta in fp64, q <= 32. Cholesky of the diagonally scaled Mr and
// cyclic Jacobi, written out here (no LAPACK); plain C++ with no device dependency.
#include "modal.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace cwf
{

int ritz_cholesky(double *A, uint32_t n)
{
    for (uint32_t j = 0; j < n; ++j)
    {
        double d = A[j * n + j];
        for (uint32_t k = 0; k < j; ++k)
            d -= A[j * n + k] * A[j * n + k];
        if (!(d > 0.0))
            return (int)j + 1;
        const double l = std::sqrt(d);
        A[j * n + j] = l;
        for (uint32_t i = j + 1; i < n; ++i)
        {
            double s = A[i * n + j];
            for (uint32_t k = 0; k < j; ++k)
                s -= A[i * n + k] * A[j * n + k];
            A[i * n + j] = s / l;
        }
        for (uint32_t c = j + 1; c < n; ++c)
            A[j * n + c] = 0.0;
    }
    return 0;
}

int ritz_jacobi(double *A, double *V, uint32_t n)
{
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j)
            V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep)
    {
        double off = 0.0, diag = 0.0;
        for (uint32_t i = 0; i < n; ++i)
        {
            diag += A[i * n + i] * A[i * n + i];
            for (uint32_t j = i + 1; j < n; ++j)
                off += A[i * n + j] * A[i * n + j];
        }
        // every remaining rotation would change an eigenvalue by less than an ulp of the spectrum's scale
        if (off <= 1e-34 * diag || off == 0.0)
            return sweep;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; ++q)
            {
                const double apq = A[p * n + q];
                if (apq == 0.0)
                    continue;
                // Rutishauser's rotation: t = tan(phi), the smaller root, |phi| <= pi / 4
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (uint32_t k = 0; k < n; ++k)  // columns p, q
                {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (uint32_t k = 0; k < n; ++k)  // rows p, q
                {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                A[p * n + q] = A[q * n + p] = 0.0;
                for (uint32_t k = 0; k < n; ++k)
                {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    return -1;
}

int ritz_solve(const double *Kr, const double *Mr, uint32_t n, double *theta, double *Q)
{
    std::vector<double> d(n), L((size_t)n * n), C((size_t)n * n), V((size_t)n * n), T((size_t)n * n);
    for (uint32_t i = 0; i < n; ++i)
    {
        if (!(Mr[i * n + i] > 0.0))
            return (int)i + 1;
        d[i] = 1.0 / std::sqrt(Mr[i * n + i]);
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j = 0; j < n; ++j)
        {
            L[i * n + j] = d[i] * Mr[i * n + j] * d[j];
            C[i * n + j] = d[i] * Kr[i * n + j] * d[j];
        }
    if (int st = ritz_cholesky(L.data(), n))
        return st;
    // T = L^-1 C (forward substitution on every column), then C = T L^-T = (L^-1 T^T)^T
    for (uint32_t c = 0; c < n; ++c)
        for (uint32_t i = 0; i < n; ++i)
        {
            double s = C[i * n + c];
            for (uint32_t k = 0; k < i; ++k)
                s -= L[i * n + k] * T[k * n + c];
            T[i * n + c] = s / L[i * n + i];
        }
    for (uint32_t r = 0; r < n; ++r)
        for (uint32_t i = 0; i < n; ++i)
        {
            double s = T[r * n + i];
            for (uint32_t k = 0; k < i; ++k)
                s -= L[i * n + k] * C[r * n + k];
            C[r * n + i] = s / L[i * n + i];
        }
    for (uint32_t i = 0; i < n; ++i)  // the two substitutions round differently: Jacobi wants exact symmetry
        for (uint32_t j = i + 1; j < n; ++j)
            C[i * n + j] = C[j * n + i] = 0.5 * (C[i * n + j] + C[j * n + i]);
    if (ritz_jacobi(C.data(), V.data(), n) < 0)
        return -1;
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return C[a * n + a] < C[b * n + b]; });
    // Q = D L^-T V: back substitution L^T z = v for every eigenvector, then the diagonal scale
    for (uint32_t o = 0; o < n; ++o)
    {
        const uint32_t c = order[o];
        theta[o] = C[c * n + c];
        for (uint32_t ii = n; ii-- > 0;)
        {
            double s = V[ii * n + c];
            for (uint32_t k = ii + 1; k < n; ++k)
                s -= L[k * n + ii] * T[k * n + o];
            T[ii * n + o] = s / L[ii * n + ii];
        }
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t o = 0; o < n; ++o)
            Q[i * n + o] = d[i] * T[i * n + o];
    return 0;
}

}  // namespace cwf
