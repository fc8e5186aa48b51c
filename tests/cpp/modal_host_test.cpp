// modal_host_test.cpp -- the host Rayleigh-Ritz step of the modal analysis (csrc/modal_ritz.cpp: Cholesky of the
// scaled Mr + cyclic Jacobi) on pairs whose eigenvalues are known by construction. No GPU call. Builds against
// libcwf_hip.so, or stand-alone together with modal_ritz.cpp (then also under -fsanitize=address,undefined).
//
// Construction: B = G1 diag(s) G2 S with G1, G2 products of Givens rotations, s in [1, 3] and S a diagonal scale, all
// in long double; Mr = B^T B and Kr = B^T Lambda B rounded to double. Then Kr q = lambda Mr q has exactly the
// eigenvalues Lambda (q = B^-1 e_i). Rounding the entries of Mr and Kr perturbs them relatively, entry by entry,
// which commutes with S: the eigenvalues move by about cond(G1 diag(s) G2)^2 eps ~ 1e-15 relative whatever S is.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "modal.hpp"

namespace
{

using ld = long double;
int failures = 0;

void check(bool ok, const char *what, double got, double bound)
{
    if (!ok)
    {
        std::printf("FAIL %s: %.3e > %.3e\n", what, got, bound);
        ++failures;
    }
}

void givens(std::vector<ld> &A, int n, int p, int q, ld angle, bool left)
{
    const ld c = std::cos(angle), s = std::sin(angle);
    for (int k = 0; k < n; ++k)
    {
        ld &x = left ? A[p * n + k] : A[k * n + p];
        ld &y = left ? A[q * n + k] : A[k * n + q];
        const ld a = x, b = y;
        x = c * a - s * b;
        y = s * a + c * b;
    }
}

// B = G1 diag(s) G2 S
std::vector<ld> make_B(int n, const std::vector<ld> &scale)
{
    std::vector<ld> B((size_t)n * n, 0.0L);
    for (int i = 0; i < n; ++i)
        B[i * n + i] = 1.0L + 2.0L * i / (n - 1);
    ld angle = 0.3L;
    for (int p = 0; p < n; ++p)
        for (int q = p + 1; q < n; ++q)
        {
            givens(B, n, p, q, angle, true);
            givens(B, n, p, q, angle * 0.7L + 0.2L, false);
            angle = std::fmod(angle * 1.7L + 0.41L, 3.0L);
        }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            B[i * n + j] *= scale[j];
    return B;
}

void run_case(const char *name, int n, const std::vector<ld> &lambda, const std::vector<ld> &scale)
{
    const std::vector<ld> B = make_B(n, scale);
    std::vector<double> Kr((size_t)n * n), Mr((size_t)n * n), Q((size_t)n * n), theta(n);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j)
        {
            ld m = 0.0L, k = 0.0L;
            for (int r = 0; r < n; ++r)
            {
                m += B[r * n + i] * B[r * n + j];
                k += B[r * n + i] * lambda[r] * B[r * n + j];
            }
            Mr[i * n + j] = Mr[j * n + i] = (double)m;
            Kr[i * n + j] = Kr[j * n + i] = (double)k;
        }
    const int st = cwf::ritz_solve(Kr.data(), Mr.data(), (uint32_t)n, theta.data(), Q.data());
    if (st)
    {
        std::printf("FAIL %s: ritz_solve returned %d\n", name, st);
        ++failures;
        return;
    }
    std::vector<ld> sorted(lambda);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (sorted[j] < sorted[i])
                std::swap(sorted[i], sorted[j]);
    double worst_ev = 0.0, worst_m = 0.0, worst_k = 0.0;
    for (int i = 0; i < n; ++i)
    {
        worst_ev = std::max(worst_ev, (double)(std::fabs((ld)theta[i] - sorted[i]) / sorted[i]));
        if (i && theta[i] < theta[i - 1])
            check(false, "ascending order", theta[i - 1], theta[i]);
    }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b)
        {
            ld m = 0.0L, k = 0.0L;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                {
                    m += (ld)Q[i * n + a] * (ld)Mr[i * n + j] * (ld)Q[j * n + b];
                    k += (ld)Q[i * n + a] * (ld)Kr[i * n + j] * (ld)Q[j * n + b];
                }
            worst_m = std::max(worst_m, (double)std::fabs(m - (a == b ? 1.0L : 0.0L)));
            // Theta's entries span a decade: each one is measured on the scale of its own pair of Ritz values
            const ld scale_k = std::sqrt((ld)theta[a] * (ld)theta[b]);
            worst_k = std::max(worst_k, (double)(std::fabs(k - (a == b ? (ld)theta[a] : 0.0L)) / scale_k));
        }
    std::printf("%s: eigenvalue %.2e, Q^T Mr Q - I %.2e, Q^T Kr Q - Theta %.2e\n", name, worst_ev, worst_m, worst_k);
    check(worst_ev <= 1e-12, name, worst_ev, 1e-12);
    check(worst_m <= 1e-12, name, worst_m, 1e-12);
    check(worst_k <= 1e-12, name, worst_k, 1e-12);
}

}  // namespace

int main()
{
    const int n = 12;
    const std::vector<ld> ones(n, 1.0L);
    // distinct eigenvalues
    run_case("spd12", n, {0.5L, 1.0L, 1.75L, 2.5L, 3.0L, 4.25L, 5.0L, 6.5L, 7.0L, 8.0L, 9.5L, 12.0L}, ones);
    // repeated: a double and a triple eigenvalue (the bending pairs of a symmetric section)
    run_case("repeated", n, {1.0L, 2.0L, 2.0L, 3.0L, 5.0L, 5.0L, 5.0L, 6.0L, 7.5L, 9.0L, 9.0L, 11.0L}, ones);
    // nearly singular Mr: columns scaled over ten decades, as a block whose columns are x_j ~ 1 / theta_j is;
    // cond(Mr) ~ 1e21 before ritz_solve's diagonal scaling
    std::vector<ld> graded(n);
    for (int j = 0; j < n; ++j)
        graded[j] = std::pow(10.0L, -(ld)((j * 7) % n) * 10.0L / (n - 1));
    run_case("graded", n, {0.5L, 1.0L, 1.75L, 2.5L, 3.0L, 4.25L, 5.0L, 6.5L, 7.0L, 8.0L, 9.5L, 12.0L}, graded);

    // a matrix that is not positive definite is reported with its pivot, not factored
    {
        double A[9] = {4.0, 2.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0, 1.0};  // rank 2: pivot 1 is 0
        const int st = cwf::ritz_cholesky(A, 3);
        check(st == 2, "cholesky pivot", (double)st, 2.0);
        double K[4] = {1.0, 0.0, 0.0, 1.0}, M[4] = {1.0, 1.0, 1.0, 1.0}, th[2], Q[4];
        check(cwf::ritz_solve(K, M, 2, th, Q) == 2, "ritz_solve rank", 0.0, 0.0);
    }
    // Jacobi on a 2 x 2 with a known spectrum: [[2, 1], [1, 2]] -> {1, 3}
    {
        double A[4] = {2.0, 1.0, 1.0, 2.0}, V[4];
        const int sweeps = cwf::ritz_jacobi(A, V, 2);
        const double lo = std::min(A[0], A[3]), hi = std::max(A[0], A[3]);
        check(sweeps >= 0 && std::fabs(lo - 1.0) <= 1e-15 && std::fabs(hi - 3.0) <= 1e-15, "jacobi 2x2", lo, hi);
    }
    // the start vectors are a pure function of (column, dof), in [-1, 1), column 0 all ones
    {
        bool ok = cwf::modal_start_value(0, 12345) == 1.0f;
        for (uint32_t c = 1; c < 32; ++c)
            for (uint64_t d = 0; d < 1000; ++d)
            {
                const float v = cwf::modal_start_value(c, d);
                ok = ok && v >= -1.0f && v < 1.0f && v == cwf::modal_start_value(c, d);
            }
        ok = ok && cwf::modal_start_value(1, 7) != cwf::modal_start_value(2, 7);
        check(ok, "start values", 0.0, 0.0);
    }
    if (failures)
        return 1;
    std::printf("ok\n");
    return 0;
}
