// modal.hpp -- what the modal analysis translation units share (modal.cpp: the subspace iteration and its C-ABI,
// modal.hip: the block kernels, modal_ritz.cpp: the host Rayleigh-Ritz step). modal_ritz.cpp and the declarations
// of its functions need no HIP header, so tests/cpp/modal_host_test.cpp can build them with the host compiler alone.
#pragma once

#include <cstdint>

namespace cwf
{

constexpr uint32_t kModalMaxBlock = 32;  // columns of a block (two 16-column MFMA tiles)
// k_block_gram cuts the rows into chunks of this many, whatever the grid or the device: one q x q fp64 partial per
// chunk, folded in ascending chunk order, so a Gram matrix's bits depend on its inputs alone
constexpr uint32_t kGramChunkRows = 4096;

// ---- modal_ritz.cpp (host, fp64, no LAPACK) ----
// Lower Cholesky factor of the symmetric positive definite A [n x n] row-major, in place (the strict upper triangle
// is zeroed). Returns 0, or j + 1 when pivot j is not positive.
int ritz_cholesky(double *A, uint32_t n);
// Cyclic Jacobi eigen-decomposition of the symmetric A [n x n] row-major: on return A's diagonal holds the
// eigenvalues (unsorted), V [n x n] row-major the eigenvectors in its columns. Returns the sweeps taken, or -1 when
// the off-diagonal did not vanish in 60 sweeps.
int ritz_jacobi(double *A, double *V, uint32_t n);
// The generalised problem Kr Q = Mr Q Theta for symmetric Kr and symmetric positive definite Mr [n x n] row-major:
// theta [n] ascending, Q [n x n] row-major with the eigenvectors in its columns, Q^T Mr Q = I. Mr is scaled to a
// unit diagonal first (the columns of a subspace-iteration block differ by orders of magnitude: x_j ~ 1 / theta_j),
// then factored: C = L^-1 D Kr D L^-T, Jacobi on C, Q = D L^-T V. Returns 0; j + 1 when the scaled Mr is not
// positive definite at pivot j (a rank-deficient block); -1 when Jacobi did not converge.
int ritz_solve(const double *Kr, const double *Mr, uint32_t n, double *theta, double *Q);

// start vector entry of (column, dof) on a free DOF: column 0 is all ones (it excites every mode a uniform load
// does), the others a fixed integer hash (splitmix64's finaliser) of the pair mapped to [-1, 1). No seed, time or
// address enters, so a handle's start block is the same on every run.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline float modal_start_value(uint32_t column, uint64_t dof)
{
    if (column == 0)
        return 1.0f;
    uint64_t z = ((uint64_t)column << 40) + dof + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(int32_t)(z >> 40) * (1.0f / 8388608.0f) - 1.0f;  // 24 bits -> [-1, 1), exact in f32
}


#if defined(__HIP__)
}  // namespace cwf
#include <hip/hip_runtime.h>
namespace cwf
{
// ---- modal.hip (device pointers throughout; mass == nullptr: W = I) ----
uint32_t modal_gram_chunks(uint32_t D);
// G [qa x qb] row-major = A^T W B; part: modal_gram_chunks(D) * qa * qb doubles of scratch
void modal_gram(const float *A, uint32_t qa, const float *B, uint32_t qb, uint32_t D, const float *mass,
                const uint32_t *mask, double *part, double *G, hipStream_t st);
// Xo = X Q (Q [q_in x q_out] row-major, device), MXo (nullable) = W Xo; out of place
void modal_rotate(const float *X, uint32_t q_in, const double *Q, uint32_t q_out, uint32_t D, const float *mass,
                  const uint32_t *mask, float *Xo, float *MXo, hipStream_t st);
void modal_start(float *X, uint32_t q, uint32_t D, const uint32_t *mask, hipStream_t st);
void modal_scale(float *dst, const float *src, double s, uint32_t D, hipStream_t st);
void modal_sign(float *X, uint32_t columns, uint32_t D, const uint32_t *perm, hipStream_t st);
#endif

}  // namespace cwf
