// modal.cpp -- modal analysis over the handle's own PCG (include/cwf_hip.h): the lowest eigenpairs of
// K phi = lambda M phi by subspace iteration with Rayleigh-Ritz (Bathe), and the public block Gram / rotation
// calls. The block lives in the handle's internal node numbering from start to finish: every column is directly a
// right-hand side or a solution of run_pcg, and only the returned modes cross into the caller's order, once.
#include <cmath>
#include <cstring>

#include "abi_internal.hpp"
#include "modal.hpp"

namespace cwf
{
namespace
{

constexpr size_t kQQ = (size_t)kModalMaxBlock * kModalMaxBlock;

template <class T> int regrow(cwf_hip_system *h, T **p, size_t count)
{
    h->mem.free(*p);
    *p = nullptr;
    return dalloc(h, p, count);
}

// three blocks of >= q columns, the fp64 scratch, and (weighted, renumbered handle, caller-order vectors) the mass and
// mask in the caller's order
int modal_workspace(cwf_hip_system *h, uint32_t q, bool caller_weights)
{
    const size_t D = h->ds.D;
    if (h->mo_cols < q)
    {
        h->mo_cols = 0;
        if (int st = regrow(h, &h->mo_blk, 3 * (size_t)q * D))
            return st;
        h->mo_cols = q;
    }
    if (!h->mo_f64)
        if (int st = dalloc(h, &h->mo_f64, ((size_t)modal_gram_chunks(h->ds.D) + 3) * kQQ))
            return st;
    if (caller_weights && h->perm && !h->mo_mass)
    {
        float *m = nullptr;
        uint32_t *k = nullptr;
        if (int st = dalloc(h, &m, h->ds.N))
            return st;
        if (int st = dalloc(h, &k, h->ds.N))
            return st;
        perm_scatter(h->perm, h->ds.mass, m, h->ds.N, 1, h->stream);
        // the mask words move as 4-B payloads (a copy kernel does no arithmetic on them)
        perm_scatter(h->perm, reinterpret_cast<const float *>(h->ds.mask), reinterpret_cast<float *>(k), h->ds.N, 1,
                     h->stream);
        HIPTRY(h, hipGetLastError());
        h->mo_mass = m;
        h->mo_mask = k;
    }
    return 0;
}

float *blk(cwf_hip_system *h, int i) { return h->mo_blk + (size_t)i * h->mo_cols * h->ds.D; }
double *gram_part(cwf_hip_system *h) { return h->mo_f64; }
double *gram_out(cwf_hip_system *h, int i) { return h->mo_f64 + ((size_t)modal_gram_chunks(h->ds.D) + i) * kQQ; }

struct ModalPlan
{
    uint32_t k, q, max_outer;
    double tol, sigma;
    bool kr_from_applies;
    cwf_pcg_settings pcg;
};

int modal_iterate(cwf_hip_system *h, const ModalPlan &mp, double *eigenvalues, float *modes_out, int kind,
                  cwf_modal_telemetry *tel)
{
    const uint32_t D = h->ds.D, q = mp.q;
    hipStream_t st = h->stream;
    if (int e = modal_workspace(h, q, false))
        return e;
    Stopwatch sw;
    if (!sw.make())
        return set_error(h, CWF_ERR_HIP, "hipEventCreate failed");
    float *X = blk(h, 0), *Xb = blk(h, 1), *Y = blk(h, 2);
    double *Kd = gram_out(h, 0), *Md = gram_out(h, 1), *Qd = gram_out(h, 2);
    const size_t qq = (size_t)q * q;
    std::vector<double> Kr(qq), Mr(qq), Q(qq, 0.0), theta(q, 0.0), prev(q, 0.0);

    // start block and its Y = M X: the rotation by the identity (later iterations get Y from their own rotation)
    sw.start(st);
    modal_start(Xb, q, D, h->ds.mask, st);
    for (uint32_t i = 0; i < q; ++i)
        Q[(size_t)i * q + i] = 1.0;
    HIPTRY(h, hipMemcpyAsync(Qd, Q.data(), qq * sizeof(double), hipMemcpyHostToDevice, st));
    modal_rotate(Xb, q, Qd, q, D, h->ds.mass, h->ds.mask, X, Y, st);
    // m1 = 1^T W 1, the mass on the free DOFs (start column 0 is all ones there): an M-orthonormal vector has an RMS
    // entry of about 1 / sqrt(m1)
    double m1 = 0.0;
    modal_gram(X, 1, X, 1, D, h->ds.mass, h->ds.mask, gram_part(h), Md, st);
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipMemcpyAsync(&m1, Md, sizeof(double), hipMemcpyDeviceToHost, st));
    sw.stop(st, &tel->block_ms);
    HIPTRY(h, hipStreamSynchronize(st));
    if (!(m1 > 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "no free DOF carries mass", "free_mass=" + std::to_string(m1));
    // Column scales. The Ritz step is invariant to the scale of a column, and the PCG's guards are absolute (the
    // reference's |p.Ap| < 1e-18 and |rho| < 1e-18): an M-orthonormal column's solve, x ~ phi / theta with an
    // energy of 1 / theta, would run into them as it converges. So Ritz vector j is carried as 2^e_j phi_j with
    // 2^e_j ~ theta_j sqrt(m1): its solve then has a solution of RMS ~ 1 and an energy of ~ theta_j m1. Powers of
    // two, so taking the scale off the returned modes is exact.
    std::vector<double> scale(q, 1.0);
    // The start block has no Ritz values yet: it takes one scale from the Rayleigh quotient rho of a hashed column
    // (one operator apply). rho lies far up the spectrum, so 2^e ~ rho sqrt(m1) over-scales the low modes the first
    // solves are dominated by, which only moves them further from the guards.
    {
        const float *probe = Xb + (size_t)(q > 1 ? 1 : 0) * D;
        double kx = 0.0, mx = 0.0;
        sw.start(st);
        HIPTRY(h, hipMemcpyAsync(h->tmp, probe, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice, st));
        keff_apply(h, h->tmp, h->Ap, st);
        modal_gram(h->tmp, 1, h->Ap, 1, D, nullptr, nullptr, gram_part(h), Kd, st);
        modal_gram(h->tmp, 1, h->tmp, 1, D, h->ds.mass, h->ds.mask, gram_part(h), Md, st);
        HIPTRY(h, hipGetLastError());
        HIPTRY(h, hipMemcpyAsync(&kx, Kd, sizeof(double), hipMemcpyDeviceToHost, st));
        HIPTRY(h, hipMemcpyAsync(&mx, Md, sizeof(double), hipMemcpyDeviceToHost, st));
        sw.stop(st, &tel->block_ms);
        HIPTRY(h, hipStreamSynchronize(st));
        const double want = kx / mx * std::sqrt(m1);
        if (want > 0.0 && std::isfinite(want))
        {
            const double s0 = std::exp2(std::round(std::log2(want)));
            for (uint32_t i = 0; i < q; ++i)
                Q[(size_t)i * q + i] = s0;
            sw.start(st);
            HIPTRY(h, hipMemcpyAsync(Qd, Q.data(), qq * sizeof(double), hipMemcpyHostToDevice, st));
            modal_rotate(Xb, q, Qd, q, D, h->ds.mass, h->ds.mask, X, Y, st);
            HIPTRY(h, hipGetLastError());
            sw.stop(st, &tel->block_ms);
        }
    }

    bool have_ritz = false;
    for (uint32_t outer = 1; outer <= mp.max_outer; ++outer)
    {
        tel->outer_iterations = outer;
        for (uint32_t j = 0; j < q; ++j)
        {
            cwf_pcg_settings set = mp.pcg;
            set.warm_start = have_ritz ? 1 : 0;
            sw.start(st);
            if (have_ritz)  // (K + sigma M) x_j ~ theta_j M x_j = theta_j y_j
                modal_scale(h->x, X + (size_t)j * D, 1.0 / theta[j], D, st);
            // through the handle's own rhs buffer, as cwf_hip_solve_pcg stages it: a column of the block starts
            // wherever j D floats fall, the solve's kernels see the allocation they always see
            HIPTRY(h, hipMemcpyAsync(h->rhs, Y + (size_t)j * D, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice,
                                     st));
            cwf_pcg_telemetry pt{};
            const int e = run_pcg(h, h->rhs, set, &pt);
            tel->pcg_iterations += pt.iterations;
            if (e)
            {
                h->ctx += (h->ctx.empty() ? "" : "\n") + std::string("outer=") + std::to_string(outer) +
                          "\ncolumn=" + std::to_string(j);
                return e;
            }
            HIPTRY(h, hipMemcpyAsync(Xb + (size_t)j * D, h->x, (size_t)D * sizeof(float), hipMemcpyDeviceToDevice,
                                     st));
            sw.stop(st, &tel->solve_ms);
        }
        if (mp.kr_from_applies)  // evaluation: Kr = Xb^T (K + sigma M) Xb with q operator applies into the X block
        {
            sw.start(st);
            for (uint32_t j = 0; j < q; ++j)
            {
                const size_t bytes = (size_t)D * sizeof(float);  // staged as cwf_hip_apply_keff stages: tmp -> Ap
                HIPTRY(h, hipMemcpyAsync(h->tmp, Xb + (size_t)j * D, bytes, hipMemcpyDeviceToDevice, st));
                keff_apply(h, h->tmp, h->Ap, st);
                HIPTRY(h, hipMemcpyAsync(X + (size_t)j * D, h->Ap, bytes, hipMemcpyDeviceToDevice, st));
            }
            HIPTRY(h, hipGetLastError());
            sw.stop(st, &tel->solve_ms);
        }
        sw.start(st);
        modal_gram(Xb, q, mp.kr_from_applies ? X : Y, q, D, nullptr, nullptr, gram_part(h), Kd, st);
        modal_gram(Xb, q, Xb, q, D, h->ds.mass, h->ds.mask, gram_part(h), Md, st);
        HIPTRY(h, hipGetLastError());
        HIPTRY(h, hipMemcpyAsync(Kr.data(), Kd, qq * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPTRY(h, hipMemcpyAsync(Mr.data(), Md, qq * sizeof(double), hipMemcpyDeviceToHost, st));
        sw.stop(st, &tel->block_ms);
        HIPTRY(h, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < q; ++i)
            for (uint32_t j = i + 1; j < q; ++j)
            {
                Kr[(size_t)i * q + j] = Kr[(size_t)j * q + i] = 0.5 * (Kr[(size_t)i * q + j] + Kr[(size_t)j * q + i]);
                // (a_i)(w a_j) and (a_j)(w a_i) round differently inside a diagonal tile
                Mr[(size_t)i * q + j] = Mr[(size_t)j * q + i] = 0.5 * (Mr[(size_t)i * q + j] + Mr[(size_t)j * q + i]);
            }
        prev = theta;
        const int rs = ritz_solve(Kr.data(), Mr.data(), q, theta.data(), Q.data());
        if (rs)
            return set_error(h, CWF_ERR_DENOM_ZERO,
                             rs > 0 ? "Ritz mass matrix is not positive definite" : "Ritz eigen-solve did not converge",
                             "outer=" + std::to_string(outer) + (rs > 0 ? "\npivot=" + std::to_string(rs - 1) : ""));
        for (uint32_t j = 0; j < q; ++j)
        {
            const double want = std::fabs(theta[j]) * std::sqrt(m1);
            scale[j] = want > 0.0 && std::isfinite(want) ? std::exp2(std::round(std::log2(want))) : 1.0;
            for (uint32_t i = 0; i < q; ++i)
                Q[(size_t)i * q + j] *= scale[j];
        }
        sw.start(st);
        HIPTRY(h, hipMemcpyAsync(Qd, Q.data(), qq * sizeof(double), hipMemcpyHostToDevice, st));
        modal_rotate(Xb, q, Qd, q, D, h->ds.mass, h->ds.mask, X, Y, st);
        HIPTRY(h, hipGetLastError());
        sw.stop(st, &tel->block_ms);
        double change = 0.0;
        for (uint32_t i = 0; i < mp.k; ++i)
            change = std::max(change, std::fabs(theta[i] - prev[i]) / std::fabs(theta[i]));
        const bool first = !have_ritz;
        have_ritz = true;
        if (!first)
        {
            tel->max_change = change;
            if (change <= mp.tol)
            {
                tel->converged = 1;
                break;
            }
        }
    }
    // The final rotation X -> the k returned modes, [q x k]: the column scales off (exact: powers of two) ...
    std::vector<double> Qf((size_t)q * mp.k, 0.0);
    for (uint32_t i = 0; i < mp.k; ++i)
        Qf[(size_t)i * mp.k + i] = 1.0 / scale[i];
    // ... or, on a FAST tet4 handle, one more Rayleigh-Ritz step over the converged block with the fp64 element
    // math of the PARITY operator (the handle holds its element records in every mode). The FAST operators are
    // approximations of K: the structured block's f32 stencil is stiff by 0.6 - 1.7e-6 in the lowest modes
    // (measured: the Rayleigh quotients of exact modes through cwf_hip_apply_keff), and the iteration converges
    // to that operator's eigenvalues. Kr = X^T (K X) with q exact-arithmetic applies gives the Ritz values of K
    // itself on the same subspace, whose error is second order in the subspace's. ritz_solve's Q makes X Q
    // M-orthonormal whatever the columns' scales.
    if (h->mode == CWF_MODE_FAST && !h->ds.hex && h->ds.E)
    {
        if (int e = parity_force_buffer(h))  // the PARITY K_eff's node tiles, built once per handle
            return e;
        sw.start(st);
        for (uint32_t j = 0; j < q; ++j)
        {
            const size_t bytes = (size_t)D * sizeof(float);
            HIPTRY(h, hipMemcpyAsync(h->tmp, X + (size_t)j * D, bytes, hipMemcpyDeviceToDevice, st));
            parity_keff(h, h->tmp, h->Ap, true, nullptr, st);
            HIPTRY(h, hipMemcpyAsync(Xb + (size_t)j * D, h->Ap, bytes, hipMemcpyDeviceToDevice, st));
        }
        HIPTRY(h, hipGetLastError());
        sw.stop(st, &tel->solve_ms);
        sw.start(st);
        modal_gram(X, q, Xb, q, D, nullptr, nullptr, gram_part(h), Kd, st);
        modal_gram(X, q, X, q, D, h->ds.mass, h->ds.mask, gram_part(h), Md, st);
        HIPTRY(h, hipGetLastError());
        HIPTRY(h, hipMemcpyAsync(Kr.data(), Kd, qq * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPTRY(h, hipMemcpyAsync(Mr.data(), Md, qq * sizeof(double), hipMemcpyDeviceToHost, st));
        sw.stop(st, &tel->block_ms);
        HIPTRY(h, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < q; ++i)
            for (uint32_t j = i + 1; j < q; ++j)
            {
                Kr[(size_t)i * q + j] = Kr[(size_t)j * q + i] = 0.5 * (Kr[(size_t)i * q + j] + Kr[(size_t)j * q + i]);
                Mr[(size_t)i * q + j] = Mr[(size_t)j * q + i] = 0.5 * (Mr[(size_t)i * q + j] + Mr[(size_t)j * q + i]);
            }
        const int rs = ritz_solve(Kr.data(), Mr.data(), q, theta.data(), Q.data());
        if (rs)
            return set_error(h, CWF_ERR_DENOM_ZERO,
                             rs > 0 ? "Ritz mass matrix is not positive definite" : "Ritz eigen-solve did not converge",
                             "outer=final" + (rs > 0 ? "\npivot=" + std::to_string(rs - 1) : std::string()));
        for (uint32_t i = 0; i < q; ++i)
            for (uint32_t o = 0; o < mp.k; ++o)
                Qf[(size_t)i * mp.k + o] = Q[(size_t)i * q + o];
    }
    for (uint32_t i = 0; i < mp.k; ++i)
        eigenvalues[i] = theta[i] - mp.sigma;
    if (modes_out)
    {
        // the k modes, signed, then into the caller's order
        sw.start(st);
        HIPTRY(h, hipMemcpyAsync(Qd, Qf.data(), Qf.size() * sizeof(double), hipMemcpyHostToDevice, st));
        modal_rotate(X, q, Qd, mp.k, D, nullptr, nullptr, Xb, nullptr, st);
        modal_sign(Xb, mp.k, D, h->perm, st);
        HIPTRY(h, hipGetLastError());
        sw.stop(st, &tel->block_ms);
        for (uint32_t i = 0; i < mp.k; ++i)
            if (int e = vec_out(h, Xb + (size_t)i * D, modes_out + (size_t)i * D, kind, 3))
                return e;
    }
    HIPTRY(h, hipStreamSynchronize(st));
    return 0;
}

int check_block(cwf_hip_system *h, uint32_t q, const char *name)
{
    if (q == 0 || q > kModalMaxBlock)
        return set_error(h, CWF_ERR_ARGUMENT, std::string(name) + " must be in [1, 32]",
                         std::string(name) + "=" + std::to_string(q));
    return 0;
}

}  // namespace
}  // namespace cwf

using namespace cwf;

extern "C" {

int cwf_hip_modal_solve(cwf_hip_system *h, const cwf_modal_settings *s, double *eigenvalues, float *modes_out,
                        int kind, cwf_modal_telemetry *tel)
{
    if (int st = check_ready(h))
        return st;
    cwf_modal_telemetry local{};
    if (tel)
        std::memset(tel, 0, sizeof *tel);
    else
        tel = &local;
    if (!s)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", "settings");
    if (s->modes == 0)
        return set_error(h, CWF_ERR_ARGUMENT, "modes must be >= 1", "modes=0");
    if (!eigenvalues)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", "eigenvalues");
    if (h->sharded())
        return set_error(h, CWF_ERR_UNSUPPORTED, "modal analysis of a sharded handle is not supported",
                         "ranks=" + std::to_string(h->nranks));
    ModalPlan mp{};
    mp.k = s->modes;
    // min(2 k, k + 8) without overflow for a huge `modes`
    mp.q = s->block ? s->block : (mp.k <= 8 ? 2 * mp.k : (mp.k <= kModalMaxBlock ? mp.k + 8 : mp.k));
    if (!s->block && mp.q > kModalMaxBlock && mp.k <= kModalMaxBlock)
        mp.q = kModalMaxBlock;
    if (mp.q < mp.k)
        return set_error(h, CWF_ERR_ARGUMENT, "block must be >= modes",
                         "block=" + std::to_string(mp.q) + "\nmodes=" + std::to_string(mp.k));
    if (mp.q > kModalMaxBlock)
        return set_error(h, CWF_ERR_ARGUMENT, "block must be <= 32",
                         "block=" + std::to_string(mp.q) + "\nmodes=" + std::to_string(mp.k));
    if (!(s->shift >= 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "shift must be >= 0", "shift=" + std::to_string(s->shift));
    if (!(s->tolerance >= 0.0))
        return set_error(h, CWF_ERR_ARGUMENT, "tolerance must be >= 0", "tolerance=" + std::to_string(s->tolerance));
    if (h->ds.D < mp.q)
        return set_error(h, CWF_ERR_ARGUMENT, "block exceeds the DOF count",
                         "block=" + std::to_string(mp.q) + "\ndofs=" + std::to_string(h->ds.D));
    mp.max_outer = s->max_outer ? s->max_outer : 40;
    mp.tol = s->tolerance > 0.0 ? s->tolerance : 1e-6;
    mp.sigma = s->shift;
    mp.kr_from_applies = (s->reserved & 1u) != 0;
    mp.pcg = s->pcg;
    if (!(mp.pcg.relative_tolerance > 0.0))
        mp.pcg.relative_tolerance = 1e-6;
    if (mp.pcg.max_iterations == 0)
        mp.pcg.max_iterations = 20000;
    tel->block = mp.q;
    // the operator of the iteration is K + sigma M; the caller's scalars return on every path out of modal_iterate
    const ScalarScope modal_scalars(h, 1.0, mp.sigma);
    try
    {
        return modal_iterate(h, mp, eigenvalues, modes_out, kind, tel);
    }
    catch (const std::bad_alloc &)
    {
        return set_error(h, CWF_ERR_ALLOC, "host allocation failed");
    }
}

int cwf_hip_block_gram(cwf_hip_system *h, const float *A, uint32_t qa, const float *B, uint32_t qb, int mass_weighted,
                       double *G, int kind)
{
    if (int st = check_ready(h))
        return st;
    if (!A || !B || !G)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", !A ? "A" : !B ? "B" : "G");
    if (int st = check_block(h, qa, "qa"))
        return st;
    if (int st = check_block(h, qb, "qb"))
        return st;
    const uint32_t D = h->ds.D;
    const bool host = kind != CWF_PTR_DEVICE;
    if (int st = modal_workspace(h, host ? std::max(qa, qb) : 1u, mass_weighted != 0))
        return st;
    const float *dA = A, *dB = B;
    if (host)
    {
        HIPTRY(h, hipMemcpyAsync(blk(h, 0), A, (size_t)qa * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        dA = blk(h, 0);
        dB = dA;
        if (B != A || qb != qa)
        {
            HIPTRY(h, hipMemcpyAsync(blk(h, 1), B, (size_t)qb * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
            dB = blk(h, 1);
        }
    }
    const float *mass = !mass_weighted ? nullptr : h->perm ? h->mo_mass : h->ds.mass;
    const uint32_t *mask = !mass_weighted ? nullptr : h->perm ? h->mo_mask : h->ds.mask;
    modal_gram(dA, qa, dB, qb, D, mass, mask, gram_part(h), gram_out(h, 0), h->stream);
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipMemcpyAsync(G, gram_out(h, 0), (size_t)qa * qb * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_block_rotate(cwf_hip_system *h, const float *X, uint32_t q_in, const double *Q, uint32_t q_out, float *X_out,
                         float *MX_out, int kind)
{
    if (int st = check_ready(h))
        return st;
    if (!X || !Q || !X_out)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer", !X ? "X" : !Q ? "Q" : "X_out");
    if (int st = check_block(h, q_in, "q_in"))
        return st;
    if (int st = check_block(h, q_out, "q_out"))
        return st;
    if (X == X_out || X == MX_out)
        return set_error(h, CWF_ERR_ARGUMENT, "block rotation is out of place", "X_out or MX_out aliases X");
    const uint32_t D = h->ds.D;
    const bool host = kind != CWF_PTR_DEVICE;
    if (int st = modal_workspace(h, host ? std::max(q_in, q_out) : 1u, MX_out != nullptr))
        return st;
    const float *dX = X;
    float *dXo = X_out, *dMo = MX_out;
    if (host)
    {
        HIPTRY(h, hipMemcpyAsync(blk(h, 0), X, (size_t)q_in * D * sizeof(float), hipMemcpyHostToDevice, h->stream));
        dX = blk(h, 0);
        dXo = blk(h, 1);
        dMo = MX_out ? blk(h, 2) : nullptr;
    }
    double *Qd = gram_out(h, 2);
    HIPTRY(h, hipMemcpyAsync(Qd, Q, (size_t)q_in * q_out * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const float *mass = h->perm ? h->mo_mass : h->ds.mass;
    const uint32_t *mask = h->perm ? h->mo_mask : h->ds.mask;
    modal_rotate(dX, q_in, Qd, q_out, D, mass, mask, dXo, dMo, h->stream);
    HIPTRY(h, hipGetLastError());
    if (host)
    {
        HIPTRY(h, hipMemcpyAsync(X_out, dXo, (size_t)q_out * D * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        if (MX_out)
            HIPTRY(h, hipMemcpyAsync(MX_out, dMo, (size_t)q_out * D * sizeof(float), hipMemcpyDeviceToHost,
                                     h->stream));
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
