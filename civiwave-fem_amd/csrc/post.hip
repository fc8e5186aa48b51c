// post.hip -- derived fields on the device, bit-exact with src/post/derived_fields.cpp:139-211.
//
// Per element (derived_fields.cpp:157-186): strain from grad(N) . u in fp64 (the reference's
// per-corner statement order, shear pairs summed before they are added), stress = D strain as the
// full row fold (structural zeros of an isotropic D skipped, exact -- see parity_common.hpp),
// von Mises from the fp64 stress, all stored as f32 {strain[6], stress[6], vm} (the 52-B layout of
// cwf::post::ElementField).
// Per node (derived_fields.cpp:188-210): the reference scatters V*strain, V*stress and V into fp64
// accumulators in ascending element order; one thread per node gathers its ascending CSR from +0.0
// (the same fold order), recomputing each incident element's fp64 strain/stress (bitwise the values
// the element pass produced), then divides by the volume weight and re-evaluates von Mises from the
// averaged stress. This TU inherits -ffp-contract=off and IEEE fp64 div/sqrt from the Makefile.
#include "cwf_internal.hpp"
#include "plasticity.hpp"
#include "soil_plasticity.hpp"

namespace cwf
{
namespace
{

constexpr int kBlock = 256;

struct ElemTensors
{
    double strain[6];
    double stress[6];
};

// derived_fields.cpp:164-180 + stiffness_mul :66-80 for element e (tet4: 4 local nodes). HEX (native
// hex8, SURVEY 8f4, parity unpinned): the same statement order over 8 corners with the element-centre
// gradients cwf_preprocess_hex8 stores in the 24 gradient slots, i.e. the centroid strain.
template <bool ISO, bool HEX = false>
__device__ __forceinline__ void element_tensors(const DevSys &s, const float *__restrict__ u, uint32_t e,
                                                ElemTensors &t)
{
    constexpr int K = HEX ? 8 : 4;
    uint32_t c[K];
    float g[3 * K];
    if constexpr (HEX)
    {
#pragma unroll
        for (int a = 0; a < 8; ++a)
            c[a] = s.hconn[8ull * e + a];
#pragma unroll
        for (int i = 0; i < 24; ++i)
            g[i] = s.hgrad[24ull * e + i];
    }
    else
    {
        const uint4 q0 = s.erec[4u * e + 0u];
        const uint4 g0 = s.erec[4u * e + 1u], g1 = s.erec[4u * e + 2u], g2 = s.erec[4u * e + 3u];
        const uint32_t cc[4] = {q0.x, q0.y, q0.z, q0.w};
        const float gg[12] = {__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z),
                              __uint_as_float(g0.w), __uint_as_float(g1.x), __uint_as_float(g1.y),
                              __uint_as_float(g1.z), __uint_as_float(g1.w), __uint_as_float(g2.x),
                              __uint_as_float(g2.y), __uint_as_float(g2.z), __uint_as_float(g2.w)};
#pragma unroll
        for (int a = 0; a < 4; ++a)
            c[a] = cc[a];
#pragma unroll
        for (int i = 0; i < 12; ++i)
            g[i] = gg[i];
    }
    double e6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < K; ++a)
    {
        const double ux = (double)u[3ull * c[a] + 0], uy = (double)u[3ull * c[a] + 1], uz = (double)u[3ull * c[a] + 2];
        const double gx = (double)g[3 * a], gy = (double)g[3 * a + 1], gz = (double)g[3 * a + 2];
        e6[0] += gx * ux;
        e6[1] += gy * uy;
        e6[2] += gz * uz;
        e6[3] += gy * ux + gx * uy;
        e6[4] += gz * uy + gy * uz;
        e6[5] += gz * ux + gx * uz;
    }
    const double *D = s.dmat + 36ull * s.mat[e];
#pragma unroll
    for (int r = 0; r < 6; ++r)
    {
        t.strain[r] = e6[r];
        double acc = 0.0;
        if constexpr (ISO)
        {
            if (r < 3)
            {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    acc += D[6 * r + k] * e6[k];
            }
            else
                acc += D[6 * r + r] * e6[r];
        }
        else
        {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                acc += D[6 * r + k] * e6[k];
        }
        t.stress[r] = acc;
    }
}

// von_mises (derived_fields.cpp:47-63): plasticity.hpp, shared with the host-side return map

// the 52-B element record {strain[6], stress[6], vm} of one element's tensors
__device__ __forceinline__ void store_element_record(float *__restrict__ o, const ElemTensors &t)
{
#pragma unroll
    for (int c = 0; c < 6; ++c)
    {
        o[c] = (float)t.strain[c];
        o[6 + c] = (float)t.stress[c];
    }
    o[12] = (float)von_mises(t.stress);
}

template <bool ISO, bool HEX>
__global__ __launch_bounds__(kBlock) void k_derived_elements(DevSys s, const float *__restrict__ u,
                                                             float *__restrict__ out)
{
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= s.E)
        return;
    ElemTensors t;
    element_tensors<ISO, HEX>(s, u, e, t);
    store_element_record(out + 13ull * e, t);
}

// Element monitors of the explicit stepper (include/cwf_hip.h "Element monitors"). They live here so that strain,
// stress and von Mises are the code above, under this file's flags.
//
// Gauges: one thread per gauge element, its derived-fields record into the sample's row [count][13].
template <bool ISO, bool HEX>
__global__ __launch_bounds__(kBlock) void k_explicit_gauges(DevSys s, const float *__restrict__ u, uint32_t count,
                                                            const uint32_t *__restrict__ elem, float *__restrict__ row)
{
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= count)
        return;
    ElemTensors t;
    element_tensors<ISO, HEX>(s, u, elem[r], t);
    store_element_record(row + 13ull * r, t);
}

// the effective shear strain 2 sqrt(J2) of the strain deviator (engineering shears), in the header's statement order
__device__ __forceinline__ double effective_shear_strain(const double e[6])
{
    const double d0 = e[0] - e[1], d1 = e[1] - e[2], d2 = e[2] - e[0];
    const double sd = d0 * d0 + d1 * d1 + d2 * d2;
    const double sg = e[3] * e[3] + e[4] * e[4] + e[5] * e[5];
    return sqrt(sd * (2.0 / 3.0) + sg);
}

// Envelopes: one thread per element. Every map is a plane of one f32 per element (the stress range: planes c and
// 6 + c hold min and max of component c, `stride` floats apart), so a wavefront reads and writes consecutive words.
// The maps' old values are loaded first, next to the element's records and its u gathers; a value is stored only
// where it replaces the old one. Which maps are active is uniform over the launch (NULL: not set).
template <bool ISO, bool HEX>
__global__ __launch_bounds__(kBlock) void k_explicit_envelope(DevSys s, const float *__restrict__ u,
                                                              float *__restrict__ vm, float *__restrict__ shear,
                                                              float *__restrict__ range, uint64_t stride)
{
    const uint32_t e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= s.E)
        return;
    float old_vm = 0.f, old_shear = 0.f, lo[6], hi[6];
    if (vm)
        old_vm = vm[e];
    if (shear)
        old_shear = shear[e];
    if (range)
    {
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            lo[c] = range[c * stride + e];
            hi[c] = range[(6 + c) * stride + e];
        }
    }
    ElemTensors t;
    element_tensors<ISO, HEX>(s, u, e, t);
    if (vm)
    {
        const float x = (float)von_mises(t.stress);
        if (x > old_vm)
            vm[e] = x;
    }
    if (shear)
    {
        const float x = (float)effective_shear_strain(t.strain);
        if (x > old_shear)
            shear[e] = x;
    }
    if (range)
    {
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            const float x = (float)t.stress[c];
            if (x < lo[c])
                range[c * stride + e] = x;
            if (x > hi[c])
                range[(6 + c) * stride + e] = x;
        }
    }
}

template <bool ISO, bool HEX>
__global__ __launch_bounds__(kBlock) void k_derived_nodes(DevSys s, const float *__restrict__ u, float *__restrict__ out)
{
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= s.N)
        return;
    double ws = 0.0, as[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, at[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t q = s.off[n]; q < s.off[n + 1]; ++q)
    {
        const uint32_t e = s.inc[q] >> (HEX ? 3 : 2);
        ElemTensors t;
        element_tensors<ISO, HEX>(s, u, e, t);
        const double vol = (double)s.vol[e];
        ws += vol;  // accumulate_node (derived_fields.cpp:82-95)
#pragma unroll
        for (int c = 0; c < 6; ++c)
        {
            as[c] += t.strain[c] * vol;
            at[c] += t.stress[c] * vol;
        }
    }
    float *o = out + 13ull * n;
    if (ws <= 0.0)  // finalize_node (derived_fields.cpp:110-134): isolated node -> zero field
    {
#pragma unroll
        for (int c = 0; c < 13; ++c)
            o[c] = 0.0f;
        return;
    }
    const double inv = 1.0 / ws;
    double avg[6];
#pragma unroll
    for (int c = 0; c < 6; ++c)
    {
        o[c] = (float)(as[c] * inv);
        avg[c] = at[c] * inv;
        o[6 + c] = (float)avg[c];
    }
    o[12] = (float)von_mises(avg);
}

// Plasticity of the explicit stepper (include/cwf_hip.h "Plasticity"). The element pass lives here so that the strain is
// element_tensors' statement order under this file's flags; the return map is plasticity.hpp's, the host's too.
//
struct alignas(4) P3  // a node's or a corner's three f32: one 12-B access
{
    float c[3];
};
// pack.cpp:41-57 safe_cast_double_to_float, as explicit.hip's
__device__ __forceinline__ float safe_cast(double v)
{
    const double fmax = 3.4028234663852886e38;  // FLT_MAX
    if (!isfinite(v))
        return v > 0.0 ? __int_as_float(0x7f800000) : v < 0.0 ? __int_as_float((int)0xff800000u) : __int_as_float(0x7fc00000);
    if (v > fmax)
        return 3.4028234663852886e38f;
    if (v < -fmax)
        return -3.4028234663852886e38f;
    return (float)v;
}

// One thread per slot (plastic element, ascending element index). Every load is issued before the first fp64
// operation: the slot's element, its 64-B record, material and volume, the 64-B state, then what depends on those (the
// four u gathers, the material's 12 D entries and its {sy, H}). The state is stored only where the element yielded.
// The corner forces are pushed: corner a's three floats go to position cpos[slot][a] of the node-major array, so the
// node pass reads each node's incidences as one contiguous run (four scattered 12-B stores here, which no lane waits
// for, instead of four scattered 12-B loads per slot there, which measured 9x their bytes in fetches). An element
// whose abar is still 0 stores nothing: its entries hold the +0.0 they were set to, and +0.0 is what its magnitude-0
// forces add to a sum that starts at +0.0.
__global__ __launch_bounds__(kBlock) void k_explicit_plastic_elements(DevSys s, const float *__restrict__ u,
                                                                      ExplicitPlasticity a)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= a.slots)
        return;
    const uint32_t e = a.elem[slot];
    const uint4 q0 = s.erec[4u * e + 0u];
    const uint4 g0 = s.erec[4u * e + 1u], g1 = s.erec[4u * e + 2u], g2 = s.erec[4u * e + 3u];
    const uint32_t m = s.mat[e];
    const float volf = s.vol[e];
    double2 *sp2 = reinterpret_cast<double2 *>(a.state + 8ull * slot);  // 64-B records in a hipMalloc'd array
    const double2 s0 = sp2[0], s1 = sp2[1], s2 = sp2[2], s3 = sp2[3];
    const uint4 cp = reinterpret_cast<const uint4 *>(a.cpos)[slot];
    const uint32_t c[4] = {q0.x, q0.y, q0.z, q0.w};
    float uf[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        uf[3 * k] = u[3ull * c[k] + 0];
        uf[3 * k + 1] = u[3ull * c[k] + 1];
        uf[3 * k + 2] = u[3ull * c[k] + 2];
    }
    const double *Dm = s.dmat + 36ull * m;
    double D[36];
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            D[6 * r + k] = Dm[6 * r + k];
        D[7 * (r + 3)] = Dm[7 * (r + 3)];
    }
    const double2 yh = reinterpret_cast<const double2 *>(a.yield_hard)[m];
    const float g[12] = {__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z), __uint_as_float(g0.w),
                         __uint_as_float(g1.x), __uint_as_float(g1.y), __uint_as_float(g1.z), __uint_as_float(g1.w),
                         __uint_as_float(g2.x), __uint_as_float(g2.y), __uint_as_float(g2.z), __uint_as_float(g2.w)};
    // element_tensors' strain
    double e6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const double ux = (double)uf[3 * k], uy = (double)uf[3 * k + 1], uz = (double)uf[3 * k + 2];
        const double gx = (double)g[3 * k], gy = (double)g[3 * k + 1], gz = (double)g[3 * k + 2];
        e6[0] += gx * ux;
        e6[1] += gy * uy;
        e6[2] += gz * uz;
        e6[3] += gy * ux + gx * uy;
        e6[4] += gz * uy + gy * uz;
        e6[5] += gz * ux + gx * uz;
    }
    double ep[6] = {s0.x, s0.y, s1.x, s1.y, s2.x, s2.y}, abar = s3.x, wp = s3.y, sp[6];
    const double V = (double)volf;
    if (j2_update(D, yh.x, yh.y, V, e6, ep, abar, wp, sp))
    {
        sp2[0] = make_double2(ep[0], ep[1]);
        sp2[1] = make_double2(ep[2], ep[3]);
        sp2[2] = make_double2(ep[4], ep[5]);
        sp2[3] = make_double2(abar, wp);
    }
    if (!(abar > 0.0))
        return;
    const uint32_t pos[4] = {cp.x, cp.y, cp.z, cp.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const double gx = (double)g[3 * k], gy = (double)g[3 * k + 1], gz = (double)g[3 * k + 2];
        P3 o;
        o.c[0] = safe_cast(V * ((gx * sp[0] + gy * sp[3]) + gz * sp[5]));
        o.c[1] = safe_cast(V * ((gy * sp[1] + gx * sp[3]) + gz * sp[4]));
        o.c[2] = safe_cast(V * ((gz * sp[2] + gy * sp[4]) + gx * sp[5]));
        *reinterpret_cast<P3 *>(a.corner + 3ull * pos[k]) = o;
    }
}

// Soil plasticity (include/cwf_hip.h "Soil plasticity"): k_explicit_plastic_elements with soil_plasticity.hpp's return
// map. The same loads in the same order, the material's {alpha, kappa, beta, H} as two 16-B loads where J2 reads
// {sy, H}, and with SIG0 the slot's stress at rest as three more (48-B records in a hipMalloc'd array, so 16-B
// aligned); a set without one runs the instantiation that reads nothing more than J2 does. State and corner forces
// are stored by J2's rules but for one case: the state where the element yielded, the corner forces where it yielded in
// this step or abar > 0 (an apex return from a stress without a deviator changes ep and leaves abar at 0).
template <bool SIG0>
__global__ __launch_bounds__(kBlock) void k_explicit_dp_elements(DevSys s, const float *__restrict__ u,
                                                                 ExplicitPlasticity a, ExplicitSoil soil)
{
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= a.slots)
        return;
    const uint32_t e = a.elem[slot];
    const uint4 q0 = s.erec[4u * e + 0u];
    const uint4 g0 = s.erec[4u * e + 1u], g1 = s.erec[4u * e + 2u], g2 = s.erec[4u * e + 3u];
    const uint32_t m = s.mat[e];
    const float volf = s.vol[e];
    double2 *sp2 = reinterpret_cast<double2 *>(a.state + 8ull * slot);
    const double2 s0 = sp2[0], s1 = sp2[1], s2 = sp2[2], s3 = sp2[3];
    const uint4 cp = reinterpret_cast<const uint4 *>(a.cpos)[slot];
    double2 z0 = make_double2(0.0, 0.0), z1 = z0, z2 = z0;
    if constexpr (SIG0)
    {
        const double2 *zp = reinterpret_cast<const double2 *>(soil.sig0 + 6ull * slot);
        z0 = zp[0];
        z1 = zp[1];
        z2 = zp[2];
    }
    const uint32_t c[4] = {q0.x, q0.y, q0.z, q0.w};
    float uf[12];
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        uf[3 * k] = u[3ull * c[k] + 0];
        uf[3 * k + 1] = u[3ull * c[k] + 1];
        uf[3 * k + 2] = u[3ull * c[k] + 2];
    }
    const double *Dm = s.dmat + 36ull * m;
    double D[36];
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            D[6 * r + k] = Dm[6 * r + k];
        D[7 * (r + 3)] = Dm[7 * (r + 3)];
    }
    const double2 ak = reinterpret_cast<const double2 *>(soil.params)[2ull * m];
    const double2 bh = reinterpret_cast<const double2 *>(soil.params)[2ull * m + 1];
    const float g[12] = {__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z), __uint_as_float(g0.w),
                         __uint_as_float(g1.x), __uint_as_float(g1.y), __uint_as_float(g1.z), __uint_as_float(g1.w),
                         __uint_as_float(g2.x), __uint_as_float(g2.y), __uint_as_float(g2.z), __uint_as_float(g2.w)};
    // element_tensors' strain
    double e6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const double ux = (double)uf[3 * k], uy = (double)uf[3 * k + 1], uz = (double)uf[3 * k + 2];
        const double gx = (double)g[3 * k], gy = (double)g[3 * k + 1], gz = (double)g[3 * k + 2];
        e6[0] += gx * ux;
        e6[1] += gy * uy;
        e6[2] += gz * uz;
        e6[3] += gy * ux + gx * uy;
        e6[4] += gz * uy + gy * uz;
        e6[5] += gz * ux + gx * uz;
    }
    double ep[6] = {s0.x, s0.y, s1.x, s1.y, s2.x, s2.y}, abar = s3.x, wp = s3.y, sp[6];
    const double par[4] = {ak.x, ak.y, bh.x, bh.y};
    const double sig0[6] = {z0.x, z0.y, z1.x, z1.y, z2.x, z2.y};
    const double V = (double)volf;
    const int branch = dp_update(D, par, SIG0 ? sig0 : nullptr, V, e6, ep, abar, wp, sp);
    if (branch)
    {
        sp2[0] = make_double2(ep[0], ep[1]);
        sp2[1] = make_double2(ep[2], ep[3]);
        sp2[2] = make_double2(ep[4], ep[5]);
        sp2[3] = make_double2(abar, wp);
    }
    // an apex return from a stress without a deviator changes ep and leaves abar at 0: that step pushes too
    if (!(branch || abar > 0.0))
        return;
    const uint32_t pos[4] = {cp.x, cp.y, cp.z, cp.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const double gx = (double)g[3 * k], gy = (double)g[3 * k + 1], gz = (double)g[3 * k + 2];
        P3 o;
        o.c[0] = safe_cast(V * ((gx * sp[0] + gy * sp[3]) + gz * sp[5]));
        o.c[1] = safe_cast(V * ((gy * sp[1] + gx * sp[3]) + gz * sp[4]));
        o.c[2] = safe_cast(V * ((gz * sp[2] + gy * sp[4]) + gx * sp[5]));
        *reinterpret_cast<P3 *>(a.corner + 3ull * pos[k]) = o;
    }
}

// One thread per affected node: its run of the node-major corner forces (ascending element, built at set time), each
// widened to double and added from +0.0 in that order, safe_cast, one 12-B store into the correction vector p the
// update pass reads. Consecutive nodes read consecutive runs. Rows of other nodes stay at the zero they were set to.
__global__ __launch_bounds__(kBlock) void k_explicit_plastic_nodes(ExplicitPlasticity a)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.affected)
        return;
    const uint32_t end = a.aoff[i + 1];
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (uint32_t j = a.aoff[i]; j < end; ++j)
    {
        const P3 c = *reinterpret_cast<const P3 *>(a.corner + 3ull * j);
        acc0 = acc0 + (double)c.c[0];
        acc1 = acc1 + (double)c.c[1];
        acc2 = acc2 + (double)c.c[2];
    }
    P3 o;
    o.c[0] = safe_cast(acc0);
    o.c[1] = safe_cast(acc1);
    o.c[2] = safe_cast(acc2);
    *reinterpret_cast<P3 *>(a.p + 3ull * a.anode[i]) = o;
}

// The node pass read cooperatively (the soil set's; J2 keeps the pass above). A wavefront owns 64 consecutive affected
// nodes, whose runs are one contiguous span of the corner array: its lanes copy the span into the wave's share of LDS
// as consecutive words, WORDS at a time (a multiple of 3, so no 12-B entry straddles two rounds; kCoopWords: 4 waves x
// 20,472 B = 81,888 B per workgroup, two workgroups in a CU's 160 KiB), and each lane then folds the part of its own
// run that the round holds, from +0.0 in ascending element order: the sums, and so the bits of p, are those of
// k_explicit_plastic_nodes. Only the wave's own lanes touch its share, and a wave's LDS accesses complete in order,
// so a wavefront-scope fence between the copy and the fold is all the ordering there is to keep.
// WORDS is a template parameter so that a test can run many short rounds on a small mesh (kCoopTestWords: a run of 24
// entries is 72 words, so most runs straddle a round's end and the accumulators are carried over).
constexpr uint32_t kCoopWords = 5118, kCoopTestWords = 96;
template <uint32_t WORDS>
__global__ __launch_bounds__(kBlock) void k_explicit_plastic_nodes_coop(ExplicitPlasticity a)
{
    static_assert(WORDS % 3u == 0u, "a round holds whole 12-B entries");
    __shared__ float lds[(kBlock / 64) * WORDS];
    float *mine = lds + (threadIdx.x / 64u) * WORDS;
    const uint32_t lane = threadIdx.x % 64u;
    const uint32_t first = (blockIdx.x * kBlock + threadIdx.x) - lane;  // the wave's first node
    if (first >= a.affected)
        return;
    const uint32_t i = first + lane;
    const bool live = i < a.affected;
    const uint32_t last = min(first + 63u, a.affected - 1u);
    const uint32_t w0 = 3u * a.aoff[first], w1 = 3u * a.aoff[last + 1u];
    const uint32_t my0 = live ? 3u * a.aoff[i] : w1, my1 = live ? 3u * a.aoff[i + 1u] : w1;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
    for (uint32_t base = w0; base < w1; base += WORDS)
    {
        const uint32_t n = min(WORDS, w1 - base);
        for (uint32_t k = lane; k < n; k += 64u)
            mine[k] = a.corner[base + k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t lo = max(my0, base), hi = min(my1, base + n);
        for (uint32_t j = lo; j < hi; j += 3u)
        {
            acc0 = acc0 + (double)mine[j - base];
            acc1 = acc1 + (double)mine[j - base + 1u];
            acc2 = acc2 + (double)mine[j - base + 2u];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (!live)
        return;
    P3 o;
    o.c[0] = safe_cast(acc0);
    o.c[1] = safe_cast(acc1);
    o.c[2] = safe_cast(acc2);
    *reinterpret_cast<P3 *>(a.p + 3ull * a.anode[i]) = o;
}

inline unsigned grid_for(uint64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

template <bool HEX>
void derived_fields_k(const DevSys &s, const float *u, float *elem_out, float *node_out, hipStream_t st)
{
    if (s.E && elem_out)
    {
        if (s.iso)
            k_derived_elements<true, HEX><<<grid_for(s.E), kBlock, 0, st>>>(s, u, elem_out);
        else
            k_derived_elements<false, HEX><<<grid_for(s.E), kBlock, 0, st>>>(s, u, elem_out);
    }
    if (s.N && node_out)
    {
        if (s.iso)
            k_derived_nodes<true, HEX><<<grid_for(s.N), kBlock, 0, st>>>(s, u, node_out);
        else
            k_derived_nodes<false, HEX><<<grid_for(s.N), kBlock, 0, st>>>(s, u, node_out);
    }
}

template <bool ISO, bool HEX>
void element_monitors_k(const DevSys &s, const float *u, const ExplicitElementPass &a, hipStream_t st)
{
    if (a.envelope)
        k_explicit_envelope<ISO, HEX><<<grid_for(s.E), kBlock, 0, st>>>(s, u, a.von_mises, a.shear_strain,
                                                                        a.stress_range, a.stride);
    if (a.gauge_row)
        k_explicit_gauges<ISO, HEX><<<grid_for(a.gauge_count), kBlock, 0, st>>>(s, u, a.gauge_count, a.gauge_elements,
                                                                                a.gauge_row);
}
}  // namespace

void explicit_element_monitors(const DevSys &s, const float *u, const ExplicitElementPass &a, hipStream_t st)
{
    if (!s.E || (!a.envelope && !a.gauge_row))
        return;
    if (s.hex)
        s.iso ? element_monitors_k<true, true>(s, u, a, st) : element_monitors_k<false, true>(s, u, a, st);
    else
        s.iso ? element_monitors_k<true, false>(s, u, a, st) : element_monitors_k<false, false>(s, u, a, st);
}

void explicit_plasticity(const DevSys &s, const float *u, const ExplicitPlasticity &a, hipStream_t st)
{
    if (!a.slots)
        return;
    k_explicit_plastic_elements<<<grid_for(a.slots), kBlock, 0, st>>>(s, u, a);
    k_explicit_plastic_nodes<<<grid_for(a.affected), kBlock, 0, st>>>(a);
}

void explicit_soil_plasticity(const DevSys &s, const float *u, const ExplicitPlasticity &a, const ExplicitSoil &soil,
                              int node_pass, hipStream_t st)
{
    if (!a.slots)
        return;
    if (soil.sig0)
        k_explicit_dp_elements<true><<<grid_for(a.slots), kBlock, 0, st>>>(s, u, a, soil);
    else
        k_explicit_dp_elements<false><<<grid_for(a.slots), kBlock, 0, st>>>(s, u, a, soil);
    if (node_pass == 2)
        k_explicit_plastic_nodes_coop<kCoopWords><<<grid_for(a.affected), kBlock, 0, st>>>(a);
    else if (node_pass == 3)
        k_explicit_plastic_nodes_coop<kCoopTestWords><<<grid_for(a.affected), kBlock, 0, st>>>(a);
    else
        k_explicit_plastic_nodes<<<grid_for(a.affected), kBlock, 0, st>>>(a);
}

void derived_fields(cwf_hip_system *h, const float *u, float *elem_out, float *node_out, hipStream_t st)
{
    if (h->ds.hex)
        derived_fields_k<true>(h->ds, u, elem_out, node_out, st);
    else
        derived_fields_k<false>(h->ds, u, elem_out, node_out, st);
}

}  // namespace cwf
