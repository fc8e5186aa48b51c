// tiles_groups.hip -- k_keff_groups_pipe: the FAST K_eff element pass over fan groups (groups.cpp; the default path
// of a tet mesh).
//
// Persistent, XCD-aware, software-pipelined like k_keff_tiles_pipe, over tiles of <= NT fan groups (one per
// lane) and <= 2 NT nodes (two per lane). A lane loads its group's <= 8 nodes {x y z v_x}{v_y v_z} from LDS,
// runs the group's f <= 6 tets {a, b, r_i, r_(i+1) mod 6} in packed fp32 (v_pk_fma_f32: tets i and i + 3 of
// the fan side by side, so a closed Kuhn fan is three packed tet pairs), sums the forces per node in
// registers and pushes one force per node to its position in the tile's local CSR (the node's run start,
// kept in LDS, plus the group's 4-bit rank in the run from the 16-B record); the node fold, partial stores,
// p.Ap share and owner p store are those of k_keff_tiles_pipe (spmv_tiles.hip).
#include "fast_common.hpp"

namespace cwf
{
namespace
{
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 splat(float v) { return f2{v, v}; }

struct GroupNext
{
    uint2 tn[2];          // records of tile nodes threadIdx.x, threadIdx.x + NT
    uint32_t slot[2];     // their node-major partial slots
    float c[2][3];        // their tile-relative coordinates
    float v[2][3], w[2][3], m[2];  // x / p_old, z and lumped mass at them
    uint4 g;              // record of group threadIdx.x
};

template <int NT>
__device__ __forceinline__ void group_issue_records(const DevSys &s, uint4 hd, GroupNext &n)
{
    const DevTiles &T = s.t;
    const uint32_t g0 = hd.x, ng = hd.y, nb = hd.z, nn = hd.w;
    const uint32_t T3 = T.total_tile_nodes;
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
        const uint32_t i = threadIdx.x + k * (uint32_t)NT;
        const uint32_t q = nb + (i < nn ? i : 0u);
        n.tn[k] = i < nn ? T.tnode[q] : uint2{0u, 0u};
        n.slot[k] = T.tslot[q];
        n.c[k][0] = T.tcoord[q];
        n.c[k][1] = T.tcoord[T3 + q];
        n.c[k][2] = T.tcoord[2 * T3 + q];
    }
    n.g = T.grec[g0 + (threadIdx.x < ng ? threadIdx.x : 0u)];
}

template <bool SANITIZE, int MODE>
__device__ __forceinline__ void group_issue_gather(const DevSys &s, const float *__restrict__ x,
                                                   const float *__restrict__ z, GroupNext &n)
{
    const __amdgpu_buffer_rsrc_t rx = whole_rsrc(x);
#pragma unroll
    for (int k = 0; k < 2; ++k)
    {
        const uint32_t g = n.tn[k].x & 0x7fffffffu;  // node 0 for idle lanes (harmless, in range)
        n.m[k] = 0.f;
        load3(rx, g, n.v[k]);
        if constexpr (MODE == 1)
        {
            load3(whole_rsrc(z), g, n.w[k]);
            n.m[k] = s.mass[g];
        }
        else if constexpr (SANITIZE)
        {
            const uint32_t mk = s.mask[g];
            n.v[k][0] = (mk & 1u) ? 0.f : n.v[k][0];
            n.v[k][1] = (mk & 2u) ? 0.f : n.v[k][1];
            n.v[k][2] = (mk & 4u) ? 0.f : n.v[k][2];
        }
    }
}

// Ring nodes k and k + 3 side by side: edge vectors d from a, values du relative to a's, w = e x d.
struct RingPair
{
    f2 d[3], du[3], w[3];
};

__device__ __forceinline__ RingPair ring_pair(const float4 *sxp, const float2 *sq, uint32_t l0, uint32_t l1,
                                              const float xa[3], const float ua[3], const float e[3])
{
    const float4 X0 = sxp[l0], X1 = sxp[l1];
    const float2 Q0 = sq[l0], Q1 = sq[l1];
    RingPair P;
    P.d[0] = f2{X0.x - xa[0], X1.x - xa[0]};
    P.d[1] = f2{X0.y - xa[1], X1.y - xa[1]};
    P.d[2] = f2{X0.z - xa[2], X1.z - xa[2]};
    P.du[0] = f2{X0.w - ua[0], X1.w - ua[0]};
    P.du[1] = f2{Q0.x - ua[1], Q1.x - ua[1]};
    P.du[2] = f2{Q0.y - ua[2], Q1.y - ua[2]};
    P.w[0] = pk_fma(splat(e[1]), P.d[2], -(splat(e[2]) * P.d[1]));
    P.w[1] = pk_fma(splat(e[2]), P.d[0], -(splat(e[0]) * P.d[2]));
    P.w[2] = pk_fma(splat(e[0]), P.d[1], -(splat(e[1]) * P.d[0]));
    return P;
}

__device__ __forceinline__ RingPair swap_pair(const RingPair &P)
{
    RingPair S;
#pragma unroll
    for (int q = 0; q < 3; ++q)
    {
        S.d[q] = P.d[q].yx;
        S.du[q] = P.du[q].yx;
        S.w[q] = P.w[q].yx;
    }
    return S;
}

// F += B(g)^T sig (g the corner's unscaled gradient, sig the scaled stress), packed over a tet pair
__device__ __forceinline__ void corner_acc(const f2 g[3], const f2 sig[6], f2 F[3])
{
    F[0] = pk_fma(g[2], sig[5], pk_fma(g[1], sig[3], pk_fma(g[0], sig[0], F[0])));
    F[1] = pk_fma(g[2], sig[4], pk_fma(g[0], sig[3], pk_fma(g[1], sig[1], F[1])));
    F[2] = pk_fma(g[0], sig[5], pk_fma(g[1], sig[4], pk_fma(g[2], sig[2], F[2])));
}

// Tets i (.x) and i + 3 (.y) of the fan: corners {a, b, r_i, r_j} with ring pairs I = (r_i, r_(i+3)) and
// J = (r_j, r_(j+3)), j = i + 1. With e = x_b - x_a, d_k = x_(r_k) - x_a and w_k = e x d_k, the cofactor rows
// (unscaled gradients) of corners b, r_i, r_j are d_i x d_j, -w_j and w_i, corner a's minus their sum, so
// the strain is sum over {b, r_i, r_j} of B(g_k) (u_k - u_a). The stress carries s_K / (6 |det|), masked to 0
// in a half whose tet does not exist. Forces accumulate on b (Fb), r_i (Fi) and r_j (Fj); corner a's is
// minus the group's other forces (partition of unity), formed once per group.
template <bool ISO>
__device__ __forceinline__ void tet_pair(const RingPair &I, const RingPair &J, const float e[3], const float db[3],
                                         const float *Dm, float sK6, bool vx, bool vy, f2 Fb[3], f2 Fi[3], f2 Fj[3])
{
    f2 g1[3];
    g1[0] = pk_fma(I.d[1], J.d[2], -(I.d[2] * J.d[1]));
    g1[1] = pk_fma(I.d[2], J.d[0], -(I.d[0] * J.d[2]));
    g1[2] = pk_fma(I.d[0], J.d[1], -(I.d[1] * J.d[0]));
    const f2 det = pk_fma(splat(e[0]), g1[0], pk_fma(splat(e[1]), g1[1], splat(e[2]) * g1[2]));
    f2 sc = {sK6 * __builtin_amdgcn_rcpf(fabsf(det.x)), sK6 * __builtin_amdgcn_rcpf(fabsf(det.y))};
    sc.x = vx ? sc.x : 0.f;
    sc.y = vy ? sc.y : 0.f;
    const f2 db0 = splat(db[0]), db1 = splat(db[1]), db2 = splat(db[2]);
    f2 eps[6];
    eps[0] = pk_fma(-J.w[0], I.du[0], pk_fma(I.w[0], J.du[0], g1[0] * db0));
    eps[1] = pk_fma(-J.w[1], I.du[1], pk_fma(I.w[1], J.du[1], g1[1] * db1));
    eps[2] = pk_fma(-J.w[2], I.du[2], pk_fma(I.w[2], J.du[2], g1[2] * db2));
    eps[3] = pk_fma(g1[0], db1, g1[1] * db0);
    eps[3] = pk_fma(I.w[0], J.du[1], pk_fma(I.w[1], J.du[0], eps[3]));
    eps[3] = pk_fma(-J.w[0], I.du[1], pk_fma(-J.w[1], I.du[0], eps[3]));
    eps[4] = pk_fma(g1[1], db2, g1[2] * db1);
    eps[4] = pk_fma(I.w[1], J.du[2], pk_fma(I.w[2], J.du[1], eps[4]));
    eps[4] = pk_fma(-J.w[1], I.du[2], pk_fma(-J.w[2], I.du[1], eps[4]));
    eps[5] = pk_fma(g1[0], db2, g1[2] * db0);
    eps[5] = pk_fma(I.w[0], J.du[2], pk_fma(I.w[2], J.du[0], eps[5]));
    eps[5] = pk_fma(-J.w[0], I.du[2], pk_fma(-J.w[2], I.du[0], eps[5]));
#pragma unroll
    for (int r = 0; r < 6; ++r)
        eps[r] *= sc;
    f2 sig[6];
    if constexpr (ISO)
    {
#pragma unroll
        for (int r = 0; r < 3; ++r)
            sig[r] = pk_fma(splat(Dm[3 * r + 2]), eps[2], pk_fma(splat(Dm[3 * r + 1]), eps[1], splat(Dm[3 * r]) * eps[0]));
#pragma unroll
        for (int r = 3; r < 6; ++r)
            sig[r] = splat(Dm[6 + r]) * eps[r];
    }
    else
    {
#pragma unroll
        for (int r = 0; r < 6; ++r)
        {
            f2 acc = splat(Dm[6 * r]) * eps[0];
#pragma unroll
            for (int c = 1; c < 6; ++c)
                acc = pk_fma(splat(Dm[6 * r + c]), eps[c], acc);
            sig[r] = acc;
        }
    }
    const f2 mwj[3] = {-J.w[0], -J.w[1], -J.w[2]};
    corner_acc(g1, sig, Fb);
    corner_acc(mwj, sig, Fi);
    corner_acc(I.w, sig, Fj);
}

// One fan group around edge (a, b). Record g: slot s (0 = a, 1 = b, 2 + k = ring node k) has the 9-bit local
// id s % 3 of word s / 3 and rank nibble s of g.w; f = g.x >> 27 tets {a, b, r_i, r_(i+1)}, i < f (ring slot 6
// is ring slot 0: a closed 6-fan; a closed fan of f < 6 repeats r_0 in ring slot f). Used slots: a, b and
// ring slots 0 .. min(f + 1, 6) - 1.
template <bool ISO>
__device__ __forceinline__ void group_forces(uint4 g, const float4 *sxp, const float2 *sq, const uint16_t *sst,
                                             float sK6, const float *Dm, float2 *sfxy, float *sfz)
{
    const auto lid = [&](int k) { return ((k < 3 ? g.x : k < 6 ? g.y : g.z) >> (9 * (k % 3))) & 0x1ffu; };
    const auto push = [&](int k, float fx, float fy, float fz) {
        const uint32_t l = lid(k);
        const uint32_t q = (uint32_t)sst[l] + ((g.w >> (4 * k)) & 15u);
        sfxy[q] = float2{fx, fy};
        sfz[q] = fz;
    };
    const int f = (int)((g.x >> 27) & 7u);
    const float4 Xa = sxp[lid(0)], Xb = sxp[lid(1)];
    const float2 Qa = sq[lid(0)], Qb = sq[lid(1)];
    const float xa[3] = {Xa.x, Xa.y, Xa.z};
    const float ua[3] = {Xa.w, Qa.x, Qa.y};
    const float e[3] = {Xb.x - Xa.x, Xb.y - Xa.y, Xb.z - Xa.z};
    const float db[3] = {Xb.w - ua[0], Qb.x - ua[1], Qb.y - ua[2]};
    const RingPair P0 = ring_pair(sxp, sq, lid(2), lid(5), xa, ua, e);
    const RingPair P1 = ring_pair(sxp, sq, lid(3), lid(6), xa, ua, e);
    f2 Fb[3] = {}, F0[3] = {}, F1[3] = {}, F2[3] = {}, F3[3] = {};
    // pair 0: tets 0, 3 (ring pairs 0, 1)
    tet_pair<ISO>(P0, P1, e, db, Dm, sK6, f > 0, f > 3, Fb, F0, F1);
    const RingPair P2 = ring_pair(sxp, sq, lid(4), lid(7), xa, ua, e);
    // pair 1: tets 1, 4 (ring pairs 1, 2); ring nodes 1 and 4 are complete after it
    tet_pair<ISO>(P1, P2, e, db, Dm, sK6, f > 1, f > 4, Fb, F1, F2);
    push(3, F1[0].x, F1[1].x, F1[2].x);
    if (f >= 4)
        push(6, F1[0].y, F1[1].y, F1[2].y);
    // pair 2: tets 2, 5 (ring pairs 2, 3 = ring pair 0 swapped: ring slot 6 is ring slot 0)
    tet_pair<ISO>(P2, swap_pair(P0), e, db, Dm, sK6, f > 2, f > 5, Fb, F2, F3);
    if (f >= 2)
        push(4, F2[0].x, F2[1].x, F2[2].x);
    if (f >= 5)
        push(7, F2[0].y, F2[1].y, F2[2].y);
    // ring node 0 = F0.x + F3.y, ring node 3 = F0.y + F3.x; a = -(everything else)
    float r0[3], r3[3], fb[3], fa[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
    {
        r0[q] = F0[q].x + F3[q].y;
        r3[q] = F0[q].y + F3[q].x;
        fb[q] = Fb[q].x + Fb[q].y;
        const f2 s12 = F1[q] + F2[q];
        fa[q] = -(((fb[q] + r0[q]) + r3[q]) + (s12.x + s12.y));
    }
    push(2, r0[0], r0[1], r0[2]);
    if (f >= 3)
        push(5, r3[0], r3[1], r3[2]);
    push(0, fa[0], fa[1], fa[2]);
    push(1, fb[0], fb[1], fb[2]);
}

// MONO: one material, D from the kernel arguments (SGPR operands); otherwise the group's material selects
// a row of the LDS table (<= 16 materials, abi.cpp)
template <bool ISO, bool SANITIZE, int MODE, int NT, bool MONO>
__global__ __launch_bounds__(NT, kGroupWavesPerSimd) void k_keff_groups_pipe(DevSys s, const float *__restrict__ x, PcgArgs pa,
                                                         const uint4 *__restrict__ hdr)
{
    constexpr int kTab = ISO ? 12 : 36;
    constexpr int SP = (int)kGroupSlotsPerLane * NT, MS = 2 * NT;
    extern __shared__ float lds[];
    const DevTiles &T = s.t;
    float2 *sfxy = reinterpret_cast<float2 *>(lds);           // [SP]
    float *sfz = lds + 2 * SP;                                // [SP]
    float4 *sxp = reinterpret_cast<float4 *>(lds + 3 * SP);  // [MS] {x, y, z, v_x}
    float2 *sq = reinterpret_cast<float2 *>(sxp + MS);       // [MS] {v_y, v_z}
    uint16_t *sst = reinterpret_cast<uint16_t *>(sq + MS);   // [MS] run start in the local CSR
    __shared__ float dtab[MONO ? 1 : kMaxM * kTab];
    __shared__ double red[2 * (NT / 64)];
    const TileRange tr = xcd_tile_range(T.ntiles);
    const uint32_t nbx = tr.nbx, t_end = tr.t_end;
    uint32_t t = tr.t;
    GroupNext cur;
    // the control flag and the first two tile headers: scalar loads issued together, one round trip (the flag was
    // a round trip of its own in front of the headers)
    const int active = MODE == 1 ? pa.ctl->active : 1;
    uint4 hd = t < t_end ? hdr[t] : uint4{0u, 0u, 0u, 0u};
    uint4 hd2 = t + nbx < t_end ? hdr[t + nbx] : uint4{0u, 0u, 0u, 0u};
    if (!active)
        return;
    if (t < t_end)
    {
        group_issue_records<NT>(s, hd, cur);
        group_issue_gather<SANITIZE, MODE>(s, x, pa.z, cur);
    }
    if constexpr (!MONO)
    {
        const uint32_t nm = s.M < kMaxM ? s.M : kMaxM;
        for (uint32_t i = threadIdx.x; i < nm * kTab; i += NT)
            dtab[i] = (float)s.dmat[36u * (i / kTab) + dsrc(ISO, i % kTab)];
    }
    float beta = 0.f;
    if constexpr (MODE == 1)
    {
        if (!residual_step<NT, 8>(pa.ctl, pa.prr, pa.prz, pa.nupd, pa.stride, pa.it, pa.hist, red, &beta, pa.abl & 32u))
            return;
    }
    const float sK6 = (float)(s.sK / 6.0), sM = (float)s.sM;
    double pap = 0.0;
    for (; t < t_end; t += nbx)
    {
        const uint32_t ng = hd.y, nn = hd.w;
        // (a) LDS fill of tile t's nodes (two per lane) from the prefetched registers
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            const uint32_t i = threadIdx.x + k * NT;
            if (i < nn)
            {
                float v0 = cur.v[k][0], v1 = cur.v[k][1], v2 = cur.v[k][2];
                if constexpr (MODE == 1)
                {
                    v0 = fmaf(beta, v0, cur.w[k][0]);
                    v1 = fmaf(beta, v1, cur.w[k][1]);
                    v2 = fmaf(beta, v2, cur.w[k][2]);
                }
                sxp[i] = float4{cur.c[k][0], cur.c[k][1], cur.c[k][2], v0};
                sq[i] = float2{v1, v2};
                sst[i] = (uint16_t)(cur.tn[k].y & 0xffffu);
            }
        }
        const uint4 gr = cur.g;
        const uint2 tn_own[2] = {cur.tn[0], cur.tn[1]};
        const uint32_t slot_own[2] = {cur.slot[0], cur.slot[1]};
        const float m_own[2] = {cur.m[0], cur.m[1]};
        __syncthreads();
        // (b) next tile's records in flight during this tile's group and fold work
        const uint32_t tn_next = t + nbx;
        const uint4 hdn = hd2;
        if (tn_next < t_end)
            group_issue_records<NT>(s, hdn, cur);
        hd2 = tn_next + nbx < t_end ? hdr[tn_next + nbx] : uint4{0u, 0u, 0u, 0u};
        // (c) this lane's group (ablation bit 64: skipped, diagnostic timing only)
        if (threadIdx.x < ng && !ablate(pa, 64u))
        {
            const float *Dm = MONO ? s.d1 : dtab + kTab * (gr.y >> 27);
            group_forces<ISO>(gr, sxp, sq, sst, sK6, Dm, sfxy, sfz);
        }
        __syncthreads();
        // (d) next tile's gathers (ablation bit 256: skipped)
        if (tn_next < t_end && !ablate(pa, 256u))
            group_issue_gather<SANITIZE, MODE>(s, x, pa.z, cur);
        // (e) fold per tile node -> node-major partials (+ p.Ap) (ablation bit 128: skipped)
#pragma unroll
        for (int k = 0; k < 2; ++k)
        {
            const uint32_t i = threadIdx.x + k * NT;
            if (i < (ablate(pa, 128u) ? 0u : nn))
            {
                const uint2 tn = tn_own[k];
                float a0, a1, a2;
                fold_run(sfxy, sfz, tn.y & 0xffffu, tn.y >> 16, a0, a1, a2);
                float p0 = 0.f, p1 = 0.f, p2 = 0.f;
                if constexpr (MODE == 1)
                {
                    p0 = sxp[i].w;
                    p1 = sq[i].x;
                    p2 = sq[i].y;
                    if (tn.x & 0x80000000u)  // the node's owner slot carries its mass term m s_M p (once)
                    {
                        const float m = m_own[k] * sM;
                        a0 = fmaf(m, p0, a0);
                        a1 = fmaf(m, p1, a1);
                        a2 = fmaf(m, p2, a2);
                        if (pa.pnew)  // and stores the new p for the update pass
                            store3(pa.pnew, whole_rsrc(pa.pnew), tn.x & 0x7fffffffu, p0, p1, p2, false);
                    }
                }
                if (!ablate(pa, 512u))
                    store3(T.part, whole_rsrc(T.part), slot_own[k], a0, a1, a2, T.wt_part != 0);
                if (MODE == 1 && (tn.x & 0x7fffffffu) < s.Nown)  // ghosts: another rank's row
                    pap += (double)fmaf(p2, a2, fmaf(p1, a1, p0 * a0));  // fp32 per node, fp64 across nodes
            }
        }
        __syncthreads();  // LDS is refilled by the next tile
        hd = hdn;
    }
    if constexpr (MODE == 1)
    {
        const double tt = block_sum<NT>(pap, red);
        if (threadIdx.x == 0)
            pa.part_dot[blockIdx.x] = tt;
    }
}

// pushed forces {f_x, f_y} + f_z per slot, then per tile node {x y z v_x} {v_y v_z} and its u16 run start
constexpr size_t group_lds(int nt) { return sizeof(float) * 3 * kGroupSlotsPerLane * nt + 2 * nt * (16 + 8 + 2); }

template <bool ISO, bool SAN, int MODE, int NT, bool MONO> Pick<HdrTileFn> groups_pick()
{
    static const std::string name = kernel_name("k_keff_groups_pipe", ISO, SAN, MODE, NT, MONO);
    return {k_keff_groups_pipe<ISO, SAN, MODE, NT, MONO>, name.c_str()};
}

HdrTilePick pick_groups(const DevSys &s, bool pcg, bool sanitize)
{
    const int nt = s.t.pipe_nt == 256 ? 256 : 128;
    return {with_bools(
                [](auto iso, auto pc, auto san, auto wide, auto mono) {
                    return groups_pick<iso(), !pc() && san(), pc() ? 1 : 0, wide() ? 256 : 128, mono()>();
                },
                s.iso != 0, pcg, sanitize, nt == 256, s.M == 1),
            nt, group_lds(nt)};
}
}  // namespace

void launch_groups(const DevSys &s, const float *x, const PcgPassArgs &pa, bool pcg, bool sanitize, hipStream_t st,
                   hipEvent_t e0, hipEvent_t e1)
{
    const HdrTilePick p = pick_groups(s, pcg, sanitize);
    launch_kernel(p.k.fn, s.t.pipe_grid, p.nt, p.lds, st, e0, e1, s, x, PcgArgs{pa}, s.t.hdr);
}

const char *groups_kernel_name(const DevSys &s) { return pick_groups(s, true, false).k.name; }

unsigned groups_pipe_grid(const DevSys &s)
{
    const HdrTilePick p = pick_groups(s, true, false);
    return xcd_grid(p.k.fn, p.nt, p.lds, s.t.ntiles);
}

}  // namespace cwf
