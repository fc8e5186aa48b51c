// lattice_body.inc -- the body of k_keff_lattice and of k_keff_lattice_layered (lattice.hip includes it once in each,
// so the one-material kernels compile from exactly the statements they always had). In scope: the kernel's
// arguments s, x, pa, coef, plane and lay, and MODE, SANITIZE, SYM, E, MU, ZR, AFF, LAY as compile-time constants.
// LAY (a layered block): the stencil blocks of a row are those of its plane's class: lay[k] & 0xFFFF times the table
// stride, fetched as a scalar (lay is a restrict kernel argument and k is workgroup-uniform), so the blocks stay
// scalar loads behind one more scalar load per plane. Never SYM: S_d is symmetric only on planes between equal
// layers (lattice.cpp).
    constexpr int BX = kLatBX, BY = kLatNT / BX, PX = BX + 2, PLANE = PX * (BY + 2);
    static_assert(PLANE <= 2 * kLatNT, "two halo entries per thread");
    __shared__ float4 pl[kLatRing][PLANE];
    __shared__ double red[2 * (kLatNT / 64)];
    __shared__ float4 czA[ZR ? kLatClasses : 1];  // ZR: each class's block inverse {a00 a01 a02 a11}, {a12 a22}
    __shared__ float2 czB[ZR ? kLatClasses : 1];
    const DevTiles &T = s.t;
    static_assert(kLatClasses <= kLatNT, "one class per thread");
    // the work item: a brick (ib, jb, kc) or a shell workgroup (its first node qs in the shell enumeration of
    // lattice_shell_node; qn nodes from there)
    bool shell;
    uint32_t ib, jb, kc, qs = 0, qn = 0;
    const uint32_t cols = max(T.lnbx * T.lnby, 1u);
    if (T.lshl == 2)
    {
        // interleaved: every item on one XCD-contiguous numbering; chunk c's cols bricks, then lnsc workgroups of
        // the perimeters of its planes (gathering lines its bricks have just brought into this XCD's L2); the
        // full planes k = 0 and nz - 1 after all chunks
        const uint32_t nw = T.lnwork, xcd = blockIdx.x & 7u;
        const uint32_t w = xcd * (nw >> 3) + min(xcd, nw & 7u) + (blockIdx.x >> 3);
        const uint32_t cw = cols + T.lnsc, nchunk = (T.lkI1 - T.lkI0 + T.lL - 1) / T.lL;
        const uint32_t nx = T.lnx, ny = T.lny, full = nx * ny, per = 2 * nx + 2 * (ny - 2);
        const uint32_t nlo = T.lk0 == 0 ? full : 0u, nmid = (T.lkI1 - T.lkI0) * per;
        if (w < nchunk * cw)
        {
            kc = w / cw;
            const uint32_t r = w % cw;
            shell = r >= cols;
            ib = r % max(T.lnbx, 1u);
            jb = r / max(T.lnbx, 1u);
            const uint32_t k0c = kc * T.lL, np = min(T.lL, T.lkI1 - T.lkI0 - k0c) * per, ql = (r - cols) * kLatNT;
            qs = nlo + k0c * per + ql;
            qn = shell && ql < np ? min(np - ql, (uint32_t)kLatNT) : 0u;
        }
        else
        {
            shell = true;
            ib = jb = kc = 0;
            const uint32_t f = w - nchunk * cw, flo = (nlo + kLatNT - 1) / kLatNT;
            qs = f < flo ? f * kLatNT : nlo + nmid + (f - flo) * kLatNT;
            qn = f < flo ? min(nlo - qs, (uint32_t)kLatNT) : min(T.lnshell - qs, (uint32_t)kLatNT);
        }
    }
    else
    {
        // lshl: the shell workgroups follow the bricks instead of leading them
        const uint32_t sb0 = T.lshl ? T.lnwm : 0u, bb0 = T.lshl ? 0u : T.lnsb;
        shell = blockIdx.x >= sb0 && blockIdx.x < sb0 + T.lnsb;
        if (shell)
        {
            qs = (blockIdx.x - sb0) * kLatNT;
            qn = qs < T.lnshell ? min(T.lnshell - qs, (uint32_t)kLatNT) : 0u;
        }
        // a brick: its work item (bricks follow the lnsb shell workgroups, a multiple of 8, so blockIdx mod 8 is
        // still the XCD), i-brick fastest, then j-brick, then k-chunk; each XCD takes a contiguous share
        const uint32_t nw = T.lnwm, bb = shell ? 0u : blockIdx.x - bb0, xcd = bb & 7u;
        const uint32_t w = xcd * (nw >> 3) + min(xcd, nw & 7u) + (bb >> 3);
        ib = w % max(T.lnbx, 1u);
        jb = (w / max(T.lnbx, 1u)) % max(T.lnby, 1u);
        kc = w / cols;
    }
    const int nx = (int)T.lnx, ny = (int)T.lny, nz = (int)T.lnz;
    const int i0 = 1 + (int)ib * BX, j0 = 1 + (int)jb * BY;
    const int kb = (int)T.lkI0 + (int)(kc * T.lL), ke = min(kb + (int)T.lL, (int)T.lkI1);
    const int ti = (int)(threadIdx.x & (BX - 1)), tj = (int)(threadIdx.x / BX);
    const int gi = i0 + ti, gj = j0 + tj;
    const bool active = gi < nx - 1 && gj < ny - 1;
    // the thread's two halo entries
    int eoff[2];
    bool evalid[2], eown[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
    {
        const int e = (int)threadIdx.x + kLatNT * u;
        const int ii = e % PX - 1, jj = e / PX - 1;
        const int hi = i0 + ii, hj = j0 + jj;
        evalid[u] = e < PLANE;
        eown[u] = evalid[u] && hi < nx - 1 && hj < ny - 1 && ii >= 0 && ii < BX && jj >= 0 && jj < BY;
        eoff[u] = min(hj, ny - 1) * nx + min(hi, nx - 1);  // the halo of the interior is inside the block
    }
    // byte offsets: 12 x (plane base) is scalar, 12 x (in-plane offset) hoisted here (no v_mul_lo_u32 per access)
    const uint32_t eoff12[2] = {12u * (uint32_t)eoff[0], 12u * (uint32_t)eoff[1]};
    const auto ld3 = [](__amdgpu_buffer_rsrc_t rs, uint32_t byteoff, float v[3]) {
        const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(rs, byteoff, 0, 0);
        v[0] = __uint_as_float(w.x);
        v[1] = __uint_as_float(w.y);
        v[2] = __uint_as_float(w.z);
    };
    const auto st3 = [](__amdgpu_buffer_rsrc_t rs, uint32_t byteoff, float a, float b, float c) {
        const u32x3 v = {__float_as_uint(a), __float_as_uint(b), __float_as_uint(c)};
        __builtin_amdgcn_raw_buffer_store_b96(v, rs, byteoff, 0, 0);
    };
    constexpr uint32_t kOob12 = 12u * kLatOob3;
    const uint32_t vbytes = 12u * s.N, sbytes = 4u * s.N;
    const __amdgpu_buffer_rsrc_t rz = sized_rsrc(MODE == 1 ? pa.z : x, vbytes), rx = sized_rsrc(x, vbytes),
                                 rmass = sized_rsrc(s.mass, sbytes), rmask = sized_rsrc(s.mask, sbytes),
                                 rpnew = sized_rsrc(pa.pnew, pa.pnew ? vbytes : 0u),
                                 rpart = sized_rsrc(T.part, vbytes), rcls = sized_rsrc(T.lcls, ZR ? s.N : 0u);
    const auto load = [&](int k, LatFill &f) {
        if (ablate(pa, 256u) && k > kb + 2)  // diagnostic: no loads past the prologue's
            return;
        const uint32_t base = lat_plane<AFF>(T, plane, min(k, nz - 1));
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            const bool go = evalid[u] && k <= ke;  // planes past the work item's last halo plane are not read
            const uint32_t n = base + (uint32_t)eoff[u], nb = go ? 12u * base + eoff12[u] : kOob12;
            ld3(rz, nb, f.a[u]);
            if constexpr (MODE == 1)
            {
                ld3(rx, nb, f.b[u]);
                if constexpr (ZR)
                    f.c[u] = __builtin_amdgcn_raw_buffer_load_b8(rcls, go ? n : 0xFFFFFFFFu, 0, 0);
                if constexpr (MU)
                    f.m[u] = 0.f;
                else
                    f.m[u] = __uint_as_float(
                        __builtin_amdgcn_raw_buffer_load_b32(rmass, 4u * (go ? n : kLatOob1), 0, 0));
            }
            else if constexpr (SANITIZE)
            {
                const uint32_t mk = __builtin_amdgcn_raw_buffer_load_b32(rmask, 4u * (go ? n : kLatOob1), 0, 0);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    f.a[u][c] = (mk >> c) & 1u ? 0.f : f.a[u][c];
            }
        }
    };
    // registers of the planes in flight: the prologue's four, then two per step
    LatFill P0, P1, FA, FB;
    if (!shell)
    {
        load(kb - 1, P0);
        load(kb, P1);
        load(kb + 1, FA);
        load(kb + 2, FB);
    }
    // ZR: the thread's class (thread c, class c) inverse, loaded with the planes in flight: the prologue has one memory
    // round trip (the planes, this, the control block and the scalar fold's shares together) instead of three (the
    // control block, then the class table, then the rest)
    float4 zA = {0.f, 0.f, 0.f, 0.f}, zB = {0.f, 0.f, 0.f, 0.f};
    if constexpr (ZR)
    {
        const uint32_t c = min((uint32_t)threadIdx.x, kLatClasses - 1u);
        zA = T.lcz[2u * c];
        zB = T.lcz[2u * c + 1u];
    }
    float beta = 0.f;
    if constexpr (MODE == 1)  // the scalar fold overlaps the first loads
    {
        const CtlPre pre = ctl_prefetch(pa.ctl, pa.it);  // vector loads, in flight with the planes and the fold's
        if (ablate(pa, 1024u) ? !pre.active
                              : !residual_step<kLatNT, 8>(pa.ctl, pa.prr, pa.prz, pa.nupd, pa.stride, pa.it, pa.hist, red,
                                                       &beta, pa.abl & 32u, &pre))
            return;
    }
    if constexpr (ZR)
    {
        if (threadIdx.x < kLatClasses)
        {
            czA[threadIdx.x] = zA;
            czB[threadIdx.x] = float2{zB.x, zB.y};
        }
        __syncthreads();
    }
    double pap = 0.0;
    if (shell)
    {
        if (threadIdx.x < qn && !ablate(pa, 2048u))  // diagnostic: no shell rows
        {
            if constexpr (LAY)  // with the planes the workgroup's nodes span (workgroup-uniform)
                pap = lattice_shell_node<MODE, SANITIZE, E, ZR, AFF, true>(
                    s, x, pa, coef, plane, qs + threadIdx.x, beta, czA, czB, lay, lattice_shell_plane(T, qs),
                    lattice_shell_plane(T, qs + max(qn, 1u) - 1u));
            else
            pap = lattice_shell_node<MODE, SANITIZE, E, ZR, AFF>(s, x, pa, coef, plane, qs + threadIdx.x, beta, czA,
                                                                 czB);
        }
    }
    else if (!ablate(pa, 4096u))  // diagnostic: no bricks
    {
    // plane q lives in LDS slot (q - kb + 1) mod 6
    const auto write = [&](int k, int slot, const LatFill &f) {
        float4 *dst = pl[slot];
        const bool own = MODE == 1 && k >= kb && k < ke;
        const uint32_t base = lat_plane<AFF>(T, plane, min(k, nz - 1));
#pragma unroll
        for (int u = 0; u < 2; ++u)
        {
            float v[3], zz[3] = {f.a[u][0], f.a[u][1], f.a[u][2]};
            if constexpr (ZR)
                lat_z(czA[f.c[u]], czB[f.c[u]], f.c[u], f.a[u], zz);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                v[c] = MODE == 1 ? fmaf(beta, f.b[u][c], zz[c]) : zz[c];
            if (evalid[u])
                dst[(int)threadIdx.x + kLatNT * u] = float4{v[0], v[1], v[2], MODE == 1 ? f.m[u] : 0.f};
            if (MODE == 1 && !ablate(pa, 512u))
            {
                const uint32_t n = base + (uint32_t)eoff[u];
                st3(rpnew, own && eown[u] && n < s.Nown ? 12u * base + eoff12[u] : kOob12, v[0], v[1], v[2]);
            }
        }
    };
    const float sK = (float)s.sK, sM = (float)s.sM;
    const int c0 = (tj + 1) * PX + ti + 1;
    const uint32_t gidx = (uint32_t)(gj * nx + gi), gidx12 = 12u * gidx;
    // the row of the thread's interior node in plane k (slots sm, s0c, sp hold planes k - 1, k, k + 1), one plane at
    // a time in scalar fp32: both planes of a step side by side in packed fp32 (v_pk_fma_f32) held twice the
    // neighbour values live (144 VGPRs, 3 waves per SIMD) and measured slower (C2 16.4 vs 15.3 us, C3 64.9 vs
    // 63.4 us, same box); the kernel is not VALU-bound
    const auto rows1 = [&](int k, int sm, int s0c, int sp, bool last) {
        int zoff;
        asm volatile("s_mov_b32 %0, 0" : "=s"(zoff));
        const float *__restrict__ cf = coef + zoff;
        if constexpr (LAY)  // the table of the plane's class
            cf += __builtin_amdgcn_readfirstlane(min(lay[min(k, nz - 1)] & 0xFFFFu, (T.llayers & 0xFFFFu) - 1u)) *
                  (9u * E::nOff);
        const float4 q0 = pl[s0c][c0];
        const float u0[3] = {q0.x, q0.y, q0.z};
        // rows 0 and 1 (and the x, y differences) in packed fp32: the same FMAs, subtractions and additions in the
        // same order as the scalar form, so bitwise its result; the device blocks are row-pair interleaved
        // (abi.cpp: {S00 S10 S01 S11 S02 S12 S20 S21 S22} per offset)
        const f2 u0xy = {q0.x, q0.y};
        f2 acc01 = {0.f, 0.f};
        float acc2 = 0.f;
#pragma unroll
        for (int o = 1; o < E::nOff; o += (SYM ? 2 : 1))
        {
            f2 wxy;
            float wz;
            const auto dv = [&](int oo, f2 &dxy, float &dz3) {
                const int dz = E::off[oo][2];
                const float4 q = pl[dz < 0 ? sm : dz > 0 ? sp : s0c][c0 + E::off[oo][1] * PX + E::off[oo][0]];
                dxy = f2{q.x, q.y} - u0xy;
                dz3 = q.z - u0[2];
            };
            dv(o, wxy, wz);
            if constexpr (SYM)
            {
                f2 vxy;
                float vz;
                dv(o + 1, vxy, vz);
                wxy += vxy;
                wz += vz;
            }
            const float *b = cf + 9 * o;
            acc01 = __builtin_elementwise_fma(f2{b[0], b[1]}, f2{wxy.x, wxy.x}, acc01);
            acc01 = __builtin_elementwise_fma(f2{b[2], b[3]}, f2{wxy.y, wxy.y}, acc01);
            acc01 = __builtin_elementwise_fma(f2{b[4], b[5]}, f2{wz, wz}, acc01);
            acc2 = fmaf(b[6], wxy.x, acc2);
            acc2 = fmaf(b[7], wxy.y, acc2);
            acc2 = fmaf(b[8], wz, acc2);
        }
        const float acc[3] = {acc01.x, acc01.y, acc2};
        const float m = MODE == 1 ? (MU ? T.lmass : q0.w) * sM : 0.f;
        float a[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            a[r] = fmaf(m, u0[r], sK * acc[r]);
        const uint32_t pb = lat_plane<AFF>(T, plane, min(k, nz - 1)), n = pb + gidx;
        const bool mine = active && !last && n < s.Nown;
        if (!ablate(pa, 512u))
            st3(rpart, mine ? 12u * pb + gidx12 : kOob12, a[0], a[1], a[2]);
        if constexpr (MODE == 1)
            pap += mine ? (double)fmaf(u0[2], a[2], fmaf(u0[1], a[1], u0[0] * a[0])) : 0.0;
    };
    write(kb - 1, 0, P0);
    write(kb, 1, P1);
    // step m: planes k = kb + 2m, k + 1; writes planes k + 1, k + 2 (slots 2m + 2, 2m + 3 mod 6), reads slots
    // 2m .. 2m + 3 (mod 6); unrolled by 3 so the slots are constants
    const auto step = [&](int k, int s0, int s1, int s2, int s3) {
        write(k + 1, s2, FA);
        write(k + 2, s3, FB);
        __syncthreads();
        load(k + 3, FA);
        load(k + 4, FB);
        if (!ablate(pa, 64u))  // diagnostic: no rows
        {
            rows1(k, s0, s1, s2, false);
            rows1(k + 1, s1, s2, s3, k + 1 >= ke);
        }
    };
    for (int k = kb; k < ke; k += 6)
    {
        step(k, 0, 1, 2, 3);
        if (k + 2 < ke)
            step(k + 2, 2, 3, 4, 5);
        if (k + 4 < ke)
            step(k + 4, 4, 5, 0, 1);
    }
    }  // bricks
    if constexpr (MODE == 1)
    {
        const double tt = block_sum<kLatNT>(pap, red);
        if (threadIdx.x == 0)
            pa.part_dot[blockIdx.x] = tt;
    }
