// keff_pick.hpp -- how the K_eff / PCG kernel translation units (the FAST units, resident.hip, parity_keff.hip) pick
// a template instantiation. Each kernel family has one picker next to its kernels: a pure function of the handle's facts
// (no HIP call) that returns a Pick. The launch, the occupancy / grid / LDS queries and cwf_hip_system_keff_kernel all
// take the instantiation from it, so the reported name is the launched kernel's.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <string>
#include <type_traits>

namespace cwf
{
// one instantiation: its address, and its name as rocprofv3 prints it less the namespaces. A family's
// `template <...> Pick<Fn> pick()` forms both from the same arguments: a name exists only for a pointer that exists
template <class Fn> struct Pick
{
    Fn fn;
    const char *name;
};

// f(std::bool_constant...) for runtime bools, the first bool first
template <class F> auto with_bools(F &&f) { return f(); }
template <class F, class... B> auto with_bools(F &&f, bool b, B... bs)
{
    const auto next = [&](auto c) { return with_bools([&](auto... cs) { return f(c, cs...); }, bs...); };
    return b ? next(std::true_type{}) : next(std::false_type{});
}

inline std::string targ(bool b) { return b ? "true" : "false"; }
inline std::string targ(int v) { return std::to_string(v); }
inline std::string targ(const char *s) { return s; }
template <class A0, class... A> std::string kernel_name(const char *base, A0 a0, A... a)
{
    std::string n = std::string(base) + "<" + targ(a0);
    ((n += ", " + targ(a)), ...);
    return n + ">";
}

// e0/e1 (optional): hipExtLaunchKernel stamps them from the dispatch packet itself, so the timed interval is the
// kernel's own execution (what rocprofv3 --kernel-trace reports), not marker latency
template <class... P, class... A>
void launch_kernel(void (*k)(P...), unsigned grid, unsigned block, size_t lds, hipStream_t st, hipEvent_t e0,
                   hipEvent_t e1, const A &...a)
{
    if (e0 && e1)
        hipExtLaunchKernelGGL(k, dim3(grid), dim3(block), (uint32_t)lds, st, e0, e1, 0, a...);
    else
        k<<<grid, block, lds, st>>>(a...);
}

// workgroups of k resident on the device at once (occupancy x CUs; 1 where a query fails)
template <class Fn> unsigned resident_blocks(Fn k, int block, size_t lds)
{
    int dev = 0, bpc = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, k, block, lds);
    return (unsigned)((bpc > 0 ? bpc : 1) * (cus > 0 ? cus : 1));
}

// a persistent grid over `ntiles` tiles: the resident workgroups in whole XCD groups of 8, no more than the tiles need
template <class Fn> unsigned xcd_grid(Fn k, int block, size_t lds, unsigned ntiles)
{
    unsigned g = resident_blocks(k, block, lds);
    g = g < 8u ? 8u : g - g % 8u;
    const unsigned need = ((ntiles + 7u) / 8u) * 8u;
    return g < need ? g : (need ? need : 8u);
}

}  // namespace cwf
