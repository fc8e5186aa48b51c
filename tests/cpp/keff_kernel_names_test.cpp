// keff_kernel_names_test.cpp -- cwf_hip_system_keff_kernel over every combination of the facts the kernel pickers
// read (keff_pick.hpp), on handles fabricated here: no create, no GPU call. One line per case, "<facts>: <name>";
// tests/test_host.py compares the output with tests/golden/keff_kernel_names.txt.
// Built and run by tests/test_host.py (g++, -D__HIP_PLATFORM_AMD__, -lcwf_hip).
#include <cstdio>

#include "cwf_internal.hpp"

using namespace cwf;

namespace
{
const uint32_t kDummy[4] = {0, 0, 0, 0};

// a FAST handle whose schedule is decided (two-kernel unless the case says otherwise)
cwf_hip_system fast_handle()
{
    cwf_hip_system h;
    h.mode = CWF_MODE_FAST;
    h.sched.state = SchedulePlan::Decided;
    h.ds.N = h.ds.Nown = 10;
    h.ds.M = 1;
    h.ds.t.ntiles = 1;
    return h;
}

void lattice_facts(DevTiles &t, int sym, int hex, int mu, int zr, int aff)
{
    t.lat = 1;
    t.lnwork = 4;
    t.lsym = sym;
    t.lhex = hex;
    t.lmu = mu;
    t.lzr = zr;
    t.lpstride = aff ? 7u : 0u;
}

#define BITS(v, n) for (int v = 0; v < (n); ++v)
}  // namespace

int main()
{
    BITS(iso, 2) BITS(compact, 2) BITS(rb, 2)
    {
        cwf_hip_system h;
        h.ds.iso = iso;
        h.ds.ptile_off = kDummy;
        h.ds.ptile_nodes = compact ? kDummy : nullptr;
        h.reduction_block = rb ? 100 : 256;
        std::printf("parity iso=%d compact=%d reduction_block=%d: %s\n", iso, compact, (int)h.reduction_block,
                    cwf_hip_system_keff_kernel(&h));
    }
    BITS(sym, 2) BITS(hex, 2) BITS(mu, 2) BITS(zr, 2) BITS(aff, 2)
    {
        cwf_hip_system h = fast_handle();
        lattice_facts(h.ds.t, sym, hex, mu, zr, aff);
        std::printf("lattice lsym=%d lhex=%d lmu=%d lzr=%d affine=%d: %s\n", sym, hex, mu, zr, aff,
                    cwf_hip_system_keff_kernel(&h));
    }
    BITS(hex, 2) BITS(aff, 2)
    {
        cwf_hip_system h = fast_handle();
        lattice_facts(h.ds.t, 0, hex, 0, 0, aff);
        h.ds.t.llayers = (2u << 16) | 3u;
        std::printf("layered lhex=%d affine=%d: %s\n", hex, aff, cwf_hip_system_keff_kernel(&h));
    }
    BITS(sym, 2) BITS(hex, 2) BITS(mu, 2) BITS(aff, 2) BITS(ghosts, 2) BITS(persist, 2)
    {
        cwf_hip_system h = fast_handle();
        lattice_facts(h.ds.t, sym, hex, mu, 0, aff);
        h.sched.launch = PcgSchedule::Fused;
        h.sched.grid = persist ? 2u : 4u;
        h.ds.Nown = ghosts ? 5 : 10;
        std::printf("fused lsym=%d lhex=%d lmu=%d affine=%d ghosts=%d grid_below_items=%d: %s\n", sym, hex, mu, aff,
                    ghosts, persist, cwf_hip_system_keff_kernel(&h));
    }
    BITS(sym, 2) BITS(hex, 2) BITS(large, 2) BITS(shard, 2)
    {
        cwf_hip_system h = fast_handle();
        lattice_facts(h.ds.t, sym, hex, 1, 0, 1);
        h.sched.launch = PcgSchedule::Fused;
        h.sched.resident = true;
        h.res.npt = large ? 4 : 3;
        h.res.nph = large ? 3 : 2;
        h.res.shard = shard != 0;
        std::printf("resident lsym=%d lhex=%d npt=%u nph=%u shard=%d: %s\n", sym, hex, h.res.npt, h.res.nph, shard,
                    cwf_hip_system_keff_kernel(&h));
    }
    BITS(iso, 2) BITS(mono, 2) BITS(wide, 2)
    {
        cwf_hip_system h = fast_handle();
        h.ds.iso = iso;
        h.ds.M = mono ? 1 : 2;
        h.ds.t.grp = h.ds.t.pipe = 1;
        h.ds.t.pipe_nt = wide ? 256 : 128;
        std::printf("groups iso=%d M=%d pipe_nt=%d: %s\n", iso, (int)h.ds.M, h.ds.t.pipe_nt, cwf_hip_system_keff_kernel(&h));
    }
    BITS(iso, 2) BITS(wide, 2) BITS(aff, 2)
    {
        cwf_hip_system h = fast_handle();
        h.ds.iso = iso;
        h.ds.t.hex = 1;
        h.ds.t.hex_nt = wide ? 256 : 128;
        h.ds.t.hex_all_affine = aff;
        std::printf("hex iso=%d hex_nt=%d all_affine=%d: %s\n", iso, h.ds.t.hex_nt, aff, cwf_hip_system_keff_kernel(&h));
    }
    BITS(iso, 2) BITS(wide, 2)
    {
        cwf_hip_system h = fast_handle();
        h.ds.iso = iso;
        h.ds.t.pipe = 1;
        h.ds.t.pipe_nt = wide ? 256 : 128;
        std::printf("pipe iso=%d pipe_nt=%d: %s\n", iso, h.ds.t.pipe_nt, cwf_hip_system_keff_kernel(&h));
    }
    BITS(iso, 2) BITS(geo, 2)
    {
        cwf_hip_system h = fast_handle();
        h.ds.iso = iso;
        h.ds.t.geo = geo;
        std::printf("records iso=%d geo=%d: %s\n", iso, geo, cwf_hip_system_keff_kernel(&h));
    }
    return 0;
}
