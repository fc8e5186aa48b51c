// resident_image.hpp -- the strides of a resident box's LDS image (resident.hip `pl`), chosen per box by a model of the
// LDS bank conflicts its accesses make. Host only, plain C++ (no HIP call): resident.cpp's plan uses it, and
// tests/cpp/resident_image_test.cpp builds it stand-alone.
//
// The image holds one float4 slot per node of the box plus its one-node ring, slot = k PXY + j PX + i. Per phase
//   - the form stores each own and each ring entry's p into its slot (ds_write_b128, one per entry), and
//   - each own node's row loads its nOff - 1 neighbours at slot + a constant per offset (ds_read_b128),
// thread t of the 512 holding entries t, t + 512, ... of the box's lists, so entries [64 w, 64 w + 64) of a list are the
// 64 lanes of one wave-instruction.
//
// The model (the LDS table of the MI355X microarchitecture guide, section "LDS"):
//   - ds_read_b128: bank = (byte address / 4) mod 64, i.e. a 16-B slot covers one of 16 bank quads, slot mod 16. A
//     wave's access is served in four fixed groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same
//     two in the upper half; only the lanes of a group conflict, identical addresses broadcast, and each extra distinct
//     address on a bank adds one LDS cycle: a group costs the largest number of distinct slots on one bank quad, at
//     least 1. A constant added to every lane's slot permutes the bank quads, so all nOff - 1 reads of a row cost what
//     its base slots cost.
//   - ds_write_b128: bank = (byte address / 4) mod 32, slot mod 8; eight groups of 8 contiguous lanes, counted the same
//     way; the wave-instruction costs its LDS-array cycles but never less than the 13 cycles its operands take to reach
//     the LDS.
// With dense strides (PX = sx + 2) a box whose lanes run along x pairs lanes l and l + sx on one bank quad, and a row of
// block-face nodes at fixed x steps j by exactly PX slots: 16 lanes on one quad for PX = 16. Padding PX and PXY moves
// both off the multiples of 16; which padding is best depends on the box's lists, so the chooser searches per box.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace cwf
{
// a list entry's place in the image: 0 and s + 1 are the ring, 1..s the box's own nodes
struct ImageNode
{
    uint16_t i, j, k;
};

struct ImageStrides
{
    unsigned px = 0, pxy = 0, slots = 0;  // slots = pxy * (sz + 2)
    uint64_t read = 0, write = 0;         // LDS-array cycles per phase: the rows' loads, the form's stores
    uint64_t cost() const { return read + write; }
};

constexpr unsigned kImageSearchPx = 16, kImageSearchPxy = 15;  // PX <= dense + 16, PXY <= PX (sy + 2) + 15: every
                                                               // residue mod 16 of both
constexpr unsigned kImageMaxSlots = 65535;  // a slot travels in 16 bits of the kernel's osc / hsc

namespace image_detail
{
// lane -> group of a ds_read_b128 (the guide's table; lanes 32-63 as 0-31, groups 2 and 3)
inline unsigned read_group(unsigned lane)
{
    const unsigned l = lane & 31u;
    const bool a = l < 4u || (l >= 12u && l < 16u) || (l >= 20u && l < 28u);
    return (a ? 0u : 1u) + 2u * (lane >> 5);
}

// the cycles of one wave-instruction's groups: lanes [0, n) at slots s[0..n), `group(lane)` in [0, NG), NB bank quads
template <unsigned NG, unsigned NB, class Group>
inline unsigned wave_cycles(const uint32_t *s, size_t n, Group group)
{
    uint32_t seen[NG][NB][64 / NG];
    unsigned cnt[NG][NB] = {};
    for (size_t l = 0; l < n; ++l)
    {
        const unsigned g = group((unsigned)l), q = s[l] % NB;
        bool dup = false;
        for (unsigned c = 0; c < cnt[g][q]; ++c)
            dup = dup || seen[g][q][c] == s[l];
        if (!dup)
            seen[g][q][cnt[g][q]++] = s[l];
    }
    unsigned cyc = 0;
    for (unsigned g = 0; g < NG; ++g)
    {
        unsigned m = 1;
        for (unsigned q = 0; q < NB; ++q)
            m = cnt[g][q] > m ? cnt[g][q] : m;
        cyc += m;
    }
    return cyc;
}
}  // namespace image_detail

// LDS-array cycles of ONE ds_read_b128 per entry of a list in thread order (a row makes nOff - 1 of them)
inline uint64_t image_read_cycles(const uint32_t *slots, size_t n)
{
    uint64_t c = 0;
    for (size_t w = 0; w < n; w += 64)
        c += image_detail::wave_cycles<4, 16>(slots + w, n - w < 64 ? n - w : 64, image_detail::read_group);
    return c;
}

// cycles of one ds_write_b128 per entry of a list in thread order
inline uint64_t image_write_cycles(const uint32_t *slots, size_t n)
{
    uint64_t c = 0;
    for (size_t w = 0; w < n; w += 64)
    {
        const unsigned a = image_detail::wave_cycles<8, 8>(slots + w, n - w < 64 ? n - w : 64, [](unsigned l) { return l >> 3; });
        c += a > 13u ? a : 13u;
    }
    return c;
}

// The cost of a box's image accesses per phase: the own list's and the halo list's slots, both in thread order, and
// the element kind's offset count (15 Kuhn, 27 hex8; offset 0 is the node itself, held in a register)
inline ImageStrides image_cost(const uint32_t *own, size_t n_own, const uint32_t *halo, size_t n_halo, int noff)
{
    ImageStrides c;
    c.read = (uint64_t)(noff - 1) * image_read_cycles(own, n_own);
    c.write = image_write_cycles(own, n_own) + image_write_cycles(halo, n_halo);
    return c;
}

inline uint32_t image_slot(const ImageNode &e, unsigned px, unsigned pxy) { return e.k * pxy + e.j * px + e.i; }

// The chooser. One object per plan: boxes with the same lists (C2: 245 boxes, 27 kinds of own list) share their tables.
class ImageChooser
{
  public:
    // the strides of an (sx, sy, sz) box with these lists: the cheapest of PX in [sx + 2, sx + 2 + kImageSearchPx],
    // PXY in [PX (sy + 2), PX (sy + 2) + kImageSearchPxy] whose image has at most min(cap, kImageMaxSlots) slots; ties
    // to the smaller image, then the smaller PX. The dense strides are the first candidate, so a box nothing improves
    // keeps them (and a box whose dense image is over the cap gets them back unchanged: the plan refuses it).
    // pad = false: the dense strides and their cost
    ImageStrides choose(unsigned sx, unsigned sy, unsigned sz, const std::vector<ImageNode> &own,
                        const std::vector<ImageNode> &halo, int noff, uint64_t cap, bool pad = true)
    {
        // distinct nodes have distinct slots under every candidate, so a list's cycles depend only on the strides'
        // residues: mod 16 for the loads, mod 8 for the stores
        Table &ro = table(rd_, own, 16), &wo = table(wr_, own, 8), &wh = table(wr_, halo, 8);
        const unsigned px0 = sx + 2;
        ImageStrides best;
        for (unsigned px = px0; px <= px0 + (pad ? kImageSearchPx : 0u); ++px)
            for (unsigned d = 0; d <= (pad ? kImageSearchPxy : 0u); ++d)
            {
                ImageStrides c;
                c.px = px, c.pxy = px * (sy + 2) + d;
                const uint64_t slots = (uint64_t)c.pxy * (sz + 2);
                if (best.px && (slots > cap || slots > kImageMaxSlots))
                    continue;
                c.slots = (unsigned)slots;
                c.read = (uint64_t)(noff - 1) * cycles(ro, own, c.px, c.pxy, 16, image_read_cycles);
                c.write = cycles(wo, own, c.px, c.pxy, 8, image_write_cycles) +
                          cycles(wh, halo, c.px, c.pxy, 8, image_write_cycles);
                if (!best.px || c.cost() < best.cost() || (c.cost() == best.cost() && c.slots < best.slots))
                    best = c;
            }
        return best;
    }

  private:
    using Key = std::vector<uint64_t>;
    using Table = std::vector<int64_t>;  // [m][m] cycles by (PX mod m, PXY mod m), -1: not computed yet
    std::map<Key, Table> rd_, wr_;
    std::vector<uint32_t> tmp_;

    static Table &table(std::map<Key, Table> &memo, const std::vector<ImageNode> &l, unsigned m)
    {
        Key k(l.size());
        for (size_t e = 0; e < l.size(); ++e)
            k[e] = (uint64_t)l[e].i | (uint64_t)l[e].j << 16 | (uint64_t)l[e].k << 32;
        Table &t = memo[k];
        if (t.empty())
            t.assign((size_t)m * m, -1);
        return t;
    }
    template <class F>
    uint64_t cycles(Table &t, const std::vector<ImageNode> &l, unsigned px, unsigned pxy, unsigned m, F f)
    {
        int64_t &c = t[(size_t)(px % m) * m + pxy % m];
        if (c < 0)
        {
            tmp_.resize(l.size());
            for (size_t e = 0; e < l.size(); ++e)
                tmp_[e] = image_slot(l[e], px, pxy);
            c = (int64_t)f(tmp_.data(), tmp_.size());
        }
        return (uint64_t)c;
    }
};

}  // namespace cwf
