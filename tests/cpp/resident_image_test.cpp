// resident_image_test.cpp -- csrc/resident_image.hpp (the LDS bank-conflict model of a resident box's image and the
// per-box stride chooser) on lists built the way csrc/resident.cpp's plan_resident builds them: block-surface nodes
// first, then k, j, i with x fastest; publication indices in that order box after box; each halo list sorted by the
// owner's publication index. Host only; prints "ok". An argument N takes every N-th sx of the shape sweep.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "resident_image.hpp"

using namespace cwf;

namespace
{
int fails = 0;
#define CHECK(c, ...)                                   \
    do                                                  \
    {                                                   \
        if (!(c))                                       \
        {                                               \
            ++fails;                                    \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #c); \
            std::printf(__VA_ARGS__);                   \
            std::printf("\n");                          \
        }                                               \
    } while (0)

// the stencil offsets besides the node itself: the Kuhn split's 14, hex8's 26
std::vector<std::vector<int>> offsets(bool hex)
{
    std::vector<std::vector<int>> o;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx)
            {
                if (!dx && !dy && !dz)
                    continue;
                const bool kuhn = (dx >= 0 && dy >= 0 && dz >= 0) || (dx <= 0 && dy <= 0 && dz <= 0);
                if (hex || kuhn)
                    o.push_back({dx, dy, dz});
            }
    return o;
}

struct Box
{
    unsigned s[3];
    std::vector<ImageNode> own, halo;
};

// the plan's lists for a lattice of n nodes cut into g boxes per axis (the plan's split: [n q / g, n (q + 1) / g))
std::vector<Box> plan(const unsigned n[3], const unsigned g[3], bool hex)
{
    const auto off = offsets(hex);
    const unsigned G = g[0] * g[1] * g[2], N = n[0] * n[1] * n[2];
    const auto node = [&](unsigned i, unsigned j, unsigned k) { return (k * n[1] + j) * n[0] + i; };
    std::vector<unsigned> lo(3 * G), hi(3 * G);
    std::vector<uint32_t> owner(N);
    for (unsigned b = 0; b < G; ++b)
    {
        const unsigned q[3] = {b % g[0], (b / g[0]) % g[1], b / (g[0] * g[1])};
        for (int a = 0; a < 3; ++a)
            lo[3 * b + a] = (unsigned)((uint64_t)n[a] * q[a] / g[a]), hi[3 * b + a] = (unsigned)((uint64_t)n[a] * (q[a] + 1) / g[a]);
        for (unsigned k = lo[3 * b + 2]; k < hi[3 * b + 2]; ++k)
            for (unsigned j = lo[3 * b + 1]; j < hi[3 * b + 1]; ++j)
                for (unsigned i = lo[3 * b]; i < hi[3 * b]; ++i)
                    owner[node(i, j, k)] = b;
    }
    const auto inside = [&](long i, long j, long k) {
        return i >= 0 && j >= 0 && k >= 0 && i < (long)n[0] && j < (long)n[1] && k < (long)n[2];
    };
    std::vector<uint8_t> needed(N, 0);
    for (unsigned k = 0; k < n[2]; ++k)
        for (unsigned j = 0; j < n[1]; ++j)
            for (unsigned i = 0; i < n[0]; ++i)
                for (const auto &o : off)
                    if (inside((long)i + o[0], (long)j + o[1], (long)k + o[2]))
                    {
                        const uint32_t m = node(i + o[0], j + o[1], k + o[2]);
                        if (owner[m] != owner[node(i, j, k)])
                            needed[m] = 1;
                    }
    std::vector<Box> boxes(G);
    std::vector<uint32_t> pub(N, 0xFFFFFFFFu);
    uint32_t npub = 0;
    for (unsigned b = 0; b < G; ++b)
    {
        Box &B = boxes[b];
        for (int a = 0; a < 3; ++a)
            B.s[a] = hi[3 * b + a] - lo[3 * b + a];
        for (int pass = 0; pass < 2; ++pass)
            for (unsigned k = lo[3 * b + 2]; k < hi[3 * b + 2]; ++k)
                for (unsigned j = lo[3 * b + 1]; j < hi[3 * b + 1]; ++j)
                    for (unsigned i = lo[3 * b]; i < hi[3 * b]; ++i)
                    {
                        const bool surface = !i || !j || !k || i == n[0] - 1 || j == n[1] - 1 || k == n[2] - 1;
                        if (surface != (pass == 0))
                            continue;
                        if (needed[node(i, j, k)])
                            pub[node(i, j, k)] = npub++;
                        B.own.push_back(ImageNode{(uint16_t)(i - lo[3 * b] + 1), (uint16_t)(j - lo[3 * b + 1] + 1),
                                                  (uint16_t)(k - lo[3 * b + 2] + 1)});
                    }
    }
    std::vector<uint32_t> seen(N, 0xFFFFFFFFu);
    for (unsigned b = 0; b < G; ++b)
    {
        std::vector<std::pair<uint32_t, ImageNode>> h;
        for (unsigned k = lo[3 * b + 2]; k < hi[3 * b + 2]; ++k)
            for (unsigned j = lo[3 * b + 1]; j < hi[3 * b + 1]; ++j)
                for (unsigned i = lo[3 * b]; i < hi[3 * b]; ++i)
                    for (const auto &o : off)
                    {
                        const long ii = (long)i + o[0], jj = (long)j + o[1], kk = (long)k + o[2];
                        if (!inside(ii, jj, kk))
                            continue;
                        const uint32_t m = node((unsigned)ii, (unsigned)jj, (unsigned)kk);
                        if (owner[m] == b || seen[m] == b)
                            continue;
                        seen[m] = b;
                        h.push_back({pub[m], ImageNode{(uint16_t)(ii - (long)lo[3 * b] + 1), (uint16_t)(jj - (long)lo[3 * b + 1] + 1),
                                                       (uint16_t)(kk - (long)lo[3 * b + 2] + 1)}});
                    }
        std::sort(h.begin(), h.end(), [](const auto &a, const auto &c) { return a.first < c.first; });
        for (const auto &e : h)
            boxes[b].halo.push_back(e.second);
    }
    return boxes;
}

std::vector<uint32_t> slots(const std::vector<ImageNode> &l, unsigned px, unsigned pxy)
{
    std::vector<uint32_t> s;
    for (const ImageNode &e : l)
        s.push_back(image_slot(e, px, pxy));
    return s;
}

// the chosen strides of a box against the dense ones: never dearer, inside the caps, every slot distinct and inside
// the image, and the chooser's figures those of image_cost on the slots it leads to
void check_box(ImageChooser &ch, const Box &B, int noff, uint64_t cap, const char *what)
{
    const ImageStrides d = ch.choose(B.s[0], B.s[1], B.s[2], B.own, B.halo, noff, cap, false),
                       c = ch.choose(B.s[0], B.s[1], B.s[2], B.own, B.halo, noff, cap);
    CHECK(d.px == B.s[0] + 2 && d.pxy == d.px * (B.s[1] + 2) && d.slots == d.pxy * (B.s[2] + 2), "%s", what);
    CHECK(c.cost() <= d.cost(), "%s: chosen %llu dense %llu", what, (unsigned long long)c.cost(), (unsigned long long)d.cost());
    CHECK(c.cost() < d.cost() || (c.px == d.px && c.pxy == d.pxy), "%s: a tie must keep the dense strides", what);
    CHECK(c.px >= d.px && c.pxy >= c.px * (B.s[1] + 2) && c.slots == c.pxy * (B.s[2] + 2), "%s", what);
    CHECK(c.slots <= cap && c.slots <= kImageMaxSlots, "%s: %u slots", what, c.slots);
    const std::vector<uint32_t> so = slots(B.own, c.px, c.pxy), sh = slots(B.halo, c.px, c.pxy);
    std::set<uint32_t> all(so.begin(), so.end());
    all.insert(sh.begin(), sh.end());
    CHECK(all.size() == so.size() + sh.size(), "%s: slots collide", what);
    CHECK(all.empty() || *all.rbegin() < c.slots, "%s: a slot outside the image", what);
    const ImageStrides m = image_cost(so.data(), so.size(), sh.data(), sh.size(), noff);
    CHECK(m.read == c.read && m.write == c.write, "%s: chooser %llu + %llu, model %llu + %llu", what,
          (unsigned long long)c.read, (unsigned long long)c.write, (unsigned long long)m.read, (unsigned long long)m.write);
}
}  // namespace

int main(int argc, char **argv)
{
    const unsigned step = argc > 1 ? (unsigned)std::max(1, std::atoi(argv[1])) : 1u;
    // the lane groups of a ds_read_b128: four of 16 lanes, {0-3, 12-15, 20-27} the first
    {
        unsigned n[4] = {};
        for (unsigned l = 0; l < 64; ++l)
            ++n[image_detail::read_group(l)];
        CHECK(n[0] == 16 && n[1] == 16 && n[2] == 16 && n[3] == 16, "group sizes");
        for (unsigned l : {0u, 3u, 12u, 15u, 20u, 27u})
            CHECK(image_detail::read_group(l) == 0 && image_detail::read_group(l + 32) == 2, "lane %u", l);
        for (unsigned l : {4u, 11u, 16u, 19u, 28u, 31u})
            CHECK(image_detail::read_group(l) == 1 && image_detail::read_group(l + 32) == 3, "lane %u", l);
        // 64 consecutive slots: conflict-free both ways; 64 lanes 16 slots apart: 16-way loads, 8-way stores
        std::vector<uint32_t> lin(65), str(64);
        for (unsigned l = 0; l < 65; ++l)
            lin[l] = 5 + l;
        for (unsigned l = 0; l < 64; ++l)
            str[l] = 16 * l;
        CHECK(image_read_cycles(lin.data(), 64) == 4 && image_write_cycles(lin.data(), 64) == 13, "linear");
        CHECK(image_read_cycles(str.data(), 64) == 64 && image_write_cycles(str.data(), 64) == 64, "strided");
        std::fill(str.begin(), str.end(), 7u);  // one address: a broadcast
        CHECK(image_read_cycles(str.data(), 64) == 4, "broadcast");
        CHECK(image_read_cycles(lin.data(), 65) == 8 && image_write_cycles(lin.data(), 1) == 13, "partial waves");
    }
    // C2: 70^3 nodes in 5 x 7 x 7 boxes of 14 x 10 x 10, the Kuhn stencil. The six kinds of box of the issue's table
    {
        const unsigned n[3] = {70, 70, 70}, g[3] = {5, 7, 7};
        const std::vector<Box> boxes = plan(n, g, false);
        const auto at = [&](unsigned bx, unsigned by, unsigned bz) -> const Box & { return boxes[(bz * 7 + by) * 5 + bx]; };
        const uint64_t floor = 22 * 14 * 4, cap = 8192;
        struct
        {
            const char *name;
            const Box &b;
            uint64_t dense;
        } kinds[] = {{"interior", at(2, 3, 3), 2464}, {"x-face", at(0, 3, 3), 4774}, {"y-face", at(2, 0, 3), 2464},
                     {"z-face", at(2, 3, 0), 2464},   {"x-y edge", at(0, 0, 3), 0},  {"corner", at(0, 0, 0), 0}};
        ImageChooser ch;
        for (const auto &k : kinds)
        {
            CHECK(k.b.s[0] == 14 && k.b.s[1] == 10 && k.b.s[2] == 10 && k.b.own.size() == 1400, "%s", k.name);
            const std::vector<uint32_t> so = slots(k.b.own, 16, 192), sh = slots(k.b.halo, 16, 192);
            const ImageStrides d = image_cost(so.data(), so.size(), sh.data(), sh.size(), 15);
            const ImageStrides c = ch.choose(14, 10, 10, k.b.own, k.b.halo, 15, cap);
            std::printf("%-9s dense read %llu write %llu; chosen (%u, %u) read %llu write %llu, %u slots\n", k.name,
                        (unsigned long long)d.read, (unsigned long long)d.write, c.px, c.pxy, (unsigned long long)c.read,
                        (unsigned long long)c.write, c.slots);
            if (k.dense)
                CHECK(d.read == k.dense, "%s: dense read cycles %llu", k.name, (unsigned long long)d.read);
            CHECK(c.read * 100 <= floor * 135, "%s: %llu read cycles", k.name, (unsigned long long)c.read);
            check_box(ch, k.b, 15, cap, k.name);
        }
        CHECK(ch.choose(14, 10, 10, at(2, 3, 3).own, at(2, 3, 3).halo, 15, cap).read == floor, "interior: the floor");
        // every box of the plan, and a cap that leaves no room: the dense strides stay
        for (const Box &b : boxes)
            check_box(ch, b, 15, cap, "C2");
        const ImageStrides t = ch.choose(14, 10, 10, at(0, 3, 3).own, at(0, 3, 3).halo, 15, 16 * 12 * 12);
        CHECK(t.px == 16 && t.pxy == 192, "tight cap: (%u, %u)", t.px, t.pxy);
    }
    // small boxes: sx 1..20 with (sy, sz) running through 1..20 each (sz = 7 sy mod 20 + 1), a 3 x 3 x 3 grid of them, so
    // a box inside the block, one on a block face of each axis and a corner box; Kuhn and hex8; the kernel's list
    // limits (2048 own, 1536 halo entries) and two caps
    for (unsigned sx = 1; sx <= 20; sx += step)
        for (unsigned sy = 1; sy <= 20; ++sy)
        {
            const unsigned sz = 7 * sy % 20 + 1;
            const unsigned n[3] = {3 * sx, 3 * sy, 3 * sz}, g[3] = {3, 3, 3};
            if (sx * sy * sz > 2048 || (sx + 2) * (sy + 2) * (sz + 2) - sx * sy * sz > 1536)
                continue;
            ImageChooser ch;
            for (int hex = 0; hex < 2; ++hex)
            {
                const std::vector<Box> boxes = plan(n, g, hex != 0);
                for (unsigned b : {13u, 12u, 10u, 22u, 0u, 26u})
                {
                    char what[64];
                    std::snprintf(what, sizeof what, "%ux%ux%u %s box %u", sx, sy, sz, hex ? "hex8" : "Kuhn", b);
                    CHECK(boxes[b].s[0] == sx && boxes[b].s[1] == sy && boxes[b].s[2] == sz, "%s", what);
                    check_box(ch, boxes[b], hex ? 27 : 15, b == 12u ? 5500 : 8192, what);
                }
            }
        }
    if (!fails)
        std::printf("ok\n");
    return fails ? 1 : 0;
}
