// devmem_test.cpp -- DeviceLedger (csrc/devmem.hpp), the host bookkeeping under every DeviceArena, on made-up
// pointers: the total after each adopt, release returning the recorded bytes and removing exactly one entry, an
// unknown pointer changing nothing, the first / a middle / the last entry leaving and the others staying, and an
// adopt after releases counted once. No GPU call, no library: prints "ok" or the first failed check.
#include <cstdio>
#include <cstdlib>

#include "devmem.hpp"

#define CHECK(cond)                                                                                            \
    do                                                                                                         \
    {                                                                                                          \
        if (!(cond))                                                                                           \
        {                                                                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                              \
            return 1;                                                                                          \
        }                                                                                                      \
    } while (0)

int main()
{
    using cwf::DeviceLedger;
    static char pool[8];  // eight distinct addresses, never dereferenced
    void *p[8];
    for (int i = 0; i < 8; ++i)
        p[i] = &pool[i];
    const size_t bytes[5] = {16, 4096, 48, 1u << 20, 16};

    static_assert(cwf::device_bytes<float>(0) == 16 && cwf::device_bytes<float>(3) == 16 &&
                      cwf::device_bytes<float>(4) == 16 && cwf::device_bytes<float>(5) == 20 &&
                      cwf::device_bytes<double>(2) == 16 && cwf::device_bytes<double>(3) == 24,
                  "one 16-B floor");

    DeviceLedger L;
    CHECK(L.total() == 0 && L.count() == 0);
    size_t sum = 0;
    for (int i = 0; i < 5; ++i)  // the total after each adopt
    {
        L.adopt(p[i], bytes[i]);
        sum += bytes[i];
        CHECK(L.total() == sum && L.count() == (size_t)i + 1);
        CHECK(L.size_of(p[i]) == bytes[i]);
    }

    // an unknown pointer: 0, nothing changes
    CHECK(L.release(p[7]) == 0 && L.release(nullptr) == 0);
    CHECK(L.total() == sum && L.count() == 5 && L.size_of(p[7]) == 0);

    // a middle entry: its bytes, exactly one entry less, the others as they were
    CHECK(L.release(p[2]) == bytes[2]);
    sum -= bytes[2];
    CHECK(L.total() == sum && L.count() == 4 && L.size_of(p[2]) == 0);
    CHECK(L.size_of(p[0]) == bytes[0] && L.size_of(p[1]) == bytes[1] && L.size_of(p[3]) == bytes[3] &&
          L.size_of(p[4]) == bytes[4]);
    CHECK(L.release(p[2]) == 0 && L.total() == sum && L.count() == 4);  // a second release finds nothing

    // the first entry
    CHECK(L.release(p[0]) == bytes[0]);
    sum -= bytes[0];
    CHECK(L.total() == sum && L.count() == 3);
    CHECK(L.size_of(p[1]) == bytes[1] && L.size_of(p[3]) == bytes[3] && L.size_of(p[4]) == bytes[4]);

    // the last entry
    CHECK(L.release(p[4]) == bytes[4]);
    sum -= bytes[4];
    CHECK(L.total() == sum && L.count() == 2);
    CHECK(L.size_of(p[1]) == bytes[1] && L.size_of(p[3]) == bytes[3]);
    CHECK(L.at(0) == p[1] && L.at(1) == p[3]);  // adopt order kept

    // an adopt after releases (a freed address may come back from the allocator): counted once
    L.adopt(p[2], 80);
    sum += 80;
    CHECK(L.total() == sum && L.count() == 3 && L.size_of(p[2]) == 80);
    CHECK(L.release(p[2]) == 80 && L.total() == sum - 80 && L.count() == 2);
    sum -= 80;

    CHECK(L.release(p[1]) == bytes[1] && L.release(p[3]) == bytes[3]);
    CHECK(L.total() == 0 && L.count() == 0);
    std::printf("ok\n");
    return 0;
}
