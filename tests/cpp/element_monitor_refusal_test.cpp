// element_monitor_refusal_test.cpp -- what cwf_hip_explicit_set_element_monitors refuses of a desc, on the host alone
// (element_monitor_refusal, abi_internal.hpp): every message with its context, the order of the checks, and the descs
// that pass. No GPU call.
#include <cstdio>
#include <string>
#include <vector>

#include "abi_internal.hpp"

namespace
{
int failures = 0;

void expect(const char *what, const cwf_explicit_element_monitor_desc &d, uint64_t E, int code, const std::string &msg,
            const std::string &ctx)
{
    std::string m = "untouched", c = "untouched";
    const int got = cwf::element_monitor_refusal(d, E, &m, &c);
    const bool ok = code ? (got == code && m == msg && c == ctx) : (got == 0 && m == "untouched" && c == "untouched");
    if (!ok)
    {
        std::printf("FAIL %s: code %d message '%s' context '%s'\n", what, got, m.c_str(), c.c_str());
        ++failures;
    }
}
}  // namespace

int main()
{
    const int arg = CWF_ERR_ARGUMENT;
    const uint64_t E = 432;
    const std::vector<uint32_t> good = {431, 0, 256, 255};
    cwf_explicit_element_monitor_desc d{};
    expect("all zero", d, E, 0, "", "");
    expect("all zero, no elements", d, 0, 0, "", "");
    d = {good.size(), good.data(), 1, 8, 0, 0, 0};
    expect("gauges", d, E, 0, "", "");
    d = {0, nullptr, 0, 0, 5, CWF_ENVELOPE_VON_MISES | CWF_ENVELOPE_SHEAR_STRAIN | CWF_ENVELOPE_STRESS_RANGE, 0};
    expect("envelopes", d, E, 0, "", "");
    d = {good.size(), good.data(), 3, 1, 1, CWF_ENVELOPE_STRESS_RANGE, 0};
    expect("both", d, E, 0, "", "");

    d = {good.size(), nullptr, 1, 8, 0, 0, 0};
    expect("null gauges", d, E, arg, "null pointer", "");
    d = {good.size(), good.data(), 0, 8, 0, 0, 0};
    expect("every 0", d, E, arg, "gauge_every must be at least 1", "");
    d = {good.size(), good.data(), 1, 0, 0, 0, 0};
    expect("capacity 0", d, E, arg, "monitor capacity must not be zero", "gauge_capacity=0");
    d = {0, nullptr, 0, 0, 1, 8u, 0};
    expect("unknown map", d, E, arg, "unknown envelope map", "maps=8");
    d = {0, nullptr, 0, 0, 1, 0x80000001u, 0};
    expect("unknown high bit", d, E, arg, "unknown envelope map", "maps=2147483649");
    d = {0, nullptr, 0, 0, 0, CWF_ENVELOPE_VON_MISES, 0};
    expect("maps without every", d, E, arg, "envelope_maps without envelope_every", "maps=1");
    d = {0, nullptr, 0, 0, 7, 0, 0};
    expect("every without maps", d, E, arg, "envelope_every without envelope_maps", "envelope_every=7");
    const std::vector<uint32_t> past = {3, 431, 432};
    d = {past.size(), past.data(), 1, 8, 0, 0, 0};
    expect("out of range", d, E, arg, "gauge element out of range", "index=2\nelement=432");
    expect("in range of a larger mesh", d, E + 1, 0, "", "");
    const std::vector<uint32_t> top = {0xFFFFFFFFu};
    d = {top.size(), top.data(), 1, 8, 0, 0, 0};
    expect("the largest id", d, E, arg, "gauge element out of range", "index=0\nelement=4294967295");
    const std::vector<uint32_t> twice = {3, 9, 431, 9};
    d = {twice.size(), twice.data(), 1, 8, 0, 0, 0};
    expect("listed twice", d, E, arg, "gauge element listed twice", "index=3\nelement=9");
    // the gauge's own fields are checked before its ids, the envelope's fields before the ids too
    d = {twice.size(), twice.data(), 0, 8, 0, 0, 0};
    expect("every before ids", d, E, arg, "gauge_every must be at least 1", "");
    d = {twice.size(), twice.data(), 1, 8, 0, CWF_ENVELOPE_VON_MISES, 0};
    expect("envelope before ids", d, E, arg, "envelope_maps without envelope_every", "maps=1");
    // a handle without elements has no valid gauge
    d = {1, good.data() + 1, 1, 8, 0, 0, 0};
    expect("no elements", d, 0, arg, "gauge element out of range", "index=0\nelement=0");
    if (failures)
        return 1;
    std::printf("ok\n");
    return 0;
}
