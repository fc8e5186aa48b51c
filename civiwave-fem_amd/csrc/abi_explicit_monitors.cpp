// abi_explicit_monitors.cpp -- what watches the explicit stepper (explicit_state.hpp): the node monitors
// (include/cwf_hip.h "Monitors": receiver traces, peak maps, the energy ledger) and the element monitors ("Element
// monitors": gauges and the stress / strain envelopes), with their share of a step's bookkeeping.
#include <algorithm>

#include "explicit_state.hpp"

using namespace cwf;

void cwf_hip_explicit::Monitors::sample(uint64_t steps, bool ledger_sampled, uint32_t blocks, const float *u,
                                        const float *v, hipStream_t st)
{
    if (ledger_sampled)
    {
        explicit_energy_fold(blocks, ecum, ecur, erows + 4 * esteps.size(), st);
        esteps.push_back(steps);
    }
    else if (eevery && steps % eevery == 0)
        ++edropped;
    if (rcount && steps % revery == 0)
    {
        if (rsteps.size() < rcap)
        {
            const size_t row = 3 * rcount * rsteps.size();
            explicit_record((uint32_t)rcount, rnode, u, v, ru + row, rv + row, st);
            rsteps.push_back(steps);
        }
        else
            ++rdropped;
    }
}

bool cwf_hip_explicit::ElementMonitors::arm(ExplicitElementPass &ep, uint64_t steps)
{
    if (!eevery && !gcount)
        return false;
    ep.von_mises = vm;
    ep.shear_strain = shear;
    ep.stress_range = range;
    ep.stride = stride;
    ep.gauge_count = (uint32_t)gcount;
    ep.gauge_elements = gelem;
    ep.envelope = eevery && steps % eevery == 0;
    ep.gauge_row = nullptr;
    if (gcount && steps % gevery == 0)
    {
        if (gsteps.size() < gcap)
            ep.gauge_row = grows + 13 * gcount * gsteps.size();
        else
            ++gdropped;
    }
    return true;
}

namespace
{
// the rows [first, first + count) of a table that holds held.size(): refused when out of range, else their step counts
int rows_in_range(cwf_hip_system *h, uint64_t first, uint64_t count, const std::vector<uint64_t> &held,
                  uint64_t *steps)
{
    if (first > held.size() || count > held.size() - first)
        return set_error(h, CWF_ERR_ARGUMENT, "monitor rows out of range",
                         "first=" + std::to_string(first) + "\ncount=" + std::to_string(count) +
                             "\nheld=" + std::to_string(held.size()));
    if (steps)
        std::copy(held.begin() + first, held.begin() + first + count, steps);
    return 0;
}

const uint32_t kBitsPlusInf = 0x7F800000u, kBitsMinusInf = 0xFF800000u;
const uint64_t kMaxBytes = 1ull << 44;  // no device holds more: a product past it is an allocation failure

// the maps at their start values: von Mises and shear strain +0.0, the stress minima +inf, the maxima -inf
hipError_t start_envelopes(const cwf_hip_explicit::ElementMonitors &m, hipStream_t s)
{
    hipError_t e = hipSuccess;
    if (m.vm)
        e = hipMemsetAsync(m.vm, 0, m.stride * sizeof(float), s);
    if (e == hipSuccess && m.shear)
        e = hipMemsetAsync(m.shear, 0, m.stride * sizeof(float), s);
    if (e == hipSuccess && m.range)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.range), (int)kBitsPlusInf, 6 * m.stride, s);
    if (e == hipSuccess && m.range)
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.range + 6 * m.stride), (int)kBitsMinusInf,
                              6 * m.stride, s);
    return e;
}
}  // namespace

// what cwf_hip_explicit_set_element_monitors refuses of a desc, on the host alone: 0, or the code with *msg and *ctx
int cwf::element_monitor_refusal(const cwf_explicit_element_monitor_desc &d, uint64_t E, std::string *msg,
                                 std::string *ctx)
{
    const auto no = [&](const char *m, std::string c = std::string()) {
        *msg = m;
        *ctx = std::move(c);
        return (int)CWF_ERR_ARGUMENT;
    };
    if (d.gauge_count && !d.gauge_elements)
        return no("null pointer");
    if (d.gauge_count && d.gauge_every < 1)
        return no("gauge_every must be at least 1");
    if (d.gauge_count && !d.gauge_capacity)
        return no("monitor capacity must not be zero", "gauge_capacity=" + std::to_string(d.gauge_capacity));
    const uint32_t known = CWF_ENVELOPE_VON_MISES | CWF_ENVELOPE_SHEAR_STRAIN | CWF_ENVELOPE_STRESS_RANGE;
    if (d.envelope_maps & ~known)
        return no("unknown envelope map", "maps=" + std::to_string(d.envelope_maps));
    if (d.envelope_maps && !d.envelope_every)
        return no("envelope_maps without envelope_every", "maps=" + std::to_string(d.envelope_maps));
    if (d.envelope_every && !d.envelope_maps)
        return no("envelope_every without envelope_maps", "envelope_every=" + std::to_string(d.envelope_every));
    std::vector<bool> seen(d.gauge_count ? E : 0, false);
    for (uint64_t i = 0; i < d.gauge_count; ++i)
    {
        const uint32_t e = d.gauge_elements[i];
        if (e >= E)
            return no("gauge element out of range", "index=" + std::to_string(i) + "\nelement=" + std::to_string(e));
        if (seen[e])
            return no("gauge element listed twice", "index=" + std::to_string(i) + "\nelement=" + std::to_string(e));
        seen[e] = true;
    }
    return 0;
}

extern "C" {

int cwf_hip_explicit_set_monitors(cwf_hip_explicit *t, const cwf_explicit_monitor_desc *desc)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_explicit_monitor_desc none{};
    const cwf_explicit_monitor_desc &d = desc ? *desc : none;
    const uint64_t N = h->ds.N;
    // everything that can be refused, on the host, before anything changes
    if (d.receiver_count && !d.receiver_nodes)
        return set_error(h, CWF_ERR_ARGUMENT, "null pointer");
    if (d.receiver_count && d.receiver_every < 1)
        return set_error(h, CWF_ERR_ARGUMENT, "receiver_every must be at least 1");
    if ((d.receiver_count && !d.receiver_capacity) || (d.energy_every && !d.energy_capacity))
        return set_error(h, CWF_ERR_ARGUMENT, "monitor capacity must not be zero",
                         "receiver_capacity=" + std::to_string(d.receiver_capacity) +
                             "\nenergy_capacity=" + std::to_string(d.energy_capacity));
    if (d.energy_every && t->beta != 0.0)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger needs rayleigh_beta == 0",
                         "rayleigh_beta=" + num17(t->beta));
    if (d.energy_every && t->pl.dev.slots)
        return set_error(h, CWF_ERR_UNSUPPORTED, "the energy ledger and plasticity exclude each other",
                         "plastic_elements=" + std::to_string(t->pl.dev.slots));
    std::vector<uint32_t> slot(d.receiver_count ? std::max<uint64_t>(N, 4) : 0, kNoSlot);
    if (int st = nodes_listed_once(h, "receiver node", "", d.receiver_nodes, d.receiver_count, slot, 0))
        return st;
    for (uint64_t i = 0; i < d.receiver_count; ++i)
        slot[d.receiver_nodes[i]] = (uint32_t)i;
    if (d.receiver_count && d.receiver_capacity > kMaxBytes / (12 * d.receiver_count))
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    if (d.energy_every && d.energy_capacity > kMaxBytes / 32)
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    HIPTRY(h, hipStreamSynchronize(h->stream));
    // the new set's buffers; the stepper's once everything went well
    ArenaStage stage(*t);
    cwf_hip_explicit::Monitors m;
    std::vector<uint32_t> back, rnode(d.receiver_count);  // the receivers' nodes in the internal order
    if (d.receiver_count)
    {
        m.rcount = d.receiver_count;
        m.revery = d.receiver_every;
        m.rcap = d.receiver_capacity;
        const size_t cells = (size_t)(3 * m.rcount * m.rcap);
        m.ru = stage.alloc<float>(cells);
        m.rv = stage.alloc<float>(cells);
        if (stage.ok())
            if (int st = slots_to_internal(*t, slot, nullptr, &back))
                return st;
        for (uint64_t n = 0; n < back.size(); ++n)
            if (back[n] != kNoSlot)
                rnode[back[n]] = (uint32_t)n;
        m.rnode = stage.put(rnode);
    }
    if (d.peaks)
    {
        m.peak_stride = std::max<uint64_t>(N, 4);
        m.peak = stage.zeros<float>(3 * m.peak_stride);
    }
    if (d.energy_every)
    {
        const size_t blocks = explicit_update_blocks((uint32_t)N);
        m.eevery = d.energy_every;
        m.ecap = d.energy_capacity;
        m.ecum = stage.zeros<double>(2 * blocks);
        m.ecur = stage.zeros<double>(2 * blocks);
        m.erows = stage.alloc<double>(4 * (size_t)m.ecap);
    }
    if (int st = stage.finish("explicit set_monitors"))
        return st;
    if (int st = t->sync_ledger_C(m.ecum != nullptr, t->dash_C, "explicit set_monitors"))
        return st;
    m.rsteps.reserve((size_t)std::min<uint64_t>(m.rcap, 1u << 20));
    m.esteps.reserve((size_t)std::min<uint64_t>(m.ecap, 1u << 20));
    m.held = stage.adopt();
    t->mon.release(t->mem);
    t->mon = std::move(m);
    return 0;
}

int cwf_hip_explicit_reset_monitors(cwf_hip_explicit *t)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    cwf_hip_explicit::Monitors &m = t->mon;
    const size_t blocks = explicit_update_blocks(h->ds.N);
    if (m.peak)
        HIPTRY(h, hipMemsetAsync(m.peak, 0, 3 * m.peak_stride * sizeof(float), h->stream));
    if (m.ecum)
    {
        HIPTRY(h, hipMemsetAsync(m.ecum, 0, 2 * blocks * sizeof(double), h->stream));
        HIPTRY(h, hipMemsetAsync(m.ecur, 0, 2 * blocks * sizeof(double), h->stream));
    }
    HIPTRY(h, hipStreamSynchronize(h->stream));
    m.rsteps.clear();
    m.esteps.clear();
    m.rdropped = m.edropped = 0;
    return 0;
}

int cwf_hip_explicit_monitor_info(cwf_hip_explicit *t, cwf_explicit_monitor_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const cwf_hip_explicit::Monitors &m = t->mon;
    cwf_explicit_monitor_info I{};
    I.receiver_count = m.rcount;
    I.receiver_every = m.revery;
    I.receiver_capacity = m.rcap;
    I.receiver_samples = m.rsteps.size();
    I.receiver_dropped = m.rdropped;
    I.energy_every = m.eevery;
    I.energy_capacity = m.ecap;
    I.energy_samples = m.esteps.size();
    I.energy_dropped = m.edropped;
    I.peaks = m.peak ? 1u : 0u;
    *info = I;
    return 0;
}

int cwf_hip_explicit_read_receivers(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, float *u,
                                    float *v)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (int st = rows_in_range(h, first, count, m.rsteps, steps))
        return st;
    if (!count)
        return 0;
    const size_t off = (size_t)(3 * m.rcount * first), len = (size_t)(3 * m.rcount * count) * sizeof(float);
    if (u)
        HIPTRY(h, hipMemcpyAsync(u, m.ru + off, len, hipMemcpyDeviceToHost, h->stream));
    if (v)
        HIPTRY(h, hipMemcpyAsync(v, m.rv + off, len, hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_peaks(cwf_hip_explicit *t, float *peak_u, float *peak_v, float *peak_a, uint64_t n, int kind)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (!m.peak)
        return set_error(h, CWF_ERR_ARGUMENT, "no peak maps are set");
    if (n != h->ds.N)
        return set_error(h, CWF_ERR_SIZE, "peak map span size mismatch",
                         "span=" + std::to_string(n) + "\nnodes=" + std::to_string(h->ds.N));
    float *out[3] = {peak_u, peak_v, peak_a};
    for (int j = 0; j < 3; ++j)
        if (out[j])
            if (int st = vec_out(h, m.peak + j * m.peak_stride, out[j], kind, 1))
                return st;
    HIPTRY(h, hipGetLastError());
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_energy(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, double *rows)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_hip_explicit::Monitors &m = t->mon;
    if (int st = rows_in_range(h, first, count, m.esteps, steps))
        return st;
    if (!count)
        return 0;
    if (rows)
        HIPTRY(h, hipMemcpyAsync(rows, m.erows + 4 * first, 4 * count * sizeof(double), hipMemcpyDeviceToHost,
                                 h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_set_element_monitors(cwf_hip_explicit *t, const cwf_explicit_element_monitor_desc *desc)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_explicit_element_monitor_desc none{};
    const cwf_explicit_element_monitor_desc &d = desc ? *desc : none;
    const uint64_t E = h->ds.E;
    // everything that can be refused, on the host, before anything changes
    std::string msg, ctx;
    if (int code = element_monitor_refusal(d, E, &msg, &ctx))
        return set_error(h, code, msg, ctx);
    if (d.gauge_count && d.gauge_capacity > kMaxBytes / (52 * d.gauge_count))
        return set_error(h, CWF_ERR_ALLOC, t->alloc_error);
    HIPTRY(h, hipStreamSynchronize(h->stream));
    // the new set's buffers; the stepper's once everything went well
    ArenaStage stage(*t);
    cwf_hip_explicit::ElementMonitors m;
    if (d.gauge_count)
    {
        m.gcount = d.gauge_count;
        m.gevery = d.gauge_every;
        m.gcap = d.gauge_capacity;
        m.gelem = stage.put(d.gauge_elements, m.gcount);  // elements keep the caller's numbering: the ids go up as given
        m.grows = stage.alloc<float>((size_t)(13 * m.gcount * m.gcap));
    }
    if (d.envelope_every)
    {
        m.eevery = d.envelope_every;
        m.maps = d.envelope_maps;
        m.stride = std::max<uint64_t>(E, 4);
        if (m.maps & CWF_ENVELOPE_VON_MISES)
            m.vm = stage.alloc<float>(m.stride);
        if (m.maps & CWF_ENVELOPE_SHEAR_STRAIN)
            m.shear = stage.alloc<float>(m.stride);
        if (m.maps & CWF_ENVELOPE_STRESS_RANGE)
            m.range = stage.alloc<float>(12 * m.stride);
    }
    if (stage.ok())
        stage.check(start_envelopes(m, h->stream));
    if (int st = stage.finish("explicit set_element_monitors"))
        return st;
    m.gsteps.reserve((size_t)std::min<uint64_t>(m.gcap, 1u << 20));
    m.held = stage.adopt();
    t->emon.release(t->mem);
    t->emon = std::move(m);
    return 0;
}

int cwf_hip_explicit_reset_element_monitors(cwf_hip_explicit *t)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    cwf_hip_explicit::ElementMonitors &m = t->emon;
    HIPTRY(h, start_envelopes(m, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    m.gsteps.clear();
    m.gdropped = m.esamples = 0;
    return 0;
}

int cwf_hip_explicit_element_monitor_info(cwf_hip_explicit *t, cwf_explicit_element_monitor_info *info)
{
    if (!t || !info)
        return set_error(nullptr, CWF_ERR_ARGUMENT, "null pointer");
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    cwf_explicit_element_monitor_info I{};
    I.gauge_count = m.gcount;
    I.gauge_every = m.gevery;
    I.gauge_capacity = m.gcap;
    I.gauge_samples = m.gsteps.size();
    I.gauge_dropped = m.gdropped;
    I.envelope_every = m.eevery;
    I.envelope_samples = m.esamples;
    I.envelope_maps = m.maps;
    *info = I;
    return 0;
}

int cwf_hip_explicit_read_gauges(cwf_hip_explicit *t, uint64_t first, uint64_t count, uint64_t *steps, float *rows)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    if (int st = rows_in_range(h, first, count, m.gsteps, steps))
        return st;
    if (!count)
        return 0;
    if (rows)
        HIPTRY(h, hipMemcpyAsync(rows, m.grows + 13 * m.gcount * first, (size_t)(13 * m.gcount * count) * sizeof(float),
                                 hipMemcpyDeviceToHost, h->stream));
    HIPTRY(h, hipStreamSynchronize(h->stream));
    return 0;
}

int cwf_hip_explicit_read_envelopes(cwf_hip_explicit *t, float *von_mises, float *shear_strain, float *stress_min,
                                    float *stress_max, uint64_t n, int kind)
{
    if (int st = explicit_ready(t))
        return st;
    cwf_hip_system *h = t->sys;
    const cwf_hip_explicit::ElementMonitors &m = t->emon;
    if ((von_mises && !m.vm) || (shear_strain && !m.shear) || ((stress_min || stress_max) && !m.range))
        return set_error(h, CWF_ERR_ARGUMENT, "envelope map is not set", "maps=" + std::to_string(m.maps));
    const uint64_t E = h->ds.E;
    if (n != E)
        return set_error(h, CWF_ERR_SIZE, "envelope map span size mismatch",
                         "span=" + std::to_string(n) + "\nelements=" + std::to_string(E));
    hipStream_t s = h->stream;
    const hipMemcpyKind back = kind == CWF_PTR_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (von_mises)
        HIPTRY(h, hipMemcpyAsync(von_mises, m.vm, E * sizeof(float), back, s));
    if (shear_strain)
        HIPTRY(h, hipMemcpyAsync(shear_strain, m.shear, E * sizeof(float), back, s));
    // the stress range: plane c of the device layout is column c of the caller's [E][6]
    float *const out[2] = {stress_min, stress_max};
    std::vector<float> plane;
    for (int q = 0; q < 2; ++q)
    {
        if (!out[q])
            continue;
        const float *src = m.range + 6 * q * m.stride;
        if (kind == CWF_PTR_DEVICE)
        {
            for (int c = 0; c < 6; ++c)
                HIPTRY(h, hipMemcpy2DAsync(out[q] + c, 6 * sizeof(float), src + c * m.stride, sizeof(float),
                                           sizeof(float), E, hipMemcpyDeviceToDevice, s));
            continue;
        }
        plane.resize(6 * m.stride);
        HIPTRY(h, hipMemcpyAsync(plane.data(), src, plane.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPTRY(h, hipStreamSynchronize(s));
        for (uint64_t e = 0; e < E; ++e)
            for (int c = 0; c < 6; ++c)
                out[q][6 * e + c] = plane[c * m.stride + e];
    }
    HIPTRY(h, hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
