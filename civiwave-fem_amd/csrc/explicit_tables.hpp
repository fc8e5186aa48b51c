// explicit_tables.hpp -- the two index tables of the explicit stepper that are pure functions of host arrays
// (explicit_tables.cpp): the load sources' CSR (abi_explicit_loads.cpp uploads it) and plasticity's slots with their
// node-major corner positions (abi_explicit_plasticity.cpp). Neither file needs a HIP header, so
// tests/cpp/explicit_tables_test.cpp builds them with the host compiler alone.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/cwf_hip.h"

namespace cwf
{

// ExplicitSources' arrays (cwf_internal.hpp) on the host
struct SourceTables
{
    std::vector<uint32_t> off;  // [L + 1] a loaded node's entries
    std::vector<uint32_t> dir;  // [entries] 8 B: where the entry's curve starts in tab, and its points
    std::vector<double> rec;    // [entries] 32-B records: A_0 A_1 A_2 tau
    std::vector<double> tab;    // per source its times, then its values
    uint64_t entries = 0, points = 0;
};
// slot: caller's node -> its index among the loaded nodes (first listing first); rank [L]: that index -> the node's
// place l in the internal node order. The entries go in source by source, so a node's entries ascend in source index.
// The descs are taken as checked (cwf_hip_explicit_set_sources refuses before it calls this).
SourceTables source_tables(const cwf_explicit_source_desc *sources, uint32_t count, const std::vector<uint32_t> &slot,
                           const std::vector<uint32_t> &rank);

// ExplicitPlasticity's index arrays on the host. A slot is a plastic element (ascending element index). Position q of
// the corner array is the q-th plastic incidence in node order, so a node's run ascends in element; cpos tells each
// slot where its four corners go. All empty when no element is plastic.
struct PlasticTables
{
    std::vector<uint32_t> elem;   // [slots] the slot's element
    std::vector<uint32_t> anode;  // [affected] the nodes with a plastic incidence, ascending
    std::vector<uint32_t> aoff;   // [affected + 1] the node's run in the corner array
    std::vector<uint32_t> cpos;   // [4 slots]
    uint64_t incidences = 0;      // plastic incidences met: 4 slots when every corner is some node's incidence, once
};
// mat [E], the node -> incidence CSR off [N + 1] / inc (element << 2 | corner, ascending in element per node) and the
// per-material plastic flags. Returns non-zero when the incidences do not cover every corner of every slot once.
int plastic_tables(const std::vector<uint32_t> &mat, const std::vector<uint32_t> &off,
                   const std::vector<uint32_t> &inc, const std::vector<uint8_t> &plastic, PlasticTables *out);

}  // namespace cwf
