// ties_tables.hpp -- the index tables of the explicit stepper's tied boundaries that are pure functions of host arrays
// (ties_tables.cpp; abi_explicit_ties.cpp uploads them): the slot and group words the update pass reads, which dashpots
// and ties share, and the groups' CSR in the handle's internal node order. No HIP header is needed, so
// tests/cpp/ties_tables_test.cpp builds the unit with the host compiler alone.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace cwf
{

constexpr uint32_t kTieNone = 0xFFFFFFFFu;  // == kNoSlot / kNoDashpot

// What set_ties refuses of a set on the host alone, for a handle of N nodes whose caller-order masks are mask [N]
// (NULL: the masks are not checked): 0, or 1 with the message and its context lines. The checks run in this order:
// offsets ("tie offsets must ascend from 0" {group}), sizes ("tie group needs at least two nodes" {group, nodes}), ids
// ("tied node out of range" / "tied node listed twice" {index, node}, across all groups), masks ("tied nodes differ in
// their constraints" {group, node, mask, first_mask}).
int tie_refusal(uint64_t N, const uint32_t *mask, uint64_t groups, const uint64_t *offsets, const uint32_t *ids,
                std::string *msg, std::string *ctx);

// The id check of tie_refusal on its own, for the host helpers of ties.cpp too (nodes_listed_once of the stepper's units
// needs a handle and HIP's headers, which this unit does without): every id below N and not yet in seen [N], which it
// marks; else 1 with "tied node out of range" / "tied node listed twice" and "<prefix>index=i\nnode=n".
int tied_ids_once(uint64_t N, const uint32_t *ids, uint64_t count, std::vector<uint8_t> &seen, const std::string &prefix,
                  std::string *msg, std::string *ctx);

// A node with a dashpot or in a tie group owns a slot. Slots 0 .. dash_count - 1 are the dashpot nodes in the order
// given (so the ledger's copy of C, indexed by the dashpot's position, is indexed by the slot); the tied nodes without
// a dashpot follow in list order. Either call order of set_dashpots and set_ties therefore ends in the same words.
struct TieSlots
{
    std::vector<uint32_t> slot;   // [max(N, 4)] caller's node -> slot, kTieNone for a node without one
    std::vector<uint32_t> node;   // [slots] slot -> caller's node
    std::vector<uint32_t> group;  // [slots] slot -> its tie group, kTieNone for an untied dashpot node
    uint32_t dash_slots = 0;      // slots below this one carry a dashpot
};
// the ids are taken as checked (distinct within each list, below N)
TieSlots tie_slots(uint64_t N, const uint32_t *dash_ids, uint64_t dash_count, uint64_t groups, const uint64_t *offsets,
                   const uint32_t *ids);

// The groups' CSR in the internal node order: tnode[j] is the internal node of member j, members in list order (the
// gather kernel's summation order). back [N]: internal node -> slot (the slot words after the permutation). Returns
// non-zero when a tied node's slot is not met exactly once in back.
struct TieCsr
{
    std::vector<uint32_t> toff;   // [groups + 1]
    std::vector<uint32_t> tnode;  // [members]
};
int tie_csr(const TieSlots &s, const std::vector<uint32_t> &back, uint64_t groups, const uint64_t *offsets,
            const uint32_t *ids, TieCsr *out);

// f32(sum f64(m_i) f64(v_i) / M_G) per group and component into every member's v [3N] (caller's order), the sums in
// member order from the first term; M_G = sum f64(m_i) likewise. Components constrained by the group's mask stay 0.
void tie_project(uint64_t groups, const uint64_t *offsets, const uint32_t *ids, const float *mass, const uint32_t *mask,
                 float *v);

}  // namespace cwf
