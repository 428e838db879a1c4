// What the two Merkle builders share (utxo_merkle.hip on the device, utxo_merkle_host.cpp on the host): the snapshot,
// its registry and the level layout. The definition of the tree is in native.h. No HIP types here: the host twin is
// plain C++ and links without the device file.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "native.h"

namespace upow {

// Every level lives in one array of 32-byte nodes: level l (0: the leaves) holds size[l] nodes from node off[l],
// each level starting at an even node (64-byte aligned) so that a pair of children is one aligned 64-byte line.
// Fewer than 2 n + 32 nodes in all.
struct MerkleLevels {
    std::vector<uint64_t> off, size;
    uint64_t nodes = 0;
    explicit MerkleLevels(uint64_t n) {
        for (uint64_t s = n; s; s = (s + 1) / 2) {
            off.push_back(nodes);
            size.push_back(s);
            nodes += (s + 1) & ~uint64_t(1);
            if (s == 1) break;
        }
    }
};

struct MerkleSnap {
    uint64_t count = 0, bytes = 0;
    MerkleLevels lv{0};
    uint8_t root[32];
    // host twin: the slots and the nodes
    std::vector<uint8_t> h_slots, h_nodes;
    // device: one allocation, the nodes first, then the slots and the level table; the device file sets the two hooks
    int device = -1;
    uint8_t* d_arena = nullptr;
    uint64_t d_slots_off = 0, d_table_off = 0;
    // lower bounds of q queries (34-byte keys: txid | index | 0) and, per wanted leaf, its slot and its path laid
    // out as one row of (levels - 1) x 32 bytes, a sibling that does not exist left untouched
    void (*d_search)(const MerkleSnap&, const uint8_t* recs, int64_t q, uint32_t* lb, uint32_t* matches) = nullptr;
    void (*d_gather)(const MerkleSnap&, const std::vector<uint32_t>& pos, uint8_t* slots, uint8_t* rows) = nullptr;
    void (*d_release)(MerkleSnap&) = nullptr;
    ~MerkleSnap() {
        if (d_release) d_release(*this);
    }
};

// the registry (utxo_merkle_host.cpp)
int64_t merkle_register(std::shared_ptr<MerkleSnap> s);
// SHA-256 of the empty string: the root of the empty set
void merkle_empty_root(uint8_t out[32]);

}  // namespace upow
