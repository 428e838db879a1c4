// UTXO proofs on the host: the Merkle tree of key records + payloads (the definition is in native.h; the GPU passes are
// csrc/utxo_merkle.hip), the snapshot registry, and what a proof needs after the search and the gather, which is the
// same for both. One or two compressions per leaf, two per inner node.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <numeric>
#include <stdexcept>
#include <unordered_map>

#include "sha256_common.h"
#include "thread_pool.h"
#include "utxo_merkle.h"

namespace upow {

namespace {

std::mutex g_mu;
std::unordered_map<int64_t, std::shared_ptr<MerkleSnap>> g_snaps;
int64_t g_next = 1;

std::shared_ptr<MerkleSnap> snap(int64_t id) {
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_snaps.find(id);
    if (it == g_snaps.end()) throw std::invalid_argument("bad Merkle snapshot id");
    return it->second;
}

// the 112-byte slot of one entry: E, zeros up to byte 108, u32le(length of E)
void make_slot(const uint8_t* rec, const uint8_t* pay, uint8_t* slot) {
    std::memset(slot, 0, kMerkleSlot);
    std::memcpy(slot, rec, 32);
    slot[32] = rec[32];  // u8(index), u8(tag): the low bytes of the record's little-endian words
    slot[33] = rec[36];
    uint32_t len = 0;
    if (pay) {
        uint32_t l;
        std::memcpy(&l, pay + 8, 4);
        if (l == 33 || l == 64) {
            len = l;
            slot[34] = pay[12] & 1;
            std::memcpy(slot + 36, pay, 8);
            std::memcpy(slot + 44, pay + 16, len);
        }
    }
    slot[35] = uint8_t(len);
    const uint32_t total = 44 + len;
    std::memcpy(slot + 108, &total, 4);  // (little-endian hosts only, as the record layout is)
}

void leaf_hash(const uint8_t* slot, uint8_t out[32]) {
    uint32_t total;
    std::memcpy(&total, slot + 108, 4);
    uint8_t m[109];
    m[0] = 0x00;
    std::memcpy(m + 1, slot, total);
    host_sha256(m, 1 + total, out);
}

void node_hash(const uint8_t* pair, uint8_t out[32]) {
    uint8_t m[65];
    m[0] = 0x01;
    std::memcpy(m + 1, pair, 64);
    host_sha256(m, 65, out);
}

}  // namespace

int64_t merkle_register(std::shared_ptr<MerkleSnap> s) {
    std::lock_guard<std::mutex> g(g_mu);
    const int64_t id = g_next++;
    g_snaps[id] = std::move(s);
    return id;
}

void merkle_empty_root(uint8_t out[32]) { host_sha256(nullptr, 0, out); }

int64_t utxo_merkle_build_records_host(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, int threads) {
    if (n < 0 || n > int64_t(0x7fffffff)) throw std::invalid_argument("record count must be in [0, 2^31)");
    auto s = std::make_shared<MerkleSnap>();
    s->count = uint64_t(n);
    s->lv = MerkleLevels(uint64_t(n));
    merkle_empty_root(s->root);
    if (n) {
        HostPool& pool = HostPool::get();
        std::vector<uint8_t> unsorted(size_t(n) * kMerkleSlot);
        pool.parallel_for(n, threads, [&](int64_t i) {
            make_slot(recs + 40 * i, pay_or_null ? pay_or_null + 80 * i : nullptr, &unsorted[size_t(i) * kMerkleSlot]);
        });
        std::vector<uint32_t> order(size_t(n), 0);
        std::iota(order.begin(), order.end(), 0u);
        // by E's first 34 bytes; equal keys (the same entry twice) keep their input order
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            return std::memcmp(&unsorted[size_t(a) * kMerkleSlot], &unsorted[size_t(b) * kMerkleSlot], 34) < 0;
        });
        s->h_slots.resize(size_t(n) * kMerkleSlot);
        s->h_nodes.assign(size_t(s->lv.nodes) * 32, 0);
        pool.parallel_for(n, threads, [&](int64_t i) {
            uint8_t* slot = &s->h_slots[size_t(i) * kMerkleSlot];
            std::memcpy(slot, &unsorted[size_t(order[size_t(i)]) * kMerkleSlot], kMerkleSlot);
            leaf_hash(slot, &s->h_nodes[size_t(i) * 32]);
        });
        for (size_t l = 0; l + 1 < s->lv.size.size(); ++l) {
            const uint8_t* below = &s->h_nodes[size_t(s->lv.off[l]) * 32];
            uint8_t* above = &s->h_nodes[size_t(s->lv.off[l + 1]) * 32];
            const uint64_t size = s->lv.size[l];
            pool.parallel_for(int64_t(s->lv.size[l + 1]), threads, [&](int64_t p) {
                if (2 * uint64_t(p) + 1 < size) node_hash(below + 64 * p, above + 32 * p);
                else std::memcpy(above + 32 * p, below + 64 * p, 32);  // the unpaired last node is promoted
            });
        }
        std::memcpy(s->root, &s->h_nodes[size_t(s->lv.off.back()) * 32], 32);
    }
    s->bytes = s->h_slots.size() + s->h_nodes.size();
    return merkle_register(std::move(s));
}

MerkleInfo utxo_merkle_info(int64_t id) {
    const std::shared_ptr<MerkleSnap> s = snap(id);
    MerkleInfo r;
    std::memcpy(r.root, s->root, 32);
    r.count = s->count;
    r.bytes = s->bytes;
    r.levels = uint32_t(s->lv.size.size());
    r.on_device = s->d_arena != nullptr;
    return r;
}

void utxo_merkle_free(int64_t id) {
    std::shared_ptr<MerkleSnap> s;  // released outside the registry lock
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_snaps.find(id);
    if (it == g_snaps.end()) return;
    s = std::move(it->second);
    g_snaps.erase(it);
}

void utxo_merkle_held(uint64_t* snapshots, uint64_t* bytes) {
    std::lock_guard<std::mutex> g(g_mu);
    *snapshots = g_snaps.size();
    *bytes = 0;
    for (const auto& kv : g_snaps) *bytes += kv.second->bytes;
}

void utxo_merkle_prove(int64_t id, const uint8_t* recs, int64_t q, MerkleProveOut& out) {
    if (q < 0 || q > int64_t(1) << 24) throw std::invalid_argument("query count must be in [0, 2^24]");
    const std::shared_ptr<MerkleSnap> s = snap(id);
    out = MerkleProveOut();
    out.first.assign(size_t(q) + 1, 0);
    out.path_first.assign(1, 0);
    if (q == 0) return;
    const uint64_t n = s->count;
    const bool dev = s->d_arena != nullptr;
    // 1. per query: the first leaf whose (txid, index, tag) is not below (txid, index, 0), and how many leaves from
    // there on have the query's outpoint
    std::vector<uint32_t> lb(size_t(q), 0), matches(size_t(q), 0);
    if (dev && n) {
        s->d_search(*s, recs, q, lb.data(), matches.data());
    } else if (n) {
        for (int64_t i = 0; i < q; ++i) {
            uint8_t key[34];
            std::memcpy(key, recs + 40 * i, 33);
            key[33] = 0;
            uint64_t lo = 0, hi = n;
            while (lo < hi) {
                const uint64_t mid = (lo + hi) / 2;
                if (std::memcmp(&s->h_slots[size_t(mid) * kMerkleSlot], key, 34) < 0) lo = mid + 1;
                else hi = mid;
            }
            lb[size_t(i)] = uint32_t(lo);
            while (lo < n && std::memcmp(&s->h_slots[size_t(lo) * kMerkleSlot], key, 33) == 0) ++lo;
            matches[size_t(i)] = uint32_t(lo) - lb[size_t(i)];
        }
    }
    // 2. the leaves to prove: the matches, or the neighbours on either side
    out.present.resize(size_t(q));
    for (int64_t i = 0; i < q; ++i) {
        const uint32_t at = lb[size_t(i)], m = matches[size_t(i)];
        if (at > n || m > n - at) throw std::runtime_error("Merkle search result out of range");
        out.present[size_t(i)] = m ? 1 : 0;
        if (m) {
            for (uint32_t k = 0; k < m; ++k) out.position.push_back(at + k);
        } else {
            if (at > 0) out.position.push_back(at - 1);
            if (at < n) out.position.push_back(at);
        }
        out.first[size_t(i) + 1] = uint32_t(out.position.size());
    }
    // 3. their slots, and their paths as rows of one sibling per level below the root
    const size_t m = out.position.size(), row = s->lv.size.empty() ? 0 : (s->lv.size.size() - 1) * 32;
    out.entry.assign(m * kMerkleSlot, 0);
    std::vector<uint8_t> rows(m * row, 0);
    if (dev && m) {
        s->d_gather(*s, out.position, out.entry.data(), rows.data());
    } else {
        for (size_t j = 0; j < m; ++j) {
            const uint64_t pos = out.position[j];
            std::memcpy(&out.entry[j * kMerkleSlot], &s->h_slots[size_t(pos) * kMerkleSlot], kMerkleSlot);
            for (size_t l = 0; l + 1 < s->lv.size.size(); ++l) {
                const uint64_t sib = (pos >> l) ^ 1;
                if (sib < s->lv.size[l]) std::memcpy(&rows[j * row + 32 * l], &s->h_nodes[size_t(s->lv.off[l] + sib) * 32], 32);
            }
        }
    }
    // 4. the audit paths: the siblings that exist, bottom up (a promoted node has none at its level)
    for (size_t j = 0; j < m; ++j) {
        const uint64_t pos = out.position[j];
        for (size_t l = 0; l + 1 < s->lv.size.size(); ++l)
            if (((pos >> l) ^ 1) < s->lv.size[l]) out.path.insert(out.path.end(), &rows[j * row + 32 * l], &rows[j * row + 32 * l] + 32);
        out.path_first.push_back(uint32_t(out.path.size() / 32));
    }
}

}  // namespace upow
