// What the UTXO translation units share (utxo_table.hip, utxo_scan.hip, utxo_owners.hip, utxo_block.hip,
// utxo_digest.hip, utxo_diff.hip, utxo_merkle.hip): the slot, key-record and payload layouts, the device helpers on
// them, the launch helper, the table handle, and the passes one file queues for another (collect() and lookup() of
// utxo_table.hip, sort_records() of utxo_block.hip). Private to those files, whose common includes are here too; the
// design is described at the top of utxo_table.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "dev_pool.h"
#include "native.h"
#include "streams.h"

namespace upow {

struct alignas(16) UtxoSlot {
    uint32_t k[8];
    uint32_t meta;
    uint32_t pad[3];
};
static_assert(sizeof(UtxoSlot) == 48, "slot size");
static_assert(offsetof(UtxoSlot, meta) == 32 && offsetof(UtxoSlot, pad) == 36, "meta + fingerprint are one aligned 16-byte word");

enum : uint32_t { ST_EMPTY = 0, ST_FULL = 1, ST_TOMB = 2, ST_BUSY = 3 };

// the meta word: state in bits 0-1, output index in bits 8-15, table tag in bits 16-23
__device__ __forceinline__ uint32_t meta_state(uint32_t m) { return m & 3u; }
__device__ __forceinline__ uint32_t meta_index(uint32_t m) { return (m >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t meta_tag(uint32_t m) { return (m >> 16) & 0xffu; }
__device__ __forceinline__ uint32_t meta_full(uint32_t idx, uint32_t tag) { return ST_FULL | (idx << 8) | (tag << 16); }
__device__ __forceinline__ uint32_t meta_tomb(uint32_t m) { return (m & ~3u) | ST_TOMB; }

struct UtxoKeyRec {  // 40 bytes: txid (raw bytes), index, tag
    uint8_t txid[32];
    uint32_t index;
    uint32_t tag;
};
static_assert(sizeof(UtxoKeyRec) == 40, "key record");

struct alignas(16) UtxoPayload {  // 80 bytes
    uint64_t amount;
    uint32_t addr_len;
    uint32_t flags;  // bit 0: is_stake (unspent_outputs.is_stake = 1)
    uint8_t addr[64];
};
constexpr uint32_t PAY_STAKE = 1u;
static_assert(sizeof(UtxoPayload) == 80, "payload");

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p) {
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}
__device__ __forceinline__ uint32_t slot_hash(const uint32_t k[8], uint32_t idx) {
    uint32_t h = k[0] ^ (idx * 0x9E3779B1u);
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    h ^= h >> 12;
    return h;
}
__device__ __forceinline__ void load_key(const UtxoKeyRec& r, uint32_t k[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ld_u32(r.txid + 4 * i);
}
__device__ __forceinline__ bool key_eq(const UtxoSlot& s, const uint32_t k[8]) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= s.k[i] ^ k[i];
    return d == 0;
}
// a live slot back as its key record (the inverse of load_key + meta_full)
__device__ __forceinline__ UtxoKeyRec slot_record(const UtxoSlot& s, uint32_t m) {
    UtxoKeyRec r;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        r.txid[4 * w] = uint8_t(s.k[w]);
        r.txid[4 * w + 1] = uint8_t(s.k[w] >> 8);
        r.txid[4 * w + 2] = uint8_t(s.k[w] >> 16);
        r.txid[4 * w + 3] = uint8_t(s.k[w] >> 24);
    }
    r.index = meta_index(m);
    r.tag = meta_tag(m);
    return r;
}

// Owner fingerprint kept in the key slot (pad[0]): address bytes 1..4 (after the 42/43 parity prefix of
// a compressed key these are x-coordinate bytes, i.e. uniformly random), so the K14 address scan can
// reject a slot from the 48-byte key line alone and touch the 80-byte payload line only on a likely hit.
__device__ __forceinline__ uint32_t addr_fingerprint(const uint8_t* addr) { return ld_u32(addr + 1); }

// The live entry of outpoint (k, idx): walk its probe chain up to the first EMPTY slot. `slot` is NO_SLOT
// when the outpoint is absent. ATOMIC reads the meta words with relaxed agent-scope atomic loads (the erase
// kernel, which goes on to CAS the word it read); the read-only kernels use plain loads.
constexpr uint32_t NO_SLOT = 0xffffffffu;
struct LiveEntry {
    uint32_t slot, meta;
};
template <bool ATOMIC>
__device__ __forceinline__ LiveEntry find_live(const UtxoSlot* tab, uint32_t mask, const uint32_t k[8], uint32_t idx) {
    uint32_t s = slot_hash(k, idx) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const uint32_t m =
            ATOMIC ? __hip_atomic_load(&tab[s].meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : tab[s].meta;
        const uint32_t st = meta_state(m);
        if (st == ST_EMPTY) break;
        if (st == ST_FULL && meta_index(m) == idx && key_eq(tab[s], k)) return {s, m};
        s = (s + 1) & mask;
    }
    return {NO_SLOT, 0u};
}

// K10's 64-bit fingerprint of an outpoint (utxo_block.hip block_dup_kernel; the debug hook of utxo_table.hip
// reports it to the suite)
__device__ __forceinline__ uint64_t outpoint_fp(const uint32_t k[8], uint32_t idx) {
    uint64_t h = (uint64_t(k[0]) << 32 | k[1]) ^ (uint64_t(k[2]) << 17) ^ (uint64_t(k[3]) * 0x9E3779B97F4A7C15ull) ^
                 (uint64_t(k[4]) << 7) ^ (uint64_t(k[5]) << 29) ^ k[6] ^ (uint64_t(k[7]) << 41) ^
                 (uint64_t(idx) * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    return h;
}

// one lane per element in 256-thread blocks on stream `st`; a failed launch throws with the kernel's name
template <typename Kernel, typename... Args>
static void launch(Kernel kernel, int64_t n, hipStream_t st, const char* name, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, args...);
    stream_check(hipGetLastError(), name);
}

static size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

struct UtxoTableDev {
    int device = 0;
    UtxoSlot* tab = nullptr;
    UtxoPayload* pay = nullptr;
    uint32_t cap = 0;
    uint32_t* d_counter = nullptr;
};

// Defined in utxo_table.hip. Every pass holds g_ut_mu from table(h) to its last use of the table; kernels are
// launched only from the file that defines them, so the two table kernels that other passes need are queued
// through collect() and lookup().
constexpr uint32_t ANY_TAG = 0xffffffffu;  // collect(): every live entry; no table tag, those are bytes
extern std::mutex g_ut_mu;
UtxoTableDev& table(int64_t h);  // under g_ut_mu; makes the table's device current
// queue the collection of table t's entries with `tag` into out / pay_out (room for t.cap each) on the node
// stream; `count` receives their number
void collect(const UtxoTableDev& t, uint32_t tag, UtxoKeyRec* out, UtxoPayload* pay_out, uint32_t* count);
// queue utxo_lookup_kernel for the n device-resident records on the node stream: tags_out[i] = tag or 0xff,
// pay_out[i] = the payload or zeros
void lookup(const UtxoTableDev& t, const UtxoKeyRec* recs, int64_t n, uint8_t* tags_out, UtxoPayload* pay_out);

// Defined in utxo_block.hip: K12's stable LSD radix sort of n (> 0) device-resident records by (txid as bytes,
// index), with by_tag by (txid, index, tag), queued on stream `st`. perm[i] is the number of the record that comes
// i-th. The permutation and the sort's scratch go back to the pool with the object, so its owner synchronises `st`
// before letting go of it.
struct SortedPerm {
    PooledBuf<uint32_t> perm_a, perm_b;
    PooledBuf<uint64_t> col_a, col_b;
    PooledBuf<uint8_t> temp;
    const uint32_t* perm = nullptr;
    SortedPerm(uint32_t n, size_t temp_bytes) : perm_a(n), perm_b(n), col_a(n), col_b(n), temp(temp_bytes) {}
};
std::unique_ptr<SortedPerm> sort_records(const UtxoKeyRec* recs, uint32_t n, bool by_tag, hipStream_t st);

}  // namespace upow
