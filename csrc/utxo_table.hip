// K7/K8/K9: HBM-resident UTXO set (outpoint -> output-table tag, amount, owner address) for gfx950.
//
// reference: the seven per-type output tables queried/inserted/deleted with
// `(tx_hash, index) = ANY($1::tx_output[])` (upow/database.py:439-825, used by upow/manager.py:531-543
// and upow/upow_transactions/transaction.py:99-124).
//
// Open addressing with linear probing over 48-byte slots {txid words[8], meta, pad[3]}; meta packs
// state (empty/full/tombstone/busy), the output index and the table tag. A block's inputs/outputs
// are applied as whole batches (one lane per outpoint): probe, insert and erase kernels. Batches of
// different kinds are separate launches, so no op races a different op; inserts claim a slot with a
// CAS on its meta word and publish it with an atomic exchange after the key words.
// The table lives in HBM for the life of the node (288 GB leaves room for ~10^9 outpoints); the
// txid's first word is already uniformly random, so it is the hash.
//
// Each slot has an 80-byte payload in a parallel array {amount u64, address length u32, pad,
// address bytes[64]} — what block validation needs from a spent output (fees, signature key,
// inputs_addresses) without touching the SQL tables. Probing scans only the compact 48-byte key
// slots; the payload line is read once, on a hit.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "dev_pool.h"
#include "native.h"
#include "streams.h"
#include "sha256_common.h"

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

// One entry into the table (the insert kernel's lane body, shared with the rehash); `p` = its payload or
// nullptr, `fp` = its owner fingerprint. The lane walks the probe chain to its first EMPTY slot, remembering
// the first reusable (EMPTY or tombstone) slot; a live entry with the same outpoint is a duplicate and is
// not inserted again (counter[1]). The remembered slot is claimed with a CAS; a lane that loses the race
// walks the chain again, for as long as its walk finds a reusable slot. A launch only ever turns reusable
// slots into claimed ones, so each lost race is a slot gone for good and a lane loses at most capacity
// times: the retries are bounded by progress, not by a constant (lanes of one wave that share a home slot
// race in lockstep, one winner a round, and other waves on the same chain make whole rounds lose, so any
// fixed count is reached by enough chosen same-home keys in one launch, on a table with room to spare).
// counter[0] counts entries whose walk found no reusable slot (table full). Lanes of one launch
// never insert the same outpoint twice (block validation rejects duplicate inputs, hence duplicate txids),
// so the walk only has to see entries published by earlier launches.
__device__ __forceinline__ void insert_one(UtxoSlot* __restrict__ tab, UtxoPayload* __restrict__ pay, uint32_t mask,
                                           const uint32_t k[8], uint32_t idx, uint32_t tag,
                                           const UtxoPayload* __restrict__ p, uint32_t fp,
                                           uint32_t* __restrict__ counter) {
    const uint32_t home = slot_hash(k, idx) & mask;
    for (uint32_t attempt = 0; attempt <= mask; ++attempt) {
        uint32_t s = home, free_slot = NO_SLOT, free_meta = 0;
        for (uint32_t probe = 0; probe <= mask; ++probe) {
            const uint32_t m = __hip_atomic_load(&tab[s].meta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t st = meta_state(m);
            if (st == ST_FULL && meta_index(m) == idx && key_eq(tab[s], k)) {
                atomicAdd(counter + 1, 1u);
                return;
            }
            if ((st == ST_EMPTY || st == ST_TOMB) && free_slot == NO_SLOT) {
                free_slot = s;
                free_meta = m;
            }
            if (st == ST_EMPTY) break;
            s = (s + 1) & mask;
        }
        if (free_slot == NO_SLOT) break;
        uint32_t* mp = &tab[free_slot].meta;
        if (atomicCAS(mp, free_meta, ST_BUSY) != free_meta) continue;  // lost the race: walk again
#pragma unroll
        for (int w = 0; w < 8; ++w) tab[free_slot].k[w] = k[w];
        if (p) {
            pay[free_slot] = *p;
        } else {
            UtxoPayload z{};
            pay[free_slot] = z;
        }
        tab[free_slot].pad[0] = fp;
        __threadfence();
        atomicExch(mp, meta_full(idx, tag));
        return;
    }
    atomicAdd(counter, 1u);
}

__global__ __launch_bounds__(256) void utxo_insert_kernel(UtxoSlot* __restrict__ tab, UtxoPayload* __restrict__ pay,
                                                          uint32_t mask, const UtxoKeyRec* __restrict__ recs,
                                                          const UtxoPayload* __restrict__ in_pay, int64_t n,
                                                          uint32_t* __restrict__ counter) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const uint32_t idx = recs[i].index & 0xffu, tag = recs[i].tag & 0xffu;
    insert_one(tab, pay, mask, k, idx, tag, in_pay ? &in_pay[i] : nullptr, in_pay ? addr_fingerprint(in_pay[i].addr) : 0u,
               counter);
}

// Rehash: one lane per slot of the old table; a live entry goes into the new table with its payload and its
// owner fingerprint as they are (tombstones and empty slots are dropped)
__global__ __launch_bounds__(256) void utxo_migrate_kernel(const UtxoSlot* __restrict__ old_tab,
                                                           const UtxoPayload* __restrict__ old_pay, uint32_t old_cap,
                                                           UtxoSlot* __restrict__ tab, UtxoPayload* __restrict__ pay,
                                                           uint32_t mask, uint32_t* __restrict__ counter) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= old_cap) return;
    const uint32_t m = old_tab[s].meta;
    if (meta_state(m) != ST_FULL) return;
    uint32_t k[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) k[w] = old_tab[s].k[w];
    insert_one(tab, pay, mask, k, meta_index(m), meta_tag(m), &old_pay[s], old_tab[s].pad[0], counter);
    atomicAdd(counter + 2, 1u);
}

// tags_out[i] = tag of the outpoint, 0xff when absent
__global__ __launch_bounds__(256) void utxo_probe_kernel(const UtxoSlot* __restrict__ tab, uint32_t mask,
                                                         const UtxoKeyRec* __restrict__ recs, int64_t n,
                                                         uint8_t* __restrict__ tags_out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const LiveEntry e = find_live<false>(tab, mask, k, recs[i].index & 0xffu);
    tags_out[i] = e.slot != NO_SLOT ? uint8_t(meta_tag(e.meta)) : 0xff;
}

// lookup = probe + payload gather (payload zeroed when absent)
__global__ __launch_bounds__(256) void utxo_lookup_kernel(const UtxoSlot* __restrict__ tab,
                                                          const UtxoPayload* __restrict__ pay, uint32_t mask,
                                                          const UtxoKeyRec* __restrict__ recs, int64_t n,
                                                          uint8_t* __restrict__ tags_out,
                                                          UtxoPayload* __restrict__ pay_out) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const LiveEntry e = find_live<false>(tab, mask, k, recs[i].index & 0xffu);
    if (e.slot != NO_SLOT) {
        tags_out[i] = uint8_t(meta_tag(e.meta));
        pay_out[i] = pay[e.slot];
    } else {
        tags_out[i] = 0xff;
        UtxoPayload z{};
        pay_out[i] = z;
    }
}

// erase: only entries whose tag matches recs[i].tag (0xff = any); erased[i] = 1 when removed
__global__ __launch_bounds__(256) void utxo_erase_kernel(UtxoSlot* __restrict__ tab, uint32_t mask,
                                                         const UtxoKeyRec* __restrict__ recs, int64_t n,
                                                         uint8_t* __restrict__ erased, uint32_t* __restrict__ count) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const uint32_t want = recs[i].tag & 0xffu;
    const LiveEntry e = find_live<true>(tab, mask, k, recs[i].index & 0xffu);
    uint8_t res = 0;
    if (e.slot != NO_SLOT && (want == 0xffu || meta_tag(e.meta) == want) &&
        atomicCAS(&tab[e.slot].meta, e.meta, meta_tomb(e.meta)) == e.meta) {
        res = 1;
        atomicAdd(count, 1u);
    }
    erased[i] = res;
}

// Collect the live entries whose tag is `tag` (ANY_TAG: every live entry) as key records, with their
// payloads when `pay_out` is given; one atomic each, so the order is whatever the atomics give (the dump's
// and K12's callers sort). ANY_TAG is no table tag: those are bytes.
constexpr uint32_t ANY_TAG = 0xffffffffu;
__global__ __launch_bounds__(256) void utxo_collect_kernel(const UtxoSlot* __restrict__ tab,
                                                           const UtxoPayload* __restrict__ pay, uint32_t cap,
                                                           uint32_t tag, UtxoKeyRec* __restrict__ out,
                                                           UtxoPayload* __restrict__ pay_out,
                                                           uint32_t* __restrict__ count) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const uint32_t m = tab[s].meta;
    if (meta_state(m) != ST_FULL || (tag != ANY_TAG && meta_tag(m) != tag)) return;
    const uint32_t o = atomicAdd(count, 1u);
    out[o] = slot_record(tab[s], m);
    if (pay_out) pay_out[o] = pay[s];
}

// K14: outputs owned by one address (reference `database.py:909-937,1138-1205`: balance / spendable
// outputs by address). One lane per slot streams the key metas and, for live slots whose tag is in
// `tag_mask`, the 80-byte payload line; the address is compared as four 16-byte vectors held in SGPRs
// (the query is uniform). The slot's owner fingerprint is checked first, so the payload line is read
// only for likely hits. Matches are rare, so they are compacted with one atomic each; the amount sum
// is a wave reduction + one 64-bit atomic per wave that found anything.
__global__ __launch_bounds__(256) void utxo_address_scan_kernel(const UtxoSlot* __restrict__ tab,
                                                                const UtxoPayload* __restrict__ pay, uint32_t cap,
                                                                uint4 q0, uint4 q1, uint4 q2, uint4 q3, uint32_t qlen,
                                                                uint32_t qfp, uint32_t tag_mask, uint32_t stake_sel,
                                                                uint32_t max_out,
                                                                UtxoKeyRec* __restrict__ out,
                                                                UtxoPayload* __restrict__ pay_out,
                                                                uint32_t* __restrict__ count,
                                                                unsigned long long* __restrict__ total) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t amt = 0;
    if (s < cap) {
        // meta and fingerprint in one 16-byte load (slot bytes 32..47, 16-byte aligned)
        const uint4 mw = *reinterpret_cast<const uint4*>(&tab[s].meta);
        const uint32_t m = mw.x;
        const uint32_t tag = meta_tag(m);
        // stake_sel: 0 any output, 1 only is_stake = 0 (spendable), 2 only is_stake = 1
        const uint32_t stake = tag == 0u ? (pay[s].flags & PAY_STAKE) : 0u;
        if (meta_state(m) == ST_FULL && tag < 32u && ((tag_mask >> tag) & 1u) && mw.y == qfp &&
            pay[s].addr_len == qlen && (stake_sel == 0u || (stake_sel == 1u) == (stake == 0u))) {
            const uint4* a = reinterpret_cast<const uint4*>(pay[s].addr);
            const uint4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
            const uint32_t d = (a0.x ^ q0.x) | (a0.y ^ q0.y) | (a0.z ^ q0.z) | (a0.w ^ q0.w) | (a1.x ^ q1.x) |
                               (a1.y ^ q1.y) | (a1.z ^ q1.z) | (a1.w ^ q1.w) | (a2.x ^ q2.x) | (a2.y ^ q2.y) |
                               (a2.z ^ q2.z) | (a2.w ^ q2.w) | (a3.x ^ q3.x) | (a3.y ^ q3.y) | (a3.z ^ q3.z) |
                               (a3.w ^ q3.w);
            if (d == 0) {
                amt = pay[s].amount;
                const uint32_t o = atomicAdd(count, 1u);
                if (o < max_out) {
                    out[o] = slot_record(tab[s], m);
                    pay_out[o] = pay[s];
                }
            }
        }
    }
    // wave64 sum: amounts are < 2^63 in total (MAX_SUPPLY in smallest units fits in 2^51)
    for (int off = 32; off > 0; off >>= 1) amt += __shfl_down(amt, off, 64);
    if ((threadIdx.x & 63u) == 0 && amt) atomicAdd(total, static_cast<unsigned long long>(amt));
}

// K14, batch form: the same pass over the table for up to SCAN_BATCH_MAX queries at once (the reference's
// `address = ANY($1)` takes an address list natively). The queries are device-resident records sorted by
// owner fingerprint; each block stages the sorted fingerprints into LDS once (the only barrier, before any
// lane returns). A live slot looks its fingerprint up with a lower_bound whose step count is uniform
// (it depends on nq alone); only a slot whose fingerprint is in the table reads its payload line, and then
// every query of the equal-fingerprint run is tested on its own (length, its tag mask, its stake selector,
// the four address words), so colliding fingerprints and one address under several filters each get
// exactly their matches. A match is compacted with one returning atomic and carries the query's position
// in the sorted table (`qbase` + its place in this launch); the amount goes into totals[query] with a
// 64-bit atomic: matches are rare and the lanes of a wave may hit different queries.
constexpr uint32_t SCAN_BATCH_MAX = 1024;  // 4 KB of fingerprints in LDS
struct alignas(16) ScanQuery {  // 80 bytes, built by utxo_address_scan_batch
    uint8_t addr[64];           // zero-padded like the payload's
    uint32_t len;
    uint32_t fp;  // addr_fingerprint() of the padded address
    uint32_t tag_mask;
    uint32_t stake_sel;
};
static_assert(sizeof(ScanQuery) == 80, "scan query");

__global__ __launch_bounds__(256) void utxo_address_scan_batch_kernel(
    const UtxoSlot* __restrict__ tab, const UtxoPayload* __restrict__ pay, uint32_t cap,
    const ScanQuery* __restrict__ qs, uint32_t nq, uint32_t qbase, uint32_t max_out, uint32_t* __restrict__ out_q,
    UtxoKeyRec* __restrict__ out, UtxoPayload* __restrict__ pay_out, uint32_t* __restrict__ count,
    unsigned long long* __restrict__ totals) {
    __shared__ uint32_t fps[SCAN_BATCH_MAX];
    for (uint32_t i = threadIdx.x; i < nq; i += blockDim.x) fps[i] = qs[i].fp;
    __syncthreads();
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap || nq == 0u) return;
    const uint4 mw = *reinterpret_cast<const uint4*>(&tab[s].meta);
    const uint32_t m = mw.x, fp = mw.y;
    const uint32_t tag = meta_tag(m);
    if (meta_state(m) != ST_FULL || tag >= 32u) return;
    // lower_bound(fps, fp): `base` ends at the last entry < fp, or at 0
    uint32_t base = 0;
    for (uint32_t n = nq; n > 1u;) {
        const uint32_t half = n >> 1;
        base = fps[base + half - 1u] < fp ? base + half : base;
        n -= half;
    }
    uint32_t j = base + (fps[base] < fp ? 1u : 0u);
    if (j >= nq || fps[j] != fp) return;
    const UtxoPayload p = pay[s];
    const uint4* a = reinterpret_cast<const uint4*>(p.addr);
    const uint32_t stake = tag == 0u ? (p.flags & PAY_STAKE) : 0u;
    for (; j < nq && fps[j] == fp; ++j) {
        const ScanQuery& q = qs[j];
        const uint32_t sel = q.stake_sel;
        if (q.len != p.addr_len || !((q.tag_mask >> tag) & 1u) || !(sel == 0u || (sel == 1u) == (stake == 0u)))
            continue;
        const uint4* b = reinterpret_cast<const uint4*>(q.addr);
        uint32_t d = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint4 x = a[w], y = b[w];
            d |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
        }
        if (d != 0u) continue;
        const uint32_t o = atomicAdd(count, 1u);
        if (o < max_out) {
            out_q[o] = qbase + j;
            out[o] = slot_record(tab[s], m);
            pay_out[o] = p;
        }
        atomicAdd(&totals[j], static_cast<unsigned long long>(p.amount));
    }
}

// ------------------------------------------------------------------------------------------------
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

static std::mutex g_ut_mu;
static std::unordered_map<int64_t, UtxoTableDev> g_tables;
static int64_t g_next_handle = 1;

static UtxoTableDev& table(int64_t h) {
    auto it = g_tables.find(h);
    if (it == g_tables.end()) throw std::invalid_argument("bad utxo table handle");
    int dev = 0;
    stream_check(hipGetDevice(&dev), "hipGetDevice");
    if (dev != it->second.device) stream_check(hipSetDevice(it->second.device), "hipSetDevice");
    return it->second;
}

// key and payload arrays of 2^log2_cap slots, zeroed on the node stream (not waited for); returns the capacity
static uint32_t table_alloc(uint32_t log2_cap, UtxoSlot*& tab, UtxoPayload*& pay) {
    if (log2_cap < 8 || log2_cap > 31) throw std::invalid_argument("log2 capacity must be in [8, 31]");
    const uint32_t cap = 1u << log2_cap;
    stream_check(hipMalloc(&tab, sizeof(UtxoSlot) * size_t(cap)), "hipMalloc utxo table");
    const hipError_t e = hipMalloc(&pay, sizeof(UtxoPayload) * size_t(cap));
    if (e != hipSuccess) {
        (void)hipFree(tab);
        tab = nullptr;
        stream_check(e, "hipMalloc utxo payload");
    }
    node_memset(tab, 0, sizeof(UtxoSlot) * size_t(cap), "memset utxo table");
    node_memset(pay, 0, sizeof(UtxoPayload) * size_t(cap), "memset utxo payload");
    return cap;
}

int64_t utxo_create(uint32_t log2_cap) {
    UtxoTableDev t;
    stream_check(hipGetDevice(&t.device), "hipGetDevice");
    t.cap = table_alloc(log2_cap, t.tab, t.pay);
    node_sync("utxo_create");
    stream_check(hipMalloc(&t.d_counter, 2 * sizeof(uint32_t)), "hipMalloc counter");
    std::lock_guard<std::mutex> lk(g_ut_mu);
    const int64_t h = g_next_handle++;
    g_tables[h] = t;
    return h;
}

// Asynchronous index update of one committed block (the block path's last GPU step): the inputs are
// packed into pinned memory owned by the table, ONE H2D copy, the insert and the erase launch and a D2H
// of their three counters are queued on the node stream and an event is recorded; the call returns
// without waiting. Every later pass on the table is queued behind it on the same stream, so it reads the
// updated table with no host round trip in between; the counters are collected (event sync) by
// utxo_apply_wait, or by the next utxo_apply_async before it reuses the buffers.
struct AsyncApply {
    hipEvent_t ev = nullptr;
    uint8_t* host = nullptr;
    size_t host_cap = 0;
    uint8_t* dev = nullptr;
    size_t dev_cap = 0;
    const uint32_t* res = nullptr;  // pinned: (entries with no free slot, duplicates skipped, erased)
    bool live = false;
};
static std::unordered_map<int64_t, AsyncApply> g_async;  // by table handle, under g_ut_mu

static bool async_collect(AsyncApply& a, uint32_t out[3]) {
    out[0] = out[1] = out[2] = 0;
    if (!a.live) return false;
    a.live = false;
    stream_check(hipEventSynchronize(a.ev), "utxo async apply");
    out[0] = a.res[0];
    out[1] = a.res[1];
    out[2] = a.res[2];
    return true;
}

static void async_release(int64_t h) {  // under g_ut_mu
    auto it = g_async.find(h);
    if (it == g_async.end()) return;
    uint32_t r[3];
    try {
        async_collect(it->second, r);
    } catch (...) {
    }
    if (it->second.ev) (void)hipEventDestroy(it->second.ev);
    if (it->second.host) (void)hipHostFree(it->second.host);
    if (it->second.dev) (void)hipFree(it->second.dev);
    g_async.erase(it);
}

bool utxo_apply_async(int64_t h, const std::vector<UtxoSeg>& ins, bool with_pay, const uint8_t* del, int64_t n_del,
                      uint32_t prev[3]) {
    int64_t n_ins = 0;
    for (const UtxoSeg& g : ins) n_ins += g.n;
    const bool ins_pay = with_pay && n_ins > 0;
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    AsyncApply& a = g_async[h];
    const bool had = async_collect(a, prev);
    const size_t off_pay = align256(size_t(n_ins) * sizeof(UtxoKeyRec));
    const size_t off_del = off_pay + align256(ins_pay ? size_t(n_ins) * sizeof(UtxoPayload) : 0);
    const size_t off_cnt = off_del + align256(size_t(n_del) * sizeof(UtxoKeyRec));
    const size_t off_st = off_cnt + 256;  // erase status bytes (device only)
    const size_t dev_need = off_st + align256(size_t(n_del));
    if (!a.ev) stream_check(hipEventCreateWithFlags(&a.ev, hipEventDisableTiming), "hipEventCreate");
    if (off_cnt + 256 > a.host_cap) {
        if (a.host) stream_check(hipHostFree(a.host), "hipHostFree");  // the previous apply was collected above
        a.host = nullptr;
        a.host_cap = std::max<size_t>(off_cnt + 256, size_t(4) << 20) * 2;
        stream_check(hipHostMalloc(reinterpret_cast<void**>(&a.host), a.host_cap, hipHostMallocDefault), "hipHostMalloc");
    }
    if (dev_need > a.dev_cap) {
        if (a.dev) {
            node_sync("utxo async regrow");
            stream_check(hipFree(a.dev), "hipFree");
        }
        a.dev = nullptr;
        a.dev_cap = std::max<size_t>(dev_need, size_t(4) << 20) * 2;
        stream_check(hipMalloc(reinterpret_cast<void**>(&a.dev), a.dev_cap), "hipMalloc");
    }
    size_t at = 0;  // the groups land back to back: no concatenation on the caller's side
    for (const UtxoSeg& g : ins) {
        if (!g.n) continue;
        std::memcpy(a.host + at * sizeof(UtxoKeyRec), g.recs, size_t(g.n) * sizeof(UtxoKeyRec));
        if (ins_pay) std::memcpy(a.host + off_pay + at * sizeof(UtxoPayload), g.pay, size_t(g.n) * sizeof(UtxoPayload));
        at += size_t(g.n);
    }
    if (n_del) std::memcpy(a.host + off_del, del, size_t(n_del) * sizeof(UtxoKeyRec));
    hipStream_t st = node_stream();
    stream_check(hipMemcpyAsync(a.dev, a.host, off_cnt, hipMemcpyHostToDevice, st), "async apply h2d");
    uint32_t* cnt = reinterpret_cast<uint32_t*>(a.dev + off_cnt);
    stream_check(hipMemsetAsync(cnt, 0, 16, st), "async apply memset");
    if (n_ins)
        launch(utxo_insert_kernel, n_ins, st, "utxo_insert_kernel (async)", t.tab, t.pay, t.cap - 1,
               reinterpret_cast<const UtxoKeyRec*>(a.dev),
               ins_pay ? reinterpret_cast<const UtxoPayload*>(a.dev + off_pay) : nullptr, n_ins, cnt);
    if (n_del)
        launch(utxo_erase_kernel, n_del, st, "utxo_erase_kernel (async)", t.tab, t.cap - 1,
               reinterpret_cast<const UtxoKeyRec*>(a.dev + off_del), n_del, a.dev + off_st, cnt + 2);
    uint32_t* res = reinterpret_cast<uint32_t*>(a.host + off_cnt);
    stream_check(hipMemcpyAsync(res, cnt, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "async apply d2h");
    stream_check(hipEventRecord(a.ev, st), "hipEventRecord");
    a.res = res;
    a.live = true;
    return had;
}

bool utxo_apply_wait(int64_t h, uint32_t out[3]) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    (void)table(h);
    auto it = g_async.find(h);
    if (it == g_async.end()) {
        out[0] = out[1] = out[2] = 0;
        return false;
    }
    return async_collect(it->second, out);
}

void utxo_destroy(int64_t h) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    async_release(h);
    auto it = g_tables.find(h);
    if (it == g_tables.end()) return;
    (void)hipFree(it->second.tab);
    (void)hipFree(it->second.pay);
    (void)hipFree(it->second.d_counter);
    g_tables.erase(it);
}

// Rebuild the table at capacity 2^log2_cap on the device (growth, or the same size to drop tombstones): the
// live entries move from the old arrays into fresh ones in one launch, no host round trip (the dump + host
// re-insert it replaced moved the whole set over PCIe twice: ~0.5 GB at 5 M outpoints). Queued on the node
// stream behind any pending async apply, so the handle stays valid throughout. Returns (live entries moved) |
// (entries that found no slot << 32); when any found no slot the new arrays are dropped and the table stays
// as it was.
uint64_t utxo_rehash(int64_t h, uint32_t log2_cap) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    UtxoSlot* tab = nullptr;
    UtxoPayload* pay = nullptr;
    const uint32_t cap = table_alloc(log2_cap, tab, pay);
    PooledBuf<uint32_t> cnt(4);
    node_memset(cnt.p, 0, 4 * sizeof(uint32_t), "memset");
    launch(utxo_migrate_kernel, t.cap, node_stream(), "utxo_migrate_kernel", t.tab, t.pay, t.cap, tab, pay, cap - 1,
           cnt.p);
    uint32_t c[4] = {0, 0, 0, 0};
    node_d2h(c, cnt.p, sizeof c, "d2h rehash counters");  // synchronises the node stream: both tables are idle
    if (c[0] == 0) {
        std::swap(t.tab, tab);
        std::swap(t.pay, pay);
        t.cap = cap;
    }
    (void)hipFree(tab);  // the old arrays, or the new ones when the rehash failed
    (void)hipFree(pay);
    return uint64_t(c[2] - c[0]) | (uint64_t(c[0]) << 32);
}

uint32_t utxo_capacity(int64_t h) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    return table(h).cap;
}

// per-call scratch (PooledBuf) comes from the caching pool (csrc/dev_pool.h): no hipMalloc/hipFree per block

uint64_t utxo_insert(int64_t h, const uint8_t* recs, int64_t n, const uint8_t* payload) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    if (n == 0) return 0;
    PooledBuf<UtxoKeyRec> d(n);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * n, "h2d recs");
    PooledBuf<UtxoPayload> dp(payload ? n : 0);
    if (payload) node_h2d(dp.p, payload, sizeof(UtxoPayload) * n, "h2d payload");
    node_memset(t.d_counter, 0, 2 * sizeof(uint32_t), "memset");
    launch(utxo_insert_kernel, n, node_stream(), "utxo_insert_kernel", t.tab, t.pay, t.cap - 1, d.p,
           payload ? dp.p : nullptr, n, t.d_counter);
    uint32_t c[2] = {0, 0};
    node_d2h(c, t.d_counter, sizeof c, "d2h failed");
    return uint64_t(c[0]) | (uint64_t(c[1]) << 32);  // (table full) | (duplicates << 32)
}

std::vector<uint8_t> utxo_lookup(int64_t h, const uint8_t* recs, int64_t n, std::vector<uint8_t>& payload_out) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    std::vector<uint8_t> out(static_cast<size_t>(n));
    payload_out.assign(static_cast<size_t>(n) * sizeof(UtxoPayload), 0);
    if (n == 0) return out;
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<uint8_t> o(n);
    PooledBuf<UtxoPayload> po(n);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * n, "h2d recs");
    launch(utxo_lookup_kernel, n, node_stream(), "utxo_lookup_kernel", t.tab, t.pay, t.cap - 1, d.p, n, o.p, po.p);
    node_d2h(out.data(), o.p, size_t(n), "d2h tags");
    node_d2h(payload_out.data(), po.p, payload_out.size(), "d2h payload");
    return out;
}

std::vector<uint8_t> utxo_probe(int64_t h, const uint8_t* recs, int64_t n) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    std::vector<uint8_t> out(static_cast<size_t>(n));
    if (n == 0) return out;
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<uint8_t> o(n);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * n, "h2d recs");
    launch(utxo_probe_kernel, n, node_stream(), "utxo_probe_kernel", t.tab, t.cap - 1, d.p, n, o.p);
    node_d2h(out.data(), o.p, size_t(n), "d2h tags");
    return out;
}

std::vector<uint8_t> utxo_erase(int64_t h, const uint8_t* recs, int64_t n) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    std::vector<uint8_t> out(static_cast<size_t>(n));
    if (n == 0) return out;
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<uint8_t> o(n);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * n, "h2d recs");
    node_memset(t.d_counter, 0, sizeof(uint32_t), "memset");
    launch(utxo_erase_kernel, n, node_stream(), "utxo_erase_kernel", t.tab, t.cap - 1, d.p, n, o.p, t.d_counter);
    node_d2h(out.data(), o.p, size_t(n), "d2h erased");
    return out;
}

std::vector<uint8_t> utxo_address_scan(int64_t h, const uint8_t* addr, uint32_t len, uint32_t tag_mask,
                                       uint32_t stake_sel, std::vector<uint8_t>& payload_out, uint64_t* total_out) {
    if (len > 64) throw std::invalid_argument("address is at most 64 bytes");
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    uint4 q[4];
    std::memset(q, 0, sizeof(q));
    std::memcpy(q, addr, len);  // payload addresses are zero-padded to 64 bytes
    uint32_t qfp = 0;           // same bytes as addr_fingerprint() on the zero-padded query
    std::memcpy(&qfp, reinterpret_cast<const uint8_t*>(q) + 1, 4);
    // first pass sizes the output; a second pass runs only if more matches than the guess came back
    uint32_t cap_out = 4096, n = 0;
    PooledBuf<unsigned long long> dt(1);
    for (int pass = 0; pass < 2; ++pass) {
        PooledBuf<UtxoKeyRec> d(cap_out);
        PooledBuf<UtxoPayload> dp(cap_out);
        node_memset(t.d_counter, 0, sizeof(uint32_t), "memset");
        node_memset(dt.p, 0, sizeof(unsigned long long), "memset");
        launch(utxo_address_scan_kernel, t.cap, node_stream(), "utxo_address_scan_kernel", t.tab, t.pay, t.cap, q[0],
               q[1], q[2], q[3], len, qfp, tag_mask, stake_sel, cap_out, d.p, dp.p, t.d_counter, dt.p);
        node_d2h(&n, t.d_counter, sizeof(uint32_t), "d2h n");
        if (n <= cap_out) {
            unsigned long long tot = 0;
            node_d2h(&tot, dt.p, sizeof(tot), "d2h total");
            *total_out = tot;
            std::vector<uint8_t> out(size_t(n) * sizeof(UtxoKeyRec));
            payload_out.assign(size_t(n) * sizeof(UtxoPayload), 0);
            if (n) {
                node_d2h(out.data(), d.p, out.size(), "d2h recs");
                node_d2h(payload_out.data(), dp.p, payload_out.size(), "d2h payload");
            }
            return out;
        }
        cap_out = n;
    }
    throw std::runtime_error("utxo_address_scan: table changed between passes");
}

void utxo_address_scan_batch(int64_t h, const uint8_t* addrs, const uint32_t* lens, const uint32_t* tag_masks,
                             const uint32_t* stake_sels, int64_t n, AddressBatchOut& r) {
    r.qidx.clear();
    r.recs.clear();
    r.payload.clear();
    r.totals.assign(size_t(std::max<int64_t>(n, 0)), 0);
    for (int64_t i = 0; i < n; ++i)
        if (lens[i] > 64) throw std::invalid_argument("address is at most 64 bytes");
    if (n <= 0) return;
    // the query records, sorted by fingerprint (then by all their bytes, so exact duplicates are neighbours)
    std::vector<ScanQuery> all(static_cast<size_t>(n));
    std::memset(all.data(), 0, sizeof(ScanQuery) * all.size());
    for (int64_t i = 0; i < n; ++i) {
        ScanQuery& q = all[i];
        std::memcpy(q.addr, addrs + 64 * i, lens[i]);  // payload addresses are zero-padded to 64 bytes
        q.len = lens[i];
        std::memcpy(&q.fp, q.addr + 1, 4);  // same bytes as addr_fingerprint() on the zero-padded query
        q.tag_mask = tag_masks[i];
        q.stake_sel = stake_sels[i];
    }
    std::vector<uint32_t> order(static_cast<size_t>(n));
    for (int64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (all[x].fp != all[y].fp) return all[x].fp < all[y].fp;
        const int c = std::memcmp(&all[x], &all[y], sizeof(ScanQuery));
        return c != 0 ? c < 0 : x < y;
    });
    // unique queries in sorted order; askers[ask_start[u] .. ask_start[u + 1]) = the caller's queries that are u
    std::vector<ScanQuery> uniq;
    std::vector<uint32_t> ask_start;
    for (int64_t i = 0; i < n; ++i) {
        if (i == 0 || std::memcmp(&all[order[i]], &all[order[i - 1]], sizeof(ScanQuery)) != 0) {
            uniq.push_back(all[order[i]]);
            ask_start.push_back(uint32_t(i));
        }
    }
    const uint32_t nu = uint32_t(uniq.size());
    ask_start.push_back(uint32_t(n));

    std::lock_guard<std::mutex> lk(g_ut_mu);  // one hold for every launch: the whole batch sees one table state
    UtxoTableDev& t = table(h);
    PooledBuf<ScanQuery> dq(nu);
    PooledBuf<unsigned long long> dt(nu);
    node_h2d(dq.p, uniq.data(), sizeof(ScanQuery) * nu, "h2d queries");
    // first pass sizes the output; a second pass runs only if more matches than the guess came back
    uint32_t cap_out = 4096, m = 0;
    for (int pass = 0; pass < 2; ++pass) {
        PooledBuf<uint32_t> di(cap_out);
        PooledBuf<UtxoKeyRec> d(cap_out);
        PooledBuf<UtxoPayload> dp(cap_out);
        node_memset(t.d_counter, 0, sizeof(uint32_t), "memset");
        node_memset(dt.p, 0, sizeof(unsigned long long) * nu, "memset");
        for (uint32_t base = 0; base < nu; base += SCAN_BATCH_MAX)
            launch(utxo_address_scan_batch_kernel, t.cap, node_stream(), "utxo_address_scan_batch_kernel", t.tab,
                   t.pay, t.cap, dq.p + base, std::min(SCAN_BATCH_MAX, nu - base), base, cap_out, di.p, d.p, dp.p,
                   t.d_counter, dt.p + base);
        node_d2h(&m, t.d_counter, sizeof(uint32_t), "d2h n");
        if (m > cap_out) {
            cap_out = m;
            continue;
        }
        std::vector<uint32_t> ids(m);
        std::vector<UtxoKeyRec> recs(m);
        std::vector<UtxoPayload> pays(m);
        std::vector<unsigned long long> tot(nu);
        if (m) {
            node_d2h(ids.data(), di.p, sizeof(uint32_t) * m, "d2h ids");
            node_d2h(recs.data(), d.p, sizeof(UtxoKeyRec) * m, "d2h recs");
            node_d2h(pays.data(), dp.p, sizeof(UtxoPayload) * m, "d2h payload");
        }
        node_d2h(tot.data(), dt.p, sizeof(unsigned long long) * nu, "d2h totals");
        // back to the caller's numbering, duplicates fanned out
        for (uint32_t u = 0; u < nu; ++u)
            for (uint32_t k = ask_start[u]; k < ask_start[u + 1]; ++k) r.totals[order[k]] = tot[u];
        size_t m_out = 0;
        for (uint32_t k = 0; k < m; ++k) {
            if (ids[k] >= nu) throw std::runtime_error("utxo_address_scan_batch: query id out of range");
            m_out += ask_start[ids[k] + 1] - ask_start[ids[k]];
        }
        r.qidx.reserve(m_out);
        r.recs.resize(m_out * sizeof(UtxoKeyRec));
        r.payload.resize(m_out * sizeof(UtxoPayload));
        size_t at = 0;
        for (uint32_t k = 0; k < m; ++k)
            for (uint32_t a = ask_start[ids[k]]; a < ask_start[ids[k] + 1]; ++a, ++at) {
                r.qidx.push_back(order[a]);
                std::memcpy(r.recs.data() + at * sizeof(UtxoKeyRec), &recs[k], sizeof(UtxoKeyRec));
                std::memcpy(r.payload.data() + at * sizeof(UtxoPayload), &pays[k], sizeof(UtxoPayload));
            }
        return;
    }
    throw std::runtime_error("utxo_address_scan_batch: table changed between passes");
}

// queue the collection of table t's entries with `tag` into out / pay_out (room for t.cap each) on the node
// stream; `count` receives their number
static void collect(const UtxoTableDev& t, uint32_t tag, UtxoKeyRec* out, UtxoPayload* pay_out, uint32_t* count) {
    node_memset(count, 0, sizeof(uint32_t), "memset");
    launch(utxo_collect_kernel, t.cap, node_stream(), "utxo_collect_kernel", t.tab, t.pay, t.cap, tag, out, pay_out,
           count);
}

std::vector<uint8_t> utxo_dump(int64_t h, std::vector<uint8_t>* payload_out) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    PooledBuf<UtxoKeyRec> d(t.cap);
    PooledBuf<UtxoPayload> dp(payload_out ? t.cap : 0);
    collect(t, ANY_TAG, d.p, payload_out ? dp.p : nullptr, t.d_counter);
    uint32_t n = 0;
    node_d2h(&n, t.d_counter, sizeof(uint32_t), "d2h n");
    std::vector<uint8_t> out(size_t(n) * sizeof(UtxoKeyRec));
    if (n) node_d2h(out.data(), d.p, out.size(), "d2h dump");
    if (payload_out) {
        payload_out->assign(size_t(n) * sizeof(UtxoPayload), 0);
        if (n) node_d2h(payload_out->data(), dp.p, payload_out->size(), "d2h payload");
    }
    return out;
}

// ================================================================================================
// Holders report: per-owner totals of the whole set in one table pass (a hash aggregation by owner key).
// ================================================================================================

// An owner is a public key: the canonical 33-byte key of a payload is the rule of csrc/txcodec.cpp
// input_address_strings ((addr[0] == 43 ? 43 : 42) | addr[1..32] for the 33-byte form, ((addr[32] & 1) ? 43 : 42)
// | addr[0..31] for the 64-byte form), held as the eight little-endian words of x and the prefix byte.
struct OwnerKey {
    uint32_t x[8];
    uint32_t p;
};
struct PayHead {  // the payload's first 16 bytes
    uint64_t amount;
    uint32_t len, flags;
};
__device__ __forceinline__ PayHead pay_head(const UtxoPayload* __restrict__ pp) {
    const uint4 h = *reinterpret_cast<const uint4*>(pp);
    return {uint64_t(h.x) | (uint64_t(h.y) << 32), h.z, h.w};
}
// the key of a payload whose length is 33 or 64: three 16-byte loads; the x of the 33-byte form starts at
// byte 1 and is realigned in registers
__device__ __forceinline__ OwnerKey owner_key(const UtxoPayload* __restrict__ pp, uint32_t len) {
    const uint4* a = reinterpret_cast<const uint4*>(pp->addr);
    const uint4 a0 = a[0], a1 = a[1], a2 = a[2];
    const uint32_t w[9] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x};
    OwnerKey k;
    if (len == 64u) {
#pragma unroll
        for (int i = 0; i < 8; ++i) k.x[i] = w[i];
        k.p = 42u + (w[8] & 1u);  // y is little-endian: its parity is bit 0 of byte 32
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) k.x[i] = (w[i] >> 8) | (w[i + 1] << 24);
        k.p = (w[0] & 0xffu) == 43u ? 43u : 42u;
    }
    return k;
}
__device__ __forceinline__ bool owner_eq(const OwnerKey& a, const OwnerKey& b) {
    uint32_t d = a.p ^ b.p;
#pragma unroll
    for (int i = 0; i < 8; ++i) d |= a.x[i] ^ b.x[i];
    return d == 0;
}
__device__ __forceinline__ uint64_t owner_hash(const OwnerKey& k) {
    uint64_t h = 0x9E3779B97F4A7C15ull * (k.p + 1u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h = (h ^ ((uint64_t(k.x[2 * i]) << 32) | k.x[2 * i + 1])) * 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    }
    h *= 0x94D049BB133111EBull;
    return h ^ (h >> 32);
}

struct alignas(16) OwnerRec {  // 112 bytes: OWNER_DTYPE of upow_amd/ledger/utxo.py
    uint32_t key[10];          // 33 key bytes, 7 zero bytes
    uint32_t outputs, outputs_full;
    uint64_t sums[8];
};
static_assert(sizeof(OwnerRec) == 112 && offsetof(OwnerRec, outputs) == 40 && offsetof(OwnerRec, sums) == 48,
              "owner record");
constexpr int OWNER_COLS = 8;
// counters of one pass (64-bit words): the eight grand totals, then these. A wave adds into the stripe its
// block number names (one 128-byte line each) and the host sums the stripes: with one line for all, the
// ~10^6 wave atomics of a 2^24-slot pass queue up behind each other and take longer than the pass itself.
enum : int { OC_OUTPUTS = 8, OC_SKIPPED = 9, OC_FAILED = 10, OC_OWNERS = 11, OC_WORDS = 16, OC_STRIPES = 128 };

// One lane per table slot. A live entry with tag <= 6 and a 33/64-byte payload finds its owner's group in the
// scratch table `words` (zeroed, gmask + 1 slots): a word packs a fingerprint tag of the owner key (high 32
// bits, masked by tag_mask) with 1 + the table slot of the entry that claimed the group, so a claimed word is
// never 0. The lane probes linearly from its hash, with a 64-bit CAS on a word it reads as empty, as K10's
// block_dup_kernel does: an empty word is claimed; a word with the lane's tag has its claimer's payload compared in full
// (pay[] is not written during the pass, so there is nothing to publish and no lane waits for another); any
// other word sends the lane on. The walk is bounded by the group-table size; a lane that finds no slot counts
// in cnt[OC_FAILED] and adds nothing. Column = tag, except tag 0 with the stake flag, which is column 7.
// The grand totals and the counts are wave64 reductions with one atomic per wave and non-zero value, into
// the block's stripe of `cnt`.
__global__ __launch_bounds__(256) void utxo_owner_group_kernel(
    const UtxoSlot* __restrict__ tab, const UtxoPayload* __restrict__ pay, uint32_t cap,
    unsigned long long* __restrict__ words, uint32_t gmask, uint32_t tag_mask, unsigned long long* __restrict__ sums,
    uint32_t* __restrict__ outputs, unsigned long long* __restrict__ cnt_stripes) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long* cnt = cnt_stripes + size_t(blockIdx.x & (OC_STRIPES - 1)) * OC_WORDS;
    uint64_t amt = 0;
    uint32_t col = OWNER_COLS;  // none
    uint64_t counts = 0;        // grouped | skipped << 16 | groups claimed << 32 (a wave sums at most 64 of each)
    if (s < cap) {
        const uint32_t m = tab[s].meta;
        if (meta_state(m) == ST_FULL) {
            const uint32_t tag = meta_tag(m);
            const PayHead hd = tag <= 6u ? pay_head(pay + s) : PayHead{0, 0, 0};
            if (tag > 6u || (hd.len != 33u && hd.len != 64u)) {
                counts = 1ull << 16;
            } else {
                const OwnerKey k = owner_key(pay + s, hd.len);
                const uint64_t h = owner_hash(k);
                const unsigned long long want = uint64_t(uint32_t(h >> 32) & tag_mask) << 32;
                const unsigned long long mine = want | (s + 1u);
                uint32_t g = uint32_t(h) & gmask;
                bool found = false;
                for (uint32_t probe = 0; probe <= gmask; ++probe) {
                    // a word, once claimed, never changes: only a word read as empty needs the CAS (the lanes
                    // of a hot owner then read its word instead of queueing a CAS each on it)
                    unsigned long long prev = __hip_atomic_load(&words[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (prev == 0ull) prev = atomicCAS(&words[g], 0ull, mine);
                    if (prev == 0ull) {  // claimed: this entry represents its owner
                        counts = 1ull << 32;
                        found = true;
                        break;
                    }
                    if ((prev & 0xFFFFFFFF00000000ull) == want) {
                        const uint32_t rep = uint32_t(prev) - 1u;  // the claiming entry's slot
                        if (rep < cap && owner_eq(owner_key(pay + rep, pay_head(pay + rep).len), k)) {
                            found = true;
                            break;
                        }
                    }
                    g = (g + 1u) & gmask;
                }
                if (found) {
                    col = tag == 0u && (hd.flags & PAY_STAKE) ? 7u : tag;
                    amt = hd.amount;
                    counts |= 1ull;
                    atomicAdd(&sums[size_t(g) * OWNER_COLS + col], static_cast<unsigned long long>(amt));
                    atomicAdd(&outputs[2 * size_t(g)], 1u);
                    if (hd.len == 64u) atomicAdd(&outputs[2 * size_t(g) + 1], 1u);
                } else {
                    atomicAdd(&cnt[OC_FAILED], 1ull);
                }
            }
        }
    }
    const bool lead = (threadIdx.x & 63u) == 0;
#pragma unroll
    for (int c = 0; c < OWNER_COLS; ++c) {
        uint64_t v = col == uint32_t(c) ? amt : 0;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lead && v) atomicAdd(&cnt[c], static_cast<unsigned long long>(v));
    }
    for (int off = 32; off > 0; off >>= 1) counts += __shfl_down(counts, off, 64);
    if (lead) {
        if (counts & 0xffffu) atomicAdd(&cnt[OC_OUTPUTS], static_cast<unsigned long long>(counts & 0xffffu));
        if ((counts >> 16) & 0xffffu) atomicAdd(&cnt[OC_SKIPPED], static_cast<unsigned long long>((counts >> 16) & 0xffffu));
        if (counts >> 32) atomicAdd(&cnt[OC_OWNERS], static_cast<unsigned long long>(counts >> 32));
    }
}

// A block turns OWNER_TILE consecutive group slots, OWNER_ITEMS per lane, into owner records: a claimed slot
// becomes one record (the key re-derived from its representative's payload), metric[] = the sum of its
// `by_mask` columns. The block takes its records' positions with ONE returning atomic (ballot counts per
// wave, summed through LDS): a returning atomic on one address costs ~11 ns whoever issues it, so one per
// wave (2.6 x 10^5 of them over a 2^24-slot group table) took 3 ms where the records themselves take a
// fraction of that. Every lane reaches both barriers; nothing is waited for but the block's own lanes.
constexpr uint32_t OWNER_ITEMS = 4, OWNER_TILE = 256 * OWNER_ITEMS;
__global__ __launch_bounds__(256) void utxo_owner_compact_kernel(
    const UtxoPayload* __restrict__ pay, uint32_t cap, const unsigned long long* __restrict__ words, uint32_t groups,
    const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ outputs, uint32_t by_mask,
    uint32_t max_out, OwnerRec* __restrict__ out, uint64_t* __restrict__ metric, uint32_t* __restrict__ count) {
    __shared__ uint32_t wave_n[4], block_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t rep[OWNER_ITEMS], before[OWNER_ITEMS];  // the slot's representative (NO_SLOT: none), records ahead of it in the wave
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < OWNER_ITEMS; ++i) {
        const uint32_t g = blockIdx.x * OWNER_TILE + i * 256u + threadIdx.x;
        const unsigned long long w = g < groups ? words[g] : 0ull;
        const bool have = w != 0ull && uint32_t(w) - 1u < cap;
        rep[i] = have ? uint32_t(w) - 1u : NO_SLOT;
        const unsigned long long peers = __ballot(have);
        before[i] = mine + uint32_t(__popcll(peers & ((1ull << lane) - 1ull)));
        mine += uint32_t(__popcll(peers));  // wave-uniform: the wave's records so far
    }
    if (lane == 0) wave_n[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        block_base = n ? atomicAdd(count, n) : 0u;
    }
    __syncthreads();
    uint32_t base = block_base;
    for (uint32_t v = 0; v < wave; ++v) base += wave_n[v];
#pragma unroll
    for (uint32_t i = 0; i < OWNER_ITEMS; ++i) {
        const uint32_t o = base + before[i];
        if (rep[i] == NO_SLOT || o >= max_out) continue;
        const uint32_t g = blockIdx.x * OWNER_TILE + i * 256u + threadIdx.x;
        const OwnerKey k = owner_key(pay + rep[i], pay_head(pay + rep[i]).len);
        OwnerRec r;
        r.key[0] = k.p | (k.x[0] << 8);
#pragma unroll
        for (int j = 1; j < 8; ++j) r.key[j] = (k.x[j - 1] >> 24) | (k.x[j] << 8);
        r.key[8] = k.x[7] >> 24;
        r.key[9] = 0;
        r.outputs = outputs[2 * size_t(g)];
        r.outputs_full = outputs[2 * size_t(g) + 1];
        uint64_t mt = 0;
#pragma unroll
        for (int c = 0; c < OWNER_COLS; ++c) {
            r.sums[c] = sums[size_t(g) * OWNER_COLS + c];
            if ((by_mask >> c) & 1u) mt += r.sums[c];
        }
        out[o] = r;
        metric[o] = mt;
    }
}

// top mode: every record whose metric is at least *threshold (the N-th greatest), boundary ties included
__global__ __launch_bounds__(256) void utxo_owner_threshold_kernel(const OwnerRec* __restrict__ recs,
                                                                   const uint64_t* __restrict__ metric, uint32_t n,
                                                                   const uint64_t* __restrict__ threshold,
                                                                   OwnerRec* __restrict__ out,
                                                                   uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || metric[i] < *threshold) return;
    out[atomicAdd(count, 1u)] = recs[i];  // at most n records: `out` has room for n
}

void utxo_owner_totals(int64_t h, int64_t top, uint32_t by_mask, uint32_t log2_groups, uint32_t tag_bits,
                       OwnerTotalsOut& r) {
    r = OwnerTotalsOut{};
    if (top < -1) throw std::invalid_argument("top must be -1 (every owner) or >= 0");
    if (by_mask == 0 || by_mask > 0xffu) throw std::invalid_argument("by_mask names columns 0..7, at least one");
    if (log2_groups != 0 && (log2_groups < 4 || log2_groups > 31))
        throw std::invalid_argument("log2 group-table size must be in [4, 31] (0: the table's capacity)");
    if (tag_bits > 32) throw std::invalid_argument("tag bits must be in [0, 32]");
    std::lock_guard<std::mutex> lk(g_ut_mu);  // one hold for every launch: the whole report sees one table state
    UtxoTableDev& t = table(h);
    uint32_t lg = log2_groups;
    if (lg == 0)  // as many group slots as table slots: distinct owners cannot exceed the entries
        while ((1u << lg) < t.cap) ++lg;
    const uint32_t groups = 1u << lg;
    const uint32_t tag_mask = tag_bits == 32 ? 0xffffffffu : (1u << tag_bits) - 1u;
    hipStream_t st = node_stream();
    PooledBuf<unsigned long long> words(groups), sums(size_t(groups) * OWNER_COLS), cnt(OC_STRIPES * OC_WORDS);
    PooledBuf<uint32_t> outputs(size_t(groups) * 2), counts(2);
    node_memset(words.p, 0, sizeof(unsigned long long) * groups, "memset groups");
    node_memset(sums.p, 0, sizeof(unsigned long long) * groups * OWNER_COLS, "memset sums");
    node_memset(outputs.p, 0, sizeof(uint32_t) * groups * 2, "memset outputs");
    node_memset(cnt.p, 0, sizeof(unsigned long long) * OC_STRIPES * OC_WORDS, "memset counters");
    node_memset(counts.p, 0, 2 * sizeof(uint32_t), "memset counts");
    launch(utxo_owner_group_kernel, t.cap, st, "utxo_owner_group_kernel", t.tab, t.pay, t.cap, words.p, groups - 1,
           tag_mask, sums.p, outputs.p, cnt.p);
    std::vector<unsigned long long> stripes(OC_STRIPES * OC_WORDS);
    node_d2h(stripes.data(), cnt.p, sizeof(unsigned long long) * stripes.size(),
             "d2h owner counters");  // synchronises: the scratch may go back to the pool
    unsigned long long c[OC_WORDS] = {0};
    for (int i = 0; i < OC_STRIPES; ++i)
        for (int k = 0; k < OC_WORDS; ++k) c[k] += stripes[size_t(i) * OC_WORDS + k];  // modulo 2^64
    if (c[OC_FAILED])
        throw std::runtime_error("utxo_owner_totals: " + std::to_string(c[OC_FAILED]) +
                                 " entries found no slot in the group table of " + std::to_string(groups) + " slots");
    for (int k = 0; k < OWNER_COLS; ++k) r.totals[k] = c[k];
    r.outputs = c[OC_OUTPUTS];
    r.skipped = c[OC_SKIPPED];
    r.owners = c[OC_OWNERS];
    if (r.owners == 0 || top == 0) return;
    const uint32_t n = uint32_t(r.owners);
    PooledBuf<OwnerRec> recs(n);
    PooledBuf<uint64_t> metric(n);
    uint32_t* d_count = counts.p;  // records compacted, records picked
    launch(utxo_owner_compact_kernel, (groups + OWNER_ITEMS - 1) / OWNER_ITEMS, st, "utxo_owner_compact_kernel",
           t.pay, t.cap, words.p, groups, sums.p, outputs.p, by_mask, n, recs.p, metric.p, d_count);
    if (top < 0 || int64_t(n) <= top) {
        uint32_t got = 0;
        node_d2h(&got, d_count, sizeof got, "d2h owner count");
        if (got != n) throw std::runtime_error("utxo_owner_totals: group table and owner count disagree");
        r.recs.resize(size_t(n) * sizeof(OwnerRec));
        node_d2h(r.recs.data(), recs.p, r.recs.size(), "d2h owners");
        return;
    }
    // more owners than asked for: the N-th greatest metric from a descending radix sort, then every record at
    // or above it
    PooledBuf<uint64_t> sorted(n);
    PooledBuf<OwnerRec> picked(n);
    size_t temp_bytes = 0;
    stream_check(hipcub::DeviceRadixSort::SortKeysDescending(nullptr, temp_bytes, metric.p, sorted.p, n, 0, 64, st),
                 "radix sort sizing");
    PooledBuf<uint8_t> temp(temp_bytes);
    stream_check(hipcub::DeviceRadixSort::SortKeysDescending(temp.p, temp_bytes, metric.p, sorted.p, n, 0, 64, st),
                 "radix sort");
    launch(utxo_owner_threshold_kernel, n, st, "utxo_owner_threshold_kernel", recs.p, metric.p, n, sorted.p + (top - 1),
           picked.p, d_count + 1);
    uint32_t got[2] = {0, 0};
    node_d2h(got, d_count, sizeof got, "d2h owner counts");
    if (got[0] != n || got[1] < uint64_t(top) || got[1] > n)
        throw std::runtime_error("utxo_owner_totals: group table and owner count disagree");
    r.recs.resize(size_t(got[1]) * sizeof(OwnerRec));
    node_d2h(r.recs.data(), picked.p, r.recs.size(), "d2h owners");
}

// ================================================================================================
// Whole-block input pass (K7 + K10 + K11 in one round trip) and the sorted UTXO-set hash (K12).
// ================================================================================================

// K10: duplicate outpoints within a block. Each lane walks a scratch table (at most half full) from the slot
// its 64-bit fingerprint of (txid, index byte) names, with one 64-bit CAS per slot; a word packs the
// fingerprint's top 40 bits with 1 + the lane id of the lane that claimed it (so no claimed word is 0, the
// empty slot, whatever the fingerprint). A lane that meets its own 40 bits compares its 32 txid bytes and
// index byte with that lane's record: equal, it reports the lane (dup_of = winner + 1) and stops; different
// (a fingerprint collision: txids are the spender's choice, and a colliding pair costs ~2^24 hashes), it
// goes on to the next slot like after any other occupied slot, until it claims a slot or meets a true
// duplicate. So every outpoint has exactly one claiming lane and each later copy reports it: a collision can
// neither fail a valid block nor hide a double spend behind another outpoint. The host confirms the reported
// pairs against the full keys once more (a cross-check; it clears nothing the kernel got right).
__device__ __forceinline__ uint64_t outpoint_fp(const uint32_t k[8], uint32_t idx) {
    uint64_t h = (uint64_t(k[0]) << 32 | k[1]) ^ (uint64_t(k[2]) << 17) ^ (uint64_t(k[3]) * 0x9E3779B97F4A7C15ull) ^
                 (uint64_t(k[4]) << 7) ^ (uint64_t(k[5]) << 29) ^ k[6] ^ (uint64_t(k[7]) << 41) ^
                 (uint64_t(idx) * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 31;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
    return h;
}

// record r names the outpoint (k, idx): all 32 txid bytes and the index byte
__device__ __forceinline__ bool same_outpoint(const UtxoKeyRec& r, const uint32_t k[8], uint32_t idx) {
    uint32_t d = (r.index & 0xffu) ^ idx;
#pragma unroll
    for (int w = 0; w < 8; ++w) d |= ld_u32(r.txid + 4 * w) ^ k[w];
    return d == 0;
}

__global__ __launch_bounds__(256) void block_dup_kernel(const UtxoKeyRec* __restrict__ recs, int64_t n,
                                                        unsigned long long* __restrict__ scratch, uint32_t mask,
                                                        uint32_t* __restrict__ dup_of) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const uint32_t idx = recs[i].index & 0xffu;
    const uint64_t fp = outpoint_fp(k, idx);
    const unsigned long long want = fp & ~0xFFFFFFull;
    const unsigned long long mine = want | (uint64_t(i + 1) & 0xFFFFFFull);  // n < 2^24: lane + 1 fits, and is not 0
    uint32_t s = uint32_t(fp) & mask;
    uint32_t res = 0;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(&scratch[s], 0ull, mine);
        if (prev == 0ull) break;  // claimed: first occurrence
        if ((prev & ~0xFFFFFFull) == want) {
            const int64_t w = int64_t(prev & 0xFFFFFFull) - 1;  // the claiming lane; records are inputs, never written
            if (w >= 0 && w < n && same_outpoint(recs[w], k, idx)) {
                res = uint32_t(w) + 1u;
                break;
            }
        }
        s = (s + 1) & mask;
    }
    dup_of[i] = res;
}

// K11: per-tx fee = sum(spent amounts) - sum(output amounts), int64 smallest units; missing[t] counts
// inputs not found with the wanted tag.
__global__ __launch_bounds__(256) void block_fee_kernel(const uint8_t* __restrict__ tags,
                                                        const UtxoPayload* __restrict__ pay,
                                                        const int32_t* __restrict__ in_start,
                                                        const uint64_t* __restrict__ out_amount,
                                                        const int32_t* __restrict__ out_start, int64_t n_tx,
                                                        uint32_t want_tag, int64_t* __restrict__ fee,
                                                        uint32_t* __restrict__ missing) {
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n_tx) return;
    int64_t acc = 0;
    uint32_t miss = 0;
    for (int32_t k = in_start[t]; k < in_start[t + 1]; ++k) {
        if (tags[k] != want_tag || pay[k].addr_len == 0) ++miss;
        acc += int64_t(pay[k].amount);
    }
    for (int32_t k = out_start[t]; k < out_start[t + 1]; ++k) acc -= int64_t(out_amount[k]);
    fee[t] = acc;
    missing[t] = miss;
}

void utxo_block_inputs(int64_t h, const uint8_t* keys, int64_t n_in, const int32_t* in_start,
                       const uint64_t* out_amount, int64_t n_out, const int32_t* out_start, int64_t n_tx,
                       uint32_t want_tag, BlockInputsOut& r) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    r.n_dup = 0;
    if (n_tx == 0) {  // no tx, so no input either: nothing to write
        return;
    }
    if (n_in >= (int64_t(1) << 24)) throw std::invalid_argument("too many inputs for one block pass");
    uint32_t log2 = 8;
    while ((int64_t(1) << log2) < 2 * n_in) ++log2;
    const uint32_t scap = 1u << log2;
    // Two arenas, one transfer each: the four inputs are packed into one pinned region laid out as the
    // device arena (one H2D), the five outputs are written into one device arena (one D2H), instead of
    // a copy call per array (each hipMemcpyAsync is ~5 us of host time on the block path).
    size_t in_off[5] = {0}, out_off[6] = {0};
    {
        const size_t in_n[4] = {sizeof(UtxoKeyRec) * size_t(n_in), 8 * size_t(n_out), 4 * size_t(n_tx + 1),
                                4 * size_t(n_tx + 1)};
        for (int i = 0; i < 4; ++i) in_off[i + 1] = align256(in_off[i] + in_n[i]);
        const size_t out_n[5] = {size_t(n_in), sizeof(UtxoPayload) * size_t(n_in), 4 * size_t(n_in),
                                 8 * size_t(n_tx), 4 * size_t(n_tx)};
        for (int i = 0; i < 5; ++i) out_off[i + 1] = align256(out_off[i] + out_n[i]);
    }
    PooledBuf<uint8_t> d_in(in_off[4]), d_outa(out_off[5]);
    PooledBuf<unsigned long long> d_scratch(scap);
    auto* d_keys = reinterpret_cast<UtxoKeyRec*>(d_in.p + in_off[0]);
    auto* d_out = reinterpret_cast<uint64_t*>(d_in.p + in_off[1]);
    auto* d_in_start = reinterpret_cast<int32_t*>(d_in.p + in_off[2]);
    auto* d_out_start = reinterpret_cast<int32_t*>(d_in.p + in_off[3]);
    auto* d_tags = d_outa.p + out_off[0];
    auto* d_pay = reinterpret_cast<UtxoPayload*>(d_outa.p + out_off[1]);
    auto* d_dup = reinterpret_cast<uint32_t*>(d_outa.p + out_off[2]);
    auto* d_fee = reinterpret_cast<int64_t*>(d_outa.p + out_off[3]);
    auto* d_miss = reinterpret_cast<uint32_t*>(d_outa.p + out_off[4]);
    StagedIO io(in_off[4] + out_off[5]);
    uint8_t* hin = io.h2d_take(in_off[4]);
    auto put = [&](int i, const void* src, size_t n) {  // (an empty input array's pointer may be null)
        if (n) std::memcpy(hin + in_off[i], src, n);
    };
    put(0, keys, sizeof(UtxoKeyRec) * size_t(n_in));
    put(1, out_amount, 8 * size_t(n_out));
    put(2, in_start, 4 * size_t(n_tx + 1));
    put(3, out_start, 4 * size_t(n_tx + 1));
    io.h2d_issue(d_in.p, hin, in_off[4]);
    node_memset(d_scratch.p, 0, sizeof(unsigned long long) * scap, "memset scratch");
    hipStream_t st = node_stream();
    if (n_in) {
        launch(utxo_lookup_kernel, n_in, st, "utxo_lookup_kernel", t.tab, t.pay, t.cap - 1, d_keys, n_in, d_tags, d_pay);
        launch(block_dup_kernel, n_in, st, "block_dup_kernel", d_keys, n_in, d_scratch.p, scap - 1, d_dup);
    }
    launch(block_fee_kernel, n_tx, st, "block_fee_kernel", d_tags, d_pay, d_in_start, d_out, d_out_start, n_tx, want_tag,
           d_fee, d_miss);
    const uint8_t* hout = io.d2h_arena(d_outa.p, out_off[5]);
    io.finish("block inputs");  // one sync, then each output copied once out of the pinned staging
    if (n_in) {  // (an empty numpy array's data pointer may be null)
        std::memcpy(r.tags, hout + out_off[0], size_t(n_in));
        std::memcpy(r.payload, hout + out_off[1], sizeof(UtxoPayload) * size_t(n_in));
        std::memcpy(r.dup_of, hout + out_off[2], 4 * size_t(n_in));
    }
    std::memcpy(r.fee, hout + out_off[3], 8 * size_t(n_tx));
    std::memcpy(r.missing, hout + out_off[4], 4 * size_t(n_tx));
    // cross-check of the reported duplicates (the kernel compared the same 33 key bytes before reporting one)
    const UtxoKeyRec* kr = reinterpret_cast<const UtxoKeyRec*>(keys);
    for (int64_t i = 0; i < n_in; ++i) {
        if (!r.dup_of[i]) continue;
        const uint32_t w = r.dup_of[i] - 1;
        if (w >= uint64_t(n_in) || std::memcmp(kr[i].txid, kr[w].txid, 32) != 0 ||
            (kr[i].index & 0xffu) != (kr[w].index & 0xffu))
            r.dup_of[i] = 0;  // not a duplicate
        else
            ++r.n_dup;
    }
}

// K12: SHA-256 over (txid || index byte) of every entry with `tag`, sorted by (txid, index). The entries
// are collected on the device (utxo_collect_kernel), sorted with a stable LSD radix sort (hipCUB): index,
// then the txid's four 64-bit big-endian words from least to most significant; the message is gathered on
// the device and hashed on the host (Merkle–Damgard is sequential).

// column c of the sort: 0 = index, 1..4 = big-endian txid word (4 - c), gathered through perm
__global__ __launch_bounds__(256) void sort_column_kernel(const UtxoKeyRec* __restrict__ recs,
                                                          const uint32_t* __restrict__ perm, uint32_t n, int c,
                                                          uint64_t* __restrict__ col) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const UtxoKeyRec& r = recs[perm[i]];
    if (c == 0) {
        col[i] = r.index & 0xffu;
        return;
    }
    const uint8_t* b = r.txid + 8 * (4 - c);
    uint64_t v = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) v = (v << 8) | b[q];
    col[i] = v;
}

__global__ __launch_bounds__(256) void iota_kernel(uint32_t* __restrict__ p, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = i;
}

__global__ __launch_bounds__(256) void set_message_kernel(const UtxoKeyRec* __restrict__ recs,
                                                          const uint32_t* __restrict__ perm, uint32_t n,
                                                          uint8_t* __restrict__ msg) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const UtxoKeyRec& r = recs[perm[i]];
    uint8_t* o = msg + size_t(i) * 33;
#pragma unroll
    for (int q = 0; q < 32; ++q) o[q] = r.txid[q];
    o[32] = uint8_t(r.index);
}

// The n (> 0) collected records of one table as K12's message, 33 bytes each in (txid, index) order, in a
// device buffer; sorted and gathered on stream `st`. The sort's scratch goes back to the pool on return, so
// the call ends with a sync of `st`.
static PooledBuf<uint8_t> k12_sorted_message(const UtxoKeyRec* recs, uint32_t n, hipStream_t st) {
    PooledBuf<uint32_t> perm_a(n), perm_b(n);
    PooledBuf<uint64_t> col_a(n), col_b(n);
    launch(iota_kernel, n, st, "iota_kernel", perm_a.p, n);
    size_t temp_bytes = 0;
    stream_check(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, col_a.p, col_b.p, perm_a.p, perm_b.p, n, 0, 64, st),
                 "radix sort sizing");
    PooledBuf<uint8_t> temp(temp_bytes);
    uint32_t* pa = perm_a.p;
    uint32_t* pb = perm_b.p;
    for (int c = 0; c <= 4; ++c) {  // least significant column first; radix sort is stable
        launch(sort_column_kernel, n, st, "sort_column_kernel", recs, pa, n, c, col_a.p);
        stream_check(hipcub::DeviceRadixSort::SortPairs(temp.p, temp_bytes, col_a.p, col_b.p, pa, pb, n, 0,
                                                        c == 0 ? 8 : 64, st),
                     "radix sort");
        std::swap(pa, pb);
    }
    PooledBuf<uint8_t> d_msg(size_t(n) * 33);
    launch(set_message_kernel, n, st, "set_message_kernel", recs, pa, n, d_msg.p);
    stream_check(hipStreamSynchronize(st), "k12 sort sync");
    return d_msg;
}

std::vector<uint8_t> utxo_set_message(int64_t h, uint32_t tag, uint64_t* count_out) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    PooledBuf<UtxoKeyRec> recs(t.cap);
    collect(t, tag, recs.p, nullptr, t.d_counter);
    uint32_t n = 0;
    node_d2h(&n, t.d_counter, sizeof(uint32_t), "d2h n");
    if (count_out) *count_out = n;
    std::vector<uint8_t> msg(size_t(n) * 33);
    if (n) {
        const PooledBuf<uint8_t> d_msg = k12_sorted_message(recs.p, n, node_stream());
        node_d2h(msg.data(), d_msg.p, msg.size(), "d2h message");
    }
    return msg;
}

// ---- K12 off the block path: the block thread takes a snapshot (one collection launch on the node stream,
// so it sees exactly this block's table; no host sync), a worker thread turns it into the digest (sort and
// gather on the aux stream, chunked D2H into pinned buffers overlapped with the host SHA-256). The next
// block's kernels never queue behind the sort, and the 33-byte-per-UTXO message never becomes one host
// allocation (165 MB at 5 M UTXOs).
struct K12Snap {
    int device = 0;
    uint32_t cap = 0;
    PooledBuf<UtxoKeyRec> recs;
    PooledBuf<uint32_t> count;
    hipEvent_t ready = nullptr;
    K12Snap(uint32_t c) : cap(c), recs(c), count(1) {}
};
static std::mutex g_k12_mu;
static std::unordered_map<int64_t, std::unique_ptr<K12Snap>> g_k12;
static int64_t g_k12_next = 1;

int64_t utxo_k12_snapshot(int64_t h, uint32_t tag) {
    std::unique_ptr<K12Snap> s;
    {
        std::lock_guard<std::mutex> lk(g_ut_mu);
        UtxoTableDev& t = table(h);
        s = std::make_unique<K12Snap>(t.cap);
        s->device = t.device;
        collect(t, tag, s->recs.p, nullptr, s->count.p);
        stream_check(hipEventCreateWithFlags(&s->ready, hipEventDisableTiming), "hipEventCreate");
        stream_check(hipEventRecord(s->ready, node_stream()), "hipEventRecord");
    }
    std::lock_guard<std::mutex> g(g_k12_mu);
    const int64_t id = g_k12_next++;
    g_k12[id] = std::move(s);
    return id;
}

std::vector<uint8_t> utxo_k12_digest(int64_t id, uint64_t* count_out) {
    std::unique_ptr<K12Snap> s;
    {
        std::lock_guard<std::mutex> g(g_k12_mu);
        auto it = g_k12.find(id);
        if (it == g_k12.end()) throw std::invalid_argument("bad K12 snapshot id");
        s = std::move(it->second);
        g_k12.erase(it);
    }
    stream_check(hipSetDevice(s->device), "hipSetDevice");
    hipStream_t st = aux_stream();
    stream_check(hipStreamWaitEvent(st, s->ready, 0), "hipStreamWaitEvent");
    uint32_t n = 0;
    stream_check(hipMemcpyAsync(&n, s->count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "d2h k12 count");
    stream_check(hipStreamSynchronize(st), "k12 count sync");
    if (count_out) *count_out = n;
    HostSha256 sha;
    if (n) {
        const PooledBuf<uint8_t> d_msg = k12_sorted_message(s->recs.p, n, st);
        // two pinned staging buffers: chunk k+1 is copied while chunk k is hashed
        constexpr size_t kChunk = size_t(16) << 20;
        static uint8_t* pinned[2] = {nullptr, nullptr};
        static std::mutex pin_mu;
        std::lock_guard<std::mutex> pl(pin_mu);
        for (auto& b : pinned)
            if (!b) stream_check(hipHostMalloc(reinterpret_cast<void**>(&b), kChunk, hipHostMallocDefault), "hipHostMalloc");
        hipEvent_t ev[2];
        for (auto& e : ev) stream_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
        const size_t total = size_t(n) * 33;
        auto issue = [&](size_t off, int b) {
            const size_t len = std::min(kChunk, total - off);
            stream_check(hipMemcpyAsync(pinned[b], d_msg.p + off, len, hipMemcpyDeviceToHost, st), "d2h k12 chunk");
            stream_check(hipEventRecord(ev[b], st), "hipEventRecord");
            return len;
        };
        size_t off = 0;
        int b = 0;
        size_t len = issue(0, 0);
        while (len) {
            stream_check(hipEventSynchronize(ev[b]), "k12 chunk sync");
            const size_t next = off + len;
            size_t next_len = 0;
            if (next < total) next_len = issue(next, 1 - b);
            sha.update(pinned[b], len);
            off = next;
            len = next_len;
            b = 1 - b;
        }
        stream_check(hipStreamSynchronize(st), "k12 sync");  // the pooled buffers may be reused after this
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    (void)hipEventDestroy(s->ready);
    std::vector<uint8_t> digest(32);
    sha.final(digest.data());
    return digest;
}

// ---- test hooks: the suite engineers probe chains and K10 fingerprint collisions from the device's own hash
// functions and checks slot layouts against the raw table. Not called by the node.
__global__ __launch_bounds__(256) void utxo_debug_hash_kernel(const UtxoKeyRec* __restrict__ recs, int64_t n,
                                                              uint32_t mask, uint32_t* __restrict__ home,
                                                              uint64_t* __restrict__ fp) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8];
    load_key(recs[i], k);
    const uint32_t idx = recs[i].index & 0xffu;
    home[i] = slot_hash(k, idx) & mask;
    fp[i] = outpoint_fp(k, idx);
}

void utxo_debug_hashes(const uint8_t* recs, int64_t n, uint32_t log2_cap, uint32_t* home_out, uint64_t* fp_out) {
    if (log2_cap < 8 || log2_cap > 31) throw std::invalid_argument("log2 capacity must be in [8, 31]");
    if (n == 0) return;
    node_device_enter();
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<uint32_t> dh(n);
    PooledBuf<uint64_t> df(n);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * size_t(n), "h2d recs");
    launch(utxo_debug_hash_kernel, n, node_stream(), "utxo_debug_hash_kernel", d.p, n, (1u << log2_cap) - 1u, dh.p,
           df.p);
    node_d2h(home_out, dh.p, sizeof(uint32_t) * size_t(n), "d2h homes");
    node_d2h(fp_out, df.p, sizeof(uint64_t) * size_t(n), "d2h fingerprints");
}

std::vector<uint8_t> utxo_debug_slots(int64_t h) {
    std::lock_guard<std::mutex> lk(g_ut_mu);
    UtxoTableDev& t = table(h);
    std::vector<uint8_t> out(sizeof(UtxoSlot) * size_t(t.cap));
    node_d2h(out.data(), t.tab, out.size(), "d2h slots");  // on the node stream: behind any pending async apply
    return out;
}

}  // namespace upow
