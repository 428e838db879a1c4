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
//
// This file is the table itself; the layouts and device helpers are in utxo_dev.h, and the passes that only
// read the table are files of their own: utxo_scan.hip (K14), utxo_owners.hip (holders report),
// utxo_block.hip (K10/K11 block input pass, K12 set hash).
#include <unordered_map>

#include "utxo_dev.h"

namespace upow {

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
// and K12's callers sort).
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

// ------------------------------------------------------------------------------------------------
std::mutex g_ut_mu;
static std::unordered_map<int64_t, UtxoTableDev> g_tables;
static int64_t g_next_handle = 1;

UtxoTableDev& table(int64_t h) {
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

void lookup(const UtxoTableDev& t, const UtxoKeyRec* recs, int64_t n, uint8_t* tags_out, UtxoPayload* pay_out) {
    launch(utxo_lookup_kernel, n, node_stream(), "utxo_lookup_kernel", t.tab, t.pay, t.cap - 1, recs, n, tags_out,
           pay_out);
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
    lookup(t, d.p, n, o.p, po.p);
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

void collect(const UtxoTableDev& t, uint32_t tag, UtxoKeyRec* out, UtxoPayload* pay_out, uint32_t* count) {
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
