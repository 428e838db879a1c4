// Holders report: per-owner totals of the whole HBM UTXO set (utxo_table.hip) in one table pass (a hash
// aggregation by owner key).
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include <string>

#include "utxo_dev.h"

namespace upow {

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

}  // namespace upow
