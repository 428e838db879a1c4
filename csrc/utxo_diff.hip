// UTXO diff: which entries differ between the HBM UTXO table (utxo_table.hip) and a set of host records, in one
// pass: probe each foreign record, compare it on a hit and mark the slot, then sweep the slots for live ones that
// nobody marked. An entry and its canonical bytes are those of the state digest (native.h).
#include <hip/hip_runtime.h>

#include <chrono>

#include "utxo_dev.h"

namespace upow {

enum : uint8_t { DIFF_SAME = 0, DIFF_MISSING = 1, DIFF_CHANGED = 2 };
constexpr uint32_t DIFF_CHUNK = 1u << 20;  // records of O on the device at a time: 126 MB with their payloads
// counters of the sweep (64-bit words): a block adds into the stripe its number names (one 128-byte line each) and
// the host sums the stripes
enum : int { DC_LIVE = 0, DC_SEEN = 1, DC_WORDS = 16, DC_STRIPES = 64 };
constexpr uint32_t DIFF_ITEMS = 4, DIFF_TILE = 256 * DIFF_ITEMS;

// What E holds of a payload besides the address: L (33, 64 or 0), and with L = 0 a zero amount and flag.
struct PayCanon {
    uint32_t amount_lo, amount_hi, len, flag;
};
__device__ __forceinline__ PayCanon pay_canon(const UtxoPayload* __restrict__ pp) {
    if (!pp) return {0u, 0u, 0u, 0u};
    const uint4 h = *reinterpret_cast<const uint4*>(pp);
    if (h.z != 33u && h.z != 64u) return {0u, 0u, 0u, 0u};
    return {h.x, h.y, h.z, h.w & PAY_STAKE};
}
// addr[0:len] of two payloads with equal len (33 or 64) as 16-byte words; the bytes past 33 are masked off
__device__ __forceinline__ bool addr_eq(const UtxoPayload* __restrict__ a, const UtxoPayload* __restrict__ b,
                                        uint32_t len) {
    const uint4* qa = reinterpret_cast<const uint4*>(a->addr);
    const uint4* qb = reinterpret_cast<const uint4*>(b->addr);
    const uint4 a0 = qa[0], a1 = qa[1], a2 = qa[2], b0 = qb[0], b1 = qb[1], b2 = qb[2];
    uint32_t d = (a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) |
                 (a1.z ^ b1.z) | (a1.w ^ b1.w);
    if (len == 33u) return (d | ((a2.x ^ b2.x) & 0xffu)) == 0u;
    const uint4 a3 = qa[3], b3 = qb[3];
    d |= (a2.x ^ b2.x) | (a2.y ^ b2.y) | (a2.z ^ b2.z) | (a2.w ^ b2.w) | (a3.x ^ b3.x) | (a3.y ^ b3.y) |
         (a3.z ^ b3.z) | (a3.w ^ b3.w);
    return d == 0u;
}

// One lane per record of the chunk. An absent outpoint is DIFF_MISSING. A live one has its canonical entry compared
// with the record's (tag, L, stake flag, amount, addr[0:L]; opay null: L = 0 on the record's side) and bit `slot`
// of `seen` set: the OR's result is not used, so no lane waits for the atomic. The probe walk is find_live's, at
// most mask + 1 steps. The table and its payloads are only read.
__global__ __launch_bounds__(256) void utxo_diff_match_kernel(const UtxoSlot* __restrict__ tab,
                                                              const UtxoPayload* __restrict__ pay, uint32_t mask,
                                                              const UtxoKeyRec* __restrict__ recs,
                                                              const UtxoPayload* __restrict__ opay, uint32_t n,
                                                              uint8_t* __restrict__ status,
                                                              uint32_t* __restrict__ seen) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2* w = reinterpret_cast<const uint2*>(recs + i);  // 40-byte records: 8-byte aligned
    const uint2 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    const uint32_t k[8] = {w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, w3.x, w3.y};
    const uint32_t idx = w4.x & 0xffu, tag = w4.y & 0xffu;
    const LiveEntry e = find_live<false>(tab, mask, k, idx);
    if (e.slot == NO_SLOT) {
        status[i] = DIFF_MISSING;
        return;
    }
    atomicOr(&seen[e.slot >> 5], 1u << (e.slot & 31u));
    const UtxoPayload* mine = opay ? opay + i : nullptr;
    const PayCanon a = pay_canon(mine), b = pay_canon(pay + e.slot);
    bool same = meta_tag(e.meta) == tag && a.len == b.len && a.flag == b.flag && a.amount_lo == b.amount_lo &&
                a.amount_hi == b.amount_hi;
    if (same && a.len) same = addr_eq(mine, pay + e.slot, a.len);
    status[i] = same ? DIFF_SAME : DIFF_CHANGED;
}

// A block sweeps DIFF_TILE consecutive slots, DIFF_ITEMS per lane. A live slot whose tag is in tag_mask and whose
// `seen` bit is clear is an extra; its record and payload are written while its position is below `limit`. The
// block takes its extras' positions with ONE returning atomic (ballot counts per wave, summed through LDS), as
// utxo_owner_compact_kernel does, so *n_extra ends as the exact count. The live entries in tag_mask and the seen
// bits met on live slots are summed the same way and added once per block to the block's stripe of `cnt`. Every
// lane reaches both barriers; nothing is waited for but the block's own lanes.
__global__ __launch_bounds__(256) void utxo_diff_extra_kernel(const UtxoSlot* __restrict__ tab,
                                                              const UtxoPayload* __restrict__ pay, uint32_t cap,
                                                              uint32_t tag_mask, const uint32_t* __restrict__ seen,
                                                              uint32_t limit, UtxoKeyRec* __restrict__ out,
                                                              UtxoPayload* __restrict__ pay_out,
                                                              uint32_t* __restrict__ n_extra,
                                                              unsigned long long* __restrict__ cnt_stripes) {
    __shared__ uint32_t wave_n[4], wave_live[4], wave_seen[4], block_base;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t meta[DIFF_ITEMS], before[DIFF_ITEMS];  // an extra's meta word (0: none), extras ahead of it in the wave
    uint32_t mine = 0, live_n = 0, seen_n = 0;      // wave-uniform
#pragma unroll
    for (uint32_t i = 0; i < DIFF_ITEMS; ++i) {
        const uint32_t s = blockIdx.x * DIFF_TILE + i * 256u + threadIdx.x;
        const uint32_t m = s < cap ? tab[s].meta : 0u;
        const bool live = meta_state(m) == ST_FULL;
        const bool marked = live && ((seen[s >> 5] >> (s & 31u)) & 1u);
        const uint32_t tag = meta_tag(m);
        const bool counted = live && tag < 32u && ((tag_mask >> tag) & 1u);
        const bool extra = counted && !marked;
        meta[i] = extra ? m : 0u;  // a FULL meta word is never 0
        const unsigned long long peers = __ballot(extra);
        before[i] = mine + uint32_t(__popcll(peers & ((1ull << lane) - 1ull)));
        mine += uint32_t(__popcll(peers));
        live_n += uint32_t(__popcll(__ballot(counted)));
        seen_n += uint32_t(__popcll(__ballot(marked)));
    }
    if (lane == 0) wave_n[wave] = mine, wave_live[wave] = live_n, wave_seen[wave] = seen_n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t n = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        const uint32_t l = wave_live[0] + wave_live[1] + wave_live[2] + wave_live[3];
        const uint32_t sn = wave_seen[0] + wave_seen[1] + wave_seen[2] + wave_seen[3];
        block_base = n ? atomicAdd(n_extra, n) : 0u;
        unsigned long long* cnt = cnt_stripes + size_t(blockIdx.x & (DC_STRIPES - 1)) * DC_WORDS;
        if (l) atomicAdd(&cnt[DC_LIVE], static_cast<unsigned long long>(l));
        if (sn) atomicAdd(&cnt[DC_SEEN], static_cast<unsigned long long>(sn));
    }
    __syncthreads();
    uint32_t base = block_base;
    for (uint32_t v = 0; v < wave; ++v) base += wave_n[v];
#pragma unroll
    for (uint32_t i = 0; i < DIFF_ITEMS; ++i) {
        const uint32_t o = base + before[i];
        if (meta[i] == 0u || o >= limit) continue;
        const uint32_t s = blockIdx.x * DIFF_TILE + i * 256u + threadIdx.x;
        const uint4* k = reinterpret_cast<const uint4*>(tab + s);
        const uint4 k0 = k[0], k1 = k[1];
        uint2* r = reinterpret_cast<uint2*>(out + o);  // the table's key words are the txid's bytes in order
        r[0] = make_uint2(k0.x, k0.y);
        r[1] = make_uint2(k0.z, k0.w);
        r[2] = make_uint2(k1.x, k1.y);
        r[3] = make_uint2(k1.z, k1.w);
        r[4] = make_uint2(meta_index(meta[i]), meta_tag(meta[i]));
        const uint4* p = reinterpret_cast<const uint4*>(pay + s);
        uint4* q = reinterpret_cast<uint4*>(pay_out + o);
#pragma unroll
        for (int j = 0; j < 5; ++j) q[j] = p[j];
    }
}

void utxo_diff(int64_t h, const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t tag_mask,
               uint32_t limit, uint32_t chunk_records, UtxoDiffOut& out) {
    out = UtxoDiffOut{};
    if (n < 0 || n > int64_t(0x7fffffff)) throw std::invalid_argument("record count must be in [0, 2^31)");
    const auto t0 = std::chrono::steady_clock::now();
    std::lock_guard<std::mutex> lk(g_ut_mu);  // one hold from the first launch to the last D2H: one table state
    const auto t1 = std::chrono::steady_clock::now();
    UtxoTableDev& t = table(h);
    hipStream_t st = node_stream();
    const uint32_t chunk =
        uint32_t(std::min<int64_t>(chunk_records ? chunk_records : DIFF_CHUNK, std::max<int64_t>(n, 1)));
    const uint32_t lim = std::min(limit, t.cap);  // extras cannot exceed the slots
    PooledBuf<uint32_t> seen(t.cap / 32u), n_extra(1);
    PooledBuf<unsigned long long> cnt(DC_STRIPES * DC_WORDS);
    PooledBuf<UtxoKeyRec> d(chunk), xr(lim);
    PooledBuf<UtxoPayload> dp(pay_or_null ? chunk : 0), xp(lim);
    PooledBuf<uint8_t> d_status{size_t(n)};
    node_memset(seen.p, 0, sizeof(uint32_t) * (t.cap / 32u), "memset seen");
    node_memset(n_extra.p, 0, sizeof(uint32_t), "memset extra count");
    node_memset(cnt.p, 0, sizeof(unsigned long long) * DC_STRIPES * DC_WORDS, "memset diff counters");
    for (int64_t at = 0; at < n; at += chunk) {  // back to back: the stream orders a chunk's upload behind the
        const int64_t m = std::min<int64_t>(chunk, n - at);  // kernel that read the one before
        node_h2d(d.p, recs + size_t(at) * sizeof(UtxoKeyRec), sizeof(UtxoKeyRec) * size_t(m), "h2d diff recs");
        if (pay_or_null)
            node_h2d(dp.p, pay_or_null + size_t(at) * sizeof(UtxoPayload), sizeof(UtxoPayload) * size_t(m),
                     "h2d diff payload");
        launch(utxo_diff_match_kernel, m, st, "utxo_diff_match_kernel", t.tab, t.pay, t.cap - 1, d.p,
               pay_or_null ? dp.p : nullptr, uint32_t(m), d_status.p + at, seen.p);
    }
    launch(utxo_diff_extra_kernel, (int64_t(t.cap) + DIFF_ITEMS - 1) / DIFF_ITEMS, st, "utxo_diff_extra_kernel", t.tab,
           t.pay, t.cap, tag_mask, seen.p, lim, xr.p, xp.p, n_extra.p, cnt.p);
    std::vector<unsigned long long> stripes(DC_STRIPES * DC_WORDS);
    uint32_t extra = 0;
    node_d2h(stripes.data(), cnt.p, sizeof(unsigned long long) * stripes.size(), "d2h diff counters");
    node_d2h(&extra, n_extra.p, sizeof extra, "d2h extra count");
    out.status.resize(size_t(n));
    node_d2h(out.status.data(), d_status.p, size_t(n), "d2h diff status");
    const size_t listed = std::min(extra, lim);
    out.extra_recs.resize(listed * sizeof(UtxoKeyRec));
    out.extra_pay.resize(listed * sizeof(UtxoPayload));
    node_d2h(out.extra_recs.data(), xr.p, out.extra_recs.size(), "d2h extra recs");
    node_d2h(out.extra_pay.data(), xp.p, out.extra_pay.size(), "d2h extra payload");
    uint64_t seen_bits = 0, found = 0;
    for (int i = 0; i < DC_STRIPES; ++i) {
        out.live += stripes[size_t(i) * DC_WORDS + DC_LIVE];
        seen_bits += stripes[size_t(i) * DC_WORDS + DC_SEEN];
    }
    for (uint8_t s : out.status) found += s != DIFF_MISSING;
    if (seen_bits > found) throw std::runtime_error("utxo_diff: more slots marked than records found");
    out.extra = extra;
    out.repeated = found - seen_bits;  // every record that found a slot set its bit: exact in any arrival order
    const auto t2 = std::chrono::steady_clock::now();
    out.wait_seconds = std::chrono::duration<double>(t1 - t0).count();
    out.hold_seconds = std::chrono::duration<double>(t2 - t1).count();
}

}  // namespace upow
