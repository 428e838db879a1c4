// K14: outputs owned by an address (reference `database.py:909-937,1138-1205`: balance / spendable outputs
// by address), as one pass over the HBM UTXO table (utxo_table.hip) for up to SCAN_BATCH_MAX queries at once
// (the reference's `address = ANY($1)` takes an address list natively). A single query is a batch of one.
#include "utxo_dev.h"

namespace upow {

// One lane per table slot. The queries are device-resident records sorted by
// owner fingerprint; each block stages the sorted fingerprints into LDS once (the only barrier, before any
// lane returns). A live slot looks its fingerprint up with a lower_bound whose step count is uniform
// (it depends on nq alone); only a slot whose fingerprint is in the table reads its payload line, and then
// every query of the equal-fingerprint run is tested on its own (length, its tag mask, its stake selector,
// the four address words), so colliding fingerprints and one address under several filters each get
// exactly their matches. A match is compacted with one returning atomic and carries the query's position
// in the sorted table (`qbase` + its place in this launch); the amount goes into totals[query] with a
// 64-bit atomic: matches are rare and the lanes of a wave may hit different queries.
// stake_sel: 0 any output, 1 only is_stake = 0 (spendable), 2 only is_stake = 1
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

// the single query: a batch of one
std::vector<uint8_t> utxo_address_scan(int64_t h, const uint8_t* addr, uint32_t len, uint32_t tag_mask,
                                       uint32_t stake_sel, std::vector<uint8_t>& payload_out, uint64_t* total_out) {
    if (len > 64) throw std::invalid_argument("address is at most 64 bytes");
    AddressBatchOut r;
    utxo_address_scan_batch(h, addr, &len, &tag_mask, &stake_sel, 1, r);  // reads addr[0:len] of row 0
    payload_out = std::move(r.payload);
    *total_out = r.totals[0];
    return std::move(r.recs);
}

}  // namespace upow
