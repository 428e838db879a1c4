// UTXO proofs: the RFC 6962 Merkle tree over the live entries of the HBM UTXO table (utxo_table.hip), or over
// host-supplied records, and the audit paths out of it. The definition is in native.h; csrc/utxo_merkle_host.cpp is
// the same on the host and holds the snapshot registry and the part of a proof both share.
//
// Build: collect (utxo_table.hip) -> cut to the wanted tags -> K12's radix sort with the tag as one more column
// (utxo_block.hip) -> one lane per sorted entry hashes its leaf and writes its slot -> one launch per level, one lane
// per parent. The tree is built level by level: neighbours are paired and an unpaired last node is promoted
// unchanged, which is the RFC's recursive split at the largest power of two below n (every left subtree is complete).
// A 5 M-entry tree takes 23 level launches, the small ones about 6 us each. Finishing the levels under one
// workgroup's worth of nodes in a single block was measured not to matter (under 2 % of the build, docs/PERF.md
// "UTXO proofs"), so there is one launch per level and no second kernel.
// Prove: one lane per query runs a lower-bound search over the sorted slots; the host turns the bounds into leaf
// positions; one lane per (leaf, level) gathers sibling (position >> level) ^ 1 where the level has it, and one more
// lane per leaf its slot. Two round trips: the bounds come back (8 bytes per query) and the positions go up before
// the gather, whose packed rows are the second D2H.
// The leaf and level kernels take `per`, the items of a 256-thread block (256, or the launch lever); the two prove
// kernels always run 256 items per block (a call with more than 256 queries crosses their block boundaries).
#include <hip/hip_runtime.h>

#include "sha256_dev.h"
#include "utxo_dev.h"
#include "utxo_merkle.h"

namespace upow {

namespace {

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// item i of this lane under `per` items per block; false: the lane has none
__device__ __forceinline__ bool my_item(uint32_t per, uint64_t n, uint64_t& i) {
    i = uint64_t(blockIdx.x) * per + threadIdx.x;
    return threadIdx.x < per && i < n;
}

__device__ __forceinline__ void store_digest(uint4* at, const uint32_t st[8]) {
    at[0] = make_uint4(bswap(st[0]), bswap(st[1]), bswap(st[2]), bswap(st[3]));
    at[1] = make_uint4(bswap(st[4]), bswap(st[5]), bswap(st[6]), bswap(st[7]));
}

__constant__ uint32_t kIV[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                                0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

// tag of record r in tag_mask (tags above 31: never)?
__device__ __forceinline__ bool tag_wanted(const UtxoKeyRec& r, uint32_t tag_mask) {
    const uint32_t tag = r.tag & 0xffu;
    return tag < 32u && ((tag_mask >> tag) & 1u);
}

// how many entries of a collection the mask keeps: when it keeps them all (the node's build: every table), the
// collection is used as it is and the 120-byte-per-entry copy below is skipped. Reads the 4 tag bytes of each record.
__global__ __launch_bounds__(256) void merkle_count_kernel(const UtxoKeyRec* __restrict__ recs, uint32_t n,
                                                           uint32_t tag_mask, uint32_t* __restrict__ count) {
    // a grid-stride walk (the host caps the grid) and one add per wave at its end: an add per wave per 64 entries,
    // 78 K of them on one address at 5 M entries, measured 0.89 ms, as much as the copy this kernel is there to save
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        mine += tag_wanted(recs[i], tag_mask) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off, 64);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(count, mine);
}

// the entries of a collection whose tag's bit is set in tag_mask, compacted in any order
__global__ __launch_bounds__(256) void merkle_filter_kernel(const UtxoKeyRec* __restrict__ recs,
                                                            const UtxoPayload* __restrict__ pay, uint32_t n,
                                                            uint32_t tag_mask, UtxoKeyRec* __restrict__ out,
                                                            UtxoPayload* __restrict__ pay_out,
                                                            uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!tag_wanted(recs[i], tag_mask)) return;
    const uint32_t o = atomicAdd(count, 1u);
    out[o] = recs[i];
    pay_out[o] = pay[i];
}

// Leaf i = SHA-256(0x00 | E) of the entry that sorts i-th, and its slot. E is put together as 27 big-endian words
// (zeros after its end); the message is E moved up by one byte, 45, 78 or 109 bytes: one block for L = 0, else two.
// Both compressions run in every lane so that the wave stays uniform, and an L = 0 lane drops the second one's
// result (as the digest kernel does with its first).
__global__ __launch_bounds__(256) void merkle_leaf_kernel(const UtxoKeyRec* __restrict__ recs,
                                                          const UtxoPayload* __restrict__ pay,
                                                          const uint32_t* __restrict__ perm, uint32_t n, uint32_t per,
                                                          uint4* __restrict__ nodes, uint4* __restrict__ slots) {
    uint64_t i;
    if (!my_item(per, n, i)) return;
    const uint32_t src = perm[i];
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(recs + src);  // 40-byte records: 4-byte aligned words
    uint32_t e[27], a[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = bswap(rw[j]);
    const uint32_t idx = rw[8] & 0xffu, tag = rw[9] & 0xffu;
    uint32_t amount_lo = 0, amount_hi = 0, flags = 0, len = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = 0;
    if (pay) {
        const uint4* q = reinterpret_cast<const uint4*>(pay + src);
        const uint4 h = q[0];
        if (h.z == 33u || h.z == 64u) {
            amount_lo = h.x, amount_hi = h.y, len = h.z, flags = h.w & PAY_STAKE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 v = q[1 + j];
                a[4 * j] = v.x, a[4 * j + 1] = v.y, a[4 * j + 2] = v.z, a[4 * j + 3] = v.w;
            }
            if (len == 33u) {  // nothing past addr[32]
                a[8] &= 0xffu;
#pragma unroll
                for (int j = 9; j < 16; ++j) a[j] = 0;
            }
        }
    }
    const bool l0 = len == 0u, l33 = len == 33u;
    e[8] = (idx << 24) | (tag << 16) | (flags << 8) | len;
    e[9] = bswap(amount_lo);
    e[10] = bswap(amount_hi);
#pragma unroll
    for (int j = 0; j < 16; ++j) e[11 + j] = bswap(a[j]);
    uint32_t w1[16], w2[16];
#pragma unroll
    for (int j = 0; j < 28; ++j) {
        const uint32_t m = ((j ? e[j - 1] : 0u) << 24) | ((j < 27 ? e[j] : 0u) >> 8);
        if (j < 16) w1[j] = m;
        else w2[j - 16] = m;
    }
    // the 0x80 after the message: byte 45 (word 11), 78 (word 19) or 109 (word 27)
    w1[11] |= l0 ? 0x00800000u : 0u;
    w2[3] |= l33 ? 0x00008000u : 0u;
    w2[11] |= (!l0 && !l33) ? 0x00800000u : 0u;
    w1[15] = l0 ? 45u * 8u : w1[15];
    w2[12] = w2[13] = w2[14] = 0u;
    w2[15] = (45u + len) * 8u;
    uint32_t st[8], st2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) st[j] = kIV[j];
    dev_compress(st, w1);
#pragma unroll
    for (int j = 0; j < 8; ++j) st2[j] = st[j];
    dev_compress(st2, w2);
#pragma unroll
    for (int j = 0; j < 8; ++j) st[j] = l0 ? st[j] : st2[j];
    store_digest(nodes + 2 * i, st);
    uint4* s = slots + 7 * i;
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = make_uint4(bswap(e[4 * j]), bswap(e[4 * j + 1]), bswap(e[4 * j + 2]), bswap(e[4 * j + 3]));
    s[6] = make_uint4(bswap(e[24]), bswap(e[25]), bswap(e[26]), 44u + len);
}

// Parent p of a level = SHA-256(0x01 | left | right) of the nodes 2p, 2p + 1 below (one aligned 64-byte line, four
// uint4 loads): the first block is 0x01 and the pair's first 63 bytes, the second the right child's last byte and
// constant padding. The unpaired last node of an odd level is copied.
__global__ __launch_bounds__(256) void merkle_level_kernel(const uint4* __restrict__ below, uint64_t size,
                                                           uint4* __restrict__ above, uint64_t parents, uint32_t per) {
    uint64_t p;
    if (!my_item(per, parents, p)) return;
    const uint4* c = below + 4 * p;
    const uint4 x0 = c[0], x1 = c[1];
    if (2 * p + 1 >= size) {
        above[2 * p] = x0;
        above[2 * p + 1] = x1;
        return;
    }
    const uint4 x2 = c[2], x3 = c[3];
    const uint32_t b[16] = {bswap(x0.x), bswap(x0.y), bswap(x0.z), bswap(x0.w), bswap(x1.x), bswap(x1.y),
                            bswap(x1.z), bswap(x1.w), bswap(x2.x), bswap(x2.y), bswap(x2.z), bswap(x2.w),
                            bswap(x3.x), bswap(x3.y), bswap(x3.z), bswap(x3.w)};
    uint32_t w[16], st[8];
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = ((j ? b[j - 1] : 0x01u) << 24) | (b[j] >> 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) st[j] = kIV[j];
    dev_compress(st, w);
    w[0] = (b[15] << 24) | 0x00800000u;
#pragma unroll
    for (int j = 1; j < 15; ++j) w[j] = 0u;
    w[15] = 65u * 8u;
    dev_compress(st, w);
    store_digest(above + 2 * p, st);
}

// the slot's key (txid, index, tag) against (k, idx, 0): is the slot's below?
__device__ __forceinline__ bool slot_below(const uint4* slot, const uint32_t k[8], uint32_t idx) {
    const uint4 s0 = slot[0], s1 = slot[1];
    const uint32_t e[8] = {bswap(s0.x), bswap(s0.y), bswap(s0.z), bswap(s0.w), bswap(s1.x), bswap(s1.y), bswap(s1.z), bswap(s1.w)};
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (e[j] != k[j]) return e[j] < k[j];
    return (bswap(slot[2].x) >> 16) < (idx << 8);
}
__device__ __forceinline__ bool slot_is(const uint4* slot, const uint32_t k[8], uint32_t idx) {
    const uint4 s0 = slot[0], s1 = slot[1];
    const uint32_t d = (bswap(s0.x) ^ k[0]) | (bswap(s0.y) ^ k[1]) | (bswap(s0.z) ^ k[2]) | (bswap(s0.w) ^ k[3]) |
                       (bswap(s1.x) ^ k[4]) | (bswap(s1.y) ^ k[5]) | (bswap(s1.z) ^ k[6]) | (bswap(s1.w) ^ k[7]) |
                       ((bswap(slot[2].x) >> 24) ^ idx);
    return d == 0;
}

// per query: lb = the first slot whose key is not below (txid, index, 0), and how many slots from there on have the
// query's outpoint
__global__ __launch_bounds__(256) void merkle_search_kernel(const uint4* __restrict__ slots, uint32_t n,
                                                            const UtxoKeyRec* __restrict__ queries, uint32_t q,
                                                            uint32_t* __restrict__ lb,
                                                            uint32_t* __restrict__ matches) {
    uint64_t i;
    if (!my_item(256u, q, i)) return;
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(queries + i);
    uint32_t k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = bswap(rw[j]);
    const uint32_t idx = rw[8] & 0xffu;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (slot_below(slots + 7 * uint64_t(mid), k, idx)) lo = mid + 1;
        else hi = mid;
    }
    lb[i] = lo;
    uint32_t end = lo;
    while (end < n && slot_is(slots + 7 * uint64_t(end), k, idx)) ++end;
    matches[i] = end - lo;
}

// item (leaf j, l): for l below the root's level, sibling (position >> l) ^ 1 of level l into row j where that level
// has it; for l = levels - 1, the leaf's slot. table = {offset, size} of each level in nodes.
__global__ __launch_bounds__(256) void merkle_gather_kernel(const uint4* __restrict__ nodes, const uint4* __restrict__ slots,
                                                            const uint64_t* __restrict__ table, uint32_t levels,
                                                            const uint32_t* __restrict__ pos, uint64_t items,
                                                            uint4* __restrict__ out_slots,
                                                            uint4* __restrict__ out_rows) {
    uint64_t t;
    if (!my_item(256u, items, t)) return;
    const uint64_t j = t / levels;
    const uint32_t l = uint32_t(t % levels);
    const uint64_t p = pos[j];
    if (l == levels - 1) {
#pragma unroll
        for (int x = 0; x < 7; ++x) out_slots[7 * j + x] = slots[7 * p + x];
        return;
    }
    const uint64_t sib = (p >> l) ^ 1u;
    if (sib >= table[2 * l + 1]) return;
    const uint4* at = nodes + 2 * (table[2 * l] + sib);
    uint4* o = out_rows + 2 * (j * (levels - 1) + l);
    o[0] = at[0];
    o[1] = at[1];
}

uint32_t items_per_block(uint32_t launch_lever) {
    if (launch_lever > 256u) throw std::invalid_argument("launch_lever is at most 256 (0: 256 items per block)");
    return launch_lever ? launch_lever : 256u;
}
// threads to launch so that n items at `per` a block each have a lane
int64_t lanes_for(uint64_t n, uint32_t per) { return int64_t((n + per - 1) / per) * 256; }

void release_device(MerkleSnap& s) {
    if (!s.d_arena) return;
    (void)hipSetDevice(s.device);
    (void)hipFree(s.d_arena);  // synchronises the device: nothing of the snapshot is in flight after it
    s.d_arena = nullptr;
}

const uint4* nodes_of(const MerkleSnap& s) { return reinterpret_cast<const uint4*>(s.d_arena); }
const uint4* slots_of(const MerkleSnap& s) { return reinterpret_cast<const uint4*>(s.d_arena + s.d_slots_off); }

void search_device(const MerkleSnap& s, const uint8_t* recs, int64_t q, uint32_t* lb, uint32_t* matches) {
    stream_check(hipSetDevice(s.device), "hipSetDevice");
    PooledBuf<UtxoKeyRec> d_q(q);
    PooledBuf<uint32_t> d_out(2 * size_t(q));
    node_h2d(d_q.p, recs, sizeof(UtxoKeyRec) * size_t(q), "h2d queries");
    launch(merkle_search_kernel, lanes_for(uint64_t(q), 256), node_stream(), "merkle_search_kernel", slots_of(s),
           uint32_t(s.count), d_q.p, uint32_t(q), d_out.p, d_out.p + q);
    std::vector<uint32_t> both(2 * size_t(q));
    node_d2h(both.data(), d_out.p, sizeof(uint32_t) * both.size(), "d2h bounds");  // syncs: the scratch may go back
    std::memcpy(lb, both.data(), sizeof(uint32_t) * size_t(q));
    std::memcpy(matches, both.data() + q, sizeof(uint32_t) * size_t(q));
}

void gather_device(const MerkleSnap& s, const std::vector<uint32_t>& pos, uint8_t* slots, uint8_t* rows) {
    stream_check(hipSetDevice(s.device), "hipSetDevice");
    const size_t m = pos.size(), levels = s.lv.size.size();
    const size_t slot_bytes = m * kMerkleSlot, row_bytes = m * (levels - 1) * 32;
    PooledBuf<uint32_t> d_pos(m);
    PooledBuf<uint8_t> d_out(slot_bytes + row_bytes);
    node_h2d(d_pos.p, pos.data(), sizeof(uint32_t) * m, "h2d positions");
    node_memset(d_out.p + slot_bytes, 0, row_bytes, "memset rows");
    launch(merkle_gather_kernel, lanes_for(uint64_t(m) * levels, 256), node_stream(), "merkle_gather_kernel", nodes_of(s),
           slots_of(s), reinterpret_cast<const uint64_t*>(s.d_arena + s.d_table_off), uint32_t(levels), d_pos.p,
           uint64_t(m) * levels, reinterpret_cast<uint4*>(d_out.p), reinterpret_cast<uint4*>(d_out.p + slot_bytes));
    std::vector<uint8_t> back(slot_bytes + row_bytes);
    node_d2h(back.data(), d_out.p, back.size(), "d2h proofs");  // syncs: the scratch may go back
    std::memcpy(slots, back.data(), slot_bytes);
    if (row_bytes) std::memcpy(rows, back.data() + slot_bytes, row_bytes);
}

// the snapshot of n device-resident records (pay may be null) on the current device; synchronises the node stream
int64_t build_device(const UtxoKeyRec* recs, const UtxoPayload* pay, uint32_t n, uint32_t per) {
    auto s = std::make_shared<MerkleSnap>();
    s->count = n;
    s->lv = MerkleLevels(n);
    merkle_empty_root(s->root);
    if (n) {
        stream_check(hipGetDevice(&s->device), "hipGetDevice");
        const size_t levels = s->lv.size.size();
        s->d_slots_off = align256(size_t(s->lv.nodes) * 32);
        s->d_table_off = s->d_slots_off + align256(size_t(n) * kMerkleSlot);
        s->bytes = s->d_table_off + align256(16 * levels);
        stream_check(hipMalloc(reinterpret_cast<void**>(&s->d_arena), s->bytes), "hipMalloc (Merkle snapshot)");
        s->d_release = release_device;
        s->d_search = search_device;
        s->d_gather = gather_device;
        hipStream_t st = node_stream();
        std::vector<uint64_t> table(2 * levels);
        for (size_t l = 0; l < levels; ++l) table[2 * l] = s->lv.off[l], table[2 * l + 1] = s->lv.size[l];
        node_h2d(s->d_arena + s->d_table_off, table.data(), 16 * levels, "h2d level table");
        uint4* nodes = reinterpret_cast<uint4*>(s->d_arena);
        const std::unique_ptr<SortedPerm> sorted = sort_records(recs, n, true, st);
        launch(merkle_leaf_kernel, lanes_for(n, per), st, "merkle_leaf_kernel", recs, pay, sorted->perm, n, per, nodes,
               reinterpret_cast<uint4*>(s->d_arena + s->d_slots_off));
        for (size_t l = 0; l + 1 < levels; ++l)
            launch(merkle_level_kernel, lanes_for(s->lv.size[l + 1], per), st, "merkle_level_kernel",
                   static_cast<const uint4*>(nodes + 2 * s->lv.off[l]), s->lv.size[l], nodes + 2 * s->lv.off[l + 1],
                   s->lv.size[l + 1], per);
        // syncs the stream: the pageable level table was read, and the sort's scratch may go back to the pool
        node_d2h(s->root, s->d_arena + size_t(s->lv.off.back()) * 32, 32, "d2h root");
    }
    return merkle_register(std::move(s));
}

}  // namespace

int64_t utxo_merkle_build(int64_t h, uint32_t tag_mask, uint32_t launch_lever) {
    const uint32_t per = items_per_block(launch_lever);
    std::unique_ptr<PooledBuf<UtxoKeyRec>> all;
    std::unique_ptr<PooledBuf<UtxoPayload>> all_pay;
    uint32_t n_all = 0;
    {
        std::lock_guard<std::mutex> lk(g_ut_mu);  // one hold: the collection runs behind any queued async apply
        UtxoTableDev& t = table(h);
        all = std::make_unique<PooledBuf<UtxoKeyRec>>(t.cap);
        all_pay = std::make_unique<PooledBuf<UtxoPayload>>(t.cap);
        collect(t, ANY_TAG, all->p, all_pay->p, t.d_counter);
        node_d2h(&n_all, t.d_counter, sizeof(uint32_t), "d2h n");
    }
    // from here on the snapshot's own copies only: the table may move on
    PooledBuf<uint32_t> count(1);
    uint32_t n = 0;
    if (n_all) {
        node_memset(count.p, 0, sizeof(uint32_t), "memset");
        const int64_t blocks = std::min<int64_t>((int64_t(n_all) + 255) / 256, 1024);  // four per compute unit
        launch(merkle_count_kernel, blocks * 256, node_stream(), "merkle_count_kernel", all->p, n_all, tag_mask, count.p);
        node_d2h(&n, count.p, sizeof(uint32_t), "d2h n");
    }
    if (n == n_all) return build_device(all->p, all_pay->p, n, per);  // every entry is wanted: no copy
    PooledBuf<UtxoKeyRec> recs(n);
    PooledBuf<UtxoPayload> pay(n);
    if (n) {
        node_memset(count.p, 0, sizeof(uint32_t), "memset");
        launch(merkle_filter_kernel, n_all, node_stream(), "merkle_filter_kernel", all->p, all_pay->p, n_all, tag_mask,
               recs.p, pay.p, count.p);
    }
    return build_device(recs.p, pay.p, n, per);
}

int64_t utxo_merkle_build_records(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t launch_lever) {
    const uint32_t per = items_per_block(launch_lever);
    if (n < 0 || n > int64_t(0x7fffffff)) throw std::invalid_argument("record count must be in [0, 2^31)");
    node_device_enter();
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<UtxoPayload> dp(pay_or_null ? n : 0);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * size_t(n), "h2d recs");
    if (pay_or_null) node_h2d(dp.p, pay_or_null, sizeof(UtxoPayload) * size_t(n), "h2d payload");
    const int64_t id = build_device(d.p, pay_or_null ? dp.p : nullptr, uint32_t(n), per);
    node_sync("merkle records sync");  // (n = 0: nothing was queued behind the copies' own staging)
    return id;
}

}  // namespace upow
