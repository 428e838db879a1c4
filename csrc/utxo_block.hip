// Whole-block input pass over the HBM UTXO table of utxo_table.hip (K7 + K10 + K11 in one round trip) and the
// sorted UTXO-set hash (K12).
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include <memory>
#include <unordered_map>

#include "sha256_common.h"
#include "utxo_dev.h"

namespace upow {

// K10: duplicate outpoints within a block. Each lane walks a scratch table (at most half full) from the slot
// its 64-bit fingerprint of (txid, index byte) names, with one 64-bit CAS per slot (outpoint_fp is in
// utxo_dev.h: the table file's test hook reports it too); a word packs the
// fingerprint's top 40 bits with 1 + the lane id of the lane that claimed it (so no claimed word is 0, the
// empty slot, whatever the fingerprint). A lane that meets its own 40 bits compares its 32 txid bytes and
// index byte with that lane's record: equal, it reports the lane (dup_of = winner + 1) and stops; different
// (a fingerprint collision: txids are the spender's choice, and a colliding pair costs ~2^24 hashes), it
// goes on to the next slot like after any other occupied slot, until it claims a slot or meets a true
// duplicate. So every outpoint has exactly one claiming lane and each later copy reports it: a collision can
// neither fail a valid block nor hide a double spend behind another outpoint. The host confirms the reported
// pairs against the full keys once more (a cross-check; it clears nothing the kernel got right).

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
        lookup(t, d_keys, n_in, d_tags, d_pay);
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

// column c of the sort: 0 = index, 1..4 = big-endian txid word (4 - c), 5 = tag, gathered through perm
__global__ __launch_bounds__(256) void sort_column_kernel(const UtxoKeyRec* __restrict__ recs,
                                                          const uint32_t* __restrict__ perm, uint32_t n, int c,
                                                          uint64_t* __restrict__ col) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const UtxoKeyRec& r = recs[perm[i]];
    if (c == 0 || c == 5) {
        col[i] = (c == 0 ? r.index : r.tag) & 0xffu;
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

// The sort (declared in utxo_dev.h: the Merkle build of utxo_merkle.hip orders its leaves with it, the tag as one
// more least-significant column): the least significant column first; radix sort is stable.
std::unique_ptr<SortedPerm> sort_records(const UtxoKeyRec* recs, uint32_t n, bool by_tag, hipStream_t st) {
    size_t temp_bytes = 0;
    stream_check(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, static_cast<uint64_t*>(nullptr),
                                                    static_cast<uint64_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                                    static_cast<uint32_t*>(nullptr), n, 0, 64, st),
                 "radix sort sizing");
    auto s = std::make_unique<SortedPerm>(n, temp_bytes);
    launch(iota_kernel, n, st, "iota_kernel", s->perm_a.p, n);
    uint32_t* pa = s->perm_a.p;
    uint32_t* pb = s->perm_b.p;
    for (int c = by_tag ? -1 : 0; c <= 4; ++c) {
        const int col = c < 0 ? 5 : c;
        launch(sort_column_kernel, n, st, "sort_column_kernel", recs, pa, n, col, s->col_a.p);
        stream_check(hipcub::DeviceRadixSort::SortPairs(s->temp.p, temp_bytes, s->col_a.p, s->col_b.p, pa, pb, n, 0,
                                                        c <= 0 ? 8 : 64, st),
                     "radix sort");
        std::swap(pa, pb);
    }
    s->perm = pa;
    return s;
}

// The n (> 0) collected records of one table as K12's message, 33 bytes each in (txid, index) order, in a
// device buffer; sorted and gathered on stream `st`. The sort's scratch goes back to the pool on return, so
// the call ends with a sync of `st`.
static PooledBuf<uint8_t> k12_sorted_message(const UtxoKeyRec* recs, uint32_t n, hipStream_t st) {
    const std::unique_ptr<SortedPerm> sorted = sort_records(recs, n, false, st);
    PooledBuf<uint8_t> d_msg(size_t(n) * 33);
    launch(set_message_kernel, n, st, "set_message_kernel", recs, sorted->perm, n, d_msg.p);
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

}  // namespace upow
