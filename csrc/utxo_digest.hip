// State digest: LtHash16/1024 of the live entries of the HBM UTXO table (utxo_table.hip), or of host-supplied
// records, in one pass. The definition is in native.h; csrc/utxo_digest_host.cpp is the same on the host.
#include <hip/hip_runtime.h>

#include <string>

#include "sha256_dev.h"
#include "utxo_dev.h"

namespace upow {

constexpr uint32_t DG_LANES = 1024;  // 64 SHA-256 digests of 16 big-endian u16 each
// what a pass hands back: DG_STRIPES lines of {u32 lane sums[1024], u64 entries, pad}. A block adds into the
// stripe its number names and the host sums the stripes (all modulo 2^32: the low 16 bits are the lane).
constexpr uint32_t DG_STRIPES = 8, DG_STRIPE_WORDS = DG_LANES + 4;
constexpr uint32_t DG_MAX_GRID = 65536;

// The element sources of utxo_digest_kernel: size() elements, of which the live() ones are digested; key() gives
// the txid as the table's eight little-endian words, the index and the tag, payload() the 80-byte payload or null.
struct DigestTableSource {  // the slots of a table; tags outside tag_mask (or above 31) are skipped
    const UtxoSlot* tab;
    const UtxoPayload* pay;
    uint32_t cap, tag_mask;
    __device__ __forceinline__ uint64_t size() const { return cap; }
    __device__ __forceinline__ bool live(uint32_t s) const {
        const uint32_t m = tab[s].meta, tag = meta_tag(m);
        return meta_state(m) == ST_FULL && tag < 32u && ((tag_mask >> tag) & 1u);
    }
    __device__ __forceinline__ void key(uint32_t s, uint32_t k[8], uint32_t& idx, uint32_t& tag) const {
        const uint4* p = reinterpret_cast<const uint4*>(tab + s);
        const uint4 a = p[0], b = p[1];
        k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w, k[4] = b.x, k[5] = b.y, k[6] = b.z, k[7] = b.w;
        const uint32_t m = tab[s].meta;
        idx = meta_index(m);
        tag = meta_tag(m);
    }
    __device__ __forceinline__ const UtxoPayload* payload(uint32_t s) const { return pay + s; }
};
struct DigestRecordSource {  // n uploaded key records, each live; pay may be null
    const UtxoKeyRec* recs;
    const UtxoPayload* pay;
    uint32_t n;
    __device__ __forceinline__ uint64_t size() const { return n; }
    __device__ __forceinline__ bool live(uint32_t) const { return true; }
    __device__ __forceinline__ void key(uint32_t i, uint32_t k[8], uint32_t& idx, uint32_t& tag) const {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(recs + i);  // 40-byte records: 4-byte aligned words
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = w[j];
        idx = w[8] & 0xffu;
        tag = w[9] & 0xffu;
    }
    __device__ __forceinline__ const UtxoPayload* payload(uint32_t i) const { return pay ? pay + i : nullptr; }
};

__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return __builtin_bswap32(x); }

// One wave digests up to 64 elements, lane l the element `e` (valid lanes only; the others add zeros), into the
// wave's accumulators acc[1024]. E's first 64 bytes do not depend on c: for L = 33 / 64 they are compressed once
// and each c restarts from that state with the second block `t` (c at byte 13 / 44 of it); for L = 0 the message
// is the single block `t` from the IV (c at byte 44). The first-block compression runs in every lane, so that the
// wave stays uniform, and an L = 0 lane drops its result: 65 compressions of issue per queued entry either way, of
// which such an entry's digest uses 64. Per c the lane's eight digest words are its 16 lane values
// (high half, then the word itself: only the low 16 bits of a sum count), summed across the wave by a
// reduce-scatter: four exchange steps halve the values a lane carries (xor 32, 16, 8, 4: 8 + 4 + 2 + 1 shuffles),
// two butterfly steps finish the sum of value k = lane / 4, which the group's first lane adds to acc[16 c + k].
template <class Src>
__device__ __forceinline__ void digest_batch(const Src& src, uint32_t e, bool valid, uint32_t lane, uint32_t* acc) {
    uint32_t k[8], idx, tag;
    src.key(e, k, idx, tag);
    const UtxoPayload* pp = src.payload(e);
    uint32_t a[16];  // the address as little-endian words
    uint32_t amount_lo = 0, amount_hi = 0, flags = 0, len = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = 0;
    if (pp) {
        const uint4* q = reinterpret_cast<const uint4*>(pp);
        const uint4 h = q[0];
        if (h.z == 33u || h.z == 64u) {
            amount_lo = h.x, amount_hi = h.y, len = h.z, flags = h.w & PAY_STAKE;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint4 v = q[1 + j];
                a[4 * j] = v.x, a[4 * j + 1] = v.y, a[4 * j + 2] = v.z, a[4 * j + 3] = v.w;
            }
        }
    }
    const bool l33 = len == 33u, l0 = len == 0u;
    uint32_t w[16], t[16], mid[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = bswap32(k[j]);
    w[8] = (idx << 24) | (tag << 16) | (flags << 8) | len;
    w[9] = bswap32(amount_lo);
    w[10] = bswap32(amount_hi);
#pragma unroll
    for (int j = 0; j < 5; ++j) w[11 + j] = bswap32(a[j]);
    // the block that carries c: the second one, or for L = 0 the only one (its words 0..10 are the first block's)
#pragma unroll
    for (int j = 0; j < 11; ++j) t[j] = l0 ? w[j] : (l33 && j > 3 ? 0u : bswap32(a[5 + j]));
    if (l33) t[3] = (t[3] & 0xff000000u) | 0x00008000u;  // addr[32], c, 0x80
    t[11] = l33 ? 0u : 0x00800000u;                       // c, 0x80
    t[12] = t[13] = t[14] = 0u;
    t[15] = l0 ? 45u * 8u : (l33 ? 78u * 8u : 109u * 8u);
    const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                            0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
#pragma unroll
    for (int j = 0; j < 8; ++j) mid[j] = iv[j];
    dev_compress(mid, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) mid[j] = l0 ? iv[j] : mid[j];
    const uint32_t c3 = l33 ? 16u : 32u, c11 = l33 ? 32u : 24u;  // c's shift in t[3] / t[11]; 32: not there
#pragma unroll 1
    for (uint32_t c = 0; c < 64u; ++c) {
        uint32_t st[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) st[j] = mid[j];
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = t[j];
        w[3] |= c3 < 32u ? c << c3 : 0u;
        w[11] |= c11 < 32u ? c << c11 : 0u;
        dev_compress(st, w);
        uint32_t v[16];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[2 * j] = valid ? st[j] >> 16 : 0u;
            v[2 * j + 1] = valid ? st[j] : 0u;
        }
#pragma unroll
        for (int half = 8, bit = 32; half >= 1; half >>= 1, bit >>= 1) {
            const bool up = (lane & uint32_t(bit)) != 0;
#pragma unroll
            for (int j = 0; j < half; ++j) {
                const uint32_t keep = up ? v[half + j] : v[j], send = up ? v[j] : v[half + j];
                v[j] = keep + __shfl_xor(send, bit, 64);
            }
        }
        uint32_t s = v[0];
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        if ((lane & 3u) == 0u) acc[16u * c + (lane >> 2)] += s;
    }
}

// A wave walks its share of the source's elements in a grid-stride loop, 64 at a time, and queues the numbers of
// the live ones in LDS (ballot + popcount: a table is at most half full, and a lane that hashed "its" slot would
// idle most of the wave for 64 compressions). Whenever 64 are queued the wave digests them with every lane busy;
// what is left after the walk is one partial batch. The wave's 1024 u32 accumulators stay in LDS for the whole
// walk; at the end the block's four waves are summed and added to the block's stripe with one atomic per lane
// value. An accumulator is only ever updated by one lane (lane 4k of its wave for value k); the zeroing before and
// the block's sum after are set apart by the two barriers, which every lane reaches: the walk's trip count depends
// on the source's size alone. The queue is written and read across the lanes of one wave only, in program order:
// the wave's DS operations complete in order, the accesses are volatile, and a wave barrier (a scheduling fence for
// the compiler, no instruction) stands at each of the three hand-overs. No lane waits for another block.
template <class Src>
__global__ __launch_bounds__(256) void utxo_digest_kernel(const Src src, uint32_t* __restrict__ stripes) {
    __shared__ uint32_t acc_s[4][DG_LANES];
    __shared__ volatile uint32_t queue_s[4][128];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t j = 0; j < DG_LANES / 64u; ++j) acc_s[j >> 2][threadIdx.x + 256u * (j & 3u)] = 0u;
    __syncthreads();
    const uint64_t n = src.size(), stride = uint64_t(gridDim.x) * 256u;
    uint32_t queued = 0;     // wave-uniform, below 64 between iterations
    uint64_t digested = 0;   // wave-uniform
    for (uint64_t base = (uint64_t(blockIdx.x) * 4u + wave) * 64u;; base += stride) {
        const bool more = base < n;  // wave-uniform
        if (more) {
            const uint64_t i = base + lane;
            const bool live = i < n && src.live(uint32_t(i));
            const unsigned long long peers = __ballot(live);
            if (live) queue_s[wave][queued + uint32_t(__popcll(peers & ((1ull << lane) - 1ull)))] = uint32_t(i);
            queued += uint32_t(__popcll(peers));  // at most 127
            __builtin_amdgcn_wave_barrier();      // the lanes' writes stay ahead of the reads below
        }
        if (queued >= 64u || (!more && queued)) {
            const uint32_t take = queued < 64u ? queued : 64u;
            const bool valid = lane < take;
            digest_batch(src, queue_s[wave][valid ? lane : 0u], valid, lane, acc_s[wave]);
            queued -= take;
            digested += take;
            __builtin_amdgcn_wave_barrier();  // the batch is read before the queue's front is overwritten
            if (lane < queued) {
                const uint32_t next = queue_s[wave][64u + lane];
                queue_s[wave][lane] = next;
            }
            __builtin_amdgcn_wave_barrier();  // and moved before the next walk step appends
        }
        if (!more) break;
    }
    __syncthreads();
    uint32_t* out = stripes + size_t(blockIdx.x & (DG_STRIPES - 1u)) * DG_STRIPE_WORDS;
#pragma unroll
    for (uint32_t j = 0; j < DG_LANES / 256u; ++j) {
        const uint32_t x = threadIdx.x + 256u * j;
        const uint32_t s = acc_s[0][x] + acc_s[1][x] + acc_s[2][x] + acc_s[3][x];
        if (s) atomicAdd(&out[x], s);
    }
    if (lane == 0 && digested)
        atomicAdd(reinterpret_cast<unsigned long long*>(out + DG_LANES), static_cast<unsigned long long>(digested));
}

// the stripes summed into the serialised state (synchronises the node stream: the scratch may go back to the pool)
static void digest_collect(const uint32_t* d_stripes, StateDigestOut& out) {
    std::vector<uint32_t> stripes(size_t(DG_STRIPES) * DG_STRIPE_WORDS);
    node_d2h(stripes.data(), d_stripes, sizeof(uint32_t) * stripes.size(), "d2h digest stripes");
    out.count = 0;
    for (uint32_t x = 0; x < DG_LANES; ++x) {
        uint32_t s = 0;
        for (uint32_t i = 0; i < DG_STRIPES; ++i) s += stripes[size_t(i) * DG_STRIPE_WORDS + x];
        out.state[2 * x] = uint8_t(s);
        out.state[2 * x + 1] = uint8_t(s >> 8);
    }
    for (uint32_t i = 0; i < DG_STRIPES; ++i) {
        uint64_t c;
        std::memcpy(&c, &stripes[size_t(i) * DG_STRIPE_WORDS + DG_LANES], sizeof c);
        out.count += c;
    }
}

// blocks of a pass over n elements: every element gets a lane, up to three blocks per compute unit (what the
// kernel's ~150 VGPRs keep resident, so the waves' equal shares of the walk all run at once)
static uint32_t digest_grid(uint64_t n, uint32_t grid_blocks) {
    if (grid_blocks > DG_MAX_GRID) throw std::invalid_argument("grid_blocks is at most 65536 (0: the default grid)");
    if (grid_blocks) return grid_blocks;
    int dev = 0, cus = 0;
    stream_check(hipGetDevice(&dev), "hipGetDevice");
    stream_check(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "compute unit count");
    const uint64_t want = (n + 255u) / 256u, most = 3u * uint64_t(cus > 0 ? cus : 1);
    return uint32_t(std::max<uint64_t>(1, std::min(want, most)));
}

template <class Src>
static void digest_run(const Src& src, uint64_t n, uint32_t grid_blocks, StateDigestOut& out) {
    const uint32_t blocks = digest_grid(n, grid_blocks);
    PooledBuf<uint32_t> stripes(size_t(DG_STRIPES) * DG_STRIPE_WORDS);
    node_memset(stripes.p, 0, sizeof(uint32_t) * DG_STRIPES * DG_STRIPE_WORDS, "memset digest stripes");
    launch(utxo_digest_kernel<Src>, int64_t(blocks) * 256, node_stream(), "utxo_digest_kernel", src, stripes.p);
    digest_collect(stripes.p, out);
}

void utxo_state_digest(int64_t h, uint32_t tag_mask, uint32_t grid_blocks, StateDigestOut& out) {
    std::lock_guard<std::mutex> lk(g_ut_mu);  // one hold: the pass runs behind any queued async apply
    UtxoTableDev& t = table(h);
    digest_run(DigestTableSource{t.tab, t.pay, t.cap, tag_mask}, t.cap, grid_blocks, out);
}

void utxo_records_digest(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t grid_blocks,
                         StateDigestOut& out) {
    if (n < 0 || n > int64_t(0x7fffffff)) throw std::invalid_argument("record count must be in [0, 2^31)");
    std::memset(out.state, 0, sizeof out.state);
    out.count = 0;
    if (grid_blocks > DG_MAX_GRID) throw std::invalid_argument("grid_blocks is at most 65536 (0: the default grid)");
    if (n == 0) return;
    node_device_enter();
    PooledBuf<UtxoKeyRec> d(n);
    PooledBuf<UtxoPayload> dp(pay_or_null ? n : 0);
    node_h2d(d.p, recs, sizeof(UtxoKeyRec) * size_t(n), "h2d recs");
    if (pay_or_null) node_h2d(dp.p, pay_or_null, sizeof(UtxoPayload) * size_t(n), "h2d payload");
    digest_run(DigestRecordSource{d.p, pay_or_null ? dp.p : nullptr, uint32_t(n)}, uint64_t(n), grid_blocks, out);
}

}  // namespace upow
