// K16: vanity address search on the GPU, a batched-affine walk over consecutive private keys (the core is
// csrc/p256_vanity.h, which also says why the walk is NOT constant-time and what it is meant for).
//
// reference: none (upow/upow_wallet/wallet.py createwallet makes one random key).
//
// MI355X design
//  * a lane owns a contiguous run of steps x 65 scalars: one fixed-base multiplication and inversion for its
//    first centre (16 mixed additions over the 16-bit window table), then per batch of 65 keys one fe_inv
//    shared by 32 pairs C + j G, C - j G and the advance to the next centre;
//  * j is wave-uniform, so j G is a lane-uniform read of gtab16[j] (window 0 of the table is b G): 66 entries,
//    4 KiB, served from the scalar cache;
//  * the 32 prefix products of a lane's batch live in a per-launch workspace from the device pool, laid out
//    [product][16-byte half][lane]: a wave's store or load of one half is 1 KiB contiguous. A full launch has
//    131,072 lanes and a 128 MiB workspace, which the pool keeps for the life of the process (csrc/dev_pool.h);
//  * per key the nine address words are tested against the sorted ranges, first the top 64 bits against the
//    union's bounds; a hit appends its index through an atomicAdd on a 64-bit counter in global memory, which
//    keeps counting past the buffer's capacity. Plain C++ throughout;
//  * one launch is at most 131,072 lanes x 16 batches x 65 keys = 136,314,880 keys (9.7 ms on an MI355X,
//    docs/PERF.md "Vanity search"); the host loops over launches on the node stream.
// Compiled with the default (occupancy-first) machine scheduler, like p256_sign.hip. From
// -Rpass-analysis=kernel-resource-usage for gfx950 (profiles/p256_vanity/isa_resources.txt): the search kernel
// takes 180 VGPRs, no AGPRs, no scratch, 10 SGPR spills (to VGPR lanes) and runs 2 waves per SIMD, which is what
// a full launch supplies; the walk hook's kernel 183 VGPRs, no scratch, 2 waves per SIMD.
//
// The same core runs on host threads (the *_host functions below) with the byte-window table: the path for
// machines without a GPU and for the CPU tests.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dev_pool.h"
#include "native.h"
#include "p256_vanity.h"
#include "streams.h"
#include "thread_pool.h"

namespace upow {

static constexpr int kVanLanesPerBlock = 256;
static constexpr int64_t kVanLaunchLanes = 131072;  // 512 blocks: two waves per SIMD on 256 CUs
static constexpr int64_t kVanLaunchKeys = kVanLaunchLanes * kVanSteps * kVanBatch;
static constexpr int64_t kVanWalkMax = int64_t(1) << 21;  // the walk hook returns 33 bytes per key
static constexpr int64_t kVanHitsMax = int64_t(1) << 24;

// a 32-byte big-endian integer at a 16-byte aligned device address
__device__ __forceinline__ fe van_load_be256(const uint8_t* p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    return fe{{__builtin_bswap32(b.w), __builtin_bswap32(b.z), __builtin_bswap32(b.y), __builtin_bswap32(b.x),
               __builtin_bswap32(a.w), __builtin_bswap32(a.z), __builtin_bswap32(a.y), __builtin_bswap32(a.x)}};
}

// a lane's prefix products in the launch's workspace: product j, half h at p[(2 j + h) stride]
struct VanDevWs {
    uint4* p;
    size_t stride;
    __device__ __forceinline__ void put(int j, const fe& a) const {
        p[size_t(2 * j) * stride] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
        p[size_t(2 * j + 1) * stride] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
    }
    __device__ __forceinline__ fe get(int j) const {
        const uint4 a = p[size_t(2 * j) * stride], b = p[size_t(2 * j + 1) * stride];
        return fe{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
    }
};

// ctl: the 64-bit hit counter, then the failure word; hits: the indexes of the first `cap` hits in no order
struct VanSearchSink {
    const uint32_t* rg;
    int nr;
    unsigned long long* counter;
    uint64_t* hits;
    uint64_t cap;
    int64_t index0;
    __device__ __forceinline__ void operator()(int64_t i, const fe& x, uint32_t parity) const {
        uint32_t w[9];
        van_words(x, parity, w);
        if (!van_match(w, rg, nr)) return;
        const unsigned long long slot = atomicAdd(counter, 1ull);
        if (slot < cap) hits[slot] = uint64_t(index0 + i);
    }
};
struct VanWalkSink {
    uint8_t* out;
    int64_t index0;
    __device__ __forceinline__ void operator()(int64_t i, const fe& x, uint32_t parity) const {
        uint8_t* o = out + 33 * (index0 + i);
        o[0] = uint8_t(42u + parity);
#pragma unroll
        for (int k = 0; k < 32; ++k) o[1 + k] = uint8_t(fe_byte(x, k));
    }
};

// lane t walks the keys [t run, t run + run) of this launch's `count`, run = steps x 65; `in` holds the call's
// base scalar (32 bytes big-endian), index0 this launch's first key
template <class Sink>
__global__ __launch_bounds__(kVanLanesPerBlock) void p256_vanity_kernel(const uint8_t* __restrict__ in, int64_t index0,
                                                                        int64_t count, int steps,
                                                                        const aff* __restrict__ gtab16,
                                                                        uint4* __restrict__ ws, Sink sink,
                                                                        uint32_t* __restrict__ fail) {
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t run = int64_t(steps) * kVanBatch, start = t * run;
    if (start >= count) return;
    const int64_t len = count - start < run ? count - start : run;
    const fe base = fe_add_u64(van_load_be256(in), uint64_t(index0));
    const VanDevWs w{ws + t, size_t(gridDim.x) * blockDim.x};
    if (!van_walk_run(MulG16{gtab16}, gtab16, base, start, len, w, sink)) *fail = 1u;
}

// ------------------------------------------------------------------------------------------------
// arguments
// ------------------------------------------------------------------------------------------------
static void check_scalars(const uint8_t base_be[32], int64_t count) {
    if (count < 0) throw std::invalid_argument("count must not be negative");
    const fe b = fe_from_be(base_be), n = fe_const_n();
    if (fe_is_zero(b) || fe_geq(b, n)) throw std::invalid_argument("base must be in [1, n - 1]");
    fe room;  // n - base >= 1: how many scalars from base on are below n
    raw_sub(room, n, b);
    bool wide = false;
    for (int i = 2; i < 8; ++i) wide = wide || room.v[i] != 0;
    if (!wide && uint64_t(count) > ((uint64_t(room.v[1]) << 32) | room.v[0]))
        throw std::invalid_argument("base + count must not exceed n");
}

// R x (lo | hi), 33 bytes big-endian each -> R x (lo[9] | hi[9]) words, word 0 most significant
static std::vector<uint32_t> range_words(const uint8_t* ranges66, int64_t nr) {
    if (nr < 1 || nr > kVanMaxRanges)
        throw std::invalid_argument("need between 1 and " + std::to_string(kVanMaxRanges) + " ranges");
    std::vector<uint32_t> w(size_t(nr) * kVanRangeWords);
    for (int64_t r = 0; r < nr; ++r) {
        const uint8_t* lo = ranges66 + 66 * r;
        if (std::memcmp(lo, lo + 33, 33) >= 0) throw std::invalid_argument("range " + std::to_string(r) + " is empty");
        if (r && std::memcmp(lo - 33, lo, 33) > 0)
            throw std::invalid_argument("ranges must be sorted and disjoint");
        for (int e = 0; e < 2; ++e) {
            const uint8_t* p = lo + 33 * e;
            uint32_t* o = &w[size_t(r) * kVanRangeWords + 9 * e];
            o[0] = p[0];
            for (int k = 0; k < 8; ++k)
                o[1 + k] = (uint32_t(p[1 + 4 * k]) << 24) | (uint32_t(p[2 + 4 * k]) << 16) | (uint32_t(p[3 + 4 * k]) << 8) |
                           p[4 + 4 * k];
        }
    }
    return w;
}

// the next launch of a call with `remaining` keys to go: its keys, batches per lane and lanes
struct VanLaunch {
    int64_t keys, lanes;
    int steps;
};
static VanLaunch plan_launch(int64_t remaining, int64_t launch_keys, int64_t launch_lanes) {
    VanLaunch l;
    l.keys = std::min(remaining, launch_keys);
    const int64_t per_step = launch_lanes * kVanBatch;
    l.steps = int(std::max<int64_t>(1, (l.keys + per_step - 1) / per_step));
    const int64_t run = int64_t(l.steps) * kVanBatch;
    l.lanes = (l.keys + run - 1) / run;
    return l;
}
// test levers: 0 means the default, anything else is clamped to it
static void launch_limits(int64_t& launch_keys, int64_t& launch_lanes) {
    if (launch_keys < 0 || launch_lanes < 0) throw std::invalid_argument("launch limits must not be negative");
    launch_lanes = launch_lanes ? std::min(launch_lanes, kVanLaunchLanes) : kVanLaunchLanes;
    launch_keys = launch_keys ? std::min(launch_keys, kVanLaunchKeys) : kVanLaunchKeys;
    // a launch of launch_keys on launch_lanes must stay within kVanSteps batches per lane
    launch_keys = std::min(launch_keys, launch_lanes * kVanSteps * kVanBatch);
}

VanityInfo p256_vanity_info() {
    return VanityInfo{kVanBatch, kVanLanesPerBlock, kVanMaxRanges, kVanLaunchKeys};
}

// ------------------------------------------------------------------------------------------------
// GPU
// ------------------------------------------------------------------------------------------------
// Every launch of one call, queued on the node stream: `make_sink(index0)` gives the launch's sink.
template <class Sink, class MakeSink>
static void run_launches(const uint8_t* d_in, int64_t count, int64_t launch_keys, int64_t launch_lanes,
                         const MakeSink& make_sink, uint32_t* d_fail) {
    const aff* d_tab = static_cast<const aff*>(p256_g16_table_device());
    // No launch has more lanes than launch_lanes (plan_launch gives it the batches per lane that fit its keys on
    // that many) nor more than one per batch of the call. A later launch with fewer keys can have MORE lanes than
    // the first (fewer batches per lane), so the first launch's lane count is no bound.
    const int64_t max_lanes = std::min(launch_lanes, (count + kVanBatch - 1) / kVanBatch);
    const int64_t max_blocks = (max_lanes + kVanLanesPerBlock - 1) / kVanLanesPerBlock;
    PooledBuf<uint4> b_ws{size_t(max_blocks) * kVanLanesPerBlock * kVanHalf * 2};
    for (int64_t done = 0; done < count;) {
        const VanLaunch l = plan_launch(count - done, launch_keys, launch_lanes);
        const int64_t blocks = (l.lanes + kVanLanesPerBlock - 1) / kVanLanesPerBlock;
        if (blocks > max_blocks || l.steps > kVanSteps) throw std::logic_error("vanity launch plan exceeds its workspace");
        hipLaunchKernelGGL(p256_vanity_kernel<Sink>, dim3(unsigned(blocks)), dim3(kVanLanesPerBlock), 0, node_stream(),
                           d_in, done, l.keys, l.steps, d_tab, b_ws.p, make_sink(done), d_fail);
        launch_check("p256_vanity_kernel");
        done += l.keys;
    }
    node_sync("p256 vanity");  // before the workspace goes back to the pool
}

static VanityHits search_gpu(const uint8_t base_be[32], int64_t count, const std::vector<uint32_t>& rg, int64_t max_hits,
                             int64_t launch_keys, int64_t launch_lanes) {
    node_device_enter();
    const size_t rg_bytes = rg.size() * 4, in_bytes = 32 + rg_bytes, ctl_bytes = 16 + 8 * size_t(max_hits);
    PooledBuf<uint8_t> b_in{in_bytes}, b_ctl{ctl_bytes};
    StagedIO io(in_bytes + 16);
    uint8_t* at = io.h2d_take(in_bytes);
    SecretScrub scrub{b_in.p, at, 32};
    std::memcpy(at, base_be, 32);
    std::memcpy(at + 32, rg.data(), rg_bytes);
    io.h2d_issue(b_in.p, at, in_bytes);
    node_memset(b_ctl.p, 0, 16, "vanity counters");
    auto* d_counter = reinterpret_cast<unsigned long long*>(b_ctl.p);
    auto* d_fail = reinterpret_cast<uint32_t*>(b_ctl.p + 8);
    auto* d_hits = reinterpret_cast<uint64_t*>(b_ctl.p + 16);
    const auto* d_rg = reinterpret_cast<const uint32_t*>(b_in.p + 32);
    const int nr = int(rg.size() / kVanRangeWords);
    run_launches<VanSearchSink>(b_in.p, count, launch_keys, launch_lanes, [&](int64_t index0) {
        return VanSearchSink{d_rg, nr, d_counter, d_hits, uint64_t(max_hits), index0};
    }, d_fail);
    const uint8_t* h = io.d2h_arena(b_ctl.p, 16);  // the counters first; then only as many hits as there are
    scrub.device();
    io.finish("p256 vanity search");
    uint64_t total;
    uint32_t fail;
    std::memcpy(&total, h, 8);
    std::memcpy(&fail, h + 8, 4);
    if (fail) throw std::runtime_error("vanity walk: a batch inversion met a zero factor");
    VanityHits r;
    r.total = total;
    r.indexes.resize(size_t(std::min<uint64_t>(total, uint64_t(max_hits))));
    node_d2h(r.indexes.data(), d_hits, 8 * r.indexes.size(), "vanity hits");
    return r;
}

static std::vector<uint8_t> walk_gpu(const uint8_t base_be[32], int64_t count, int64_t launch_keys, int64_t launch_lanes) {
    node_device_enter();
    const size_t out_bytes = 33 * size_t(count);
    PooledBuf<uint8_t> b_in{32}, b_out{out_bytes}, b_fail{16};
    StagedIO io(32 + out_bytes + 16);
    uint8_t* at = io.h2d_take(32);
    SecretScrub scrub{b_in.p, at, 32};
    std::memcpy(at, base_be, 32);
    io.h2d_issue(b_in.p, at, 32);
    node_memset(b_fail.p, 0, 16, "vanity failure word");
    run_launches<VanWalkSink>(b_in.p, count, launch_keys, launch_lanes, [&](int64_t index0) {
        return VanWalkSink{b_out.p, index0};
    }, reinterpret_cast<uint32_t*>(b_fail.p));
    const uint8_t* h = io.d2h_arena(b_out.p, out_bytes);
    const uint8_t* hf = io.d2h_arena(b_fail.p, 16);
    scrub.device();
    io.finish("p256 vanity walk");
    uint32_t fail;
    std::memcpy(&fail, hf, 4);
    if (fail) throw std::runtime_error("vanity walk: a batch inversion met a zero factor");
    return std::vector<uint8_t>(h, h + out_bytes);
}

// ------------------------------------------------------------------------------------------------
// the same core on host threads: one run of up to kVanSteps batches per work item
// ------------------------------------------------------------------------------------------------
struct VanHostSearchSink {
    const uint32_t* rg;
    int nr;
    std::atomic<uint64_t>* counter;
    uint64_t* hits;
    uint64_t cap;
    void operator()(int64_t i, const fe& x, uint32_t parity) const {
        uint32_t w[9];
        van_words(x, parity, w);
        if (!van_match(w, rg, nr)) return;
        const uint64_t slot = counter->fetch_add(1, std::memory_order_relaxed);
        if (slot < cap) hits[slot] = uint64_t(i);
    }
};
struct VanHostWalkSink {
    uint8_t* out;
    void operator()(int64_t i, const fe& x, uint32_t parity) const {
        uint8_t* o = out + 33 * i;
        o[0] = uint8_t(42u + parity);
        fe_to_le(x, o + 1);
    }
};

template <class Sink>
static void walk_host(const uint8_t base_be[32], int64_t count, int threads, const Sink& sink) {
    const aff* tab = static_cast<const aff*>(p256_g_table_host());  // window 0: tab[b] = b G
    const MulG8 mulg{tab};
    const fe base = fe_from_be(base_be);
    // Batches per work item: as many as leave every thread about eight items, so that a short search still runs
    // on all of them (HostPool::parallel_for runs fewer than 64 items on the calling thread alone, so a call below
    // 64 batches = 4,160 keys is serial whatever `threads` says); kVanSteps at most, as on the device.
    const int64_t batches = (count + kVanBatch - 1) / kVanBatch;
    const int64_t want_items = std::max<int64_t>(64, int64_t(std::max(threads, 1)) * 8);
    const int64_t run = std::clamp<int64_t>(batches / want_items, 1, kVanSteps) * kVanBatch;
    std::atomic<bool> fail{false};
    HostPool::get().parallel_for((count + run - 1) / run, threads, [&](int64_t t) {
        VanHostWs ws;
        Sink s = sink;
        if (!van_walk_run(mulg, tab, base, t * run, std::min(run, count - t * run), ws, s)) fail.store(true);
    });
    if (fail.load()) throw std::runtime_error("vanity walk: a batch inversion met a zero factor");
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
VanityHits p256_vanity_search(const uint8_t base_be[32], int64_t count, const uint8_t* ranges66, int64_t n_ranges,
                              int64_t max_hits, bool gpu, int threads, int64_t launch_keys, int64_t launch_lanes) {
    check_scalars(base_be, count);
    const std::vector<uint32_t> rg = range_words(ranges66, n_ranges);
    if (max_hits < 0 || max_hits > kVanHitsMax) throw std::invalid_argument("max_hits must be in [0, 2^24]");
    launch_limits(launch_keys, launch_lanes);
    VanityHits r;
    if (count == 0) return r;
    if (gpu) {
        r = search_gpu(base_be, count, rg, max_hits, launch_keys, launch_lanes);
    } else {
        std::atomic<uint64_t> counter{0};
        std::vector<uint64_t> hits(size_t(std::min<int64_t>(max_hits, count)));
        walk_host(base_be, count, threads,
                  VanHostSearchSink{rg.data(), int(n_ranges), &counter, hits.data(), uint64_t(hits.size())});
        r.total = counter.load();
        hits.resize(size_t(std::min<uint64_t>(r.total, hits.size())));
        r.indexes = std::move(hits);
    }
    std::sort(r.indexes.begin(), r.indexes.end());
    return r;
}

std::vector<uint8_t> p256_vanity_walk(const uint8_t base_be[32], int64_t count, bool gpu, int threads,
                                      int64_t launch_keys, int64_t launch_lanes) {
    check_scalars(base_be, count);
    if (count > kVanWalkMax) throw std::invalid_argument("the walk hook returns at most 2^21 keys");
    launch_limits(launch_keys, launch_lanes);
    if (count == 0) return {};
    if (gpu) return walk_gpu(base_be, count, launch_keys, launch_lanes);
    std::vector<uint8_t> out(33 * size_t(count));
    walk_host(base_be, count, threads, VanHostWalkSink{out.data()});
    return out;
}

}  // namespace upow
