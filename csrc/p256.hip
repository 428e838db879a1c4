// K5: P-256 ECDSA batch verify (the verify TU: the host verifiers, the lane-group kernel, the key kernel of the
// fused block path and the launch logic; the tables are csrc/p256_tables.hip, decompression and on-curve
// csrc/p256_keys.hip, signing csrc/p256_sign.hip).
//
// reference: fastecdsa ecdsa.verify, called one signature at a time from
// upow/upow_transactions/transaction_input.py:84-120 and upow/upow_transactions/transaction.py:484-497.
//
// GPU design (gfx950): batches up to 32k signatures (a block) take four lanes per signature (the quad
// kernel, see "four lanes per signature" in csrc/p256_steps.h); larger batches one signature per lane:
//  * u1*G uses a fixed-base byte-window table T[j][b] = b*256^j*G (32 x 255 affine points, 522 KB,
//    L2/Infinity-Cache resident) -> 32 mixed additions and no doublings;
//  * u2*Q uses signed 5-bit windows (BoothW5) over a per-signature table {1..16}Q kept in global
//    scratch (1.5-2 KB per signature does not fit LDS at useful occupancy) -> 255 doublings + 52
//    additions (unsigned 4-bit windows: 252 + 64);
//  * no field inversion: x(R) == r is tested as X == r*Z^2 (and (r+n)*Z^2 when r+n < p);
//  * s^-1 mod n by Bernstein-Yang divsteps (p256_field.h sc_inv_safegcd_mont: 20 rounds of 30, no
//    divergence; the binary extended Euclid it replaced, sc_inv_bgcd_mont, stays for the A/B build);
//  * status per item: 1 valid, 0 invalid, 2 public key not on curve, 3 r/s out of [1, n]
//    (fastecdsa raises for 2/3; the Python layer turns them into EcdsaError).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <optional>
#include <thread>
#include <type_traits>
#include <vector>

#include "dev_pool.h"
#include "native.h"
#include "streams.h"
#include "p256_field.h"
#include "p256_steps.h"
#include "p256_verify.h"

namespace upow {
using namespace p256;

void p256_scalar_inv_mont_host(uint64_t out[4], const uint64_t s[4]) {
    fe a;
    std::memcpy(a.v, s, 32);
    const fe r = sc_inv_safegcd_mont(a);
    std::memcpy(out, r.v, 32);
}

// ------------------------------------------------------------------------------------------------
// shared verify core
// ------------------------------------------------------------------------------------------------

static uint8_t verify_one_host(const VerifyItem& it, const aff* gtab) {
    aff q;
    fe r, u1, u2;
    const uint8_t pro = verify_prologue(it, q, r, u1, u2);
    if (pro != 255) return pro;
    jac tbl[17];  // k*Q, k = 1..16 (signed 5-bit windows)
    tbl[0] = jac_inf();
    tbl[1] = jac_from_aff(q);
    for (int k = 2; k <= 16; ++k) tbl[k] = jac_madd(tbl[k - 1], q);
    jac acc = jac_inf();
    BoothW5 bw(u2);
    for (int w = kBoothWindows - 1; w >= 0; --w) {
        if (!jac_is_inf(acc))
            for (int k = 0; k < 5; ++k) acc = jac_dbl(acc);
        const int d = bw.next();
        if (d) {
            jac e = tbl[d < 0 ? -d : d];
            if (d < 0) e.y = fe_neg(e.y);
            acc = jac_add(acc, e);
        }
    }
    const jac R = jac_add(mul_g(u1, gtab), acc);
    return verify_epilogue(R, r);
}

// the lane-group step schedule (csrc/p256_steps.h) played by one host thread under the host policy P
template <class P>
static uint8_t verify_one_host_steps(const VerifyItem& it, const aff* gtab) {
    aff q;
    fe r, u1, u2;
    const uint8_t pro = verify_prologue(it, q, r, u1, u2);
    if (pro != 255) return pro;
    xz tab[16];
    return verify_quad_core(P{}, q, r, u2, tab, [&](auto K) { return jac_to_xz(mul_g_quarter(u1, gtab, K)); });
}
static uint8_t verify_one_host_quad(const VerifyItem& it, const aff* gtab) { return verify_one_host_steps<QuadHost>(it, gtab); }

// ------------------------------------------------------------------------------------------------
// device kernels
// ------------------------------------------------------------------------------------------------

// G::kLanes lanes per signature (G = QuadDev: four, 16 signatures per wave; OctDev: eight, 8 per wave), four
// waves per workgroup. Exits are group-uniform. With OctDev both quads of an octet hold the same point state;
// the u1*G quarters are computed by each quad (lane & 3) and broadcast within it.
static constexpr int64_t kQuadMaxBatch = 32 * 1024;  // 2,048 waves of 16 signatures: two per SIMD
static constexpr int64_t kBatchSlice = 4 * 1024 * 1024;  // one-lane batch launches: signatures per launch
template <class G>
__global__ __launch_bounds__(256, 1) void p256_verify_group_kernel(const VerifyItem* __restrict__ items, int64_t n,
                                                                    const aff* __restrict__ gtab16,
                                                                    xz* __restrict__ scratch,
                                                                    uint8_t* __restrict__ status) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t i = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * (64 / G::kLanes) + lane / G::kLanes;
    if (i >= n) return;
    const G pp = G::of_lane(lane);
    const VerifyItem it = items[i];
    aff q;
    fe r, u1, u2;
    const uint8_t pro = verify_prologue(it, q, r, u1, u2);
    if (pro != 255) {
        if (G::leader(lane)) status[i] = pro;
        return;
    }
    const xz mine = jac_to_xz(mul_g16_quarter(u1, gtab16, lane & 3));  // this lane's quarter of u1*G
    const uint8_t st = verify_quad_core(pp, q, r, u2, scratch + i * 16, [&](auto K) {
        constexpr int k = decltype(K)::value;
        return xz{fe_quad_bcast<k>(mine.x), fe_quad_bcast<k>(mine.y), fe_quad_bcast<k>(mine.zz), fe_quad_bcast<k>(mine.zzz)};
    });
    if (G::leader(lane)) status[i] = st;
}

// The key kernel of p256_verify_fused_gpu. Thread t < n_jobs: signer key jobkeys[t] decompressed into verify
// item t, whose r | s | digest come from sigdig[t]; a key off the curve (or x >= p) gets x = y = 0, which the
// verify prologue reports as a bad key (status 2), as the separate decompression's failure did. Threads
// past n_jobs: output address t - n_jobs, curve check only (transaction_output.py: string_to_point).
__global__ __launch_bounds__(256) void p256_keyrec_kernel(const uint8_t* __restrict__ jobkeys,
                                                           const uint8_t* __restrict__ sigdig, int64_t n_jobs,
                                                           const uint8_t* __restrict__ outkeys, int64_t n_out,
                                                           VerifyItem* __restrict__ items, uint8_t* __restrict__ out_ok) {
    const int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n_jobs + n_out) return;
    const bool job = t < n_jobs;
    const uint8_t* a = job ? jobkeys + 33 * t : outkeys + 33 * (t - n_jobs);
    const fe x = fe_from_le(a + 1);
    const bool odd = a[0] == 43;
    fe y;
    const bool good = curve_y(x, y);
    if (!job) {
        out_ok[t - n_jobs] = good ? 1 : 0;
        return;
    }
    if ((y.v[0] & 1u) != uint32_t(odd)) y = fe_neg(y);
    VerifyItem* it = items + t;
    fe_to_le(good ? x : fe_zero(), it->qx);
    fe_to_le(good ? y : fe_zero(), it->qy);
    const uint8_t* sd = sigdig + 96 * t;
    uint8_t* rse = reinterpret_cast<uint8_t*>(it) + 64;  // r | s | e: the item's last 96 bytes
#pragma unroll 8
    for (int k = 0; k < 96; ++k) rse[k] = sd[k];
}

// ------------------------------------------------------------------------------------------------
// host API
// ------------------------------------------------------------------------------------------------
std::vector<uint8_t> p256_verify_host(const uint8_t* items, int64_t n, int threads) {
    std::vector<uint8_t> st(static_cast<size_t>(n));
    const aff* tab = static_cast<const aff*>(p256_g_table_host());
    const VerifyItem* it = reinterpret_cast<const VerifyItem*>(items);
    // UPOW_P256_HOST32 (read per call): '1' = the 32-bit-limb single-lane code the one-lane GPU kernels
    // run; 'quad' = the four-lane step schedule of the quad kernel played by one host thread (CPU tests
    // of both GPU code paths); 'oct' = the same schedule with the eight-lane kernel's pair-split products;
    // unset = the 64-bit-limb host verifier.
    const char* h32 = std::getenv("UPOW_P256_HOST32");
    const int mode = !h32 ? 0 : (std::strcmp(h32, "quad") == 0 ? 2 : std::strcmp(h32, "oct") == 0 ? 3 : (h32[0] == '1' ? 1 : 0));
    threads = int(std::max<int64_t>(1, std::min<int64_t>(threads, n)));
    auto work = [&](int t) {
        if (mode == 1)
            for (int64_t i = t; i < n; i += threads) st[i] = verify_one_host(it[i], tab);
        else if (mode == 2)
            for (int64_t i = t; i < n; i += threads) st[i] = verify_one_host_quad(it[i], tab);
        else if (mode == 3)  // the eight-lane kernel's pair-split products
            for (int64_t i = t; i < n; i += threads) st[i] = verify_one_host_steps<OctHost>(it[i], tab);
        else
            for (int64_t i = t; i < n; i += threads)
                st[i] = p256_verify_one_host64(reinterpret_cast<const uint8_t*>(&it[i]));
    };
    if (threads <= 1) {
        work(0);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    return st;
}

// Scratch of one verify launch: kept by the caller until its stream sync.
struct VerifyScratch {
    std::optional<PooledBuf<xz>> quad;
    std::optional<PooledBuf<jac>> one;
};

// One launch of the lane-group kernel over n device items, with its window-table scratch.
template <class G>
static void launch_group(const VerifyItem* d_items, int64_t n, const aff* d_tab, uint8_t* d_st, VerifyScratch& sc) {
    sc.quad.emplace(size_t(16) * size_t(n));
    const int64_t per_wave = 64 / G::kLanes, waves = (n + per_wave - 1) / per_wave;
    hipLaunchKernelGGL(p256_verify_group_kernel<G>, dim3(unsigned((waves + 3) / 4)), dim3(256), 0, node_stream(), d_items,
                       n, d_tab, sc.quad->p, d_st);
    launch_check("p256_verify_group_kernel");
}

// Launches the verify of n device items into d_st on the node stream.
// Variant (UPOW_P256_VARIANT, read per call): unset/'a' = auto, '4' = four lanes per signature,
// '8' = eight, '0'..'3' = one lane per signature (below). Auto takes the quad kernel up to 32k signatures
// (2,048 waves, two per SIMD): there it cuts the latency of block-sized batches; past that the chip is
// full either way and one lane per signature does half the total work.
static void verify_launch(const VerifyItem* d_items, int64_t n, const aff* d_tab, uint8_t* d_st, VerifyScratch& sc) {
    const char* var = std::getenv("UPOW_P256_VARIANT");
    char v = var && var[0] ? var[0] : 'a';
    const bool autov = v == 'a';
    if (v == 'a') v = n <= kQuadMaxBatch ? '4' : '1';
    if (v == '8') return launch_group<OctDev>(d_items, n, d_tab, d_st, sc);
    if (v == '4') return launch_group<QuadDev>(d_items, n, d_tab, d_st, sc);
    const char* spw_env = std::getenv("UPOW_P256_SPW");
    int spw = spw_env ? std::atoi(spw_env) : 64;
    if (spw < 1 || spw > 64) spw = 64;
    // one lane per signature (csrc/p256_batch.hip), one launch per kBatchSlice signatures (UPOW_P256_SLICE
    // for the A/B): slicing a 531,200-signature batch into 128 k or 256 k launches measured 12 % / 9 % slower
    // than one launch (each launch ends in a tail of half-idle SIMDs; profiles/r5/p256batch), so the default
    // slice only bounds the window-table scratch (16 x 96 B per signature)
    const char* sl_env = std::getenv("UPOW_P256_SLICE");
    const int64_t slice = std::max<int64_t>(1024, sl_env ? std::atoll(sl_env) : kBatchSlice);
    // Every one-lane wave runs the same fixed-window chain, so the kernel takes whole "rounds" of one wave
    // lifetime: 4 waves per SIMD x 1,024 SIMDs x 64 lanes = 262,144 signatures per round on MI355X. A batch
    // a little past a multiple of that (531,200 = 2 rounds + 6,912) paid a third round for 3 % of its work.
    // Auto mode runs the whole rounds on the one-lane kernel and a remainder of at most kQuadMaxBatch on the
    // four-lanes-per-signature kernel, which finishes it in a quarter of a wave lifetime.
    int64_t n_one = n, n_quad = 0;
    if (autov && v == '1' && spw == 64 && !sl_env && std::getenv("UPOW_P256_TAIL") == nullptr) {
        int dev = 0, cus = 0;
        stream_check(hipGetDevice(&dev), "hipGetDevice");
        stream_check(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "CU count");
        const int64_t round = int64_t(cus) * 4 /* SIMDs */ * 4 /* waves per SIMD */ * 64;
        const int64_t full = round > 0 ? (n / round) * round : 0, rem = n - full;
        if (full > 0 && rem > 0 && rem <= kQuadMaxBatch) {
            n_one = full;
            n_quad = rem;
        }
    }
    sc.one.emplace(size_t(16) * size_t(std::min(n_one, slice)));
    for (int64_t off = 0; off < n_one; off += slice)
        p256_batch_launch(v, d_items + off, std::min(slice, n_one - off), d_tab, sc.one->p, d_st + off, spw, node_stream());
    if (n_quad) launch_group<QuadDev>(d_items + n_one, n_quad, d_tab, d_st + n_one, sc);
}

std::vector<uint8_t> p256_verify_gpu(const uint8_t* items, int64_t n) {
    std::vector<uint8_t> st(static_cast<size_t>(n));
    if (n == 0) return st;
    node_device_enter();
    const aff* d_tab = static_cast<const aff*>(p256_g16_table_device());
    PooledBuf<VerifyItem> b_items{size_t(n)};
    PooledBuf<uint8_t> b_st{size_t(n)};
    StagedIO io(sizeof(VerifyItem) * size_t(n) + size_t(n));
    io.h2d(b_items.p, items, sizeof(VerifyItem) * size_t(n));
    VerifyScratch sc;
    verify_launch(b_items.p, n, d_tab, b_st.p, sc);
    io.d2h(st.data(), b_st.p, size_t(n));
    io.finish("verify status");
    return st;
}

// One block's signatures from compressed keys (csrc/txcodec.cpp block_verify_fused): `fill` packs the
// inputs straight into pinned staging -- n_jobs 33-byte signer keys, n_jobs x 96 B (r | s | digest), n_out
// 33-byte output addresses -- then ONE stream order runs the key kernel (decompression into the verify items
// on the device, the outputs' curve check) and the verify, with one sync for the statuses and the output
// flags. `items_out` receives the device's verify items only when some status is INVALID (0): the caller's
// ASCII-hex retry rebuilds those records with another digest.
void p256_verify_fused_gpu(int64_t n_jobs, int64_t n_out, const std::function<void(uint8_t*, uint8_t*, uint8_t*)>& fill,
                           uint8_t* st, uint8_t* out_ok, std::vector<uint8_t>* items_out) {
    if (n_jobs + n_out == 0) return;
    node_device_enter();
    const aff* d_tab = static_cast<const aff*>(p256_g16_table_device());
    const size_t in_bytes = 129 * size_t(n_jobs) + 33 * size_t(n_out);
    PooledBuf<uint8_t> b_in{in_bytes}, b_st{size_t(n_jobs + n_out)};
    PooledBuf<VerifyItem> b_items{size_t(n_jobs)};
    StagedIO io(in_bytes + size_t(n_jobs + n_out));
    uint8_t* at = io.h2d_take(in_bytes);
    fill(at, at + 33 * size_t(n_jobs), at + 129 * size_t(n_jobs));
    io.h2d_issue(b_in.p, at, in_bytes);
    const int64_t nt = n_jobs + n_out;
    hipLaunchKernelGGL(p256_keyrec_kernel, dim3(unsigned((nt + 255) / 256)), dim3(256), 0, node_stream(), b_in.p,
                       b_in.p + 33 * n_jobs, n_jobs, b_in.p + 129 * n_jobs, n_out, b_items.p, b_st.p + n_jobs);
    launch_check("p256_keyrec_kernel");
    VerifyScratch sc;
    if (n_jobs) verify_launch(b_items.p, n_jobs, d_tab, b_st.p, sc);
    // statuses and output flags are adjacent on the device: one D2H for both
    const uint8_t* hst = io.d2h_arena(b_st.p, size_t(n_jobs + n_out));
    io.finish("fused verify");
    std::memcpy(st, hst, size_t(n_jobs));
    std::memcpy(out_ok, hst + n_jobs, size_t(n_out));
    if (items_out && std::find(st, st + n_jobs, uint8_t(0)) != st + n_jobs) {
        items_out->resize(sizeof(VerifyItem) * size_t(n_jobs));
        node_d2h(items_out->data(), b_items.p, items_out->size(), "d2h verify items");
    }
}

}  // namespace upow
