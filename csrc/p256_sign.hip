// K15 batched: P-256 public keys and RFC 6979 signatures, one item per lane (the core is csrc/p256_sign.h,
// which also says why this signer is NOT constant-time and what it is meant for).
//
// reference: fastecdsa keys.get_public_key / ecdsa.sign, one call at a time from upow/helpers.py:58-62,135-144
// and upow/upow_transactions/transaction.py:148-180.
//
// Like p256_batch.hip this file is compiled with the default (occupancy-first) machine scheduler. An item is
// 22 SHA-256 compressions (the HMAC_DRBG), 16 mixed additions over the 16-bit window table, one field
// inversion and one divsteps inversion mod n; nothing is shared between lanes and there is no barrier, so a
// lane whose key is out of range simply retires early. The nonce lives in registers only.
//
// The same core runs on host threads (p256_*_many_host below) with the portable SHA-256 compression and the
// byte-window table: the kernels' code path for machines without a GPU and for the CPU tests.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "dev_pool.h"
#include "native.h"
#include "p256_sign.h"
#include "sha256_common.h"
#include "sha256_dev.h"
#include "streams.h"
#include "thread_pool.h"

namespace upow {

struct DevCompress {
    __device__ __forceinline__ void operator()(uint32_t st[8], uint32_t w[16]) const { dev_compress(st, w); }
};
struct HostCompress {
    void operator()(uint32_t st[8], const uint32_t w[16]) const { host_compress_words(st, w); }
};

// a 32-byte big-endian integer at a 16-byte aligned device address
__device__ __forceinline__ fe load_be256(const uint8_t* p) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
    return fe{{__builtin_bswap32(b.w), __builtin_bswap32(b.z), __builtin_bswap32(b.y), __builtin_bswap32(b.x),
               __builtin_bswap32(a.w), __builtin_bswap32(a.z), __builtin_bswap32(a.y), __builtin_bswap32(a.x)}};
}
// two little-endian 256-bit integers (x | y, r | s) to a 16-byte aligned 64-byte record
__device__ __forceinline__ void store_le512(uint8_t* p, const fe& a, const fe& b) {
    uint4* o = reinterpret_cast<uint4*>(p);
    o[0] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
    o[1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
    o[2] = make_uint4(b.v[0], b.v[1], b.v[2], b.v[3]);
    o[3] = make_uint4(b.v[4], b.v[5], b.v[6], b.v[7]);
}

__global__ __launch_bounds__(256) void p256_pubkey_kernel(const uint8_t* __restrict__ keys_be, int64_t n,
                                                           const aff* __restrict__ gtab16,
                                                           uint8_t* __restrict__ out_le, uint8_t* __restrict__ ok) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aff q;
    const bool good = pubkey_one(MulG16{gtab16}, load_be256(keys_be + 32 * i), q);
    store_le512(out_le + 64 * i, fe_select(good, q.x, fe_zero()), fe_select(good, q.y, fe_zero()));
    ok[i] = good ? 1 : 0;
}

__global__ __launch_bounds__(256) void p256_sign_kernel(const uint8_t* __restrict__ keys_be,
                                                         const uint8_t* __restrict__ digests, int64_t n,
                                                         const aff* __restrict__ gtab16,
                                                         uint8_t* __restrict__ rs_le, uint8_t* __restrict__ ok) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe r, s;
    const bool good = sign_one(DevCompress{}, MulG16{gtab16}, load_be256(keys_be + 32 * i),
                               load_be256(digests + 32 * i), r, s);
    store_le512(rs_le + 64 * i, fe_select(good, r, fe_zero()), fe_select(good, s, fe_zero()));
    ok[i] = good ? 1 : 0;
}

// test hook: the first `count` candidates of the DRBG for key_digest = key (32 B BE) | digest (32 B), each
// 32 bytes big-endian, accepted or not. One thread.
__global__ __launch_bounds__(64) void p256_candidates_kernel(const uint8_t* __restrict__ key_digest, int count,
                                                              uint32_t* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Rfc6979<DevCompress> drbg;
    drbg.init(DevCompress{}, load_be256(key_digest), sc_reduce(load_be256(key_digest + 32)));
#pragma nounroll
    for (int j = 0; j < count; ++j) {
        const fe k = drbg.next(DevCompress{});
#pragma unroll
        for (int w = 0; w < 8; ++w) out[8 * j + w] = __builtin_bswap32(k.v[7 - w]);
    }
}

// ------------------------------------------------------------------------------------------------
// host entry points (GPU)
// ------------------------------------------------------------------------------------------------
// Keys (| digests) in one H2D, one launch, x | y (r | s) and the ok flags adjacent on the device and back in
// one D2H, all on the node stream. digests == nullptr: public keys.
static void sign_or_pubkey_gpu(const uint8_t* keys_be, const uint8_t* digests, int64_t n, uint8_t* out, uint8_t* ok) {
    if (n == 0) return;
    node_device_enter();
    const aff* d_tab = static_cast<const aff*>(p256_g16_table_device());
    const size_t nk = 32 * size_t(n), in_bytes = digests ? 2 * nk : nk;
    PooledBuf<uint8_t> b_in{in_bytes}, b_out{65 * size_t(n)};
    StagedIO io(in_bytes + 65 * size_t(n));
    uint8_t* at = io.h2d_take(in_bytes);
    SecretScrub scrub{b_in.p, at, nk};
    std::memcpy(at, keys_be, nk);
    if (digests) std::memcpy(at + nk, digests, nk);
    io.h2d_issue(b_in.p, at, in_bytes);
    const dim3 grid(unsigned((n + 255) / 256)), block(256);
    uint8_t* d_ok = b_out.p + 64 * size_t(n);
    if (digests) {
        hipLaunchKernelGGL(p256_sign_kernel, grid, block, 0, node_stream(), b_in.p, b_in.p + nk, n, d_tab, b_out.p, d_ok);
        launch_check("p256_sign_kernel");
    } else {
        hipLaunchKernelGGL(p256_pubkey_kernel, grid, block, 0, node_stream(), b_in.p, n, d_tab, b_out.p, d_ok);
        launch_check("p256_pubkey_kernel");
    }
    const uint8_t* h = io.d2h_arena(b_out.p, 65 * size_t(n));
    scrub.device();
    io.finish(digests ? "p256 sign" : "p256 pubkey");
    std::memcpy(out, h, 64 * size_t(n));
    std::memcpy(ok, h + 64 * size_t(n), size_t(n));
}

void p256_pubkey_gpu(const uint8_t* keys_be, int64_t n, uint8_t* out_le, uint8_t* ok) {
    sign_or_pubkey_gpu(keys_be, nullptr, n, out_le, ok);
}

void p256_sign_gpu(const uint8_t* keys_be, const uint8_t* digests, int64_t n, uint8_t* rs_le, uint8_t* ok) {
    sign_or_pubkey_gpu(keys_be, digests, n, rs_le, ok);
}

// test hook (leaks the nonce): the candidates leave through a device buffer and pinned staging, both
// overwritten like the key's
void p256_candidates_gpu(const uint8_t key_be[32], const uint8_t digest[32], int count, uint8_t* out) {
    if (count <= 0) return;
    node_device_enter();
    const size_t nb = 32 * size_t(count);
    PooledBuf<uint8_t> b_in{64}, b_out{nb};
    StagedIO io(64 + nb);
    uint8_t* at = io.h2d_take(64);
    SecretScrub scrub_key{b_in.p, at, 32};
    std::memcpy(at, key_be, 32);
    std::memcpy(at + 32, digest, 32);
    io.h2d_issue(b_in.p, at, 64);
    hipLaunchKernelGGL(p256_candidates_kernel, dim3(1), dim3(64), 0, node_stream(), b_in.p, count,
                       reinterpret_cast<uint32_t*>(b_out.p));
    launch_check("p256_candidates_kernel");
    uint8_t* h = io.h2d_take(nb);  // pinned space for the D2H, writable so it can be cleared
    SecretScrub scrub_out{b_out.p, h, nb};
    stream_check(hipMemcpyAsync(h, b_out.p, nb, hipMemcpyDeviceToHost, node_stream()), "d2h candidates");
    scrub_key.device();
    scrub_out.device();
    io.finish("rfc6979 candidates");
    std::memcpy(out, h, nb);
}

// ------------------------------------------------------------------------------------------------
// the same core on host threads
// ------------------------------------------------------------------------------------------------
void p256_pubkey_many_host(const uint8_t* keys_be, int64_t n, uint8_t* out_le, uint8_t* ok, int threads) {
    const MulG8 mulg{static_cast<const aff*>(p256_g_table_host())};
    HostPool::get().parallel_for(n, threads, [&](int64_t i) {
        aff q;
        const bool good = pubkey_one(mulg, fe_from_be(keys_be + 32 * i), q);
        fe_to_le(good ? q.x : fe_zero(), out_le + 64 * i);
        fe_to_le(good ? q.y : fe_zero(), out_le + 64 * i + 32);
        ok[i] = good ? 1 : 0;
    });
}

void p256_sign_many_host(const uint8_t* keys_be, const uint8_t* digests, int64_t n, uint8_t* rs_le, uint8_t* ok,
                         int threads) {
    const MulG8 mulg{static_cast<const aff*>(p256_g_table_host())};
    HostPool::get().parallel_for(n, threads, [&](int64_t i) {
        fe r, s;
        const bool good = sign_one(HostCompress{}, mulg, fe_from_be(keys_be + 32 * i), fe_from_be(digests + 32 * i), r, s);
        fe_to_le(good ? r : fe_zero(), rs_le + 64 * i);
        fe_to_le(good ? s : fe_zero(), rs_le + 64 * i + 32);
        ok[i] = good ? 1 : 0;
    });
}

void p256_candidates_host(const uint8_t key_be[32], const uint8_t digest[32], int count, uint8_t* out) {
    Rfc6979<HostCompress> drbg;
    drbg.init(HostCompress{}, fe_from_be(key_be), sc_reduce(fe_from_be(digest)));
    for (int j = 0; j < count; ++j) fe_to_be(drbg.next(HostCompress{}), out + 32 * j);
}

// ------------------------------------------------------------------------------------------------
// single-signature host reference (wallets): written separately from sign_one, byte-wise, so the tests can
// compare the two
// ------------------------------------------------------------------------------------------------
bool p256_pubkey(const uint8_t d_be[32], uint8_t out_le[64]) {
    const fe d = fe_from_be(d_be);
    if (fe_is_zero(d) || fe_geq(d, fe_const_n())) return false;
    aff a;
    if (!jac_to_aff(mul_g(d, static_cast<const aff*>(p256_g_table_host())), a)) return false;
    fe_to_le(a.x, out_le);
    fe_to_le(a.y, out_le + 32);
    return true;
}

// HMAC-SHA256
static void hmac_sha256(const uint8_t* key, size_t klen, const uint8_t* msg, size_t mlen, uint8_t out[32]) {
    uint8_t k0[64] = {0};
    if (klen > 64) host_sha256(key, klen, k0); else std::memcpy(k0, key, klen);
    uint8_t ipad[64], opad[64];
    for (int i = 0; i < 64; ++i) { ipad[i] = k0[i] ^ 0x36; opad[i] = k0[i] ^ 0x5c; }
    HostSha256 h1;
    h1.update(ipad, 64);
    h1.update(msg, mlen);
    uint8_t inner[32];
    h1.final(inner);
    HostSha256 h2;
    h2.update(opad, 64);
    h2.update(inner, 32);
    h2.final(out);
}

// RFC 6979 (HMAC-SHA256, qlen = 256) + ECDSA sign over a SHA-256 digest. Returns r,s little-endian.
bool p256_sign(const uint8_t d_be[32], const uint8_t digest[32], uint8_t r_le[32], uint8_t s_le[32]) {
    const fe d = fe_from_be(d_be);
    const fe n = fe_const_n();
    if (fe_is_zero(d) || fe_geq(d, n)) return false;
    const fe e = sc_reduce(fe_from_be(digest));
    uint8_t h1[32];
    fe_to_be(e, h1);  // bits2octets(h1) = int2octets(bits2int(h1) mod q)
    uint8_t V[32], K[32];
    std::memset(V, 0x01, 32);
    std::memset(K, 0x00, 32);
    uint8_t buf[32 + 1 + 32 + 32];
    auto step = [&](uint8_t sep) {
        std::memcpy(buf, V, 32);
        buf[32] = sep;
        std::memcpy(buf + 33, d_be, 32);
        std::memcpy(buf + 65, h1, 32);
        hmac_sha256(K, 32, buf, sizeof(buf), K);
        hmac_sha256(K, 32, V, 32, V);
    };
    step(0x00);
    step(0x01);
    const aff* tab = static_cast<const aff*>(p256_g_table_host());
    for (int attempt = 0; attempt < 64; ++attempt) {
        hmac_sha256(K, 32, V, 32, V);
        const fe k = fe_from_be(V);
        if (!fe_is_zero(k) && !fe_geq(k, n)) {
            aff R;
            if (jac_to_aff(mul_g(k, tab), R)) {
                const fe r = sc_reduce(R.x);
                if (!fe_is_zero(r)) {
                    // s = k^-1 (e + r d) mod n
                    const fe k_m = sc_to_mont(k);
                    const fe kinv_m = sc_inv_mont(k_m);                  // k^-1 R
                    const fe rd = sc_mont_mul(sc_to_mont(r), d);         // r d
                    fe sum;
                    const uint32_t c = raw_add(sum, e, rd);
                    fe red;
                    const uint32_t br = raw_sub(red, sum, n);
                    sum = fe_select(c || br == 0, red, sum);
                    const fe s = sc_mont_mul(sum, kinv_m);               // (e + rd) k^-1
                    if (!fe_is_zero(s)) {
                        fe_to_le(r, r_le);
                        fe_to_le(s, s_le);
                        return true;
                    }
                }
            }
        }
        uint8_t b2[33];
        std::memcpy(b2, V, 32);
        b2[32] = 0x00;
        hmac_sha256(K, 32, b2, 33, K);
        hmac_sha256(K, 32, V, 32, V);
    }
    return false;
}

}  // namespace upow
