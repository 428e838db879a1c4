// K15 batched: P-256 key derivation and RFC 6979 ECDSA signing, one item per GPU lane or host thread.
//
// reference: fastecdsa keys.get_public_key / ecdsa.sign (RFC 6979 nonces, no low-s normalisation) as called
// from upow/helpers.py:58-62,135-144 and upow/upow_transactions/transaction.py:148-180.
//
// The text below is UPOW_HD and templated on the SHA-256 compression (`Compress`: st[8], w[16] -> st, w may
// be clobbered) and on the fixed-base multiplication (`MulG`: scalar -> k*G in Jacobian form), so the kernels
// of csrc/p256_sign.hip (dev_compress, the 16-bit window table in HBM) and a host thread (host_compress_words,
// the byte-window table) run the same code. csrc/p256_sign.hip's p256_sign / p256_pubkey are written separately
// (byte-oriented HMAC, Fermat inverse) and stay the reference this code is tested against.
//
// NOT CONSTANT TIME: the fixed-base multiplication skips zero windows of the secret scalar, the table reads
// are indexed by its windows, the divsteps inverse exits early and the candidate loop branches on the nonce.
// This is for bulk signing (test chains, benchmark traffic, payout runs) on a machine the operator trusts;
// single wallet signatures stay on the host path.
//
// All octet strings of RFC 6979 are 32 bytes here (qlen = hlen = 256), held as eight big-endian words: word i
// of int2octets(x) is limb 7 - i of the fe x.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "p256_field.h"
#include "p256_verify.h"

namespace upow {
using namespace p256;

UPOW_HD void sha256_iv(uint32_t st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// state after the key block of HMAC's inner (pad = 0x36363636) or outer (0x5c5c5c5c) hash, 32-byte key
template <class Compress>
UPOW_HD void hmac_key_block(const Compress& c, const uint32_t key[8], uint32_t pad, uint32_t st[8]) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        w[i] = key[i] ^ pad;
        w[8 + i] = pad;
    }
    sha256_iv(st);
    c(st, w);
}

// out = H((key ^ opad) || inner): the outer hash over the finished inner state
template <class Compress>
UPOW_HD void hmac_outer(const Compress& c, const uint32_t key[8], const uint32_t inner[8], uint32_t out[8]) {
    uint32_t st[8], w[16];
    hmac_key_block(c, key, 0x5c5c5c5cu, st);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = inner[i];
    w[8] = 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 32) * 8;
    c(st, w);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = st[i];
}

// out = HMAC(key, v) (zero = false) or HMAC(key, v || 0x00) (zero = true); out may alias key or v
template <class Compress>
UPOW_HD void hmac_v(const Compress& c, const uint32_t key[8], const uint32_t v[8], bool zero, uint32_t out[8]) {
    uint32_t st[8], w[16];
    hmac_key_block(c, key, 0x36363636u, st);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = v[i];
    w[8] = zero ? 0x00800000u : 0x80000000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = zero ? (64 + 33) * 8 : (64 + 32) * 8;
    c(st, w);
    hmac_outer(c, key, st, out);
}

// out = HMAC(key, v || sep || x || h) (97 bytes: x and h sit one byte off the word grid); out may alias key
template <class Compress>
UPOW_HD void hmac_seed(const Compress& c, const uint32_t key[8], const uint32_t v[8], uint32_t sep,
                       const uint32_t x[8], const uint32_t h[8], uint32_t out[8]) {
    uint32_t st[8], w[16];
    hmac_key_block(c, key, 0x36363636u, st);
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = v[i];
    w[8] = (sep << 24) | (x[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; ++i) w[8 + i] = (x[i - 1] << 24) | (x[i] >> 8);
    c(st, w);
    w[0] = (x[7] << 24) | (h[0] >> 8);
#pragma unroll
    for (int i = 1; i < 8; ++i) w[i] = (h[i - 1] << 24) | (h[i] >> 8);
    w[8] = (h[7] << 24) | 0x00800000u;
#pragma unroll
    for (int i = 9; i < 15; ++i) w[i] = 0;
    w[15] = (64 + 97) * 8;
    c(st, w);
    hmac_outer(c, key, st, out);
}

UPOW_HD void fe_to_octets(const fe& a, uint32_t o[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = a.v[7 - i];
}

// RFC 6979 section 3.2 HMAC_DRBG for P-256 with SHA-256: init() is steps b-g, next() step h. Every call
// of next() returns T = bits2int(V) whether or not it is a usable nonce; asked again, it first makes the
// K = HMAC(K, V || 0x00), V = HMAC(K, V) update that follows a rejected candidate.
template <class Compress>
struct Rfc6979 {
    uint32_t K[8], V[8];
    bool again;

    // d: the private key; h1: bits2int(digest) mod n (bits2octets)
    UPOW_HD void init(const Compress& c, const fe& d, const fe& h1) {
        uint32_t x[8], h[8];
        fe_to_octets(d, x);
        fe_to_octets(h1, h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            V[i] = 0x01010101u;
            K[i] = 0;
        }
#pragma nounroll
        for (uint32_t sep = 0; sep < 2; ++sep) {
            hmac_seed(c, K, V, sep, x, h, K);
            hmac_v(c, K, V, false, V);
        }
        again = false;
    }

    UPOW_HD fe next(const Compress& c) {
        if (again) {
            hmac_v(c, K, V, true, K);
            hmac_v(c, K, V, false, V);
        }
        again = true;
        hmac_v(c, K, V, false, V);
        fe k;
#pragma unroll
        for (int i = 0; i < 8; ++i) k.v[i] = V[7 - i];
        return k;
    }
};

static constexpr int kSignMaxCandidates = 64;

UPOW_HD bool sign_key_ok(const fe& d) { return !fe_is_zero(d) && !fe_geq(d, fe_const_n()); }

// Q = d*G for d in [1, n - 1]
template <class MulG>
UPOW_HD bool pubkey_one(const MulG& mulg, const fe& d, aff& q) {
    if (!sign_key_ok(d)) return false;
    return jac_to_aff(mulg(d), q);
}

// ECDSA over the digest (as the integer bits2int(digest), not yet reduced) with the RFC 6979 nonce; the steps
// of p256_sign (csrc/p256_sign.hip). false: key outside [1, n - 1], or no usable candidate in kSignMaxCandidates.
template <class Compress, class MulG>
UPOW_HD bool sign_one(const Compress& c, const MulG& mulg, const fe& d, const fe& digest, fe& r, fe& s) {
    if (!sign_key_ok(d)) return false;
    const fe n = fe_const_n();
    const fe e = sc_reduce(digest);
    Rfc6979<Compress> drbg;
    drbg.init(c, d, e);
#pragma nounroll
    for (int attempt = 0; attempt < kSignMaxCandidates; ++attempt) {
        const fe k = drbg.next(c);
        if (fe_is_zero(k) || fe_geq(k, n)) continue;
        aff R;
        if (!jac_to_aff(mulg(k), R)) continue;
        r = sc_reduce(R.x);
        if (fe_is_zero(r)) continue;
        // s = k^-1 (e + r d) mod n
        const fe kinv_m = sc_inv_safegcd_mont(k);            // k^-1 R
        const fe rd = sc_mont_mul(sc_to_mont(r), d);         // r d
        fe sum, red;
        const uint32_t cy = raw_add(sum, e, rd);
        const uint32_t br = raw_sub(red, sum, n);
        sum = fe_select(cy || br == 0, red, sum);
        s = sc_mont_mul(sum, kinv_m);                        // (e + r d) k^-1
        if (!fe_is_zero(s)) return true;
    }
    return false;
}

// the fixed-base multiplications the core is instantiated with
// jac_madd (madd-2007-bl) for the fixed-base windows, written without early exits: merged in the rolled window
// loop below, jac_madd's four return paths put the accumulator in scratch memory (68 bytes per lane); this form
// compiles to registers only. p at infinity gives q. h = 0 (p = +-q) sets `bad` and nothing else: it cannot
// happen for a scalar in [1, n - 1], whose partial sum below window j is smaller than every entry of window j
// and, added to one, smaller than n.
UPOW_HD jac madd_window(const jac& p, const aff& q, bool& bad) {
    const fe z1z1 = fe_sqr(p.z);
    const fe u2 = fe_mul(q.x, z1z1);
    const fe s2 = fe_mul(fe_mul(q.y, p.z), z1z1);
    const fe h = fe_sub(u2, p.x);
    const fe rr0 = fe_sub(s2, p.y);
    const fe hh = fe_sqr(h);
    fe i = fe_add(hh, hh);
    i = fe_add(i, i);
    const fe j = fe_mul(h, i);
    const fe rr = fe_add(rr0, rr0);
    const fe v = fe_mul(p.x, i);
    const fe x3 = fe_sub(fe_sub(fe_sqr(rr), j), fe_add(v, v));
    const fe y1j = fe_mul(p.y, j);
    const fe y3 = fe_sub(fe_mul(rr, fe_sub(v, x3)), fe_add(y1j, y1j));
    const fe zh = fe_add(p.z, h);
    const fe z3 = fe_sub(fe_sub(fe_sqr(zh), z1z1), hh);
    const bool pinf = fe_is_zero(p.z);
    bad = bad || (!pinf && fe_is_zero(h));
    return jac{fe_select(pinf, q.x, x3), fe_select(pinf, q.y, y3), fe_select(pinf, fe_one(), z3)};
}

struct MulG16 {  // the kernels: the 16-bit windows of mul_g16 over the table in HBM
    const aff* tab16;
    // The windows are shifted out of the scalar instead of indexed (mul_g16's k.v[j >> 1]): with the loop left
    // rolled, to keep one copy of the mixed addition, a runtime limb index would put the secret scalar in
    // scratch memory. A `bad` addition yields infinity, which every caller treats as failure.
    UPOW_HD jac operator()(fe k) const {
        jac acc = jac_inf();
        bool bad = false;
#pragma nounroll
        for (int j = 0; j < kG16Win; ++j) {
            const uint32_t b = k.v[0] & 0xffffu;
#pragma unroll
            for (int l = 0; l < 7; ++l) k.v[l] = (k.v[l] >> 16) | (k.v[l + 1] << 16);
            k.v[7] >>= 16;
            if (b) acc = madd_window(acc, tab16[size_t(j) * kG16Ent + b], bad);
        }
        acc.z = fe_select(bad, fe_zero(), acc.z);
        return acc;
    }
};
struct MulG8 {  // host threads: byte windows
    const aff* tab;
    UPOW_HD jac operator()(const fe& k) const { return mul_g(k, tab); }
};

}  // namespace upow
