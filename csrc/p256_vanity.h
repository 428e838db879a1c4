// K16: vanity address search, a walk over consecutive P-256 private keys with batched affine additions.
//
// reference: none. The reference wallet makes one random key (upow/upow_wallet/wallet.py createwallet via
// fastecdsa keys.gen_keypair); a search there would pay a full scalar multiplication per candidate.
//
// Consecutive scalars differ by G, so a lane (or host thread) that owns the contiguous run of scalars
// base + start .. base + start + len - 1 derives them in batches of kVanBatch = 2 H + 1 keys around a centre
// C = c G: the centre itself and C + j G, C - j G for j = 1 .. H, with j G read from the fixed-base tables
// (window 0 of both the 16-bit table in HBM and the host's byte-window table is b G). C + j G and C - j G share
// dx_j = x(j G) - x(C), and all dx_j of a batch are inverted with one fe_inv (Montgomery's trick: prefix products,
// one inversion, back-substitution). The prefix products go through `Ws` (a per-launch device workspace laid out
// lane-interleaved; a local array on a host thread), never through a runtime-indexed local array on the device.
// Per pair of keys that is 3 products for the shared inverse and, per key, 2 products and a squaring: lambda,
// x3 = lambda^2 - x1 - x2 in full, and y3 = lambda (x1 - x3) - y1, of which the address needs only the parity.
// The first centre of a run comes from the fixed-base multiplication (`MulG`, as in p256_sign.h); each further
// one is the previous centre + kVanBatch G, whose dx rides in the same batch inversion.
//
// Exceptional cases. dx = 0 means C = +-j G, so a batch may only use j with 1 <= c - j and c + j <= n - 1. A full
// batch inside [1, n - 1] does; a partial one (the tail of a run) is centred in its own span, and when that span
// has an even number of keys the unused extra position is put on the side that stays inside [1, n - 1]. j beyond
// a partial batch's reach contribute the factor 1. The centre advance C + kVanBatch G is a doubling when
// c = kVanBatch (a run starting at scalar H + 1): that factor is then left out and the next centre comes from
// MulG, as it does after the advance into a partial batch would need another table point. A zero product after
// all that is a defect: it would poison every inverse of the batch, so the run reports failure and the call
// raises instead of returning keys.
//
// NOT CONSTANT TIME, like p256_sign.h: MulG skips zero windows of the secret scalar and indexes the table by
// them. The walk is for a machine the operator trusts. `base` (the found private key minus a small index) is a
// secret; the wrappers in p256_vanity.hip overwrite its device and pinned copies.
//
// An address is the 33 bytes (42 + parity of y) | x little-endian. Read as a big-endian integer N of nine
// 32-bit words (word 0 = 42 + parity, word 1 + k = bswap32(limb k of x)), "the base58 text starts with P" is
// N in [v(P) 58^(45 - |P|), (v(P) + 1) 58^(45 - |P|)): the search tests N against up to kVanMaxRanges sorted,
// disjoint half-open ranges and never encodes base58.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "p256_field.h"
#include "p256_sign.h"
#include "p256_verify.h"

namespace upow {
using namespace p256;

static constexpr int kVanHalf = 32;                  // H: table points j G, j = 1 .. H, per batch
static constexpr int kVanBatch = 2 * kVanHalf + 1;   // B: keys per batch inversion
static constexpr int kVanSteps = 16;                 // batches per run in a full launch
static constexpr int kVanMaxRanges = 64;
static constexpr int kVanRangeWords = 18;            // lo[9] | hi[9], word 0 most significant
static_assert(kVanBatch < 256, "the host's byte-window table has b G for b < 256 only");

// a + k without reduction (the callers keep the sum at or below n)
UPOW_HD fe fe_add_u64(const fe& a, uint64_t k) {
    fe r;
    unsigned c = 0;
    r.v[0] = __builtin_addc(a.v[0], uint32_t(k), c, &c);
    r.v[1] = __builtin_addc(a.v[1], uint32_t(k >> 32), c, &c);
#pragma unroll
    for (int i = 2; i < 8; ++i) r.v[i] = __builtin_addc(a.v[i], 0u, c, &c);
    return r;
}

UPOW_HD void van_words(const fe& x, uint32_t parity, uint32_t w[9]) {
    w[0] = 42u + parity;
#pragma unroll
    for (int k = 0; k < 8; ++k) w[1 + k] = __builtin_bswap32(x.v[k]);
}
// a < b, nine words each, word 0 most significant: the final borrow of a - b
UPOW_HD bool van_less(const uint32_t a[9], const uint32_t* b) {
    unsigned c = 0;
#pragma unroll
    for (int i = 8; i >= 0; --i) (void)__builtin_subc(a[i], b[i], c, &c);
    return c != 0;
}
UPOW_HD uint64_t van_top64(const uint32_t* w) { return (uint64_t(w[0]) << 32) | w[1]; }
// w in one of the nr ranges at rg. Nearly every key fails the first test, its top 64 bits against the union's
// bounds; a range is compared in full only when the top 64 bits cannot decide.
UPOW_HD bool van_match(const uint32_t w[9], const uint32_t* rg, int nr) {
    const uint64_t key = van_top64(w);
    if (key < van_top64(rg) || key > van_top64(rg + kVanRangeWords * (nr - 1) + 9)) return false;
    bool hit = false;
#pragma nounroll
    for (int r = 0; r < nr; ++r) {
        const uint32_t* lo = rg + kVanRangeWords * r;
        if (key < van_top64(lo) || key > van_top64(lo + 9)) continue;
        hit = hit || (!van_less(w, lo) && van_less(w, lo + 9));
    }
    return hit;
}

// lambda = (qy - c.y) dinv; x3 and the parity of y3 (y3 in full through *y_out when the point goes on)
UPOW_HD fe van_add(const aff& c, const fe& qx, const fe& qy, const fe& dinv, uint32_t& parity, fe* y_out) {
    const fe lam = fe_mul(fe_sub(qy, c.y), dinv);
    const fe x3 = fe_sub(fe_sub(fe_sqr(lam), c.x), qx);
    const fe y3 = fe_sub(fe_mul(lam, fe_sub(c.x, x3)), c.y);
    parity = y3.v[0] & 1u;
    if (y_out) *y_out = y3;
    return x3;
}

// The keys of scalars base + start .. base + start + len - 1 (all inside [1, n - 1]; len >= 1), each handed to
// sink(index, x, parity of y) with index counted from `base`, in no particular order. jg[j] = j G for
// 1 <= j <= kVanBatch. false: a batch product was zero or a centre came out at infinity; the keys that
// were delivered are then not to be trusted.
template <class MulG, class Ws, class Sink>
UPOW_HD bool van_walk_run(const MulG& mulg, const aff* jg, const fe& base, int64_t start, int64_t len, Ws& ws,
                          Sink& sink) {
    aff c{fe_zero(), fe_zero()}, nxt{fe_zero(), fe_zero()};
    bool have_next = false, bad = false;
#pragma nounroll
    for (int64_t off = 0; off < len; off += kVanBatch) {
        const int64_t left = len - off;
        const int m = left < kVanBatch ? int(left) : kVanBatch;
        int lo_n = m >> 1, hi_n = m - 1 - lo_n;  // keys below and above the centre
        // m even: the symmetric window has one position more than the batch, above it; below when that is n
        if (!(m & 1) && fe_eq(fe_add_u64(base, uint64_t(start + off + m)), fe_const_n())) {
            lo_n -= 1;
            hi_n += 1;
        }
        const int jmax = lo_n > hi_n ? lo_n : hi_n;
        const int64_t ci = start + off + lo_n;
        if (!have_next) {
            if (!jac_to_aff(mulg(fe_add_u64(base, uint64_t(ci))), c)) bad = true;
        } else {
            c = nxt;
        }
        have_next = false;
        sink(ci, c.x, c.y.v[0] & 1u);
        // the next centre is this one + B G when both batches are full
        const bool adv = m == kVanBatch && left - kVanBatch >= kVanBatch;
        if (jmax == 0 && !adv) continue;
        fe d0 = fe_sub(jg[kVanBatch].x, c.x);
        const bool use_adv = adv && !fe_is_zero(d0);  // zero: c = B, the advance would double the centre
        d0 = fe_select(use_adv, d0, fe_one());
        fe run = d0;
#pragma nounroll
        for (int j = 1; j <= kVanHalf; ++j) {
            ws.put(j - 1, run);
            run = fe_mul(run, fe_select(j <= jmax, fe_sub(jg[j].x, c.x), fe_one()));
        }
        bad = bad || fe_is_zero(run);
        fe inv = fe_inv(run);
#pragma nounroll
        for (int j = kVanHalf; j >= 1; --j) {
            const aff q = jg[j];
            const fe dinv = fe_mul(inv, ws.get(j - 1));
            inv = fe_mul(inv, fe_select(j <= jmax, fe_sub(q.x, c.x), fe_one()));
            uint32_t par;
            if (j <= hi_n) {
                const fe x3 = van_add(c, q.x, q.y, dinv, par, nullptr);
                sink(ci + j, x3, par);
            }
            if (j <= lo_n) {
                const fe x3 = van_add(c, q.x, fe_neg(q.y), dinv, par, nullptr);
                sink(ci - j, x3, par);
            }
        }
        if (use_adv) {  // inv = 1 / d0
            const aff q = jg[kVanBatch];
            uint32_t par;
            nxt.x = van_add(c, q.x, q.y, inv, par, &nxt.y);
            have_next = true;
        }
    }
    return !bad;
}

// the prefix products of one host thread
struct VanHostWs {
    fe p[kVanHalf];
    UPOW_HD void put(int j, const fe& a) { p[j] = a; }
    UPOW_HD fe get(int j) const { return p[j]; }
};

}  // namespace upow
