// The lane-group step schedule of the block-latency verify (four or eight lanes per signature), written once
// and shared by the kernels (csrc/p256.hip), their one-thread host emulation (p256_verify_host, modes 'quad'
// and 'oct') and the arithmetic probe (csrc/p256_probe.h): XYZZ points, the pair-split product, the host and
// device step policies, the point formulas over a policy, the quarter multiplications of u1*G and the shared
// verify body.
//
// reference: fastecdsa ecdsa.verify as called from upow/upow_transactions/transaction_input.py:84-120.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "p256_field.h"
#include "p256_verify.h"

namespace upow {
using namespace p256;

// XYZZ coordinates (x = X/ZZ, y = Y/ZZZ) of the lane-group kernels
struct xz { fe x, y, zz, zzz; };  // XYZZ point; zz == 0 <=> infinity
static_assert(sizeof(xz) == 128, "xz layout");

// Jacobian (X, Y, Z) -> XYZZ (X, Y, Z^2, Z^3): the same affine point, one lane on its own
UPOW_HD xz jac_to_xz(const jac& p) {
    const fe zz = fe_sqr(p.z);
    return xz{p.x, p.y, zz, fe_mul(zz, p.z)};
}

// The arithmetic of the eight-lane kernel's pair-split product (OctDev::mul_pair below): each lane of a
// pair (k, k + 4) runs four of the eight schoolbook rows (`split_rows`), the lower lane adds the upper lane's
// 12-word partial sum to its own and reduces (`combine_rows`). mul_pair_host plays both lanes on one thread;
// tests/test_p256_arith.py (check_field_binary, operation 'mul_pair' of the p256_probe hook) compares it with
// a*b mod p on the operand pairs fe_mul gets, among them the ones whose column-11 carry runs through columns
// 12..15, and tests/test_p256_arith_gpu.py runs the same pairs through both device builds.
UPOW_HD void split_rows(uint32_t p[12], const fe& a, const fe& b, bool upper) {
    uint32_t ar[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ar[i] = upper ? a.v[4 + i] : a.v[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) p[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned cy = 0;
        uint32_t prev = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t t = uint64_t(ar[i]) * b.v[j] + p[i + j];
            p[i + j] = __builtin_addc(uint32_t(t), prev, cy, &cy);
            prev = uint32_t(t >> 32);
        }
        p[i + 8] = prev + cy;
    }
}
// lo: columns 0..11 of the lower rows; hi: columns 4..15 of the upper rows (hi[w] is column w + 4)
UPOW_HD fe combine_rows(const uint32_t lo[12], const uint32_t hi[12]) {
    uint32_t c[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) c[w] = lo[w];
    unsigned cy = 0;
#pragma unroll
    for (int w = 4; w < 12; ++w) c[w] = __builtin_addc(lo[w], hi[w - 4], cy, &cy);
#pragma unroll
    for (int w = 12; w < 16; ++w) c[w] = __builtin_addc(0u, hi[w - 4], cy, &cy);
    return fe_reduce(c);
}

UPOW_HD fe mul_pair_host(const fe& a, const fe& b) {
    uint32_t lo[12], hi[12];
    split_rows(lo, a, b, false);
    split_rows(hi, a, b, true);
    return combine_rows(lo, hi);
}

// ------------------------------------------------------------------------------------------------
// four lanes per signature (latency path for one block)
// ------------------------------------------------------------------------------------------------
// One 2 MB block is ~8,300 signatures = 130 waves at one signature per lane: 130 of the chip's 1,024
// SIMDs are busy and the launch takes as long as one wave's serial chain (~3 ms). A wave64 VALU op
// costs its four passes whatever the exec mask (profiles/p256_latency_ab.txt: 16 signatures per wave
// run no faster than 64), so the only way to cut that latency is to split each signature's chain over
// more lanes. Here a lane quad (4k .. 4k+3) owns one signature: all four lanes keep the whole point
// state (redundantly) and the field products of the point formulas are scheduled in "steps" of up to
// four independent products, one per lane; DPP quad_perm broadcasts hand every lane the others'
// results (8 v_mov_dpp per product). Adds/subs stay redundant: they are cheap next to a 256x256-bit
// product. Points are in XYZZ coordinates (x = X/ZZ, y = Y/ZZZ), whose formulas are shallow:
//   doubling (a = -3, dbl-2008-s-1)            9 products, depth 3  -> 3 steps (the first all squares)
//   addition (add-2008-s)                      14 products, depth 4 -> 4 steps
// (Jacobian doubling is 8 products but depth 4: 4 steps however many lanes.) A 4-bit window (4
// doublings + 1 addition) is 16 steps instead of 48 serial products; with signed 5-bit windows
// (Booth recoding: 52 windows of 5 doublings + 1 addition) u2*Q is 51 x 15 + 52 x 4 = 973 steps. The
// window table k*Q (k = 1..16) is built the same way (3 + 14 x 4 steps). u1*G (32 fixed-base byte windows) splits by quarters:
// each lane accumulates 8 windows on its own (Jacobian mixed adds), converts to XYZZ, and the four
// partial points are broadcast and added. s^-1 runs redundantly on all four lanes (binary Euclid).
// Waves go four to a workgroup so they land on four different SIMDs of a CU (single-wave workgroups
// double up on one SIMD once there are more waves than CUs: profiles/p256_latency_ab.txt).
//
// The schedule is written once over a policy type: QuadDev broadcasts through DPP on the GPU;
// QuadHost (one host thread) computes every product of a step itself, which lets the CPU tests check
// the formulas and the step schedule bit for bit against the reference verifier.
//
// The host policy, by its product and (when it has its own code) square function: QuadHost plays the quad
// kernel's lanes (fe_mul, and fe_sqr for the all-squares step), OctHost the eight-lane kernel's pair-split
// product for both.
template <fe (*MUL)(const fe&, const fe&), fe (*SQR)(const fe&) = nullptr>
struct HostSteps {
    static UPOW_HD fe sqr(const fe& a) {
        if constexpr (SQR != nullptr) return SQR(a);
        else return MUL(a, a);
    }
    UPOW_HD void sqr4(const fe& a0, const fe& a1, const fe& a2, const fe& a3, fe& r0, fe& r1, fe& r2, fe& r3) const {
        const fe m0 = sqr(a0), m1 = sqr(a1), m2 = sqr(a2), m3 = sqr(a3);
        r0 = m0;
        r1 = m1;
        r2 = m2;
        r3 = m3;
    }
    UPOW_HD void mul4(const fe& a0, const fe& b0, const fe& a1, const fe& b1, const fe& a2, const fe& b2,
                      const fe& a3, const fe& b3, fe& r0, fe& r1, fe& r2, fe& r3) const {
        const fe m0 = MUL(a0, b0), m1 = MUL(a1, b1), m2 = MUL(a2, b2), m3 = MUL(a3, b3);
        r0 = m0;
        r1 = m1;
        r2 = m2;
        r3 = m3;
    }
};
using QuadHost = HostSteps<fe_mul, fe_sqr>;
using OctHost = HostSteps<mul_pair_host>;

template <int K>
__device__ __forceinline__ fe fe_quad_bcast(const fe& a) {  // every lane of the quad gets lane K's value
    fe r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.v[i] = uint32_t(__builtin_amdgcn_mov_dpp(int(a.v[i]), K * 0x55, 0xF, 0xF, true));
    return r;
}
// the end of every device step: lane K's product to every lane of its quad as r<K>
__device__ __forceinline__ void fe_quad_bcast4(const fe& m, fe& r0, fe& r1, fe& r2, fe& r3) {
    r0 = fe_quad_bcast<0>(m);
    r1 = fe_quad_bcast<1>(m);
    r2 = fe_quad_bcast<2>(m);
    r3 = fe_quad_bcast<3>(m);
}

// A device policy also names its group's geometry for the kernels built over it: kLanes lanes per group,
// of_lane(lane) this lane's policy, leader(lane) the one lane of a group that stores the group's result.
struct QuadDev {
    static constexpr int kLanes = 4;
    bool odd, hi;  // this lane's role in its quad (lane & 3): bit 0 and bit 1
    static __device__ __forceinline__ QuadDev of_lane(int lane) { return QuadDev{(lane & 1) != 0, (lane & 2) != 0}; }
    static __device__ __forceinline__ bool leader(int lane) { return (lane & 3) == 0; }
    // a_role as a two-level select tree on the role's bits: the compiler folds a select of two identical
    // operands, so the schedule's repeated operands cost less than three selects per word — (a, b, c, c)
    // and (v, v, m, z) take two, (x, y, x, y) one (the linear chain on role == 1/2/3 folded less)
    __device__ __forceinline__ fe pick(const fe& a0, const fe& a1, const fe& a2, const fe& a3) const {
        fe r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t lo = odd ? a1.v[i] : a0.v[i];
            const uint32_t up = odd ? a3.v[i] : a2.v[i];
            r.v[i] = hi ? up : lo;
        }
        return r;
    }
    // a step whose four products are all squares: the squaring row code (36 partial products, not 64)
    __device__ __forceinline__ void sqr4(const fe& a0, const fe& a1, const fe& a2, const fe& a3, fe& r0, fe& r1, fe& r2,
                                         fe& r3) const {
        fe_quad_bcast4(fe_sqr(pick(a0, a1, a2, a3)), r0, r1, r2, r3);
    }
    __device__ __forceinline__ void mul4(const fe& a0, const fe& b0, const fe& a1, const fe& b1, const fe& a2,
                                         const fe& b2, const fe& a3, const fe& b3, fe& r0, fe& r1, fe& r2,
                                         fe& r3) const {
        fe_quad_bcast4(fe_mul(pick(a0, a1, a2, a3), pick(b0, b1, b2, b3)), r0, r1, r2, r3);
    }
};

// Eight lanes per signature (two quads, `hi` = the upper one): every product of a step is split over a lane
// PAIR (k, k + 4). Each lane runs four of the eight schoolbook rows (32 v_mad_u64_u32 instead of 64: the
// quarter-rate 64-bit multiply-adds are half of a step's time), the upper lane's 12-word partial sum
// crosses to its partner with DPP row_shl:4, the lower lane adds it and reduces, and row_shr:4 hands the
// reduced product back to the upper lane; quad_perm broadcasts then give all four products to every lane
// of both quads. 8,300 signatures fill 1,038 waves, one per SIMD of the chip, where the quad kernel left
// half of the SIMDs idle. `split_rows` / `combine_rows` (above) are the arithmetic;
// tests/test_p256_arith.py runs them on one thread (mul_pair_host: both halves) against a*b mod p, and
// tests/test_p256_arith_gpu.py checks what every lane of an octet receives from mul_pair and the broadcasts.
struct OctDev {
    static constexpr int kLanes = 8;
    bool is1, is2, is3, hi;  // lane & 3, and whether the lane is in the octet's upper quad
    static __device__ __forceinline__ OctDev of_lane(int lane) {
        const int role = lane & 3;
        return OctDev{role == 1, role == 2, role == 3, (lane & 4) != 0};
    }
    static __device__ __forceinline__ bool leader(int lane) { return (lane & 3) == 0 && (lane & 4) == 0; }
    __device__ __forceinline__ fe pick(const fe& a0, const fe& a1, const fe& a2, const fe& a3) const {
        fe r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t t = a0.v[i];
            t = is1 ? a1.v[i] : t;
            t = is2 ? a2.v[i] : t;
            r.v[i] = is3 ? a3.v[i] : t;
        }
        return r;
    }
    __device__ __forceinline__ fe mul_pair(const fe& a, const fe& b) const {
        uint32_t p[12], q[12];
        split_rows(p, a, b, hi);
#pragma unroll
        for (int w = 0; w < 12; ++w) q[w] = uint32_t(__builtin_amdgcn_mov_dpp(int(p[w]), 0x104, 0xF, 0xF, true));  // row_shl:4
        const fe m = combine_rows(p, q);  // meaningful on the lower quad
        fe r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t from_lo = uint32_t(__builtin_amdgcn_mov_dpp(int(m.v[i]), 0x114, 0xF, 0xF, true));  // row_shr:4
            r.v[i] = hi ? from_lo : m.v[i];
        }
        return r;
    }
    __device__ __forceinline__ void sqr4(const fe& a0, const fe& a1, const fe& a2, const fe& a3, fe& r0, fe& r1, fe& r2,
                                         fe& r3) const {
        const fe a = pick(a0, a1, a2, a3);
        fe_quad_bcast4(mul_pair(a, a), r0, r1, r2, r3);
    }
    __device__ __forceinline__ void mul4(const fe& a0, const fe& b0, const fe& a1, const fe& b1, const fe& a2,
                                         const fe& b2, const fe& a3, const fe& b3, fe& r0, fe& r1, fe& r2,
                                         fe& r3) const {
        fe_quad_bcast4(mul_pair(pick(a0, a1, a2, a3), pick(b0, b1, b2, b3)), r0, r1, r2, r3);
    }
};

// fewer products per step: the spare lanes repeat the last product (its broadcast is dead code)
template <class P>
UPOW_HD void mul3(const P& pp, const fe& a0, const fe& b0, const fe& a1, const fe& b1, const fe& a2, const fe& b2,
                  fe& r0, fe& r1, fe& r2) {
    fe d;
    pp.mul4(a0, b0, a1, b1, a2, b2, a2, b2, r0, r1, r2, d);
}
template <class P>
UPOW_HD void mul2(const P& pp, const fe& a0, const fe& b0, const fe& a1, const fe& b1, fe& r0, fe& r1) {
    fe d0, d1;
    pp.mul4(a0, b0, a1, b1, a1, b1, a1, b1, r0, r1, d0, d1);
}
template <class P>
UPOW_HD void mul1(const P& pp, const fe& a0, const fe& b0, fe& r0) {
    fe d0, d1, d2;
    pp.mul4(a0, b0, a0, b0, a0, b0, a0, b0, r0, d0, d1, d2);
}

UPOW_HD fe fe_x3(const fe& a) { return fe_add(fe_add(a, a), a); }

// dbl-2008-s-1 with a = -3: M = 3 X^2 - 3 ZZ^2. The first step is three squarings (U^2, X^2, ZZ^2),
// issued with the squaring code. Infinity (ZZ = 0) stays infinity.
template <class P>
UPOW_HD void dbl4(const P& pp, xz& p) {
    const fe u = fe_add(p.y, p.y);
    fe v, xx, zz2, unused;
    pp.sqr4(u, p.x, p.zz, p.zz, v, xx, zz2, unused);
    const fe m = fe_x3(fe_sub(xx, zz2));
    fe w, s, mm, zz3;
    pp.mul4(u, v, p.x, v, m, m, v, p.zz, w, s, mm, zz3);
    const fe x3 = fe_sub(mm, fe_add(s, s));
    fe ya, wy, zzz3;
    mul3(pp, m, fe_sub(s, x3), w, p.y, w, p.zzz, ya, wy, zzz3);
    p.x = x3;
    p.y = fe_sub(ya, wy);
    p.zz = zz3;
    p.zzz = zzz3;
}

// add-2008-s with the reference verifier's special cases (infinity, P == Q, P == -Q)
template <class P>
UPOW_HD void add4(const P& pp, xz& p, const xz& q) {
    if (fe_is_zero(q.zz)) return;
    if (fe_is_zero(p.zz)) { p = q; return; }
    fe u1, u2, s1, s2;
    pp.mul4(p.x, q.zz, q.x, p.zz, p.y, q.zzz, q.y, p.zzz, u1, u2, s1, s2);
    const fe ph = fe_sub(u2, u1), r = fe_sub(s2, s1);
    if (fe_is_zero(ph)) {
        if (fe_is_zero(r)) dbl4(pp, p);
        else p.zz = p.zzz = fe_zero();
        return;
    }
    fe pp2, rr, zz12, zzz12;
    pp.mul4(ph, ph, r, r, p.zz, q.zz, p.zzz, q.zzz, pp2, rr, zz12, zzz12);
    fe ppp, qq, zz3;
    mul3(pp, ph, pp2, u1, pp2, zz12, pp2, ppp, qq, zz3);
    const fe x3 = fe_sub(fe_sub(rr, ppp), fe_add(qq, qq));
    fe ya, s1p, zzz3;
    mul3(pp, r, fe_sub(qq, x3), s1, ppp, zzz12, ppp, ya, s1p, zzz3);
    p.x = x3;
    p.y = fe_sub(ya, s1p);
    p.zz = zz3;
    p.zzz = zzz3;
}

// the 64 bits of k that one lane's quarter (0..3) of u1*G covers, selected without dynamic register indexing
UPOW_HD void quarter_limbs(const fe& k, int quarter, uint32_t& lo, uint32_t& hi) {
    lo = k.v[0];
    hi = k.v[1];
#pragma unroll
    for (int l = 1; l < 4; ++l) {
        lo = quarter == l ? k.v[2 * l] : lo;
        hi = quarter == l ? k.v[2 * l + 1] : hi;
    }
}

// u1*G over the byte windows [8*quarter, 8*quarter + 8) (one lane's share), Jacobian mixed adds
UPOW_HD jac mul_g_quarter(const fe& k, const aff* tab, int quarter) {
    jac acc = jac_inf();
    uint32_t lo, hi;  // this quarter's 64 bits, consumed a byte at a time
    quarter_limbs(k, quarter, lo, hi);
    const aff* t = tab + quarter * 8 * kGEnt;
    for (int j = 0; j < 8; ++j) {
        const uint32_t b = lo & 0xffu;
        lo = (lo >> 8) | (hi << 24);
        hi >>= 8;
        if (b) acc = jac_madd(acc, t[j * kGEnt + b]);
    }
    return acc;
}

UPOW_HD jac mul_g16_quarter(const fe& k, const aff* tab16, int quarter) {
    uint32_t lo, hi;  // this quarter's 64 bits, consumed 16 at a time
    quarter_limbs(k, quarter, lo, hi);
    const aff* t = tab16 + size_t(quarter) * 4 * kG16Ent;
    jac acc = jac_inf();
    for (int j = 0; j < 4; ++j) {
        const uint32_t b = lo & 0xffffu;
        lo = (lo >> 16) | (hi << 16);
        hi >>= 16;
        if (b) acc = jac_madd(acc, t[size_t(j) * kG16Ent + b]);
    }
    return acc;
}

// Shared verify body. `tab` holds this signature's 16 window entries 1Q..16Q (global scratch on the GPU, a
// local array on the host); `gpart(K)` yields quarter K of u1*G in XYZZ form (on the GPU: lane K's own
// quarter, broadcast). On the GPU every lane of the quad stores the (identical)
// entries, so each later table read is of the lane's own store.
template <class P, class GPart>
UPOW_HD uint8_t verify_quad_core(const P& pp, const aff& q, const fe& r, const fe& u2, xz* tab, GPart gpart) {
    const fe one = fe_one();
    const xz t1{q.x, q.y, one, one};
    xz t = t1;
    tab[0] = t;  // tab[k - 1] = k*Q, k = 1..16
    dbl4(pp, t);
    tab[1] = t;
    for (int k = 3; k <= 16; ++k) {
        add4(pp, t, t1);
        tab[k - 1] = t;
    }
    // u2*Q: 52 signed 5-bit windows (BoothW5) from the top, so 52 additions instead of the 64 of
    // unsigned 4-bit windows; a negative digit adds the entry with -Y
    xz acc{one, one, fe_zero(), fe_zero()};
    BoothW5 bw(u2);
    for (int w = kBoothWindows - 1; w >= 0; --w) {
        const int d = bw.next();
        xz e;
        if (d) {
            e = tab[(d < 0 ? -d : d) - 1];
            if (d < 0) e.y = fe_neg(e.y);
        }
        if (w != kBoothWindows - 1) {
            dbl4(pp, acc);
            dbl4(pp, acc);
            dbl4(pp, acc);
            dbl4(pp, acc);
            dbl4(pp, acc);
        }
        if (d) add4(pp, acc, e);
    }
    // + u1*G, added a quarter at a time
    add4(pp, acc, gpart(std::integral_constant<int, 0>{}));
    add4(pp, acc, gpart(std::integral_constant<int, 1>{}));
    add4(pp, acc, gpart(std::integral_constant<int, 2>{}));
    add4(pp, acc, gpart(std::integral_constant<int, 3>{}));
    if (fe_is_zero(acc.zz)) return 0;
    return x_matches_r(acc.x, acc.zz, r);
}

}  // namespace upow
