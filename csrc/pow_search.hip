// K1: SHA-256 proof-of-work nonce search for gfx950 (CDNA4, wave64).
//
// reference hot loop: miner.py:83-98 (one hashlib.sha256 per nonce in Python) with the predicate of
// miner.py:43-61 / upow/manager.py:130-151.
//
// MI355X design
//  * one nonce per lane, 64 nonces per wavefront, grid-strided over the 2^32 nonce space (variant 10: a wave
//    walks U with its lanes 2^p words apart, a range cut into power-of-two pieces);
//  * the header's first 64-byte block is nonce independent -> host midstate;
//  * v2 header (108 B): the tail block's words W0..W9 are nonce independent too, so the host also
//    runs rounds 0..9 and the kernel starts at round 10 (W10 = the nonce word);
//    v1 header (138 B): the nonce straddles W1/W2 of the third block; the kernel starts at round 1;
//  * every job constant is a kernel argument -> SGPRs, and so is every nonce-independent value of the
//    tail block (constant schedule words folded with K, the constant part of partly constant words, the
//    first dependent round's sums): make_pow_job computes them once per job, so no lane-uniform value is
//    computed with VALU rotates in the prologue and kept in a VGPR for the loop (61 VGPRs, 8 waves/SIMD;
//    the compiler-hoisted form of the same loop, kept as variant 3, needs 85 VGPRs -> 5 waves/SIMD);
//  * the message schedule is kept in VGPRs (a 16-entry rolling window), not LDS: each W word is
//    produced once and consumed 4x within ~16 rounds; an LDS round trip per use would add a
//    ds_write+4 ds_read per word (≈240 LDS dword ops per nonce) against ≈1.2k VALU ops, making LDS a
//    co-bottleneck (MI355X_MICROARCH.md §LDS: 32 dwords/clk/CU for b32 vs 128 VALU lane-ops/clk/CU);
//  * rotates lower to v_alignbit_b32, the 3-input XORs of the Sigma functions and Maj to the gfx950
//    v_bitop3_b32 (truth tables 0x96 / 0xE8), 3-input adds to v_add3_u32 (1107 VALU ops per nonce in
//    the v2 loop body vs 1359 with 2-input XORs);
//  * variant 9 (pow_h0_sched) issues pow_h0_pre's instructions in a pinned order with an s_sleep 0 in front of
//    every v_alignbit_b32 and v_add3_u32: behind that sequencer-only instruction the two slow opcodes cost about
//    a cycle less (3.66 against 3.94 cycles per VALU instruction, docs/PERF.md);
//  * variant 10 (pow_a_split) is variant 9 with the lane index in the TOP bits of the nonce
//    word, v = vb + U + (lane << p): what all 64 lanes of a wave would compute alike (the low p bits of W10, a11,
//    e11, W17, W24 and their sigmas, round 11's Ch and Maj) is done once per wave on the SALU, one scalar
//    instruction in the place of one s_sleep 0, and the per-lane high bits are loop-invariant VGPRs: 1,085 VALU
//    instructions per nonce against 1,108, 446 rotates against 462 (docs/PERF.md, "PoW lane/uniform split");
//  * the default v2 kernel (pow_a_fill, variant 11) is variant 10 with exactly one scalar or sequencer instruction in
//    front of every v_alignbit_b32 and v_add3_u32 and none doubled up: each K[i] is loaded in a scalar slot of its own,
//    rounds 12 and 13 are pinned too, and the nonce word, W17 and the range check's add are not VALU instructions any
//    more: 1,082 VALU instructions per nonce (docs/PERF.md, "PoW scalar slots");
//  * the default kernel (pow_search_claim_kernel, variant 12) runs variant 11's loop with no fixed share per wave: a
//    wave claims 32 values of U at a time from a counter until the dispatch's range is used up, and a sweep is one
//    dispatch. With fixed shares the eight waves of a SIMD finish one after the other, oldest first, and the median
//    wave lives for 0.54 of its dispatch (docs/PERF.md, "PoW claimed chunks");
//  * the predicate only needs digest word H0 for difficulty < 8 (8 hex nibbles) -> one compare per
//    nonce (variant 10: one add and one unsigned compare, (H0 - tword) < width); hits are appended with an atomic to a small candidate list and re-checked exactly on the
//    host (covers d >= 8 and the d < 1 "whole hash" quirk).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>

#include "native.h"
#include "streams.h"
#include "sha256_common.h"

namespace upow {

struct PowJobDev {
    uint32_t st[8];   // working state after the nonce-independent rounds of the tail block
    uint32_t mid[8];  // chaining value before the tail block (feed-forward)
    uint32_t w[16];   // tail block words (nonce bits zero)
    uint32_t tmask;   // H0 bits that must equal tword
    uint32_t tword;
    uint32_t frac_shift;  // right shift of H0 that brings the fractional nibble to bits 0..3
    uint32_t frac_limit;  // nibble must be < frac_limit (16 == no fractional check)
    // Nonce-independent values of the tail block, computed once per job on the host (make_pow_job) and read
    // by pow_h0_pre as kernel arguments, i.e. from SGPRs. R0 = first nonce-dependent round (v2: 10, v1: 1).
    uint32_t ca, ce;   // round R0 with a constant state: a' = ca + W[R0], e' = ce + W[R0]
    uint32_t hk[3];    // rounds R0+1..R0+3, whose h is still constant: h + K[i] (+ W[i] where W[i] is constant)
    uint32_t kw[64];   // W[i] constant: K[i] + W[i]; W[i] partly constant (i >= 16): the sum of its constant terms
    // Variant 10 (pow_h0_split, 108-byte header). W17 = kw[17] + v already; the rest of what it adds:
    uint32_t c24;      // W24 = c24 + v (kw[24] + kw[17])
    uint32_t he;       // round R0+1: e' = he + Sigma1(e) + Ch(e, f, g), he = st[2] + hk[0]
    uint32_t fxg, bxc; // round R0+1: Ch(e, f, g) = g ^ (e & fxg), Maj(a, b, c) = (b & c) ^ (a & bxc)
    // the hit predicate as one range check, (H0 - tword) < range_width unsigned, with H0 = mid[0] + a:
    // a + range_base < range_width. range_ok = 0: the mask is no prefix or the width no 32-bit number.
    uint32_t range_ok, range_base, range_width;
};
// What variant 11 adds to the job constants. An argument of its own kernels: PowJobDev keeps its size, and with it
// the other variants' kernels their code.
struct PowFillDev {
    uint32_t k17w;     // round 17: h + K[17] + W17 = h + (k17w + sv) + lanep, k17w = K[17] + kw[17]
    uint32_t c33;      // W33's first add: kw[33] + W17 = (c33 + sv) + lanep, c33 = kw[33] + kw[17]
    uint32_t k63r;     // round 63's K with the range check's base in it: the loop ends in a + range_base
};
__host__ __device__ __forceinline__ PowFillDev make_pow_fill(const PowJobDev& j) {
    return {kSha256K[17] + j.kw[17], j.kw[33] + j.kw[17], kSha256K[63] + j.range_base};
}

// Which words of the tail block's message schedule depend on the nonce (vec) and, of those, which also have
// nonce-independent terms (has_const). Shared by the host precomputation and the unrolled device loop.
struct PowWordKinds {
    bool vec[64];
    bool has_const[64];
};
constexpr PowWordKinds pow_word_kinds(int layout) {
    PowWordKinds k{};
    for (int i = 0; i < 16; ++i) k.vec[i] = layout == 2 ? i == 10 : (i == 1 || i == 2);
    for (int i = 16; i < 64; ++i) {
        const int src[4] = {i - 16, i - 15, i - 7, i - 2};
        bool v = false, c = false;
        for (int t = 0; t < 4; ++t) {
            if (k.vec[src[t]]) v = true; else c = true;
        }
        k.vec[i] = v;
        k.has_const[i] = v && c;
    }
    return k;
}

#define ROTR(x, n) __builtin_amdgcn_alignbit((x), (x), (n))
// gfx950 v_bitop3_b32: 3-input bitwise op from an 8-bit truth table. XOR3 (0x96) and MAJ (0xE8) are
// symmetric in their inputs, so the immediates do not depend on the operand->table-column order.
#define XOR3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)
#define BSIG0(x) XOR3(ROTR((x), 2), ROTR((x), 13), ROTR((x), 22))
#define BSIG1(x) XOR3(ROTR((x), 6), ROTR((x), 11), ROTR((x), 25))
#define SSIG0(x) XOR3(ROTR((x), 7), ROTR((x), 18), ((x) >> 3))
#define SSIG1(x) XOR3(ROTR((x), 17), ROTR((x), 19), ((x) >> 10))
#define CH(e, f, g) (((e) & (f)) | (~(e) & (g)))
#define MAJ(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0xE8)

__constant__ uint32_t dK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// H0 of SHA256(header) for the lane's nonce word `v`.
//  LAYOUT 2: v is W10 of the tail block (v = bswap(nonce_le)); rounds 0..9 precomputed.
//  LAYOUT 1: v is the little-endian nonce; W1 low half = n0,n1, W2 high half = n2,n3; round 0 precomputed.
template <int LAYOUT>
__device__ __forceinline__ uint32_t pow_h0(const PowJobDev& job, uint32_t v) {
    constexpr int R0 = LAYOUT == 2 ? 10 : 1;
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = job.w[i];
    if (LAYOUT == 2) {
        w[10] = v;
    } else {
        w[1] = job.w[1] | ((v & 0xffu) << 8) | ((v >> 8) & 0xffu);
        w[2] = job.w[2] | (((v >> 16) & 0xffu) << 24) | ((v >> 24) << 16);
    }
    uint32_t a = job.st[0], b = job.st[1], c = job.st[2], d = job.st[3];
    uint32_t e = job.st[4], f = job.st[5], g = job.st[6], h = job.st[7];
#pragma unroll
    for (int i = R0; i < 64; ++i) {
        uint32_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            wi = w[i & 15] + SSIG0(w[(i - 15) & 15]) + w[(i - 7) & 15] + SSIG1(w[(i - 2) & 15]);
            w[i & 15] = wi;
        }
        uint32_t t1 = h + BSIG1(e) + CH(e, f, g) + dK[i] + wi;
        uint32_t t2 = BSIG0(a) + MAJ(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    return job.mid[0] + a;
}

// The same H0 from the host-precomputed constants of PowJobDev: no lane-uniform value is computed (or kept in
// a VGPR) on the device, and K comes from the compile-time table. Compiled for the host too, where the
// tests check the precomputed constants against hashlib (pow_job_h0_host).
#if defined(__HIP_DEVICE_COMPILE__)
#define P_ROTR(x, n) ROTR(x, n)
#define P_XOR3(a, b, c) XOR3(a, b, c)
#define P_MAJ(a, b, c) MAJ(a, b, c)
#else
#define P_ROTR(x, n) host_rotr((x), (n))
#define P_XOR3(a, b, c) ((a) ^ (b) ^ (c))
#define P_MAJ(a, b, c) (((a) & (b)) ^ ((a) & (c)) ^ ((b) & (c)))
#endif
// Ch(e, f, g) as one v_bitop3_b32 whatever the operands (a second uniform operand costs a v_mov before the loop)
#if defined(__HIP_DEVICE_COMPILE__)
#define P_CH(e, f, g) __builtin_amdgcn_bitop3_b32((e), (f), (g), 0xCA)
#else
#define P_CH(e, f, g) CH(e, f, g)
#endif
#define P_BSIG0(x) P_XOR3(P_ROTR((x), 2), P_ROTR((x), 13), P_ROTR((x), 22))
#define P_BSIG1(x) P_XOR3(P_ROTR((x), 6), P_ROTR((x), 11), P_ROTR((x), 25))
#define P_SSIG0(x) P_XOR3(P_ROTR((x), 7), P_ROTR((x), 18), ((x) >> 3))
#define P_SSIG1(x) P_XOR3(P_ROTR((x), 17), P_ROTR((x), 19), ((x) >> 10))

template <int LAYOUT>
__host__ __device__ __forceinline__ uint32_t pow_h0_pre(const PowJobDev& job, uint32_t v) {
    constexpr int R0 = LAYOUT == 2 ? 10 : 1;
    constexpr PowWordKinds kinds = pow_word_kinds(LAYOUT);
    uint32_t w[16] = {};  // only the nonce-dependent words ever live here
    if (LAYOUT == 2) {
        w[10] = v;
    } else {
        w[1] = job.w[1] | ((v & 0xffu) << 8) | ((v >> 8) & 0xffu);
        w[2] = job.w[2] | (((v >> 16) & 0xffu) << 24) | ((v >> 24) << 16);
    }
    uint32_t a = job.ca + w[R0], b = job.st[0], c = job.st[1], d = job.st[2];
    uint32_t e = job.ce + w[R0], f = job.st[4], g = job.st[5], h = 0;
#pragma unroll
    for (int i = R0 + 1; i < 64; ++i) {
        uint32_t wi = 0;
        if (kinds.vec[i]) {
            if (i < 16) {
                wi = w[i];
            } else {
                if (kinds.has_const[i]) wi = job.kw[i];
                if (kinds.vec[i - 16]) wi += w[i & 15];
                if (kinds.vec[i - 15]) wi += P_SSIG0(w[(i - 15) & 15]);
                if (kinds.vec[i - 7]) wi += w[(i - 7) & 15];
                if (kinds.vec[i - 2]) wi += P_SSIG1(w[(i - 2) & 15]);
                w[i & 15] = wi;
            }
        }
        uint32_t x;  // h + K[i] + W[i]
        if (i <= R0 + 3) x = kinds.vec[i] ? job.hk[i - R0 - 1] + wi : job.hk[i - R0 - 1];
        else x = kinds.vec[i] ? h + kSha256K[i] + wi : h + job.kw[i];
        const uint32_t t1 = x + P_BSIG1(e) + CH(e, f, g);
        const uint32_t t2 = P_BSIG0(a) + P_MAJ(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    return job.mid[0] + a;
}

// pow_h0_pre<2> with the order of its instructions written out and pinned (variants 6..9): the same
// arithmetic on the same PowJobDev constants, instruction for instruction, so only the issue order differs.
//  D         schedule run-ahead: word W[i+D] is produced during round i, one of its (up to ten) instructions
//            after each of the round's first ten; D = 0 produces W[i] in one piece just before round i.
//  TWO_PATH  within a round the Sigma1/Ch/t1 path alternates with the Sigma0/Maj path and h + K + W, so that no
//            instruction follows its producer directly; otherwise the round runs path after path.
//  FILL      an s_sleep 0 in front of 1: every rotate, 2: every rotate and add3 (the two opcodes that issue at
//            4.1 cycles). It sleeps for no time and is handled by the sequencer, not the VALU; with it in front
//            the slow instruction costs about one cycle less (docs/PERF.md, "PoW issue order").
// The order is held by empty asm statements that emit nothing. The one after instruction n reads n's result,
// so n comes before it, and redefines ("+v") a VGPR input of instruction n+2, so n+2 comes after it; volatile
// asm statements keep their own order, and a sched_barrier after each keeps the machine scheduler from
// moving n+1 in front of it. (Redefining an input of n+1 itself is no option: the hazard pass puts an s_nop
// between an asm statement's VGPR result and an instruction that reads it at once.)
// Rounds R0+1..R0+3, whose state is still partly uniform, and the words that are due before the first pinned
// round produces them are left to the compiler.
struct PowSchedRegs {
    uint32_t w[16];  // the rolling window; only nonce-dependent words ever live here
    uint32_t s[8];   // a..h, rotating: in round i, a = s[-i & 7] .. h = s[(7 - i) & 7]
    uint32_t t[4], u[4], q[3];  // temporaries of the schedule word, the Sigma1/Ch path and the Sigma0/Maj path
    // SPLIT (variant 10) only: the sigmas of W10, W17 and W24 in two halves, wave-uniform low bits (xs, SGPRs) and
    // per-lane high bits (xl, VGPRs that do not change from iteration to iteration); sigma = xs ^ xl.
    //  0 sigma0(W10)   1 sigma1(W17)   2 sigma0(W17)   3 sigma1(W24)   4 sigma0(W24)
    uint32_t xs[5], xl[5];
    // G11 (variant 11) only: the K word (or scalar sum) that the coming h + K + W reads, loaded in the scalar slot
    // in front of it; lane << p; and the wave-uniform parts c24 + sv, kw[26] + sv, c33 + sv of the sums that take
    // the nonce word as (uniform part) + lanep
    uint32_t kx, lanep, us[3];
};
// Index into xs / xl of sigma0(W[j-15]) and of sigma1(W[j-2]), or -1 where the word is not split
constexpr int pow_split_s0(int j) { return j - 15 == 10 ? 0 : j - 15 == 17 ? 2 : j - 15 == 24 ? 4 : -1; }
constexpr int pow_split_s1(int j) { return j - 2 == 17 ? 1 : j - 2 == 24 ? 3 : -1; }
// What one instruction is pinned by: its VGPR inputs and its result (all null: the instruction does not exist)
struct PowOpRegs {
    uint32_t* in[3] = {nullptr, nullptr, nullptr};
    uint32_t* out = nullptr;
    __host__ __device__ __forceinline__ bool reads(const uint32_t* p) const {
        return p != nullptr && (in[0] == p || in[1] == p || in[2] == p);
    }
};

// Instruction k (0..9) of schedule word W[j]; instructions of terms that are nonce independent do not exist.
//  0-3 sigma0(W[j-15]) -> t[0]    4-7 sigma1(W[j-2]) -> t[1]    8 the first add of a four-term sum    9 W[j]
// split: a split word's sigma is one XOR, xs ^ xl, in the place of the XOR3 (k = 3 / 7); its rotates and shift go
// g11: W17 = kw[17] + v is not made; each of its readers takes (its own constant + sv) + lanep instead.
constexpr bool pow_sched_op_exists(const PowWordKinds& kinds, int j, int k, bool split = false, bool g11 = false) {
    if (j < 16 || j > 63 || !kinds.vec[j]) return false;
    if (g11 && j == 17) return false;
    if (k < 4) return kinds.vec[j - 15] && !(split && pow_split_s0(j) >= 0 && k < 3);
    if (k < 8) return kinds.vec[j - 2] && !(split && pow_split_s1(j) >= 0 && k < 7);
    const int n = int(kinds.has_const[j]) + int(kinds.vec[j - 16]) + int(kinds.vec[j - 15]) + int(kinds.vec[j - 7]) +
                  int(kinds.vec[j - 2]);
    return k == 9 || n == 4;
}

// RUN: execute the instruction; otherwise only name its registers
template <int LAYOUT, int J, int K, bool RUN, bool SPLIT = false, bool G11 = false>
__host__ __device__ __forceinline__ PowOpRegs pow_sched_op(const PowJobDev& job, PowSchedRegs& r) {
    constexpr PowWordKinds kinds = pow_word_kinds(LAYOUT);
    PowOpRegs o;
    if constexpr (G11 && ((J == 24 && K == 9) || (J == 26 && K == 8) || (J == 33 && K == 8))) {
        // W24 = c24 + v, and the first adds of W26 (kw[26] + W10) and W33 (kw[33] + W17): an SGPR plus lanep
        constexpr int n = J == 24 ? 0 : J == 26 ? 1 : 2;
        o = {{nullptr, nullptr, nullptr}, J == 24 ? &r.w[J & 15] : &r.t[2]};
        if (RUN) *o.out = r.us[n] + r.lanep;
    } else if constexpr (pow_sched_op_exists(kinds, J, K, SPLIT, G11)) {
        constexpr int j = J, k = K;
        constexpr bool c = kinds.has_const[j], v16 = kinds.vec[j - 16], v15 = kinds.vec[j - 15],
                       v7 = kinds.vec[j - 7], v2 = kinds.vec[j - 2];
        uint32_t(&w)[16] = r.w;
        uint32_t(&t)[4] = r.t;
        uint32_t& x15 = w[(j - 15) & 15];
        uint32_t& x2 = w[(j - 2) & 15];
        // a split sigma reads an SGPR and a VGPR that lives across iterations: neither is pinned (as w[10] is not)
        if constexpr (k < 4 && SPLIT && pow_split_s0(j) >= 0) {
            o = {{nullptr, nullptr, nullptr}, &t[0]};
            if (RUN) t[0] = r.xs[pow_split_s0(j)] ^ r.xl[pow_split_s0(j)];
        } else if constexpr (k >= 4 && k < 8 && SPLIT && pow_split_s1(j) >= 0) {
            o = {{nullptr, nullptr, nullptr}, &t[1]};
            if (RUN) t[1] = r.xs[pow_split_s1(j)] ^ r.xl[pow_split_s1(j)];
        } else if constexpr (k < 4) {
            if (k == 3) o = {{&t[2], &t[1], &t[0]}, &t[0]};
            else o = {{&x15, nullptr, nullptr}, &t[k]};
            if (RUN) *o.out = k == 0 ? P_ROTR(x15, 7) : k == 1 ? P_ROTR(x15, 18) : k == 2 ? x15 >> 3 : P_XOR3(t[0], t[1], t[2]);
        } else if constexpr (k < 8) {
            if (k == 7) o = {{&t[3], &t[2], &t[1]}, &t[1]};
            else o = {{&x2, nullptr, nullptr}, &t[k - 3]};
            if (RUN) *o.out = k == 4 ? P_ROTR(x2, 17) : k == 5 ? P_ROTR(x2, 19) : k == 6 ? x2 >> 10 : P_XOR3(t[1], t[2], t[3]);
        } else {
            constexpr int n = int(c) + int(v16) + int(v15) + int(v7) + int(v2);
            uint32_t* reg[7] = {};  // the sum's terms that are in VGPRs, in the order they are added
            int nr = 0;
            if (v16) reg[nr++] = &w[j & 15];
            if (v15) reg[nr++] = &t[0];
            if (v7) reg[nr++] = &w[(j - 7) & 15];
            if (v2) reg[nr++] = &t[1];
            // a four-term sum adds its first two terms (one may be the constant) first
            if (k == 8) o = {{reg[0], c ? nullptr : reg[1], nullptr}, &t[2]};
            else if (n == 4) o = {{&t[2], reg[nr - 1], reg[nr - 2]}, &w[j & 15]};
            else o = {{reg[nr - 1], nr > 1 ? reg[nr - 2] : nullptr, nr > 2 ? reg[nr - 3] : nullptr}, &w[j & 15]};
            if (RUN) {
                uint32_t term[5] = {};
                int m = 0;
                if (c) term[m++] = job.kw[j];
                if (v16) term[m++] = w[j & 15];
                if (v15) term[m++] = t[0];
                if (v7) term[m++] = w[(j - 7) & 15];
                if (v2) term[m++] = t[1];
                if (k == 8) t[2] = term[0] + term[1];
                else w[j & 15] = n == 4 ? t[2] + term[2] + term[3] : term[0] + term[1] + term[2];
            }
        }
    }
    return o;
}

// The fourteen instructions of compression round i. h + K[i] + W[i], then t1, then the next a take h's place;
// the next e takes d's.
enum PowRoundOp { R_X, R_R1, R_R2, R_R3, R_CH, R_S1, R_T1, R_E, R_Q1, R_Q2, R_Q3, R_S0, R_MJ, R_A };

// G11: K comes from r.kx; round 17 reads lanep for W17 (r.kx holds the rest); rounds 12 and 13 are pinned too, where
// h is still a job constant (folded into hk, no R_X) and c, d, g (round 12) and d (round 13) are as well: SGPR
// operands, which no fence names.
template <int LAYOUT, int I, int OP, bool RUN, bool G11 = false>
__host__ __device__ __forceinline__ PowOpRegs pow_round_op(const PowJobDev& job, PowSchedRegs& r) {
    constexpr PowWordKinds kinds = pow_word_kinds(LAYOUT);
    constexpr int i = I;
    constexpr bool early = G11 && i < 14;  // h uniform
    uint32_t(&s)[8] = r.s;
    uint32_t(&u)[4] = r.u;
    uint32_t(&q)[3] = r.q;
    uint32_t &a = s[(0 - i) & 7], &b = s[(1 - i) & 7], &c = s[(2 - i) & 7], &d = s[(3 - i) & 7];
    uint32_t &e = s[(4 - i) & 7], &f = s[(5 - i) & 7], &g = s[(6 - i) & 7], &h = s[(7 - i) & 7];
    PowOpRegs o;
    if constexpr (OP == R_X && G11) {
        if constexpr (!early) {
            o = {{&h, kinds.vec[i] && i != 17 ? &r.w[i & 15] : nullptr, nullptr}, &h};
            if (RUN) h = i == 17 ? h + r.kx + r.lanep : kinds.vec[i] ? h + r.kx + r.w[i & 15] : h + job.kw[i];
        }
    } else if constexpr (OP == R_X) {
        o = {{&h, kinds.vec[i] ? &r.w[i & 15] : nullptr, nullptr}, &h};
        if (RUN) h = kinds.vec[i] ? h + kSha256K[i] + r.w[i & 15] : h + job.kw[i];
    } else if constexpr (OP == R_R1) {
        o = {{&e, nullptr, nullptr}, &u[0]};
        if (RUN) u[0] = P_ROTR(e, 6);
    } else if constexpr (OP == R_R2) {
        o = {{&e, nullptr, nullptr}, &u[1]};
        if (RUN) u[1] = P_ROTR(e, 11);
    } else if constexpr (OP == R_R3) {
        o = {{&e, nullptr, nullptr}, &u[2]};
        if (RUN) u[2] = P_ROTR(e, 25);
    } else if constexpr (OP == R_CH) {
        o = {{&e, &f, G11 && i == 12 ? nullptr : &g}, &u[3]};
        if (RUN) u[3] = P_CH(e, f, g);
    } else if constexpr (OP == R_S1) {
        o = {{&u[2], &u[1], &u[0]}, &u[0]};
        if (RUN) u[0] = P_XOR3(u[0], u[1], u[2]);
    } else if constexpr (OP == R_T1) {
        o = {{&u[0], &u[3], early ? nullptr : &h}, &h};
        if (RUN) h = (early ? job.hk[(i - 11) % 3] : h) + u[0] + u[3];
    } else if constexpr (OP == R_E) {
        if constexpr (i != 63) {  // nothing reads the last e
            o = {{&h, early ? nullptr : &d, nullptr}, &d};
            if (RUN) d = d + h;
        }
    } else if constexpr (OP == R_Q1) {
        o = {{&a, nullptr, nullptr}, &q[0]};
        if (RUN) q[0] = P_ROTR(a, 2);
    } else if constexpr (OP == R_Q2) {
        o = {{&a, nullptr, nullptr}, &q[1]};
        if (RUN) q[1] = P_ROTR(a, 13);
    } else if constexpr (OP == R_Q3) {
        o = {{&a, nullptr, nullptr}, &q[2]};
        if (RUN) q[2] = P_ROTR(a, 22);
    } else if constexpr (OP == R_S0) {
        o = {{&q[2], &q[1], &q[0]}, &q[0]};
        if (RUN) q[0] = P_XOR3(q[0], q[1], q[2]);
    } else if constexpr (OP == R_MJ) {
        o = {{&a, &b, G11 && i == 12 ? nullptr : &c}, &q[1]};
        if (RUN) q[1] = P_MAJ(a, b, c);
    } else {
        o = {{&q[1], &q[0], &h}, &h};
        if (RUN) h = h + q[0] + q[1];
    }
    return o;
}

// f(integral_constant<int, B>) .. f(integral_constant<int, E - 1>) in order, unrolled by the front end
template <int B, class F, int... I>
__host__ __device__ __forceinline__ void pow_static_for(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, B + I>{}), ...);
}
template <int B, int E, class F>
__host__ __device__ __forceinline__ void pow_static_for(F&& f) {
    pow_static_for<B>(f, std::make_integer_sequence<int, (E > B ? E - B : 0)>{});
}

// G11 (variant 11): rounds 12 and 13 are pinned as well, K[i] is loaded by a scalar slot of its own (k_slot), and
// the first step of all has a filler in front of it too.
template <int LAYOUT, int D, bool TWO_PATH, bool SPLIT = false, bool G11 = false>
struct PowOrder {
    // first pinned round. R0 + 4 is the first round whose whole state is nonce dependent
    static constexpr int R0 = 10, FIRST = G11 ? R0 + 2 : R0 + 4;
    static constexpr bool kG11 = G11;
    static constexpr PowWordKinds kKinds = pow_word_kinds(LAYOUT);
    static constexpr int SLOTS = 24, STEPS = (64 - FIRST) * SLOTS;
    static constexpr int kOnePath[14] = {R_X, R_R1, R_R2, R_R3, R_CH, R_S1, R_T1, R_Q1, R_E, R_Q2, R_Q3, R_S0, R_MJ, R_A};
    static constexpr int kTwoPath[14] = {R_R1, R_Q1, R_R2, R_Q2, R_R3, R_Q3, R_CH, R_S1, R_X, R_S0, R_T1, R_MJ, R_E, R_A};
    // step g of the pinned part: slot g % 24 of round FIRST + g / 24
    static constexpr int round_of(int g) { return FIRST + g / SLOTS; }
    static constexpr bool is_sched(int g) {
        const int n = g % SLOTS;
        return D == 0 ? n < 10 : (n < 20 && (n & 1));
    }
    static constexpr int sched_k(int g) { return D == 0 ? g % SLOTS : (g % SLOTS) / 2; }
    static constexpr int round_op(int g) {
        const int n = g % SLOTS, k = D == 0 ? n - 10 : n < 20 ? n / 2 : n - 10;
        return TWO_PATH ? kTwoPath[k] : kOnePath[k];
    }
    static constexpr bool exists(int g) {
        if (g < 0 || g >= STEPS) return false;
        if (is_sched(g)) return pow_sched_op_exists(kKinds, round_of(g) + D, sched_k(g), SPLIT, G11);
        if (G11 && round_op(g) == R_X && round_of(g) < R0 + 4) return false;  // h is a constant, folded into hk
        return !(round_op(g) == R_E && round_of(g) == 63);
    }
    // An h + K[i] + W[i] that reads its K from PowSchedRegs::kx, and the step whose scalar slot loads that K: the
    // one before it (the round before's last add3), not its own, because an SGPR that an asm statement defines
    // costs an s_nop when the very next instruction reads it.
    static constexpr bool reads_kx(int g) {
        return G11 && exists(g) && !is_sched(g) && round_op(g) == R_X && kKinds.vec[round_of(g)];
    }
    static constexpr bool k_slot(int g) { return G11 && g >= 0 && exists(g) && slow(g) && reads_kx(next(g)); }
    // v_alignbit_b32 and v_add3_u32 issue at 4.1 cycles, everything else here at 2.3 (docs/PERF.md)
    static constexpr bool slow(int g) {
        if (!exists(g)) return false;
        const PowWordKinds& kinds = kKinds;
        if (is_sched(g)) {
            const int k = sched_k(g), j = round_of(g) + D;
            if (k < 8) return (k & 3) < 2;
            const int n = int(kinds.has_const[j]) + int(kinds.vec[j - 16]) + int(kinds.vec[j - 15]) +
                          int(kinds.vec[j - 7]) + int(kinds.vec[j - 2]);
            return k == 9 && n >= 3;
        }
        const int op = round_op(g);
        if (op == R_X) return kinds.vec[round_of(g)];
        return op == R_R1 || op == R_R2 || op == R_R3 || op == R_Q1 || op == R_Q2 || op == R_Q3 || op == R_T1 || op == R_A;
    }
    static constexpr bool rotate(int g) {
        if (!exists(g)) return false;
        if (is_sched(g)) return sched_k(g) < 8 && (sched_k(g) & 3) < 2;
        const int op = round_op(g);
        return op == R_R1 || op == R_R2 || op == R_R3 || op == R_Q1 || op == R_Q2 || op == R_Q3;
    }
    // FILL: an s_sleep 0, which does nothing and is no VALU instruction, goes in front of step g
    //  1 if g is a rotate    2 if g is slow (a rotate or an add3)
    static constexpr bool fill_before(int fill, int g) { return fill == 1 ? rotate(g) : fill == 2 ? slow(g) : false; }
    // Variant 10 puts one scalar instruction of its wave-uniform work into a filler's place: the first kUopsPerRound
    // fillers of a round (every round has its six rotates and two add3) are numbered on through the rounds. The
    // number of the filler in front of step g, or -1. The first step of all has no filler in front of it.
    static constexpr int kUopsPerRound = 8;
    static constexpr int uop_index(int fill, int g) {
        if (g < 0 || !fill_before(fill, g)) return -1;
        const int first = exists(0) ? 0 : next(0), begin = (g / SLOTS) * SLOTS;
        int local = 0;
        for (int h = begin; h < g; ++h)
            if (h != first && fill_before(fill, h)) ++local;
        return g != first && local < kUopsPerRound ? (g / SLOTS) * kUopsPerRound + local : -1;
    }
    static constexpr int next(int g) {  // the next step that has an instruction, or -1
        if (g < 0) return -1;
        for (int n = g + 1; n < STEPS; ++n)
            if (exists(n)) return n;
        return -1;
    }
    template <int G, bool RUN>
    static __host__ __device__ __forceinline__ PowOpRegs op(const PowJobDev& job, PowSchedRegs& r) {
        if constexpr (!exists(G)) return {};
        else if constexpr (is_sched(G)) return pow_sched_op<LAYOUT, round_of(G) + D, sched_k(G), RUN, SPLIT, G11>(job, r);
        else return pow_round_op<LAYOUT, round_of(G), round_op(G), RUN, G11>(job, r);
    }
};

// G11: the fillers that take a step of the scalar program are numbered without gaps, a round's first
// kUopsPerRound fillers that are no K slot and not in front of the first step (a round whose last add3 loads the
// next round's K can have fewer than that many left). at[g]: the number of the filler in front of step g, or -1;
// first[i]: the number of round i's first such filler.
template <class O>
struct PowUopTable {
    struct T { int at[O::STEPS]; int first[64]; };
    static constexpr T make() {
        T t{};
        const int first = O::exists(0) ? 0 : O::next(0);
        int n = 0, local = 0;
        for (int i = 0; i < 64; ++i) t.first[i] = -1;
        for (int g = 0; g < O::STEPS; ++g) {
            if (g % O::SLOTS == 0) local = 0;
            t.at[g] = -1;
            if (g == first || !O::fill_before(2, g) || O::k_slot(g)) continue;
            if (local++ < O::kUopsPerRound) {
                if (t.first[O::round_of(g)] < 0) t.first[O::round_of(g)] = n;
                t.at[g] = n++;
            }
        }
        return t;
    }
    static constexpr T k = make();
};
template <class O>
constexpr int pow_uop_index(int fill, int g) {
    if constexpr (O::kG11) return g >= 0 && fill == 2 ? PowUopTable<O>::k.at[g] : -1;
    else return O::uop_index(fill, g);
}
using PowFillOrder = PowOrder<2, 2, false, true, true>;

template <int LAYOUT, int FROM, int TO>
__host__ __device__ __forceinline__ void pow_sched_open_rounds(const PowJobDev& job, PowSchedRegs& r);
// The scalar program of a pinned loop: uop<N> is one SALU instruction that goes into filler N's place
struct PowNoScalar {
    static constexpr int kCount = 0;
    static constexpr bool has(int) { return false; }
    template <int N>
    __host__ __device__ __forceinline__ void uop(const PowJobDev&, PowSchedRegs&) {}
    template <int I>
    __host__ __device__ __forceinline__ uint32_t kx(const PowJobDev&) const { return kSha256K[I]; }
};
template <class O, int FILL, class S>
__host__ __device__ __forceinline__ void pow_sched_pinned(const PowJobDev& job, PowSchedRegs& r, S& sc);

template <int LAYOUT, int D, bool TWO_PATH, int FILL>
__host__ __device__ __forceinline__ uint32_t pow_h0_sched(const PowJobDev& job, uint32_t v) {
    static_assert(LAYOUT == 2, "the pinned order is written for the 108-byte header");
    static_assert(D >= 0 && D < 16, "W[i+D] takes the place of W[i+D-16], which round i must not need any more");
    using O = PowOrder<LAYOUT, D, TWO_PATH>;
    constexpr int R0 = O::R0, FIRST = O::FIRST;
    PowSchedRegs r = {};
    r.w[10] = v;
    {
        uint32_t(&s)[8] = r.s;
        constexpr int i = R0 + 1;
        s[(0 - i) & 7] = job.ca + v; s[(1 - i) & 7] = job.st[0]; s[(2 - i) & 7] = job.st[1]; s[(3 - i) & 7] = job.st[2];
        s[(4 - i) & 7] = job.ce + v; s[(5 - i) & 7] = job.st[4]; s[(6 - i) & 7] = job.st[5]; s[(7 - i) & 7] = 0;
    }
    pow_static_for<16, FIRST + D>([&](auto j) {
        pow_static_for<0, 10>([&](auto k) { pow_sched_op<LAYOUT, decltype(j)::value, decltype(k)::value, true>(job, r); });
    });
    constexpr PowWordKinds kinds = pow_word_kinds(LAYOUT);
#pragma unroll
    for (int i = R0 + 1; i < FIRST; ++i) {
        uint32_t(&s)[8] = r.s;
        uint32_t &a = s[(0 - i) & 7], &b = s[(1 - i) & 7], &c = s[(2 - i) & 7], &d = s[(3 - i) & 7];
        uint32_t &e = s[(4 - i) & 7], &f = s[(5 - i) & 7], &g = s[(6 - i) & 7], &h = s[(7 - i) & 7];
        const uint32_t x = kinds.vec[i] ? job.hk[i - R0 - 1] + r.w[i & 15] : job.hk[i - R0 - 1];
        uint32_t t1 = x + P_BSIG1(e) + P_CH(e, f, g);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(t1));  // one add3 here, then e and a from it, as in pow_h0_pre
#endif
        const uint32_t t2 = P_BSIG0(a) + P_MAJ(a, b, c);
        d = d + t1;
        h = t1 + t2;
    }
    PowNoScalar none;
    pow_sched_pinned<O, FILL>(job, r, none);
    return job.mid[0] + r.s[(0 - 64) & 7];
}

// Rounds FROM..TO-1 of the rounds whose state is still partly uniform, in the compiler's order: the loop of
// pow_h0_sched for variant 10. (pow_h0_sched keeps its own copy: called through this function the compiler orders
// variant 6-9's rounds 11..13 differently, and those kernels are kept instruction for instruction.)
template <int LAYOUT, int FROM, int TO>
__host__ __device__ __forceinline__ void pow_sched_open_rounds(const PowJobDev& job, PowSchedRegs& r) {
    constexpr int R0 = 10;
    constexpr PowWordKinds kinds = pow_word_kinds(LAYOUT);
#pragma unroll
    for (int i = FROM; i < TO; ++i) {
        uint32_t(&s)[8] = r.s;
        uint32_t &a = s[(0 - i) & 7], &b = s[(1 - i) & 7], &c = s[(2 - i) & 7], &d = s[(3 - i) & 7];
        uint32_t &e = s[(4 - i) & 7], &f = s[(5 - i) & 7], &g = s[(6 - i) & 7], &h = s[(7 - i) & 7];
        const uint32_t x = kinds.vec[i] ? job.hk[i - R0 - 1] + r.w[i & 15] : job.hk[i - R0 - 1];
        uint32_t t1 = x + P_BSIG1(e) + P_CH(e, f, g);
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(t1));  // one add3 here, then e and a from it, as in pow_h0_pre
#endif
        const uint32_t t2 = P_BSIG0(a) + P_MAJ(a, b, c);
        d = d + t1;
        h = t1 + t2;
    }
}

// The pinned part: every step of order O from round O::FIRST on, FILL as above. Where the scalar program sc has
// an instruction for a filler's place it goes there and the s_sleep 0 does not: a scalar instruction in front of a
// slow one does what the filler does (docs/PERF.md, "PoW lane/uniform split").
template <class O, int FILL, class S>
__host__ __device__ __forceinline__ void pow_sched_pinned(const PowJobDev& job, PowSchedRegs& r, S& sc) {
    if constexpr (O::FIRST < O::R0 + 4) {  // G11: the first step's filler
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (O::fill_before(FILL, O::exists(0) ? 0 : O::next(0))) __builtin_amdgcn_s_sleep(0);
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
    pow_static_for<0, O::STEPS>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (O::exists(g)) {
            const PowOpRegs me = O::template op<g, true>(job, r);
            constexpr int g1 = O::next(g), g2 = O::next(g1);
            constexpr int uop = S::kCount > 0 ? pow_uop_index<O>(FILL, g1) : -1;
            constexpr bool kslot = g1 >= 0 && O::k_slot(g1);
#if defined(__HIP_DEVICE_COMPILE__)
            const PowOpRegs n1 = O::template op<g1, false>(job, r), n2 = O::template op<g2, false>(job, r);
            // An asm result must not be read by the very next instruction (s_nop), and the nonce word is live
            // across iterations (redefining it would cost a copy). Redefining this instruction's own result as
            // well keeps the optimiser from re-associating sums across the pinned instructions.
            uint32_t* nin = n2.in[0];
            if (nin == n1.out || n1.reads(nin) || nin == &r.w[10]) nin = nullptr;
            uint32_t* own = n1.reads(me.out) ? nullptr : me.out;
            if (nin != nullptr && own != nullptr && nin != own) asm volatile("" : "+v"(*nin), "+v"(*own));
            else if (own != nullptr) asm volatile("" : "+v"(*own));
            else if (nin != nullptr) asm volatile("" : "+v"(*nin) : "v"(*me.out));
            else asm volatile("" ::"v"(*me.out));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (O::fill_before(FILL, g1)) {
                if constexpr (kslot) {
                    // K, or the scalar sum that stands for K and W's uniform part, of the h + K + W after g1: one
                    // SALU instruction in the filler's place
                    uint32_t k = sc.template kx<O::round_of(kslot ? O::next(g1) : 0)>(job);
                    asm volatile("" : "+s"(k));
                    r.kx = k;
                } else if constexpr (uop >= 0 && S::has(uop)) sc.template uop<uop>(job, r);
                else __builtin_amdgcn_s_sleep(0);
                __builtin_amdgcn_sched_barrier(0);
            }
#else
            (void)me;
            (void)g2;
            if constexpr (kslot) r.kx = sc.template kx<O::round_of(kslot ? O::next(g1) : 0)>(job);
            else if constexpr (uop >= 0 && S::has(uop)) sc.template uop<uop>(job, r);
#endif
        }
    });
}

// Variant 10: the lane index in the nonce word's top bits, wave-uniform work on the SALU.
// A piece of the search is v = vb + U + (lane << p), U in [0, 2^p) the same for all 64 lanes of a wave. The
// nonce word enters the tail block additively five times: W10 = v itself, a11 = ca + v, e11 = ce + v,
// W17 = kw[17] + v and W24 = c24 + v. Each is x = s + (lane << p) with a wave-uniform s = c + vb + U, so
//   x = lo | hi,   lo = s & (2^p - 1) wave-uniform,   hi = ((s >> p) + lane) << p,
// and hi changes only when s >> p does, once per piece as U grows (the carry out of bit p-1). The sigmas are
// GF(2)-linear and Ch / Maj with uniform second and third operands bitwise, and lo and hi have no bit in common:
//   sigma(x) = sigma(lo) ^ sigma(hi),   Ch(x, f, g) = (Ch(lo, f, g) & (2^p - 1)) + (Ch(hi, f, g) & ~(2^p - 1)).
// The lo halves are plain C++ on uniform values (SALU); the hi halves are per-lane constants in VGPRs, recomputed
// in a wave-uniform branch when their s >> p differs from the cached one. That takes the rotates of
// sigma0(W10), sigma0/1(W17), sigma0/1(W24) and of round 11 out of the loop; every other instruction is
// variant 9's, in its order and with its fillers.
struct PowSplitKeys { uint32_t v, e, a, w17, w24; };  // the five sums, or their s >> p
struct PowSplitLane {
    uint32_t lanep;           // lane << p
    uint32_t xl[5];           // PowSchedRegs::xl
    uint32_t s1, ch, s0, cm;  // round 11: Sigma1(e_hi), Ch(e_hi, f, g), Sigma0(a_hi), Ch(e_hi, f, g) + Maj(a_hi, b, c)
};
// Rotates of a wave-uniform value x on the SALU, which has no rotate: x twice in an SGPR pair, and a 64-bit right
// shift by n leaves rotr(x, n) in the low word.
#define U_PAIR(x) ((uint64_t(x) << 32) | (x))
#define U_ROTR(xx, n) uint32_t((xx) >> (n))
__host__ __device__ __forceinline__ uint32_t pow_u_bsig0(uint32_t x) { const uint64_t xx = U_PAIR(x); return U_ROTR(xx, 2) ^ U_ROTR(xx, 13) ^ U_ROTR(xx, 22); }
__host__ __device__ __forceinline__ uint32_t pow_u_bsig1(uint32_t x) { const uint64_t xx = U_PAIR(x); return U_ROTR(xx, 6) ^ U_ROTR(xx, 11) ^ U_ROTR(xx, 25); }

// The wave-uniform program, one SALU instruction per step (uop<N>), each in the place of one filler of the pinned
// loop (PowOrder::uop_index). Steps 0..32 make this iteration's xs (the first is needed in round 17, the steps
// run in rounds 14..18); steps 33..56 make round 11's scalars of the NEXT iteration, sv + 1, which the top of the
// loop then only reads. On the device every step sits between two empty asm statements that redefine the
// program's registers: they hold the step's place among the pinned instructions, keep the values in SGPRs and
// hide from the compiler that a shift pair is a rotate, which it would select as v_alignbit_b32, back on the VALU.
// G11 (variant 11): the pinned part starts two rounds earlier, so the steps run from round 12 on; steps 34 and 45
// keep the next iteration's ce + sv and ca + sv (es, as: a11 and e11 are these plus lanep); three more steps make
// the uniform parts of W24 and of the first adds of W26 and W33 (PowSchedRegs::us) at the head of the round that
// reads them; and kx<I> is the SALU instruction in front of round I's h + K + W.
template <bool G11>
struct PowSplitScalarT {
    // G11: the first slots of rounds 22, 24 and 31, in which W24, W26 and W33 are made
    static constexpr int kW24 = G11 ? PowUopTable<PowFillOrder>::k.first[22] : 57;
    static constexpr int kW26 = G11 ? PowUopTable<PowFillOrder>::k.first[24] : 58;
    static constexpr int kW33 = G11 ? PowUopTable<PowFillOrder>::k.first[31] : 59;
    static_assert(kW24 >= 57 && kW26 > kW24 && kW33 > kW26, "after the sigma halves and the next round 11");
    static constexpr int kCount = G11 ? kW33 + 1 : 57;
    static constexpr bool has(int n) { return n < 57 || (G11 && (n == kW24 || n == kW26 || n == kW33)); }
    uint32_t es, as;         // G11: ce + sv and ca + sv of the coming iteration
    uint32_t k63;            // G11: round 63's K; the range-form kernel has the range check's base in it
    uint32_t k17w, c33;      // G11: PowFillDev's
    uint32_t sv;             // this iteration's vb + U
    uint32_t m, glo, bclo;   // 2^p - 1, g & m, b & c & m (round 11's g, b, c)
    uint32_t x1, x0, se, sa; // round 11: Sigma1(e_lo), Sigma0(a_lo), he + Ch_lo, hk[0] + Ch_lo + Maj_lo
    uint32_t a, b, t, l;     // temporaries
    uint64_t pp;

    // Round 11's scalars for the word sum at `at`, all at once (the prologue; the steps below do the same)
    __host__ __device__ __forceinline__ void round11(const PowJobDev& job, uint32_t at) {
        const uint32_t elo = (at + job.ce) & m, alo = (at + job.ca) & m;
        const uint32_t chlo = (elo & job.fxg) ^ glo, mjlo = (alo & job.bxc) ^ bclo;
        x1 = pow_u_bsig1(elo);
        x0 = pow_u_bsig0(alo);
        se = chlo + job.he;
        sa = chlo + mjlo + job.hk[0];
        if (G11) {
            es = at + job.ce;
            as = at + job.ca;
        }
    }

    template <int I>
    __host__ __device__ __forceinline__ uint32_t kx(const PowJobDev& job) const {
        if constexpr (I == 17) return sv + k17w;
        else if constexpr (I == 63) return k63;
        else return kSha256K[I];
    }

    template <int N>
    __host__ __device__ __forceinline__ void uop(const PowJobDev& job, PowSchedRegs& r) {
        static_assert(N >= 0 && N < kCount && has(N), "no such step");
        uint32_t(&xs)[5] = r.xs;
        if constexpr (N >= 57) {  // on their own: one SGPR each, made where it is read
            constexpr int n = N == kW24 ? 0 : N == kW26 ? 1 : 2;
            r.us[n] = sv + (n == 0 ? job.c24 : n == 1 ? job.kw[26] : c33);
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(r.us[n]));
#endif
            return;
        }
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(a), "+s"(b), "+s"(t), "+s"(l), "+s"(pp), "+s"(sv));
#endif
        // sigma1, sigma0 of the pair pp / the word l into xs[K1], xs[K0]: ten steps from FIRST on
#define U_SIG1(FIRST, K1)                                                                                      \
        else if constexpr (N == FIRST) a = U_ROTR(pp, 17); else if constexpr (N == FIRST + 1) b = U_ROTR(pp, 19); \
        else if constexpr (N == FIRST + 2) a ^= b; else if constexpr (N == FIRST + 3) b = l >> 10;                \
        else if constexpr (N == FIRST + 4) xs[K1] = a ^ b;
#define U_SIG0(FIRST, K0)                                                                                      \
        else if constexpr (N == FIRST) a = U_ROTR(pp, 7); else if constexpr (N == FIRST + 1) b = U_ROTR(pp, 18); \
        else if constexpr (N == FIRST + 2) a ^= b; else if constexpr (N == FIRST + 3) b = l >> 3;                \
        else if constexpr (N == FIRST + 4) xs[K0] = a ^ b;
        if constexpr (N == 0) l = sv + job.kw[17];
        else if constexpr (N == 1) l &= m;
        else if constexpr (N == 2) pp = U_PAIR(l);
        U_SIG1(3, 1)
        U_SIG0(8, 2)
        else if constexpr (N == 13) l = sv & m;
        else if constexpr (N == 14) pp = U_PAIR(l);
        U_SIG0(15, 0)
        else if constexpr (N == 20) l = sv + job.c24;
        else if constexpr (N == 21) l &= m;
        else if constexpr (N == 22) pp = U_PAIR(l);
        U_SIG1(23, 3)
        U_SIG0(28, 4)
        // the next iteration's round 11
        else if constexpr (N == 33) t = sv + 1u;
        else if constexpr (N == 34 && G11) es = t + job.ce;
        else if constexpr (N == 35 && G11) l = es & m;
        else if constexpr (N == 34) l = t + job.ce;
        else if constexpr (N == 35) l &= m;
        else if constexpr (N == 36) pp = U_PAIR(l);
        else if constexpr (N == 37) a = U_ROTR(pp, 6);
        else if constexpr (N == 38) b = U_ROTR(pp, 11);
        else if constexpr (N == 39) a ^= b;
        else if constexpr (N == 40) b = U_ROTR(pp, 25);
        else if constexpr (N == 41) x1 = a ^ b;
        else if constexpr (N == 42) a = l & job.fxg;
        else if constexpr (N == 43) a ^= glo;  // Ch_lo
        else if constexpr (N == 44) se = a + job.he;
        else if constexpr (N == 45 && G11) as = t + job.ca;
        else if constexpr (N == 46 && G11) l = as & m;
        else if constexpr (N == 45) l = t + job.ca;
        else if constexpr (N == 46) l &= m;
        else if constexpr (N == 47) pp = U_PAIR(l);
        else if constexpr (N == 48) b = U_ROTR(pp, 2);
        else if constexpr (N == 49) t = U_ROTR(pp, 13);
        else if constexpr (N == 50) b ^= t;
        else if constexpr (N == 51) t = U_ROTR(pp, 22);
        else if constexpr (N == 52) x0 = b ^ t;
        else if constexpr (N == 53) b = l & job.bxc;
        else if constexpr (N == 54) b ^= bclo;  // Maj_lo
        else if constexpr (N == 55) a += b;
        else if constexpr (N == 56) sa = a + job.hk[0];
#undef U_SIG1
#undef U_SIG0
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (G11) {
            // only what the step wrote: an xs that is not made yet stays out of the SGPRs
            asm volatile("" : "+s"(a), "+s"(b), "+s"(t), "+s"(l), "+s"(pp), "+s"(x1), "+s"(x0), "+s"(se), "+s"(sa));
            constexpr int k = N == 7 ? 1 : N == 12 ? 2 : N == 19 ? 0 : N == 27 ? 3 : N == 32 ? 4 : -1;
            if constexpr (k >= 0) asm volatile("" : "+s"(xs[k]));
            if constexpr (N == 34) asm volatile("" : "+s"(es));
            if constexpr (N == 45) asm volatile("" : "+s"(as));
        } else {
            asm volatile("" : "+s"(a), "+s"(b), "+s"(t), "+s"(l), "+s"(pp), "+s"(x1), "+s"(x0), "+s"(se), "+s"(sa),
                              "+s"(xs[0]), "+s"(xs[1]), "+s"(xs[2]), "+s"(xs[3]), "+s"(xs[4]));
        }
#endif
    }
};
using PowSplitScalar = PowSplitScalarT<false>;
template <bool G11>
struct PowSplitCacheT {
    PowSplitKeys key;   // s >> p of the five sums, which the lane constants were computed from
    uint32_t next;      // the first vb + U at which one of them is another
    PowSplitScalarT<G11> sc;  // the scalar program's registers; x1, x0, se, sa are those of the coming iteration
};
using PowSplitCache = PowSplitCacheT<false>;

// sv = vb + U
__host__ __device__ __forceinline__ PowSplitKeys pow_split_sums(const PowJobDev& job, uint32_t sv) {
    return {sv, job.ce + sv, job.ca + sv, job.kw[17] + sv, job.c24 + sv};
}

// At sv: the lane constants whose key differs from the cached one (all: every one, for the prologue), and the next
// sv at which a key changes. A sum's s >> p changes when its low p bits wrap, so the first of the five to do so is
// the one with the largest low part: 2^p minus that many steps from here.
template <class Cache>
__host__ __device__ __forceinline__ void pow_split_lane_update(const PowJobDev& job, uint32_t p, uint32_t sv, uint32_t lane,
                                                               Cache& cached, PowSplitLane& lc, bool all) {
    const uint32_t m = (1u << p) - 1u, hm = ~m;
    const PowSplitKeys s = pow_split_sums(job, sv);
    const PowSplitKeys key = {s.v >> p, s.e >> p, s.a >> p, s.w17 >> p, s.w24 >> p};
    if (all || key.v != cached.key.v) {
        const uint32_t x = (key.v + lane) << p;
        lc.xl[0] = P_SSIG0(x);
    }
    if (all || key.w17 != cached.key.w17) {
        const uint32_t x = (key.w17 + lane) << p;
        lc.xl[1] = P_SSIG1(x);
        lc.xl[2] = P_SSIG0(x);
    }
    if (all || key.w24 != cached.key.w24) {
        const uint32_t x = (key.w24 + lane) << p;
        lc.xl[3] = P_SSIG1(x);
        lc.xl[4] = P_SSIG0(x);
    }
    if (all || key.e != cached.key.e || key.a != cached.key.a) {
        const uint32_t eh = (key.e + lane) << p, ah = (key.a + lane) << p;
        lc.s1 = P_BSIG1(eh);
        lc.ch = CH(eh, job.st[4], job.st[5]) & hm;
        lc.s0 = P_BSIG0(ah);
        lc.cm = lc.ch + (P_MAJ(ah, job.st[0], job.st[1]) & hm);
    }
    cached.key = key;
    uint32_t top = s.v & m;
    top = (s.e & m) > top ? (s.e & m) : top;
    top = (s.a & m) > top ? (s.a & m) : top;
    top = (s.w17 & m) > top ? (s.w17 & m) : top;
    top = (s.w24 & m) > top ? (s.w24 & m) : top;
    cached.next = sv + (m - top) + 1u;
}

// Before a wave's first iteration, whose sv is vb + U
template <class Cache>
__host__ __device__ __forceinline__ void pow_split_prologue(const PowJobDev& job, uint32_t p, uint32_t sv, uint32_t lane,
                                                            Cache& cached, PowSplitLane& lc) {
    lc.lanep = lane << p;
    pow_split_lane_update(job, p, sv, lane, cached, lc, true);
    auto& sc = cached.sc;
    sc = {};
    sc.m = (1u << p) - 1u;
    sc.glo = job.st[5] & sc.m;
    sc.bclo = job.st[0] & job.st[1] & sc.m;
    sc.round11(job, sv);
}

// a after round 63 (H0 = mid[0] + a) for the lane's nonce word sv + (lane << p); p <= 26. sv goes up by one from
// call to call after the prologue: the keys can only change at cached.next, and round 11's scalars for this sv
// were made during the call before.
template <int FILL>
__host__ __device__ __forceinline__ uint32_t pow_a_split(const PowJobDev& job, uint32_t p, uint32_t sv, uint32_t lane,
                                                         PowSplitCache& cached, PowSplitLane& lc) {
    using O = PowOrder<2, 2, false, true>;
    static_assert(PowSplitScalar::kCount <= (64 - O::FIRST) * O::kUopsPerRound, "a filler's place for every step");
    if (sv == cached.next) pow_split_lane_update(job, p, sv, lane, cached, lc, false);
    PowSplitScalar& sc = cached.sc;
    sc.sv = sv;
    PowSchedRegs r = {};
#pragma unroll
    for (int k = 0; k < 5; ++k) r.xl[k] = lc.xl[k];
    const uint32_t v = sv + lc.lanep;
    r.w[10] = v;
    {
        // round 11 from the halves; b, c, f, g are still job constants
        const uint32_t x1 = sc.x1 ^ lc.s1, x0 = sc.x0 ^ lc.s0;
        uint32_t(&s)[8] = r.s;
        constexpr int i = O::R0 + 1;
        s[(0 - i) & 7] = job.ca + v; s[(1 - i) & 7] = job.st[0]; s[(2 - i) & 7] = job.st[1];
        s[(4 - i) & 7] = job.ce + v; s[(5 - i) & 7] = job.st[4]; s[(6 - i) & 7] = job.st[5];
        s[(3 - i) & 7] = x1 + lc.ch + sc.se;           // e12 = d + t1
        s[(7 - i) & 7] = (x1 + x0 + lc.cm) + sc.sa;  // a12 = t1 + t2
    }
    pow_sched_open_rounds<2, O::R0 + 2, O::FIRST>(job, r);
    pow_sched_pinned<O, FILL>(job, r, sc);
    return r.s[(0 - 64) & 7];
}

// Variant 11: variant 10 with one scalar or sequencer instruction in front of every rotate and add3 and nothing else
// between VALU instructions. Rounds 12 and 13 are pinned too; each K is loaded in the slot in front of its own
// h + K + W and is dead after it; the nonce word and W17 are not materialised (their readers take an SGPR sum plus
// lanep). Returns a after round 63; range: a + range_base, which round 63 adds with its K.
template <int FILL>
__host__ __device__ __forceinline__ uint32_t pow_a_fill(const PowJobDev& job, uint32_t p, uint32_t sv, uint32_t lane,
                                                        PowSplitCacheT<true>& cached, PowSplitLane& lc,
                                                        const PowFillDev& fx, bool range) {
    using O = PowFillOrder;
    using S = PowSplitScalarT<true>;
    static_assert(PowUopTable<O>::k.first[63] + O::kUopsPerRound > S::kCount, "a filler's place for every step");
    if (sv == cached.next) {
        pow_split_lane_update(job, p, sv, lane, cached, lc, false);
#if defined(__HIP_DEVICE_COMPILE__)
        // the maximum of the five low parts comes from v_max3_u32: back to an SGPR here, off the hot path, so that
        // the test above is a scalar compare
        cached.next = __builtin_amdgcn_readfirstlane(cached.next);
#endif
    }
    S& sc = cached.sc;
    sc.sv = sv;
    sc.k63 = range ? fx.k63r : kSha256K[63];
    sc.k17w = fx.k17w;
    sc.c33 = fx.c33;
    PowSchedRegs r = {};
#pragma unroll
    for (int k = 0; k < 5; ++k) r.xl[k] = lc.xl[k];
    r.lanep = lc.lanep;
    {
        // round 11 from the halves, as in pow_a_split; a11 and e11 from the sums the last iteration left
        const uint32_t x1 = sc.x1 ^ lc.s1, x0 = sc.x0 ^ lc.s0;
        uint32_t(&s)[8] = r.s;
        constexpr int i = O::R0 + 1;
        s[(0 - i) & 7] = sc.as + lc.lanep; s[(1 - i) & 7] = job.st[0]; s[(2 - i) & 7] = job.st[1];
        s[(4 - i) & 7] = sc.es + lc.lanep; s[(5 - i) & 7] = job.st[4]; s[(6 - i) & 7] = job.st[5];
        s[(3 - i) & 7] = x1 + lc.ch + sc.se;           // e12 = d + t1
        s[(7 - i) & 7] = (x1 + x0 + lc.cm) + sc.sa;  // a12 = t1 + t2
    }
    pow_sched_pinned<O, FILL>(job, r, sc);
    return r.s[(0 - 64) & 7];
}

// One nonce word through the split function (the tests' H0 of variants 10 and 11): the word as lane << 26 | U
template <bool G11 = false>
__host__ __device__ __forceinline__ uint32_t pow_h0_split(const PowJobDev& job, uint32_t v) {
    const uint32_t p = 26, lane = v >> p, sv = v & ((1u << p) - 1u);
    PowSplitCacheT<G11> cached;
    PowSplitLane lc;
    pow_split_prologue(job, p, sv, lane, cached, lc);
    if constexpr (G11) return job.mid[0] + pow_a_fill<2>(job, p, sv, lane, cached, lc, make_pow_fill(job), false);
    else return job.mid[0] + pow_a_split<2>(job, p, sv, lane, cached, lc);
}


// Variant 2 (A/B evidence for the design note above): the same v2 search with the expanded message
// schedule W16..W63 staged in LDS instead of VGPRs. Each lane owns a 16-word ring in LDS laid out
// [word][lane] (consecutive lanes -> consecutive banks, conflict-free); every produced word is one
// ds_write_b32 and each of its four consumers one ds_read_b32. `volatile` keeps the compiler from
// forwarding the stores back into registers, so this really is the LDS-staged form.
typedef __attribute__((address_space(3))) volatile uint32_t lds_u32;

__device__ __forceinline__ uint32_t pow_h0_lds(const PowJobDev& job, uint32_t v, lds_u32* ring) {
    const uint32_t tid = threadIdx.x;
    // words 0..15 are job constants (SGPRs) or the nonce word; only W16..W63 live in LDS
    auto W = [&](int i) -> uint32_t { return i < 16 ? (i == 10 ? v : job.w[i]) : ring[(i & 15) * 256 + tid]; };
    uint32_t a = job.st[0], b = job.st[1], c = job.st[2], d = job.st[3];
    uint32_t e = job.st[4], f = job.st[5], g = job.st[6], h = job.st[7];
#pragma unroll
    for (int i = 10; i < 64; ++i) {
        uint32_t wi;
        if (i < 16) {
            wi = W(i);
        } else {
            wi = W(i - 16) + SSIG0(W(i - 15)) + W(i - 7) + SSIG1(W(i - 2));
            ring[(i & 15) * 256 + tid] = wi;
        }
        uint32_t t1 = h + BSIG1(e) + CH(e, f, g) + dK[i] + wi;
        uint32_t t2 = BSIG0(a) + MAJ(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    return job.mid[0] + a;
}

__global__ __launch_bounds__(256, 1) void pow_search_lds_kernel(PowJobDev job, uint32_t v_base, uint32_t iters,
                                                                uint32_t* __restrict__ out_count,
                                                                uint32_t* __restrict__ out_words, uint32_t cap) {
    __shared__ uint32_t ring[16 * 256];
    const uint32_t nthreads = gridDim.x * blockDim.x;
    uint32_t v = v_base + blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t it = 0; it < iters; ++it, v += nthreads) {
        const uint32_t h0 = pow_h0_lds(job, v, (lds_u32*)ring);
        const bool hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        if (__builtin_expect(hit, 0)) {
            const uint32_t slot = atomicAdd(out_count, 1u);
            if (slot < cap) out_words[slot] = v;
        }
    }
}

template <int LAYOUT, int MIN_WAVES_PER_SIMD>
__global__ __launch_bounds__(256, MIN_WAVES_PER_SIMD) void pow_search_kernel(PowJobDev job, uint32_t v_base, uint32_t iters,
                                                         uint32_t* __restrict__ out_count,
                                                         uint32_t* __restrict__ out_words, uint32_t cap) {
    const uint32_t nthreads = gridDim.x * blockDim.x;
    uint32_t v = v_base + blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t it = 0; it < iters; ++it, v += nthreads) {
        const uint32_t h0 = pow_h0<LAYOUT>(job, v);
        const bool hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        if (__builtin_expect(hit, 0)) {
            const uint32_t slot = atomicAdd(out_count, 1u);
            if (slot < cap) out_words[slot] = v;
        }
    }
}

template <int LAYOUT, int MIN_WAVES_PER_SIMD>
__global__ __launch_bounds__(256, MIN_WAVES_PER_SIMD) void pow_search_pre_kernel(PowJobDev job, uint32_t v_base, uint32_t iters,
                                                             uint32_t* __restrict__ out_count,
                                                             uint32_t* __restrict__ out_words, uint32_t cap) {
    const uint32_t nthreads = gridDim.x * blockDim.x;
    uint32_t v = v_base + blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t it = 0; it < iters; ++it, v += nthreads) {
        const uint32_t h0 = pow_h0_pre<LAYOUT>(job, v);
        const bool hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        if (__builtin_expect(hit, 0)) {
            const uint32_t slot = atomicAdd(out_count, 1u);
            if (slot < cap) out_words[slot] = v;
        }
    }
}

template <int D, bool TWO_PATH, int FILL, int MIN_WAVES_PER_SIMD>
__global__ __launch_bounds__(256, MIN_WAVES_PER_SIMD) void pow_search_sched_kernel(PowJobDev job, uint32_t v_base, uint32_t iters,
                                                               uint32_t* __restrict__ out_count,
                                                               uint32_t* __restrict__ out_words, uint32_t cap) {
    const uint32_t nthreads = gridDim.x * blockDim.x;
    uint32_t v = v_base + blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t it = 0; it < iters; ++it, v += nthreads) {
        const uint32_t h0 = pow_h0_sched<2, D, TWO_PATH, FILL>(job, v);
        const bool hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        if (__builtin_expect(hit, 0)) {
            const uint32_t slot = atomicAdd(out_count, 1u);
            if (slot < cap) out_words[slot] = v;
        }
    }
}

// Variant 10. One dispatch covers U in [u_begin, u_end) of the piece v = vb + U + (lane << p): wave w of the grid
// (four per block) takes the `iters` values from u_begin + w * iters on, cut at u_end. The host keeps
// (waves + 3) * iters below 2^32. RANGE: the job's hit predicate is the one range check (PowJobDev::range_ok).
// Variant 11, the same dispatch as variant 10 (pow_search_split_kernel below). RANGE: round 63's K carries
// range_base, so the loop ends in the compare; a wave with no hit takes one branch over the cold block.
// __launch_bounds__(256, 7): the compiler's SGPR budget for 8 waves/SIMD is 80 and makes it spill to VGPR lanes and
// reload in the loop; for 7 it is 96, of which the kernel takes 90, and with those and its 43 VGPRs it still runs
// 8 waves/SIMD.
template <bool RANGE>
__global__ __launch_bounds__(256, 7) void pow_search_fill_kernel(PowJobDev job, uint32_t vb, uint32_t p, uint32_t u_begin,
                                                                 uint32_t u_end, uint32_t iters,
                                                                 uint32_t* __restrict__ out_count,
                                                                 uint32_t* __restrict__ out_words, uint32_t cap,
                                                                 PowFillDev fx) {
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t u = u_begin + wave * iters;
    if (u >= u_end) return;
    const uint32_t u_stop = u_end - u < iters ? u_end : u + iters;
    PowSplitCacheT<true> cached;
    PowSplitLane lc;
    pow_split_prologue(job, p, vb + u, lane, cached, lc);
    cached.next = __builtin_amdgcn_readfirstlane(cached.next);  // see pow_a_fill
    for (; u < u_stop; ++u) {
        const uint32_t sv = vb + u;
        const uint32_t a = pow_a_fill<2>(job, p, sv, lane, cached, lc, fx, RANGE);
        bool hit;
        if (RANGE) {
            hit = a < job.range_width;
        } else {
            const uint32_t h0 = job.mid[0] + a;
            hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        }
#if defined(__HIP_DEVICE_COMPILE__)
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit) != 0, 0)) {
            if (hit) {
                const uint32_t slot = atomicAdd(out_count, 1u);
                if (slot < cap) out_words[slot] = sv + lc.lanep;
            }
        }
#endif
    }
}

// Variant 12: variant 11's loop under a claiming wave loop. A dispatch covers the same [u_begin, u_end) as variant
// 11's, but no wave has a fixed share of it: a wave takes `claim` values of U from *counter (zero when the dispatch
// starts), runs them and takes the next, until the range is used up, so the eight waves of a SIMD stay live until the
// pool is empty and not until the oldest of them has done its share (docs/PERF.md, "PoW claimed chunks"). Waves of
// a block claim independently: no LDS, no barrier. The host keeps (waves + 1) * claim + (u_end - u_begin) below
// 2^32, so the counter does not wrap before every wave has seen it past the range. `iters` is the share a wave
// would have had: the host sizes the grid by it; the kernel does not read it.
// The arguments that only the claim reads (u_begin, u_end, claim, counter) are loaded from the kernel argument
// segment at each claim, through a pointer that an asm statement redefines so that the loads stay where they are
// written: held in SGPRs across the hot loop they do not fit next to the 90 it takes, and the compiler spills them
// to VGPR lanes. PowClaimKernArgs is the kernel's argument list as a struct, which has the segment's layout.
struct PowClaimKernArgs {
    PowJobDev job;
    uint32_t vb, p, u_begin, u_end, iters;
    uint32_t *out_count, *out_words;
    uint32_t cap;
    PowFillDev fx;
    uint32_t claim;
    uint32_t* counter;
};
template <bool RANGE>
__global__ __launch_bounds__(256, 7) void pow_search_claim_kernel(PowJobDev job, uint32_t vb, uint32_t p, uint32_t u_begin,
                                                                  uint32_t u_end, uint32_t iters,
                                                                  uint32_t* __restrict__ out_count,
                                                                  uint32_t* __restrict__ out_words, uint32_t cap,
                                                                  PowFillDev fx, uint32_t claim, uint32_t* counter) {
    const uint32_t lane = threadIdx.x & 63u;
#if defined(__HIP_DEVICE_COMPILE__)
    for (;;) {
        auto ka = (__attribute__((address_space(4))) const PowClaimKernArgs*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(ka));
        const uint32_t step = ka->claim, n_u = ka->u_end - ka->u_begin;
        uint32_t taken = 0;
        if (lane == 0) taken = __hip_atomic_fetch_add(ka->counter, step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        taken = __builtin_amdgcn_readfirstlane(taken);
        if (taken >= n_u) return;
        uint32_t u = ka->u_begin + taken;
        const uint32_t u_stop = n_u - taken < step ? ka->u_end : u + step;
        PowSplitCacheT<true> cached;
        PowSplitLane lc;
        pow_split_prologue(job, p, vb + u, lane, cached, lc);
        cached.next = __builtin_amdgcn_readfirstlane(cached.next);  // see pow_a_fill
        for (; u < u_stop; ++u) {
            const uint32_t sv = vb + u;
            const uint32_t a = pow_a_fill<2>(job, p, sv, lane, cached, lc, fx, RANGE);
            bool hit;
            if (RANGE) {
                hit = a < job.range_width;
            } else {
                const uint32_t h0 = job.mid[0] + a;
                hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
            }
            if (__builtin_expect(__builtin_amdgcn_ballot_w64(hit) != 0, 0)) {
                if (hit) {
                    const uint32_t slot = atomicAdd(out_count, 1u);
                    if (slot < cap) out_words[slot] = sv + lc.lanep;
                }
            }
        }
    }
#endif
}
// Keep PowClaimKernArgs and the kernel's parameter list in step: the kernel argument segment holds the arguments in
// order, each at its own alignment, and the checks below compute that layout from the kernel's signature. A
// parameter added, removed, retyped or moved without the same change to the struct does not compile.
template <class F>
struct PowKernargLayout;
template <class... A>
struct PowKernargLayout<void (*)(A...)> {
    static constexpr size_t kCount = sizeof...(A);
    static constexpr size_t offset(size_t index) {  // of argument `index`; index == kCount: the segment's size
        constexpr size_t size[] = {sizeof(A)...}, align[] = {alignof(A)...};
        size_t at = 0;
        for (size_t i = 0; i < kCount; ++i) {
            at = (at + align[i] - 1) / align[i] * align[i];
            if (i == index) return at;
            at += size[i];
        }
        return at;
    }
};
using PowClaimLayout = PowKernargLayout<decltype(&pow_search_claim_kernel<true>)>;
static_assert(std::is_same_v<decltype(&pow_search_claim_kernel<true>), decltype(&pow_search_claim_kernel<false>)>);
static_assert(PowClaimLayout::kCount == 12 && std::is_standard_layout_v<PowClaimKernArgs>);
static_assert(offsetof(PowClaimKernArgs, job) == PowClaimLayout::offset(0) && offsetof(PowClaimKernArgs, vb) == PowClaimLayout::offset(1) &&
              offsetof(PowClaimKernArgs, p) == PowClaimLayout::offset(2) && offsetof(PowClaimKernArgs, u_begin) == PowClaimLayout::offset(3) &&
              offsetof(PowClaimKernArgs, u_end) == PowClaimLayout::offset(4) && offsetof(PowClaimKernArgs, iters) == PowClaimLayout::offset(5) &&
              offsetof(PowClaimKernArgs, out_count) == PowClaimLayout::offset(6) && offsetof(PowClaimKernArgs, out_words) == PowClaimLayout::offset(7) &&
              offsetof(PowClaimKernArgs, cap) == PowClaimLayout::offset(8) && offsetof(PowClaimKernArgs, fx) == PowClaimLayout::offset(9) &&
              offsetof(PowClaimKernArgs, claim) == PowClaimLayout::offset(10) && offsetof(PowClaimKernArgs, counter) == PowClaimLayout::offset(11),
              "PowClaimKernArgs must mirror pow_search_claim_kernel's parameters");
static_assert(offsetof(PowClaimKernArgs, u_begin) == 456 && offsetof(PowClaimKernArgs, claim) == 504 &&
              offsetof(PowClaimKernArgs, counter) == 512, "the offsets in the code object's metadata (.args) at the time of writing");

template <bool RANGE>
__global__ __launch_bounds__(256, 8) void pow_search_split_kernel(PowJobDev job, uint32_t vb, uint32_t p, uint32_t u_begin,
                                                                  uint32_t u_end, uint32_t iters,
                                                                  uint32_t* __restrict__ out_count,
                                                                  uint32_t* __restrict__ out_words, uint32_t cap) {
    const uint32_t wave = blockIdx.x * 4u + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t u = u_begin + wave * iters;
    if (u >= u_end) return;
    const uint32_t u_stop = u_end - u < iters ? u_end : u + iters;
    PowSplitCache cached;
    PowSplitLane lc;
    pow_split_prologue(job, p, vb + u, lane, cached, lc);
    for (; u < u_stop; ++u) {
        const uint32_t sv = vb + u;
        const uint32_t a = pow_a_split<2>(job, p, sv, lane, cached, lc);
        bool hit;
        if (RANGE) {
            hit = a + job.range_base < job.range_width;
        } else {
            const uint32_t h0 = job.mid[0] + a;
            hit = ((h0 ^ job.tword) & job.tmask) == 0 && ((h0 >> job.frac_shift) & 0xfu) < job.frac_limit;
        }
        if (__builtin_expect(hit, 0)) {
            const uint32_t slot = atomicAdd(out_count, 1u);
            if (slot < cap) out_words[slot] = sv + lc.lanep;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// Variant 10 cuts a range into pieces of 2^(p+6) nonce words, kPowSplitMinLog2 <= p <= kPowSplitMaxLog2. 26 is a
// whole sweep (six bits of the word are the lane index). Below 2^14 words a piece is at most 256 wave-iterations
// behind a prologue of its own and a dispatch of its own, and the unsplit kernel does all of what is left in one
// launch, so the rest of a range (fewer than 2^14 words) goes to it.
constexpr int kPowSplitMinLog2 = 8, kPowSplitMaxLog2 = 26;

PowJobDev make_pow_job(const PowJobHost& hj) {
    PowJobDev j{};
    const uint8_t* hdr = hj.header.data();
    const size_t len = hj.header.size();
    if (len != 108 && len != 138) throw std::invalid_argument("header must be 108 (v2) or 138 (v1) bytes");
    uint32_t st[8];
    std::memcpy(st, kSha256IV, sizeof(st));
    const int full_blocks = len == 108 ? 1 : 2;
    for (int b = 0; b < full_blocks; ++b) host_compress(st, hdr + 64 * b);
    uint8_t tail[64] = {0};
    const size_t rem = len - 64 * full_blocks;
    std::memcpy(tail, hdr + 64 * full_blocks, rem);
    // zero the nonce bytes (last 4 bytes of the header) in the template
    std::memset(tail + rem - 4, 0, 4);
    tail[rem] = 0x80;
    const uint64_t bits = uint64_t(len) * 8;
    for (int i = 0; i < 8; ++i) tail[56 + i] = uint8_t(bits >> (56 - 8 * i));
    for (int i = 0; i < 16; ++i) j.w[i] = load_be32(tail + 4 * i);
    std::memcpy(j.mid, st, sizeof(st));
    uint32_t ws[8];
    std::memcpy(ws, st, sizeof(st));
    host_rounds(ws, j.w, len == 108 ? 10 : 1);
    std::memcpy(j.st, ws, sizeof(ws));
    j.tmask = hj.tmask;
    j.tword = hj.tword;
    j.frac_shift = hj.frac_shift;
    j.frac_limit = hj.frac_limit;
    // nonce-independent values for pow_h0_pre
    const int r0 = len == 108 ? 10 : 1;
    const PowWordKinds kinds = pow_word_kinds(len == 108 ? 2 : 1);
    auto ssig0 = [](uint32_t x) { return host_rotr(x, 7) ^ host_rotr(x, 18) ^ (x >> 3); };
    auto ssig1 = [](uint32_t x) { return host_rotr(x, 17) ^ host_rotr(x, 19) ^ (x >> 10); };
    uint32_t wc[64] = {0};  // the constant words' values
    for (int i = 0; i < 64; ++i) {
        if (i < 16) {
            if (!kinds.vec[i]) wc[i] = j.w[i];
        } else {
            uint32_t sum = 0;
            if (!kinds.vec[i - 16]) sum += wc[i - 16];
            if (!kinds.vec[i - 15]) sum += ssig0(wc[i - 15]);
            if (!kinds.vec[i - 7]) sum += wc[i - 7];
            if (!kinds.vec[i - 2]) sum += ssig1(wc[i - 2]);
            if (!kinds.vec[i]) wc[i] = sum;
            else j.kw[i] = sum;
        }
        if (!kinds.vec[i]) j.kw[i] = kSha256K[i] + wc[i];
    }
    {
        const uint32_t* s = j.st;
        const uint32_t t1 = s[7] + (host_rotr(s[4], 6) ^ host_rotr(s[4], 11) ^ host_rotr(s[4], 25)) +
                            ((s[4] & s[5]) ^ (~s[4] & s[6])) + kSha256K[r0];
        const uint32_t t2 = (host_rotr(s[0], 2) ^ host_rotr(s[0], 13) ^ host_rotr(s[0], 22)) +
                            ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
        j.ce = s[3] + t1;
        j.ca = t1 + t2;
        for (int k = 0; k < 3; ++k) {
            const int i = r0 + 1 + k;
            j.hk[k] = s[6 - k] + (kinds.vec[i] ? kSha256K[i] : j.kw[i]);
        }
    }
    // variant 10 (108-byte header)
    j.c24 = j.kw[24] + j.kw[17];
    j.he = j.st[2] + j.hk[0];
    j.fxg = j.st[4] ^ j.st[5];
    j.bxc = j.st[0] ^ j.st[1];
    // The predicate ((H0 ^ tword) & tmask) == 0 && ((H0 >> frac_shift) & 15) < frac_limit is tword <= H0 <
    // tword + width where tmask is the nibbles above the fractional one (width = frac_limit << frac_shift) or,
    // with no fractional nibble, a prefix from the top of the word (width = its lowest set bit).
    {
        uint32_t width = 0;
        bool ok = false;
        if (j.frac_limit < 16) {
            const uint32_t above = j.frac_shift + 4 >= 32 ? 0u : ~((1u << (j.frac_shift + 4)) - 1u);
            ok = j.frac_shift <= 28 && j.tmask == above;
            width = j.frac_limit << (j.frac_shift & 31);
        } else if (j.tmask != 0) {
            width = j.tmask & (0u - j.tmask);
            ok = j.tmask == 0u - width;
        }
        ok = ok && width != 0 && (j.tword & ~j.tmask) == 0;
        j.range_ok = ok ? 1 : 0;
        j.range_base = j.mid[0] - j.tword;
        j.range_width = ok ? width : 0;
    }
    return j;
}

PowSplitConsts pow_split_consts(const PowJobHost& hj) {
    if (hj.header.size() != 108) throw std::invalid_argument("the split kernel is for the 108-byte header");
    const PowJobDev j = make_pow_job(hj);
    PowSplitConsts c;
    c.ca = j.ca; c.ce = j.ce; c.c17 = j.kw[17]; c.c24 = j.c24;
    c.mid0 = j.mid[0];
    c.range_ok = j.range_ok != 0;
    c.range_base = j.range_base;
    c.range_width = j.range_width;
    c.min_log2 = kPowSplitMinLog2;
    c.max_log2 = kPowSplitMaxLog2;
    return c;
}

bool pow_range_hit_host(const PowJobHost& hj, uint32_t h0) {
    const PowJobDev j = make_pow_job(hj);
    if (!j.range_ok) throw std::invalid_argument("this job's predicate has no range form");
    const uint32_t a = h0 - j.mid[0];  // the kernel has a, not H0
    return a + j.range_base < j.range_width;
}

template <bool G11>
static std::vector<uint32_t> pow_split_wave_loop(const PowJobDev& job, uint32_t vb, uint32_t p, uint32_t u_first,
                                                 uint32_t iters) {
    PowSplitCacheT<G11> cached[64];
    PowSplitLane lc[64];
    const PowFillDev fx = make_pow_fill(job);
    (void)fx;
    for (uint32_t lane = 0; lane < 64; ++lane) pow_split_prologue(job, p, vb + u_first, lane, cached[lane], lc[lane]);
    std::vector<uint32_t> out(size_t(iters) * 64);
    for (uint32_t it = 0; it < iters; ++it)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t sv = vb + u_first + it;
            if constexpr (G11) out[size_t(it) * 64 + lane] = job.mid[0] + pow_a_fill<2>(job, p, sv, lane, cached[lane], lc[lane], fx, false);
            else out[size_t(it) * 64 + lane] = job.mid[0] + pow_a_split<2>(job, p, sv, lane, cached[lane], lc[lane]);
        }
    return out;
}

std::vector<uint32_t> pow_split_wave_host(const PowJobHost& hj, uint32_t vb, uint32_t p, uint32_t u_first,
                                          uint32_t iters, int variant) {
    if (hj.header.size() != 108) throw std::invalid_argument("the split kernel is for the 108-byte header");
    if (p > uint32_t(kPowSplitMaxLog2)) throw std::invalid_argument("p must be at most 26: the lane index takes six bits");
    if (variant == 0) variant = 12;  // kPowDefaultVariant, checked below
    if (variant == 12) variant = 11;  // the claiming kernel runs variant 11's wave loop
    if (variant != 10 && variant != 11) throw std::invalid_argument("the wave loop is variant 10's, 11's and 12's");
    const PowJobDev job = make_pow_job(hj);
    return variant == 11 ? pow_split_wave_loop<true>(job, vb, p, u_first, iters)
                         : pow_split_wave_loop<false>(job, vb, p, u_first, iters);
}

// the range-form compare of variant 11's kernel on a digest word: a' = a + range_base comes out of round 63
bool pow_range_hit_folded_host(const PowJobHost& hj, uint32_t h0) {
    const PowJobDev j = make_pow_job(hj);
    if (!j.range_ok) throw std::invalid_argument("this job's predicate has no range form");
    const uint32_t a = h0 - j.mid[0];                     // a after round 63 with the plain K[63]
    const uint32_t folded = a - kSha256K[63] + make_pow_fill(j).k63r;    // the same round with k63r in K[63]'s place
    return folded < j.range_width;
}

// H0 of SHA256(header with nonce word v) through pow_h0_pre on the host: the kernel's arithmetic on the
// precomputed job constants, for the tests.
uint32_t pow_job_h0_host(const PowJobHost& hj, uint32_t v) {
    const PowJobDev job = make_pow_job(hj);
    return hj.header.size() == 108 ? pow_h0_pre<2>(job, v) : pow_h0_pre<1>(job, v);
}

// Claim counters of variant 12, one per dispatch of a search: they lie behind the hit count in one allocation, so
// that the memset at the start of a search zeroes both.
constexpr uint32_t kPowClaimCounters = 63;
struct PowDeviceBuffers {
    int device = -1;
    uint32_t* d_count = nullptr;   // the hit count, then kPowClaimCounters claim counters
    uint32_t* d_words = nullptr;
    uint32_t cap = 0;
};

static thread_local PowDeviceBuffers g_pow_bufs;

static PowDeviceBuffers& pow_buffers(uint32_t cap) {
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    PowDeviceBuffers& b = g_pow_bufs;
    if (b.device != dev || b.cap < cap) {
        if (b.d_count) { (void)hipFree(b.d_count); (void)hipFree(b.d_words); }
        hip_check(hipMalloc(&b.d_count, sizeof(uint32_t) * (1 + kPowClaimCounters)), "hipMalloc count");
        hip_check(hipMalloc(&b.d_words, sizeof(uint32_t) * cap), "hipMalloc words");
        b.device = dev;
        b.cap = cap;
    }
    return b;
}

// Kernel variants (bench.py --variant / UPOW_POW_VARIANT, scripts/pow_variants.py A/Bs them in one process):
//  1  the original loop forced to 8 waves/SIMD (spills)          2  message schedule staged in LDS
//  3  the original loop: K from a __constant__ table, uniforms hoisted by the compiler into VGPRs
//  4  host-precomputed uniforms in SGPRs (pow_h0_pre): 62 VGPRs, 103 SGPRs -> 7 waves/SIMD
//  5  as 4 with the SGPR budget of 8 waves/SIMD: the compiler re-materialises K words with s_mov in the loop
//     (SALU, no extra VALU), 61 VGPRs, no scratch
//  6-9  variant 5's instructions in a pinned order (pow_h0_sched), W[i+2] produced during round i, 8 waves/SIMD:
//     6  two-path rounds: next to no instruction follows its producer      7  rounds path after path
//     8  as 7 with an s_sleep 0 in front of every rotate      9  as 7 with one in front of every rotate and add3
//  10  variant 9 with the lane index in the top bits of the nonce word (pow_a_split, pow_search_split_kernel): the
//     wave-uniform low bits of W10, W17, W24, a11 and e11 go through the SALU, one scalar instruction in the place
//     of one filler; their per-lane high bits are loop-invariant VGPRs, and the hit predicate is one range check.
//     Pieces of 2^14..2^32 words; what is left of a range below 2^14 words runs on variant 9's kernel
//  0  the default, kPowDefaultVariant
// v1 headers have the original loop (1-3) and the precomputed one (4 and up) only.
//  11  variant 10 with one scalar or sequencer instruction in front of every slow instruction (pow_a_fill,
//     pow_search_fill_kernel): each K loaded in the slot in front of its add3, rounds 12 and 13 pinned, the nonce
//     word and W17 not materialised, the range check's base folded into round 63's K
//  12  variant 11's loop under a claiming wave loop (pow_search_claim_kernel): a wave takes `claim` values of U at a
//     time from a counter until the dispatch's range is used up, so no SIMD drains before the dispatch ends; a piece
//     is one dispatch unless chunk_iters, UPOW_POW_DISPATCH_LOG2 or a live node stream says otherwise
constexpr int kPowDefaultVariant = 12;
constexpr int kPowSplitVariant = 10;
constexpr int kPowFillVariant = 11;
constexpr int kPowClaimVariant = 12;
constexpr int kPowVariantCount = 13;
// Values of U a wave claims at a time where the caller names none: the best of 8..128 over a 2^32 sweep, where 16 to
// 64 are within 0.2 % of one another (docs/PERF.md, "PoW claimed chunks")
constexpr uint32_t kPowClaimDefault = 32;
static_assert(kPowDefaultVariant == 12, "pow_split_wave_host resolves 0 to the default variant by its number");
static bool pow_is_split(int variant) {
    return variant == kPowSplitVariant || variant == kPowFillVariant || variant == kPowClaimVariant;
}

using PowKernelFn = void (*)(PowJobDev, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t);

static int pow_resolve_variant(int variant) {
    if (variant < 0 || variant >= kPowVariantCount) throw std::invalid_argument("unknown PoW kernel variant");
    return variant == 0 ? kPowDefaultVariant : variant;
}

// The grid-strided kernel of a variant; for variant 10 the one that runs what its pieces leave over
static PowKernelFn pow_kernel_fn(bool v2, int variant) {
    variant = pow_resolve_variant(variant);
    if (v2 && pow_is_split(variant)) variant = 9;
    // v1 at 7 waves/SIMD: left to itself the compiler takes 106 SGPRs and spills some to VGPR lanes in the loop
    if (!v2) return variant >= 4 ? &pow_search_pre_kernel<1, 7> : &pow_search_kernel<1, 1>;
    switch (variant) {
        case 1: return &pow_search_kernel<2, 8>;
        case 2: return &pow_search_lds_kernel;
        case 4: return &pow_search_pre_kernel<2, 1>;
        case 5: return &pow_search_pre_kernel<2, 8>;
        case 6: return &pow_search_sched_kernel<2, true, 0, 8>;
        case 7: return &pow_search_sched_kernel<2, false, 0, 8>;
        case 8: return &pow_search_sched_kernel<2, false, 1, 8>;
        case 9: return &pow_search_sched_kernel<2, false, 2, 8>;
        default: return &pow_search_kernel<2, 1>;
    }
}

int pow_variant_count() { return kPowVariantCount; }

// The same through the device function of kernel variant `variant` (the pinned orders exist for 108-byte
// headers; every other variant and header is pow_h0_pre).
uint32_t pow_job_h0_host(const PowJobHost& hj, uint32_t v, int variant) {
    if (hj.header.size() != 108) return pow_job_h0_host(hj, v);
    const PowJobDev job = make_pow_job(hj);
    if (variant == 0) variant = kPowDefaultVariant;
    switch (variant) {
        case 6: return pow_h0_sched<2, 2, true, 0>(job, v);
        case 7: return pow_h0_sched<2, 2, false, 0>(job, v);
        case 8: return pow_h0_sched<2, 2, false, 1>(job, v);
        case 9: return pow_h0_sched<2, 2, false, 2>(job, v);
        case 10: return pow_h0_split<false>(job, v);
        case 11: case 12: return pow_h0_split<true>(job, v);
        default: return pow_h0_pre<2>(job, v);
    }
}

// Grid = exactly the resident capacity of the chip (CUs x blocks/CU for this kernel's VGPR/SGPR use),
// so every launch is one full "wave" of workgroups with no tail round.
static int pow_resident_blocks(bool v2, int variant) {
    int dev = 0, cus = 0, per_cu = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), "attr");
    const int rv = pow_resolve_variant(variant);
    const void* fn = v2 && rv == kPowClaimVariant   ? reinterpret_cast<const void*>(&pow_search_claim_kernel<true>)
                     : v2 && rv == kPowFillVariant  ? reinterpret_cast<const void*>(&pow_search_fill_kernel<true>)
                     : v2 && rv == kPowSplitVariant ? reinterpret_cast<const void*>(&pow_search_split_kernel<true>)
                                                    : reinterpret_cast<const void*>(pow_kernel_fn(v2, variant));
    hip_check(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, 0), "occupancy");
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 8) per_cu = 8;
    return cus * per_cu;
}

PowKernelInfo pow_kernel_info(int variant) {
    PowKernelInfo k;
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipDeviceGetAttribute(&k.cus, hipDeviceAttributeMultiprocessorCount, dev), "attr");
    k.resident_blocks = pow_resident_blocks(true, variant);
    k.blocks_per_cu = k.resident_blocks / (k.cus ? k.cus : 1);
    return k;
}

// Search nonce words [start, start + count) (count a multiple of the grid size is not required:
// the tail is covered by an extra short launch). Returns all candidate nonce words (host re-checks).
PowResult pow_search_gpu(const PowJobHost& hj, uint64_t start, uint64_t count, int grid_blocks,
                         uint32_t chunk_iters, uint32_t cap, int variant, uint32_t claim) {
    PowJobDev job = make_pow_job(hj);
    const bool v2 = hj.header.size() == 108;
    const PowKernelFn kernel = pow_kernel_fn(v2, variant);
    node_device_enter();  // a rank's search from any of its threads runs on the rank's own GPU
    PowDeviceBuffers& buf = pow_buffers(cap);
    hipStream_t st = miner_stream();  // least priority: node kernels go first (csrc/streams.h)
    const bool claiming = v2 && pow_resolve_variant(variant) == kPowClaimVariant;
    hip_check(hipMemsetAsync(buf.d_count, 0, sizeof(uint32_t) * (claiming ? 1 + kPowClaimCounters : 1), st), "memset");
    const uint32_t block = 256;
    if (grid_blocks <= 0) grid_blocks = pow_resident_blocks(v2, variant);
    const uint64_t per_launch_threads = uint64_t(grid_blocks) * block;
    bool whole_pieces = false;
    if (chunk_iters == 0) {
        // nonces per dispatch: 2^28 (~7.6 ms on MI355X) for a dedicated miner; 2^23 (~0.25 ms) once this
        // process also runs node kernels, so a queued node kernel waits at most one short dispatch (the miner
        // CLI next to a node process uses 2^23 too); UPOW_POW_DISPATCH_LOG2 overrides both.
        // Variant 12 as a dedicated miner: a piece is one dispatch. Every dispatch of claiming waves still ends in a
        // drain of up to one claim per wave, which sixteen times a sweep costs more than claiming gains.
        const bool node = node_stream_live().load();
        int lg = node ? 23 : 28;
        const char* e = std::getenv("UPOW_POW_DISPATCH_LOG2");
        if (e) lg = std::max(16, std::min(32, std::atoi(e)));
        whole_pieces = claiming && !node && !e;
        chunk_iters = uint32_t(std::max<uint64_t>(1, (uint64_t(1) << lg) / per_launch_threads));
    }
    uint64_t done = 0;
    if (v2 && pow_is_split(pow_resolve_variant(variant))) {
        // Maximal power-of-two pieces, largest first; grid_blocks and chunk_iters keep their meaning: blocks per
        // dispatch and iterations (values of U) per wave per dispatch. A piece smaller than a dispatch is spread
        // over as many waves as it has iterations for.
        const bool fill = pow_resolve_variant(variant) == kPowFillVariant;
        const auto claimed = job.range_ok ? &pow_search_claim_kernel<true> : &pow_search_claim_kernel<false>;
        // a claim that the caller names stands; UPOW_POW_CLAIM takes the place of the automatic value only
        if (claiming && claim == 0) {
            if (const char* e = std::getenv("UPOW_POW_CLAIM")) claim = uint32_t(std::max(0, std::atoi(e)));
        }
        uint32_t dispatches = 0;
        const auto split = job.range_ok ? &pow_search_split_kernel<true> : &pow_search_split_kernel<false>;
        const auto filled = job.range_ok ? &pow_search_fill_kernel<true> : &pow_search_fill_kernel<false>;
        const PowFillDev fx = make_pow_fill(job);
        const uint64_t waves = uint64_t(grid_blocks) * (block / 64);
        while (count - done >= (uint64_t(1) << (kPowSplitMinLog2 + 6))) {
            int lg = 63 - __builtin_clzll(count - done);
            const uint32_t p = uint32_t(std::min(lg - 6, kPowSplitMaxLog2));
            const uint32_t vb = uint32_t(start + done), n_u = uint32_t(1) << p;
            for (uint32_t u = 0; u < n_u;) {
                const uint32_t left = n_u - u;
                const uint32_t iters = uint32_t(std::min<uint64_t>(whole_pieces ? left : chunk_iters, (left + waves - 1) / waves));
                const uint64_t need = (uint64_t(left) + iters - 1) / iters;  // waves that have an iteration
                const uint32_t gb = uint32_t(std::min<uint64_t>(uint64_t(grid_blocks), (need + 3) / 4));
                const uint32_t u_end = uint32_t(std::min<uint64_t>(n_u, u + uint64_t(gb) * 4 * iters));
                if (claiming) {
                    // Automatic: never more than a quarter of a wave's share, so that no resident wave is left
                    // without work because the claims are too coarse. Any claim: at most the range, and small
                    // enough that the counter, which every wave pushes once past the range, does not wrap.
                    const uint32_t n = u_end - u;
                    uint32_t c = claim ? claim : std::min(kPowClaimDefault, std::max(1u, iters / 4));
                    c = uint32_t(std::min<uint64_t>(std::min(c, n), (0xffffffffull - n) / (uint64_t(gb) * 4 + 1)));
                    c = std::max(c, 1u);
                    // a counter of its own for each dispatch; when they are used up, zero them again behind the
                    // dispatches that used them
                    const uint32_t k = dispatches++ % kPowClaimCounters;
                    if (k == 0 && dispatches > 1)
                        hip_check(hipMemsetAsync(buf.d_count + 1, 0, sizeof(uint32_t) * kPowClaimCounters, st), "memset claims");
                    hipLaunchKernelGGL(claimed, dim3(gb), dim3(block), 0, st, job, vb, p, u, u_end, iters, buf.d_count,
                                       buf.d_words, cap, fx, c, buf.d_count + 1 + k);
                } else if (fill)
                    hipLaunchKernelGGL(filled, dim3(gb), dim3(block), 0, st, job, vb, p, u, u_end, iters, buf.d_count,
                                       buf.d_words, cap, fx);
                else
                    hipLaunchKernelGGL(split, dim3(gb), dim3(block), 0, st, job, vb, p, u, u_end, iters, buf.d_count,
                                       buf.d_words, cap);
                hip_check(hipGetLastError(), "pow_search_split_kernel launch");
                u = u_end;
            }
            done += uint64_t(1) << (p + 6);
        }
    }
    while (done < count) {
        const uint64_t left = count - done;
        uint32_t iters = chunk_iters;
        uint32_t gb = grid_blocks;
        if (uint64_t(iters) * per_launch_threads > left) {
            iters = uint32_t(left / per_launch_threads);
            if (iters == 0) {
                iters = 1;
                gb = uint32_t((left + block - 1) / block);
                if (uint64_t(gb) * block > left) {
                    // final ragged piece: round down to whole blocks, then single lanes via the host
                    gb = uint32_t(left / block);
                    if (gb == 0) break;
                }
            }
        }
        const uint32_t vb = uint32_t(start + done);
        hipLaunchKernelGGL(kernel, dim3(gb), dim3(block), 0, st, job, vb, iters, buf.d_count, buf.d_words, cap);
        hip_check(hipGetLastError(), "pow_search_kernel launch");
        done += uint64_t(iters) * gb * block;
    }
    uint32_t n = 0;
    hip_check(hipMemcpyAsync(&n, buf.d_count, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "copy count");
    hip_check(hipStreamSynchronize(st), "miner stream sync");
    PowResult r;
    r.searched = done;
    r.total_hits = n;
    const uint32_t stored = n < cap ? n : cap;
    r.words.resize(stored);
    if (stored)
    {
        hip_check(hipMemcpyAsync(r.words.data(), buf.d_words, sizeof(uint32_t) * stored, hipMemcpyDeviceToHost, st),
                  "copy words");
        hip_check(hipStreamSynchronize(st), "miner stream sync");
    }
    // any ragged remainder (< 256 nonces) is searched on the host so the requested range is exact
    if (done < count) {
        for (uint64_t k = done; k < count; ++k) {
            const uint32_t v = uint32_t(start + k);
            if (pow_check_word_host(hj, v)) { r.words.push_back(v); r.total_hits++; }
        }
        r.searched = count;
    }
    return r;
}

}  // namespace upow
