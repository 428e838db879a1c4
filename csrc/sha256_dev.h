// The gfx950 SHA-256 compression shared by the batched hashing kernel (csrc/sha256_batch.hip) and the
// RFC 6979 signing kernels (csrc/p256_sign.hip). Device code only: include it from a .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace upow {

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

static __constant__ uint32_t bK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

// One compression of the block `w` (16 big-endian words, overwritten by the message schedule) into `st`.
__device__ __forceinline__ void dev_compress(uint32_t st[8], uint32_t w[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t wi;
        if (i < 16) {
            wi = w[i];
        } else {
            wi = w[i & 15] + SSIG0(w[(i - 15) & 15]) + w[(i - 7) & 15] + SSIG1(w[(i - 2) & 15]);
            w[i & 15] = wi;
        }
        uint32_t t1 = h + BSIG1(e) + CH(e, f, g) + bK[i] + wi;
        uint32_t t2 = BSIG0(a) + MAJ(a, b, c);
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

}  // namespace upow
