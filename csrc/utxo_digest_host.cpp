// State digest on the host: LtHash16/1024 of key records + payloads (the definition is in native.h; the GPU
// passes are csrc/utxo_digest.hip). 1 + 64 compressions per entry with a 33/64-byte address, 64 without.
#include <cstring>
#include <mutex>
#include <stdexcept>

#include "native.h"
#include "sha256_common.h"
#include "thread_pool.h"

namespace upow {

namespace {

// Entries per work item. The pool runs fewer than 64 items on the caller and hands out at least 16 at a time, so
// sets of 1,024 entries and more are spread over the threads, 256 entries a claim; an item's 1,024-word merge is
// ~1 % of its ~1,000 compressions. The sums commute, so neither the split nor the order shows in the result.
constexpr int64_t kChunk = 16;

// the 1024 lanes of one entry added to acc (modulo 2^32: the low 16 bits are the lane)
void digest_entry(const uint8_t* rec, const uint8_t* pay, uint32_t acc[1024]) {
    uint8_t e[109] = {0};  // E | c
    std::memcpy(e, rec, 32);
    e[32] = rec[32];  // u8(index), u8(tag): the low bytes of the record's little-endian words
    e[33] = rec[36];
    size_t len = 0;
    if (pay) {
        uint32_t l;
        std::memcpy(&l, pay + 8, 4);
        if (l == 33 || l == 64) {
            len = l;
            e[34] = pay[12] & 1;
            std::memcpy(e + 36, pay, 8);  // amount: little-endian in the payload and in E
            std::memcpy(e + 44, pay + 16, len);
        }
    }
    e[35] = uint8_t(len);
    const size_t total = 44 + len + 1;  // 45, 78 or 109 bytes: one or two blocks
    uint32_t mid[8];
    std::memcpy(mid, kSha256IV, sizeof mid);
    uint8_t last[64] = {0};
    size_t c_at;
    if (len) {
        host_compress(mid, e);  // the first 64 bytes do not depend on c
        std::memcpy(last, e + 64, total - 1 - 64);
        c_at = total - 1 - 64;
    } else {
        std::memcpy(last, e, 44);
        c_at = 44;
    }
    last[c_at + 1] = 0x80;
    last[62] = uint8_t((total * 8) >> 8);
    last[63] = uint8_t(total * 8);
    for (uint32_t c = 0; c < 64; ++c) {
        uint32_t st[8];
        std::memcpy(st, mid, sizeof st);
        last[c_at] = uint8_t(c);
        host_compress(st, last);
        for (int j = 0; j < 8; ++j) {
            acc[16 * c + 2 * j] += st[j] >> 16;
            acc[16 * c + 2 * j + 1] += st[j];
        }
    }
}

}  // namespace

void utxo_records_digest_host(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, int threads,
                              StateDigestOut& out) {
    if (n < 0) throw std::invalid_argument("record count must be >= 0");
    std::vector<uint32_t> sum(1024, 0);
    std::mutex mu;
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    HostPool::get().parallel_for(chunks, threads, [&](int64_t ch) {
        uint32_t acc[1024] = {0};
        const int64_t end = std::min(n, (ch + 1) * kChunk);
        for (int64_t i = ch * kChunk; i < end; ++i)
            digest_entry(recs + 40 * i, pay_or_null ? pay_or_null + 80 * i : nullptr, acc);
        std::lock_guard<std::mutex> g(mu);  // sums commute: the order of the chunks does not matter
        for (int x = 0; x < 1024; ++x) sum[size_t(x)] += acc[x];
    });
    for (int x = 0; x < 1024; ++x) {
        out.state[2 * x] = uint8_t(sum[size_t(x)]);
        out.state[2 * x + 1] = uint8_t(sum[size_t(x)] >> 8);
    }
    out.count = uint64_t(n);
}

}  // namespace upow
