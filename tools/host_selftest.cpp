// Host-side self-test of the native library's CPU paths, built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tools/sanitize_host.sh ("Build the C++ with ASan/UBSan").
// Known-answer vectors: FIPS 180-2 SHA-256 "abc", RFC 6979 A.2.5 (P-256, SHA-256, "sample"),
// SEC 2 generator G, the state digest's five sets (csrc/native.h); everything else is a round-trip or a cross-check between two code paths.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../csrc/native.h"
#include "../csrc/sha256_common.h"

using namespace upow;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static std::vector<uint8_t> unhex(const char* h) {
    std::vector<uint8_t> out;
    for (size_t i = 0; h[i] && h[i + 1]; i += 2) {
        unsigned v;
        std::sscanf(h + i, "%2x", &v);
        out.push_back(uint8_t(v));
    }
    return out;
}

static std::vector<uint8_t> sha(const uint8_t* p, size_t n) {
    HostSha256 s;
    s.update(p, n);
    std::vector<uint8_t> d(32);
    s.final(d.data());
    return d;
}

static void test_sha256() {
    auto d = sha(reinterpret_cast<const uint8_t*>("abc"), 3);
    CHECK(d == unhex("ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"));
    // batch (threaded) == scalar for lengths across the 55/56/64-byte padding boundaries
    std::mt19937 rng(7);
    std::vector<uint8_t> data;
    std::vector<int64_t> off{0};
    for (int len = 0; len < 300; ++len) {
        for (int k = 0; k < len; ++k) data.push_back(uint8_t(rng()));
        off.push_back(int64_t(data.size()));
    }
    auto b = sha256_batch_host(data.data(), off.data(), int64_t(off.size() - 1), 4);
    for (size_t i = 0; i + 1 < off.size(); ++i) {
        auto ref = sha(data.data() + off[i], size_t(off[i + 1] - off[i]));
        CHECK(std::memcmp(b.data() + 32 * i, ref.data(), 32) == 0);
    }
    // SHA-NI block function == scalar rounds (multi-block runs from random states)
    if (sha256_ni_enabled()) {
        for (int t = 0; t < 200; ++t) {
            const size_t nb = 1 + rng() % 5;
            std::vector<uint8_t> blk(64 * nb);
            for (auto& x : blk) x = uint8_t(rng());
            uint32_t a[8], c[8];
            for (int i = 0; i < 8; ++i) a[i] = c[i] = uint32_t(rng());
            sha256_ni_blocks(a, blk.data(), nb);
            for (size_t k = 0; k < nb; ++k) host_compress_scalar(c, blk.data() + 64 * k);
            CHECK(std::memcmp(a, c, sizeof(a)) == 0);
        }
    } else {
        std::printf("note: no SHA-NI on this CPU, scalar path only\n");
    }
}

static void test_base58() {
    std::mt19937 rng(11);
    for (int t = 0; t < 200; ++t) {
        std::vector<uint8_t> v(size_t(rng() % 70));
        for (auto& x : v) x = uint8_t(rng());
        for (int z = 0; z < t % 4 && z < int(v.size()); ++z) v[size_t(z)] = 0;  // leading zeros -> '1'
        CHECK(b58decode(b58encode(v.data(), v.size())) == v);
    }
    bool threw = false;
    try {
        b58decode("0OIl");
    } catch (...) {
        threw = true;
    }
    CHECK(threw);
}

static void test_p256() {
    uint8_t d[32] = {0}, pub[64];
    d[31] = 1;
    CHECK(p256_pubkey(d, pub));
    auto gx = unhex("6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296");
    for (int i = 0; i < 32; ++i) CHECK(pub[i] == gx[31 - i]);  // little-endian x
    // RFC 6979 A.2.5, SHA-256, message "sample"
    auto dk = unhex("c9afa9d845ba75166b5c215767b1d6934e50c3db36e89b127b8a622b120f6721");
    auto e = sha(reinterpret_cast<const uint8_t*>("sample"), 6);
    uint8_t r[32], s[32];
    CHECK(p256_sign(dk.data(), e.data(), r, s));
    auto rr = unhex("efd48b2aacb6a8fd1140dd9cd45e81d69d2c877b56aaf991c34d0ea84eaf3716");
    auto ss = unhex("f7cb1c942d657c41d436c7a1b6e29f65f3e900dbb9aff4064dc4ab2f843acda8");
    for (int i = 0; i < 32; ++i) {
        CHECK(r[i] == rr[31 - i]);
        CHECK(s[i] == ss[31 - i]);
    }
    // batch verify: valid / wrong digest / off-curve key / s = 0, over several thread counts
    std::mt19937 rng(3);
    const int n = 64;
    std::vector<uint8_t> items(160 * n);
    std::vector<uint8_t> want(n);
    for (int k = 0; k < n; ++k) {
        uint8_t key[32], q[64], dig[32];
        for (auto& x : key) x = uint8_t(rng());
        key[0] &= 0x7f;
        for (auto& x : dig) x = uint8_t(rng());
        CHECK(p256_pubkey(key, q));
        CHECK(p256_sign(key, dig, r, s));
        uint8_t* it = items.data() + 160 * k;
        std::memcpy(it, q, 64);
        std::memcpy(it + 64, r, 32);
        std::memcpy(it + 96, s, 32);
        std::memcpy(it + 128, dig, 32);
        want[size_t(k)] = 1;
        if (k % 4 == 1) { it[128] ^= 1; want[size_t(k)] = 0; }
        if (k % 4 == 2) { it[32] ^= 1; want[size_t(k)] = 2; }
        if (k % 4 == 3) { std::memset(it + 96, 0, 32); want[size_t(k)] = 3; }
        if (k == 0) {  // compressed round trip through the decompressor
            uint8_t c[33], out[64], ok = 0;
            c[0] = (q[32] & 1) ? 43 : 42;
            std::memcpy(c + 1, q, 32);
            p256_decompress_host(c, 1, out, &ok);
            CHECK(ok == 1 && std::memcmp(out, q, 64) == 0);
        }
    }
    for (int threads : {1, 3, 8}) CHECK(p256_verify_host(items.data(), n, threads) == want);
}

// K16 on the host pool: a short walk and one search from base = 1 against p256_pubkey, key by key
static void test_vanity_host() {
    const VanityInfo info = p256_vanity_info();
    const int64_t count = 70 * info.keys_per_lane + 3;  // 71 work items: enough for the pool to use its threads
    uint8_t base[32] = {0};
    base[31] = 1;
    std::vector<std::vector<uint8_t>> want;
    for (int64_t i = 0; i < count; ++i) {
        uint8_t d[32] = {0}, q[64];
        d[29] = uint8_t((1 + i) >> 16);
        d[30] = uint8_t((1 + i) >> 8);
        d[31] = uint8_t(1 + i);
        CHECK(p256_pubkey(d, q));
        std::vector<uint8_t> a(33);
        a[0] = (q[32] & 1) ? 43 : 42;
        std::memcpy(a.data() + 1, q, 32);
        want.push_back(a);
    }
    for (int threads : {1, 4}) {
        const std::vector<uint8_t> got = p256_vanity_walk(base, count, false, threads, 0, 0);
        CHECK(int64_t(got.size()) == 33 * count);
        for (int64_t i = 0; i < count && got.size() == size_t(33 * count); ++i)
            CHECK(std::memcmp(got.data() + 33 * i, want[size_t(i)].data(), 33) == 0);
    }
    // the even-y half of the address space, and the one-value range of key 7 (33 bytes big-endian: the address itself)
    uint8_t ranges[2 * 66] = {0};
    ranges[0] = 42;
    ranges[33] = 43;
    std::vector<uint64_t> even;
    for (int64_t i = 0; i < count; ++i)
        if (want[size_t(i)][0] == 42) even.push_back(uint64_t(i));
    VanityHits h = p256_vanity_search(base, count, ranges, 1, count, false, 4, 0, 0);
    CHECK(h.total == even.size() && h.indexes == even);
    h = p256_vanity_search(base, count, ranges, 1, 3, false, 4, 0, 0);  // more hits than the buffer takes
    CHECK(h.total == even.size() && h.indexes.size() == 3);
    std::memcpy(ranges, want[7].data(), 33);
    std::memcpy(ranges + 33, want[7].data(), 33);
    for (int k = 65; k >= 33 && ++ranges[k] == 0; --k) {}  // hi = lo + 1
    h = p256_vanity_search(base, count, ranges, 1, 8, false, 1, 0, 0);
    CHECK(h.total == 1 && h.indexes == std::vector<uint64_t>{7});
    bool threw = false;
    try {
        uint8_t zero[32] = {0};
        p256_vanity_walk(zero, 1, false, 1, 0, 0);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw);
}

// State digest (LtHash16/1024, csrc/utxo_digest_host.cpp): the known answers of the sets {}, {A}, {B}, {C}, {A, B, C}
// (lanes 0..3, lane 1023, the short id SHA-256("upow-utxo-state-v1" | u64le(count) | state)), computed with
// hashlib from the definition; the result does not depend on the thread count, the split or the order.
static void put_entry(std::vector<uint8_t>& recs, std::vector<uint8_t>& pay, const uint8_t txid[32], uint32_t index,
                      uint32_t tag, uint32_t flags, uint64_t amount, const std::vector<uint8_t>& addr) {
    const size_t r = recs.size(), p = pay.size();
    recs.resize(r + 40, 0);
    pay.resize(p + 80, 0);
    std::memcpy(&recs[r], txid, 32);
    std::memcpy(&recs[r + 32], &index, 4);
    std::memcpy(&recs[r + 36], &tag, 4);
    const uint32_t len = uint32_t(addr.size());
    std::memcpy(&pay[p], &amount, 8);
    std::memcpy(&pay[p + 8], &len, 4);
    std::memcpy(&pay[p + 12], &flags, 4);
    if (len) std::memcpy(&pay[p + 16], addr.data(), len);
}

static std::string state_short_id(const StateDigestOut& d) {
    std::vector<uint8_t> m;
    const char* dom = "upow-utxo-state-v1";
    m.insert(m.end(), dom, dom + std::strlen(dom));
    for (int i = 0; i < 8; ++i) m.push_back(uint8_t(d.count >> (8 * i)));
    m.insert(m.end(), d.state, d.state + sizeof d.state);
    std::string hex;
    char b[3];
    for (uint8_t x : sha(m.data(), m.size())) {
        std::snprintf(b, sizeof b, "%02x", x);
        hex += b;
    }
    return hex;
}

static void test_state_digest() {
    uint8_t ta[32], tb[32], tc[32];
    std::vector<uint8_t> aa{42}, ab;
    for (int i = 0; i < 32; ++i) {
        ta[i] = uint8_t(i);
        tb[i] = uint8_t(32 + i);
        tc[i] = 0xff;
        aa.push_back(uint8_t(1 + i));
    }
    for (int i = 0; i < 64; ++i) ab.push_back(uint8_t(100 + i));
    struct Known {
        int set;  // bit 0: A, bit 1: B, bit 2: C
        uint16_t lanes[4], last;
        const char* id;
    };
    const Known known[] = {
        {0, {0, 0, 0, 0}, 0, "4577ffd454ce69e51a2270ed607b8d177f6ab4f55a4ab9ee86b35ddf0ec5701e"},
        {1, {26070, 32850, 57441, 7641}, 5172, "c75477d194dae8dfccf51124c0ef15ba6592b7b3e62cd51f80d8549c00a2c72c"},
        {2, {41818, 58637, 24425, 48484}, 60684, "ae5bf37023ce0473a10759302c5d2c7c50c135a99a038404b26068fafc2606f4"},
        {4, {59715, 39545, 44934, 31578}, 42120, "171ca47560425b0c0365767be9f81f650a7c04a04f661feb57919f663bb43790"},
        {7, {62067, 65496, 61264, 22167}, 42440, "6240967130b264ca49cfa3f850b080d1420d54710a2bdf6f430949378e3248a8"}};
    auto lane = [](const StateDigestOut& d, int x) { return uint16_t(d.state[2 * x] | (d.state[2 * x + 1] << 8)); };
    for (const Known& k : known) {
        std::vector<uint8_t> recs, pay;
        if (k.set & 1) put_entry(recs, pay, ta, 0, 0, 0, 1, aa);
        if (k.set & 2) put_entry(recs, pay, tb, 255, 0, 1, 600000000, ab);
        if (k.set & 4) put_entry(recs, pay, tc, 7, 6, 0, 12345, {});
        const int64_t n = int64_t(recs.size() / 40);
        for (int threads : {1, 3}) {
            StateDigestOut d;
            utxo_records_digest_host(recs.data(), pay.data(), n, threads, d);
            CHECK(d.count == uint64_t(n));
            for (int x = 0; x < 4; ++x) CHECK(lane(d, x) == k.lanes[x]);
            CHECK(lane(d, 1023) == k.last);
            CHECK(state_short_id(d) == k.id);
        }
    }
    // C with a flag, an amount and three address bytes is C (nothing of a payload of unknown length is hashed), and
    // so is C without payload
    std::vector<uint8_t> recs, pay;
    put_entry(recs, pay, tc, 7, 6, 1, 999, {'x', 'y', 'z'});
    StateDigestOut d, e;
    utxo_records_digest_host(recs.data(), pay.data(), 1, 1, d);
    utxo_records_digest_host(recs.data(), nullptr, 1, 1, e);
    CHECK(state_short_id(d) == known[3].id && state_short_id(e) == known[3].id);
    // 2,000 random entries: 125 work items, enough for the pool to run them on its threads (it keeps fewer than 64
    // on the caller), so the per-item accumulators and the locked merge run concurrently here; every thread count
    // gives the same bytes; two parts add up
    std::mt19937 rng(17);
    recs.clear();
    pay.clear();
    for (int i = 0; i < 2000; ++i) {
        uint8_t t[32];
        for (auto& x : t) x = uint8_t(rng());
        std::vector<uint8_t> addr(size_t(i % 3 == 0 ? 33 : (i % 3 == 1 ? 64 : 0)));
        for (auto& x : addr) x = uint8_t(rng());
        put_entry(recs, pay, t, rng() & 0xff, rng() % 7, rng() & 1, (uint64_t(rng()) << 20) | rng(), addr);
    }
    StateDigestOut one, many, lo, hi;
    utxo_records_digest_host(recs.data(), pay.data(), 2000, 1, one);
    utxo_records_digest_host(recs.data(), pay.data(), 2000, 16, many);
    CHECK(std::memcmp(one.state, many.state, sizeof one.state) == 0 && one.count == 2000 && many.count == 2000);
    utxo_records_digest_host(recs.data(), pay.data(), 300, 3, lo);  // 19 items: on the caller
    utxo_records_digest_host(recs.data() + 40 * 300, pay.data() + 80 * 300, 1700, 3, hi);
    for (int x = 0; x < 1024; ++x) CHECK(uint16_t(lane(lo, x) + lane(hi, x)) == lane(one, x));
}

// UTXO proofs (csrc/utxo_merkle_host.cpp): the known roots of the sets {}, {A}, {A, B, C} of the state digest's entries
// (computed with hashlib from the recursive RFC 6962 definition), C's payload noise dropped, every leaf of a 300-entry
// tree rehashed up its audit path, absence at both ends, and the same tree from every thread count.
static std::vector<uint8_t> fold_path(const MerkleProveOut& p, size_t j, uint64_t count) {
    uint32_t len;
    std::memcpy(&len, &p.entry[j * kMerkleSlot + 108], 4);
    std::vector<uint8_t> m{0x00};
    m.insert(m.end(), &p.entry[j * kMerkleSlot], &p.entry[j * kMerkleSlot] + len);
    std::vector<uint8_t> r = sha(m.data(), m.size());
    uint64_t fn = p.position[j], sn = count - 1;  // RFC 9162 2.1.3.2
    for (uint32_t k = p.path_first[j]; k < p.path_first[j + 1]; ++k) {
        const uint8_t* h = &p.path[32 * size_t(k)];
        std::vector<uint8_t> node{0x01};
        if ((fn & 1) || fn == sn) {
            node.insert(node.end(), h, h + 32);
            node.insert(node.end(), r.begin(), r.end());
            while (fn && !(fn & 1)) fn >>= 1, sn >>= 1;
        } else {
            node.insert(node.end(), r.begin(), r.end());
            node.insert(node.end(), h, h + 32);
        }
        r = sha(node.data(), node.size());
        fn >>= 1, sn >>= 1;
    }
    CHECK(sn == 0);
    return r;
}

static void test_merkle_host() {
    uint8_t ta[32], tb[32], tc[32];
    std::vector<uint8_t> aa{42}, ab;
    for (int i = 0; i < 32; ++i) {
        ta[i] = uint8_t(i);
        tb[i] = uint8_t(32 + i);
        tc[i] = 0xff;
        aa.push_back(uint8_t(1 + i));
    }
    for (int i = 0; i < 64; ++i) ab.push_back(uint8_t(100 + i));
    const struct { int set; const char* root; } known[] = {
        {0, "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"},
        {1, "d68a3c66ecda39a9b29757e377b40021584637bb9d1f9564ca3bd761b0fa8e5a"},
        {7, "55a26afe2b59d453ddabdd176be6de0df1f39d6a98386e104ea651b2d26daa3b"}};
    for (const auto& k : known) {
        std::vector<uint8_t> recs, pay;
        if (k.set & 4) put_entry(recs, pay, tc, 7, 6, 1, 999, {'x', 'y', 'z'});  // canonicalised: C
        if (k.set & 2) put_entry(recs, pay, tb, 255, 0, 1, 600000000, ab);
        if (k.set & 1) put_entry(recs, pay, ta, 0, 0, 0, 1, aa);
        for (int threads : {1, 3}) {
            const int64_t id = utxo_merkle_build_records_host(recs.data(), pay.data(), int64_t(recs.size() / 40), threads);
            const MerkleInfo info = utxo_merkle_info(id);
            CHECK(std::vector<uint8_t>(info.root, info.root + 32) == unhex(k.root));
            CHECK(info.count == recs.size() / 40 && !info.on_device);
            utxo_merkle_free(id);
        }
    }
    std::mt19937 rng(23);
    std::vector<uint8_t> recs, pay;
    for (int i = 0; i < 300; ++i) {
        uint8_t t[32];
        for (auto& x : t) x = uint8_t(rng());
        t[0] = uint8_t(1 + i % 200);  // never the smallest or the greatest possible txid
        std::vector<uint8_t> addr(size_t(i % 3 == 0 ? 33 : (i % 3 == 1 ? 64 : 0)));
        for (auto& x : addr) x = uint8_t(rng());
        put_entry(recs, pay, t, rng() & 0xff, rng() % 7, rng() & 1, (uint64_t(rng()) << 20) | rng(), addr);
    }
    uint64_t held_n = 0, held_b = 0, n1 = 0, b1 = 0;
    utxo_merkle_held(&held_n, &held_b);
    const int64_t one = utxo_merkle_build_records_host(recs.data(), pay.data(), 300, 1);
    const int64_t many = utxo_merkle_build_records_host(recs.data(), pay.data(), 300, 16);
    const MerkleInfo info = utxo_merkle_info(one), info16 = utxo_merkle_info(many);
    CHECK(std::memcmp(info.root, info16.root, 32) == 0 && info.count == 300 && info.levels == 10);
    std::vector<uint8_t> queries = recs;
    queries.resize(40 * 302, 0);  // + the smallest outpoint and the greatest
    std::memset(&queries[40 * 301], 0xff, 33);
    MerkleProveOut p;
    utxo_merkle_prove(many, queries.data(), 302, p);
    CHECK(p.present.size() == 302 && p.first.back() == 302 && p.position.size() == 302);
    for (size_t j = 0; j < p.position.size(); ++j)
        CHECK(fold_path(p, j, 300) == std::vector<uint8_t>(info.root, info.root + 32));
    for (int i = 0; i < 300; ++i) CHECK(p.present[size_t(i)] == 1);
    CHECK(!p.present[300] && p.position[300] == 0 && !p.present[301] && p.position[301] == 299);
    utxo_merkle_prove(one, queries.data(), 0, p);
    CHECK(p.present.empty() && p.first.size() == 1 && p.path.empty());
    utxo_merkle_free(one);
    utxo_merkle_held(&n1, &b1);
    CHECK(n1 == held_n + 1 && b1 == held_b + info16.bytes);
    utxo_merkle_free(many);
    utxo_merkle_free(many);  // an unknown id is ignored
    utxo_merkle_held(&n1, &b1);
    CHECK(n1 == held_n && b1 == held_b);
}

static void test_pow_host() {
    PowJobHost job;
    job.header.assign(108, 0);
    job.header[0] = 2;
    for (int i = 1; i < 104; ++i) job.header[size_t(i)] = uint8_t(i * 37);
    job.tmask = 0xff000000u;  // 2 nibbles
    job.tword = 0x00000000u;
    PowResult res = pow_search_host(job, 0, 1u << 18, 4);
    CHECK(res.searched == (1u << 18));
    CHECK(!res.words.empty());
    for (uint32_t w : res.words) CHECK(pow_check_word_host(job, w));
}

int main() {
    test_sha256();
    test_base58();
    test_p256();
    test_vanity_host();
    test_state_digest();
    test_merkle_host();
    test_pow_host();
    if (failures) {
        std::fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    std::printf("host selftest: all checks passed\n");
    return 0;
}
