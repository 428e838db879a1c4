// Declarations shared between the pybind11 bindings (bindings.cpp, host C++) and the HIP
// translation units (*.hip). Only plain host types cross this boundary.
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace upow {

// ---------------------------------------------------------------- PoW (K1)
struct PowJobHost {
    std::vector<uint8_t> header;  // full 108-byte (v2) or 138-byte (v1) header; nonce bytes ignored
    uint32_t tmask = 0, tword = 0, frac_shift = 0, frac_limit = 16;
};

struct PowResult {
    uint64_t searched = 0;
    uint32_t total_hits = 0;
    std::vector<uint32_t> words;  // candidate nonce words (v2: bswap(nonce), v1: nonce)
};

struct PowKernelInfo {
    int cus = 0, blocks_per_cu = 0, resident_blocks = 0;
};
PowKernelInfo pow_kernel_info(int variant);
int pow_variant_count();  // kernel variants are numbered 0 (the default) .. pow_variant_count() - 1
// H0 of SHA256(header with nonce word v) computed on the host from the job constants the GPU kernel uses
uint32_t pow_job_h0_host(const PowJobHost& job, uint32_t v);
uint32_t pow_job_h0_host(const PowJobHost& job, uint32_t v, int variant);  // through variant's device function

// Kernel variant 10 (the lane/uniform split of the 108-byte search, csrc/pow_search.hip): the job constants it
// adds, for the tests. A piece of the search is v = vb + U + (lane << p), U in [0, 2^p) uniform across a wave.
struct PowSplitConsts {
    uint32_t ca = 0, ce = 0, c17 = 0, c24 = 0;  // a11 = ca + v, e11 = ce + v, W17 = c17 + v, W24 = c24 + v
    uint32_t mid0 = 0;                          // H0 = mid0 + a64
    bool range_ok = false;                      // the hit predicate is (H0 - tword) < range_width, unsigned
    uint32_t range_base = 0, range_width = 0;   // range_base = mid0 - tword
    int min_log2 = 0, max_log2 = 0;             // the p of the smallest and the largest piece pow_search_gpu cuts
};
PowSplitConsts pow_split_consts(const PowJobHost& job);
// The kernel's range form of the hit predicate on a given H0 (range_ok jobs only)
bool pow_range_hit_host(const PowJobHost& job, uint32_t h0);
// The same for variant 11's kernel, whose round 63 adds range_base with K[63]: the compare it is left with
bool pow_range_hit_folded_host(const PowJobHost& job, uint32_t h0);
// The wave loop of variant 10 or 11 (0: the default variant) on the host: 64 lanes with cached lane constants that
// are recomputed when a carry flips, U = u_first .. u_first + iters - 1. Returns H0 of every lane per iteration,
// [iteration][lane].
std::vector<uint32_t> pow_split_wave_host(const PowJobHost& job, uint32_t vb, uint32_t p, uint32_t u_first,
                                          uint32_t iters, int variant = 0);

bool pow_check_word_host(const PowJobHost& job, uint32_t v);
PowResult pow_search_host(const PowJobHost& job, uint64_t start, uint64_t count, int threads);
PowResult pow_search_gpu(const PowJobHost& job, uint64_t start, uint64_t count, int grid_blocks,
                         uint32_t chunk_iters, uint32_t cap, int variant, uint32_t claim = 0);

// ---------------------------------------------------------------- batched SHA-256 (K3/K4/K12)
// messages packed back to back in `data`, message i = data[offsets[i] .. offsets[i+1])
std::vector<uint8_t> sha256_batch_host(const uint8_t* data, const int64_t* offsets, int64_t n, int threads);
std::vector<uint8_t> sha256_batch_gpu(const uint8_t* data, int64_t nbytes, const int64_t* offsets, int64_t n);

// ---------------------------------------------------------------- P-256 (K5/K6/K15)
// verify items: 160-byte records {qx LE, qy LE, r LE, s LE, e = SHA-256 digest BE}
// status: 1 valid, 0 invalid, 2 key off-curve, 3 r/s out of range
std::vector<uint8_t> p256_verify_host(const uint8_t* items, int64_t n, int threads);
// one 160-byte VerifyItem on 64-bit limbs (csrc/p256_host.cpp); status as p256_verify_host
uint8_t p256_verify_one_host64(const uint8_t* item);
// p256_tables.hip's fixed-base table: 32 x 256 affine points, each x[8] y[8] little-endian u32 words
const void* p256_g_table_host();
// s^-1 * 2^256 mod n for s in [1, n) (little-endian 64-bit limbs): the divsteps inverse of p256_field.h
void p256_scalar_inv_mont_host(uint64_t out[4], const uint64_t s[4]);
// the cluster's per-block commit vote on a native RCCL communicator of its own (csrc/rccl_vote.hip)
// one-lane-per-signature batch verify launch (csrc/p256_batch.hip): VerifyItem items, 16-bit G table,
// 16 window-table entries of scratch per signature, status bytes
void p256_batch_launch(char variant, const void* items, int64_t n, const void* gtab16, void* scratch, uint8_t* status,
                       int spw, void* stream);
std::string rccl_unique_id();
int64_t rccl_vote_create(const std::string& uid, int world, int rank);
void rccl_vote_start(int64_t h, int value);
int64_t rccl_vote_finish(int64_t h, double timeout_s);  // SUM of the votes, -1 on timeout
void rccl_vote_destroy(int64_t h, bool abort);
std::vector<double> rccl_vote_stats(int64_t h);  // votes, then seconds in the all-gather, copy, event enqueues
// entries [first, first + count) of the device's 16-bit fixed-base window table (x, y little-endian each)
std::vector<uint8_t> p256_g16_entries(int64_t first, int64_t count);
// that table on the current device (a device pointer to 16 x 65,536 x {x[8], y[8]}), built on first use
const void* p256_g16_table_device();
std::vector<uint8_t> p256_verify_gpu(const uint8_t* items, int64_t n);
// decompression of 33-byte addresses (csrc/p256_keys.hip, as the on-curve check below)
void p256_decompress_host(const uint8_t* in33, int64_t n, uint8_t* out64, uint8_t* ok);
void p256_decompress_gpu(const uint8_t* in33, int64_t n, uint8_t* out64, uint8_t* ok);
// signer keys decompressed into verify items on the device, output addresses curve-checked, signatures
// verified: one stream order, one sync (p256.hip); fill(jobkeys33, sigdig96, outkeys33) packs the inputs
void p256_verify_fused_gpu(int64_t n_jobs, int64_t n_out, const std::function<void(uint8_t*, uint8_t*, uint8_t*)>& fill,
                           uint8_t* st, uint8_t* out_ok, std::vector<uint8_t>* items_out);
// on-curve check of 64-byte (version-1) addresses x LE | y LE: ok[i] = 1 iff x, y < p and y^2 = x^3 - 3x + b
void p256_on_curve_host(const uint8_t* xy64, int64_t n, uint8_t* ok, int threads);
void p256_on_curve_gpu(const uint8_t* xy64, int64_t n, uint8_t* ok);
// pin node-side GPU work of this process to one device (csrc/streams.h node_device_enter); -1 = unpinned
void set_node_device_native(int dev);
bool p256_pubkey(const uint8_t d_be[32], uint8_t out_le[64]);
bool p256_sign(const uint8_t d_be[32], const uint8_t digest[32], uint8_t r_le[32], uint8_t s_le[32]);
// K15 batched (core: csrc/p256_sign.h, not constant-time): n x 32-byte big-endian keys (and n x 32-byte SHA-256
// digests) -> n x 64 bytes x | y (r | s) little-endian and ok[n]; a key outside [1, n - 1] gets 64 zero bytes
// and ok = 0. _many_host: the kernels' core on the host pool; _gpu: one H2D, one launch, one D2H on the node
// stream, the device and pinned copies of the keys overwritten before return (csrc/p256_sign.hip)
void p256_pubkey_many_host(const uint8_t* keys_be, int64_t n, uint8_t* out_le, uint8_t* ok, int threads);
void p256_sign_many_host(const uint8_t* keys_be, const uint8_t* digests, int64_t n, uint8_t* rs_le, uint8_t* ok,
                         int threads);
void p256_pubkey_gpu(const uint8_t* keys_be, int64_t n, uint8_t* out_le, uint8_t* ok);
void p256_sign_gpu(const uint8_t* keys_be, const uint8_t* digests, int64_t n, uint8_t* rs_le, uint8_t* ok);
// test hooks: the first `count` RFC 6979 candidates (32 bytes big-endian each, accepted or not) from the shared
// core on one host thread / one GPU thread. They leak the nonce.
void p256_candidates_host(const uint8_t key_be[32], const uint8_t digest[32], int count, uint8_t* out);
void p256_candidates_gpu(const uint8_t key_be[32], const uint8_t digest[32], int count, uint8_t* out);
// K16 vanity search (core: csrc/p256_vanity.h, not constant-time; csrc/p256_vanity.hip): the keys of the scalars
// base + i, i in [0, count), walked with batched affine additions on the GPU or by the same core on the host
// pool; needs 1 <= base and base + count <= n. `ranges66` are n_ranges x (lo | hi), 33 bytes big-endian each:
// half-open, non-empty, sorted and disjoint ranges of the 33 address bytes read as a big-endian integer.
// total = the number of i whose address lies in a range; indexes = those i ascending, any max_hits of them when
// there are more. launch_keys / launch_lanes (0: the defaults of p256_vanity_info) shrink a GPU launch: test
// levers. std::invalid_argument for arguments outside these rules; std::runtime_error if a batch inversion
// met a zero factor (a defect: no keys are returned then). The device and pinned copies of base are overwritten.
struct VanityInfo {
    int keys_per_lane, lanes_per_block, max_ranges;  // keys per batch inversion; threads per block; ranges per call
    int64_t keys_per_launch;
};
VanityInfo p256_vanity_info();
struct VanityHits {
    uint64_t total = 0;
    std::vector<uint64_t> indexes;
};
VanityHits p256_vanity_search(const uint8_t base_be[32], int64_t count, const uint8_t* ranges66, int64_t n_ranges,
                              int64_t max_hits, bool gpu, int threads, int64_t launch_keys, int64_t launch_lanes);
// test hook: the 33 address bytes of every walked key, from the search's core with another sink (count <= 2^21)
std::vector<uint8_t> p256_vanity_walk(const uint8_t base_be[32], int64_t count, bool gpu, int threads,
                                      int64_t launch_keys, int64_t launch_lanes);
// test hook (not called by the node; csrc/p256_probe.h): operation `op` of the kernels' field, scalar and point
// arithmetic on n items of flat little-endian 32-bit words, operands a (and b, empty for one-operand operations).
// mode 'host': a host loop; 'ilp': a kernel of p256_probe.hip (ILP-first scheduler); 'occ': a kernel of p256_batch.hip
// (default scheduler). The lane-group operations ('quad_' / 'oct_' + mul4, sqr4, dbl4, add4; host and ilp only)
// return one copy of the result per lane of each group on the device (4 or 8), one per group on the host.
// std::invalid_argument for an unknown op or mode, or operand lengths that are not n whole items.
std::vector<uint8_t> p256_probe(const std::string& op, const uint8_t* a, size_t a_bytes, const uint8_t* b, size_t b_bytes,
                                const std::string& mode);
void p256_probe_occ_launch(int op, const uint32_t* a, const uint32_t* b, uint8_t* out, int64_t n, void* stream);

// ---------------------------------------------------------------- HBM UTXO index (K7/K8/K9): utxo_table.hip
// key records: 40 bytes {txid[32] raw, uint32 index, uint32 tag}
int64_t utxo_create(uint32_t log2_cap);
void utxo_destroy(int64_t h);
uint32_t utxo_capacity(int64_t h);
uint64_t utxo_rehash(int64_t h, uint32_t log2_cap);  // #moved | (#no slot << 32); any no slot: table unchanged
// payload records: 80 bytes {u64 amount, u32 address length, u32 pad, address[64]} (nullptr = zeros)
uint64_t utxo_insert(int64_t h, const uint8_t* recs, int64_t n, const uint8_t* payload);  // #full | (#duplicates << 32)
std::vector<uint8_t> utxo_probe(int64_t h, const uint8_t* recs, int64_t n);  // tag or 0xff
std::vector<uint8_t> utxo_lookup(int64_t h, const uint8_t* recs, int64_t n, std::vector<uint8_t>& payload_out);
std::vector<uint8_t> utxo_erase(int64_t h, const uint8_t* recs, int64_t n);  // 1 if erased
// queue one block's inserts + erases on the node stream and return; prev = the previous async apply's
// (no free slot, duplicates, erased) counters, collected first (returns whether there was one)
struct UtxoSeg { const uint8_t* recs; const uint8_t* pay; int64_t n; };  // n x 40 records, n x 80 payloads
bool utxo_apply_async(int64_t h, const std::vector<UtxoSeg>& ins, bool with_pay, const uint8_t* del, int64_t n_del,
                      uint32_t prev[3]);
bool utxo_apply_wait(int64_t h, uint32_t out[3]);  // collect the pending async apply's counters
std::vector<uint8_t> utxo_dump(int64_t h, std::vector<uint8_t>* payload_out);
// test hooks (not called by the node): the table's home slot at capacity 2^log2_cap and K10's fingerprint of
// each of n key records, from the kernels' own hash functions; the table's raw 48-byte slots (cap x 48 bytes)
void utxo_debug_hashes(const uint8_t* recs, int64_t n, uint32_t log2_cap, uint32_t* home_out, uint64_t* fp_out);
std::vector<uint8_t> utxo_debug_slots(int64_t h);

// ---------------------------------------------------------------- K14 address scan: utxo_scan.hip
// live outputs whose payload address equals addr[0:len] and whose tag is in tag_mask (a batch of one)
std::vector<uint8_t> utxo_address_scan(int64_t h, const uint8_t* addr, uint32_t len, uint32_t tag_mask,
                                       uint32_t stake_sel, std::vector<uint8_t>& payload_out, uint64_t* total_out);
// K14 for n queries in one table pass (ceil(n / 1024) launches under one lock hold): query i is addrs[64 i ..
// 64 i + lens[i]) with its own tag mask and stake selector. Matches come back in no particular order, each
// with the index of the query it answers (a slot matching several queries appears once per query; exact
// duplicate queries get equal answers); totals[i] = the amount sum of query i's matches.
struct AddressBatchOut {
    std::vector<uint32_t> qidx;    // per match: query index in the caller's numbering
    std::vector<uint8_t> recs;     // per match: 40-byte key record
    std::vector<uint8_t> payload;  // per match: 80-byte payload
    std::vector<uint64_t> totals;  // per query
};
void utxo_address_scan_batch(int64_t h, const uint8_t* addrs, const uint32_t* lens, const uint32_t* tag_masks,
                             const uint32_t* stake_sels, int64_t n, AddressBatchOut& out);

// ---------------------------------------------------------------- holders report: utxo_owners.hip
// Every owner's totals in one table pass (a hash aggregation by canonical 33-byte owner key,
// the 33- and 64-byte forms of a key folded). `recs` are 112-byte records {key[33], pad[7], u32 outputs, u32
// outputs in the 64-byte form, u64 sums[8]} in no particular order: every owner when top is -1, none when it
// is 0, else every owner whose metric (sum of the by_mask columns mod 2^64) is at least the top-th greatest,
// boundary ties included, so at least min(top, owners) of them. The counts and totals are over the whole set.
// log2_groups (0: as many slots as the table; else in [4, 31]) and tag_bits (in [0, 32]) size the scratch group
// table and mask its fingerprint tag: test levers, not set by the node. Entries that find no group slot make
// the call throw std::runtime_error with their count; the table is only read.
struct OwnerTotalsOut {
    std::vector<uint8_t> recs;
    uint64_t owners = 0, outputs = 0, skipped = 0;
    uint64_t totals[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
void utxo_owner_totals(int64_t h, int64_t top, uint32_t by_mask, uint32_t log2_groups, uint32_t tag_bits,
                       OwnerTotalsOut& out);

// ---------------------------------------------------------------- state digest: utxo_digest.hip, utxo_digest_host.cpp
// LtHash16/1024 of a set of entries (key record + payload): the lane-wise sum modulo 2^16 of each entry's 1024
// lanes, and the entry count. With L = addr_len if it is 33 or 64, else 0 (then amount and flags count as 0; an
// entry without payload has L = 0):
//   E = txid[32] | u8(index) | u8(tag) | u8(flags & 1) | u8(L) | u64le(amount) | addr[0:L]
//   lane[16 c + k] = the big-endian u16 at bytes 2k, 2k + 1 of SHA-256(E | u8(c)),  c in [0, 64), k in [0, 16)
// `state` is the 1024 lanes as little-endian u16. Sums of disjoint sets add lane-wise, so the digest after a block
// is the digest before + that of its created entries - that of its spent entries.
// utxo_state_digest: the live entries of table h whose tag's bit is set in tag_mask (tags above 31: none), in one
// table pass behind any queued async apply. utxo_records_digest: n host records (40 bytes) and payloads (80
// bytes, nullptr: none) on the GPU; _host: the same on `threads` host threads, the result independent of them.
// grid_blocks (0: the default grid, else at most 65,536) is a test lever, not set by the node.
struct StateDigestOut {
    uint8_t state[2048];
    uint64_t count = 0;
};
void utxo_state_digest(int64_t h, uint32_t tag_mask, uint32_t grid_blocks, StateDigestOut& out);
void utxo_records_digest(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t grid_blocks,
                         StateDigestOut& out);
void utxo_records_digest_host(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, int threads,
                              StateDigestOut& out);

// ---------------------------------------------------------------- UTXO proofs: utxo_merkle.hip, utxo_merkle_host.cpp
// A Merkle tree over a set of entries, so that one entry can be checked against 32 bytes and a count.
//   entry   E as the state digest defines it above (44, 77 or 108 bytes)
//   order   ascending by E's first 34 bytes: txid as 32 bytes, then u8(index), then u8(tag). Outpoints are unique in
//           a healthy index; the tag only makes the order total.
//   tree    RFC 6962 / RFC 9162 2.1.1: leaf = SHA-256(0x00 | E), node = SHA-256(0x01 | left | right), the tree of n
//           leaves split at the largest power of two below n; the root of the empty set is SHA-256 of the empty
//           string. Both builders go level by level instead: neighbours are paired and an unpaired last node is
//           promoted unchanged, which gives the same tree (the left subtree of every split is complete).
//   commitment  (root, count): a verifier needs both.
//   leaf proof  the leaf's position, its E and the RFC 9162 2.1.3 audit path, bottom up (a promoted node adds none).
//   outpoint proof (txid, index)  present: the leaf proofs of every leaf with that outpoint (normally one); absent:
//           those of the predecessor and the successor in the order (adjacent positions whose keys bracket the
//           query; one of the two when the query sorts before the first or after the last leaf, none for the empty
//           set).
// A snapshot is built from one state (utxo_merkle_build: the entries of table h whose tag's bit is set in tag_mask,
// tags above 31 never, collected under ONE hold of the table lock behind any queued async apply) and then owns its
// buffers: it answers without the table lock until it is freed. It holds, per entry, a 112-byte slot (E, zeros up
// to byte 108, then u32le(length of E)) and every level's 32-byte nodes: about 176 bytes. _build_records builds from
// n host records (40 bytes) and payloads (80 bytes, nullptr: none) on the GPU, _build_records_host on `threads` host
// threads with the same result whatever their number. launch_lever (0: 256 items per block; else 1..256, the items
// a 256-thread block takes, so that tiny inputs cross block boundaries in the leaf and level kernels) is a test
// lever, not set by the node.
constexpr size_t kMerkleSlot = 112;
struct MerkleInfo {
    uint8_t root[32];
    uint64_t count = 0, bytes = 0;  // bytes: what the snapshot holds (device or host)
    uint32_t levels = 0;            // stored levels, the leaves' included: 0 for the empty set
    bool on_device = false;
};
// Answers to q queries (40-byte records; the tag is ignored): query i is present[i] and owns the leaf proofs
// [first[i], first[i + 1]); leaf proof j is position[j], the slot entry[112 j ..] and the sibling hashes
// path[32 path_first[j] .. 32 path_first[j + 1]), bottom up.
struct MerkleProveOut {
    std::vector<uint8_t> present;
    std::vector<uint32_t> first, position, path_first;
    std::vector<uint8_t> entry, path;
};
int64_t utxo_merkle_build(int64_t h, uint32_t tag_mask, uint32_t launch_lever);
int64_t utxo_merkle_build_records(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t launch_lever);
int64_t utxo_merkle_build_records_host(const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, int threads);
MerkleInfo utxo_merkle_info(int64_t id);
void utxo_merkle_prove(int64_t id, const uint8_t* recs, int64_t q, MerkleProveOut& out);
void utxo_merkle_free(int64_t id);  // an unknown id is ignored
void utxo_merkle_held(uint64_t* snapshots, uint64_t* bytes);  // over all live snapshots

// ---------------------------------------------------------------- UTXO diff: utxo_diff.hip
// Which entries differ between table h and n host records (40 bytes) with payloads (80 bytes, nullptr: none), an
// entry being what the state digest hashes (E above) and the outpoint (txid, index) alone its identity. status[i]
// of record i: 0 the table holds the same E, 1 the outpoint is not live, 2 it is live with another E (a tag outside
// tag_mask included). An extra is a live entry with a tag in tag_mask that no record names: min(extra, limit) of
// them come back, which ones and in what order is not specified; the counts are exact. `repeated` is the number of
// records that name a live outpoint another record named already. The records go up in chunks of chunk_records
// (0: 2^20; a test lever) under ONE hold of the table lock, behind any queued async apply, so the whole diff sees
// one table state; hold_seconds is that hold and wait_seconds the wait for it. The table is only read.
struct UtxoDiffOut {
    std::vector<uint8_t> status;                 // per record: 0 same, 1 missing, 2 changed
    std::vector<uint8_t> extra_recs, extra_pay;  // min(extra, limit) entries, any order
    uint64_t extra = 0, repeated = 0, live = 0;  // exact; live = the table's entries with a tag in tag_mask
    double wait_seconds = 0, hold_seconds = 0;
};
void utxo_diff(int64_t h, const uint8_t* recs, const uint8_t* pay_or_null, int64_t n, uint32_t tag_mask,
               uint32_t limit, uint32_t chunk_records, UtxoDiffOut& out);

// ---------------------------------------------------------------- block input pass, K12 set hash: utxo_block.hip
// whole-block input pass: lookup (K7) + duplicate candidates (K10) + per-tx fees (K11) in one round trip
// Outputs of the whole-block input pass, written in place (the caller's arrays: no intermediate copies)
struct BlockInputsOut {
    uint8_t* tags;      // per input: table tag (0xff absent)
    uint8_t* payload;   // per input: 80-byte payload
    uint32_t* dup_of;   // per input: 1 + index of the earlier identical input, else 0
    int64_t* fee;       // per tx: sum(spent) - sum(outputs), smallest units
    uint32_t* missing;  // per tx: inputs not found with want_tag (or without payload)
    uint32_t n_dup = 0;
};
void utxo_block_inputs(int64_t h, const uint8_t* keys, int64_t n_in, const int32_t* in_start,
                       const uint64_t* out_amount, int64_t n_out, const int32_t* out_start, int64_t n_tx,
                       uint32_t want_tag, BlockInputsOut& r);
// K12 = SHA-256 over (txid || index byte) of the entries with `tag`, sorted by (txid, index).
// utxo_set_message: that message without the hash tail (the caller hashes it);
// utxo_k12_snapshot + utxo_k12_digest: the digest of the table as it was at the snapshot, computed later
std::vector<uint8_t> utxo_set_message(int64_t h, uint32_t tag, uint64_t* count_out);
int64_t utxo_k12_snapshot(int64_t h, uint32_t tag);
std::vector<uint8_t> utxo_k12_digest(int64_t id, uint64_t* count_out);

// ---------------------------------------------------------------- base58
std::string b58encode(const uint8_t* data, size_t n);  // n <= kB58MaxInput
// allocation-free form: writes at most kB58MaxOutput characters to out, returns how many
constexpr size_t kB58MaxInput = 64, kB58MaxOutput = 88;  // 64 bytes -> at most 88 digits
size_t b58encode_to(const uint8_t* data, size_t n, char* out);
std::vector<uint8_t> b58decode(const std::string& s);

// ---------------------------------------------------------------- device info
int gpu_device_count();
std::string gpu_arch_name(int device);

}  // namespace upow
