// Native block-transaction codec: the whole-block replacement of Transaction.parse + hex() + txid.
//
// reference: upow/upow_transactions/transaction.py:46-88 (hex / hash), 520-592 (from_hex),
// transaction_output.py (tobytes), helpers.py:160-192 (address strings). The node receives a block
// as a list of tx hex strings (POST /push_block, sync pages); the Python object model costs ~20 µs
// per tx just to parse and re-serialise. Here one call, threaded over the txs with the GIL released:
//
//   hex -> bytes -> fields (same reading rules as Transaction.parse)
//       -> canonical re-serialisation (exactly what Transaction.hex() would produce: normalised
//          address prefix, minimal amount length, de-duplicated signatures)
//       -> txid = SHA-256(canonical bytes), signed-message digest = SHA-256(hex(False) bytes)
//       -> address strings (base58 / hex), outputs JSON columns, merkle root
//
// Governance transactions decode like any other: their output types and the tx type carried in the
// message (helpers.py:97-112, ASCII digits) come out as columns, and the block path checks their rules
// in batch (upow_amd/ledger/govcheck.py). A tx the fast path does not cover (coinbase specifier,
// grouped signatures that need ledger public keys, amounts wider than 64 bits, malformed encodings, ...)
// is flagged; the caller then runs the general Python path for the whole block, which reproduces the
// reference's exact behaviour and error messages.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "thread_pool.h"
#include "native.h"
#include "sha256_common.h"
#include "txdecode.h"

namespace py = pybind11;

namespace upow {

// CPython objects for the (all-ASCII) strings the codec produces: PyUnicode_New(len, 127) + memcpy
// is the cheapest constructor, and a PyList_New list is filled with PyList_SET_ITEM (steals the ref).
static PyObject* ascii_str(const char* p, size_t n) {
    PyObject* o = PyUnicode_New(Py_ssize_t(n), 127);
    if (!o) throw py::error_already_set();
    std::memcpy(PyUnicode_DATA(o), p, n);
    return o;
}

static py::list new_list(size_t n) {
    PyObject* l = PyList_New(Py_ssize_t(n));
    if (!l) throw py::error_already_set();
    return py::reinterpret_steal<py::list>(l);
}

template <typename F>
static void parallel_for(int64_t n, int threads, F&& f) {
    HostPool::get().parallel_for(n, threads, std::forward<F>(f));
}

// The same with at least `grain` items per thread: a pass whose items cost tens of nanoseconds (a base58
// string, a memcpy) runs on fewer threads, or on the caller alone, when waking the pool would cost more
// than it saves (a 200-tx sync block's 400 input strings: 22 us on one thread, 190 us spread over eight)
template <typename F>
static void parallel_for_grain(int64_t n, int threads, int64_t grain, F&& f) {
    const int64_t cap = std::max<int64_t>(1, n / std::max<int64_t>(1, grain));
    HostPool::get().parallel_for(n, int(std::min<int64_t>(threads, cap)), std::forward<F>(f));
}

// merkle root: SHA-256 over the txids of the txs sorted by their canonical bytes (manager.py:365-378)
static std::string merkle_of(const std::vector<DecTx>& txs, size_t n) {
    // sort by (big-endian 8-byte prefix, full bytes): canonical txs start with version, n_in and a
    // random input txid, so the integer prefix decides almost every comparison without touching
    // the tx bytes (zero padding of short txs is resolved by the full comparison on a tie)
    std::vector<std::pair<uint64_t, int>> order(n);
    for (size_t i = 0; i < order.size(); ++i) {
        const auto& c = txs[i].canon;
        uint64_t key = 0;
        for (size_t k = 0; k < 8; ++k) key = (key << 8) | (k < c.size() ? c[k] : 0u);
        order[i] = {key, int(i)};
    }
    std::sort(order.begin(), order.end(), [&](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) {
        if (a.first != b.first) return a.first < b.first;
        const auto& x = txs[size_t(a.second)].canon;
        const auto& y = txs[size_t(b.second)].canon;
        return std::lexicographical_compare(x.begin(), x.end(), y.begin(), y.end());
    });
    HostSha256 h;
    for (const auto& o : order) h.update(txs[size_t(o.second)].txid, 32);
    uint8_t out[32];
    h.final(out);
    return to_hex(out, 32);
}

static py::bytes as_bytes(const std::vector<uint8_t>& v) {
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size());
}

// Text arena: all strings of one column concatenated + int64 offsets[n+1]. The bulk ledger writer
// (csrc/ledger_sql.cpp, column kind 'arena') binds slices of it, so the per-output strings never
// become Python objects.
struct Arena {
    std::string blob;
    std::vector<int64_t> off{0};
    void add(const char* p, size_t n) {
        blob.append(p, n);
        off.push_back(int64_t(blob.size()));
    }
    py::tuple py() const {
        return py::make_tuple(py::bytes(blob), py::bytes(reinterpret_cast<const char*>(off.data()), off.size() * 8));
    }
};

// Decode workspaces: the per-tx DecTx objects (and all their buffers) outlive a call and are reused by
// the next one, so a steady stream of blocks decodes without heap traffic. Concurrent callers (the
// ledger thread and the sync pipeline's decode-ahead thread) each lease their own workspace.
struct DecWorkspace {
    std::vector<DecTx> txs;
};
class DecWorkspaceLease {
public:
    DecWorkspaceLease() {
        std::lock_guard<std::mutex> g(mu());
        if (!free_list().empty()) {
            ws_ = std::move(free_list().back());
            free_list().pop_back();
        } else {
            ws_ = std::make_unique<DecWorkspace>();
        }
    }
    ~DecWorkspaceLease() {
        // a workspace that grew for an unusually large call is dropped rather than pinned forever
        if (ws_->txs.size() > (1u << 16)) return;
        std::lock_guard<std::mutex> g(mu());
        if (free_list().size() < 4) free_list().push_back(std::move(ws_));
    }
    DecWorkspace& get() { return *ws_; }

private:
    static std::mutex& mu() {
        static std::mutex m;
        return m;
    }
    static std::vector<std::unique_ptr<DecWorkspace>>& free_list() {
        static auto* l = new std::vector<std::unique_ptr<DecWorkspace>>();  // never destroyed at exit
        return *l;
    }
    std::unique_ptr<DecWorkspace> ws_;
};

// The block's merkle root, computed on its own thread from the decode workspace, which the job holds
// until the root has been taken: the caller checks it against the header when it needs the verdict
// (after the UTXO pass and the signatures), not when the decode returns.
struct MerkleJob {
    std::optional<DecWorkspaceLease> lease;
    std::thread th;
    std::string root;
    ~MerkleJob() {
        if (th.joinable()) th.join();
    }
    std::string result() {
        if (th.joinable()) {
            py::gil_scoped_release rel;
            th.join();
        }
        lease.reset();  // the workspace goes back to the pool
        return root;
    }
};

// A zero-copy view of a str's text (compact ASCII str objects expose their buffer).
static void str_view(PyObject* o, const char*& p, size_t& len) {
    if (!PyUnicode_Check(o)) throw py::type_error("transaction hex must be str");
    Py_ssize_t sz = 0;
    p = PyUnicode_AsUTF8AndSize(o, &sz);
    if (!p) throw py::error_already_set();
    len = size_t(sz);
}

static py::dict decode_views(const std::vector<const char*>& srcp, const std::vector<size_t>& srcl, int threads,
                             PyObject* hexes);

// decode_block_txs(hexes, threads) -> dict (see module docstring of upow_amd/ledger/fastpath.py)
static py::dict decode_block_txs(py::list hexes, int threads) {
    const size_t N = size_t(hexes.size());
    std::vector<const char*> srcp(N);
    std::vector<size_t> srcl(N);
    // the list holds a reference per str; the GIL-free pool reads only views taken here, and a copy of the
    // list (not the caller's) keeps them alive even if another thread edits the caller's list meanwhile
    py::list own = py::reinterpret_steal<py::list>(PyList_GetSlice(hexes.ptr(), 0, Py_ssize_t(N)));
    if (!own) throw py::error_already_set();
    for (size_t i = 0; i < N; ++i) str_view(PyList_GET_ITEM(own.ptr(), Py_ssize_t(i)), srcp[i], srcl[i]);
    return decode_views(srcp, srcl, threads, own.ptr());
}

// decode_block_spans(body, spans, extra, threads): the same decode for txs that are (start, length) spans
// of one request body (csrc/jsonspan.cpp), followed by the str txs of ``extra`` -- no Python str per tx.
// The returned dict has no "hex" list; "hex_fix" lists (index, canonical hex) for the txs whose text is
// not already their canonical lowercase hex (upow_amd/utils/hexspans.py builds d['hex'] from it).
static py::dict decode_block_spans(py::bytes body, py::bytes spans, py::list extra, int threads) {
    char* b = nullptr;
    Py_ssize_t blen = 0;
    if (PyBytes_AsStringAndSize(body.ptr(), &b, &blen) != 0) throw py::error_already_set();
    const std::string sp = spans;
    if (sp.size() % 16) throw py::value_error("spans: (start, length) int64 pairs");
    const size_t ns = sp.size() / 16, ne = size_t(extra.size()), N = ns + ne;
    std::vector<const char*> srcp(N);
    std::vector<size_t> srcl(N);
    for (size_t i = 0; i < ns; ++i) {
        int64_t st, ln;
        std::memcpy(&st, sp.data() + 16 * i, 8);
        std::memcpy(&ln, sp.data() + 16 * i + 8, 8);
        if (st < 0 || ln < 0 || st > blen || ln > blen - st) throw py::value_error("span outside the body");
        srcp[i] = b + st;
        srcl[i] = size_t(ln);
    }
    py::list own = py::reinterpret_steal<py::list>(PyList_GetSlice(extra.ptr(), 0, Py_ssize_t(ne)));
    if (!own) throw py::error_already_set();
    for (size_t i = 0; i < ne; ++i) str_view(PyList_GET_ITEM(own.ptr(), Py_ssize_t(i)), srcp[ns + i], srcl[ns + i]);
    return decode_views(srcp, srcl, threads, nullptr);
}

static py::dict decode_views(const std::vector<const char*>& srcp, const std::vector<size_t>& srcl, int threads,
                             PyObject* hexes) {
    const size_t N = srcp.size();
    const int64_t n = int64_t(N);
    auto job = std::make_shared<MerkleJob>();
    job->lease.emplace();
    std::vector<DecTx>& txs = job->lease->get().txs;
    if (txs.size() < N) txs.resize(N);
    const bool prof = std::getenv("UPOW_TXCODEC_PROFILE") != nullptr;
    auto t0 = std::chrono::steady_clock::now();
    // each decoding thread also writes its txs' sizes and scalars into one contiguous array: the serial passes
    // below (segment starts, arena offsets, the hex list) read that instead of every tx's scattered buffers
    struct TxSum {
        uint8_t flag, version, tx_type, grouped, canonical, upper_hex;
        int32_t n_in, n_out, n_sig, signed_len, msg_off, msg_len, canon, ajson, mjson, addr_bytes;
    };
    std::vector<TxSum> sum(N);
    {
        py::gil_scoped_release rel;
        parallel_for(n, threads, [&](int64_t i) {
            {
                DecTx& t = txs[size_t(i)];
                decode_one(srcp[size_t(i)], srcl[size_t(i)], t);
                TxSum& u = sum[size_t(i)];
                u.flag = t.flag;
                u.version = t.version;
                u.tx_type = t.tx_type;
                u.grouped = t.grouped;
                u.canonical = t.canonical;
                u.upper_hex = t.upper_hex;
                u.n_in = int32_t(t.ins.size());
                u.n_out = int32_t(t.outs.size());
                u.n_sig = int32_t(t.sigs.size() / 64);
                u.signed_len = t.signed_len;
                u.msg_off = t.msg_off;
                u.msg_len = t.msg_len;
                u.canon = int32_t(t.canon.size());
                u.ajson = int32_t(t.out_addr_json.size());
                u.mjson = int32_t(t.out_amount_json.size());
                int32_t ab = 0;  // the address strings exist for the fast-path form only
                if (t.flag == TX_FAST)
                    for (size_t j = 0; j < t.outs.size() && j < t.out_addr.size(); ++j) ab += int32_t(t.out_addr[j].size());
                u.addr_bytes = ab;
            }
        });
    }
    auto t1 = std::chrono::steady_clock::now();
    py::dict d;
    std::vector<uint8_t> flags(N), version(N), tx_type(N), grouped(N);
    std::vector<int32_t> in_start(N + 1), out_start(N + 1), sig_start(N + 1), signed_len(N), msg_off(N), msg_len(N),
        hex_len(N);
    int64_t n_in = 0, n_out = 0, n_sig = 0;
    bool all_fast = true;
    for (int64_t i = 0; i < n; ++i) {
        const TxSum& t = sum[size_t(i)];
        flags[size_t(i)] = t.flag;
        all_fast &= t.flag == TX_FAST;
        version[size_t(i)] = t.version;
        tx_type[size_t(i)] = t.tx_type;
        grouped[size_t(i)] = t.grouped;
        in_start[size_t(i)] = int32_t(n_in);
        out_start[size_t(i)] = int32_t(n_out);
        sig_start[size_t(i)] = int32_t(n_sig);
        n_in += t.n_in;
        n_out += t.n_out;
        n_sig += t.n_sig;
        signed_len[size_t(i)] = t.signed_len;
        msg_off[size_t(i)] = t.msg_off;
        msg_len[size_t(i)] = t.msg_len;
        hex_len[size_t(i)] = 2 * t.canon;
    }
    in_start[size_t(n)] = int32_t(n_in);
    out_start[size_t(n)] = int32_t(n_out);
    sig_start[size_t(n)] = int32_t(n_sig);
    auto i32 = [](const std::vector<int32_t>& v) {
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * 4);
    };
    d["n"] = n;
    d["all_fast"] = all_fast;
    d["flags"] = as_bytes(flags);
    d["version"] = as_bytes(version);
    d["tx_type"] = as_bytes(tx_type);
    d["grouped"] = as_bytes(grouped);  // per tx: signatures grouped by owner key (sig_first_in -1 until resolved)
    d["in_start"] = i32(in_start);
    d["out_start"] = i32(out_start);
    d["sig_start"] = i32(sig_start);
    d["signed_len"] = i32(signed_len);
    d["msg_off"] = i32(msg_off);
    d["msg_len"] = i32(msg_len);
    d["hex_len"] = i32(hex_len);
    if (!all_fast) return d;  // the caller takes the general path; skip building the rest

    const size_t NI = static_cast<size_t>(n_in), NO = static_cast<size_t>(n_out), NS = static_cast<size_t>(n_sig);
    // The merkle root (a sort of the canonical bytes, then one SHA-256 over the txids) runs on its own
    // thread while the pool fills the flat columns below (both only read `txs`) and beyond: the job owns
    // the thread and the workspace (an exception below joins it in the job's destructor).
    auto tM0 = std::chrono::steady_clock::now();
    {
        MerkleJob* j = job.get();
        j->th = std::thread([j, &txs, N] { j->root = merkle_of(txs, N); });
    }
    auto tM1 = std::chrono::steady_clock::now();
    // Every column is filled in place inside its final Python bytes object (allocated here, with the GIL;
    // written by the pool without it): no staging vector and no copy on the way out.
    auto pyb = [](size_t len, char*& p) {
        PyObject* o = PyBytes_FromStringAndSize(nullptr, Py_ssize_t(len));
        if (!o) throw py::error_already_set();
        p = PyBytes_AS_STRING(o);
        return py::reinterpret_steal<py::bytes>(o);
    };
    char *c_in_keys, *c_in_type, *c_sigs, *c_txid, *c_digest, *c_out_addr, *c_out_len, *c_out_type, *c_in_sig,
        *c_in_tx, *c_out_tx, *c_sig_first, *c_out_amount;
    d["in_keys"] = pyb(NI * 40, c_in_keys);
    d["in_type"] = pyb(NI, c_in_type);
    d["in_sig"] = pyb(NI * 4, c_in_sig);
    d["sig_first_in"] = pyb(NS * 4, c_sig_first);
    d["in_tx"] = pyb(NI * 4, c_in_tx);
    d["sigs"] = pyb(NS * 64, c_sigs);
    d["txid"] = pyb(N * 32, c_txid);
    d["digest"] = pyb(N * 32, c_digest);
    d["out_addr"] = pyb(NO * 64, c_out_addr);
    d["out_len"] = pyb(NO, c_out_len);
    d["out_type"] = pyb(NO, c_out_type);
    d["out_tx"] = pyb(NO * 4, c_out_tx);
    d["out_amount"] = pyb(NO * 8, c_out_amount);
    uint8_t* in_keys = reinterpret_cast<uint8_t*>(c_in_keys);
    uint8_t* in_type = reinterpret_cast<uint8_t*>(c_in_type);
    uint8_t* sigs = reinterpret_cast<uint8_t*>(c_sigs);
    uint8_t* txid = reinterpret_cast<uint8_t*>(c_txid);
    uint8_t* digest = reinterpret_cast<uint8_t*>(c_digest);
    uint8_t* out_addr = reinterpret_cast<uint8_t*>(c_out_addr);
    uint8_t* out_len = reinterpret_cast<uint8_t*>(c_out_len);
    uint8_t* out_type = reinterpret_cast<uint8_t*>(c_out_type);
    int32_t* in_sig = reinterpret_cast<int32_t*>(c_in_sig);
    int32_t* in_tx = reinterpret_cast<int32_t*>(c_in_tx);
    int32_t* out_tx = reinterpret_cast<int32_t*>(c_out_tx);
    int32_t* sig_first_in = reinterpret_cast<int32_t*>(c_sig_first);
    uint64_t* out_amount = reinterpret_cast<uint64_t*>(c_out_amount);
    // text arenas (offsets serial and cheap, blobs filled in parallel): output address strings, the two
    // per-tx JSON columns, and the canonical tx bytes (the stored tx_hex column, hex-rendered by the writer)
    // per-tx arena offsets from the summary; the per-output address offsets are written by the fill pass
    std::vector<int64_t> addr_base(N + 1), ajson_off(N + 1), mjson_off(N + 1), canon_off(N + 1);
    addr_base[0] = ajson_off[0] = mjson_off[0] = canon_off[0] = 0;
    for (size_t i = 0; i < N; ++i) {
        const TxSum& t = sum[i];
        addr_base[i + 1] = addr_base[i] + t.addr_bytes;
        ajson_off[i + 1] = ajson_off[i] + t.ajson;
        mjson_off[i + 1] = mjson_off[i] + t.mjson;
        canon_off[i + 1] = canon_off[i] + t.canon;
    }
    auto offs = [](const std::vector<int64_t>& v) {
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * 8);
    };
    char *addr_blob, *ajson_blob, *mjson_blob, *canon_blob, *addr_off_p;
    py::bytes addr_off_b = pyb((NO + 1) * 8, addr_off_p);
    int64_t* addr_off = reinterpret_cast<int64_t*>(addr_off_p);
    addr_off[0] = 0;
    d["out_addr_str"] = py::make_tuple(pyb(size_t(addr_base[N]), addr_blob), addr_off_b);
    d["out_addr_json"] = py::make_tuple(pyb(size_t(ajson_off[N]), ajson_blob), offs(ajson_off));
    d["out_amount_json"] = py::make_tuple(pyb(size_t(mjson_off[N]), mjson_blob), offs(mjson_off));
    d["canon"] = py::make_tuple(pyb(size_t(canon_off[N]), canon_blob), offs(canon_off));
    auto tF0 = std::chrono::steady_clock::now();
    {
        py::gil_scoped_release rel;
        auto fill_one = [&](int64_t ii) {  // a few small copies per tx
            const size_t i = size_t(ii);
            const DecTx& t = txs[i];
            std::memcpy(&txid[32 * i], t.txid, 32);
            std::memcpy(&digest[32 * i], t.digest, 32);
            size_t k = size_t(in_start[i]);
            int32_t k_new_sig = 0;
            for (const DecIn& in : t.ins) {
                std::memcpy(&in_keys[40 * k], in.txid, 32);
                const uint32_t idx = in.index, tag = 0xffu;
                std::memcpy(&in_keys[40 * k + 32], &idx, 4);
                std::memcpy(&in_keys[40 * k + 36], &tag, 4);
                in_type[k] = in.type;
                in_sig[k] = in.sig < 0 ? -1 : sig_start[i] + in.sig;
                // signatures are numbered in order of first use within the tx: the first input that uses
                // a signature is the one for which it is the next new number
                if (in.sig == k_new_sig) {
                    sig_first_in[size_t(sig_start[i] + in.sig)] = int32_t(k);
                    ++k_new_sig;
                }
                in_tx[k] = int32_t(i);
                ++k;
            }
            if (t.grouped)
                for (size_t g = 0; g < t.sigs.size() / 64; ++g) sig_first_in[size_t(sig_start[i]) + g] = -1;
            if (!t.sigs.empty()) std::memcpy(&sigs[64 * size_t(sig_start[i])], t.sigs.data(), t.sigs.size());
            size_t o = size_t(out_start[i]);
            int64_t a = addr_base[i];
            for (size_t j = 0; j < t.outs.size(); ++j, ++o) {
                std::memset(&out_addr[64 * o], 0, 64);
                std::memcpy(&out_addr[64 * o], t.outs[j].addr, t.outs[j].len);
                out_len[o] = t.outs[j].len;
                out_type[o] = t.outs[j].type;
                out_amount[o] = t.outs[j].amount;
                out_tx[o] = int32_t(i);
                std::memcpy(addr_blob + a, t.out_addr[j].data(), t.out_addr[j].size());
                a += int64_t(t.out_addr[j].size());
                addr_off[o + 1] = a;
            }
            std::memcpy(ajson_blob + ajson_off[i], t.out_addr_json.data(), t.out_addr_json.size());
            std::memcpy(mjson_blob + mjson_off[i], t.out_amount_json.data(), t.out_amount_json.size());
            std::memcpy(canon_blob + canon_off[i], t.canon.data(), t.canon.size());
        };
        parallel_for_grain(n, threads, 512, fill_one);
    }
    // the stored hex column as str objects (object-path parity, mempool and cluster mirroring): the input
    // string is reused when it already is the canonical lowercase hex of the tx
    auto tA = std::chrono::steady_clock::now();
    if (hexes) {
        py::list canon_hex = new_list(N);
        for (size_t i = 0; i < N; ++i) {
            const TxSum& u = sum[i];
            if (u.canonical && !u.upper_hex && srcl[i] == 2 * size_t(u.canon)) {
                PyObject* obj = PyList_GET_ITEM(hexes, Py_ssize_t(i));
                Py_INCREF(obj);
                PyList_SET_ITEM(canon_hex.ptr(), Py_ssize_t(i), obj);
            } else {
                const DecTx& t = txs[i];
                const std::string h = to_hex(t.canon.data(), t.canon.size());
                PyList_SET_ITEM(canon_hex.ptr(), Py_ssize_t(i), ascii_str(h.data(), h.size()));
            }
        }
        d["hex"] = canon_hex;
    } else {
        py::list fix;
        for (size_t i = 0; i < N; ++i) {
            const TxSum& u = sum[i];
            if (u.canonical && !u.upper_hex && srcl[i] == 2 * size_t(u.canon)) continue;
            const DecTx& t = txs[i];
            const std::string h = to_hex(t.canon.data(), t.canon.size());
            fix.append(py::make_tuple(int64_t(i), py::reinterpret_steal<py::object>(ascii_str(h.data(), h.size()))));
        }
        d["hex_fix"] = fix;
    }
    auto tB = std::chrono::steady_clock::now();
    auto t2 = std::chrono::steady_clock::now();
    d["merkle_job"] = job;
    if (prof) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[txcodec] decode %.2f ms, columns %.2f ms (fill %.2f [head %.2f, merkle spawn %.2f, "
                     "alloc %.2f, copies %.2f], hex list %.2f)\n", ms(t0, t1), ms(t1, t2), ms(t1, tA), ms(t1, tM0),
                     ms(tM0, tM1), ms(tM1, tF0), ms(tF0, tA), ms(tA, tB));
    }
    return d;
}

// A new Python bytes object of `len` bytes to be filled in place (GIL held for the allocation only).
static py::bytes new_pybytes(size_t len, char*& p) {
    PyObject* o = PyBytes_FromStringAndSize(nullptr, Py_ssize_t(len));
    if (!o) throw py::error_already_set();
    p = PyBytes_AS_STRING(o);
    return py::reinterpret_steal<py::bytes>(o);
}

template <class T>
static const T* buf_view(const py::buffer_info& bi, size_t& count) {
    const size_t total = size_t(bi.size) * size_t(bi.itemsize);
    if (total % sizeof(T)) throw std::invalid_argument("buffer size is not a multiple of its element");
    count = total / sizeof(T);
    return static_cast<const T*>(bi.ptr);
}

// tx segment starts int32[n_tx + 1] over `n_items` rows: non-decreasing, from 0, ending at n_items
static void check_starts(const int32_t* st, size_t n_tx, size_t n_items, const char* what) {
    if (st[0] != 0 || size_t(st[n_tx]) != n_items) throw std::invalid_argument(std::string(what) + ": bad segment starts");
    for (size_t t = 0; t < n_tx; ++t)
        if (st[t + 1] < st[t]) throw std::invalid_argument(std::string(what) + ": segment starts decrease");
}

// Canonical compressed address strings for spent outputs (database._input_address): 33-byte
// addresses keep x with the normalised prefix, 64-byte ones take the parity of y. Returns the
// per-tx inputs_addresses JSON column as a text arena (blob, int64 offsets[n_tx + 1]) and, with
// `per_input`, each input's string as a second arena. Every pass is parallel over the pool and writes
// straight into the result bytes; the strings live in fixed slots (no per-input allocation).
static py::tuple input_address_strings(py::buffer addrs64, py::buffer lens, py::buffer in_start_b, int threads,
                                       bool per_input) {
    const py::buffer_info abi = addrs64.request(), lbi = lens.request(), sbi = in_start_b.request();
    size_t n_a = 0, n_in = 0, n_st = 0;
    const uint8_t* a = buf_view<uint8_t>(abi, n_a);
    const uint8_t* l = buf_view<uint8_t>(lbi, n_in);
    const int32_t* st = buf_view<int32_t>(sbi, n_st);
    if (n_st < 1) throw std::invalid_argument("in_start must have n_tx + 1 entries");
    const size_t n_tx = n_st - 1;
    if (n_a != 64 * n_in) throw std::invalid_argument("addrs64 must be 64 bytes per input");
    check_starts(st, n_tx, n_in, "input_address_strings");
    struct Slot {
        char s[46];
        uint8_t len;
    };
    std::vector<Slot> out(n_in);
    std::atomic<bool> bad{false};
    {
        py::gil_scoped_release rel;
        parallel_for_grain(int64_t(n_in), threads, 2048, [&](int64_t i) {
            const uint8_t* p = a + 64 * size_t(i);
            uint8_t c[33];
            if (l[size_t(i)] == 33) {
                c[0] = p[0] == 43 ? 43 : 42;
                std::memcpy(c + 1, p + 1, 32);
            } else if (l[size_t(i)] == 64) {
                c[0] = (p[32] & 1) ? 43 : 42;  // y little-endian: parity is bit 0 of byte 32
                std::memcpy(c + 1, p, 32);
            } else {
                bad = true;
                return;
            }
            thread_local std::string scratch;
            b58_33(c, scratch);
            if (scratch.size() > sizeof(out[0].s)) {
                bad = true;
                return;
            }
            std::memcpy(out[size_t(i)].s, scratch.data(), scratch.size());
            out[size_t(i)].len = uint8_t(scratch.size());
        });
    }
    if (bad) throw std::invalid_argument("input address payload missing");
    // JSON rows: ["a","b",...] -> 2 + sum(len + 2) + (k - 1) commas (2 for an empty list)
    std::vector<int64_t> joff(n_tx + 1, 0);
    for (size_t t = 0; t < n_tx; ++t) {
        int64_t len = 2;
        for (int32_t k = st[t]; k < st[t + 1]; ++k) len += out[size_t(k)].len + 2 + (k > st[t] ? 1 : 0);
        joff[t + 1] = joff[t] + len;
    }
    char* jb;
    py::bytes jblob = new_pybytes(size_t(joff[n_tx]), jb);
    std::vector<int64_t> eoff;
    char* eb = nullptr;
    py::bytes eblob;
    if (per_input) {
        eoff.assign(n_in + 1, 0);
        for (size_t i = 0; i < n_in; ++i) eoff[i + 1] = eoff[i] + out[i].len;
        eblob = new_pybytes(size_t(eoff[n_in]), eb);
    }
    {
        py::gil_scoped_release rel;
        parallel_for_grain(int64_t(n_tx), threads, 8192, [&](int64_t t) {
            char* q = jb + joff[size_t(t)];
            *q++ = '[';
            for (int32_t k = st[t]; k < st[t + 1]; ++k) {
                if (k > st[t]) *q++ = ',';
                *q++ = '"';
                std::memcpy(q, out[size_t(k)].s, out[size_t(k)].len);
                q += out[size_t(k)].len;
                *q++ = '"';
            }
            *q = ']';
        });
        if (per_input)
            parallel_for_grain(int64_t(n_in), threads, 16384, [&](int64_t i) {
                std::memcpy(eb + eoff[size_t(i)], out[size_t(i)].s, out[size_t(i)].len);
            });
    }
    auto offs = [](const std::vector<int64_t>& v) {
        return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * 8);
    };
    if (!per_input) return py::make_tuple(jblob, offs(joff));
    return py::make_tuple(jblob, offs(joff), eblob, offs(eoff));
}

// address_transactions rows of a block's txs: every distinct address among each tx's input owners and
// output addresses (the set the reference's json_each(inputs_addresses) UNION json_each(outputs_addresses)
// yields per tx). Inputs: per-input and per-output string arenas with their tx segment starts. Returns
// (address arena blob, int64 offsets, int64 tx index per row). Two parallel passes over the txs: count
// (rows, bytes) per tx, then fill at the prefix-summed positions.
static py::tuple address_pairs(py::buffer in_blob, py::buffer in_off_b, py::buffer in_start_b, py::buffer out_blob,
                               py::buffer out_off_b, py::buffer out_start_b, int threads) {
    const py::buffer_info ibi = in_blob.request(), iobi = in_off_b.request(), isbi = in_start_b.request(),
                          obi = out_blob.request(), oobi = out_off_b.request(), osbi = out_start_b.request();
    size_t ib_n, io_n, is_n, ob_n, oo_n, os_n;
    const char* ib = buf_view<char>(ibi, ib_n);
    const int64_t* ioff = buf_view<int64_t>(iobi, io_n);
    const int32_t* ist = buf_view<int32_t>(isbi, is_n);
    const char* ob = buf_view<char>(obi, ob_n);
    const int64_t* ooff = buf_view<int64_t>(oobi, oo_n);
    const int32_t* ost = buf_view<int32_t>(osbi, os_n);
    if (is_n < 1 || os_n != is_n) throw std::invalid_argument("address_pairs: tx counts differ");
    if (io_n < 1 || oo_n < 1) throw std::invalid_argument("address_pairs: empty offsets");
    const size_t n = is_n - 1, n_in = io_n - 1, n_out = oo_n - 1;
    check_starts(ist, n, n_in, "address_pairs inputs");
    check_starts(ost, n, n_out, "address_pairs outputs");
    auto check_off = [](const int64_t* off, size_t m, size_t blen) {
        if (off[0] < 0) throw std::invalid_argument("address_pairs: negative offset");
        for (size_t j = 0; j < m; ++j)
            if (off[j + 1] < off[j]) throw std::invalid_argument("address_pairs: offsets decrease");
        if (size_t(off[m]) > blen) throw std::invalid_argument("address_pairs: offsets past the blob");
    };
    check_off(ioff, n_in, ib_n);
    check_off(ooff, n_out, ob_n);
    // the distinct strings of tx k in first-seen order, as (blob, offset index) pairs
    auto each_distinct = [&](size_t k, auto&& emit) {
        std::string_view seen[64];
        size_t n_seen = 0;
        std::vector<std::string_view> more;  // txs with more than 64 distinct addresses (rare)
        auto take = [&](std::string_view v) {
            for (size_t q = 0; q < n_seen; ++q)
                if (seen[q] == v) return;
            for (auto& w : more)
                if (w == v) return;
            if (n_seen < 64) seen[n_seen++] = v;
            else more.push_back(v);
            emit(v);
        };
        for (int64_t j = ist[k]; j < ist[k + 1]; ++j) take(std::string_view(ib + ioff[j], size_t(ioff[j + 1] - ioff[j])));
        for (int64_t o = ost[k]; o < ost[k + 1]; ++o) take(std::string_view(ob + ooff[o], size_t(ooff[o + 1] - ooff[o])));
    };
    std::vector<int64_t> rows(n + 1, 0), bytes(n + 1, 0);
    {
        py::gil_scoped_release rel;
        parallel_for_grain(int64_t(n), threads, 512, [&](int64_t k) {
            int64_t r = 0, b = 0;
            each_distinct(size_t(k), [&](std::string_view v) {
                ++r;
                b += int64_t(v.size());
            });
            rows[size_t(k) + 1] = r;
            bytes[size_t(k) + 1] = b;
        });
    }
    for (size_t k = 0; k < n; ++k) {
        rows[k + 1] += rows[k];
        bytes[k + 1] += bytes[k];
    }
    const size_t R = size_t(rows[n]);
    char *blob, *offp, *txp;
    py::bytes blob_b = new_pybytes(size_t(bytes[n]), blob), off_b = new_pybytes((R + 1) * 8, offp),
              tx_b = new_pybytes(R * 8, txp);
    int64_t* off = reinterpret_cast<int64_t*>(offp);
    int64_t* tx = reinterpret_cast<int64_t*>(txp);
    off[0] = 0;
    {
        py::gil_scoped_release rel;
        parallel_for_grain(int64_t(n), threads, 512, [&](int64_t k) {
            int64_t r = rows[size_t(k)], b = bytes[size_t(k)];
            each_distinct(size_t(k), [&](std::string_view v) {
                std::memcpy(blob + b, v.data(), v.size());
                b += int64_t(v.size());
                off[r + 1] = b;
                tx[r] = k;
                ++r;
            });
        });
    }
    return py::make_tuple(blob_b, off_b, tx_b);
}

// ---- column helpers for the bulk ledger writes (ledger/fastpath.py)

// numeric(Decimal(fee) / 10**8, 6): fee in smallest units rounded half up to 6 decimals, as a text arena
// (blob, int64 offsets[n + 1]) that the bulk ledger writer binds directly
static py::tuple fee_strings(py::bytes fee_b) {
    std::string f = fee_b;
    const int64_t* v = reinterpret_cast<const int64_t*>(f.data());
    const size_t n = f.size() / 8;
    Arena out;
    out.blob.reserve(n * 12);
    out.off.reserve(n + 1);
    for (size_t i = 0; i < n; ++i) {
        if (v[i] < 0) throw std::invalid_argument("negative fee");
        const uint64_t q = uint64_t(v[i] + 50) / 100;
        char buf[32];
        char* e = buf + sizeof(buf);
        char* p = e;
        uint64_t frac = q % 1000000, whole = q / 1000000;
        for (int k = 0; k < 6; ++k) {
            *--p = char('0' + frac % 10);
            frac /= 10;
        }
        *--p = '.';
        do {
            *--p = char('0' + whole % 10);
            whole /= 10;
        } while (whole);
        out.add(p, size_t(e - p));
    }
    return out.py();
}

// Distinct rows of an (n x width) byte matrix: (unique rows in first-seen order, inverse int32[n]).
// Replaces np.unique over a void dtype (a full sort of opaque records) for the per-block public-key
// set: open addressing keyed by the row's leading bytes after the prefix (P-256 x coordinates are
// uniformly distributed, so they are a good hash as they are).
static py::tuple unique_rows(py::buffer buf, int width) {
    py::buffer_info bi = buf.request();
    const size_t total = size_t(bi.size) * size_t(bi.itemsize);
    if (width <= 0 || total % size_t(width)) throw std::invalid_argument("buffer is not n x width bytes");
    const size_t n = total / size_t(width);
    const uint8_t* d = static_cast<const uint8_t*>(bi.ptr);
    size_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    std::vector<int32_t> slot(cap, -1);
    std::vector<int32_t> inv(n), first;
    first.reserve(n);
    {
        py::gil_scoped_release nogil;
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* r = d + i * size_t(width);
            uint64_t h = 1469598103934665603ull;
            for (int k = 0; k < width; ++k) h = (h ^ r[k]) * 1099511628211ull;
            size_t s = size_t(h) & (cap - 1);
            for (;;) {
                const int32_t u = slot[s];
                if (u < 0) {
                    slot[s] = int32_t(first.size());
                    inv[i] = int32_t(first.size());
                    first.push_back(int32_t(i));
                    break;
                }
                if (std::memcmp(d + size_t(first[size_t(u)]) * size_t(width), r, size_t(width)) == 0) {
                    inv[i] = u;
                    break;
                }
                s = (s + 1) & (cap - 1);
            }
        }
    }
    std::string uniq(first.size() * size_t(width), '\0');
    for (size_t u = 0; u < first.size(); ++u)
        std::memcpy(&uniq[u * size_t(width)], d + size_t(first[u]) * size_t(width), size_t(width));
    return py::make_tuple(py::bytes(uniq), py::bytes(reinterpret_cast<const char*>(inv.data()), inv.size() * 4));
}

// The key + record stage of the native block path (ledger/fastpath.py) in one call: every 33-byte
// address of the block (spent outputs' owners and new outputs) is deduplicated, the distinct keys are
// decompressed in one batch (GPU when there are at least `gpu_min` of them), and the 160-byte verify
// records [x | y | r | s | digest] of the signature jobs are assembled from the signers' points.
// Returns (1, records) when every key is a curve point, (0, b"") when one is not, and (-1, b"") when an
// address is not in the 33-byte form (64-byte keys: the caller's general path checks those).
// `over_idx` / `over_addr` (optional): inputs whose signer is not the spent output's owner (revokes are signed
// by the voter, ledger/govcheck.py): input over_idx[k] takes the 64-byte address row over_addr[k] (+ its
// length over_len[k]) instead of its pay row, without the caller copying the whole payload column.
static py::tuple block_signer_records(py::buffer pay_addr_b, py::buffer pay_len_b, py::buffer out_addr_b,
                                      py::buffer out_len_b, py::buffer job_input_b, py::buffer sigs_b,
                                      py::buffer sig_ids_b, py::buffer digest_b, py::buffer job_tx_b, int64_t gpu_min,
                                      py::object over_idx_o, py::object over_addr_o, py::object over_len_o) {
    auto view = [](py::buffer& b, size_t elem, const char* what) {
        py::buffer_info bi = b.request();
        const size_t total = size_t(bi.size) * size_t(bi.itemsize);
        if (total % elem) throw std::invalid_argument(std::string(what) + ": size is not a multiple of its row");
        return std::make_pair(static_cast<const uint8_t*>(bi.ptr), total / elem);
    };
    const auto [pay_addr, n_in] = view(pay_addr_b, 64, "pay_addr");
    const auto [pay_len, n_in2] = view(pay_len_b, 1, "pay_len");
    const auto [out_addr, n_out] = view(out_addr_b, 64, "out_addr");
    const auto [out_len, n_out2] = view(out_len_b, 1, "out_len");
    const auto [job_input_p, n_jobs] = view(job_input_b, 8, "job_input");
    const auto [sigs, n_sig] = view(sigs_b, 64, "sigs");
    const auto [sig_ids_p, n_jobs2] = view(sig_ids_b, 8, "sig_ids");
    const auto [digest, n_tx] = view(digest_b, 32, "digest");
    const auto [job_tx_p, n_jobs3] = view(job_tx_b, 8, "job_tx");
    if (n_in != n_in2 || n_out != n_out2 || n_jobs != n_jobs2 || n_jobs != n_jobs3)
        throw std::invalid_argument("block_signer_records: column lengths differ");
    const int64_t* job_input = reinterpret_cast<const int64_t*>(job_input_p);
    const int64_t* sig_ids = reinterpret_cast<const int64_t*>(sig_ids_p);
    const int64_t* job_tx = reinterpret_cast<const int64_t*>(job_tx_p);
    std::vector<const uint8_t*> over(n_in, nullptr);  // per input: its override row, if any
    std::vector<uint8_t> over_len_of(n_in, 0);
    if (!over_idx_o.is_none()) {
        py::buffer oi_b = over_idx_o.cast<py::buffer>(), oa_b = over_addr_o.cast<py::buffer>(),
                   ol_b = over_len_o.cast<py::buffer>();
        const auto [oi_p, n_o] = view(oi_b, 8, "over_idx");
        const auto [oa_p, n_o2] = view(oa_b, 64, "over_addr");
        const auto [ol_p, n_o3] = view(ol_b, 1, "over_len");
        if (n_o != n_o2 || n_o != n_o3) throw std::invalid_argument("block_signer_records: override lengths differ");
        const int64_t* oi = reinterpret_cast<const int64_t*>(oi_p);
        for (size_t k = 0; k < n_o; ++k) {
            if (oi[k] < 0 || size_t(oi[k]) >= n_in) throw std::invalid_argument("block_signer_records: override index");
            over[size_t(oi[k])] = oa_p + 64 * k;
            over_len_of[size_t(oi[k])] = ol_p[k];
        }
    }
    for (size_t i = 0; i < n_in; ++i)
        if ((over[i] ? over_len_of[i] : pay_len[i]) != 33) return py::make_tuple(-1, py::bytes());
    for (size_t i = 0; i < n_out; ++i)
        if (out_len[i] != 33) return py::make_tuple(-1, py::bytes());
    for (size_t j = 0; j < n_jobs; ++j)
        if (job_input[j] < 0 || size_t(job_input[j]) >= n_in || sig_ids[j] < 0 || size_t(sig_ids[j]) >= n_sig ||
            job_tx[j] < 0 || size_t(job_tx[j]) >= n_tx)
            throw std::invalid_argument("block_signer_records: job index out of range");
    std::vector<uint8_t> uniq;     // U x 33 distinct keys
    std::vector<int32_t> pay_uid(n_in);
    std::vector<uint8_t> xy, okb;  // U x 64, U
    std::string recs(n_jobs * 160, '\0');
    bool all_ok = true;
    {
        py::gil_scoped_release nogil;
        const size_t n = n_in + n_out;
        size_t cap = 16;
        while (cap < 2 * n) cap <<= 1;
        std::vector<int32_t> slot(cap, -1);
        std::vector<const uint8_t*> first;
        auto key_of = [&](size_t i) {
            return i < n_in ? (over[i] ? over[i] : pay_addr + 64 * i) : out_addr + 64 * (i - n_in);
        };
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* r = key_of(i);
            uint64_t w[4];
            std::memcpy(w, r + 1, 32);
            uint64_t h = (w[0] * 0x9E3779B97F4A7C15ull) ^ (w[1] * 0xC2B2AE3D27D4EB4Full) ^
                         (w[2] * 0x165667B19E3779F9ull) ^ (w[3] * 0x27D4EB2F165667C5ull) ^ r[0];
            h ^= h >> 29;
            size_t sl = size_t(h) & (cap - 1);
            int32_t uid;
            for (;;) {
                const int32_t u = slot[sl];
                if (u < 0) {
                    uid = int32_t(first.size());
                    slot[sl] = uid;
                    first.push_back(r);
                    break;
                }
                if (std::memcmp(first[size_t(u)], r, 33) == 0) {
                    uid = u;
                    break;
                }
                sl = (sl + 1) & (cap - 1);
            }
            if (i < n_in) pay_uid[i] = uid;
        }
        const size_t U = first.size();
        uniq.resize(U * 33);
        for (size_t u = 0; u < U; ++u) std::memcpy(&uniq[33 * u], first[u], 33);
        xy.resize(U * 64);
        okb.resize(U);
        if (U) {
            if (int64_t(U) >= gpu_min) p256_decompress_gpu(uniq.data(), int64_t(U), xy.data(), okb.data());
            else p256_decompress_host(uniq.data(), int64_t(U), xy.data(), okb.data());
        }
        for (size_t u = 0; u < U; ++u) all_ok &= okb[u] != 0;
        if (all_ok) {
            for (size_t j = 0; j < n_jobs; ++j) {
                char* rec = &recs[160 * j];
                std::memcpy(rec, &xy[64 * size_t(pay_uid[size_t(job_input[j])])], 64);
                std::memcpy(rec + 64, sigs + 64 * size_t(sig_ids[j]), 64);
                std::memcpy(rec + 128, digest + 32 * size_t(job_tx[j]), 32);
            }
        }
    }
    if (!all_ok) return py::make_tuple(0, py::bytes());
    return py::make_tuple(1, py::bytes(recs));
}

// The key + verify stages of the native block path fused on the GPU (csrc/p256.hip p256_verify_fused_gpu): the
// signer keys go to the device compressed and are decompressed into the verify items there, next to the
// curve check of every other 33-byte address of the block (spent outputs' owners and new outputs), and the
// verify runs behind them in the same stream order -- no host deduplication, no decompressed keys coming
// back, no host record assembly, one sync. Same verdicts as block_signer_records + p256_verify: a signer key
// off the curve gives status 2 (bad key), any other address off the curve gives all_ok False.
// Returns (-1, b"", False, None) when an address is not in the 33-byte form (the caller's general path),
// else (1, status bytes, all addresses on the curve, verify items when a status is INVALID (0) else None).
static py::tuple block_verify_fused(py::buffer pay_addr_b, py::buffer pay_len_b, py::buffer out_addr_b,
                                    py::buffer out_len_b, py::buffer job_input_b, py::buffer sigs_b, py::buffer sig_ids_b,
                                    py::buffer digest_b, py::buffer job_tx_b, int threads, bool gpu) {
    auto view = [](py::buffer& b, size_t elem, const char* what) {
        py::buffer_info bi = b.request();
        const size_t total = size_t(bi.size) * size_t(bi.itemsize);
        if (total % elem) throw std::invalid_argument(std::string(what) + ": size is not a multiple of its row");
        return std::make_pair(static_cast<const uint8_t*>(bi.ptr), total / elem);
    };
    const auto [pay_addr, n_in] = view(pay_addr_b, 64, "pay_addr");
    const auto [pay_len, n_in2] = view(pay_len_b, 1, "pay_len");
    const auto [out_addr, n_out] = view(out_addr_b, 64, "out_addr");
    const auto [out_len, n_out2] = view(out_len_b, 1, "out_len");
    const auto [job_input_p, n_jobs] = view(job_input_b, 8, "job_input");
    const auto [sigs, n_sig] = view(sigs_b, 64, "sigs");
    const auto [sig_ids_p, n_jobs2] = view(sig_ids_b, 8, "sig_ids");
    const auto [digest, n_tx] = view(digest_b, 32, "digest");
    const auto [job_tx_p, n_jobs3] = view(job_tx_b, 8, "job_tx");
    if (n_in != n_in2 || n_out != n_out2 || n_jobs != n_jobs2 || n_jobs != n_jobs3)
        throw std::invalid_argument("block_verify_fused: column lengths differ");
    const int64_t* job_input = reinterpret_cast<const int64_t*>(job_input_p);
    const int64_t* sig_ids = reinterpret_cast<const int64_t*>(sig_ids_p);
    const int64_t* job_tx = reinterpret_cast<const int64_t*>(job_tx_p);
    for (size_t i = 0; i < n_in; ++i)
        if (pay_len[i] != 33) return py::make_tuple(-1, py::bytes(), false, py::none());
    for (size_t i = 0; i < n_out; ++i)
        if (out_len[i] != 33) return py::make_tuple(-1, py::bytes(), false, py::none());
    for (size_t j = 0; j < n_jobs; ++j)
        if (job_input[j] < 0 || size_t(job_input[j]) >= n_in || sig_ids[j] < 0 || size_t(sig_ids[j]) >= n_sig ||
            job_tx[j] < 0 || size_t(job_tx[j]) >= n_tx)
            throw std::invalid_argument("block_verify_fused: job index out of range");
    std::string st(n_jobs, '\0');
    std::vector<uint8_t> ok(n_in + n_out), items;
    {
        py::gil_scoped_release nogil;
        const size_t nj = n_jobs, nc = n_in + n_out;
        auto fill = [&](uint8_t* keys, uint8_t* sigdig, uint8_t* checks) {
            // every job and every checked address in parallel: 2 MB of small gathers into pinned memory
            parallel_for(int64_t(nj + nc), threads, [&](int64_t ii) {
                const size_t i = size_t(ii);
                if (i < nj) {
                    std::memcpy(keys + 33 * i, pay_addr + 64 * size_t(job_input[i]), 33);
                    std::memcpy(sigdig + 96 * i, sigs + 64 * size_t(sig_ids[i]), 64);
                    std::memcpy(sigdig + 96 * i + 64, digest + 32 * size_t(job_tx[i]), 32);
                } else {
                    const size_t c = i - nj;
                    std::memcpy(checks + 33 * c, c < n_in ? pay_addr + 64 * c : out_addr + 64 * (c - n_in), 33);
                }
            });
        };
        if (gpu) {
            p256_verify_fused_gpu(int64_t(nj), int64_t(nc), fill, reinterpret_cast<uint8_t*>(&st[0]), ok.data(), &items);
        } else {  // the same stages on the host (CPU tests of the packing and the verdicts)
            std::vector<uint8_t> in(129 * nj + 33 * nc), xy(64 * (nj + nc)), kok(nj + nc);
            fill(in.data(), in.data() + 33 * nj, in.data() + 129 * nj);
            std::vector<uint8_t> keys(33 * (nj + nc));
            std::memcpy(keys.data(), in.data(), 33 * nj);
            std::memcpy(keys.data() + 33 * nj, in.data() + 129 * nj, 33 * nc);
            p256_decompress_host(keys.data(), int64_t(nj + nc), xy.data(), kok.data());
            std::vector<uint8_t> rec(160 * nj, 0);
            for (size_t j = 0; j < nj; ++j) {
                if (kok[j]) std::memcpy(&rec[160 * j], &xy[64 * j], 64);
                std::memcpy(&rec[160 * j + 64], in.data() + 33 * nj + 96 * j, 96);
            }
            const std::vector<uint8_t> hs = p256_verify_host(rec.data(), int64_t(nj), std::max(1, threads));
            std::memcpy(&st[0], hs.data(), nj);
            std::memcpy(ok.data(), kok.data() + nj, nc);
            if (std::find(hs.begin(), hs.end(), uint8_t(0)) != hs.end()) items = std::move(rec);
        }
    }
    bool all_ok = true;
    for (uint8_t f : ok) all_ok &= f != 0;
    py::object it = items.empty() ? py::object(py::none())
                                  : py::object(py::bytes(reinterpret_cast<const char*>(items.data()), items.size()));
    return py::make_tuple(1, py::bytes(st), all_ok, it);
}

// HBM index records of a block's created outputs: 40-byte keys (txid | index u32 | table tag u32) and
// 80-byte payloads (amount u64 | address length u32 | flags u32 | address, prefix normalised as
// bytes_to_string does) in one pass, instead of a dozen numpy passes over the block's outputs.
static py::tuple output_index_records(py::buffer txid_b, py::buffer index_b, py::buffer tag_b, py::buffer amount_b,
                                      py::buffer addr_b, py::buffer len_b, py::buffer stake_b) {
    const py::buffer_info ti = txid_b.request(), ii = index_b.request(), gi = tag_b.request(), ai = amount_b.request(),
                          di = addr_b.request(), li = len_b.request(), si = stake_b.request();
    size_t n_t, n_i, n_g, n_a, n_d, n_l, n_s;
    const uint8_t* txid = buf_view<uint8_t>(ti, n_t);
    const int64_t* idx = buf_view<int64_t>(ii, n_i);
    const uint32_t* tag = buf_view<uint32_t>(gi, n_g);
    const uint64_t* amount = buf_view<uint64_t>(ai, n_a);
    const uint8_t* addr = buf_view<uint8_t>(di, n_d);
    const uint8_t* len = buf_view<uint8_t>(li, n_l);
    const uint8_t* stake = buf_view<uint8_t>(si, n_s);
    const size_t n = n_i;
    if (n_t != 32 * n || n_g != n || n_a != n || n_d != 64 * n || n_l != n || (n_s && n_s != n))
        throw std::invalid_argument("output_index_records: column lengths differ");
    char *rp, *pp;
    py::bytes recs = new_pybytes(40 * n, rp), pay = new_pybytes(80 * n, pp);
    {
        py::gil_scoped_release rel;
        for (size_t o = 0; o < n; ++o) {
            uint8_t* r = reinterpret_cast<uint8_t*>(rp) + 40 * o;
            std::memcpy(r, txid + 32 * o, 32);
            const uint32_t ix = uint32_t(idx[o]);
            std::memcpy(r + 32, &ix, 4);
            std::memcpy(r + 36, &tag[o], 4);
            uint8_t* q = reinterpret_cast<uint8_t*>(pp) + 80 * o;
            std::memcpy(q, &amount[o], 8);
            const uint32_t l = len[o], fl = (n_s && stake[o]) ? 1u : 0u;
            std::memcpy(q + 8, &l, 4);
            std::memcpy(q + 12, &fl, 4);
            std::memcpy(q + 16, addr + 64 * o, 64);
            if (l == 33) q[16] = q[16] == 43 ? 43 : 42;
        }
    }
    return py::make_tuple(recs, pay);
}

// the block's spent outpoints as erase records (the codec's input keys with each input's table tag) and
// their output indexes as int64
static py::tuple spent_index_records(py::buffer keys_b, py::buffer tag_b) {
    const py::buffer_info ki = keys_b.request(), gi = tag_b.request();
    size_t n_k, n_g;
    const uint8_t* keys = buf_view<uint8_t>(ki, n_k);
    const uint32_t* tag = buf_view<uint32_t>(gi, n_g);
    if (n_k != 40 * n_g) throw std::invalid_argument("spent_index_records: 40-byte keys, one tag per key");
    char *sp, *ip;
    py::bytes spent = new_pybytes(n_k, sp), idx = new_pybytes(8 * n_g, ip);
    {
        py::gil_scoped_release rel;
        for (size_t j = 0; j < n_g; ++j) {
            uint8_t* r = reinterpret_cast<uint8_t*>(sp) + 40 * j;
            std::memcpy(r, keys + 40 * j, 36);
            std::memcpy(r + 36, &tag[j], 4);
            uint32_t ix;
            std::memcpy(&ix, keys + 40 * j + 32, 4);
            const int64_t v = ix;
            std::memcpy(ip + 8 * j, &v, 8);
        }
    }
    return py::make_tuple(spent, idx);
}

// Cluster op frames (upow_amd/parallel/cluster.py pack_txs / unpack_txs): a block's tx hex strings as raw
// bytes, u32 count then u32 length + bytes per tx, hex-decoded on the host pool without the GIL; and back
// to lower-case hex strings on the follower. A string that is not even-length hex raises ValueError.
// The frame of pack_tx_hexes from text views (the caller keeps the text alive).
static py::bytes pack_views(const std::vector<const char*>& ptr, const std::vector<size_t>& hexlen, int threads) {
    const size_t n = ptr.size();
    std::vector<size_t> len(n), off(n + 1);
    off[0] = 4;
    for (size_t i = 0; i < n; ++i) {
        if (hexlen[i] % 2) throw py::value_error("tx hex of odd length");
        len[i] = hexlen[i] / 2;
        off[i + 1] = off[i] + 4 + len[i];
    }
    char* out = nullptr;
    py::bytes res = new_pybytes(off[n], out);
    const uint32_t cnt = uint32_t(n);
    std::memcpy(out, &cnt, 4);
    std::atomic<bool> bad{false};
    {
        py::gil_scoped_release nogil;
        parallel_for(int64_t(n), threads, [&](int64_t i) {
            uint8_t* d = reinterpret_cast<uint8_t*>(out) + off[size_t(i)];
            const uint32_t l = uint32_t(len[size_t(i)]);
            std::memcpy(d, &l, 4);
            const uint8_t* h = reinterpret_cast<const uint8_t*>(ptr[size_t(i)]);
            uint8_t acc = 0;
            for (size_t j = 0; j < l; ++j) {
                const uint8_t hi = kHexTab[h[2 * j]], lo = kHexTab[h[2 * j + 1]];
                acc |= hi | lo;
                d[4 + j] = uint8_t(hi << 4 | (lo & 15));
            }
            if (acc & 0x80) bad.store(true, std::memory_order_relaxed);
        });
    }
    if (bad.load()) throw py::value_error("tx hex holds a non-hex character");
    return res;
}

static py::bytes pack_tx_hexes(py::list hexes, int threads) {
    const size_t n = hexes.size();
    std::vector<const char*> ptr(n);
    std::vector<size_t> len(n);
    py::list own = py::reinterpret_steal<py::list>(PyList_GetSlice(hexes.ptr(), 0, Py_ssize_t(n)));
    if (!own) throw py::error_already_set();
    for (size_t i = 0; i < n; ++i) str_view(PyList_GET_ITEM(own.ptr(), Py_ssize_t(i)), ptr[i], len[i]);
    return pack_views(ptr, len, threads);  // `own` keeps the str objects alive
}

// pack_tx_hexes for txs given as (start, length) spans of one body, then the str txs of ``extra``.
static py::bytes pack_tx_spans(py::bytes body, py::bytes spans, py::list extra, int threads) {
    char* b = nullptr;
    Py_ssize_t blen = 0;
    if (PyBytes_AsStringAndSize(body.ptr(), &b, &blen) != 0) throw py::error_already_set();
    const std::string sp = spans;
    if (sp.size() % 16) throw py::value_error("spans: (start, length) int64 pairs");
    const size_t ns = sp.size() / 16, ne = size_t(extra.size());
    std::vector<const char*> ptr(ns + ne);
    std::vector<size_t> len(ns + ne);
    for (size_t i = 0; i < ns; ++i) {
        int64_t st, ln;
        std::memcpy(&st, sp.data() + 16 * i, 8);
        std::memcpy(&ln, sp.data() + 16 * i + 8, 8);
        if (st < 0 || ln < 0 || st > blen || ln > blen - st) throw py::value_error("span outside the body");
        ptr[i] = b + st;
        len[i] = size_t(ln);
    }
    py::list own = py::reinterpret_steal<py::list>(PyList_GetSlice(extra.ptr(), 0, Py_ssize_t(ne)));
    if (!own) throw py::error_already_set();
    for (size_t i = 0; i < ne; ++i) str_view(PyList_GET_ITEM(own.ptr(), Py_ssize_t(i)), ptr[ns + i], len[ns + i]);
    return pack_views(ptr, len, threads);
}

static py::list unpack_tx_hexes(py::bytes frame, int threads) {
    char* p = nullptr;
    Py_ssize_t total = 0;
    PyBytes_AsStringAndSize(frame.ptr(), &p, &total);
    const size_t nb = size_t(total);
    if (nb < 4) throw py::value_error("cluster frame: short tx list");
    uint32_t cnt;
    std::memcpy(&cnt, p, 4);
    std::vector<size_t> off, len;
    size_t at = 4;
    for (uint32_t i = 0; i < cnt; ++i) {
        if (nb - at < 4) throw py::value_error("cluster frame: truncated tx list");
        uint32_t l;
        std::memcpy(&l, p + at, 4);
        if (nb - at - 4 < l) throw py::value_error("cluster frame: truncated tx");
        off.push_back(at + 4);
        len.push_back(l);
        at += 4 + size_t(l);
    }
    if (at != nb) throw py::value_error("cluster frame: trailing bytes after the tx list");
    py::list out = new_list(cnt);
    std::vector<PyObject*> strs(cnt);
    for (uint32_t i = 0; i < cnt; ++i) {
        strs[i] = PyUnicode_New(Py_ssize_t(2 * len[i]), 127);
        if (!strs[i]) throw py::error_already_set();
        PyList_SET_ITEM(out.ptr(), Py_ssize_t(i), strs[i]);  // the list owns it from here
    }
    std::vector<char*> dst(cnt);
    for (uint32_t i = 0; i < cnt; ++i) dst[i] = static_cast<char*>(PyUnicode_DATA(strs[i]));
    {
        py::gil_scoped_release nogil;
        parallel_for(int64_t(cnt), threads, [&](int64_t i) {
            const uint8_t* b = reinterpret_cast<const uint8_t*>(p) + off[size_t(i)];
            char* h = dst[size_t(i)];
            for (size_t j = 0; j < len[size_t(i)]; ++j) {
                h[2 * j] = kHex[b[j] >> 4];
                h[2 * j + 1] = kHex[b[j] & 15];
            }
        });
    }
    return out;
}

// Signature -> input assignment of grouped txs (1 < k < n signatures, reference transaction.py:578-590),
// the block path's `_resolve_groups`: each listed tx's inputs grouped by owner key (x and the parity of y:
// a 33-byte address's prefix 43 = odd, anything else even; a 64-byte address's y byte 0) in order of first
// appearance; signature g's verify job is group g's first input. Returns the updated job_input column
// (int64) or None when some tx's group count differs from its signature count or its tx type is not
// REGULAR (the object path decides those).
static py::object resolve_groups(py::buffer grouped_b, py::buffer in_start_b, py::buffer sig_start_b, py::buffer tx_type_b,
                                 py::buffer pay_addr_b, py::buffer pay_len_b, py::buffer job_input_b) {
    auto view = [](py::buffer& b) { return b.request(); };
    const py::buffer_info gi = view(grouped_b), isi = view(in_start_b), ssi = view(sig_start_b), tti = view(tx_type_b),
                          pai = view(pay_addr_b), pli = view(pay_len_b), jii = view(job_input_b);
    if (gi.itemsize != 8 || isi.itemsize != 4 || ssi.itemsize != 4 || tti.itemsize != 1 || jii.itemsize != 8 ||
        pli.itemsize != 1)
        throw std::invalid_argument("resolve_groups: column types");
    const size_t n_tx = size_t(tti.size), n_in = size_t(pli.size), n_jobs = size_t(jii.size);
    if (size_t(isi.size) != n_tx + 1 || size_t(ssi.size) != n_tx + 1 || size_t(pai.size * pai.itemsize) != 64 * n_in)
        throw std::invalid_argument("resolve_groups: column lengths");
    const int64_t* grouped = static_cast<const int64_t*>(gi.ptr);
    const int32_t* in_start = static_cast<const int32_t*>(isi.ptr);
    const int32_t* sig_start = static_cast<const int32_t*>(ssi.ptr);
    const uint8_t* tx_type = static_cast<const uint8_t*>(tti.ptr);
    const uint8_t* pay_addr = static_cast<const uint8_t*>(pai.ptr);
    const uint8_t* pay_len = static_cast<const uint8_t*>(pli.ptr);
    std::vector<int64_t> jobs(static_cast<const int64_t*>(jii.ptr), static_cast<const int64_t*>(jii.ptr) + n_jobs);
    bool ok = true;
    {
        py::gil_scoped_release nogil;
        std::vector<std::array<uint8_t, 33>> keys;
        std::vector<int64_t> first;
        for (ssize_t g = 0; g < gi.size && ok; ++g) {
            const int64_t t = grouped[g];
            if (t < 0 || size_t(t) >= n_tx || tx_type[t] != 0) {
                ok = false;
                break;
            }
            keys.clear();
            first.clear();
            for (int32_t j = in_start[t]; j < in_start[t + 1]; ++j) {
                if (j < 0 || size_t(j) >= n_in) throw std::invalid_argument("resolve_groups: input index");
                const uint8_t* a = pay_addr + 64 * size_t(j);
                std::array<uint8_t, 33> k;
                if (pay_len[j] == 33) {
                    std::memcpy(k.data(), a + 1, 32);
                    k[32] = a[0] == 43 ? 1 : 0;
                } else {
                    std::memcpy(k.data(), a, 32);
                    k[32] = a[32] & 1;
                }
                bool seen = false;
                for (auto& q : keys)
                    if (q == k) {
                        seen = true;
                        break;
                    }
                if (!seen) {
                    keys.push_back(k);
                    first.push_back(j);
                }
            }
            const int32_t s0 = sig_start[t], s1 = sig_start[t + 1];
            if (int64_t(first.size()) != int64_t(s1 - s0) || s0 < 0 || size_t(s1) > n_jobs) {
                ok = false;
                break;
            }
            for (int32_t q = s0; q < s1; ++q) jobs[size_t(q)] = first[size_t(q - s0)];
        }
    }
    if (!ok) return py::none();
    return py::bytes(reinterpret_cast<const char*>(jobs.data()), jobs.size() * 8);
}

void register_txcodec(py::module_& m) {
    m.def("resolve_groups", &resolve_groups, py::arg("grouped"), py::arg("in_start"), py::arg("sig_start"),
          py::arg("tx_type"), py::arg("pay_addr"), py::arg("pay_len"), py::arg("job_input"));
    m.def("pack_tx_hexes", &pack_tx_hexes, py::arg("hexes"), py::arg("threads") = 8);
    m.def("pack_tx_spans", &pack_tx_spans, py::arg("body"), py::arg("spans"), py::arg("extra"), py::arg("threads") = 8);
    m.def("unpack_tx_hexes", &unpack_tx_hexes, py::arg("frame"), py::arg("threads") = 8);
    m.def("output_index_records", &output_index_records, py::arg("txid"), py::arg("index"), py::arg("tag"),
          py::arg("amount"), py::arg("addr"), py::arg("len"), py::arg("stake"));
    m.def("spent_index_records", &spent_index_records, py::arg("keys"), py::arg("tag"));
    py::class_<MerkleJob, std::shared_ptr<MerkleJob>>(m, "MerkleJob")
        .def("result", &MerkleJob::result, "the block's merkle root (hex); waits for the merkle thread");
    m.def("fee_strings", &fee_strings);
    m.def("unique_rows", &unique_rows, py::arg("buf"), py::arg("width"),
          "(unique rows in first-seen order, inverse int32) of an n x width byte matrix");
    m.def("block_signer_records", &block_signer_records, py::arg("pay_addr"), py::arg("pay_len"), py::arg("out_addr"),
          py::arg("out_len"), py::arg("job_input"), py::arg("sigs"), py::arg("sig_ids"), py::arg("digest"),
          py::arg("job_tx"), py::arg("gpu_min"), py::arg("over_idx") = py::none(), py::arg("over_addr") = py::none(),
          py::arg("over_len") = py::none());
    m.def("block_verify_fused", &block_verify_fused, py::arg("pay_addr"), py::arg("pay_len"), py::arg("out_addr"),
          py::arg("out_len"), py::arg("job_input"), py::arg("sigs"), py::arg("sig_ids"), py::arg("digest"),
          py::arg("job_tx"), py::arg("threads") = 8, py::arg("gpu") = true);
    m.def("decode_block_txs", &decode_block_txs, py::arg("hexes"), py::arg("threads") = 8,
          "Decode, canonicalise and hash a block's transactions (see csrc/txcodec.cpp)");
    m.def("decode_block_spans", &decode_block_spans, py::arg("body"), py::arg("spans"), py::arg("extra"),
          py::arg("threads") = 8, "decode_block_txs for txs given as (start, length) spans of a request body");
    m.def("address_pairs", &address_pairs, py::arg("in_blob"), py::arg("in_off"), py::arg("in_start"),
          py::arg("out_blob"), py::arg("out_off"), py::arg("out_start"), py::arg("threads") = 8);
    m.def("input_address_strings", &input_address_strings, py::arg("addrs64"), py::arg("lens"), py::arg("in_start"),
          py::arg("threads") = 8, py::arg("per_input") = false);
}

}  // namespace upow
