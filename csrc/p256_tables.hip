// The fixed-base tables of k*G: the host's byte-window table T[j][b] = b*256^j*G, built once, and per device
// its copy and the 16-bit-window table T16 the GPU kernels read (csrc/p256_verify.h mul_g / mul_g16), built
// from that copy by build_g16_kernel on first use.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "native.h"
#include "p256_field.h"
#include "p256_verify.h"
#include "streams.h"

namespace upow {
using namespace p256;

// ------------------------------------------------------------------------------------------------
// fixed-base table (host-built once, uploaded once per device)
// ------------------------------------------------------------------------------------------------
static std::once_flag g_tab_once;
static std::vector<aff> g_tab;  // [kGWin][kGEnt]

static void build_g_table() {
    std::vector<jac> jt(size_t(kGWin) * kGEnt);
    jac base = jac_from_aff(aff{fe{P256_GX}, fe{P256_GY}});
    for (int j = 0; j < kGWin; ++j) {
        jac acc = jac_inf();
        for (int b = 1; b < kGEnt; ++b) {
            acc = jac_add(acc, base);
            jt[size_t(j) * kGEnt + b] = acc;
        }
        // base <- 256 * base
        jac nb = base;
        for (int k = 0; k < 8; ++k) nb = jac_dbl(nb);
        base = nb;
    }
    // batch-normalise (Montgomery's trick) skipping entry 0
    std::vector<fe> pref(jt.size());
    fe run = fe_one();
    for (size_t i = 0; i < jt.size(); ++i) {
        if (i % kGEnt == 0) { pref[i] = run; continue; }
        pref[i] = run;
        run = fe_mul(run, jt[i].z);
    }
    fe inv = fe_inv(run);
    g_tab.assign(jt.size(), aff{fe_zero(), fe_zero()});
    for (size_t ii = jt.size(); ii-- > 0;) {
        if (ii % kGEnt == 0) continue;
        const fe zi = fe_mul(inv, pref[ii]);
        inv = fe_mul(inv, jt[ii].z);
        const fe zi2 = fe_sqr(zi);
        g_tab[ii].x = fe_mul(jt[ii].x, zi2);
        g_tab[ii].y = fe_mul(jt[ii].y, fe_mul(zi2, zi));
    }
}

static const std::vector<aff>& g_table() {
    std::call_once(g_tab_once, build_g_table);
    return g_tab;
}

const void* p256_g_table_host() { return g_table().data(); }

struct DeviceGTable {
    int device = -1;
    aff* d_tab = nullptr;
    aff* d_tab16 = nullptr;
};

// T16[j][b] = b * 2^(16 j) * G from the byte-window table: b = lo + 256 hi -> T[2j][lo] + T[2j+1][hi] (one
// mixed addition; the two are never equal or opposite, lo * 256^(2j) < 256^(2j+1) <= hi * 256^(2j+1)), then
// to affine with the thread's own inversion. One thread per entry; entry 0 of each window stays zero.
__global__ __launch_bounds__(256) void build_g16_kernel(const aff* __restrict__ tab8, aff* __restrict__ tab16) {
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= int64_t(kG16Win) * kG16Ent) return;
    const int j = int(e / kG16Ent);
    const uint32_t b = uint32_t(e % kG16Ent), lo = b & 0xffu, hi = b >> 8;
    aff out{fe_zero(), fe_zero()};
    if (b) {
        jac acc = jac_inf();
        if (lo) acc = jac_madd(acc, tab8[(2 * j) * kGEnt + lo]);
        if (hi) acc = jac_madd(acc, tab8[(2 * j + 1) * kGEnt + hi]);
        (void)jac_to_aff(acc, out);
    }
    tab16[e] = out;
}
static std::mutex g_dev_mu;
static DeviceGTable g_dev_tabs[16];

static const aff* device_g_table() {
    int dev = 0;
    stream_check(hipGetDevice(&dev), "hipGetDevice");
    if (dev < 0 || dev >= 16) throw std::runtime_error("device index out of range");
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DeviceGTable& t = g_dev_tabs[dev];
    if (!t.d_tab) {
        const auto& h = g_table();
        stream_check(hipMalloc(&t.d_tab, sizeof(aff) * h.size()), "hipMalloc gtab");
        node_h2d(t.d_tab, h.data(), sizeof(aff) * h.size(), "h2d gtab");
        node_sync("gtab upload");
        t.device = dev;
    }
    return t.d_tab;
}

static const aff* device_g16_table() {
    const aff* tab8 = device_g_table();
    int dev = 0;
    stream_check(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(g_dev_mu);
    DeviceGTable& t = g_dev_tabs[dev];
    if (!t.d_tab16) {
        const int64_t n = int64_t(kG16Win) * kG16Ent;
        aff* d = nullptr;
        stream_check(hipMalloc(&d, sizeof(aff) * size_t(n)), "hipMalloc gtab16");
        hipLaunchKernelGGL(build_g16_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, node_stream(), tab8, d);
        launch_check("build_g16_kernel");
        node_sync("gtab16 build");
        t.d_tab16 = d;
    }
    return t.d_tab16;
}

// entries [first, first + count) of the device's 16-bit-window table, for its differential test
std::vector<uint8_t> p256_g16_entries(int64_t first, int64_t count) {
    const int64_t n = int64_t(kG16Win) * kG16Ent;
    if (first < 0 || count < 0 || first + count > n) throw std::invalid_argument("g16 entry range");
    node_device_enter();
    const aff* d = device_g16_table();
    std::vector<uint8_t> out(size_t(count) * sizeof(aff));
    node_d2h(out.data(), d + first, out.size(), "d2h gtab16");
    return out;
}

// the current device's 16-bit-window table for the kernels' host entry points (csrc/p256.hip,
// csrc/p256_sign.hip, csrc/p256_vanity.hip); call after node_device_enter()
const void* p256_g16_table_device() { return device_g16_table(); }

void set_node_device_native(int dev) { set_node_device(dev); }

}  // namespace upow
