// Arithmetic probe (test hook, csrc/p256_probe.h; never called by the node): the host loop, the kernels built
// with the ILP-first scheduler of the verify TU csrc/p256.hip (`ilp`; p256_batch.hip has the `occ` twin under
// the default one) and the dispatcher p256_probe.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "dev_pool.h"
#include "native.h"
#include "p256_probe.h"
#include "streams.h"

namespace upow {
using namespace p256;

// One item per lane.
template <int OP>
__global__ __launch_bounds__(256) void p256_probe_ilp_kernel(const uint32_t* __restrict__ a,
                                                              const uint32_t* __restrict__ b, uint8_t* __restrict__ out,
                                                              int64_t n, int a_words, int b_words, int out_bytes) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    probe::one<OP>(a + i * a_words, b + i * b_words, out + i * out_bytes);
}

// One group per G::kLanes lanes (G = QuadDev or OctDev) in the geometry of p256_verify_group_kernel<G> (16 or 8
// groups per wave, four waves per workgroup, a group at or past n returns as a whole). Every lane stores all
// it holds after the operation, as copy (lane mod G::kLanes) of its group: 128 bytes, the four products of mul4 /
// sqr4 or the point of dbl4 / add4.
template <class G, int OP>
__global__ __launch_bounds__(256, 1) void p256_probe_group_kernel(const uint32_t* __restrict__ a,
                                                                   const uint32_t* __restrict__ b,
                                                                   uint8_t* __restrict__ out, int64_t n, int a_words,
                                                                   int b_words) {
    const int lane = int(threadIdx.x) & 63;
    const int64_t g = (int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6)) * (64 / G::kLanes) + lane / G::kLanes;
    if (g >= n) return;
    probe::group<OP>(G::of_lane(lane), a + g * a_words, b + g * b_words,
                     out + (g * G::kLanes + (lane & (G::kLanes - 1))) * 128);
}

std::vector<uint8_t> p256_probe(const std::string& op_name, const uint8_t* a, size_t a_bytes, const uint8_t* b,
                                size_t b_bytes, const std::string& mode) {
    // 'quad_' / 'oct_' select the step policy of a lane-group operation
    int lanes = 1;
    std::string base = op_name;
    if (base.rfind("quad_", 0) == 0) { lanes = 4; base = base.substr(5); }
    else if (base.rfind("oct_", 0) == 0) { lanes = 8; base = base.substr(4); }
    int op = -1;
    for (int k = 0; k < probe::kOps; ++k)
        if (base == probe::shape(k).name) op = k;
    if (op < 0 || (lanes == 1) != (op < probe::kOneLaneOps)) throw std::invalid_argument("p256_probe: unknown op " + op_name);
    const bool host = mode == "host", ilp = mode == "ilp", occ = mode == "occ";
    if (!host && !ilp && !occ) throw std::invalid_argument("p256_probe: unknown mode " + mode);
    if (occ && lanes != 1) throw std::invalid_argument("p256_probe: the lane-group operations have modes host and ilp");
    if (!host && lanes == 1 && op >= probe::kOneLaneDeviceOps)
        throw std::invalid_argument("p256_probe: " + op_name + " has mode host only");
    const probe::Shape sh = probe::shape(op);
    const size_t ia = 4 * size_t(sh.a_words), ib = 4 * size_t(sh.b_words);
    if (a_bytes % ia) throw std::invalid_argument("p256_probe: operand a is not a whole number of items");
    const int64_t n = int64_t(a_bytes / ia);
    if (b_bytes != size_t(n) * ib) throw std::invalid_argument("p256_probe: operand b does not match operand a");
    const size_t copies = host ? 1 : size_t(lanes);
    std::vector<uint8_t> out(size_t(n) * copies * size_t(sh.out_bytes));
    if (n == 0) return out;
    if (host) {
        std::vector<uint32_t> wa(a_bytes / 4), wb(b_bytes / 4 + 1);
        std::memcpy(wa.data(), a, a_bytes);
        if (b_bytes) std::memcpy(wb.data(), b, b_bytes);
        auto loop = [&](auto&& item) {
            for (int64_t i = 0; i < n; ++i)
                item(wa.data() + i * sh.a_words, wb.data() + i * sh.b_words, out.data() + i * sh.out_bytes);
        };
        if (lanes == 1)
            probe::dispatch_one(op, [&](auto K) {
                loop([](const uint32_t* x, const uint32_t* y, uint8_t* o) { probe::one<decltype(K)::value>(x, y, o); });
            });
        else if (lanes == 4)
            probe::dispatch_group(op, [&](auto K) {
                loop([](const uint32_t* x, const uint32_t* y, uint8_t* o) { probe::group<decltype(K)::value>(QuadHost{}, x, y, o); });
            });
        else
            probe::dispatch_group(op, [&](auto K) {
                loop([](const uint32_t* x, const uint32_t* y, uint8_t* o) { probe::group<decltype(K)::value>(OctHost{}, x, y, o); });
            });
        return out;
    }
    node_device_enter();
    PooledBuf<uint32_t> b_a{a_bytes / 4}, b_b{b_bytes / 4};
    PooledBuf<uint8_t> b_out{out.size()};
    StagedIO io(a_bytes + b_bytes + out.size());
    io.h2d(b_a.p, a, a_bytes);
    io.h2d(b_b.p, b, b_bytes);
    hipStream_t st = node_stream();
    if (occ) {
        p256_probe_occ_launch(op, b_a.p, b_b.p, b_out.p, n, st);
    } else if (lanes == 1) {
        probe::dispatch_one(op, [&](auto K) {
            constexpr int k = decltype(K)::value;
            if constexpr (k < probe::kOneLaneDeviceOps)
                hipLaunchKernelGGL(p256_probe_ilp_kernel<k>, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, b_a.p, b_b.p,
                                   b_out.p, n, sh.a_words, sh.b_words, sh.out_bytes);
        });
        launch_check("p256_probe_ilp_kernel");
    } else {
        const int64_t waves = lanes == 4 ? (n + 15) / 16 : (n + 7) / 8;
        const dim3 grid(unsigned((waves + 3) / 4));
        probe::dispatch_group(op, [&](auto K) {
            constexpr int k = decltype(K)::value;
            if (lanes == 4)
                hipLaunchKernelGGL((p256_probe_group_kernel<QuadDev, k>), grid, dim3(256), 0, st, b_a.p, b_b.p, b_out.p, n,
                                   sh.a_words, sh.b_words);
            else
                hipLaunchKernelGGL((p256_probe_group_kernel<OctDev, k>), grid, dim3(256), 0, st, b_a.p, b_b.p, b_out.p, n,
                                   sh.a_words, sh.b_words);
        });
        launch_check("p256_probe_group_kernel");
    }
    io.d2h(out.data(), b_out.p, out.size());
    io.finish("p256 probe");
    return out;
}

}  // namespace upow
