// K6: P-256 public keys as addresses carry them: decompression of 33-byte addresses and the on-curve check of
// 64-byte ones, one key per lane, with the same code on the host. (The fused block path decompresses its signer
// keys in csrc/p256.hip p256_keyrec_kernel, in the verify's stream order.)
//
// reference: fastecdsa util.mod_sqrt / curve.is_point_on_curve as called from upow/helpers.py:135-144 and
// upow/upow_transactions/transaction_output.py:25-26.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_pool.h"
#include "native.h"
#include "p256_field.h"
#include "p256_verify.h"
#include "streams.h"
#include "thread_pool.h"

namespace upow {
using namespace p256;

// item: 33-byte compressed address [spec | x LE]; out: x LE | y LE (64 B) and ok flag
__global__ __launch_bounds__(256) void p256_decompress_kernel(const uint8_t* __restrict__ in, int64_t n,
                                                               uint8_t* __restrict__ out, uint8_t* __restrict__ ok) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* a = in + 33 * i;
    const fe x = fe_from_le(a + 1);
    const bool odd = a[0] == 43;
    fe y;
    const bool good = curve_y(x, y);
    if ((y.v[0] & 1u) != uint32_t(odd)) y = fe_neg(y);
    fe_to_le(x, out + 64 * i);
    fe_to_le(y, out + 64 * i + 32);
    ok[i] = good ? 1 : 0;
}

__global__ __launch_bounds__(256) void p256_on_curve_kernel(const uint8_t* __restrict__ in, int64_t n,
                                                             uint8_t* __restrict__ ok) {
    const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ok[i] = on_curve_64(in + 64 * i);
}

void p256_decompress_host(const uint8_t* in, int64_t n, uint8_t* out, uint8_t* ok) {
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t* a = in + 33 * i;
        const fe x = fe_from_le(a + 1);
        const bool odd = a[0] == 43;
        fe y;
        const bool good = curve_y(x, y);
        if ((y.v[0] & 1u) != uint32_t(odd)) y = fe_neg(y);
        fe_to_le(x, out + 64 * i);
        fe_to_le(y, out + 64 * i + 32);
        ok[i] = good ? 1 : 0;
    }
}

void p256_decompress_gpu(const uint8_t* in, int64_t n, uint8_t* out, uint8_t* ok) {
    if (n == 0) return;
    node_device_enter();
    PooledBuf<uint8_t> b_in{33 * size_t(n)}, b_out{64 * size_t(n)}, b_ok{size_t(n)};
    uint8_t *d_in = b_in.p, *d_out = b_out.p, *d_ok = b_ok.p;
    StagedIO io(98 * size_t(n));
    io.h2d(d_in, in, 33 * size_t(n));
    const int block = 256;
    hipLaunchKernelGGL(p256_decompress_kernel, dim3(int((n + block - 1) / block)), dim3(block), 0, node_stream(), d_in, n,
                       d_out, d_ok);
    launch_check("p256_decompress_kernel");
    io.d2h(out, d_out, 64 * size_t(n));
    io.d2h(ok, d_ok, size_t(n));
    io.finish("decompress");
}

void p256_on_curve_host(const uint8_t* in, int64_t n, uint8_t* ok, int threads) {
    HostPool::get().parallel_for(n, threads, [&](int64_t i) { ok[i] = on_curve_64(in + 64 * i); });
}

void p256_on_curve_gpu(const uint8_t* in, int64_t n, uint8_t* ok) {
    if (n == 0) return;
    node_device_enter();
    PooledBuf<uint8_t> b_in{64 * size_t(n)}, b_ok{size_t(n)};
    StagedIO io(65 * size_t(n));
    io.h2d(b_in.p, in, 64 * size_t(n));
    const int block = 256;
    hipLaunchKernelGGL(p256_on_curve_kernel, dim3(int((n + block - 1) / block)), dim3(block), 0, node_stream(), b_in.p, n,
                       b_ok.p);
    launch_check("p256_on_curve_kernel");
    io.d2h(ok, b_ok.p, size_t(n));
    io.finish("on-curve");
}

}  // namespace upow
