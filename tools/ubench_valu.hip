// VALU throughput micro-benchmark for the SHA-256 instruction mix on gfx950.
// Each kernel runs ILP independent chains of one opcode per lane; throughput reported as
// lane-ops per clock per CU (128 == one wave64 VALU op per 2 cycles on each of the 4 SIMD32s).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1);} } while (0)

template <int OP>
__global__ __launch_bounds__(256) void k(unsigned* out, unsigned seed, int iters) {
    unsigned a0 = seed ^ threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19;
    unsigned b = seed * 0x9e3779b9u + 1, c = seed + 12345;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
#define STEP(x) \
    if (OP == 0) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(b)); \
    if (OP == 1) asm volatile("v_alignbit_b32 %0, %0, %0, 7" : "+v"(x)); \
    if (OP == 2) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(b), "v"(c)); \
    if (OP == 3) asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c)); \
    if (OP == 4) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(x) : "v"(b)); \
    if (OP == 5) asm volatile("v_lshl_or_b32 %0, %0, 3, %1" : "+v"(x) : "v"(b)); \
    if (OP == 6) asm volatile("v_lshrrev_b32 %0, 3, %0" : "+v"(x)); \
    if (OP == 7) asm volatile("v_xad_u32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c)); \
    if (OP == 8) asm volatile("v_alignbit_b32 %0, %0, %1, 7" : "+v"(x) : "v"(b)); \
    if (OP == 9) asm volatile("v_bfi_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c)); \
    if (OP == 10) asm volatile("v_mad_u64_u32 %0, s[0:1], %1, %2, %0" : "+v"(*(unsigned long long*)&x) : "v"(b), "v"(c) : "s0", "s1"); \
    if (OP == 11) asm volatile("v_lshrrev_b64 %0, 7, %0" : "+v"(*(unsigned long long*)&x)); \
    if (OP == 12) asm volatile("v_alignbyte_b32 %0, %0, %1, 3" : "+v"(x) : "v"(b)); \
    if (OP == 13) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c)); \
    if (OP == 14) asm volatile("v_pk_mov_b32 %0, %0, %0 op_sel:[1,0]" : "+v"(*(unsigned long long*)&x)); \
    if (OP == 15) asm volatile("v_lshl_add_u32 %0, %0, 3, %1" : "+v"(x) : "v"(b));
            if (OP == 10 || OP == 11 || OP == 14) { STEP(a0) STEP(a2) STEP(a4) STEP(a6) }
            else { STEP(a0) STEP(a1) STEP(a2) STEP(a3) STEP(a4) STEP(a5) STEP(a6) STEP(a7) }
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
}

template <int OP>
double run(const char* name, int blocks_per_cu, int cus, unsigned* d, double ghz_hint) {
    const int grid = cus * blocks_per_cu;
    const int iters = 2000;
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(256), 0, 0, d, 1u, 10);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(e0));
    hipLaunchKernelGGL(k<OP>, dim3(grid), dim3(256), 0, 0, d, 1u, iters);
    CHK(hipEventRecord(e1));
    CHK(hipEventSynchronize(e1));
    float ms = 0;
    CHK(hipEventElapsedTime(&ms, e0, e1));
    const double ops_per_lane = double(iters) * 16 * ((OP == 10 || OP == 11 || OP == 14) ? 4 : 8);
    const double lane_ops = ops_per_lane * grid * 256.0;
    const double per_s = lane_ops / (ms * 1e-3);
    printf("%-16s blocks/CU=%d  %8.2f Tlane-op/s  = %6.1f lane-ops/clk/CU @%.2fGHz\n", name, blocks_per_cu,
           per_s / 1e12, per_s / cus / (ghz_hint * 1e9), ghz_hint);
    return per_s;
}

// ------------------------------------------------------------------------------------------------
// Mixed-stream modes (`ubench_valu m <mode>`): the PoW loop's opcode mix instead of one opcode, to find
// which condition makes a ~2.4-cycle op (v_bitop3 / v_add_u32) pay the 4 cycles of a v_alignbit.
// SLOW = v_alignbit_b32, FAST = v_bitop3_b32. Every kernel stamps s_memtime / s_memrealtime (100 MHz)
// around its loop, so cycles per wave-instruction are reported at the clock the kernel ran at.
//   S, F        one opcode only, in this harness (the calibration rows)
//   a           alternating SLOW/FAST over 8 independent chains
//   b1 b4 b16   runs of k SLOW then k FAST, round-robin over the 8 chains
//   c1 c2 c4    the SHA Sigma shape: 3 rotates of x -> bitop3 -> v_add_u32 back into x, one serial
//               chain per copy, 1 / 2 / 4 copies per lane interleaved instruction by instruction
//   d           `a` with one source of the FAST op an SGPR
//   e           `a` with three distinct VGPR sources on both ops, different registers per chain
//   e1          `a` with a single VGPR feeding all sources of both ops
// ------------------------------------------------------------------------------------------------
enum { MX_S, MX_F, MX_A, MX_B1, MX_B4, MX_B16, MX_C1, MX_C2, MX_C4, MX_D, MX_E, MX_E1, MX_COUNT };
static const char* const kMixedNames[MX_COUNT] = {"S", "F", "a", "b1", "b4", "b16", "c1", "c2", "c4", "d", "e", "e1"};

#define M_SLOW(x) asm volatile("v_alignbit_b32 %0, %0, %0, 7" : "+v"(x))
#define M_FAST(x) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(b), "v"(c))
#define M_FAST_SGPR(x) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "s"(sb), "v"(c))
#define M_SLOW_3V(x, p, q) asm volatile("v_alignbit_b32 %0, %0, %1, %2" : "+v"(x) : "v"(p), "v"(q))
#define M_FAST_3V(x, p, q) asm volatile("v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96" : "+v"(x) : "v"(p), "v"(q))
#define M_FAST_1V(x) asm volatile("v_bitop3_b32 %0, %0, %0, %0 bitop3:0x96" : "+v"(x))

// VALU instructions per lane and loop iteration, and how many of them are SLOW
__host__ __device__ constexpr int mixed_insts(int mode) {
    return mode == MX_C1 ? 120 : mode == MX_C2 ? 240 : mode == MX_C4 ? 480 : 128;
}
__host__ __device__ constexpr int mixed_slow(int mode) {
    return mode == MX_S ? 128 : mode == MX_F ? 0 : (mode >= MX_C1 && mode <= MX_C4) ? mixed_insts(mode) * 3 / 5 : 64;
}

template <int MODE>
__global__ __launch_bounds__(256) void km(unsigned* out, unsigned long long* stamps, unsigned seed, int iters) {
    unsigned a[8], pb[8], pc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = (seed ^ threadIdx.x) * (2 * j + 3);
        pb[j] = threadIdx.x * 0x9e3779b9u + j;
        pc[j] = (threadIdx.x + 7 * j) & 31;
    }
    unsigned b = threadIdx.x * 0x9e3779b9u + 1, c = threadIdx.x + 12345;
    const unsigned sb = seed * 0x9e3779b9u + 1;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
        if constexpr (MODE >= MX_C1 && MODE <= MX_C4) {
            constexpr int NC = MODE == MX_C1 ? 1 : MODE == MX_C2 ? 2 : 4;
            unsigned t1[NC], t2[NC], t3[NC];
#pragma unroll
            for (int u = 0; u < 24; ++u) {
#pragma unroll
                for (int q = 0; q < NC; ++q) asm volatile("v_alignbit_b32 %0, %1, %1, 2" : "=v"(t1[q]) : "v"(a[q]));
#pragma unroll
                for (int q = 0; q < NC; ++q) asm volatile("v_alignbit_b32 %0, %1, %1, 13" : "=v"(t2[q]) : "v"(a[q]));
#pragma unroll
                for (int q = 0; q < NC; ++q) asm volatile("v_alignbit_b32 %0, %1, %1, 22" : "=v"(t3[q]) : "v"(a[q]));
#pragma unroll
                for (int q = 0; q < NC; ++q)
                    asm volatile("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(t1[q]) : "v"(t1[q]), "v"(t2[q]), "v"(t3[q]));
#pragma unroll
                for (int q = 0; q < NC; ++q) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a[q]) : "v"(t1[q]), "v"(b));
            }
        } else {
#pragma unroll
            for (int n = 0; n < 128; ++n) {
                constexpr int K = MODE == MX_B4 ? 4 : MODE == MX_B16 ? 16 : 1;
                const int j = n & 7;
                const bool slow = MODE == MX_S ? true : MODE == MX_F ? false
                                  : (MODE >= MX_B1 && MODE <= MX_B16) ? ((n / K) & 1) == 0
                                                                    : ((n + (n >> 3)) & 1) == 0;
                if (slow) {
                    if (MODE == MX_E) M_SLOW_3V(a[j], pb[j], pc[j]); else M_SLOW(a[j]);
                } else {
                    if (MODE == MX_D) M_FAST_SGPR(a[j]);
                    else if (MODE == MX_E) M_FAST_3V(a[j], pb[(j + 3) & 7], pc[(j + 5) & 7]);
                    else if (MODE == MX_E1) M_FAST_1V(a[j]);
                    else M_FAST(a[j]);
                }
            }
        }
    }
    const unsigned long long t1e = __builtin_amdgcn_s_memtime(), r1e = __builtin_amdgcn_s_memrealtime();
    unsigned x = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) x ^= a[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = x;
    if (threadIdx.x == 0) {
        stamps[2 * blockIdx.x] = t1e - t0;
        stamps[2 * blockIdx.x + 1] = r1e - r0;
    }
}

static int cmp_u64(const void* p, const void* q) {
    const unsigned long long x = *(const unsigned long long*)p, y = *(const unsigned long long*)q;
    return x < y ? -1 : x > y;
}

template <int MODE>
void run_mixed(int blocks_per_cu, int cus, unsigned* d, unsigned long long* d_stamps) {
    const int grid = cus * blocks_per_cu;
    const int iters = 4000;
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
    for (int w = 0; w < 8; ++w) hipLaunchKernelGGL(km<MODE>, dim3(grid), dim3(256), 0, 0, d, d_stamps, 1u, iters);
    CHK(hipDeviceSynchronize());
    CHK(hipEventRecord(e0));
    hipLaunchKernelGGL(km<MODE>, dim3(grid), dim3(256), 0, 0, d, d_stamps, 1u, iters);
    CHK(hipEventRecord(e1));
    CHK(hipEventSynchronize(e1));
    float ms = 0;
    CHK(hipEventElapsedTime(&ms, e0, e1));
    unsigned long long* st = (unsigned long long*)malloc(sizeof(unsigned long long) * 2 * grid);
    CHK(hipMemcpy(st, d_stamps, sizeof(unsigned long long) * 2 * grid, hipMemcpyDeviceToHost));
    // per-workgroup clock = d(s_memtime) / d(s_memrealtime) x 100 MHz; medians over the workgroups
    unsigned long long* cyc = (unsigned long long*)malloc(sizeof(unsigned long long) * grid);
    double* ghzs = (double*)malloc(sizeof(double) * grid);
    for (int g = 0; g < grid; ++g) { cyc[g] = st[2 * g]; ghzs[g] = double(st[2 * g]) / double(st[2 * g + 1]) * 0.1; }
    qsort(cyc, grid, sizeof(*cyc), cmp_u64);
    for (int g = 1; g < grid; ++g) for (int h = g; h > 0 && ghzs[h] < ghzs[h - 1]; --h) { double t = ghzs[h]; ghzs[h] = ghzs[h - 1]; ghzs[h - 1] = t; }
    const double ghz = ghzs[grid / 2], wave_cycles = double(cyc[grid / 2]);
    const double insts = double(iters) * mixed_insts(MODE);
    const double per_s = insts * grid * 256.0 / (ms * 1e-3);
    // a SIMD holds blocks_per_cu waves (one wave of each 256-lane block); its issue cost per wave-instruction:
    const double cpi_stamp = wave_cycles / (insts * blocks_per_cu);
    const double cpi_event = ms * 1e-3 * ghz * 1e9 / (insts * blocks_per_cu);
    const double slow = double(mixed_slow(MODE)) / mixed_insts(MODE);
    printf("mixed %-4s blocks/CU=%d  slow=%4.2f  %7.2f Tlane-op/s  clk=%.3f GHz  cyc/wave-inst=%.3f (stamps) %.3f (events)"
           "  per-opcode model=%.3f\n",
           kMixedNames[MODE], blocks_per_cu, slow, per_s / 1e12, ghz, cpi_stamp, cpi_event, slow * 4.0 + (1 - slow) * 2.4);
    free(st); free(cyc); free(ghzs);
}

template <int MODE>
bool run_mixed_if(const char* name, int cus, unsigned* d, unsigned long long* d_stamps) {
    if (strcmp(name, kMixedNames[MODE]) != 0) return false;
    for (int bpc : {4, 5, 8}) run_mixed<MODE>(bpc, cus, d, d_stamps);
    return true;
}

int main(int argc, char** argv) {
    int cus = 0;
    CHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    unsigned* d;
    CHK(hipMalloc(&d, sizeof(unsigned) * cus * 8 * 256));
    if (argc > 2 && argv[1][0] == 'm') {
        unsigned long long* d_stamps;
        CHK(hipMalloc(&d_stamps, sizeof(unsigned long long) * 2 * cus * 8));
        const char* m = argv[2];
        const bool ok = run_mixed_if<MX_S>(m, cus, d, d_stamps) || run_mixed_if<MX_F>(m, cus, d, d_stamps) ||
                        run_mixed_if<MX_A>(m, cus, d, d_stamps) || run_mixed_if<MX_B1>(m, cus, d, d_stamps) ||
                        run_mixed_if<MX_B4>(m, cus, d, d_stamps) || run_mixed_if<MX_B16>(m, cus, d, d_stamps) ||
                        run_mixed_if<MX_C1>(m, cus, d, d_stamps) || run_mixed_if<MX_C2>(m, cus, d, d_stamps) ||
                        run_mixed_if<MX_C4>(m, cus, d, d_stamps) || run_mixed_if<MX_D>(m, cus, d, d_stamps) ||
                        run_mixed_if<MX_E>(m, cus, d, d_stamps) || run_mixed_if<MX_E1>(m, cus, d, d_stamps);
        if (!ok) { printf("unknown mixed mode %s\n", m); return 2; }
        return 0;
    }
    if (argc > 1 && argv[1][0] == 'c') {
        // PMC calibration: ONE launch with a known VALU count (16 x 8 v_add_u32 per loop iteration plus
        // the loop's own VALU overhead, see the ISA), to read rocprofv3's SQ_INSTS_VALU / SQ_WAVES scale
        // against (docs/PERF.md §1).
        const int grid = cus * 4, iters = 1000;
        hipLaunchKernelGGL(k<0>, dim3(grid), dim3(256), 0, 0, d, 1u, iters);
        CHK(hipDeviceSynchronize());
        printf("calib: waves=%d  v_add_u32 per wave=%d  (expected SQ_INSTS_VALU >= %.4e, SQ_WAVES = %d)\n",
               grid * 4, iters * 128, double(grid) * 4 * iters * 128, grid * 4);
        return 0;
    }
    const double ghz = 2.1;
    for (int bpc : {4, 8}) {
        run<0>("v_add_u32", bpc, cus, d, ghz);
        run<4>("v_xor_b32", bpc, cus, d, ghz);
        run<1>("v_alignbit(x,x)", bpc, cus, d, ghz);
        run<8>("v_alignbit(x,y)", bpc, cus, d, ghz);
        run<2>("v_bitop3_b32", bpc, cus, d, ghz);
        run<3>("v_add3_u32", bpc, cus, d, ghz);
        run<5>("v_lshl_or_b32", bpc, cus, d, ghz);
        run<6>("v_lshrrev_b32", bpc, cus, d, ghz);
        run<7>("v_xad_u32", bpc, cus, d, ghz);
        run<9>("v_bfi_b32", bpc, cus, d, ghz);
        run<10>("v_mad_u64_u32", bpc, cus, d, ghz);
        run<11>("v_lshrrev_b64", bpc, cus, d, ghz);
        run<12>("v_alignbyte_b32", bpc, cus, d, ghz);
        run<13>("v_perm_b32", bpc, cus, d, ghz);
        run<14>("v_pk_mov_b32", bpc, cus, d, ghz);
        run<15>("v_lshl_add_u32", bpc, cus, d, ghz);
    }
    return 0;
}
