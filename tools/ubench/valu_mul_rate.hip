// What one integer multiply of k_vara_i8p's tile row-dot costs on gfx950: cycles per instruction of v_mul_lo_u32, v_mad_i32_i24, v_bfe_i32
// and v_add_u32, and of the row-dot's two forms per product (v_bfe_i32 + v_mul_lo_u32 + v_add_u32 against v_bfe_i32 + v_mad_i32_i24), as
// one dependent chain and as four independent ones, one wave per SIMD (256 workgroups of 4 waves) and two (8 waves).  s_memtime stamps
// around the loop, written to a buffer of their own; the median over the waves is printed.  A dependent chain shows max(latency, issue
// cost); four independent chains show the issue cost alone, which is what the row-dot pays (its products are independent, only the
// adds chain).
// Build: hipcc -O3 --offload-arch=gfx950 tools/ubench/valu_mul_rate.hip -o tools/ubench/valu_mul_rate
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

enum Op { MUL_LO, MAD24, BFE, ADD, DOT32, DOT24 };
constexpr int UNROLL = 64;   // instructions (or products) per loop iteration and chain set

__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// one step on accumulator x with the operands y (a multiplier / an addend) and g (four packed bytes)
template <Op OP>
__device__ __forceinline__ void step(int& x, int y, int g) {
    int e;
    if constexpr (OP == MUL_LO) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(x) : "v"(y));
    if constexpr (OP == MAD24) asm volatile("v_mad_i32_i24 %0, %1, %2, %0" : "+v"(x) : "v"(y), "v"(g));
    if constexpr (OP == BFE) asm volatile("v_bfe_i32 %0, %0, 8, 8" : "+v"(x));
    if constexpr (OP == ADD) asm volatile("v_add_u32 %0, %0, %1" : "+v"(x) : "v"(y));
    if constexpr (OP == DOT32)
        asm volatile("v_bfe_i32 %1, %3, 8, 8\n\tv_mul_lo_u32 %1, %2, %1\n\tv_add_u32 %0, %0, %1" : "+v"(x), "=&v"(e) : "v"(y), "v"(g));
    if constexpr (OP == DOT24) asm volatile("v_bfe_i32 %1, %3, 8, 8\n\tv_mad_i32_i24 %0, %2, %1, %0" : "+v"(x), "=&v"(e) : "v"(y), "v"(g));
}

template <Op OP, int CHAINS>
__global__ __launch_bounds__(512) void k_chain(const int* __restrict__ in, int* __restrict__ sink, unsigned long long* __restrict__ stamps, int iters) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int x[CHAINS];
    for (int c = 0; c < CHAINS; c++) x[c] = in[(t + c) & 1023];
    const int y = in[(t + 7) & 1023] | 1, g = in[(t + 11) & 1023];
    const unsigned long long t0 = stamp();
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int u = 0; u < UNROLL / CHAINS; u++)
#pragma unroll
            for (int c = 0; c < CHAINS; c++) step<OP>(x[c], y, g);
    }
    const unsigned long long t1 = stamp();
    int s = 0;
    for (int c = 0; c < CHAINS; c++) s += x[c];
    sink[t] = s;
    if ((threadIdx.x & 63) == 0) stamps[t >> 6] = t1 - t0;
}

template <Op OP, int CHAINS>
static void run(const char* name, int per_step, int waves_per_simd, const int* dIn, int* dSink, unsigned long long* dStamps, int iters) {
    const int threads = 256 * waves_per_simd, nwaves = 256 * threads / 64;
    std::vector<unsigned long long> h(nwaves);
    double med = 0;
    for (int rep = 0; rep < 2; rep++) {
        hipLaunchKernelGGL((k_chain<OP, CHAINS>), dim3(256), dim3(threads), 0, 0, dIn, dSink, dStamps, iters);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(h.data(), dStamps, sizeof(unsigned long long) * nwaves, hipMemcpyDeviceToHost));
        std::sort(h.begin(), h.end());
        med = (double)h[nwaves / 2];
    }
    const double steps = (double)iters * UNROLL;
    printf("%-44s chains %d  waves/SIMD %d : %7.2f cycles per step of one wave (%d instr), %6.2f per instr; per SIMD %6.2f per step\n", name, CHAINS,
           waves_per_simd, med / steps, per_step, med / steps / per_step, med / steps / waves_per_simd);
}

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 2000;
    std::vector<int> in(1024);
    srand(7);
    for (auto& v : in) v = rand();
    int *dIn, *dSink; unsigned long long* dStamps;
    CHECK(hipMalloc((void**)&dIn, 4096)); CHECK(hipMalloc((void**)&dSink, 256 * 512 * 4)); CHECK(hipMalloc((void**)&dStamps, 256 * 8 * 8));
    CHECK(hipMemcpy(dIn, in.data(), 4096, hipMemcpyHostToDevice));
    for (int wps = 1; wps <= 2; wps++) {
        run<ADD, 1>("v_add_u32", 1, wps, dIn, dSink, dStamps, iters);
        run<ADD, 4>("v_add_u32", 1, wps, dIn, dSink, dStamps, iters);
        run<BFE, 1>("v_bfe_i32", 1, wps, dIn, dSink, dStamps, iters);
        run<BFE, 4>("v_bfe_i32", 1, wps, dIn, dSink, dStamps, iters);
        run<MUL_LO, 1>("v_mul_lo_u32", 1, wps, dIn, dSink, dStamps, iters);
        run<MUL_LO, 4>("v_mul_lo_u32", 1, wps, dIn, dSink, dStamps, iters);
        run<MAD24, 1>("v_mad_i32_i24", 1, wps, dIn, dSink, dStamps, iters);
        run<MAD24, 4>("v_mad_i32_i24", 1, wps, dIn, dSink, dStamps, iters);
        run<DOT32, 1>("row-dot product: bfe + mul_lo + add", 3, wps, dIn, dSink, dStamps, iters);
        run<DOT32, 4>("row-dot product: bfe + mul_lo + add", 3, wps, dIn, dSink, dStamps, iters);
        run<DOT24, 1>("row-dot product: bfe + mad_i32_i24", 2, wps, dIn, dSink, dStamps, iters);
        run<DOT24, 4>("row-dot product: bfe + mad_i32_i24", 2, wps, dIn, dSink, dStamps, iters);
    }
    return 0;
}
