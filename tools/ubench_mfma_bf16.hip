// Issue cost of v_mfma_f32_4x4x4_16b_bf16 against v_mfma_f32_4x4x1_16b_f32 on gfx950, in one process
// (runner: tools/ubench_mfma_bf16.py; record: profiles/ubench_mfma_bf16.txt).
//   * back-to-back, four independent accumulators and one chained accumulator;
//   * interleaved with k independent v_fma_f32 per MFMA, one and two waves per SIMD (the cost model of csrc/snsde_m4_kernel.h:
//     does the MFMA share the VALU issue port, i.e. does  MFMA + k VALU  cost  t_mfma + k t_valu  or  max(t_mfma, k t_valu));
//   * the k VALU ops alone.
// Every wave times its own loop with s_memtime (shader clock); the table reports the mean over all waves of 256 workgroups
// (256 threads = one wave per SIMD, 512 = two).
// build: hipcc --offload-arch=gfx950 -O3 -o tools/ubench_mfma_bf16 tools/ubench_mfma_bf16.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#define BF(acc) acc = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(a16, b16, acc, 0, 0, 4)
#define F32(acc) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a32, b32, acc, 0, 0, 4)
#define FMA(x) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(x) : "v"(one))

constexpr int UNROLL = 8;

// KIND 0: bf16 MFMA, 1: f32 MFMA, 2: no MFMA (VALU alone).  CHAIN: one accumulator instead of four.  K: v_fma_f32 per MFMA.
template <int KIND, bool CHAIN, int K>
__global__ void __launch_bounds__(512) ubench(float* out, unsigned long long* cyc, int iters) {
    const int lane = threadIdx.x & 63;
    const float a32 = lane * 0.001f, b32 = 0.5f + lane;
    const s16x4 a16 = {(short)(0x3f80 + lane), 0x3f80, 0x3f00, 0x3e80}, b16 = {0x3f80, (short)(0x3f00 + lane), 0x3f80, 0x3f00};
    f32x4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
    float v[8] = {1.f * lane, 2.f, 3.f, 4.f, 5.f, 6.f, 7.f, 8.f};
    const float one = 1.0f;
    __syncthreads();
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            f32x4& c = CHAIN ? c0 : (u % 4 == 0 ? c0 : u % 4 == 1 ? c1 : u % 4 == 2 ? c2 : c3);
            if constexpr (KIND == 0) BF(c);
            if constexpr (KIND == 1) F32(c);
#pragma unroll
            for (int j = 0; j < K; ++j) FMA(v[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    const f32x4 c = c0 + c1 + c2 + c3;
    float s = c[0] + c[1] + c[2] + c[3];
    for (int j = 0; j < 8; ++j) s += v[j];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (lane == 0) cyc[blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6)] = t1 - t0;
}

template <int KIND, bool CHAIN, int K>
void run(const char* name, int threads, float* out, unsigned long long* cyc) {
    const int iters = 2000, grid = 256;
    hipLaunchKernelGGL((ubench<KIND, CHAIN, K>), dim3(grid), dim3(threads), 0, 0, out, cyc, iters);      // warm-up
    hipLaunchKernelGGL((ubench<KIND, CHAIN, K>), dim3(grid), dim3(threads), 0, 0, out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return; }
    std::vector<unsigned long long> h(grid * threads / 64);
    (void)hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost);
    double s = 0;
    for (auto x : h) s += (double)x;
    s /= (double)h.size();
    const double per = s / ((double)iters * UNROLL);
    const double kslots = KIND == 0 ? 4.0 : (KIND == 1 ? 1.0 : 0.0);
    printf("%-9s %-7s k=%d  waves/SIMD=%d  cycles/group %7.2f", name, KIND == 2 ? "-" : (CHAIN ? "chain" : "indep4"), K,
           threads / 256, per);
    if (kslots > 0) printf("  cycles/k-slot %6.2f", per / kslots);
    printf("\n");
}

template <int KIND>
void sweep(const char* name, int threads, float* out, unsigned long long* cyc) {
    run<KIND, false, 0>(name, threads, out, cyc);
    run<KIND, false, 1>(name, threads, out, cyc);
    run<KIND, false, 2>(name, threads, out, cyc);
    run<KIND, false, 4>(name, threads, out, cyc);
    run<KIND, false, 8>(name, threads, out, cyc);
}

int main() {
    float* out;
    unsigned long long* cyc;
    if (hipMalloc(&out, 256 * 512 * 4) != hipSuccess || hipMalloc(&cyc, 256 * 8 * 8) != hipSuccess) return 1;
    for (int threads : {256, 512}) {
        run<0, true, 0>("bf16-4x4x4", threads, out, cyc);
        run<1, true, 0>("f32-4x4x1", threads, out, cyc);
        sweep<0>("bf16-4x4x4", threads, out, cyc);
        sweep<1>("f32-4x4x1", threads, out, cyc);
        run<2, false, 1>("valu", threads, out, cyc);
        run<2, false, 2>("valu", threads, out, cyc);
        run<2, false, 4>("valu", threads, out, cyc);
        run<2, false, 8>("valu", threads, out, cyc);
    }
    return 0;
}
