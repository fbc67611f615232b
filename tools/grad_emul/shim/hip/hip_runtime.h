// Host emulation shim for csrc/grad.hip (tools/grad_emul.py): <hip/hip_runtime.h> replaced by one
// std::thread per GPU thread (a std::barrier is __syncthreads), workgroups run one after another,
// the fp32 MFMA emulated per wave in the fragment order the kernel assumes.  Global buffers and the
// dynamic LDS are exact-size heap blocks, static LDS arrays are globals: AddressSanitizer sees every
// access outside them.
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>
#include <algorithm>
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct int2 { int x, y; };   // ecorr_internal.h names it (the volume-free backward's workspace origins)
inline thread_local dim3 threadIdx;
inline dim3 blockIdx, gridDim;
inline std::barrier<>* g_bar;
inline std::barrier<>* g_wbar[16];
inline float* g_dynlds;
inline float g_sa[16][64], g_sb[16][64];
#define __syncthreads() g_bar->arrive_and_wait()
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __shared__ static
typedef void* hipStream_t;
typedef int hipError_t;
constexpr int hipSuccess = 0;
inline hipError_t hipGetLastError() { return 0; }
inline const char* hipGetErrorString(hipError_t) { return "emul"; }
inline float __fadd_rn(float a, float b) { return a + b; }
inline float __fsub_rn(float a, float b) { return a - b; }
inline float __fmul_rn(float a, float b) { return a * b; }
inline float __fdiv_rn(float a, float b) { return a / b; }
// csrc/mfma_f32_frame.h: `typedef float floatx16 __attribute__((ext_vector_type(16)))` is clang's; g++ has
// the same 16 subscriptable floats as vector_size (bytes)
#define ext_vector_type(n) vector_size(sizeof(float) * (n))
typedef float emul_f16 __attribute__((vector_size(64)));
inline emul_f16 emul_mfma(float a, float b, emul_f16 acc) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    g_sa[w][lane] = a; g_sb[w][lane] = b;
    g_wbar[w]->arrive_and_wait();
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = lane & 31;
        for (int k = 0; k < 2; ++k) acc[r] = __builtin_fmaf(g_sa[w][k * 32 + row], g_sb[w][k * 32 + col], acc[r]);
    }
    g_wbar[w]->arrive_and_wait();
    return acc;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, x, y, z) emul_mfma(a, b, c)
template <class F>
void emul_launch(F body, dim3 grid, dim3 block, size_t lds) {
    std::vector<float> dyn(lds / 4 + 1);   // heap: ASan sees overruns of the dynamic LDS
    g_dynlds = dyn.data();
    gridDim = grid;
    const int nt = block.x;
    for (unsigned z = 0; z < grid.z; ++z) for (unsigned y = 0; y < grid.y; ++y) for (unsigned x = 0; x < grid.x; ++x) {
        blockIdx = dim3(x, y, z);
        std::barrier<> bar(nt);
        g_bar = &bar;
        std::vector<std::barrier<>*> wb;
        for (int w = 0; w < (nt + 63) / 64; ++w) { wb.push_back(new std::barrier<>(std::min(64, nt - 64 * w))); g_wbar[w] = wb.back(); }
        std::vector<std::thread> th;
        for (int t = 0; t < nt; ++t) th.emplace_back([&, t] { threadIdx = dim3(t); body(); });
        for (auto& t : th) t.join();
        for (auto* b : wb) delete b;
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emul_launch([&] { kernel(__VA_ARGS__); }, grid, block, lds)
