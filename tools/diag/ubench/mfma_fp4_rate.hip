// Issue rate of the block-scaled FP4 MFMA on gfx950, the measurement of mfma_i8_rate.hip for v_mfma_scale_f32_32x32x64_f8f6f4
// with e2m1 operands (cbsz:4 blgp:4, four VGPRs each): ns and shader ticks per instruction per SIMD, one or two waves per
// SIMD, independent accumulators vs one dependent chain; then the matcher's loop (operand unpacked by VALU right before
// its MFMAs) and its epilogue alone.  hipcc -O3 --offload-arch=gfx950 mfma_fp4_rate.hip -o mfma_fp4_rate
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
#define FP4 4
#define SCALE 133   // e8m0 2^6

__device__ __forceinline__ v16f mfma(v8i a, v8i b, v16f c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, FP4, FP4, 0, SCALE, 0, SCALE);
}

template <int CHAINS>
__global__ __launch_bounds__(256) void k(int iters, float* out, unsigned long long* cyc) {
    v8i a = {0x22222222 ^ (int)threadIdx.x, 0x2a2a2a2a, 0x22a222a2, 0x2222aaaa, 0, 0, 0, 0};
    v8i b = {0x2a2a2a2a, 0x22222222, 0x2222aaaa ^ (int)blockIdx.x, 0x22a222a2, 0, 0, 0, 0};
    v16f c[4] = {};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u % CHAINS] = mfma(a, b, c[u % CHAINS]);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0;
    for (int u = 0; u < 4; ++u) for (int r = 0; r < 16; ++r) s += c[u][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

// the matcher's inner loop: 4 k-steps, the A operand of each built by VALU (shift + bitop3 per dword) right before the NT MFMAs that use it
template <int MODE, int NT>
__global__ __launch_bounds__(256) void kmix(int iters, float* out, unsigned long long* cyc, const uint4* src) {
    v8i b[NT][4];
    for (int u = 0; u < NT; ++u) for (int s = 0; s < 4; ++s) b[u][s] = v8i{0x22222222 ^ ((int)threadIdx.x + u), 0x2a2a2a2a ^ s, 0x22a222a2, 0x2222aaaa ^ (int)blockIdx.x, 0, 0, 0, 0};
    v16f c[4] = {};
    uint4 w = src[threadIdx.x];
    const unsigned sign = 0x88888888u, one = 0x22222222u;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
        if (MODE == 2) { w.x += i; w.y ^= i; }
        v8i a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            a[s] = v8i{};
            if (MODE == 0) { a[s][0] = w.x | one; a[s][1] = w.y | one; a[s][2] = w.z | one; a[s][3] = w.w | one; }   // operand (almost) straight from registers
            else {
                a[s][0] = (int)__builtin_amdgcn_bitop3_b32(w.x << (3 - s), sign, one, 0xAE); a[s][1] = (int)__builtin_amdgcn_bitop3_b32(w.y << (3 - s), sign, one, 0xAE);
                a[s][2] = (int)__builtin_amdgcn_bitop3_b32(w.z << (3 - s), sign, one, 0xAE); a[s][3] = (int)__builtin_amdgcn_bitop3_b32(w.w << (3 - s), sign, one, 0xAE);
            }
        }
#pragma unroll
        for (int g = 0; g < NT; g += 4)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int u = 0; u < 4; ++u) c[u] = mfma(a[s], b[g + u][s], c[u]);
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float sum = 0;
    for (int u = 0; u < 4; ++u) for (int r = 0; r < 16; ++r) sum += c[u][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = sum;
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

// the matcher's epilogue alone: 4 x 16 positive f32 keys folded into (best, second) with v_min_i32 (on the bit patterns) + v_med3_f32
template <int MODE>
__global__ __launch_bounds__(256) void kepi(int iters, float* out, unsigned long long* cyc, const int* src) {
    float c[4][16];
    for (int u = 0; u < 4; ++u) for (int r = 0; r < 16; ++r) c[u][r] = (float)(src[(threadIdx.x + 17 * u + 3 * r) & 255] & 0xFFFFF) + 1.0f;
    float kb[4] = {0x1p30f, 0x1p30f, 0x1p30f, 0x1p30f}, ks[4] = {0x1p30f, 0x1p30f, 0x1p30f, 0x1p30f};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float k = c[u][r] + (float)i;
                ks[u] = __builtin_amdgcn_fmed3f(kb[u], ks[u], k);
                if (MODE == 0) kb[u] = __int_as_float(min(__float_as_int(kb[u]), __float_as_int(k)));
                else kb[u] = __builtin_fminf(kb[u], k);   // with the compiler's v_max_f32 x, x in front
            }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * blockDim.x + threadIdx.x] = kb[0] + kb[1] + kb[2] + kb[3] + ks[0] + ks[1] + ks[2] + ks[3];
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <typename F>
void timed(F launch, int warm, int iters, float* ms, unsigned long long* ticks, unsigned long long* cyc) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    launch(warm);
    hipEventRecord(e0);
    launch(iters);
    hipEventRecord(e1); hipEventSynchronize(e1);
    hipEventElapsedTime(ms, e0, e1);
    hipMemcpy(ticks, cyc, 8, hipMemcpyDeviceToHost);
    hipEventDestroy(e0); hipEventDestroy(e1);
}

template <int CHAINS>
void run(const char* name, int blocks) {
    float* out; unsigned long long* cyc;
    hipMalloc(&out, sizeof(float) * blocks * 256); hipMalloc(&cyc, 8);
    const int iters = 2000;
    float ms; unsigned long long hc;
    timed([&](int n) { k<CHAINS><<<blocks, 256>>>(n, out, cyc); }, 10, iters, &ms, &hc, cyc);
    const double n = 8.0 * iters * (blocks / 256.0);   // MFMAs per SIMD (one wave of a block per SIMD)
    printf("%-28s blocks %4d (%.0f waves/SIMD): %.2f ns per MFMA per SIMD, %.1f memtime ticks per MFMA of one wave\n", name, blocks, blocks / 256.0,
           ms * 1e6 / n, (double)hc / (8.0 * iters));
    hipFree(out); hipFree(cyc);
}

template <int MODE, int NT>
void runmix(const char* name, int blocks) {
    float* out; unsigned long long* cyc; uint4* src;
    hipMalloc(&out, sizeof(float) * blocks * 256); hipMalloc(&cyc, 8); hipMalloc(&src, 16 * 256); hipMemset(src, 0x5a, 16 * 256);
    const int iters = 500;
    float ms; unsigned long long hc;
    timed([&](int n) { kmix<MODE, NT><<<blocks, 256>>>(n, out, cyc, src); }, 10, iters, &ms, &hc, cyc);
    const double n = 4.0 * NT * iters * (blocks / 256.0);
    printf("%-52s blocks %4d: %.2f ns per MFMA per SIMD, %.1f ticks per MFMA of one wave\n", name, blocks, ms * 1e6 / n, (double)hc / (4.0 * NT * iters));
    hipFree(out); hipFree(cyc); hipFree(src);
}

template <int MODE>
void runepi(const char* name, int blocks) {
    float* out; unsigned long long* cyc; int* src;
    hipMalloc(&out, sizeof(float) * blocks * 256); hipMalloc(&cyc, 8); hipMalloc(&src, 1024); hipMemset(src, 0x11, 1024);
    const int iters = 1000;
    float ms; unsigned long long hc;
    timed([&](int n) { kepi<MODE><<<blocks, 256>>>(n, out, cyc, src); }, 10, iters, &ms, &hc, cyc);
    printf("%-52s blocks %4d: %.1f ns per 64-key epilogue per SIMD, %.0f ticks per epilogue of one wave\n", name, blocks, ms * 1e6 / (iters * (blocks / 256.0)), (double)hc / iters);
    hipFree(out); hipFree(cyc); hipFree(src);
}

int main() {
    run<4>("32x32x64 fp4, 4 chains", 256);
    run<4>("32x32x64 fp4, 4 chains", 512);
    run<2>("32x32x64 fp4, 2 chains", 256);
    run<1>("32x32x64 fp4, 1 chain", 256);
    run<1>("32x32x64 fp4, 1 chain", 512);
    runepi<0>("epilogue, add + med3_f32 + min_i32 per key", 256);
    runepi<0>("epilogue, add + med3_f32 + min_i32 per key", 512);
    runepi<1>("epilogue, add + med3_f32 + max + min_f32 per key", 512);
    runmix<0, 4>("loop of 4 steps x 4 MFMA, A from registers", 256);
    runmix<0, 4>("loop of 4 steps x 4 MFMA, A from registers", 512);
    runmix<2, 4>("... A unpacked by VALU per step (w changes)", 256);
    runmix<2, 4>("... A unpacked by VALU per step (w changes)", 512);
    runmix<2, 8>("loop of 2 x 4 steps x 4 MFMA, A unpacked once", 512);
    return 0;
}
