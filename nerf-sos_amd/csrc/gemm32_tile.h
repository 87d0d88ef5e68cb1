// The fp32 GEMM tile of the image models (dino_gemm_kernel in dino_vit.hip, lpips_conv_kernel in lpips.hip), once:
//   out[row][col] = epilogue(sum_k A[row][k] * Wt[k][col] + bias[col]),  Wt [K][N] row-major, A whatever the caller's loader reads.
// 64x64 outputs per workgroup of 256 threads, four waves of 32x32, K in steps of 32 through LDS, the next tile's global loads in
// flight under this tile's MFMAs (v_mfma_f32_32x32x2_f32).  Per output element the 32 products of a K tile are one fma chain, k
// ascending, and the tiles are taken in ascending order; how a tile's chain joins the running sum is the caller's policy.
#pragma once
#include "mlp_common.h"   // f32x16

namespace nsos {
namespace gemm32 {

constexpr int GM = 64, GN = 64, GK = 32, LDA = GK + 1;   // odd A stride: the 32 rows a wave reads per k fall in 32 banks

// A thread's share of an A tile (64 x 32): four consecutive k from a_k() of the rows a_row() and a_row() + 32.
__device__ __forceinline__ int a_row() { return threadIdx.x >> 3; }
__device__ __forceinline__ int a_k() { return (threadIdx.x & 7) * 4; }

// The output column of this thread in the tile at n0: all 16 of its outputs are in that column.  A caller that forms `out + out_col(n0)`
// before the call gives every store one 64-bit add (the row offset) instead of two.
__device__ __forceinline__ int out_col(int n0) { return n0 + ((threadIdx.x >> 6) & 1) * 32 + (threadIdx.x & 31); }

// ---- accumulation policies: start() is the C operand of a K tile's first MFMA, add() receives the chain's result ----------------
struct OneChain {   // one fma chain over all of K
    f32x16 acc;
    __device__ __forceinline__ OneChain() {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    }
    __device__ __forceinline__ f32x16 start() const { return acc; }
    __device__ __forceinline__ void add(const f32x16& chain) { acc = chain; }
    __device__ __forceinline__ float value(int r) const { return acc[r]; }
};
struct TwoSumOfTiles {   // every tile a chain from zero; the tiles' sums p_0, p_1, .. added as (tot, lo) with Knuth's two-sum
    f32x16 tot, lo;
    __device__ __forceinline__ TwoSumOfTiles() {
#pragma unroll
        for (int i = 0; i < 16; ++i) tot[i] = 0.0f, lo[i] = 0.0f;
    }
    __device__ __forceinline__ f32x16 start() const {
        f32x16 z;
#pragma unroll
        for (int i = 0; i < 16; ++i) z[i] = 0.0f;
        return z;
    }
    __device__ __forceinline__ void add(const f32x16& acc) {
        const f32x16 t = tot + acc, bb = t - tot;   // t + e = tot + acc exactly
        lo = lo + ((tot - (t - bb)) + (acc - bb));
        tot = t;
    }
    __device__ __forceinline__ float value(int r) const { return tot[r] + lo[r]; }
};

// One workgroup's 64x64 outputs at (m0, n0).  load_a(k0, ra): this thread's two float4 of the A tile at k0 (see a_row / a_k), called
// once per tile with k0 ascending, one tile ahead of its use -- a loader may keep running state.  epilogue(row, col, value) is called
// for the thread's outputs with row < M, value = fl(sum + bias[col]); rows past M are the loader's to clamp.  N % 64 == 0,
// K % 32 == 0, Wt 16-byte aligned.
template <class Sum, class LoadA, class Epilogue>
__device__ __forceinline__ void tile(int K, int m0, int n0, int M, const float* __restrict__ Wt,
                                     const float* __restrict__ bias, int N, LoadA&& load_a, Epilogue&& epilogue) {
    __shared__ float As[GM * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[GK * GN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int ar = a_row(), ak = a_k();
    const int bk = tid >> 4, bn = (tid & 15) * 4;   // B tile 32x64: two float4 per thread (rows bk, bk + 16)
    float4 ra[2], rb0, rb1;
    auto gload = [&](int k0) {
        load_a(k0, ra);
        rb0 = *reinterpret_cast<const float4*>(Wt + (size_t)(k0 + bk) * N + n0 + bn);
        rb1 = *reinterpret_cast<const float4*>(Wt + (size_t)(k0 + bk + 16) * N + n0 + bn);
    };
    Sum sum;
    gload(0);
    const int a_off = (wm * 32 + (lane & 31)) * LDA + (lane >> 5), b_off = (lane >> 5) * GN + wn * 32 + (lane & 31);
#pragma unroll 1   // one copy of the body whatever K is (a constant K of 384 would otherwise unroll into 12 copies and 24 barriers)
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();   // the previous tile has been consumed
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float* d = As + (ar + 32 * r) * LDA + ak;
            d[0] = ra[r].x, d[1] = ra[r].y, d[2] = ra[r].z, d[3] = ra[r].w;
        }
        *reinterpret_cast<float4*>(Bs + bk * GN + bn) = rb0;
        *reinterpret_cast<float4*>(Bs + (bk + 16) * GN + bn) = rb1;
        __syncthreads();
        if (k0 + GK < K) gload(k0 + GK);   // in flight under this tile's MFMAs
        f32x16 acc = sum.start();
#pragma unroll
        for (int kk = 0; kk < GK; kk += 2)   // k ascending: one fma chain per output element
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[a_off + kk], Bs[b_off + kk * GN], acc, 0, 0, 0);
        sum.add(acc);
    }
    const int col = out_col(n0);
    const float bv = bias[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {   // C/D: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < M) epilogue(row, col, sum.value(r) + bv);
    }
}

}  // namespace gemm32
}  // namespace nsos
