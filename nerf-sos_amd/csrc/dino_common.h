// What the fp32 (dino_vit.hip) and the 16-bit (dino_vit16.hip) DINO ViT-S/16 kernels share: the geometry, the resize index rule and
// the prepared pixel (so that both paths produce the same [B,3,224,224] network input bit for bit), the wave reductions.
#pragma once
#include "common.h"

namespace nsos {
namespace dino {

constexpr int D = NSOS_DINO_WIDTH, T = NSOS_DINO_TOKENS, NP = T - 1, HEADS = NSOS_DINO_HEADS, HD = 64, HID = NSOS_DINO_HIDDEN;
constexpr int IMG = NSOS_DINO_IMAGE, PS = NSOS_DINO_PATCH, GRID = IMG / PS, KE = 3 * PS * PS;   // 14 patches a side, 768 inputs each
static_assert(D == HEADS * HD && NP == GRID * GRID, "ViT-S/16 geometry");

// torch's `nearest` source index (ATen UpSample.h nearest_neighbor_compute_source_index): scale and product in fp32
__host__ __device__ inline int dino_nearest(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    const int s = (int)floorf((float)dst * scale);
    return s < in - 1 ? s : in - 1;
}
// steps 1-2 composed: 224 -> in*stride -> in  (stride <= 0: 224 -> in)
__host__ __device__ inline int dino_source_index(int dst, int in, int stride) {
    if (stride <= 0) return dino_nearest(dst, in, IMG);
    const int mid = in * stride;
    return dino_nearest(dino_nearest(dst, mid, IMG), in, mid);
}

// pixel (c, y, xx) of image b of the prepared [B,3,224,224] network input (flags: NSOS_DINO_*)
__device__ __forceinline__ float dino_prepared_pixel(const float* __restrict__ in, int b, int c, int y, int xx, int in_h, int in_w, int stride,
                                                     int flags) {
    if (flags & NSOS_DINO_PREPARED) return in[(((size_t)b * 3 + c) * IMG + y) * IMG + xx];
    const int s1 = (flags & NSOS_DINO_STEP1) ? stride : 0;
    const int sy = dino_source_index(y, in_h, s1), sx = dino_source_index(xx, in_w, s1);
    float v = (flags & NSOS_DINO_NHWC) ? in[(((size_t)b * in_h + sy) * in_w + sx) * 3 + c] : in[(((size_t)b * 3 + c) * in_h + sy) * in_w + sx];
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    if (flags & NSOS_DINO_STEP1) v = (v - mean) / sd;   // engines/trainer.py:24-29 normalize_batch
    return (v - mean) / sd;                             // models/extractor.py:205-208
}

__device__ __forceinline__ float dino_wave_sum(float v) {   // xor butterfly 32,16,8,4,2,1: every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float dino_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace dino
}  // namespace nsos
