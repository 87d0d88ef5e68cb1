// What the fp32 (dino_vit.hip) and the 16-bit (dino_vit16.hip) DINO ViT-S/16 kernels share: the geometry, the resize index rule and
// the prepared pixel (so that both paths produce the same [B,3,224,224] network input bit for bit), the wave reductions, the
// element-wise kernels (outputs, copy, add) and the argument checks of the pack / forward entry points.
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

using nsos::blocks_for;

// The element-wise kernels are templates over a tag that names the path: each .hip file instantiates its own copies (no ODR
// question between the translation units), and a trace or a per-kernel check of the code object (tests/test_dino16_abi.py) tells
// dino_copy_kernel<dino32_path> from dino_copy_kernel<dino16_path> as it told dino_copy_kernel from dino16_copy_kernel.
struct dino32_path {};
struct dino16_path {};

// ---- outputs: cls = x[:,0], feat = x[:,1:], attn = mean over the heads (0..5 in order) of the saved row 0 ----------------------
template <class Path>
__global__ __launch_bounds__(256) void dino_outputs_kernel(const float* __restrict__ x, const float* __restrict__ row0, int batch,
                                                           float* __restrict__ feat, float* __restrict__ cls, float* __restrict__ attn) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)batch * T * D) return;
    const int c = (int)(e % D), t = (int)((e / D) % T), b = (int)(e / ((long long)T * D));
    const float v = x[e];
    if (t == 0) {
        if (cls) cls[(size_t)b * D + c] = v;
        if (attn && row0)
            for (int j = c; j < NP; j += D) {
                float s = 0.0f;
                for (int h = 0; h < HEADS; ++h) s += row0[((size_t)b * HEADS + h) * NP + j];
                attn[(size_t)b * NP + j] = s / (float)HEADS;
            }
    } else if (feat) {
        feat[((size_t)b * NP + t - 1) * D + c] = v;
    }
}
template <class Path>
__global__ __launch_bounds__(256) void dino_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = src[e];
}
template <class Path>
__global__ __launch_bounds__(256) void dino_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dst, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = a[e] + b[e];
}

// ---- argument checks.  The ORDER is part of the C ABI (a call that is wrong in two ways reports the first; mlp_host.h) ----------
// every pointer of the checkpoint: NSOS_ERR_NULL_POINTER for the table itself or any of its 4 + 12 x 12 tensors
inline int32_t dino_check_tensors(const nsos_dino_tensors* t) {
    NSOS_REQUIRE(t && t->cls_token && t->pos_embed && t->patch_w && t->patch_b, NSOS_ERR_NULL_POINTER);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const nsos_dino_block_tensors& b = t->blocks[i];
        NSOS_REQUIRE(b.norm1_w && b.norm1_b && b.qkv_w && b.qkv_b && b.proj_w && b.proj_b && b.norm2_w && b.norm2_b && b.fc1_w &&
                         b.fc1_b && b.fc2_w && b.fc2_b,
                     NSOS_ERR_NULL_POINTER);
    }
    return NSOS_OK;
}
// nsos_dino_forward / nsos_dino_forward16: NULL pointer -> shape -> flag bits -> [precision] -> PREPARED -> STEP1 -> size limits ->
// alignment -> workspace size.  `need` is the entry point's own workspace-bytes function; fp32 has no precision to refuse.
// nsos_dino_backward takes the same path with its input GRADIENT in the place of `input`; what it has of further pointers joins the NULL
// check (`others`) and the alignment check (`others_aligned`) at their places in the order.
inline int32_t dino_check_forward(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                                  const void* packed, const void* workspace, size_t workspace_bytes, size_t (*need)(int32_t),
                                  bool precision_ok = true, bool others = true, bool others_aligned = true) {
    NSOS_REQUIRE(input && packed && workspace && others, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(batch > 0 && in_h > 0 && in_w > 0, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE((flags & ~7) == 0, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(precision_ok, NSOS_ERR_UNSUPPORTED);
    if (flags & NSOS_DINO_PREPARED) {
        NSOS_REQUIRE(flags == NSOS_DINO_PREPARED, NSOS_ERR_UNSUPPORTED);
        NSOS_REQUIRE(in_h == IMG && in_w == IMG, NSOS_ERR_BAD_SHAPE);
    }
    if (flags & NSOS_DINO_STEP1) {
        NSOS_REQUIRE(patch_stride > 0, NSOS_ERR_BAD_SHAPE);   // an intermediate image of extent 0
        NSOS_REQUIRE(patch_stride <= (1 << 10), NSOS_ERR_UNSUPPORTED);
    }
    NSOS_REQUIRE(batch <= NSOS_DINO_MAX_BATCH && in_h <= (1 << 14) && in_w <= (1 << 14), NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)input & 3) == 0 && others_aligned,
                 NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(workspace_bytes >= need(batch), NSOS_ERR_BUFFER_TOO_SMALL);
    return NSOS_OK;
}

}  // namespace dino
}  // namespace nsos
