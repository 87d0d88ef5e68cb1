// DINO ViT-S/16 feature extractor, the forward, fp32 (include/nerf_sos_hip.h "DINO ViT-S/16").  Its backward to the
// input image is dino_vit_bwd.hip; dino_layout32.h holds what the two share.
// Replaces engines/trainer.py:103-106 (resize + normalize_batch), models/extractor.py:204-213 (get_vit_attn_feat) and
// models/vision_transformer.py:196-215 (vit_small(patch_size=16): prepare_tokens + 12 blocks) with four kernels:
//   dino_prepare_kernel   steps 1-2 (two nearest resizes as one gather, two normalisations) fused with the patch embedding's im2col
//   dino_gemm_kernel      C = A[M,K] . Wt[K,N] on v_mfma_f32_32x32x2_f32, epilogue bias / GELU / residual / (embedding) + pos_embed
//   dino_layernorm_kernel one wave per token row of 384
//   dino_attention_kernel one workgroup per (32 query rows, head, image) on v_mfma_f32_16x16x4_f32
// and, for the full-image path of engines/eval.py:133-144 (models/extractor.py:215-224 get_vit_attn_feat_noresize, DESIGN.md
// 4.10.1), a runtime patch grid: dino_full_pos_kernel (bicubic position embedding), dino_full_prepare_kernel, the same GEMM and
// LayerNorm, dino_flash_attention_kernel (streaming, online softmax) and the find_fg kernels dino_fg_*.
// Every sum runs in a fixed order (the header states it); no atomics; each workgroup reads one image only, so an image's bits do
// not depend on the batch it travels in.
#include "common.h"
#include "mlp_common.h"
#include "dino_common.h"
#include "gemm32_tile.h"
#include "dino_layout32.h"   // the packed stream and the workspace (shared with dino_vit_bwd.hip)

namespace {

using namespace nsos::dino;   // geometry, resize index rule, prepared pixel, wave reductions: dino_common.h
using namespace nsos::dino32;

// ---- prepare: tokens[b*196 + t][c*256 + py*16 + px] = prepared[b][c][16*ty + py][16*tx + px]; also x[b][0][:] = cls + pos[0] ----
__global__ __launch_bounds__(256) void dino_prepare_kernel(const float* __restrict__ in, int batch, int in_h, int in_w, int stride, int flags,
                                                           const float* __restrict__ clspos, float* __restrict__ tokens, float* __restrict__ x,
                                                           float* __restrict__ prepared) {
    const long long n = (long long)batch * NP * KE;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int k = (int)(e % KE);
    const int t = (int)((e / KE) % NP);
    const int b = (int)(e / ((long long)KE * NP));
    const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
    const int y = (t / GRID) * PS + py, xx = (t % GRID) * PS + px;
    const float v = dino_prepared_pixel(in, b, c, y, xx, in_h, in_w, stride, flags);
    tokens[e] = v;
    if (prepared) prepared[(((size_t)b * 3 + c) * IMG + y) * IMG + xx] = v;
    if (t == 0 && k < D) x[(size_t)b * T * D + k] = clspos[k];
}

// ---- GEMM: out[M,N] = epilogue(A[M,K] . Wt[K,N]) on the shared 64x64x32 tile (gemm32_tile.h): dense A rows, one fma chain over K.
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESIDUAL = 2, EPI_EMBED = 3 };
using nsos::gemm32::GK;
using nsos::gemm32::GM;
using nsos::gemm32::GN;

// K is a template parameter: a constant trip count, and proj (K 384) / fc2 (K 1536) show up as separate kernels in a trace.
template <int EPI, int K>
__global__ __launch_bounds__(256) void dino_gemm_kernel(const float* __restrict__ A, const float* __restrict__ Wt, const float* __restrict__ bias,
                                                        float* out, const float* extra, int M, int N, int np) {
    const int m0 = blockIdx.y * GM, n0 = blockIdx.x * GN;
    const int ar = nsos::gemm32::a_row(), ak = nsos::gemm32::a_k();
    const int row0 = min(m0 + ar, M - 1), row1 = min(m0 + ar + 32, M - 1);   // rows past M repeat the last one; never stored
    float* out_col = out + nsos::gemm32::out_col(n0);   // column bases: one 64-bit add per row in the epilogue
    const float* extra_col = (EPI == EPI_RESIDUAL || EPI == EPI_EMBED) ? extra + nsos::gemm32::out_col(n0) : nullptr;
    nsos::gemm32::tile<nsos::gemm32::OneChain>(
        K, m0, n0, M, Wt, bias, N,
        [&](int k0, float4(&ra)[2]) {
            ra[0] = *reinterpret_cast<const float4*>(A + (size_t)row0 * K + k0 + ak);
            ra[1] = *reinterpret_cast<const float4*>(A + (size_t)row1 * K + k0 + ak);
        },
        [&](int row, int, float v) {
            if constexpr (EPI == EPI_GELU) v = v * 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
            if constexpr (EPI == EPI_RESIDUAL) v = extra_col[(size_t)row * N] + v;
            if constexpr (EPI == EPI_EMBED) {   // row = b*np + t -> token row b*(np+1) + 1 + t; + pos_embed[1 + t]  (np = 196 at 224x224)
                const int b = row / np, t = row - b * np;
                v = v + extra_col[(size_t)(1 + t) * N];
                out_col[((size_t)b * (np + 1) + 1 + t) * N] = v;
            } else {
                out_col[(size_t)row * N] = v;
            }
        });
}

// ---- LayerNorm over 384, eps 1e-6 (biased variance about the mean, as nn.LayerNorm); one wave per row ---------------------------
__global__ __launch_bounds__(256) void dino_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             float* __restrict__ y, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * D;
    float v[6], s = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] = xr[lane + 64 * j], s += v[j];
    const float mean = dino_wave_sum(s) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] -= mean, q += v[j] * v[j];
    const float rstd = 1.0f / sqrtf(dino_wave_sum(q) / (float)D + 1e-6f);
#pragma unroll
    for (int j = 0; j < 6; ++j) y[(size_t)row * D + lane + 64 * j] = v[j] * rstd * w[lane + 64 * j] + b[lane + 64 * j];
}

// ---- attention (models/vision_transformer.py:80-92): softmax(q k^T / 8) v for 32 query rows of one head of one image -----------
constexpr int QT = 32, LDQ = 66, LDK = 66, LDV = 80, TP = 200, LDP = 226;   // strides: conflict-free 16x16x4 operand reads (32 banks)
constexpr int KV_FLOATS = (T * LDK > TP * LDV) ? T * LDK : TP * LDV;
constexpr int ATT_LDS_BYTES = (QT * LDQ + KV_FLOATS + QT * LDP) * 4;
static_assert(ATT_LDS_BYTES <= 160 * 1024, "one CU's LDS");

__global__ __launch_bounds__(256) void dino_attention_kernel(const float* __restrict__ qkv, float* __restrict__ ao, float* __restrict__ row0) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [32][LDQ]
    float* KVs = Qs + QT * LDQ;         // K [197][LDK], later V [200][LDV]
    float* Ps = KVs + KV_FLOATS;        // scores, then probabilities [32][LDP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * QT, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * 3 * D + h * HD;
    for (int i = tid; i < QT * (HD / 4); i += 256) {   // query rows past 196 repeat row 196; their results are never stored
        const int r = i >> 4, c = (i & 15) * 4;
        const float4 v = *reinterpret_cast<const float4*>(base + (size_t)min(q0 + r, T - 1) * 3 * D + c);
        float* d = Qs + r * LDQ + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    for (int i = tid; i < T * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float4 v = *reinterpret_cast<const float4*>(base + (size_t)r * 3 * D + D + c);
        float* d = KVs + r * LDK + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    __syncthreads();
    // scores: 13 column tiles of 16 keys (the last: keys 192..207, clamped to 196 and masked below), both 16-row halves per wave
    const int li = lane & 15, lk = lane >> 4;
    for (int tj = wave; tj < 13; tj += 4) {
        f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
        const float* qa = Qs + li * LDQ + lk;
        const float* kb = KVs + min(tj * 16 + li, T - 1) * LDK + lk;
#pragma unroll
        for (int k0 = 0; k0 < HD; k0 += 4) {   // d ascending
            const float bb = kb[k0];
            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[k0], bb, s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[16 * LDQ + k0], bb, s1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // C/D: col = lane & 15, row = 4 * (lane >> 4) + r
            Ps[(lk * 4 + r) * LDP + tj * 16 + li] = s0[r] * 0.125f;   // scale = 64^-0.5
            Ps[(16 + lk * 4 + r) * LDP + tj * 16 + li] = s1[r] * 0.125f;
        }
    }
    __syncthreads();   // K is dead from here: V takes its place
    for (int i = tid; i < TP * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};   // keys 197..199: zero rows under zero probabilities
        if (r < T) v = *reinterpret_cast<const float4*>(base + (size_t)r * 3 * D + 2 * D + c);
        *reinterpret_cast<float4*>(KVs + r * LDV + c) = v;
    }
    // softmax with the row maximum subtracted: wave w owns rows 8w..8w+7, a lane the columns lane, lane+64, lane+128, lane+192
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        float* pr = Ps + r * LDP;
        float v[4], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            v[j] = c < T ? pr[c] : -INFINITY;
            m = fmaxf(m, v[j]);
        }
        m = dino_wave_max(m);
        float s = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = (lane + 64 * j) < T ? expf(v[j] - m) : 0.0f;
            s += v[j];
        }
        s = dino_wave_sum(s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c < TP) pr[c] = v[j] / s;
        }
    }
    __syncthreads();
    if (row0 && q0 == 0 && tid < NP) row0[((size_t)b * HEADS + h) * NP + tid] = Ps[1 + tid];   // block 11: row 0, columns 1..196
    // out = P V: wave w owns output columns 16w..16w+15, both row halves; keys ascending
    {
        f32x4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0;
        const float* pa = Ps + li * LDP + lk;
        const float* vb = KVs + lk * LDV + wave * 16 + li;
#pragma unroll 10
        for (int k0 = 0; k0 < TP; k0 += 4) {
            const float bb = vb[k0 * LDV];
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k0], bb, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[16 * LDP + k0], bb, o1, 0, 0, 0);
        }
        float* dst = ao + (size_t)b * T * D + h * HD + wave * 16 + li;   // (attn @ v).transpose(1, 2).reshape(B, N, C)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ra = q0 + lk * 4 + r, rb = ra + 16;
            if (ra < T) dst[(size_t)ra * D] = o0[r];
            if (rb < T) dst[(size_t)rb * D] = o1[r];
        }
    }
}

// dst[i][o] = src[o][i]  (nn.Linear [out,in] -> the GEMM's [in,out])
__global__ __launch_bounds__(256) void dino_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int n_out, int n_in) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_out * n_in) return;
    const int o = (int)(e % n_out), i = (int)(e / n_out);
    dst[e] = src[(size_t)o * n_in + i];
}

template <int EPI, int K>
void launch_gemm(const float* A, const float* Wt, const float* bias, float* out, const float* extra, int M, int N, hipStream_t st, int np = NP) {
    static_assert(K % GK == 0, "GEMM tiles");
    dino_gemm_kernel<EPI, K><<<dim3(N / GN, (M + GM - 1) / GM), 256, 0, st>>>(A, Wt, bias, out, extra, M, N, np);
}

// The attention kernel's 99 KB of dynamic LDS needs the attribute once per device.  nsos_dino_pack sets it too, so a forward call
// that is the first one inside a stream capture finds it done.
int32_t dino_configure() {
    static NsosPerDeviceFlag configured;
    if (!configured.here()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dino_attention_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           ATT_LDS_BYTES);
        if (e != hipSuccess) return (int32_t)e;
        configured.here() = true;
    }
    return NSOS_OK;
}
static_assert(D % GN == 0 && (3 * D) % GN == 0 && HID % GN == 0 && D % GK == 0 && KE % GK == 0 && HID % GK == 0, "GEMM tiles");

// ================================================================================================================================
// Full-image path (models/extractor.py:215-224 get_vit_attn_feat_noresize, as engines/eval.py:133-144 calls it for find_fg):
// a runtime patch grid rows x cols = (H // 16) x (W // 16), T = 1 + rows*cols tokens, the position embedding interpolated.
// ================================================================================================================================
constexpr int FULL_MAX_NP = NSOS_DINO_FULL_MAX_PATCHES;

// models/vision_transformer.py:174-194 for patch token t of a rows x cols grid, channel c.  pos: the packed [197][384] table (row
// 1 + i*14 + j = grid cell (i, j)).  npatch == 196 and H == W: the table as it is.  Otherwise ATen's upsample_bicubic2d with
// align_corners=False and scale_factor sf = (rows + 0.1) / 14: source coordinate (dst + 0.5) * (1 / sf) - 0.5, taps floor - 1 ..
// floor + 2 clamped to the grid, A = -0.75, a row of four x-interpolations then one y-interpolation -- evaluated in fp64 (the
// fp64 reference's arithmetic) and rounded once.
__host__ __device__ inline void dino_cubic_coeffs(double t, double c[4]) {
    const double A = -0.75;
    auto c1 = [&](double x) { return ((A + 2) * x - (A + 3)) * x * x + 1; };
    auto c2 = [&](double x) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; };
    c[0] = c2(t + 1.0), c[1] = c1(t), c[2] = c1(1.0 - t), c[3] = c2(2.0 - t);
}
__host__ __device__ inline float dino_pos_value(const float* pos, int rows, int cols, int h, int w, int t, int c) {
    if (rows * cols == NP && h == w) return pos[(size_t)(1 + t) * D + c];
    const int oy = t / cols, ox = t - oy * cols;
    const double ry = (1.0 / ((rows + 0.1) / (double)GRID)) * (oy + 0.5) - 0.5, rx = (1.0 / ((cols + 0.1) / (double)GRID)) * (ox + 0.5) - 0.5;
    const double fy = floor(ry), fx = floor(rx);
    double cy[4], cx[4];
    dino_cubic_coeffs(ry - fy, cy);
    dino_cubic_coeffs(rx - fx, cx);
    const int iy = (int)fy, ix = (int)fx;
    double acc = 0.0;
    for (int i = 0; i < 4; ++i) {
        const int yy = min(max(iy - 1 + i, 0), GRID - 1);
        double r = 0.0;
        for (int j = 0; j < 4; ++j) r = r + (double)pos[(size_t)(1 + yy * GRID + min(max(ix - 1 + j, 0), GRID - 1)) * D + c] * cx[j];
        acc = acc + r * cy[i];
    }
    return (float)acc;
}

// table[t][c], t = 0..T-1: row 0 is the packed cls_token + pos_embed[0] (the class position is prepended unchanged)
__global__ __launch_bounds__(256) void dino_full_pos_kernel(const float* __restrict__ pos, int rows, int cols, int h, int w,
                                                            float* __restrict__ table) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int np = rows * cols;
    if (e >= (long long)(np + 1) * D) return;
    const int c = (int)(e % D), t = (int)(e / D);
    table[e] = t == 0 ? pos[c] : dino_pos_value(pos, rows, cols, h, w, t - 1, c);
}

// tokens[b*np + t][c*256 + py*16 + px] = image[b][c][16*ty + py][16*tx + px] (t = ty*cols + tx; the remainder rows / columns are
// never read), normalised once ((v - mean) / std, models/extractor.py:217-219) or, with NORMALIZE, twice (engines/eval.py:136 first);
// also x[b][0][:] = cls_token + pos_embed[0]
__global__ __launch_bounds__(256) void dino_full_prepare_kernel(const float* __restrict__ in, int batch, int h, int w, int cols, int np,
                                                                int flags, const float* __restrict__ clspos, float* __restrict__ tokens,
                                                                float* __restrict__ x) {
    const long long n = (long long)batch * np * KE;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int k = (int)(e % KE);
    const int t = (int)((e / KE) % np);
    const int b = (int)(e / ((long long)KE * np));
    const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
    const int y = (t / cols) * PS + py, xx = (t % cols) * PS + px;
    float v = (flags & NSOS_DINO_FULL_NHWC) ? in[(((size_t)b * h + y) * w + xx) * 3 + c] : in[(((size_t)b * 3 + c) * h + y) * w + xx];
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    if (flags & NSOS_DINO_FULL_NORMALIZE) v = (v - mean) / sd;   // engines/eval.py:24-29 normalize_batch
    v = (v - mean) / sd;                                         // models/extractor.py:219
    tokens[e] = v;
    if (t == 0 && k < D) x[(size_t)b * (np + 1) * D + k] = clspos[k];
}

// ---- streaming attention: softmax(q k^T / 8) v for 64 query rows (16 per wave) of one head of one image, any T ------------------
// K/V tiles of 64 keys, ascending, register-staged (the next tile's global loads are in flight under this tile's MFMAs) and shared
// by the four waves through LDS.  Per query row a running maximum m and sum l (online softmax): per tile
//   s = (q / 8) . k   (d = 0..63 ascending, v_mfma_f32_16x16x4_f32; scaling q by 2^-3 first is exact)
//   m' = max(m, max_tile s); a = exp(m - m'); p = exp(s - m'); l = l * a + sum_tile p; o = o * a + p . v (keys ascending)
// with the tile's row max / sum taken over a lane's four column blocks in order, then an xor butterfly 1, 2, 4, 8 over the 16 lanes
// of the row; at the end o / l.  With `sc0`, the tile holding query 0 stores its scaled scores (every key) and final (m, l).
constexpr int FQ = 64, FK = 64, FLDK = 66, FLDV = 80, FLDP = 66;

__device__ __forceinline__ float dino_row16_max(float v) {
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float dino_row16_sum(float v) {
#pragma unroll
    for (int m = 1; m <= 8; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void dino_flash_attention_kernel(const float* __restrict__ qkv, float* __restrict__ ao, int T,
                                                                   float* __restrict__ sc0, float* __restrict__ ml0) {
    __shared__ __attribute__((aligned(16))) float Ks[FK * FLDK];
    __shared__ __attribute__((aligned(16))) float Vs[FK * FLDV];
    __shared__ float Ps[4 * 16 * FLDP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int q0 = blockIdx.x * FQ + wave * 16, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * 3 * D + h * HD;
    float qa[16];   // A operand: row li, d = 4j + lk; rows past T repeat the last one and are never stored
    {
        const float* qr = base + (size_t)min(q0 + li, T - 1) * 3 * D + lk;
#pragma unroll
        for (int j = 0; j < 16; ++j) qa[j] = qr[4 * j] * 0.125f;
    }
    float4 rk[4], rv[4];
    auto gload = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tid + 256 * j, key = k0 + (i >> 4), c = (i & 15) * 4;
            rk[j] = rv[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // keys past T: zero rows, masked below
            if (key < T) {
                rk[j] = *reinterpret_cast<const float4*>(base + (size_t)key * 3 * D + D + c);
                rv[j] = *reinterpret_cast<const float4*>(base + (size_t)key * 3 * D + 2 * D + c);
            }
        }
    };
    const bool row0 = sc0 && q0 == 0;
    float* Pw = Ps + wave * 16 * FLDP;
    float m[4], l[4];
    f32x4 o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = -INFINITY, l[r] = 0.0f, o[r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int nt = (T + FK - 1) / FK;
    gload(0);
    for (int kt = 0; kt < nt; ++kt) {
        __syncthreads();   // the previous tile has been consumed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tid + 256 * j, r = i >> 4, c = (i & 15) * 4;
            *reinterpret_cast<float2*>(Ks + r * FLDK + c) = make_float2(rk[j].x, rk[j].y);
            *reinterpret_cast<float2*>(Ks + r * FLDK + c + 2) = make_float2(rk[j].z, rk[j].w);
            *reinterpret_cast<float4*>(Vs + r * FLDV + c) = rv[j];
        }
        __syncthreads();
        if (kt + 1 < nt) gload((kt + 1) * FK);
        f32x4 s[4];
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) {   // C/D: key column tj*16 + li, query row 4*lk + r
            s[tj] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const float* kb = Ks + (tj * 16 + li) * FLDK + lk;
#pragma unroll
            for (int j = 0; j < 16; ++j) s[tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[j], kb[4 * j], s[tj], 0, 0, 0);
            const int key = kt * FK + tj * 16 + li;
            if (key >= T) s[tj] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (row0 && lk == 0 && key < T) sc0[((size_t)b * HEADS + h) * T + key] = s[tj][0];
        }
        float a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mx = fmaxf(fmaxf(s[0][r], s[1][r]), fmaxf(s[2][r], s[3][r]));
            const float mn = fmaxf(m[r], dino_row16_max(mx));
            a[r] = expf(m[r] - mn);   // exp(-inf) = 0 on the first tile
            float sum = 0.0f;
#pragma unroll
            for (int tj = 0; tj < 4; ++tj) {
                const float p = expf(s[tj][r] - mn);
                sum += p;
                Pw[(4 * lk + r) * FLDP + tj * 16 + li] = p;
            }
            l[r] = l[r] * a[r] + dino_row16_sum(sum);
            m[r] = mn;
        }
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[db][r] *= a[r];
        __builtin_amdgcn_wave_barrier();
        const float* pa = Pw + li * FLDP + lk;   // A operand: query row li, key k0 + lk
#pragma unroll
        for (int k0 = 0; k0 < FK; k0 += 4) {
            const float av = pa[k0];
            const float* vb = Vs + (k0 + lk) * FLDV + li;
#pragma unroll
            for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, vb[db * 16], o[db], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = q0 + 4 * lk + r;
        if (row >= T) continue;
        float* dst = ao + ((size_t)b * T + row) * D + h * HD + li;   // (attn @ v).transpose(1, 2).reshape(B, N, C)
#pragma unroll
        for (int db = 0; db < 4; ++db) dst[db * 16] = o[db][r] / l[r];
    }
    if (row0 && lane == 0) ml0[((size_t)b * HEADS + h) * 2] = m[0], ml0[((size_t)b * HEADS + h) * 2 + 1] = l[0];
}

// cls = x[:,0], feat = x[:,1:]; attn[b][j] = (sum over heads 0..5 in order of exp(s_h[1+j] - m_h) / l_h) / 6
__global__ __launch_bounds__(256) void dino_full_outputs_kernel(const float* __restrict__ x, const float* __restrict__ sc0,
                                                                const float* __restrict__ ml0, int batch, int T, float* __restrict__ feat,
                                                                float* __restrict__ cls, float* __restrict__ attn) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)batch * T * D) return;
    const int c = (int)(e % D), t = (int)((e / D) % T), b = (int)(e / ((long long)T * D));
    const float v = x[e];
    if (t == 0) {
        if (cls) cls[(size_t)b * D + c] = v;
        if (attn)
            for (int j = c; j < T - 1; j += D) {
                float s = 0.0f;
                for (int hh = 0; hh < HEADS; ++hh) {
                    const size_t q = (size_t)b * HEADS + hh;
                    s += expf(sc0[q * T + 1 + j] - ml0[2 * q]) / ml0[2 * q + 1];
                }
                attn[(size_t)b * (T - 1) + j] = s / (float)HEADS;
            }
    } else if (feat) {
        feat[((size_t)b * (T - 1) + t - 1) * D + c] = v;
    }
}

// workspace of the full path, in floats (every section a multiple of 4: 16-byte aligned); 0 = refused.  The patch tokens share
// the MLP's hidden section (used before block 0 only).
struct FullLayout {
    size_t pos, sc0, ml0, x, ln, qkv, ao, hid, total;
};
inline size_t round4(size_t n) { return (n + 3) & ~(size_t)3; }
bool full_layout(long long batch, long long h, long long w, FullLayout& L) {
    if (batch < 1 || batch > NSOS_DINO_MAX_BATCH || h < PS || w < PS) return false;
    const long long rows = h / PS, cols = w / PS;
    if (rows > FULL_MAX_NP || cols > FULL_MAX_NP || rows * cols > FULL_MAX_NP) return false;
    const long long T = rows * cols + 1, M = batch * T;
    if ((M + GM - 1) / GM > 65535) return false;   // the GEMMs' grid rows
    size_t s = 0;
    const size_t Bn = (size_t)batch, Tn = (size_t)T;
    auto add = [&](size_t n, size_t& off) -> bool {
        off = s;
        if (__builtin_add_overflow(s, round4(n), &s)) return false;
        return true;
    };
    size_t btd;
    if (__builtin_mul_overflow(Bn * Tn, (size_t)D, &btd)) return false;
    bool ok = add(Tn * D, L.pos) && add(Bn * HEADS * Tn, L.sc0) && add(Bn * HEADS * 2, L.ml0) && add(btd, L.x) && add(btd, L.ln) &&
              add(btd * 3, L.qkv) && add(btd, L.ao) && add(btd * (HID / D), L.hid);
    if (!ok || s > SIZE_MAX / sizeof(float)) return false;
    L.total = s;
    return true;
}

// ---- find_fg (engines/eval.py:138-144): per-cluster sums of the nearest-upsampled attention, fp64, in a fixed two-stage order ---
constexpr int FG_BLOCKS = 256;
constexpr size_t FG_WS_BYTES = (size_t)FG_BLOCKS * 4 * sizeof(double) + 16;

// block g takes pixels [g*chunk, (g+1)*chunk), thread i every 256th of them ascending; then a tree over the 256 threads (128, 64, .. 1)
__global__ __launch_bounds__(256) void dino_fg_partial_kernel(const int32_t* __restrict__ labels, const float* __restrict__ attn, int h,
                                                              int w, float* __restrict__ attn_up, double* __restrict__ part) {
    __shared__ double red[4][256];
    const int rows = h / PS, cols = w / PS, tid = threadIdx.x;
    const long long n = (long long)h * w, chunk = (n + FG_BLOCKS - 1) / FG_BLOCKS;
    const long long lo = blockIdx.x * chunk, hi = min(n, lo + chunk);
    double s0 = 0.0, s1 = 0.0, c0 = 0.0, c1 = 0.0;
    for (long long i = lo + tid; i < hi; i += 256) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const float a = attn[(size_t)dino_nearest(y, rows, h) * cols + dino_nearest(x, cols, w)];   // F.interpolate(attn, (H, W))
        if (attn_up) attn_up[i] = a;
        const int32_t lab = labels[i];
        if (lab == 0) s0 += (double)a, c0 += 1.0;
        if (lab == 1) s1 += (double)a, c1 += 1.0;
    }
    red[0][tid] = s0, red[1][tid] = s1, red[2][tid] = c0, red[3][tid] = c1;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st)
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + st];
        __syncthreads();
    }
    if (tid < 4) part[(size_t)blockIdx.x * 4 + tid] = red[tid][0];
}

// the 256 partials by the same tree; mean = sum / count (0 / 0 = NaN for an empty cluster); flip = mean1 < mean0 (False with a NaN)
__global__ __launch_bounds__(256) void dino_fg_finish_kernel(const double* __restrict__ part, int32_t* __restrict__ flag,
                                                             double* __restrict__ means, int32_t* __restrict__ flipped) {
    __shared__ double red[4][256];
    const int tid = threadIdx.x;
    for (int q = 0; q < 4; ++q) red[q][tid] = part[(size_t)tid * 4 + q];
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if (tid < st)
            for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        const double m0 = red[0][0] / red[2][0], m1 = red[1][0] / red[3][0];
        const int32_t f = m1 < m0 ? 1 : 0;
        flag[0] = f;
        if (means) means[0] = m0, means[1] = m1;
        if (flipped) flipped[0] = f;
    }
}

// clustering = 1 - clustering where flipped (np.ones_like(c) - c: 2 -> -1; wrapping int32 arithmetic, as numpy's)
__global__ __launch_bounds__(256) void dino_fg_apply_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ flag, long long n,
                                                            int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t v = (uint32_t)labels[i];
    out[i] = (int32_t)(flag[0] ? 1u - v : v);
}
static_assert(FG_BLOCKS == 256, "the finishing tree reads one partial per thread");

}  // namespace

extern "C" size_t nsos_dino_packed_bytes(void) { return P_SIZE * sizeof(float); }

extern "C" size_t nsos_dino_workspace_bytes(int32_t batch) {
    return (batch >= 1 && batch <= NSOS_DINO_MAX_BATCH) ? (size_t)batch * W_SIZE * sizeof(float) : 0;
}

extern "C" int32_t nsos_dino_resize_indices(int32_t in_size, int32_t patch_stride, int32_t* idx) {
    NSOS_REQUIRE(idx, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(in_size > 0, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(in_size <= (1 << 14) && patch_stride <= (1 << 10), NSOS_ERR_UNSUPPORTED);
    for (int i = 0; i < IMG; ++i) idx[i] = dino_source_index(i, in_size, patch_stride);
    return NSOS_OK;
}

extern "C" int32_t nsos_dino_pack(const nsos_dino_tensors* t, void* packed, size_t packed_bytes, void* stream) {
    NSOS_REQUIRE(packed, NSOS_ERR_NULL_POINTER);
    if (int32_t c = dino_check_tensors(t)) return c;
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(packed_bytes >= P_SIZE * sizeof(float), NSOS_ERR_BUFFER_TOO_SMALL);
    if (int32_t c = dino_configure()) return c;
    hipStream_t st = (hipStream_t)stream;
    float* p = (float*)packed;
    auto copy = [&](const float* src, float* dst, long long n) {
        dino_copy_kernel<dino32_path><<<blocks_for(n), 256, 0, st>>>(src, dst, n);
    };
    auto transpose = [&](const float* src, float* dst, int n_out, int n_in) {
        dino_transpose_kernel<<<blocks_for((long long)n_out * n_in), 256, 0, st>>>(src, dst, n_out, n_in);
    };
    copy(t->pos_embed + D, p + P_POS + D, (long long)NP * D);
    dino_add_kernel<dino32_path><<<blocks_for(D), 256, 0, st>>>(t->cls_token, t->pos_embed, p + P_POS, D);
    transpose(t->patch_w, p + P_EMB_W, D, KE);
    copy(t->patch_b, p + P_EMB_B, D);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const nsos_dino_block_tensors& b = t->blocks[i];
        float* q = p + P_BLOCKS + (size_t)i * B_SIZE;
        copy(b.norm1_w, q + B_LN1W, D), copy(b.norm1_b, q + B_LN1B, D);
        transpose(b.qkv_w, q + B_QKVW, 3 * D, D), copy(b.qkv_b, q + B_QKVB, 3 * D);
        transpose(b.proj_w, q + B_PROJW, D, D), copy(b.proj_b, q + B_PROJB, D);
        copy(b.norm2_w, q + B_LN2W, D), copy(b.norm2_b, q + B_LN2B, D);
        transpose(b.fc1_w, q + B_FC1W, HID, D), copy(b.fc1_b, q + B_FC1B, HID);
        transpose(b.fc2_w, q + B_FC2W, D, HID), copy(b.fc2_b, q + B_FC2B, D);
    }
    return nsos_launch_status();
}

// nsos_dino_forward (saved == nullptr: exactly its launches) and nsos_dino_forward_save (saved[i] = the input of block i)
static int32_t dino_forward32(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                              const void* packed, void* workspace, float* feat, float* cls, float* attn, float* prepared, float* blocks,
                              float* saved, void* stream) {
    if (int32_t c = dino_configure()) return c;
    hipStream_t st = (hipStream_t)stream;
    const float* p = (const float*)packed;
    float* ws = (float*)workspace;
    const size_t Bn = (size_t)batch;
    float *x = ws + Bn * W_X, *ln = ws + Bn * W_LN, *qkv = ws + Bn * W_QKV, *ao = ws + Bn * W_AO, *hid = ws + Bn * W_HID,
          *tok = ws + Bn * W_TOK, *row0 = ws + Bn * W_ROW0;
    const int M = batch * T;

    dino_prepare_kernel<<<blocks_for((long long)batch * NP * KE), 256, 0, st>>>(input, batch, in_h, in_w, patch_stride, flags, p + P_POS, tok, x,
                                                                                prepared);
    launch_gemm<EPI_EMBED, KE>(tok, p + P_EMB_W, p + P_EMB_B, x, p + P_POS, batch * NP, D, st);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const float* q = p + P_BLOCKS + (size_t)i * B_SIZE;
        if (saved)
            dino_copy_kernel<dino32_path><<<blocks_for((long long)M * D), 256, 0, st>>>(x, saved + (size_t)i * M * D, (long long)M * D);
        dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x, q + B_LN1W, q + B_LN1B, ln, M);
        launch_gemm<EPI_BIAS, D>(ln, q + B_QKVW, q + B_QKVB, qkv, nullptr, M, 3 * D, st);
        dino_attention_kernel<<<dim3((T + QT - 1) / QT, HEADS, batch), 256, ATT_LDS_BYTES, st>>>(
            qkv, ao, (i == NSOS_DINO_DEPTH - 1 && attn) ? row0 : nullptr);
        launch_gemm<EPI_RESIDUAL, D>(ao, q + B_PROJW, q + B_PROJB, x, x, M, D, st);
        dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x, q + B_LN2W, q + B_LN2B, ln, M);
        launch_gemm<EPI_GELU, D>(ln, q + B_FC1W, q + B_FC1B, hid, nullptr, M, HID, st);
        launch_gemm<EPI_RESIDUAL, HID>(hid, q + B_FC2W, q + B_FC2B, x, x, M, D, st);
        if (blocks)
            dino_copy_kernel<dino32_path><<<blocks_for((long long)M * D), 256, 0, st>>>(x, blocks + (size_t)i * M * D, (long long)M * D);
    }
    if (feat || cls || attn)
        dino_outputs_kernel<dino32_path><<<blocks_for((long long)M * D), 256, 0, st>>>(x, attn ? row0 : nullptr, batch, feat, cls,
                                                                                       attn);
    return nsos_launch_status();
}

extern "C" int32_t nsos_dino_forward(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                                     const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn,
                                     float* prepared, float* blocks, void* stream) {
    if (int32_t c = dino_check_forward(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, workspace_bytes, nsos_dino_workspace_bytes))
        return c;
    return dino_forward32(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, feat, cls, attn, prepared, blocks, nullptr, stream);
}

extern "C" int32_t nsos_dino_forward_save(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                                          const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn,
                                          float* saved, void* stream) {
    if (int32_t c = dino_check_forward(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, workspace_bytes, nsos_dino_workspace_bytes,
                                       true, saved != nullptr, ((uintptr_t)saved & 15) == 0))
        return c;
    return dino_forward32(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, feat, cls, attn, nullptr, nullptr, saved, stream);
}

// ---- for dino_vit_bwd.hip (dino_layout32.h) ------------------------------------------------------------------------------------
int32_t nsos::dino32::configure() { return dino_configure(); }

void nsos::dino32::recompute_block(const float* q, const float* x_in, float* xmid, float* ln, float* qkv, float* ao, float* hid, int batch,
                                   hipStream_t st) {
    const int M = batch * T;
    dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x_in, q + B_LN1W, q + B_LN1B, ln, M);
    launch_gemm<EPI_BIAS, D>(ln, q + B_QKVW, q + B_QKVB, qkv, nullptr, M, 3 * D, st);
    dino_attention_kernel<<<dim3((T + QT - 1) / QT, HEADS, batch), 256, ATT_LDS_BYTES, st>>>(qkv, ao, nullptr);
    launch_gemm<EPI_RESIDUAL, D>(ao, q + B_PROJW, q + B_PROJB, xmid, x_in, M, D, st);
    dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(xmid, q + B_LN2W, q + B_LN2B, ln, M);
    launch_gemm<EPI_BIAS, D>(ln, q + B_FC1W, q + B_FC1B, hid, nullptr, M, HID, st);
}

// ---- full-image path -----------------------------------------------------------------------------------------------------------
extern "C" size_t nsos_dino_full_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    FullLayout L;
    return full_layout(batch, h, w, L) ? L.total * sizeof(float) : 0;
}

extern "C" int32_t nsos_dino_interp_pos(const float* pos_embed, int32_t h, int32_t w, float* out) {
    NSOS_REQUIRE(pos_embed && out, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(h >= PS && w >= PS, NSOS_ERR_BAD_SHAPE);
    const long long rows = h / PS, cols = w / PS;
    NSOS_REQUIRE(rows <= FULL_MAX_NP && cols <= FULL_MAX_NP && rows * cols <= FULL_MAX_NP, NSOS_ERR_UNSUPPORTED);
    for (int c = 0; c < D; ++c) out[c] = pos_embed[c];
    for (int t = 0; t < (int)(rows * cols); ++t)
        for (int c = 0; c < D; ++c) out[(size_t)(1 + t) * D + c] = dino_pos_value(pos_embed, (int)rows, (int)cols, h, w, t, c);
    return NSOS_OK;
}

extern "C" int32_t nsos_dino_forward_full(const float* input, int32_t batch, int32_t h, int32_t w, int32_t flags, const void* packed,
                                          void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn, float* pos,
                                          void* stream) {
    NSOS_REQUIRE(input && packed && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(batch > 0 && h >= PS && w >= PS, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE((flags & ~(NSOS_DINO_FULL_NHWC | NSOS_DINO_FULL_NORMALIZE)) == 0, NSOS_ERR_UNSUPPORTED);
    FullLayout L;
    NSOS_REQUIRE(full_layout(batch, h, w, L), NSOS_ERR_UNSUPPORTED);   // batch, token cap, grid, size_t
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)input & 3) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(workspace_bytes >= L.total * sizeof(float), NSOS_ERR_BUFFER_TOO_SMALL);

    if (int32_t c = dino_configure()) return c;
    hipStream_t st = (hipStream_t)stream;
    const float* p = (const float*)packed;
    float* ws = (float*)workspace;
    const int rows = h / PS, cols = w / PS, np = rows * cols, Tn = np + 1, M = batch * Tn;
    float *table = ws + L.pos, *sc0 = ws + L.sc0, *ml0 = ws + L.ml0, *x = ws + L.x, *ln = ws + L.ln, *qkv = ws + L.qkv, *ao = ws + L.ao,
          *hid = ws + L.hid, *tok = hid;

    dino_full_pos_kernel<<<blocks_for((long long)Tn * D), 256, 0, st>>>(p + P_POS, rows, cols, h, w, table);
    dino_full_prepare_kernel<<<blocks_for((long long)batch * np * KE), 256, 0, st>>>(input, batch, h, w, cols, np, flags, p + P_POS, tok, x);
    launch_gemm<EPI_EMBED, KE>(tok, p + P_EMB_W, p + P_EMB_B, x, table, batch * np, D, st, np);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const float* q = p + P_BLOCKS + (size_t)i * B_SIZE;
        const bool last = i == NSOS_DINO_DEPTH - 1 && attn;
        dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x, q + B_LN1W, q + B_LN1B, ln, M);
        launch_gemm<EPI_BIAS, D>(ln, q + B_QKVW, q + B_QKVB, qkv, nullptr, M, 3 * D, st);
        dino_flash_attention_kernel<<<dim3((Tn + FQ - 1) / FQ, HEADS, batch), 256, 0, st>>>(qkv, ao, Tn, last ? sc0 : nullptr,
                                                                                            last ? ml0 : nullptr);
        launch_gemm<EPI_RESIDUAL, D>(ao, q + B_PROJW, q + B_PROJB, x, x, M, D, st);
        dino_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x, q + B_LN2W, q + B_LN2B, ln, M);
        launch_gemm<EPI_GELU, D>(ln, q + B_FC1W, q + B_FC1B, hid, nullptr, M, HID, st);
        launch_gemm<EPI_RESIDUAL, HID>(hid, q + B_FC2W, q + B_FC2B, x, x, M, D, st);
    }
    if (feat || cls || attn)
        dino_full_outputs_kernel<<<blocks_for((long long)M * D), 256, 0, st>>>(x, sc0, ml0, batch, Tn, feat, cls, attn);
    if (pos) dino_copy_kernel<dino32_path><<<blocks_for((long long)Tn * D), 256, 0, st>>>(table, pos, (long long)Tn * D);
    return nsos_launch_status();
}

extern "C" size_t nsos_dino_find_fg_workspace_bytes(void) { return FG_WS_BYTES; }

extern "C" int32_t nsos_dino_find_fg(const int32_t* labels, const float* attn, int32_t h, int32_t w, int32_t* out_labels, float* attn_up,
                                     double* means, int32_t* flipped, void* workspace, size_t workspace_bytes, void* stream) {
    NSOS_REQUIRE(labels && attn && out_labels && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(h >= PS && w >= PS, NSOS_ERR_BAD_SHAPE);
    const long long rows = h / PS, cols = w / PS;
    NSOS_REQUIRE(rows <= FULL_MAX_NP && cols <= FULL_MAX_NP && rows * cols <= FULL_MAX_NP, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)attn & 3) == 0 && ((uintptr_t)out_labels & 3) == 0 &&
                     ((uintptr_t)attn_up & 3) == 0 && ((uintptr_t)means & 7) == 0 && ((uintptr_t)flipped & 3) == 0 &&
                     ((uintptr_t)workspace & 15) == 0,
                 NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(workspace_bytes >= FG_WS_BYTES, NSOS_ERR_BUFFER_TOO_SMALL);
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    int32_t* flag = (int32_t*)(part + (size_t)FG_BLOCKS * 4);
    const long long n = (long long)h * w;
    dino_fg_partial_kernel<<<FG_BLOCKS, 256, 0, st>>>(labels, attn, h, w, attn_up, part);
    dino_fg_finish_kernel<<<1, 256, 0, st>>>(part, flag, means, flipped);
    dino_fg_apply_kernel<<<blocks_for(n), 256, 0, st>>>(labels, flag, n, out_labels);
    return nsos_launch_status();
}
