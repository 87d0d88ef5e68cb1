// DINO ViT-S/16 feature extractor: the gradient of feat / cls with respect to the input image, fp32 (include/nerf_sos_hip.h "DINO
// ViT-S/16, backward to the input").  The weights are frozen: input gradients only.
//
// What is kept and what is recomputed.  nsos_dino_forward_save keeps the input of every block, saved [12][B][197][384] (3.63 MB per
// image).  The backward walks the blocks 11..0; for each it first re-runs the block's forward from its saved input with the forward's
// own kernels (dino32::recompute_block in dino_vit.hip: LN1, qkv, attention, proj + residual, LN2, fc1 without GELU), which leaves
// qkv, the residual midpoint and the MLP's pre-activation in the workspace (4.25 MB per image), then
//   dh   = (g . Wfc2) * GELU'(pre)         dino_bwd_gemm_kernel<GELU_GRAD>   [M,1536]   (exact erf form; in place over `pre`)
//   g   += LN2'(dh . Wfc1; xmid)           dino_bwd_gemm_kernel<STORE>, dino_bwd_layernorm_kernel (adds into the residual gradient)
//   dao  = g . Wproj                       dino_bwd_gemm_kernel<STORE>
//   dqkv = attention'(qkv, dao)            dino_bwd_attn_dq_kernel, dino_bwd_attn_dkv_kernel (probabilities recomputed, never stored)
//   g   += LN1'(dqkv . Wqkv; x_in)         dino_bwd_gemm_kernel<STORE>, dino_bwd_layernorm_kernel
// and after block 0 the patch embedding (dino_bwd_gemm_kernel<TOKENS>: the 16x16 patches do not overlap, so im2col's transpose is
// a permutation) and the two nearest resizes as one gather (dino_bwd_input_kernel).
//
// Data-gradient GEMMs: dA[M,K] = dOut[M,N] . W[N,K] on the forward's tile (gemm32_tile.h, v_mfma_f32_32x32x2_f32); nn.Linear's own
// [out,in] matrix is the [K'][N'] row-major operand the tile wants, so the backward has a packed stream of its own that holds the five
// kinds of matrices as the state dict has them, and 1536 zeros that serve as the tile's bias.
//
// Summation orders (fixed; no atomics; two calls give the same bits, and an image's bits do not depend on its batch -- every
// workgroup of the attention and input kernels reads one image, every GEMM / LayerNorm output row depends on its own row only):
//   GEMM           one fp32 fma chain per output element over the out-features 0..N-1 ascending, from 0
//   LayerNorm'     the row sums (mean, variance, sum dxhat, sum dxhat*xhat): six strided elements per lane ascending, then the xor
//                  butterfly 32,16,8,4,2,1
//   attention'     s = q.k over d ascending, * 1/8, p = exp(s - m) / l with the forward's row maximum m and sum l (bit-equal to the
//                  forward's probabilities); dP = dO.v over d ascending; delta = rowsum(dP * P): four strided columns per lane
//                  ascending, then the butterfly; dS = P * (dP - delta); dQ = (dS.K) / 8 over the keys 0..196 ascending;
//                  dV = P^T.dO and dK = (dS^T.Q) / 8 over the QUERIES 0..196 ascending inside one workgroup per 32 keys
//                  (the second, fixed-order pass; it reads m, l, delta of every query row from the first)
//   input          a source pixel sums the token gradients of its preimage under dino_source_index (an interval per axis, the
//                  map is monotone) in ascending (y, x) order, then / sd_c (twice with NSOS_DINO_STEP1); empty preimage: 0.0
#include "common.h"
#include "mlp_common.h"
#include "dino_common.h"
#include "gemm32_tile.h"
#include "dino_layout32.h"

namespace {

using namespace nsos::dino;
using namespace nsos::dino32;
using nsos::gemm32::GK;
using nsos::gemm32::GM;
using nsos::gemm32::GN;

struct dino32b_path {};   // this file's copies of the element-wise kernels of dino_common.h

// ---- packed stream of the backward (floats): the tile's zero bias, then every matrix as the state dict has it ([out][in]) --------
constexpr size_t Q_ZERO = 0;                                  // [1536] zeros
constexpr size_t Q_EMB_W = Q_ZERO + HID;                      // [384][768]   patch_embed.proj.weight
constexpr size_t Q_BLOCKS = Q_EMB_W + (size_t)D * KE;
constexpr size_t C_QKVW = 0, C_PROJW = C_QKVW + (size_t)3 * D * D, C_FC1W = C_PROJW + (size_t)D * D, C_FC2W = C_FC1W + (size_t)HID * D,
                 C_SIZE = C_FC2W + (size_t)D * HID;
constexpr size_t Q_SIZE = Q_BLOCKS + (size_t)NSOS_DINO_DEPTH * C_SIZE;
static_assert(Q_EMB_W % 4 == 0 && Q_BLOCKS % 4 == 0 && C_SIZE % 4 == 0 && C_PROJW % 4 == 0 && C_FC1W % 4 == 0 && C_FC2W % 4 == 0, "float4 rows");

// ---- workspace (floats per image): 4.25 MB -------------------------------------------------------------------------------------------
constexpr size_t V_STATN = ((size_t)3 * HEADS * T + 3) & ~(size_t)3;   // per head: m[197], l[197], delta[197]
constexpr size_t V_XM = 0, V_LN = V_XM + (size_t)T * D, V_QKV = V_LN + (size_t)T * D, V_AO = V_QKV + (size_t)T * 3 * D,
                 V_HID = V_AO + (size_t)T * D, V_G = V_HID + (size_t)T * HID, V_DQKV = V_G + (size_t)T * D,
                 V_STAT = V_DQKV + (size_t)T * 3 * D, V_SIZE = V_STAT + V_STATN;
static_assert(V_SIZE % 4 == 0 && V_LN % 4 == 0 && V_QKV % 4 == 0 && V_HID % 4 == 0 && V_G % 4 == 0 && V_DQKV % 4 == 0 && V_STAT % 4 == 0,
              "16-byte aligned sections for every batch size");
static_assert((size_t)NP * KE <= (size_t)T * HID, "the token gradients share the MLP's hidden section");

// ---- the residual-stream gradient at the output of block 11: cls -> token 0, feat -> tokens 1..196; a NULL upstream gradient is zero
__global__ __launch_bounds__(256) void dino_bwd_init_kernel(const float* __restrict__ g_feat, const float* __restrict__ g_cls, int batch,
                                                            float* __restrict__ g) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)batch * T * D) return;
    const int c = (int)(e % D), t = (int)((e / D) % T), b = (int)(e / ((long long)T * D));
    float v = 0.0f;
    if (t == 0) {
        if (g_cls) v = g_cls[(size_t)b * D + c];
    } else if (g_feat) {
        v = g_feat[((size_t)b * NP + t - 1) * D + c];
    }
    g[e] = v;
}

// ---- data-gradient GEMM: out[M,N'] = epilogue(A[M,K'] . W[K'][N']), W = nn.Linear's [out,in] matrix (K' = out, N' = in) -----------
enum { BEPI_STORE = 0, BEPI_GELU_GRAD = 1, BEPI_TOKENS = 2 };

template <int EPI, int K>
__global__ __launch_bounds__(256) void dino_bwd_gemm_kernel(const float* __restrict__ A, const float* __restrict__ W, const float* __restrict__ zero,
                                                            float* out, const float* pre, int M, int N) {
    const int m0 = blockIdx.y * GM, n0 = blockIdx.x * GN;
    const int ar = nsos::gemm32::a_row(), ak = nsos::gemm32::a_k();
    int row0 = min(m0 + ar, M - 1), row1 = min(m0 + ar + 32, M - 1);   // rows past M repeat the last one; never stored
    if constexpr (EPI == BEPI_TOKENS) {   // output row b*196 + t reads the gradient of token row b*197 + 1 + t
        row0 = row0 / NP * T + 1 + row0 % NP;
        row1 = row1 / NP * T + 1 + row1 % NP;
    }
    float* out_col = out + nsos::gemm32::out_col(n0);
    const float* pre_col = EPI == BEPI_GELU_GRAD ? pre + nsos::gemm32::out_col(n0) : nullptr;
    nsos::gemm32::tile<nsos::gemm32::OneChain>(
        K, m0, n0, M, W, zero, N,
        [&](int k0, float4(&ra)[2]) {
            ra[0] = *reinterpret_cast<const float4*>(A + (size_t)row0 * K + k0 + ak);
            ra[1] = *reinterpret_cast<const float4*>(A + (size_t)row1 * K + k0 + ak);
        },
        [&](int row, int, float v) {
            if constexpr (EPI == BEPI_GELU_GRAD) {   // d/dh of h/2 (1 + erf(h / sqrt 2)) = (1 + erf(h / sqrt 2)) / 2 + h exp(-h^2 / 2) / sqrt(2 pi)
                const float h = pre_col[(size_t)row * N];
                v = v * (0.5f * (1.0f + erff(h * 0.70710678118654752440f)) + h * expf(-0.5f * h * h) * 0.39894228040143267794f);
            }
            out_col[(size_t)row * N] = v;
        });
}

template <int EPI, int K>
void launch_bwd_gemm(const float* A, const float* W, const float* zero, float* out, const float* pre, int M, int N, hipStream_t st) {
    static_assert(K % GK == 0, "GEMM tiles");
    dino_bwd_gemm_kernel<EPI, K><<<dim3(N / GN, (M + GM - 1) / GM), 256, 0, st>>>(A, W, zero, out, pre, M, N);
}
static_assert(D % GN == 0 && HID % GN == 0 && KE % GN == 0 && D % GK == 0 && (3 * D) % GK == 0 && HID % GK == 0, "GEMM tiles");

// ---- LayerNorm backward (input gradient; biased variance, eps 1e-6), one wave per row: g[row] += dx -----------------------------------
//   xhat = (x - mean) * rstd, dxhat = dy * w, dx = rstd * (dxhat - mean(dxhat) - xhat * mean(dxhat * xhat))
__global__ __launch_bounds__(256) void dino_bwd_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                 const float* __restrict__ dy, float* __restrict__ g, int M) {
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
    float d[6], s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        d[j] = dy[(size_t)row * D + lane + 64 * j] * w[lane + 64 * j];
        v[j] *= rstd;
        s1 += d[j];
        s2 += d[j] * v[j];
    }
    const float m1 = dino_wave_sum(s1) / (float)D, m2 = dino_wave_sum(s2) / (float)D;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float* gp = g + (size_t)row * D + lane + 64 * j;
        *gp = *gp + rstd * (d[j] - m1 - v[j] * m2);
    }
}

// ---- attention backward: one workgroup per (32 rows, head, image) on v_mfma_f32_16x16x4_f32 -----------------------------------------
// Two operand images, as in the forward: LDR = 66 for a matrix read with its row on the lane (k along the row: q.k^T-like products),
// LDC = 80 for one read with its column on the lane (k down the rows, zero rows 197..199: p.v-like products).
constexpr int RT = 32, LDR = 66, LDC = 80, TP = 200, LDP = 226;
constexpr int BIG_FLOATS = TP * LDC;
static_assert(BIG_FLOATS >= T * LDR && (RT * LDR) % 4 == 0 && BIG_FLOATS % 4 == 0 && (RT * LDP) % 4 == 0, "LDS sections");
constexpr int ATTB_LDS_BYTES = (2 * RT * LDR + BIG_FLOATS + 2 * RT * LDP) * 4;
static_assert(ATTB_LDS_BYTES <= 160 * 1024, "one CU's LDS");

// rows r0 .. r0+31 of a [197][64] matrix (row stride `stride`), rows past 196 repeat row 196 (their results are never stored)
__device__ __forceinline__ void attb_load_tile(const float* __restrict__ src, int stride, int r0, float* dst) {
    for (int i = threadIdx.x; i < RT * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)min(r0 + r, T - 1) * stride + c);
        float* d = dst + r * LDR + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}
// all 197 rows at stride LDR
__device__ __forceinline__ void attb_load_rows(const float* __restrict__ src, int stride, float* dst) {
    for (int i = threadIdx.x; i < T * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * stride + c);
        float* d = dst + r * LDR + c;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
}
// all 197 rows at stride LDC, rows 197..199 zero
__device__ __forceinline__ void attb_load_cols(const float* __restrict__ src, int stride, float* dst) {
    for (int i = threadIdx.x; i < TP * (HD / 4); i += 256) {
        const int r = i >> 4, c = (i & 15) * 4;
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < T) v = *reinterpret_cast<const float4*>(src + (size_t)r * stride + c);
        *reinterpret_cast<float4*>(dst + r * LDC + c) = v;
    }
}
// out[32][LDP] (columns 0..207) = scale * tile[32][64] . rows[197][64]^T, d ascending; columns past 196 repeat row 196 (masked by the caller)
__device__ __forceinline__ void attb_row_product(const float* tile, const float* rows, float* out, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    for (int tj = wave; tj < 13; tj += 4) {
        f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
        const float* qa = tile + li * LDR + lk;
        const float* kb = rows + min(tj * 16 + li, T - 1) * LDR + lk;
#pragma unroll
        for (int k0 = 0; k0 < HD; k0 += 4) {
            const float bb = kb[k0];
            s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[k0], bb, s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[16 * LDR + k0], bb, s1, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // C/D: col = lane & 15, row = 4 * (lane >> 4) + r
            out[(lk * 4 + r) * LDP + tj * 16 + li] = s0[r] * scale;
            out[(16 + lk * 4 + r) * LDP + tj * 16 + li] = s1[r] * scale;
        }
    }
}
// dst[r0 + i][16 wave + ..] = scale * sum over k = 0..199 ascending of mat[i][k] * cols[k][..], rows r0 + i < 197 stored (row stride 3*384)
__device__ __forceinline__ void attb_col_product(const float* mat, const float* cols, float* __restrict__ dst, int r0, float scale) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
    f32x4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0;
    const float* pa = mat + li * LDP + lk;
    const float* vb = cols + lk * LDC + wave * 16 + li;
#pragma unroll 10
    for (int k0 = 0; k0 < TP; k0 += 4) {
        const float bb = vb[k0 * LDC];
        o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[k0], bb, o0, 0, 0, 0);
        o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[16 * LDP + k0], bb, o1, 0, 0, 0);
    }
    float* d = dst + wave * 16 + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ra = r0 + lk * 4 + r, rb = ra + 16;
        if (ra < T) d[(size_t)ra * 3 * D] = o0[r] * scale;
        if (rb < T) d[(size_t)rb * 3 * D] = o1[r] * scale;
    }
}

// first pass, 32 QUERY rows: P (the forward's arithmetic), dP = dO.V^T, delta, dS, dQ = dS.K / 8; leaves m, l, delta of its rows in `stat`
__global__ __launch_bounds__(256) void dino_bwd_attn_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dao,
                                                               float* __restrict__ dqkv, float* __restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Qs = lds;                    // [32][LDR]
    float* Os = Qs + RT * LDR;          // dO rows [32][LDR]
    float* Big = Os + RT * LDR;         // K rows, then V rows, then K columns
    float* Ps = Big + BIG_FLOATS;       // scores, P, then dS [32][LDP]
    float* Ds = Ps + RT * LDP;          // dP [32][LDP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * RT, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * 3 * D + h * HD;
    const float* dob = dao + (size_t)b * T * D + h * HD;
    float* st = stat + (size_t)b * V_STATN + (size_t)h * 3 * T;
    attb_load_tile(base, 3 * D, q0, Qs);
    attb_load_tile(dob, D, q0, Os);
    attb_load_rows(base + D, 3 * D, Big);
    __syncthreads();
    attb_row_product(Qs, Big, Ps, 0.125f);   // scale = 64^-0.5, as the forward
    __syncthreads();                         // K is dead: V takes its place
    attb_load_rows(base + 2 * D, 3 * D, Big);
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {   // the forward's softmax: wave w owns rows 8w..8w+7, a lane the columns lane + 64 j
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
        if (lane == 0 && q0 + r < T) st[q0 + r] = m, st[T + q0 + r] = s;
    }
    __syncthreads();
    attb_row_product(Os, Big, Ds, 1.0f);   // dP[i][j] = dO_i . v_j
    __syncthreads();                       // V is dead: K again, column image
    attb_load_cols(base + D, 3 * D, Big);
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        float* pr = Ps + r * LDP;
        const float* dr = Ds + r * LDP;
        float p[4], dp[4], s = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            p[j] = c < T ? pr[c] : 0.0f;
            dp[j] = c < T ? dr[c] : 0.0f;
            s += dp[j] * p[j];
        }
        const float delta = dino_wave_sum(s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c < TP) pr[c] = p[j] * (dp[j] - delta);   // columns 197..199: p = 0
        }
        if (lane == 0 && q0 + r < T) st[2 * T + q0 + r] = delta;
    }
    __syncthreads();
    attb_col_product(Ps, Big, dqkv + (size_t)b * T * 3 * D + h * HD, q0, 0.125f);
}

// second pass, 32 KEY rows against every query: P^T and dS^T from the first pass's m, l, delta; dV = P^T.dO, dK = dS^T.Q / 8
__global__ __launch_bounds__(256) void dino_bwd_attn_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dao,
                                                                float* __restrict__ dqkv, const float* __restrict__ stat) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Ks = lds;                    // [32][LDR]
    float* Vs = Ks + RT * LDR;          // [32][LDR]
    float* Big = Vs + RT * LDR;         // Q rows, dO rows, dO columns, Q columns
    float* Ps = Big + BIG_FLOATS;       // scores^T, then P^T [32 keys][LDP queries]
    float* Ds = Ps + RT * LDP;          // dP^T, then dS^T
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = blockIdx.x * RT, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * 3 * D + h * HD;
    const float* dob = dao + (size_t)b * T * D + h * HD;
    const float* st = stat + (size_t)b * V_STATN + (size_t)h * 3 * T;
    float* out = dqkv + (size_t)b * T * 3 * D + h * HD;
    attb_load_tile(base + D, 3 * D, j0, Ks);
    attb_load_tile(base + 2 * D, 3 * D, j0, Vs);
    attb_load_rows(base, 3 * D, Big);
    __syncthreads();
    attb_row_product(Ks, Big, Ps, 0.125f);   // k_j . q_i: the same products in the same order as q_i . k_j
    __syncthreads();
    attb_load_rows(dob, D, Big);
    float m[4], l[4], delta[4];   // of the query columns lane + 64 j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = min(lane + 64 * j, T - 1);
        m[j] = st[c], l[j] = st[T + c], delta[j] = st[2 * T + c];
    }
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        float* pr = Ps + r * LDP;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c < TP) pr[c] = c < T ? expf(pr[c] - m[j]) / l[j] : 0.0f;
        }
    }
    __syncthreads();
    attb_row_product(Vs, Big, Ds, 1.0f);   // dP^T[j][i] = v_j . dO_i
    __syncthreads();
    attb_load_cols(dob, D, Big);
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        const float* pr = Ps + r * LDP;
        float* dr = Ds + r * LDP;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            if (c < TP) dr[c] = c < T ? pr[c] * (dr[c] - delta[j]) : 0.0f;
        }
    }
    __syncthreads();
    attb_col_product(Ps, Big, out + 2 * D, j0, 1.0f);      // dV
    __syncthreads();                                       // dO is dead: Q, column image
    attb_load_cols(base, 3 * D, Big);
    __syncthreads();
    attb_col_product(Ds, Big, out + D, j0, 0.125f);        // dK
}

// ---- the input: the gather that transposes im2col and the two nearest resizes ------------------------------------------------------
// the first of the 224 destinations whose source index is >= target (224: none); dino_source_index is monotone in the destination
__device__ __forceinline__ int dino_bwd_first_dst(int target, int in, int stride) {
    int lo = 0, hi = IMG;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (dino_source_index(mid, in, stride) >= target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// one thread per input element of image blockIdx.y; dtok [B*196][768] is the gradient of the im2col tokens
__global__ __launch_bounds__(256) void dino_bwd_input_kernel(const float* __restrict__ dtok, int in_h, int in_w, int stride, int flags,
                                                             float* __restrict__ g_in) {
    const long long per = 3LL * in_h * in_w;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    const int b = blockIdx.y;
    int c, sy, sx;
    if (flags & NSOS_DINO_NHWC) {
        c = (int)(e % 3), sx = (int)((e / 3) % in_w), sy = (int)(e / (3LL * in_w));
    } else {
        sx = (int)(e % in_w), sy = (int)((e / in_w) % in_h), c = (int)(e / ((long long)in_w * in_h));
    }
    int y0 = sy, y1 = sy + 1, x0 = sx, x1 = sx + 1;   // NSOS_DINO_PREPARED: the identity
    if (!(flags & NSOS_DINO_PREPARED)) {
        const int s1 = (flags & NSOS_DINO_STEP1) ? stride : 0;
        y0 = dino_bwd_first_dst(sy, in_h, s1), y1 = dino_bwd_first_dst(sy + 1, in_h, s1);
        x0 = dino_bwd_first_dst(sx, in_w, s1), x1 = dino_bwd_first_dst(sx + 1, in_w, s1);
    }
    const float* tb = dtok + (size_t)b * NP * KE + c * (PS * PS);
    float s = 0.0f;
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) s += tb[(size_t)((y >> 4) * GRID + (x >> 4)) * KE + (y & 15) * PS + (x & 15)];
    if (!(flags & NSOS_DINO_PREPARED)) {
        const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        s = s / sd;                                  // models/extractor.py:205-208
        if (flags & NSOS_DINO_STEP1) s = s / sd;     // engines/trainer.py:24-29 normalize_batch
    }
    g_in[(size_t)b * per + e] = s;
}

__global__ __launch_bounds__(256) void dino_bwd_zero_kernel(float* __restrict__ dst, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = 0.0f;
}

// the two attention kernels' 136 KB of dynamic LDS need the attribute once per device (nsos_dino_pack_backward sets it too)
int32_t dino_bwd_configure() {
    static NsosPerDeviceFlag configured;
    if (!configured.here()) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dino_bwd_attn_dq_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           ATTB_LDS_BYTES);
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dino_bwd_attn_dkv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    ATTB_LDS_BYTES);
        if (e != hipSuccess) return (int32_t)e;
        configured.here() = true;
    }
    return nsos::dino32::configure();   // the recomputed forward's attention kernel
}

}  // namespace

extern "C" size_t nsos_dino_saved_bytes(int32_t batch) {
    return (batch >= 1 && batch <= NSOS_DINO_MAX_BATCH) ? (size_t)NSOS_DINO_DEPTH * batch * T * D * sizeof(float) : 0;
}

extern "C" size_t nsos_dino_backward_packed_bytes(void) { return Q_SIZE * sizeof(float); }

extern "C" size_t nsos_dino_backward_workspace_bytes(int32_t batch) {
    return (batch >= 1 && batch <= NSOS_DINO_MAX_BATCH) ? (size_t)batch * V_SIZE * sizeof(float) : 0;
}

extern "C" int32_t nsos_dino_pack_backward(const nsos_dino_tensors* t, void* packed, size_t packed_bytes, void* stream) {
    NSOS_REQUIRE(packed, NSOS_ERR_NULL_POINTER);
    if (int32_t c = dino_check_tensors(t)) return c;
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(packed_bytes >= Q_SIZE * sizeof(float), NSOS_ERR_BUFFER_TOO_SMALL);
    if (int32_t c = dino_bwd_configure()) return c;
    hipStream_t st = (hipStream_t)stream;
    float* p = (float*)packed;
    auto copy = [&](const float* src, float* dst, long long n) {
        dino_copy_kernel<dino32b_path><<<blocks_for(n), 256, 0, st>>>(src, dst, n);
    };
    dino_bwd_zero_kernel<<<blocks_for(HID), 256, 0, st>>>(p + Q_ZERO, HID);
    copy(t->patch_w, p + Q_EMB_W, (long long)D * KE);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const nsos_dino_block_tensors& b = t->blocks[i];
        float* q = p + Q_BLOCKS + (size_t)i * C_SIZE;
        copy(b.qkv_w, q + C_QKVW, (long long)3 * D * D);
        copy(b.proj_w, q + C_PROJW, (long long)D * D);
        copy(b.fc1_w, q + C_FC1W, (long long)HID * D);
        copy(b.fc2_w, q + C_FC2W, (long long)D * HID);
    }
    return nsos_launch_status();
}

extern "C" int32_t nsos_dino_backward(int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags, const void* packed,
                                      const void* packed_bwd, const float* saved, const float* g_feat, const float* g_cls, void* workspace,
                                      size_t workspace_bytes, float* g_input, float* g_blocks, void* stream) {
    const bool others = packed_bwd && saved && (g_feat || g_cls);
    const bool others_aligned = ((uintptr_t)packed_bwd & 15) == 0 && ((uintptr_t)saved & 15) == 0 && ((uintptr_t)g_feat & 3) == 0 &&
                                ((uintptr_t)g_cls & 3) == 0 && ((uintptr_t)g_blocks & 3) == 0;
    if (int32_t c = dino_check_forward(g_input, batch, in_h, in_w, patch_stride, flags, packed, workspace, workspace_bytes,
                                       nsos_dino_backward_workspace_bytes, true, others, others_aligned))
        return c;
    if (int32_t c = dino_bwd_configure()) return c;
    hipStream_t st = (hipStream_t)stream;
    const float* p = (const float*)packed;
    const float* pb = (const float*)packed_bwd;
    const float* zero = pb + Q_ZERO;
    float* ws = (float*)workspace;
    const size_t Bn = (size_t)batch;
    float *xm = ws + Bn * V_XM, *ln = ws + Bn * V_LN, *qkv = ws + Bn * V_QKV, *ao = ws + Bn * V_AO, *hid = ws + Bn * V_HID, *g = ws + Bn * V_G,
          *dqkv = ws + Bn * V_DQKV, *stat = ws + Bn * V_STAT, *dtok = hid;
    const int M = batch * T;
    const long long MD = (long long)M * D;
    const dim3 att((T + RT - 1) / RT, HEADS, batch);

    dino_bwd_init_kernel<<<blocks_for(MD), 256, 0, st>>>(g_feat, g_cls, batch, g);
    for (int i = NSOS_DINO_DEPTH - 1; i >= 0; --i) {
        const float* q = p + P_BLOCKS + (size_t)i * B_SIZE;
        const float* w = pb + Q_BLOCKS + (size_t)i * C_SIZE;
        const float* x_in = saved + (size_t)i * M * D;
        nsos::dino32::recompute_block(q, x_in, xm, ln, qkv, ao, hid, batch, st);
        launch_bwd_gemm<BEPI_GELU_GRAD, D>(g, w + C_FC2W, zero, hid, hid, M, HID, st);      // dh, in place over the pre-activation
        launch_bwd_gemm<BEPI_STORE, HID>(hid, w + C_FC1W, zero, ao, nullptr, M, D, st);     // d LN2 output
        dino_bwd_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(xm, q + B_LN2W, ao, g, M);   // g: the gradient of the residual midpoint
        launch_bwd_gemm<BEPI_STORE, D>(g, w + C_PROJW, zero, ln, nullptr, M, D, st);        // d attention output
        dino_bwd_attn_dq_kernel<<<att, 256, ATTB_LDS_BYTES, st>>>(qkv, ln, dqkv, stat);
        dino_bwd_attn_dkv_kernel<<<att, 256, ATTB_LDS_BYTES, st>>>(qkv, ln, dqkv, stat);
        launch_bwd_gemm<BEPI_STORE, 3 * D>(dqkv, w + C_QKVW, zero, ao, nullptr, M, D, st);  // d LN1 output
        dino_bwd_layernorm_kernel<<<(M + 3) / 4, 256, 0, st>>>(x_in, q + B_LN1W, ao, g, M); // g: the gradient of the block's input
        if (g_blocks) dino_copy_kernel<dino32b_path><<<blocks_for(MD), 256, 0, st>>>(g, g_blocks + (size_t)i * M * D, MD);
    }
    launch_bwd_gemm<BEPI_TOKENS, D>(g, pb + Q_EMB_W, zero, dtok, nullptr, batch * NP, KE, st);
    dino_bwd_input_kernel<<<dim3(blocks_for(3LL * in_h * in_w), batch), 256, 0, st>>>(dtok, in_h, in_w, patch_stride, flags, g_input);
    return nsos_launch_status();
}
