// DINO ViT-S/16 feature extractor with 16-bit matrix operands (fp16 or bf16) and fp32 accumulation: nsos_dino_pack16 /
// nsos_dino_forward16 (include/nerf_sos_hip.h "DINO ViT-S/16, 16-bit operands").  The 224 x 224 path of
// dino_vit.hip with the same kernel split and launch sequence:
//   dino16_prepare_kernel    the same prepared pixel (dino_common.h), im2col tokens written in 16 bits
//   dino16_gemm_kernel       C = A[M,K] . W[N,K]^T on v_mfma_f32_16x16x32_{f16,bf16}; epilogue bias / GELU / residual / embedding in fp32
//   dino16_layernorm_kernel  fp32 statistics and affine, output rounded once to 16 bits
//   dino16_attention_kernel  one workgroup per (32 query rows, head, image); fp32 softmax, probabilities rounded after the division
// The rounding contract: the two operands of every matrix product (patch embedding, qkv, q.k^T, p.v, proj, fc1, fc2) are 16-bit,
// rounded ONCE, to nearest even, by the kernel that produces them (weights at pack time); everything else -- the residual stream x,
// LayerNorm, softmax (row max, expf, row sum, division), bias, GELU (erf), the residual add, the three outputs -- is fp32.
// fp16 and bf16 are two instantiations of the same templates (nsos::lp::F16 / BF16, as mlp_lp16_kernel).
// Every sum runs in a fixed order; no atomics; each output element depends on one image only.
#include "common.h"
#include "lp_common.h"
#include "dino_common.h"

namespace {

using namespace nsos::dino;
using nsos::lp::BF16;
using nsos::lp::F16;
using nsos::lp::u32x2;
using nsos::lp::u32x4;
typedef unsigned short h16;   // the bits of one 16-bit operand

// ---- packed stream: an fp32 section (what the epilogues and LayerNorm read), then every matrix in 16 bits --------------------------
// Matrices keep nn.Linear's [out][in] layout: an MFMA B operand is eight consecutive k of one output column, i.e. 16 contiguous bytes.
constexpr size_t F_POS = 0;                                  // [197][384], row 0 = cls_token + pos_embed[0]
constexpr size_t F_EMB_B = F_POS + (size_t)T * D;
constexpr size_t F_BLOCKS = F_EMB_B + D;
constexpr size_t FB_LN1W = 0, FB_LN1B = FB_LN1W + D, FB_QKVB = FB_LN1B + D, FB_PROJB = FB_QKVB + 3 * D, FB_LN2W = FB_PROJB + D,
                 FB_LN2B = FB_LN2W + D, FB_FC1B = FB_LN2B + D, FB_FC2B = FB_FC1B + HID, FB_SIZE = FB_FC2B + D;
constexpr size_t F_SIZE = F_BLOCKS + (size_t)NSOS_DINO_DEPTH * FB_SIZE;          // floats
constexpr size_t H_EMB_W = 0;                                                     // [384][768]
constexpr size_t H_BLOCKS = H_EMB_W + (size_t)D * KE;
constexpr size_t HB_QKVW = 0, HB_PROJW = HB_QKVW + (size_t)3 * D * D, HB_FC1W = HB_PROJW + (size_t)D * D, HB_FC2W = HB_FC1W + (size_t)HID * D,
                 HB_SIZE = HB_FC2W + (size_t)D * HID;
constexpr size_t H_SIZE = H_BLOCKS + (size_t)NSOS_DINO_DEPTH * HB_SIZE;          // 16-bit elements
constexpr size_t P16_BYTES = F_SIZE * 4 + H_SIZE * 2;
static_assert((F_SIZE * 4) % 16 == 0 && F_BLOCKS % 4 == 0 && FB_SIZE % 4 == 0 && H_BLOCKS % 8 == 0 && HB_SIZE % 8 == 0 && HB_PROJW % 8 == 0 &&
                  HB_FC1W % 8 == 0 && HB_FC2W % 8 == 0,
              "16-byte rows");

// ---- workspace (bytes per image; section s of a batch B starts at B * W16_s) -----------------------------------------------------
constexpr size_t W16_X = 0,                                        // fp32 residual stream [197][384]
    W16_LN = W16_X + (size_t)T * D * 4,                            // 16-bit from here: LayerNorm output
    W16_QKV = W16_LN + (size_t)T * D * 2, W16_AO = W16_QKV + (size_t)T * 3 * D * 2, W16_HID = W16_AO + (size_t)T * D * 2,
    W16_TOK = W16_HID + (size_t)T * HID * 2,                       // im2col tokens [196][768]
    W16_ROW0 = W16_TOK + (size_t)NP * KE * 2,                      // fp32 [6][196]: block 11's softmax row 0
    W16_SIZE = W16_ROW0 + (size_t)HEADS * NP * 4;
static_assert(W16_LN % 16 == 0 && W16_QKV % 16 == 0 && W16_AO % 16 == 0 && W16_HID % 16 == 0 && W16_TOK % 16 == 0 && W16_ROW0 % 16 == 0 &&
                  W16_SIZE % 16 == 0,
              "16-byte aligned sections for every batch size");

// ---- prepare: two neighbouring pixels per thread, tokens[b*196 + t][c*256 + py*16 + px] in 16 bits; also x[b][0][:] = cls + pos[0] ----
template <class P>
__global__ __launch_bounds__(256) void dino16_prepare_kernel(const float* __restrict__ in, int batch, int in_h, int in_w, int stride, int flags,
                                                             const float* __restrict__ clspos, unsigned* __restrict__ tokens,
                                                             float* __restrict__ x, float* __restrict__ prepared) {
    const long long n = (long long)batch * NP * (KE / 2);
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int k = 2 * (int)(e % (KE / 2));
    const int t = (int)((e / (KE / 2)) % NP);
    const int b = (int)(e / ((long long)(KE / 2) * NP));
    const int c = k >> 8, py = (k >> 4) & 15, px = k & 15;
    const int y = (t / GRID) * PS + py, xx = (t % GRID) * PS + px;
    const float v0 = dino_prepared_pixel(in, b, c, y, xx, in_h, in_w, stride, flags);
    const float v1 = dino_prepared_pixel(in, b, c, y, xx + 1, in_h, in_w, stride, flags);
    tokens[e] = P::pack2(v0, v1);
    if (prepared) {
        float* d = prepared + (((size_t)b * 3 + c) * IMG + y) * IMG + xx;
        d[0] = v0, d[1] = v1;
    }
    if (t == 0 && k < D) {
        float* d = x + (size_t)b * T * D + k;
        d[0] = clspos[k], d[1] = clspos[k + 1];
    }
}

// ---- GEMM: out[M,N] = epilogue(A[M,K] . W[N,K]^T), both operands 16-bit and k-contiguous, fp32 accumulators ---------------------
// BM x 64 outputs per workgroup (BM 64: four waves of 32x32; BM 32: four waves of 16x32, for the N = 384 products whose 64-row grid
// would leave 40 % of the CUs idle), K in steps of 64 through LDS with rows padded to 144 bytes (ds_read_b128 of 16 rows then covers
// all 64 banks), the next tile's global loads in flight under this tile's MFMAs.  v_mfma_f32_16x16x32 with the WEIGHT fragment as the
// A operand: the accumulator then holds C^T, i.e. a lane owns four consecutive output columns of one row -- one 16-byte (fp32) or
// 8-byte (16-bit) store, bias and residual as one float4 load.  Each output is one chain over k ascending in steps of 32.
enum { EPI16_BIAS = 0, EPI16_GELU = 1, EPI16_RESIDUAL = 2, EPI16_EMBED = 3 };
constexpr int BN = 64, BK = 64, LDT = BK + 8;

template <class P, int EPI, int K, int BM>
__global__ __launch_bounds__(256) void dino16_gemm_kernel(const h16* __restrict__ A, const h16* __restrict__ W, const float* __restrict__ bias,
                                                          void* out_, const float* extra, int M, int N, int np) {
    constexpr int FM = BM / 32;   // 16-row fragments per wave
    __shared__ __attribute__((aligned(16))) h16 As[BM * LDT];
    __shared__ __attribute__((aligned(16))) h16 Ws[BN * LDT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, li = lane & 15, lk = lane >> 4;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int lr = tid >> 3, lc = (tid & 7) * 8;   // a 16-byte piece per thread: 32 rows of 64 k per pass
    u32x4 ra[FM], rw[2];
    const h16* ap[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) ap[i] = A + (size_t)min(m0 + lr + 32 * i, M - 1) * K + lc;   // rows past M repeat the last one; never stored
    const h16* wp = W + (size_t)(n0 + lr) * K + lc;
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < FM; ++i) ra[i] = *reinterpret_cast<const u32x4*>(ap[i] + k0);
        rw[0] = *reinterpret_cast<const u32x4*>(wp + k0);
        rw[1] = *reinterpret_cast<const u32x4*>(wp + (size_t)32 * K + k0);
    };
    f32x4 acc[FM][2];
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[i][0] = acc[i][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    gload(0);
    const h16* a_rd = As + (wm * 16 * FM + li) * LDT + lk * 8;
    const h16* w_rd = Ws + (wn * 32 + li) * LDT + lk * 8;
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();   // the previous tile has been consumed
#pragma unroll
        for (int i = 0; i < FM; ++i) *reinterpret_cast<u32x4*>(As + (lr + 32 * i) * LDT + lc) = ra[i];
        *reinterpret_cast<u32x4*>(Ws + lr * LDT + lc) = rw[0];
        *reinterpret_cast<u32x4*>(Ws + (lr + 32) * LDT + lc) = rw[1];
        __syncthreads();
        if (k0 + BK < K) gload(k0 + BK);   // in flight under this tile's MFMAs
#pragma unroll
        for (int kk = 0; kk < BK; kk += 32) {
            u32x4 fa[FM], fw[2];
#pragma unroll
            for (int i = 0; i < FM; ++i) fa[i] = *reinterpret_cast<const u32x4*>(a_rd + i * 16 * LDT + kk);
#pragma unroll
            for (int j = 0; j < 2; ++j) fw[j] = *reinterpret_cast<const u32x4*>(w_rd + j * 16 * LDT + kk);
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = P::mfma_k32(fw[j], fa[i], acc[i][j]);   // C^T: row = output column, col = output row
        }
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        const int row = m0 + wm * 16 * FM + i * 16 + li;
        if (row >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 32 + j * 16 + 4 * lk;   // columns col .. col + 3
            const float4 bv = *reinterpret_cast<const float4*>(bias + col);
            float v[4] = {acc[i][j][0] + bv.x, acc[i][j][1] + bv.y, acc[i][j][2] + bv.z, acc[i][j][3] + bv.w};
            if constexpr (EPI == EPI16_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] * 0.5f * (1.0f + erff(v[r] * 0.70710678118654752440f));
            }
            if constexpr (EPI == EPI16_BIAS || EPI == EPI16_GELU) {   // the only consumer is a matrix product: 16 bits, rounded here
                *reinterpret_cast<u32x2*>((h16*)out_ + (size_t)row * N + col) = u32x2{P::pack2(v[0], v[1]), P::pack2(v[2], v[3])};
            } else if constexpr (EPI == EPI16_RESIDUAL) {
                const float4 xv = *reinterpret_cast<const float4*>(extra + (size_t)row * N + col);
                *reinterpret_cast<float4*>((float*)out_ + (size_t)row * N + col) = make_float4(xv.x + v[0], xv.y + v[1], xv.z + v[2], xv.w + v[3]);
            } else {   // row = b*np + t -> token row b*(np+1) + 1 + t; + pos_embed[1 + t]
                const int b = row / np, t = row - b * np;
                const float4 pv = *reinterpret_cast<const float4*>(extra + (size_t)(1 + t) * N + col);
                *reinterpret_cast<float4*>((float*)out_ + ((size_t)b * (np + 1) + 1 + t) * N + col) =
                    make_float4(v[0] + pv.x, v[1] + pv.y, v[2] + pv.z, v[3] + pv.w);
            }
        }
    }
}

// ---- LayerNorm over 384, eps 1e-6, fp32 (biased variance about the mean); one wave per row, a lane three pairs of neighbours ------
template <class P>
__global__ __launch_bounds__(256) void dino16_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                               unsigned* __restrict__ y, int M) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (size_t)row * D;
    float v[6], s = 0.0f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float2 t = *reinterpret_cast<const float2*>(xr + 2 * lane + 128 * j);
        v[2 * j] = t.x, v[2 * j + 1] = t.y, s += t.x, s += t.y;
    }
    const float mean = dino_wave_sum(s) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < 6; ++j) v[j] -= mean, q += v[j] * v[j];
    const float rstd = 1.0f / sqrtf(dino_wave_sum(q) / (float)D + 1e-6f);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = 2 * lane + 128 * j;
        y[((size_t)row * D + c) >> 1] = P::pack2(v[2 * j] * rstd * w[c] + b[c], v[2 * j + 1] * rstd * w[c + 1] + b[c + 1]);
    }
}

// ---- attention: softmax(q k^T / 8) v for 32 query rows of one head of one image -------------------------------------------------
// q and k fragments come straight from the 16-bit qkv rows (d is the contiguous index of both); V is transposed into LDS ([d][key],
// two keys per 32-bit write) because p.v sums over keys.  Scores (fp32) go to LDS, a wave owns 8 rows of the softmax: row max, expf,
// row sum, one division per element, all fp32 -- block 11's row 0 is stored from these fp32 probabilities -- and the probabilities,
// rounded once, overwrite the front of their own score row (every lane has read its scores before any lane writes).  Keys 197..223
// are zero probabilities on zero V columns.  p.v as V^T . P^T: a lane owns four consecutive d of one query, one 8-byte store.
constexpr int AQT = 32, ALDP = 212, AKP = 224, ALDV = 232;   // floats per score row; padded key count (7 x 32); 16-bit elements per V^T row
static_assert(ALDP * 2 >= AKP && ALDV >= AKP && (ALDP * 4) % 16 == 0 && (ALDV * 2) % 16 == 0 && ALDP >= 13 * 16, "attention LDS rows");

template <class P>
__global__ __launch_bounds__(256) void dino16_attention_kernel(const h16* __restrict__ qkv, h16* __restrict__ ao, float* __restrict__ row0) {
    __shared__ __attribute__((aligned(16))) float Ps[AQT * ALDP];
    __shared__ __attribute__((aligned(16))) h16 Vt[HD * ALDV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int q0 = blockIdx.x * AQT, h = blockIdx.y, b = blockIdx.z;
    const h16* base = qkv + (size_t)b * T * 3 * D + h * HD;
    for (int i = tid; i < (ALDV / 2) * (HD / 8); i += 256) {   // consecutive lanes: consecutive key pairs = consecutive LDS words
        const int key = 2 * (i % (ALDV / 2)), dc = (i / (ALDV / 2)) * 8;
        u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = v0;
        if (key < T) v0 = *reinterpret_cast<const u32x4*>(base + (size_t)key * 3 * D + 2 * D + dc);
        if (key + 1 < T) v1 = *reinterpret_cast<const u32x4*>(base + (size_t)(key + 1) * 3 * D + 2 * D + dc);
        unsigned* dst = reinterpret_cast<unsigned*>(Vt + dc * ALDV + key);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dst[(2 * j) * (ALDV / 2)] = (v0[j] & 0xffffu) | (v1[j] << 16);
            dst[(2 * j + 1) * (ALDV / 2)] = (v0[j] >> 16) | (v1[j] & 0xffff0000u);
        }
    }
    {   // scores: 13 column tiles of 16 keys (the last: keys 192..207, clamped to 196 and masked below), both 16-row halves per wave
        u32x4 qa[2][2];   // query rows past 196 repeat row 196; their results are never stored
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const h16* qr = base + (size_t)min(q0 + 16 * hh + li, T - 1) * 3 * D + 8 * lk;
            qa[hh][0] = *reinterpret_cast<const u32x4*>(qr), qa[hh][1] = *reinterpret_cast<const u32x4*>(qr + 32);
        }
        for (int tj = wave; tj < 13; tj += 4) {
            const h16* kr = base + (size_t)min(tj * 16 + li, T - 1) * 3 * D + D + 8 * lk;
            const u32x4 kb0 = *reinterpret_cast<const u32x4*>(kr), kb1 = *reinterpret_cast<const u32x4*>(kr + 32);
            f32x4 s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = s0;
            s0 = P::mfma_k32(qa[0][0], kb0, s0), s0 = P::mfma_k32(qa[0][1], kb1, s0);   // d ascending
            s1 = P::mfma_k32(qa[1][0], kb0, s1), s1 = P::mfma_k32(qa[1][1], kb1, s1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {   // C/D: col = lane & 15 (key), row = 4 * (lane >> 4) + r (query)
                Ps[(lk * 4 + r) * ALDP + tj * 16 + li] = s0[r] * 0.125f;   // scale = 64^-0.5
                Ps[(16 + lk * 4 + r) * ALDP + tj * 16 + li] = s1[r] * 0.125f;
            }
        }
    }
    __syncthreads();
    // softmax with the row maximum subtracted: wave w owns rows 8w..8w+7, a lane the columns lane, lane+64, lane+128, lane+192
    for (int r = wave * 8; r < wave * 8 + 8; ++r) {
        float* pr = Ps + r * ALDP;
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
        h16* p16 = reinterpret_cast<h16*>(pr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = lane + 64 * j;
            const float p = v[j] / s;
            if (row0 && q0 == 0 && r == 0 && c >= 1 && c < T) row0[((size_t)b * HEADS + h) * NP + c - 1] = p;   // block 11: fp32 probabilities
            if (c < AKP) p16[c] = P::bits(p);
        }
    }
    __syncthreads();
    {   // out^T = V^T . P^T: wave w owns d = 16w..16w+15, both query halves; keys ascending in steps of 32
        f32x4 o0 = {0.0f, 0.0f, 0.0f, 0.0f}, o1 = o0;
        const h16* va = Vt + (wave * 16 + li) * ALDV + 8 * lk;
        const h16* pb0 = reinterpret_cast<const h16*>(Ps + li * ALDP) + 8 * lk;
        const h16* pb1 = reinterpret_cast<const h16*>(Ps + (16 + li) * ALDP) + 8 * lk;
#pragma unroll
        for (int k0 = 0; k0 < AKP; k0 += 32) {
            const u32x4 a = *reinterpret_cast<const u32x4*>(va + k0);
            o0 = P::mfma_k32(a, *reinterpret_cast<const u32x4*>(pb0 + k0), o0);
            o1 = P::mfma_k32(a, *reinterpret_cast<const u32x4*>(pb1 + k0), o1);
        }
        // C/D: row = 4 * (lane >> 4) + r (d), col = lane & 15 (query); (attn @ v).transpose(1, 2).reshape(B, N, C)
        const int qa_ = q0 + li, qb_ = qa_ + 16;
        h16* dst = ao + (size_t)b * T * D + h * HD + wave * 16 + 4 * lk;
        if (qa_ < T) *reinterpret_cast<u32x2*>(dst + (size_t)qa_ * D) = u32x2{P::pack2(o0[0], o0[1]), P::pack2(o0[2], o0[3])};
        if (qb_ < T) *reinterpret_cast<u32x2*>(dst + (size_t)qb_ * D) = u32x2{P::pack2(o1[0], o1[1]), P::pack2(o1[2], o1[3])};
    }
}

// the one rounding of a weight: fp32 -> 16 bits, to nearest even, layout unchanged
template <class P>
__global__ __launch_bounds__(256) void dino16_round_kernel(const float* __restrict__ src, h16* __restrict__ dst, long long n) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < n) dst[e] = P::bits(src[e]);
}

template <class P, int EPI, int K, int BM>
void launch_gemm16(const h16* A, const h16* W, const float* bias, void* out, const float* extra, int M, int N, hipStream_t st) {
    static_assert(K % BK == 0, "GEMM tiles");
    dino16_gemm_kernel<P, EPI, K, BM><<<dim3(N / BN, (M + BM - 1) / BM), 256, 0, st>>>(A, W, bias, out, extra, M, N, NP);
}
static_assert(D % BN == 0 && (3 * D) % BN == 0 && HID % BN == 0 && D % BK == 0 && KE % BK == 0 && HID % BK == 0, "GEMM tiles");

template <class P>
int32_t pack16(const nsos_dino_tensors* t, void* packed, hipStream_t st) {
    float* f = (float*)packed;
    h16* hw = (h16*)((char*)packed + F_SIZE * 4);
    auto copy = [&](const float* src, float* dst, long long n) {
        dino_copy_kernel<dino16_path><<<blocks_for(n), 256, 0, st>>>(src, dst, n);
    };
    auto round = [&](const float* src, h16* dst, long long n) { dino16_round_kernel<P><<<blocks_for(n), 256, 0, st>>>(src, dst, n); };
    copy(t->pos_embed + D, f + F_POS + D, (long long)NP * D);
    dino_add_kernel<dino16_path><<<blocks_for(D), 256, 0, st>>>(t->cls_token, t->pos_embed, f + F_POS, D);
    round(t->patch_w, hw + H_EMB_W, (long long)D * KE);
    copy(t->patch_b, f + F_EMB_B, D);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const nsos_dino_block_tensors& b = t->blocks[i];
        float* q = f + F_BLOCKS + (size_t)i * FB_SIZE;
        h16* g = hw + H_BLOCKS + (size_t)i * HB_SIZE;
        copy(b.norm1_w, q + FB_LN1W, D), copy(b.norm1_b, q + FB_LN1B, D);
        round(b.qkv_w, g + HB_QKVW, (long long)3 * D * D), copy(b.qkv_b, q + FB_QKVB, 3 * D);
        round(b.proj_w, g + HB_PROJW, (long long)D * D), copy(b.proj_b, q + FB_PROJB, D);
        copy(b.norm2_w, q + FB_LN2W, D), copy(b.norm2_b, q + FB_LN2B, D);
        round(b.fc1_w, g + HB_FC1W, (long long)HID * D), copy(b.fc1_b, q + FB_FC1B, HID);
        round(b.fc2_w, g + HB_FC2W, (long long)D * HID), copy(b.fc2_b, q + FB_FC2B, D);
    }
    return nsos_launch_status();
}

template <class P>
int32_t forward16(const float* input, int batch, int in_h, int in_w, int patch_stride, int flags, const void* packed, void* workspace,
                  float* feat, float* cls, float* attn, float* prepared, float* blocks, hipStream_t st) {
    const float* f = (const float*)packed;
    const h16* hw = (const h16*)((const char*)packed + F_SIZE * 4);
    char* ws = (char*)workspace;
    const size_t Bn = (size_t)batch;
    float *x = (float*)(ws + Bn * W16_X), *row0 = (float*)(ws + Bn * W16_ROW0);
    h16 *ln = (h16*)(ws + Bn * W16_LN), *qkv = (h16*)(ws + Bn * W16_QKV), *ao = (h16*)(ws + Bn * W16_AO), *hid = (h16*)(ws + Bn * W16_HID),
        *tok = (h16*)(ws + Bn * W16_TOK);
    const int M = batch * T;

    dino16_prepare_kernel<P><<<blocks_for((long long)batch * NP * (KE / 2)), 256, 0, st>>>(input, batch, in_h, in_w, patch_stride, flags, f + F_POS,
                                                                                           (unsigned*)tok, x, prepared);
    launch_gemm16<P, EPI16_EMBED, KE, 32>(tok, hw + H_EMB_W, f + F_EMB_B, x, f + F_POS, batch * NP, D, st);
    for (int i = 0; i < NSOS_DINO_DEPTH; ++i) {
        const float* q = f + F_BLOCKS + (size_t)i * FB_SIZE;
        const h16* g = hw + H_BLOCKS + (size_t)i * HB_SIZE;
        dino16_layernorm_kernel<P><<<(M + 3) / 4, 256, 0, st>>>(x, q + FB_LN1W, q + FB_LN1B, (unsigned*)ln, M);
        launch_gemm16<P, EPI16_BIAS, D, 64>(ln, g + HB_QKVW, q + FB_QKVB, qkv, nullptr, M, 3 * D, st);
        dino16_attention_kernel<P><<<dim3((T + AQT - 1) / AQT, HEADS, batch), 256, 0, st>>>(qkv, ao,
                                                                                            (i == NSOS_DINO_DEPTH - 1 && attn) ? row0 : nullptr);
        launch_gemm16<P, EPI16_RESIDUAL, D, 32>(ao, g + HB_PROJW, q + FB_PROJB, x, x, M, D, st);
        dino16_layernorm_kernel<P><<<(M + 3) / 4, 256, 0, st>>>(x, q + FB_LN2W, q + FB_LN2B, (unsigned*)ln, M);
        launch_gemm16<P, EPI16_GELU, D, 64>(ln, g + HB_FC1W, q + FB_FC1B, hid, nullptr, M, HID, st);
        launch_gemm16<P, EPI16_RESIDUAL, HID, 32>(hid, g + HB_FC2W, q + FB_FC2B, x, x, M, D, st);
        if (blocks)
            dino_copy_kernel<dino16_path><<<blocks_for((long long)M * D), 256, 0, st>>>(x, blocks + (size_t)i * M * D, (long long)M * D);
    }
    if (feat || cls || attn)
        dino_outputs_kernel<dino16_path><<<blocks_for((long long)M * D), 256, 0, st>>>(x, attn ? row0 : nullptr, batch, feat, cls,
                                                                                       attn);
    return nsos_launch_status();
}

}  // namespace

extern "C" size_t nsos_dino_packed16_bytes(void) { return P16_BYTES; }

extern "C" size_t nsos_dino_workspace16_bytes(int32_t batch) {
    return (batch >= 1 && batch <= NSOS_DINO_MAX_BATCH) ? (size_t)batch * W16_SIZE : 0;
}

extern "C" int32_t nsos_dino_pack16(const nsos_dino_tensors* t, int32_t precision, void* packed, size_t packed_bytes, void* stream) {
    NSOS_REQUIRE(packed, NSOS_ERR_NULL_POINTER);
    if (int32_t c = dino_check_tensors(t)) return c;
    NSOS_REQUIRE(precision == NSOS_DTYPE_F16 || precision == NSOS_DTYPE_BF16, NSOS_ERR_UNSUPPORTED);   // fp32: nsos_dino_pack
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(packed_bytes >= P16_BYTES, NSOS_ERR_BUFFER_TOO_SMALL);
    return precision == NSOS_DTYPE_F16 ? pack16<F16>(t, packed, (hipStream_t)stream) : pack16<BF16>(t, packed, (hipStream_t)stream);
}

extern "C" int32_t nsos_dino_forward16(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                                       int32_t precision, const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls,
                                       float* attn, float* prepared, float* blocks, void* stream) {
    if (int32_t c = dino_check_forward(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, workspace_bytes,
                                       nsos_dino_workspace16_bytes, precision == NSOS_DTYPE_F16 || precision == NSOS_DTYPE_BF16))   // fp32: nsos_dino_forward
        return c;
    hipStream_t st = (hipStream_t)stream;
    return precision == NSOS_DTYPE_F16
               ? forward16<F16>(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, feat, cls, attn, prepared, blocks, st)
               : forward16<BF16>(input, batch, in_h, in_w, patch_stride, flags, packed, workspace, feat, cls, attn, prepared, blocks, st);
}
