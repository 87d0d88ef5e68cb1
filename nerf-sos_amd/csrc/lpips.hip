// LPIPS v0.1, net='alex', lpips=True, spatial=False, eval mode; forward only, fp32 (include/nerf_sos_hip.h "LPIPS").
// Replaces utils/image.py:149-160 (lpips -> lpips_alex) as engines/eval.py:87 calls it, with five kernels:
//   lpips_pack_conv_kernel  conv weight [Cout][Cin][k][k] -> Wt[K][Cout], K index (ky*k + kx)*Cin + c, rows past K zero
//   lpips_conv_kernel       implicit GEMM on v_mfma_f32_32x32x2_f32: rows = the output pixels of all 2N images, columns = Cout,
//                           epilogue bias + ReLU; conv1's gather applies the scaling layer (and 2x-1) and reads NCHW or NHWC
//   lpips_pool_kernel       max-pool k3 s2 (floor) on pixel-major features
//   lpips_distance_kernel   per (layer, pair): channel norms, lin-weighted squared difference, per-block pixel sums
//   lpips_finish_kernel     per pair: the blocks' sums, / pixels, the five layers added in order 0..4
// Activations are pixel-major [image][y][x][channel], image 2b = img0[b], image 2b+1 = img1[b].  Every sum runs in a fixed order
// (the header states it); no atomics; an output element of a convolution is one chain that reads its own image only, and a
// distance workgroup reads one image pair only, so an image's bits do not depend on the batch it travels in.
#include "common.h"
#include "gemm32_tile.h"

namespace {

using nsos::blocks_for;
using nsos::gemm32::GK;
using nsos::gemm32::GM;
using nsos::gemm32::GN;

constexpr int NL = NSOS_LPIPS_LAYERS;
constexpr int CIN[NL] = {3, 64, 192, 384, 256}, COUT[NL] = {64, 192, 384, 256, 256}, KS[NL] = {11, 5, 3, 3, 3};
constexpr int kdim(int l) { return CIN[l] * KS[l] * KS[l]; }
constexpr int kpad(int l) { return (kdim(l) + GK - 1) / GK * GK; }   // conv1: 363 -> 384, the others are multiples of 32
constexpr int DB = NSOS_LPIPS_DIST_BLOCKS;

// ---- packed stream (floats) ----------------------------------------------------------------------------------------------------
struct PackedLayout {
    size_t shift, scale, w[NL], b[NL], lin[NL], total;
};
constexpr PackedLayout packed_layout() {
    PackedLayout L = {};
    size_t s = 0;
    L.shift = s, s += 4;
    L.scale = s, s += 4;
    for (int l = 0; l < NL; ++l) {
        L.w[l] = s, s += (size_t)kpad(l) * COUT[l];
        L.b[l] = s, s += COUT[l];
    }
    for (int l = 0; l < NL; ++l) L.lin[l] = s, s += COUT[l];
    L.total = s;
    return L;
}
constexpr PackedLayout PL = packed_layout();
static_assert(PL.w[0] % 4 == 0 && PL.w[1] % 4 == 0 && PL.w[2] % 4 == 0 && PL.w[3] % 4 == 0 && PL.w[4] % 4 == 0, "float4 rows");
static_assert(COUT[0] % GN == 0 && COUT[1] % GN == 0 && COUT[2] % GN == 0 && COUT[3] % GN == 0 && COUT[4] % GN == 0, "GEMM tiles");
static_assert(CIN[1] % GK == 0 && CIN[2] % GK == 0 && CIN[3] % GK == 0 && CIN[4] % GK == 0, "a K tile lies inside one tap");

// ---- geometry of one call ------------------------------------------------------------------------------------------------------
struct Geometry {
    int h[NL], w[NL];      // feature maps
    int ph[2], pw[2];      // pooled maps (inputs of conv2 and conv3)
    size_t feat[NL], pool[2], part, total;   // workspace offsets in floats
};
// false = refused: a size outside 31..16384, a batch outside 1..1024, more GEMM rows than an int holds
bool geometry(long long batch, long long h, long long w, Geometry& G) {
    if (batch < 1 || batch > NSOS_LPIPS_MAX_BATCH || h < NSOS_LPIPS_MIN_SIZE || w < NSOS_LPIPS_MIN_SIZE || h > (1 << 14) || w > (1 << 14))
        return false;
    G.h[0] = (int)((h + 4 - 11) / 4 + 1), G.w[0] = (int)((w + 4 - 11) / 4 + 1);
    G.ph[0] = (G.h[0] - 3) / 2 + 1, G.pw[0] = (G.w[0] - 3) / 2 + 1;
    G.h[1] = G.ph[0], G.w[1] = G.pw[0];
    G.ph[1] = (G.h[1] - 3) / 2 + 1, G.pw[1] = (G.w[1] - 3) / 2 + 1;
    for (int l = 2; l < NL; ++l) G.h[l] = G.ph[1], G.w[l] = G.pw[1];
    if (2 * batch * G.h[0] * G.w[0] > (long long)INT32_MAX - GM) return false;
    size_t s = 0;
    const size_t n = 2 * (size_t)batch;
    for (int l = 0; l < NL; ++l) G.feat[l] = s, s += n * G.h[l] * G.w[l] * COUT[l];
    for (int i = 0; i < 2; ++i) G.pool[i] = s, s += n * G.ph[i] * G.pw[i] * COUT[i];
    G.part = s, s += 2 * (size_t)batch * NL * DB;   // doubles
    G.total = s;
    return true;
}

// ---- pack ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lpips_pack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int cin, int cout, int ks,
                                                              int kp) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)kp * cout) return;
    const int o = (int)(e % cout), k = (int)(e / cout);
    float v = 0.0f;
    if (k < cin * ks * ks) {
        const int tap = k / cin, c = k - tap * cin, ky = tap / ks, kx = tap - ky * ks;
        v = src[(((size_t)o * cin + c) * ks + ky) * ks + kx];
    }
    dst[e] = v;
}
__global__ __launch_bounds__(256) void lpips_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int n_pad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_pad) dst[e] = e < n ? src[e] : 0.0f;
}

// ---- convolution: out[row][col] = relu(bias[col] + sum_k A[row][k] * Wt[k][col]), row = (image, oy, ox), k = (ky*KS + kx)*Cin + c.
// 64x64 outputs per workgroup, four waves of 32x32, K in steps of 32 through LDS.  Per output element: every K tile is one fma chain
// over its 32 products, k ascending, from zero; the tiles' partial sums p_0, p_1, .. are added in ascending order as (tot, lo) with
// two-sum (tot' = fl(tot + p), lo += the exact rounding error of that addition); the result is fl(fl(tot + lo) + bias), then ReLU.
// One chain over all K (up to 3456 products) sits 4-5x further from fp64 than ATen's blocked sums, and the distance amplifies
// feature errors by 1 / (the relative difference of the two images): it missed the tests' bar on 97x130 images.
// A tap outside the image contributes a = 0 (the convolution's zero padding): fma(0, w, acc) = acc.
struct ConvArgs {
    const float *in0, *in1;   // FIRST: img0, img1 ([N,3,H,W] or [N,H,W,3]); otherwise in0 = pixel-major [2N][Hi][Wi][Cin]
    const float *Wt, *bias, *sc;   // sc: shift[4], scale[4] (FIRST)
    float* out;
    int Hi, Wi, Ho, Wo, Cin, Cout, M, flags;
};

template <int KSZ, int STRIDE, int PAD, bool FIRST>
__global__ __launch_bounds__(256) void lpips_conv_kernel(ConvArgs a) {
    const int nt = a.Cout / GN;
    const int m0 = (blockIdx.x / nt) * GM, n0 = (blockIdx.x % nt) * GN;
    const int ar = nsos::gemm32::a_row(), ak = nsos::gemm32::a_k();
    int img[2], iy0[2], ix0[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {   // rows past M repeat the last one; never stored
        const int row = min(m0 + ar + 32 * r, a.M - 1);
        const int hw = a.Ho * a.Wo;
        img[r] = row / hw;
        const int rem = row - img[r] * hw, oy = rem / a.Wo;
        iy0[r] = oy * STRIDE - PAD, ix0[r] = (rem - oy * a.Wo) * STRIDE - PAD;
    }
    float shift[3], scale[3];
    if constexpr (FIRST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) shift[c] = a.sc[c], scale[c] = a.sc[4 + c];
    }
    int ky = 0, kx = 0, c0 = 0;   // the tap and first channel of the K tile the loader fetches next (not FIRST)
    auto load_a = [&](int k0, float4(&ra)[2]) {
        if constexpr (FIRST) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = k0 + ak + j, tap = k / 3, c = k - 3 * tap, ty = tap / KSZ, tx = tap - ty * KSZ;
                    const int iy = iy0[r] + ty, ix = ix0[r] + tx;
                    v[j] = 0.0f;
                    if (k < kdim(0) && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) {
                        const float* src = (img[r] & 1) ? a.in1 : a.in0;
                        const int b = img[r] >> 1;
                        float x = (a.flags & NSOS_LPIPS_NHWC) ? src[(((size_t)b * a.Hi + iy) * a.Wi + ix) * 3 + c]
                                                              : src[(((size_t)b * 3 + c) * a.Hi + iy) * a.Wi + ix];
                        if (a.flags & NSOS_LPIPS_NORMALIZE) x = 2.0f * x - 1.0f;
                        v[j] = (x - shift[c]) / scale[c];   // the scaling layer
                    }
                }
                ra[r] = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int iy = iy0[r] + ky, ix = ix0[r] + kx;
                ra[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi)
                    ra[r] = *reinterpret_cast<const float4*>(a.in0 + (((size_t)img[r] * a.Hi + iy) * a.Wi + ix) * a.Cin + c0 + ak);
            }
            c0 += GK;
            if (c0 == a.Cin) {
                c0 = 0;
                if (++kx == KSZ) kx = 0, ++ky;
            }
        }
    };
    float* out_col = a.out + nsos::gemm32::out_col(n0);   // column base: one 64-bit add per row in the epilogue
    nsos::gemm32::tile<nsos::gemm32::TwoSumOfTiles>(FIRST ? kpad(0) : a.Cin * KSZ * KSZ, m0, n0, a.M, a.Wt, a.bias, a.Cout, load_a,
                                                    [&](int row, int, float v) {
                                                        out_col[(size_t)row * a.Cout] = v < 0.0f ? 0.0f : v;   // ReLU; a NaN stays a NaN
                                                    });
}

// ---- max-pool k3 s2, no padding, floor: out[i][py][px][c] = max over dy, dx = 0..2 (dy outer) of in[i][2py + dy][2px + dx][c] ----
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out, int n_img, int Hi, int Wi, int Hp,
                                                         int Wp, int C) {
    const int c4 = C / 4;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_img * Hp * Wp * c4) return;
    const int c = (int)(e % c4) * 4;
    long long p = e / c4;
    const int px = (int)(p % Wp);
    p /= Wp;
    const int py = (int)(p % Hp), i = (int)(p / Hp);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float4 v = *reinterpret_cast<const float4*>(in + (((size_t)i * Hi + 2 * py + dy) * Wi + 2 * px + dx) * C + c);
            m.x = fmaxf(m.x, v.x), m.y = fmaxf(m.y, v.y), m.z = fmaxf(m.z, v.z), m.w = fmaxf(m.w, v.w);
        }
    *reinterpret_cast<float4*>(out + (((size_t)i * Hp + py) * Wp + px) * C + c) = m;
}

// ---- distance ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lpips_wave_sum(float v) {   // xor butterfly 32,16,8,4,2,1: every lane ends with the same bits
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct DistArgs {
    const float* f[NL];     // [2N][P][C]
    const float* lin[NL];
    int P[NL], C[NL];
};

// workgroup (g, layer, pair): pixels [g*chunk, (g+1)*chunk), chunk = ceil(P / DB); wave w takes every 4th of them ascending, one
// pixel at a time: lane j holds channels j, j+64, ..; sums over the channels = the lane's own in ascending order, then the butterfly.
//   s0 = sum f0^2, s1 = sum f1^2; n = sqrt(s) + 1e-10; t = sum lin[c] * (f0[c]/n0 - f1[c]/n1)^2   (fp32)
// The wave adds its pixels' t in fp64; the block's value is wave 0 + 1 + 2 + 3 in that order.
__global__ __launch_bounds__(256) void lpips_distance_kernel(DistArgs d, double* __restrict__ part) {
    __shared__ double red[4];
    const int g = blockIdx.x, l = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int P = d.P[l], C = d.C[l];
    const float* f0 = d.f[l] + (size_t)(2 * b) * P * C;
    const float* f1 = f0 + (size_t)P * C;
    const float* lin = d.lin[l];
    const int chunk = (P + DB - 1) / DB, lo = g * chunk, hi = min(P, lo + chunk);
    float w[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) w[j] = (lane + 64 * j) < C ? lin[lane + 64 * j] : 0.0f;
    double acc = 0.0;
    for (int p = lo + wave; p < hi; p += 4) {
        float u[6], v[6], s0 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            u[j] = v[j] = 0.0f;
            if (lane + 64 * j < C) {
                u[j] = f0[(size_t)p * C + lane + 64 * j], v[j] = f1[(size_t)p * C + lane + 64 * j];
                s0 += u[j] * u[j], s1 += v[j] * v[j];
            }
        }
        const float n0 = sqrtf(lpips_wave_sum(s0)) + 1e-10f, n1 = sqrtf(lpips_wave_sum(s1)) + 1e-10f;
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < 6; ++j)
            if (lane + 64 * j < C) {
                const float df = u[j] / n0 - v[j] / n1;
                t += w[j] * (df * df);
            }
        acc += (double)lpips_wave_sum(t);
    }
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[((size_t)b * NL + l) * DB + g] = ((red[0] + red[1]) + red[2]) + red[3];
}

// per pair: d_l = (float)((sum of the layer's DB partials, g ascending, fp64) / P_l); out = (((d_0 + d_1) + d_2) + d_3) + d_4 in fp32
struct FinishArgs {
    int P[NL];
};
__global__ __launch_bounds__(64) void lpips_finish_kernel(const double* __restrict__ part, FinishArgs f, float* __restrict__ out,
                                                          float* __restrict__ layers) {
    __shared__ float dl[NL];
    const int b = blockIdx.x, l = threadIdx.x;
    if (l < NL) {
        double s = 0.0;
        for (int g = 0; g < DB; ++g) s += part[((size_t)b * NL + l) * DB + g];
        dl[l] = (float)(s / (double)f.P[l]);
        if (layers) layers[(size_t)b * NL + l] = dl[l];
    }
    __syncthreads();
    if (l == 0) {
        float v = dl[0];
        for (int i = 1; i < NL; ++i) v += dl[i];
        out[b] = v;
    }
}

template <int KSZ, int STRIDE, int PAD, bool FIRST>
void launch_conv(const ConvArgs& a, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.M + GM - 1) / GM) * (unsigned)(a.Cout / GN);
    lpips_conv_kernel<KSZ, STRIDE, PAD, FIRST><<<blocks, 256, 0, st>>>(a);
}

}  // namespace

extern "C" size_t nsos_lpips_packed_bytes(void) { return PL.total * sizeof(float); }

extern "C" size_t nsos_lpips_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
    Geometry G;
    return geometry(batch, h, w, G) ? G.total * sizeof(float) : 0;
}

extern "C" int32_t nsos_lpips_pack(const nsos_lpips_tensors* t, void* packed, size_t packed_bytes, void* stream) {
    NSOS_REQUIRE(t && packed && t->shift && t->scale, NSOS_ERR_NULL_POINTER);
    for (int l = 0; l < NL; ++l) NSOS_REQUIRE(t->conv_w[l] && t->conv_b[l] && t->lin_w[l], NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(((uintptr_t)packed & 15) == 0, NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(packed_bytes >= PL.total * sizeof(float), NSOS_ERR_BUFFER_TOO_SMALL);
    hipStream_t st = (hipStream_t)stream;
    float* p = (float*)packed;
    lpips_copy_kernel<<<1, 256, 0, st>>>(t->shift, p + PL.shift, 3, 4);
    lpips_copy_kernel<<<1, 256, 0, st>>>(t->scale, p + PL.scale, 3, 4);
    for (int l = 0; l < NL; ++l) {
        lpips_pack_conv_kernel<<<blocks_for((long long)kpad(l) * COUT[l]), 256, 0, st>>>(t->conv_w[l], p + PL.w[l], CIN[l], COUT[l], KS[l], kpad(l));
        lpips_copy_kernel<<<blocks_for(COUT[l]), 256, 0, st>>>(t->conv_b[l], p + PL.b[l], COUT[l], COUT[l]);
        lpips_copy_kernel<<<blocks_for(COUT[l]), 256, 0, st>>>(t->lin_w[l], p + PL.lin[l], COUT[l], COUT[l]);
    }
    return nsos_launch_status();
}

extern "C" int32_t nsos_lpips_forward(const float* img0, const float* img1, int32_t batch, int32_t h, int32_t w, int32_t flags,
                                      const void* packed, float* out, float* layers, float* feats, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    NSOS_REQUIRE(img0 && img1 && packed && out && workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(batch >= 0 && h > 0 && w > 0, NSOS_ERR_BAD_SHAPE);
    if (batch == 0) return NSOS_OK;
    NSOS_REQUIRE((flags & ~(NSOS_LPIPS_NHWC | NSOS_LPIPS_NORMALIZE)) == 0, NSOS_ERR_UNSUPPORTED);
    Geometry G;
    NSOS_REQUIRE(geometry(batch, h, w, G), NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(((uintptr_t)img0 & 3) == 0 && ((uintptr_t)img1 & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)layers & 3) == 0 &&
                     ((uintptr_t)packed & 15) == 0 && ((uintptr_t)feats & 15) == 0 && ((uintptr_t)workspace & 15) == 0,
                 NSOS_ERR_MISALIGNED);
    NSOS_REQUIRE(workspace_bytes >= G.total * sizeof(float), NSOS_ERR_BUFFER_TOO_SMALL);

    hipStream_t st = (hipStream_t)stream;
    const float* p = (const float*)packed;
    float* ws = (float*)workspace;
    const int n_img = 2 * batch;
    float* F[NL];
    for (int l = 0; l < NL; ++l) F[l] = feats ? feats + G.feat[l] : ws + G.feat[l];   // `feats` has the workspace's feature layout
    float* pool[2] = {ws + G.pool[0], ws + G.pool[1]};
    double* part = (double*)(ws + G.part);

    auto conv_args = [&](int l, const float* in0, const float* in1, int Hi, int Wi) {
        ConvArgs a;
        a.in0 = in0, a.in1 = in1, a.Wt = p + PL.w[l], a.bias = p + PL.b[l], a.sc = p + PL.shift, a.out = F[l];
        a.Hi = Hi, a.Wi = Wi, a.Ho = G.h[l], a.Wo = G.w[l], a.Cin = CIN[l], a.Cout = COUT[l], a.M = n_img * G.h[l] * G.w[l], a.flags = flags;
        return a;
    };
    launch_conv<11, 4, 2, true>(conv_args(0, img0, img1, h, w), st);
    lpips_pool_kernel<<<blocks_for((long long)n_img * G.ph[0] * G.pw[0] * (COUT[0] / 4)), 256, 0, st>>>(F[0], pool[0], n_img, G.h[0], G.w[0], G.ph[0],
                                                                                                        G.pw[0], COUT[0]);
    launch_conv<5, 1, 2, false>(conv_args(1, pool[0], nullptr, G.ph[0], G.pw[0]), st);
    lpips_pool_kernel<<<blocks_for((long long)n_img * G.ph[1] * G.pw[1] * (COUT[1] / 4)), 256, 0, st>>>(F[1], pool[1], n_img, G.h[1], G.w[1], G.ph[1],
                                                                                                        G.pw[1], COUT[1]);
    launch_conv<3, 1, 1, false>(conv_args(2, pool[1], nullptr, G.ph[1], G.pw[1]), st);
    launch_conv<3, 1, 1, false>(conv_args(3, F[2], nullptr, G.h[2], G.w[2]), st);
    launch_conv<3, 1, 1, false>(conv_args(4, F[3], nullptr, G.h[3], G.w[3]), st);

    DistArgs d;
    FinishArgs f;
    for (int l = 0; l < NL; ++l) d.f[l] = F[l], d.lin[l] = p + PL.lin[l], d.C[l] = COUT[l], d.P[l] = f.P[l] = G.h[l] * G.w[l];
    lpips_distance_kernel<<<dim3(DB, NL, batch), 256, 0, st>>>(d, part);
    lpips_finish_kernel<<<batch, 64, 0, st>>>(part, f, out, layers);
    return nsos_launch_status();
}
