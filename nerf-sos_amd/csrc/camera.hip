// CameraTransformer (models/camera.py:81-143): per-camera pose corrections applied to rays that carry a camera id, and the
// backward that ends the ray-gradient path in rvec.grad / tvec.grad.  Formulas, summation order and the out-of-range rule are
// stated in include/nerf_sos_hip.h ("CameraTransformer"); DESIGN.md section 4.12 says why the reduction is the one below.
//
//   camera_forward_kernel  : one thread per ray: R(rvec[id]) recomputed per thread (a root, four divisions, ~30 flops: cheaper
//                            than a second launch), d' = R d, o' = o + t.  24 B read + 4 B id, 24 B written per ray.
//   camera_partial_kernel  : grid (chunk k, camera c): the workgroup scans chunk k's ids and sums camera c's rays in fp64.
//   camera_finish_kernel   : one thread per camera: the K partials in order, the contraction with dR/dq and the theta terms in fp64.
//   camera_ray_grad_kernel : one thread per ray: g_o = g_o', g_d = R^T g_d'.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSums = 12;   // g_tvec[3] then G[3][3] row-major

struct CamRot { float r[9]; };

// camera.py:104-118 in fp32, every operation rounded on its own (the Makefile's -ffp-contract=off), `** 2` as x * x
__device__ __forceinline__ CamRot cam_rot(const float* __restrict__ q) {
    const float x = q[0], y = q[1], z = q[2], w = q[3];
    const float theta = sqrtf(1e-5f + (((x * x + y * y) + z * z) + w * w));
    const float a = x / theta, b = y / theta, c = z / theta, s = w / theta;
    CamRot R;
    R.r[0] = (1.0f - 2.0f * (b * b)) - 2.0f * (c * c);
    R.r[1] = 2.0f * (a * b - c * s);
    R.r[2] = 2.0f * (a * c + b * s);
    R.r[3] = 2.0f * (a * b + c * s);
    R.r[4] = (1.0f - 2.0f * (a * a)) - 2.0f * (c * c);
    R.r[5] = 2.0f * (b * c - a * s);
    R.r[6] = 2.0f * (a * c - b * s);
    R.r[7] = 2.0f * (a * s + b * c);
    R.r[8] = (1.0f - 2.0f * (a * a)) - 2.0f * (b * b);
    return R;
}

__global__ __launch_bounds__(kThreads) void camera_forward_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                  const int32_t* __restrict__ ids, const float* __restrict__ rvec,
                                                                  const float* __restrict__ tvec, int64_t n, int n_cams,
                                                                  float* __restrict__ out_o, float* __restrict__ out_d) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = ids[i];
    if (c < 0 || c >= n_cams) {   // the reference raises; here: NaN, and nothing outside rvec / tvec is read
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 3; ++k) out_o[3 * i + k] = out_d[3 * i + k] = nan;
        return;
    }
    const CamRot R = cam_rot(rvec + 4 * (int64_t)c);
    const float d0 = rays_d[3 * i], d1 = rays_d[3 * i + 1], d2 = rays_d[3 * i + 2];
    const float o0 = rays_o[3 * i], o1 = rays_o[3 * i + 1], o2 = rays_o[3 * i + 2];
    const float* t = tvec + 3 * (int64_t)c;
#pragma unroll
    for (int r = 0; r < 3; ++r) out_d[3 * i + r] = (d0 * R.r[3 * r] + d1 * R.r[3 * r + 1]) + d2 * R.r[3 * r + 2];   // camera.py:138
    out_o[3 * i] = o0 + t[0];                                                                                        // camera.py:141
    out_o[3 * i + 1] = o1 + t[1];
    out_o[3 * i + 2] = o2 + t[2];
}

// grid (K, n_cams).  partial [n_cams][K][12] fp64; every slot is written (zeros for a chunk without a ray of this camera)
__global__ __launch_bounds__(kThreads) void camera_partial_kernel(const float* __restrict__ g_o, const float* __restrict__ g_d,
                                                                  const float* __restrict__ rays_d, const int32_t* __restrict__ ids,
                                                                  int64_t n, int64_t chunk, double* __restrict__ partial) {
    const int k = blockIdx.x, c = blockIdx.y, K = gridDim.x;
    const int64_t b = (int64_t)k * chunk;
    const int64_t e = b + chunk < n ? b + chunk : n;
    double acc[kSums];
#pragma unroll
    for (int v = 0; v < kSums; ++v) acc[v] = 0.0;
    for (int64_t i = b + threadIdx.x; i < e; i += kThreads) {
        if (ids[i] != c) continue;
        const double go[3] = {(double)g_o[3 * i], (double)g_o[3 * i + 1], (double)g_o[3 * i + 2]};
        const double gd[3] = {(double)g_d[3 * i], (double)g_d[3 * i + 1], (double)g_d[3 * i + 2]};
        const double dd[3] = {(double)rays_d[3 * i], (double)rays_d[3 * i + 1], (double)rays_d[3 * i + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            acc[r] += go[r];
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[3 + 3 * r + j] += gd[r] * dd[j];   // exact product (2 x 24 bits), one rounding per add
        }
    }
    __shared__ double s[kThreads / NSOS_WAVE][kSums];
    const int lane = threadIdx.x % NSOS_WAVE, wave = threadIdx.x / NSOS_WAVE;
#pragma unroll
    for (int v = 0; v < kSums; ++v) {
        const double t = nsos_wave_sum(acc[v]);
        if (lane == 0) s[wave][v] = t;
    }
    __syncthreads();
    if (threadIdx.x < kSums) {
        const int v = threadIdx.x;
        partial[((size_t)c * K + k) * kSums + v] = ((s[0][v] + s[1][v]) + s[2][v]) + s[3][v];
    }
}

// one thread per camera
__global__ __launch_bounds__(NSOS_WAVE) void camera_finish_kernel(const double* __restrict__ partial, const float* __restrict__ rvec,
                                                                  int n_cams, int K, float* __restrict__ g_rvec, float* __restrict__ g_tvec) {
    const int c = blockIdx.x * NSOS_WAVE + threadIdx.x;
    if (c >= n_cams) return;
    double S[kSums];
#pragma unroll
    for (int v = 0; v < kSums; ++v) S[v] = 0.0;
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < kSums; ++v) S[v] += partial[((size_t)c * K + k) * kSums + v];
    if (g_tvec)
        for (int v = 0; v < 3; ++v) g_tvec[3 * c + v] = (float)S[v];
    if (!g_rvec) return;
    const double* G = S + 3;
    const double q[4] = {(double)rvec[4 * c], (double)rvec[4 * c + 1], (double)rvec[4 * c + 2], (double)rvec[4 * c + 3]};
    const double theta = sqrt((double)1e-5f + (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]));   // the forward's fp32 epsilon
    const double x = q[0] / theta, y = q[1] / theta, z = q[2] / theta, w = q[3] / theta;
    // d R_ij / d (x, y, z, w) of the nine expressions in cam_rot, contracted with G_ij = sum g_d'[i] d[j]
    double gq[4];
    gq[0] = 2.0 * (y * G[1] + z * G[2] + y * G[3] - 2.0 * x * G[4] - w * G[5] + z * G[6] + w * G[7] - 2.0 * x * G[8]);
    gq[1] = 2.0 * (-2.0 * y * G[0] + x * G[1] + w * G[2] + x * G[3] + z * G[5] - w * G[6] + z * G[7] - 2.0 * y * G[8]);
    gq[2] = 2.0 * (-2.0 * z * G[0] - w * G[1] + x * G[2] + w * G[3] - 2.0 * z * G[4] + y * G[5] + x * G[6] + y * G[7]);
    gq[3] = 2.0 * (-z * G[1] + y * G[2] + z * G[3] - x * G[5] - y * G[6] + x * G[7]);
    const double dot = ((q[0] * gq[0] + q[1] * gq[1]) + q[2] * gq[2]) + q[3] * gq[3];
    const double t3 = theta * theta * theta;
    for (int v = 0; v < 4; ++v) g_rvec[4 * c + v] = (float)(gq[v] / theta - q[v] * dot / t3);
}

__global__ __launch_bounds__(kThreads) void camera_ray_grad_kernel(const float* __restrict__ g_o, const float* __restrict__ g_d,
                                                                   const int32_t* __restrict__ ids, const float* __restrict__ rvec,
                                                                   int64_t n, int n_cams, float* __restrict__ g_rays_o,
                                                                   float* __restrict__ g_rays_d) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int c = ids[i];
    const bool ok = c >= 0 && c < n_cams;   // an out-of-range ray's outputs are NaN whatever it holds: no gradient
    if (g_rays_o)
#pragma unroll
        for (int k = 0; k < 3; ++k) g_rays_o[3 * i + k] = ok ? g_o[3 * i + k] : 0.0f;
    if (g_rays_d) {
        if (!ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) g_rays_d[3 * i + k] = 0.0f;
            return;
        }
        const CamRot R = cam_rot(rvec + 4 * (int64_t)c);
        const float g0 = g_d[3 * i], g1 = g_d[3 * i + 1], g2 = g_d[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) g_rays_d[3 * i + j] = (g0 * R.r[j] + g1 * R.r[3 + j]) + g2 * R.r[6 + j];
    }
}

inline int camera_chunks(int64_t n_rays) {
    const int64_t k = (n_rays + NSOS_CAMERA_CHUNK - 1) / NSOS_CAMERA_CHUNK;
    return k < 1 ? 1 : (k > NSOS_CAMERA_MAX_CHUNKS ? NSOS_CAMERA_MAX_CHUNKS : (int)k);
}

}  // namespace

extern "C" size_t nsos_camera_workspace_bytes(int64_t n_rays, int32_t n_cams) {
    if (n_cams <= 0 || n_rays < 0) return 0;
    return (size_t)n_cams * camera_chunks(n_rays) * kSums * sizeof(double);
}

extern "C" int32_t nsos_camera_transform(const float* rays_o, const float* rays_d, const int32_t* cam_ids, const float* rvec,
                                         const float* tvec, int64_t n_rays, int32_t n_cams, float* out_o, float* out_d, void* stream) {
    NSOS_REQUIRE(n_cams > 0 && n_rays >= 0, NSOS_ERR_BAD_SHAPE);
    if (n_rays == 0) return NSOS_OK;
    NSOS_REQUIRE(rays_o && rays_d && cam_ids && rvec && tvec && out_o && out_d, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(n_cams <= NSOS_CAMERA_MAX_CAMS && (n_rays + kThreads - 1) / kThreads < (int64_t)1 << 31, NSOS_ERR_UNSUPPORTED);
    hipLaunchKernelGGL(camera_forward_kernel, dim3((unsigned)((n_rays + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       rays_o, rays_d, cam_ids, rvec, tvec, n_rays, n_cams, out_o, out_d);
    return nsos_launch_status();
}

extern "C" int32_t nsos_camera_transform_backward(const float* g_out_o, const float* g_out_d, const float* rays_d, const int32_t* cam_ids,
                                                  const float* rvec, int64_t n_rays, int32_t n_cams, void* workspace, size_t workspace_bytes,
                                                  float* g_rvec, float* g_tvec, float* g_rays_o, float* g_rays_d, void* stream) {
    NSOS_REQUIRE(n_cams > 0 && n_rays >= 0, NSOS_ERR_BAD_SHAPE);
    if (n_rays == 0) return NSOS_OK;
    NSOS_REQUIRE(g_out_o && g_out_d && rays_d && cam_ids && rvec, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(g_rvec || g_tvec || g_rays_o || g_rays_d, NSOS_ERR_NULL_POINTER);
    const bool params = g_rvec || g_tvec;
    NSOS_REQUIRE(!params || workspace, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(n_cams <= NSOS_CAMERA_MAX_CAMS && (n_rays + kThreads - 1) / kThreads < (int64_t)1 << 31, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(!params || workspace_bytes >= nsos_camera_workspace_bytes(n_rays, n_cams), NSOS_ERR_BUFFER_TOO_SMALL);
    hipStream_t st = (hipStream_t)stream;
    if (params) {
        const int K = camera_chunks(n_rays);
        const int64_t chunk = ((n_rays + K - 1) / K + kThreads - 1) / kThreads * kThreads;
        double* partial = static_cast<double*>(workspace);
        hipLaunchKernelGGL(camera_partial_kernel, dim3((unsigned)K, (unsigned)n_cams), dim3(kThreads), 0, st, g_out_o, g_out_d, rays_d,
                           cam_ids, n_rays, chunk, partial);
        hipLaunchKernelGGL(camera_finish_kernel, dim3((unsigned)((n_cams + NSOS_WAVE - 1) / NSOS_WAVE)), dim3(NSOS_WAVE), 0, st, partial,
                           rvec, n_cams, K, g_rvec, g_tvec);
    }
    if (g_rays_o || g_rays_d)
        hipLaunchKernelGGL(camera_ray_grad_kernel, dim3((unsigned)((n_rays + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g_out_o,
                           g_out_d, cam_ids, rvec, n_rays, n_cams, g_rays_o, g_rays_d);
    return nsos_launch_status();
}
