// Host side of the persistent MLP kernel families (mlp_fused, mlp_lp, mlp_lp16, mlp_x3, mlp_x316, mlp_x3_bwd): the
// argument checks, the parameter fill, the sem_mode / dtype dispatch and the launch they all share.  No device code.
// The ORDER of the checks is part of the C ABI (a call that is wrong in two ways reports the first): every family refuses in
//   NULL pointer -> shape -> [n_rays bound] -> [mode] -> alignment -> tile count,
// and what differs between them is an argument here, not a copy there.
#pragma once
#include "common.h"

#include <initializer_list>
#include <type_traits>

// ---- launch ---------------------------------------------------------------------------------------------------------
// One workgroup per CU at most, each walking the tiles: grid = min(n_tiles, CUs).  The kernel is a template argument, so every
// instantiation has its own per-device "LDS opt-in done" flag, as a function-local static (no lookup on the call path).
template <auto Kernel, class P>
int32_t nsos_launch_persistent(const P& params, int n_tiles, int block, int lds_bytes, hipStream_t stream) {
    static NsosPerDeviceFlag configured_on;
    bool& configured = configured_on.here();
    if (!configured) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return (int32_t)e;
        configured = true;
    }
    const int cus = nsos_device_cus();
    hipLaunchKernelGGL(Kernel, dim3(n_tiles < cus ? n_tiles : cus), dim3(block), lds_bytes, stream, params);
    return nsos_launch_status();
}

// ---- dispatch -------------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, I>{}) for the I in [0, N) that equals i; NSOS_ERR_UNSUPPORTED for any other i.  A combination
// that has no kernel is refused inside f with `if constexpr`, so it is never instantiated.
template <int N, class F>
int32_t nsos_dispatch_below(int i, F&& f) {
    if constexpr (N == 0) return NSOS_ERR_UNSUPPORTED;
    else return i == N - 1 ? f(std::integral_constant<int, N - 1>{}) : nsos_dispatch_below<N - 1>(i, f);
}
template <class F>
int32_t nsos_dispatch_sem(int32_t sem_mode, F&& f) {   // NSOS_SEM_NONE / _PLAIN / _COORD = 0 / 1 / 2
    return nsos_dispatch_below<3>(sem_mode, f);
}
template <class F>
int32_t nsos_dispatch_bool(bool b, F&& f) {
    return nsos_dispatch_below<2>(b ? 1 : 0, f);
}
// f(T16{}) with the family's number-format class of `dtype` (lp_common.h: lp::F16, lp::BF16)
template <class F16T, class BF16T, class F>
int32_t nsos_dispatch_dtype(int32_t dtype, F&& f) {
    if (dtype == NSOS_DTYPE_F16) return f(F16T{});
    if (dtype == NSOS_DTYPE_BF16) return f(BF16T{});
    return NSOS_ERR_UNSUPPORTED;
}
inline bool nsos_sem_mode_ok(int32_t sem_mode) { return sem_mode >= 0 && sem_mode <= 2; }
inline bool nsos_dtype16_ok(int32_t dtype) { return dtype == NSOS_DTYPE_F16 || dtype == NSOS_DTYPE_BF16; }

// ---- checks ---------------------------------------------------------------------------------------------------------
inline bool nsos_aligned16(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15) return false;
    return true;
}
// the additional outputs of a call: none NULL, [the mode supports them,] all 16-byte aligned
inline int32_t nsos_check_outputs(std::initializer_list<const void*> ptrs, bool mode_ok = true) {
    for (const void* p : ptrs) NSOS_REQUIRE(p, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(mode_ok, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(nsos_aligned16(ptrs), NSOS_ERR_MISALIGNED);
    return NSOS_OK;
}

// nsos_mlp_tensors as a packer needs it.  with_biases = false: what the backward chain packs -- weights only, and not layer 0
// (nothing propagates below the first layer).
inline int32_t nsos_check_mlp_tensors(const nsos_mlp_tensors* T, int32_t sem_mode, bool with_biases) {
    for (int l = with_biases ? 0 : 1; l < NSOS_NET_DEPTH; ++l) NSOS_REQUIRE(T->pts_w[l] && (T->pts_b[l] || !with_biases), NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(T->alpha_w && T->feature_w && T->views_w && T->rgb_w, NSOS_ERR_NULL_POINTER);
    if (with_biases) NSOS_REQUIRE(T->alpha_b && T->feature_b && T->views_b && T->rgb_b, NSOS_ERR_NULL_POINTER);
    if (sem_mode) NSOS_REQUIRE(T->sem0_w && T->sem2_w && ((T->sem0_b && T->sem2_b) || !with_biases), NSOS_ERR_NULL_POINTER);
    return NSOS_OK;
}
// a pack call: mode_ok = "sem_mode (and dtype) are known"; need = bytes the packed buffer must hold
inline int32_t nsos_check_pack(const nsos_mlp_tensors* T, int32_t sem_mode, bool mode_ok, const void* packed, size_t packed_bytes,
                               size_t need, bool with_biases = true) {
    NSOS_REQUIRE(T && packed, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(mode_ok, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(packed_bytes >= need, NSOS_ERR_BUFFER_TOO_SMALL);
    NSOS_REQUIRE(nsos_aligned16({packed}), NSOS_ERR_MISALIGNED);
    return nsos_check_mlp_tensors(T, sem_mode, with_biases);
}

// ---- ray calls ------------------------------------------------------------------------------------------------------
struct NsosRayCall {   // the arguments every nsos_mlp_*_rays* entry point starts with (an empty batch has returned NSOS_OK before)
    const void* packed;
    const float *rays_o, *rays_d, *viewdirs, *z_vals;
    int64_t n_rays;
    int32_t n_samples;
    float* raw;
};
// bound_rays: refuse n_rays >= 2^31 (the 16-bit and split-fp16 families index rays with 32 bits; the fp32 kernel does not).
// mode_ok: sem_mode / dtype are known -- `true` where the family finds out at its dispatch, after every other check.
inline int32_t nsos_check_ray_call(const NsosRayCall& c, bool bound_rays, bool mode_ok) {
    NSOS_REQUIRE(c.packed && c.rays_o && c.rays_d && c.viewdirs && c.z_vals && c.raw, NSOS_ERR_NULL_POINTER);
    NSOS_REQUIRE(c.n_rays > 0 && c.n_samples >= 1, NSOS_ERR_BAD_SHAPE);
    NSOS_REQUIRE(!bound_rays || c.n_rays < (1ll << 31), NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(mode_ok, NSOS_ERR_UNSUPPORTED);
    NSOS_REQUIRE(nsos_aligned16({c.packed, c.raw}), NSOS_ERR_MISALIGNED);
    return NSOS_OK;
}
// n_pts and n_tiles of any *Params (the kernels count tiles with 32 bits), ...
template <class P>
int32_t nsos_fill_points(P& p, long long n_pts, int tile_pts) {
    const long long n_tiles = (n_pts + tile_pts - 1) / tile_pts;
    NSOS_REQUIRE(n_tiles < (1ll << 31), NSOS_ERR_UNSUPPORTED);
    p.n_pts = n_pts;
    p.n_tiles = (int)n_tiles;
    return NSOS_OK;
}
// ... and the ray fields MlpParams, LpParams, X3Params and X316Params have in common
template <class P>
int32_t nsos_fill_ray_call(P& p, const NsosRayCall& c, int tile_pts) {
    p.rays_o = c.rays_o; p.rays_d = c.rays_d; p.viewdirs = c.viewdirs; p.z_vals = c.z_vals;
    p.raw = c.raw; p.n_samples = c.n_samples;
    return nsos_fill_points(p, (long long)c.n_rays * c.n_samples, tile_pts);
}
