/* nerf_sos_hip.h -- C ABI of the MI355X (gfx950) NeRF-SOS volumetric-rendering path.
 *
 * The reference (VITA-Group/NeRF-SOS) is 100 % Python and has no FFI/plugin interface: its
 * boundary for this path is the nn.Module duck-type NeRFNet.forward()/render_rays()
 * (models/nerf_net.py:71-195).  `nerf-sos_amd/` mirrors that module in Python; THIS header is
 * what it binds underneath (ctypes), one entry point per fusion group of SURVEY.md section 2.3.
 * Each function cites the reference lines whose arithmetic it replaces.
 *
 * Conventions (all functions):
 *   - every pointer is a DEVICE pointer to fp32 (or int64 where stated), row-major, dense;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only enqueue
 *     work: they never synchronise, never allocate, never free, never touch host copies of
 *     the data; the caller owns all buffers and keeps them alive until the stream drains;
 *   - return value: NSOS_OK (0), a negative NSOS_ERR_* validation code, or a positive
 *     hipError_t from the launch;
 *   - stateless and re-entrant; thread-safe as far as the HIP runtime is.
 *   - there is NO CPU fallback: without a gfx950 device every launch returns a hipError_t.
 */
#ifndef NERF_SOS_HIP_H
#define NERF_SOS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped whenever an existing entry point's arguments or buffer formats change (2: 16-bit / tile-major saved operands of
 * nsos_mlp_forward_rays_save16_lp and nsos_sem_head_wgrad_x3; 3: pose_rows in nsos_patch_batch / nsos_pixel_batch; 4: the tile-major
 * sem_hid16 of the default 16-bit kernel, nsos_mlp_save16_layout's NSOS_SEM_HID_TILED bit; 6: `scale` of nsos_mlp_input_grads_x3[_a16]
 * is three floats -- trunk scale, colour-branch factor, semantic-branch factor; 7: the generic kernels' packed program gained a field
 * (GenOp::ksplit_off: an older binding's buffer sizes still agree, but the two sides must match) + nsos_wgrad_batch; 9: evaluation metrics
 * nsos_ssim, nsos_adjusted_rand, nsos_kmeans; 10: the DINO ViT-S/16 feature extractor nsos_dino_*;
 * 11: the 16-bit packed weights hold two streams instead of three -- nsos_mlp_packed_bytes_lp -- and nsos_mlp_lp_select_kernel /
 * NSOS_LP_KERNEL refuse the retired kernel 2).  The folded fp32 stream
 * (nsos_mlp_pack_fold / nsos_mlp_*_fold) only ADDS entry points -- no existing argument list or buffer format moved, so the version
 * stands; a library without them fails to bind (every declared symbol is resolved at load) and reports another source hash.  The same
 * holds for LPIPS (nsos_lpips_*): four new entry points, nothing existing moved -- for the camera layer (nsos_camera_*): three -- and for
 * DINO's backward to the input (nsos_dino_forward_save, nsos_dino_backward and their four size / pack functions). */
#define NSOS_ABI_VERSION 11

enum {
    NSOS_OK = 0,
    NSOS_ERR_NULL_POINTER = -1,   /* a required pointer argument is NULL */
    NSOS_ERR_BAD_SHAPE = -2,      /* negative / zero / inconsistent sizes */
    NSOS_ERR_UNSUPPORTED = -3,    /* shape outside what the kernels are specialised for */
    NSOS_ERR_BUFFER_TOO_SMALL = -4,
    NSOS_ERR_MISALIGNED = -5      /* a pointer that must be 16-byte aligned is not */
};

/* Fixed architecture of every shipped config (configs/ (all 34): N_samples 64, N_importance 128,
 * use_viewdirs; run_nerf.py:96-101 defaults netdepth 8 / netwidth 256; models/nerf_net.py:44 skips=[4];
 * run_nerf.py:109-112 multires 10 / multires_views 4). */
#define NSOS_NET_DEPTH 8
#define NSOS_NET_WIDTH 256
#define NSOS_XYZ_FREQS 10
#define NSOS_DIR_FREQS 4
#define NSOS_XYZ_DIM 63 /* 3 + 6*10 */
#define NSOS_DIR_DIM 27 /* 3 + 6*4  */

/* Semantic-head variants (models/nerf_mlp.py:53-64; run_nerf.py:180-190). */
enum { NSOS_SEM_NONE = 0, NSOS_SEM_PLAIN = 1, NSOS_SEM_COORD = 2 };

/* The tensors of ONE NeRFMLP.mlp in PyTorch nn.Linear layout ([out,in] row-major fp32, device
 * memory): exactly the state-dict entries `<net>.mlp.*` (models/nerf_mlp.py:40-64). */
typedef struct nsos_mlp_tensors {
    const float* pts_w[NSOS_NET_DEPTH]; /* pts_linears.i.weight: [256,63] [256,256]x4 [256,319] [256,256]x2 */
    const float* pts_b[NSOS_NET_DEPTH]; /* pts_linears.i.bias  : [256] */
    const float* alpha_w;               /* alpha_linear.weight  [1,256]   */
    const float* alpha_b;               /* alpha_linear.bias    [1]       */
    const float* feature_w;             /* feature_linear.weight[256,256] */
    const float* feature_b;             /* feature_linear.bias  [256]     */
    const float* views_w;               /* views_linears.0.weight [128,283] */
    const float* views_b;               /* views_linears.0.bias   [128]     */
    const float* rgb_w;                 /* rgb_linear.weight    [3,128]   */
    const float* rgb_b;                 /* rgb_linear.bias      [3]       */
    const float* sem0_w;                /* semantic_linear.0.weight [128,319] (COORD) / [128,256] (PLAIN) / NULL */
    const float* sem0_b;                /* semantic_linear.0.bias   [128] */
    const float* sem2_w;                /* semantic_linear.2.weight [2,128]   */
    const float* sem2_b;                /* semantic_linear.2.bias   [2]       */
} nsos_mlp_tensors;

int32_t nsos_abi_version(void);
/* First 16 hex digits of the sha256 over the kernel sources and headers under csrc, this header and the compiler flags the library was built
 * from ("unstamped" for a hand-run make): lets a CPU-only check refuse a stale binary (tests/test_abi.py). */
const char* nsos_source_hash(void);
const char* nsos_error_string(int32_t code);

/* ---- weight packing ---------------------------------------------------------------------
 * The fused MLP kernel streams its weights through LDS as 32 KiB chunks of MFMA A-operands in
 * issue order (DESIGN.md "HBM layout").  nsos_mlp_pack gathers one net's tensors into that
 * stream (call again whenever a parameter changes).  `packed` must be 16-byte aligned and hold
 * nsos_mlp_packed_bytes(sem_mode) bytes.  Replaces nothing in the reference: nn.Linear keeps
 * [out,in] tensors (models/nerf_mlp.py:40-64) and ATen re-reads them per addmm. */
size_t nsos_mlp_packed_bytes(int32_t sem_mode);
int32_t nsos_mlp_pack(const nsos_mlp_tensors* tensors, int32_t sem_mode, void* packed, size_t packed_bytes,
                      void* stream);
/* The FOLDED stream.  feature_linear has no activation behind it (models/nerf_mlp.py:86-90) and its only consumer is
 * views_linears.0, so W' = W_v[:, :256] W_f [128,256] and b' = W_v[:, :256] b_f + b_v depend on the weights alone, and
 *   relu(views_linears.0(cat([feature_linear(h7), d27]))) = relu(W' h7 + W_v[:, 256:] d27 + b').
 * nsos_mlp_pack_fold forms W' and b' on the device (one small kernel in front of the pack kernel, stream-ordered, no allocation,
 * no host synchronisation: capturable) -- fp64 accumulation in the fixed order j = 0..255, separate multiply and add, ONE
 * rounding to fp32 -- into a scratch region at the end of `packed` (float offset nsos_mlp_packed_bytes(sem_mode) / 4:
 * [W' | W_v[:, 256:]] as [128,283] row-major, then b' [128]) and packs the view layer from there; the eight feature_linear
 * chunks move to the END of the stream, where only the full-backward variant (which stores the feature vector) reads them.
 * `packed` holds nsos_mlp_packed_bytes_fold(sem_mode) bytes and is consumed ONLY by the nsos_mlp_*_fold entries below, which
 * take the arguments of their namesakes.  sigma, the semantic logits and every saved block except NSOS_ACTS_VIEWS are
 * bit-identical to the unfolded kernels'; rgb differs by rounding (one 256-term chain instead of two), 11 % fewer MFMAs. */
size_t nsos_mlp_packed_bytes_fold(int32_t sem_mode);
int32_t nsos_mlp_pack_fold(const nsos_mlp_tensors* tensors, int32_t sem_mode, void* packed, size_t packed_bytes,
                           void* stream);

/* ---- K2-G: the MLP for any architecture the reference's constructors accept (csrc/mlp_generic.hip) -------------------------
 * nn.Linear tensors ([out,in] row-major fp32, device memory) of ONE NeRFMLP.mlp, described as the reference builds it
 * (models/nerf_mlp.py:40-64; NeRFMLP.__init__ :136-166): depth D, width W, the skip set as a bit mask (bit i: "i in skips", the
 * output of pts_linears.i is concatenated with input_pts, :73-74), multires / multires_views (xyz_freqs / dir_freqs; -1 = no
 * embedding: the raw 3-vector), use_viewdirs (0: output_linear only, :97-98), the semantic head as its Linear modules in order
 * (sem_layers of them: 2 for sem_layer <= 2, sem_layer otherwise, :58-63; ReLU between them), sem_with_coord (cat([h,
 * input_pts]), :79), sem_with_geo (geo[0..1] = geo_map_sem's two Linears on alpha; semantics *= mapping, :60,:81-83).
 * Exact-fp32 MFMA arithmetic: every Linear is an fmaf chain over its inputs in k order starting from the bias (the accumulators'
 * initial value) -- EXCEPT single-tile output ops (alpha 1 row, rgb 3, output_linear 4, the last Linear of the semantic chain), whose
 * K range is split into n_waves (4 or 8, chosen from the architecture's LDS footprint: two workgroups per CU -> 4, one -> 8) partial
 * chains that wave 0 adds in a fixed order: the same Linear therefore rounds differently under different architectures (always
 * deterministic; every case is held to the reference goldens at 1e-4, tests/test_generic_arch.py, re-validated after the change of
 * the reduction order in round 5).  Wave-wide sums / scans of the compositing, loss and eval kernels are DPP / permlane trees in a
 * fixed association (csrc/common.h nsos_wave_sum, nsos_wave_excl_scan).  Training: the K7-G entries below.
 * raw: [n, 4 + sem_dim] (4 without view directions).
 * The shipped architecture (8 x 256, skips {4}, 10 / 4 octaves, view directions, two-Linear head) should use nsos_mlp_forward_*:
 * this path is ~2x slower there.  Limits: depth <= 16, sem_layers <= 8, sem_dim <= 8, and the per-tile
 * activation buffers (ceil(W / 32) * 32 rows each) within 160 KiB of LDS: 32-point tiles up to W = 576 (384 with a deep semantic
 * head), 16-point tiles (half the matrix rate; chosen automatically) up to W = 800; NSOS_ERR_UNSUPPORTED otherwise. */
#define NSOS_GENERIC_MAX_DEPTH 16
#define NSOS_GENERIC_MAX_SEM 8
typedef struct nsos_generic_linear {
    const float* weight;   /* [out_dim, in_dim] */
    const float* bias;     /* [out_dim] */
    int32_t out_dim, in_dim;
} nsos_generic_linear;
typedef struct nsos_generic_mlp {
    int32_t depth, width, skip_mask;
    int32_t xyz_freqs, dir_freqs;              /* octaves; -1: use_embed = False */
    int32_t use_viewdirs, use_semantics, sem_dim, sem_with_coord, sem_with_geo, sem_layers;
    nsos_generic_linear pts[NSOS_GENERIC_MAX_DEPTH];
    nsos_generic_linear alpha, feature, views, rgb;   /* use_viewdirs */
    nsos_generic_linear output;                        /* !use_viewdirs */
    nsos_generic_linear sem[NSOS_GENERIC_MAX_SEM];
    nsos_generic_linear geo[2];
} nsos_generic_mlp;
size_t nsos_mlp_generic_packed_bytes(const nsos_generic_mlp* mlp);      /* 0: unsupported description */
int32_t nsos_mlp_generic_out_channels(const nsos_generic_mlp* mlp);    /* 0: unsupported description */
int32_t nsos_mlp_generic_pack(const nsos_generic_mlp* mlp, void* packed, size_t packed_bytes, void* stream);
/* Weights only, into a buffer nsos_mlp_generic_pack filled before for the same architecture (the program at its head depends on the
 * architecture alone): kernels only -- no host-to-device copy, so a training step that re-packs can be captured in a HIP graph. */
int32_t nsos_mlp_generic_repack(const nsos_generic_mlp* mlp, void* packed, size_t packed_bytes, void* stream);
/* `mlp` must describe the same architecture `packed` was packed for (its tensor pointers are not read here). */
int32_t nsos_mlp_generic_forward_rays(const nsos_generic_mlp* mlp, const void* packed, const float* rays_o, const float* rays_d,
                                      const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                      float* raw, void* stream);
int32_t nsos_mlp_generic_forward_points(const nsos_generic_mlp* mlp, const void* packed, const float* pts, const float* dirs,
                                        int64_t n_pts, float* raw, void* stream);

/* ---- K7-G: training a generic-architecture net (every parameter; autograd of models/nerf_mlp.py:67-100 over the points of a ray
 * batch, the model the reference trains in engines/trainer.py:201-203 when its constructor arguments are not the shipped ones).
 *   forward_rays_save  = forward_rays + `acts` [n_rays * n_samples, ld]: per point the two encodings and every Linear's
 *                        post-activation output, each in a column block padded to 32 with zeros (ld and the blocks: save_layout),
 *                        and behind the blocks (ABI 7) the ReLU patterns as BITS: one 32-bit word per output tile of every ReLU
 *                        Linear, in program order (bit r + 16 h = [feature 32 t + (r & 3) + 8 (r >> 2) + 4 h of tile t > 0]); the row
 *                        is padded to a multiple of 4 floats.  The chain reads its masks from these words, never from the blocks.
 *   pack_bwd           the transposed weight streams + the reversed program, into nsos_mlp_generic_bwd_packed_bytes(mlp) bytes
 *                        (re-pack whenever a weight changed, like nsos_mlp_generic_pack).
 *   input_grads        one kernel: g_raw [n_pts, out_channels] (d loss / d raw, e.g. from nsos_composite_backward) -> `gbuf`
 *                        [n_pts, ld]: every Linear's pre-activation gradient in its column block (ReLU masks from `acts`' bit words).
 *   save_layout        table[0] = ld, table[1] = number of Linear ops, then NSOS_GENERIC_LAYOUT_STRIDE ints per op in forward order:
 *                        position of the Linear in nsos_generic_mlp (pts 0..15, alpha 16, feature 17, views 18, rgb 19, output 20,
 *                        sem 21..28, geo 29..30), its column block, out_dim, number of input segments, then per segment (3 slots)
 *                        {column block of the segment's rows in `acts`, rows, first column of the Linear's weight they multiply}.
 *                        Returns the number of ints written.  dW = gbuf[:, block]^T acts[:, segment block] and db = column sums of
 *                        gbuf[:, block] are nsos_wgrad calls (M, N in 32-multiples: the blocks' zero padding makes them exact).
 *   input_grads != 0 at pack time: the chain also carries the gradient into the two positional encodings, and
 *   input_grads_rays   (same kernel) writes d loss / d point [n_pts, 3] and / d view direction [n_pts, 3] (NULL without view
 *                        directions) through them (autograd of models/embedder.py:34-48); nsos_ray_grad_reduce folds them back onto
 *                        the rays: pts = o + d z (models/sampler.py:70,166), viewdirs = d / |d| (models/nerf_net.py:160-163) and the
 *                        renderer's dists * |d| (models/renderer.py:41; from the compositing's own d loss / d sigma in `g_raw` and
 *                        `raw`, + noise * noise_std as the forward added it) -> g_rays_o, g_rays_d [n_rays, 3].
 * Exact-fp32 MFMA like the forward. */
#define NSOS_GENERIC_LAYOUT_STRIDE 13
int32_t nsos_mlp_generic_save_layout(const nsos_generic_mlp* mlp, int32_t* table, int32_t capacity);
int32_t nsos_mlp_generic_forward_rays_save(const nsos_generic_mlp* mlp, const void* packed, const float* rays_o, const float* rays_d,
                                           const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                           float* raw, float* acts, void* stream);
/* forward_rays_save for a trainable subset (the mask of nsos_mlp_generic_pack_bwd_subset, bit 31 included): only the blocks that subset's
 * backward reads are stored (the inputs of the trainable Linears, the factors of semantics * mapping) + the bit words, always; the other
 * columns of `acts` stay unwritten.  trainable = 1u << 31 (pose refinement against a frozen net): the bit words alone. */
int32_t nsos_mlp_generic_forward_rays_save_subset(const nsos_generic_mlp* mlp, const void* packed, const float* rays_o, const float* rays_d,
                                                  const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                                  float* raw, float* acts, uint32_t trainable, void* stream);
size_t nsos_mlp_generic_bwd_packed_bytes(const nsos_generic_mlp* mlp, int32_t input_grads);   /* 0: unsupported description */
int32_t nsos_mlp_generic_pack_bwd(const nsos_generic_mlp* mlp, void* packed_bwd, size_t packed_bytes, int32_t input_grads, void* stream);
/* The chain for a SUBSET of trainable Linears (bit p of `trainable` = position p of the Linear in nsos_generic_mlp, as in save_layout):
 * only the pre-activation gradients of those Linears and of everything downstream of them are formed -- with a frozen backbone (the
 * shipped recipe, run_nerf.py:307-318) the chain stops at the semantic head.  gbuf blocks of the other Linears are left unwritten.
 * with_header = 0: weights only, as nsos_mlp_generic_repack (same subset as the pack that wrote the header).
 * Bit 31 of `trainable` (ABI 7): the program ALSO carries the gradient into the encodings (as input_grads != 0 of nsos_mlp_generic_pack_bwd;
 * packed_bytes of nsos_mlp_generic_bwd_packed_bytes(mlp, 1)): every gradient of the chain is formed, and only the trainable Linears'
 * are written to gbuf -- a frozen net's chain (trainable = 1u << 31) touches neither the activation blocks nor gbuf. */
int32_t nsos_mlp_generic_pack_bwd_subset(const nsos_generic_mlp* mlp, void* packed_bwd, size_t packed_bytes, uint32_t trainable,
                                         int32_t with_header, void* stream);
int32_t nsos_mlp_generic_repack_bwd(const nsos_generic_mlp* mlp, void* packed_bwd, size_t packed_bytes, int32_t input_grads, void* stream);  /* as nsos_mlp_generic_repack */
int32_t nsos_mlp_generic_input_grads(const nsos_generic_mlp* mlp, const void* packed_bwd, const float* g_raw, const float* acts,
                                     float* gbuf, int64_t n_pts, void* stream);
int32_t nsos_mlp_generic_input_grads_rays(const nsos_generic_mlp* mlp, const void* packed_bwd, const float* g_raw, const float* acts,
                                          float* gbuf, const float* rays_o, const float* rays_d, const float* viewdirs,
                                          const float* z_vals, int64_t n_rays, int32_t n_samples, float* g_pts, float* g_dirs,
                                          void* stream);
/* The same two kernels for the point-query entry (NeRFMLP.forward, models/nerf_mlp.py:179-215) and for MLP.forward's own input, the
 * PRE-ENCODED row [n, input_ch + input_ch_views] (models/nerf_mlp.py:67-68; `encoded` non-NULL: pts / dirs are not read, encodings
 * are taken as given), with saved activations (acts may be NULL: inference) -- and their input gradients (packed with input_grads):
 * d loss / d point and / d direction through the encodings, or (g_encoded non-NULL) d loss / d the encoded inputs themselves. */
int32_t nsos_mlp_generic_forward_points_save(const nsos_generic_mlp* mlp, const void* packed, const float* pts, const float* dirs,
                                             const float* encoded, int64_t n_pts, float* raw, float* acts, void* stream);
int32_t nsos_mlp_generic_input_grads_points(const nsos_generic_mlp* mlp, const void* packed_bwd, const float* g_raw, const float* acts,
                                            float* gbuf, const float* pts, const float* dirs, int64_t n_pts, float* g_pts,
                                            float* g_dirs, float* g_encoded, void* stream);
int32_t nsos_ray_grad_reduce(const float* g_pts, const float* g_dirs, const float* z_vals, const float* rays_d, const float* raw,
                             const float* g_raw, const float* noise, float noise_std, int64_t n_rays, int32_t n_samples,
                             int32_t n_ch, float* g_rays_o, float* g_rays_d, void* stream);

/* ---- K0: pinhole ray generation (SURVEY.md section 8f "next", rank 1) ------------------------------------
 * get_persp_rays (utils/ray.py:12-22; callers data/gen_dataset.py:189,202) for the pixels
 * [pix_begin, pix_end) of an H x W image in row-major order (pixel = j*W + i):
 *   dirs = [(i-cx)/fx, -(j-cy)/fy, -1];  rays_d = dirs @ c2w[:3,:3]^T (unnormalised);  rays_o = c2w[:3,3].
 * c2w_host: HOST pointer to the 12 floats of c2w[:3,:4] row-major (poses are tiny and live on the host);
 * rays_o, rays_d out: device [pix_end-pix_begin, 3].  Removes the [N,H,W,2,3] ray tensors from disk / PCIe. */
int32_t nsos_generate_rays(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* c2w_host,
                           int64_t pix_begin, int64_t pix_end, float* rays_o, float* rays_d, void* stream);

/* ---- training-batch assembly on the device ---------------------------------
 * The scene's images (rgbs [n_images,H,W,rgb_ch] fp32), masks ([n_images,H,W,*]: `mask_words` 4-byte words per pixel --
 * int64 labels after the reference's thresholding, data/datasets.py:66-69, are 2 words per channel, float masks 1) and
 * poses ([n_images,pose_rows,pose_cols] fp32 exactly as poses_<split>.npy holds them: LLFF [3,5], blender / toydesk / tankstemple
 * [4,4], data/gen_dataset.py:228-233; rays use [:3,:4]) stay resident in device memory; a batch is gathered per
 * step, with the rays generated from the poses by K0's arithmetic (bit-identical to the reference's stored ray files).
 * Any of (rays_o+rays_d), target, masks_out may be NULL (that output is skipped).
 *
 * nsos_patch_batch: PatchNeRFDataset.__getitem__ (data/datasets.py:240-254) for n_patches items + PatchBatchCollater
 *   (data/collater.py:31-61).  Item b = (image, h_idx, w_idx) = sel[3b..3b+2] -- the caller draws the origins (the reference
 *   uses Python's random.randint(0, H - crop_size), crop_size = patch*stride) and passes them EITHER as a HOST array
 *   (sel_host: validated, travels in the kernel arguments, no copy) OR as a DEVICE array (sel_dev: out-of-range values are
 *   clamped; for captured graphs).  Output pixel (a, c) of item b is image pixel (h_idx + a*stride, w_idx + c*stride):
 *   rays_o / rays_d [n_patches, patch*patch, 3], target [n_patches, patch*patch, rgb_ch], masks_out [.., mask_words words],
 *   poses_out [n_patches, pose_rows, pose_cols] (the items' poses, :251) and start_out [n_patches, 2] = (h_idx, w_idx) as floats
 *   (:252); both optional.
 * nsos_pixel_batch: the same records for an explicit device list of flat pixel indices pix[k] = (image*H + y)*W + x:
 *   RayNeRFDataset items + RayBatchCollater (data/datasets.py:149-171, data/collater.py:7-29) and ViewNeRFDataset's
 *   np.random.choice pixels of one view + ViewBatchCollater (data/datasets.py:279-300, data/collater.py:63-84). */
int32_t nsos_patch_batch(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* poses,
                         int32_t pose_rows, int32_t pose_cols, int32_t n_images, const float* rgbs, int32_t rgb_ch, const void* masks,
                         int32_t mask_words, const int32_t* sel_host, const int32_t* sel_dev, int32_t n_patches,
                         int32_t patch, int32_t stride, float* rays_o, float* rays_d, float* target, void* masks_out,
                         float* poses_out, float* start_out, void* stream);
int32_t nsos_pixel_batch(int32_t H, int32_t W, float fx, float fy, float cx, float cy, const float* poses,
                         int32_t pose_rows, int32_t pose_cols, int32_t n_images, const float* rgbs, int32_t rgb_ch, const void* masks,
                         int32_t mask_words, const int64_t* pix, int64_t n, float* rays_o, float* rays_d, float* target,
                         void* masks_out, void* stream);

/* ---- K1: ray set-up -----------------------------------------------------------------------
 * viewdirs = d/|d| (models/nerf_net.py:163-166) and the stratified depths z
 * (StratifiedSampler.forward, models/sampler.py:46-68): z = near(1-t)+far*t, t=linspace(0,1,S);
 * if t_rand != NULL (perturb > 0) jitter inside the mid-point intervals with t_rand [R,S].
 *   rays_d [R,3]; near, far [R]; z_vals out [R,S]; viewdirs out [R,3] (may be NULL). */
int32_t nsos_ray_setup(const float* rays_d, const float* near, const float* far, const float* t_rand,
                       int64_t n_rays, int32_t n_samples, float* z_vals, float* viewdirs, void* stream);

/* pts = o + d*z (models/sampler.py:70,166) -- only for callers that ask for `retpts`; the MLP
 * kernel forms the points on the fly and never reads this tensor.  pts out [R,S,3]. */
int32_t nsos_ray_points(const float* rays_o, const float* rays_d, const float* z_vals, int64_t n_rays,
                        int32_t n_samples, float* pts, void* stream);

/* ---- K2: positional encoding + MLP, fused ---------------------------------------------------
 * PositionEncoder.forward x2 (models/embedder.py:34-48), the encoder join (models/nerf_mlp.py:208),
 * MLP.forward (models/nerf_mlp.py:67-100) and the point-chunk loop (models/nerf_mlp.py:190-210)
 * for R*S points x = o + d*z of R rays, with the per-ray view direction broadcast
 * (models/nerf_net.py:94,111).  raw out [R,S,C], C = 4 (NSOS_SEM_NONE) or 6: [r,g,b,sigma,(sem0,sem1)]. */
int32_t nsos_mlp_forward_rays(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                              const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                              float* raw, void* stream);

/* Same network on explicit points, the NeRFMLP.__call__(pts, viewdirs) form used by density
 * export (engines/eval.py:297; models/nerf_mlp.py:179-215).  pts, dirs [P,3]; raw out [P,C]. */
int32_t nsos_mlp_forward_points(const void* packed, int32_t sem_mode, const float* pts, const float* dirs,
                                int64_t n_pts, float* raw, void* stream);
/* The same two on the folded stream of nsos_mlp_pack_fold. */
int32_t nsos_mlp_forward_rays_fold(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                   const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                   float* raw, void* stream);
int32_t nsos_mlp_forward_points_fold(const void* packed, int32_t sem_mode, const float* pts, const float* dirs,
                                     int64_t n_pts, float* raw, void* stream);

/* ---- K5: training with a frozen backbone (run_nerf.py:307-318, --fix_backbone) -------------------------------
 * nsos_mlp_forward_rays_save = nsos_mlp_forward_rays that also stores, per point, what the semantic head's
 * backward needs: sem_in out [R*S,320] = [relu(h7) (256) | x63 (63) | 1.0] (the input of semantic_linear.0,
 * models/nerf_mlp.py:79-80, plus a ones column that turns the bias gradient into the same GEMM) and
 * sem_hid out [R*S,128] = relu(semantic_linear.0(...)).  sem_mode must be PLAIN or COORD.
 * nsos_sem_head_backward: the element-wise part of d(semantics)/d(semantic_linear.*) (models/renderer.py:64-66,
 * models/nerf_mlp.py:61): g_logits out [R*S,2] = weights * g_semantics[ray], g_hid out [R*S,128] =
 * (sem_hid > 0) * (g_logits @ semantic_linear.2.weight).  The weight gradients are then plain GEMMs of these
 * with sem_hid / sem_in (done by the host with the BLAS library). */
int32_t nsos_mlp_forward_rays_save(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                   const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                   float* raw, float* sem_in, float* sem_hid, void* stream);
int32_t nsos_mlp_forward_rays_save_fold(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                        const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                        float* raw, float* sem_in, float* sem_hid, void* stream);   /* folded stream; raw = nsos_mlp_forward_rays_fold's */
/* ---- K7: full backward (every parameter trainable) --------------------------------------------------
 * nsos_mlp_forward_rays_save_all = nsos_mlp_forward_rays that also stores every layer's activations, row-major
 * acts out [R*S, NSOS_ACTS_DIM] fp32, so that the backward is GEMMs + masks over saved data:
 *   [256 l, 256 l + 256)  relu(pts_linears.l(...)), l = 0..7        NSOS_ACTS_FEAT   feature_linear output (no activation)
 *   NSOS_ACTS_VIEWS  relu(views_linears.0(...)) [128]              NSOS_ACTS_SEM    relu(semantic_linear.0(...)) [128]
 *   NSOS_ACTS_X      encoded xyz [63] then 1.0                     NSOS_ACTS_D      encoded view direction [27], zero pad
 * (10.4 KB per point; training only).  Outputs are bit-identical to nsos_mlp_forward_rays. */
#define NSOS_ACTS_FEAT 2048
#define NSOS_ACTS_VIEWS 2304
#define NSOS_ACTS_SEM 2432
#define NSOS_ACTS_X 2560
#define NSOS_ACTS_D 2624
#define NSOS_ACTS_DIM 2656
int32_t nsos_mlp_forward_rays_save_all(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                       const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                       float* raw, float* acts, void* stream);
/* On the folded stream: raw bit-identical to nsos_mlp_forward_rays_fold; NSOS_ACTS_VIEWS comes from the folded chain,
 * NSOS_ACTS_FEAT is feature_linear(h7) as before (computed for storing only: it is an operand of views_linears.0's weight gradient). */
int32_t nsos_mlp_forward_rays_save_all_fold(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                            const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                            float* raw, float* acts, void* stream);
/* Building blocks of the full backward over saved activations (the input-gradient GEMMs g_in = g_out W are plain
 * [P,256]x[256,256] products and go through the BLAS library):
 * nsos_wgrad: dW [M, N] (row stride ldw) = sum_p G[p, 0:M]^T X[p, 0:N], db [M] = sum_p G[p, 0:M] (db may be NULL);
 *   G, X row-major with row strides ldg, ldx (slices of larger buffers); M, N in {32, 64, 128, 256}.  Exact-fp32 MFMA
 *   with K = points; deterministic.  workspace: nsos_wgrad_workspace_bytes().
 * nsos_relu_mask: g[p, c] = h[p, c] > 0 ? g[p, c] : 0 in place over n_cols (multiple of 4) columns. */
size_t nsos_wgrad_workspace_bytes(void);
int32_t nsos_wgrad(const float* G, int32_t ldg, const float* X, int32_t ldx, int64_t n_pts, int32_t M, int32_t N,
                   float* dW, int32_t ldw, float* db, void* workspace, size_t workspace_bytes, void* stream);
int32_t nsos_relu_mask(float* g, int32_t ldg, const float* h, int32_t ldh, int64_t n_pts, int32_t n_cols, void* stream);
/* nsos_wgrad_batch (ABI 7): a list of nsos_wgrad reductions over column blocks of ONE (G, X) pair -- all weight gradients of a
 * generic-architecture net (autograd of every Linear of models/nerf_mlp.py:40-64) in one call.  Item i: dW = out + w_off [M, N] with row
 * stride ldw = sum_p G[p, g_col : g_col + M]^T X[p, x_col : x_col + N], db = out + b_off [M] (b_off < 0: none); offsets in floats.  Items
 * run in list order and share the workspace; each is exactly one nsos_wgrad call (same numbers). */
typedef struct nsos_wgrad_item {
    int64_t w_off, b_off;
    int32_t g_col, x_col, M, N, ldw, reserved;
} nsos_wgrad_item;
int32_t nsos_wgrad_batch(const nsos_wgrad_item* items, int32_t n_items, const float* G, int32_t ldg, const float* X, int32_t ldx,
                         int64_t n_pts, float* out, void* workspace, size_t workspace_bytes, void* stream);
int32_t nsos_sem_head_backward(const float* weights, const float* g_semantics, const float* sem2_w,
                               const float* sem_hid, int64_t n_rays, int32_t n_samples, float* g_hid,
                               float* g_logits, void* stream);
/* The whole backward of the semantic head in one pass over the points (what NeRFNet uses): the element-wise part
 * above fused into the weight-gradient reductions, on the exact-fp32 MFMA.  Out: gw1_aug [128,320] =
 * [d semantic_linear.0.weight (first in_dim columns) | unused | d semantic_linear.0.bias (column 319)],
 * gw2 [2,128] = d semantic_linear.2.weight, gb2 [2] = d semantic_linear.2.bias.  g_hid / g_logits are never
 * materialised.  workspace: nsos_sem_head_wgrad_workspace_bytes() bytes.  Deterministic (block-ordered reduction).
 * gb1 != NULL (round 4): the first output is written as the CONTIGUOUS [128, in_dim] weight gradient instead (in_dim = 256 or
 * 319: semantic_linear.0's fan-in) and the bias gradient goes to gb1 [128] -- the tensors autograd takes, without slicing copies. */
size_t nsos_sem_head_wgrad_workspace_bytes(void);
int32_t nsos_sem_head_wgrad(const float* weights, const float* g_semantics, const float* sem2_w, const float* sem_hid,
                            const float* sem_in, int64_t n_rays, int32_t n_samples, float* gw1_aug, float* gw2,
                            float* gb2, void* workspace, size_t workspace_bytes, float* gb1, int32_t in_dim, void* stream);
/* The same on the 16-bit matrix pipe with split-fp16 operands (fp32 accumulate): HBM-bound instead of MFMA-bound.
 * g_hid = (g_logits @ W_sem2) * mask is brought into fp16 range by a power of two and gw1_aug divided by it again on
 * the way out: `scale` = that power of two as a device scalar, or NULL to have it derived on the device from
 * max |g_semantics| * max_m (|W_sem2[0,m]| + |W_sem2[1,m]|) (one extra small launch).  gw2 / gb2 are plain fp32 sums.
 * sem_in_dtype: NSOS_DTYPE_F32 for the fp32 matrix (three MFMAs per product), NSOS_DTYPE_F16 / NSOS_DTYPE_BF16 for the
 * compact 16-bit matrices of nsos_mlp_forward_rays_save16_lp -- sem_hid is then 16-bit [P,128] in the same format too, fp32
 * [P,128] otherwise -- (half the operand traffic; a 16-bit operand has no lo part:
 * two MFMAs per product on the format's own MFMA; csrc/sem_wgrad16.hip), optionally OR-ed with NSOS_SEM_IN_TILED (below) when
 * sem_in is in the tile-major layout.  n_samples >= 8, n_rays * n_samples < 2^31. */
int32_t nsos_sem_head_wgrad_x3(const float* weights, const float* g_semantics, const float* sem2_w, const void* sem_hid,
                               const void* sem_in, int32_t sem_in_dtype, int64_t n_rays, int32_t n_samples,
                               const float* scale, float* gw1_aug, float* gw2, float* gb2, void* workspace,
                               size_t workspace_bytes, float* gb1, int32_t in_dim, void* stream);

/* ---- K2-LP: the same fused network with 16-bit MFMA inputs and fp32 accumulation (reduced-precision configs) ----
 * For BASELINE configs C3 (bf16) and C5 (fp16, eval-only).  NOT bit/1e-4-comparable with the reference's fp32
 * arithmetic (fp16: ~1e-3 relative, bf16: ~1e-2); never used by the fp32 parity path.  Weights are packed to 16
 * bit by nsos_mlp_pack_lp into their own layout (nsos_mlp_packed_bytes_lp bytes): [the vector-ALU heads' block, 4 KiB | the
 * stream of mlp_lp_kernel, 37 / 39 / 40 chunks of 36 KiB for sem_mode 0 / 1 / 2 | the stream of mlp_lp16_kernel, 37 / 39 / 39
 * chunks of 36 KiB + 4 KiB].  raw out is fp32. */
enum { NSOS_DTYPE_F32 = 0, NSOS_DTYPE_F16 = 1, NSOS_DTYPE_BF16 = 2 };
size_t nsos_mlp_packed_bytes_lp(int32_t sem_mode);
int32_t nsos_mlp_pack_lp(const nsos_mlp_tensors* tensors, int32_t sem_mode, int32_t dtype, void* packed,
                         size_t packed_bytes, void* stream);
/* Re-pack only what depends on semantic_linear.* (the head's chunks of the SELECTED kernel's stream, with the vector-ALU heads'
 * block where that kernel reads it) into a buffer that already holds a full nsos_mlp_pack_lp of the same trunk: the shipped recipe
 * trains the semantic heads alone (run_nerf.py:307-318), so a training step re-packs 3 chunks instead of 37-40.  The other stream
 * keeps its old heads: a launch that takes it needs a full pack first.  sem_mode PLAIN / COORD only. */
int32_t nsos_mlp_pack_lp_heads(const nsos_mlp_tensors* tensors, int32_t sem_mode, int32_t dtype, void* packed,
                               size_t packed_bytes, void* stream);
int32_t nsos_mlp_forward_rays_lp(const void* packed, int32_t sem_mode, int32_t dtype, const float* rays_o,
                                 const float* rays_d, const float* viewdirs, const float* z_vals, int64_t n_rays,
                                 int32_t n_samples, float* raw, void* stream);
/* Training with a frozen backbone at reduced precision (config C3): as nsos_mlp_forward_rays_save, with sem_in
 * holding the 16-bit values the semantic head actually consumed (widened to fp32) and sem_hid its fp32 hidden
 * activations; nsos_sem_head_backward and the weight-gradient GEMMs are the same as for the fp32 path. */
int32_t nsos_mlp_forward_rays_save_lp(const void* packed, int32_t sem_mode, int32_t dtype, const float* rays_o,
                                      const float* rays_d, const float* viewdirs, const float* z_vals, int64_t n_rays,
                                      int32_t n_samples, float* raw, float* sem_in, float* sem_hid, void* stream);
/* The same with BOTH saved matrices kept in the 16-bit format `dtype`: sem_in16 [P,320] halves (640 B per point instead of
 * 1280: the values are 16-bit anyway) and sem_hid16 [P,128] halves (256 B instead of 512: relu of the fp32 accumulators,
 * rounded to nearest even -- the ReLU pattern is unchanged, the values feed only d semantic_linear.2.weight, at the
 * format's precision like everything else on this path).  896 B per point in all (round 2: 1152).
 * Consumer: nsos_sem_head_wgrad_x3 with the matching sem_in_dtype.
 * LAYOUT -- nsos_mlp_save16_layout(n_points) says what the call will write: NSOS_SEM_IN_ROWS (both matrices row-major: the
 * round-1 kernel) or NSOS_SEM_IN_TILED | NSOS_SEM_HID_TILED (both tile-major: the default kernel), or a negative NSOS_ERR_*.
 *   NSOS_SEM_IN_ROWS  (0):  [P, 320] row-major;
 *   NSOS_SEM_IN_TILED (16): tile-major, the layout the two-waves-per-SIMD kernel (the default) stores without touching 32
 *     different rows per instruction: groups of 32 consecutive points, [group][K 0..19][kg 0..1][point 0..31][8 channels] --
 *     channel 16 K + 8 kg + c of point 32 g + i is element ((g * 20 + K) * 64 + kg * 32 + i) * 8 + c.  The buffer must hold
 *     ceil(P / 32) * 32 rows of 320 elements; rows past P are not written.
 * OR the layout value into nsos_sem_head_wgrad_x3's sem_in_dtype.
 * sem_hid16: [P, 128] row-major, or -- NSOS_SEM_HID_TILED (32) set in the layout value: the 16x16x32 kernel, the default since
 * round 4 -- tile-major like sem_in: [group of 32 points][octet 0..15][point][8 channels] (8 KiB per group; rows past P of the
 * last group are never written): every store instruction of the kernel then writes four runs of 256 contiguous bytes instead of
 * 64 pieces of 16 bytes in as many 256-byte rows (partial-line writes are filled from memory first: the training variant's
 * excess read traffic of round 3). */
enum { NSOS_SEM_IN_ROWS = 0, NSOS_SEM_IN_TILED = 16, NSOS_SEM_HID_TILED = 32 };
int32_t nsos_mlp_save16_layout(int64_t n_points);
int32_t nsos_mlp_forward_rays_save16_lp(const void* packed, int32_t sem_mode, int32_t dtype, const float* rays_o,
                                        const float* rays_d, const float* viewdirs, const float* z_vals, int64_t n_rays,
                                        int32_t n_samples, float* raw, void* sem_in16, void* sem_hid16, void* stream);

/* ---- K2-X3: the same fused network on the 16-bit matrix pipe with SPLIT-fp16 operands (fp32-grade results) -------
 * Every weight and activation is carried as hi = fp16(v), lo = fp16(v - hi) and every product as the three MFMAs
 * hi.hi + hi.lo + lo.hi with fp32 accumulation (the weights' lo parts scaled by 2^11 so that they stay normal fp16
 * numbers): max / rms error against an fp64 evaluation equal to plain fp32 arithmetic's (~1e-7 .. 2e-6 max), i.e.
 * three orders of magnitude inside the 1e-4 parity tolerance, at ~2.8x the exact-fp32 kernel's speed.
 * Limits: |activation| must stay below 65504 (fp16 range).  Opt-in; inference and frozen-backbone training.
 * Weights are packed by nsos_mlp_pack_x3 into their own stream layout (nsos_mlp_packed_bytes_x3 bytes).
 * ABI 8 (round 6): the buffer holds TWO streams -- [aux | the 32x32x16 kernel's (csrc/mlp_x3.hip: training variants, backward
 * chain) | the 16x16x32 kernel's (csrc/mlp_x316.hip: inference; mlp_lp16's workgroup and chunk schedule, three MFMAs per product)];
 * nsos_mlp_pack_x3 writes both, nsos_mlp_forward_rays_x3 runs the selected one (default: 16x16x32).  The two kernels agree to the
 * split format's accuracy (other contraction order inside the MFMAs), not bit for bit. */
size_t nsos_mlp_packed_bytes_x3(int32_t sem_mode);
/* Diagnostics / A-B: 1 = mlp_x3_kernel (32x32x16, one wave per SIMD), 2 = mlp_x316_kernel (16x16x32, two waves per SIMD; default;
 * NSOS_X3_KERNEL=1|2 in the environment chooses at first use).  Applies to nsos_mlp_forward_rays_x3 / nsos_mlp_profile_rays_x3. */
int32_t nsos_mlp_x3_select_kernel(int32_t kernel);
int32_t nsos_mlp_x3_selected_kernel(void);
int32_t nsos_mlp_pack_x3(const nsos_mlp_tensors* tensors, int32_t sem_mode, void* packed, size_t packed_bytes,
                         void* stream);
int32_t nsos_mlp_forward_rays_x3(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                 const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                 float* raw, void* stream);
/* Training with a frozen backbone (--fix_backbone, run_nerf.py:307-318) on the split-fp16 kernel: as
 * nsos_mlp_forward_rays_save, with sem_in holding the fp32 values hi + lo the semantic head consumed and sem_hid its
 * fp32 hidden activations; the backward kernels are the fp32 path's.  sem_mode must be 1 or 2. */
int32_t nsos_mlp_forward_rays_save_x3(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                      const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                      float* raw, float* sem_in, float* sem_hid, void* stream);
/* Full training (every parameter trainable) on the split-fp16 kernel: as nsos_mlp_forward_rays_save_all, acts holding
 * the fp32 values hi + lo each layer handed to the next.  relu_masks (nsos_mlp_relu_masks_bytes_x3(n_pts) bytes, 16-byte
 * aligned) receives the ReLU patterns of the 8 trunk layers as bits in the kernel's own lane order (32 B per point per
 * layer instead of 1 KB of fp32 reads): the input of nsos_mlp_input_grads_x3. */
size_t nsos_mlp_relu_masks_bytes_x3(int64_t n_pts);
int32_t nsos_mlp_forward_rays_save_all_x3(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                          const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                          float* raw, float* acts, void* relu_masks, void* stream);
/* Full training with 16-bit saved activations (round 4): the same kernels with `acts` [P, NSOS_ACTS_DIM] stored as IEEE half floats
 * -- the hi parts of the split-fp16 activations as the MFMAs consumed them -- 5.3 KB per point instead of 10.6.  The chain reads
 * only the two 128-wide heads' ReLU patterns from it (the trunk's come as the forward's bit masks, which are required here); the
 * weight-gradient reductions take it as their X operand (ldx in ELEMENTS): exact widening, G stays fp32. */
int32_t nsos_mlp_forward_rays_save_all16_x3(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                            const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                            float* raw, void* acts_f16, void* relu_masks, void* stream);
int32_t nsos_mlp_input_grads_x3_a16(const void* packed, int32_t sem_mode, const float* g_raw, const void* acts_f16,
                                    const void* relu_masks, int64_t n_pts, const float* scale, float* gbuf, void* stream);
int32_t nsos_wgrad_xh(const float* G, int32_t ldg, const void* X_f16, int32_t ldx, int64_t n_pts, int32_t M, int32_t N, float* dW,
                      int32_t ldw, float* db, void* workspace, size_t workspace_bytes, void* stream);
int32_t nsos_wgrad_x3_xh(const float* G, int32_t ldg, const void* X_f16, int32_t ldx, int64_t n_pts, float* dW, int32_t ldw, float* db,
                         void* workspace, size_t workspace_bytes, void* stream);

/* nsos_wgrad for M = N = 256 on the 16-bit matrix pipe: both operands split on the fly into fp16 hi + lo, three MFMAs per
 * product, fp32 accumulation (K7-X3).  |G| and |X| must be within fp16 range (G from nsos_mlp_input_grads_x3 is, by its
 * scale); same workspace, same deterministic reduction as nsos_wgrad. */
int32_t nsos_wgrad_x3(const float* G, int32_t ldg, const float* X, int32_t ldx, int64_t n_pts, float* dW, int32_t ldw,
                      float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K7-X3: the input-gradient chain of the full backward as one fused split-fp16 kernel --------------------------
 * Replaces the library GEMMs g_in = g_out @ W and the ReLU-mask passes of the full backward (autograd of
 * models/nerf_mlp.py:67-100): from g_raw [P,C] (C = 4 or 6: d loss / d [r,g,b,sigma,(sem0,sem1)]) and the activations
 * acts [P,NSOS_ACTS_DIM] saved by nsos_mlp_forward_rays_save_all[_x3] it writes gbuf [P,NSOS_GBUF_DIM], the gradients
 * with respect to every layer's pre-activation in the column map of acts (256 l: pts_linears.l, NSOS_ACTS_FEAT:
 * feature_linear output, NSOS_ACTS_VIEWS: views_linears.0, NSOS_ACTS_SEM: semantic_linear.0), each the GEMM input of
 * nsos_wgrad.  `scale`: THREE powers of two in device memory, applied to g_raw on load -- scale[0] brings max |g_raw| over all
 * channels to ~2^4 (the trunk's columns 256 l of gbuf carry it); scale[1] >= 1 is the colour branch's extra factor (blocks
 * NSOS_ACTS_VIEWS and NSOS_ACTS_FEAT carry scale[0] scale[1]); scale[2] >= 1 the semantic branch's (block NSOS_ACTS_SEM carries
 * scale[0] scale[2]): a branch whose upstream gradient is decades under the largest one keeps fp16's full precision (ABI 6).  The
 * weight gradients must be divided by the scale their gbuf block carries.  relu_masks: the bit masks written by
 * nsos_mlp_forward_rays_save_all_x3 for the same points, or NULL to derive the trunk masks from acts (fp32 reads).
 * Weights are packed (transposed, split fp16) by
 * nsos_mlp_bwd_pack_x3 into nsos_mlp_bwd_packed_bytes_x3 bytes. */
#define NSOS_GBUF_DIM 2560
size_t nsos_mlp_bwd_packed_bytes_x3(int32_t sem_mode);
int32_t nsos_mlp_bwd_pack_x3(const nsos_mlp_tensors* tensors, int32_t sem_mode, void* packed, size_t packed_bytes,
                             void* stream);
int32_t nsos_mlp_input_grads_x3(const void* packed, int32_t sem_mode, const float* g_raw, const float* acts,
                                const void* relu_masks, int64_t n_pts, const float* scale, float* gbuf, void* stream);

/* Diagnostics: nsos_mlp_forward_rays plus per-phase shader-clock stamps (s_memtime) of the first tile of
 * workgroups 0..3: stamps out uint64 [16 waves][64 slots] (slot meaning: scripts/phase_profile.py).
 * Not on the product path; used to attribute the kernel's non-MFMA cycles (profiles/). */
int32_t nsos_mlp_profile_rays(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                              const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                              float* raw, uint64_t* stamps, void* stream);
/* ... of the folded kernel (slot 10, the feature_linear phase, is empty: stamped together with slot 9's end). */
int32_t nsos_mlp_profile_rays_fold(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                   const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                   float* raw, uint64_t* stamps, void* stream);
/* Same for the reduced-precision kernel; it stamps the SECOND tile of workgroups 0..3 (steady state), so give it
 * more than 2 x 256 x (CU count) points.  Slot meaning: scripts/phase_profile_lp.py. */
/* Diagnostics: stamp EVERY following 16-bit MLP launch (the training variants included) into `stamps` (layout of
 * nsos_mlp_profile_rays_lp), or stop with NULL.  scripts/phase_profile_lp.py --save. */
int32_t nsos_mlp_lp_set_stamp_buffer(uint64_t* stamps);

/* Diagnostics: which kernel serves the 16-bit entry points above.  3 (default) = mlp_lp16_kernel, two 256-register waves per
 * SIMD with 32 points each on 16x16x32 MFMAs (mlp_lp16.hip); 1 = mlp_lp_kernel, the round-1 kernel, one 512-register wave per
 * SIMD with 64 points on 32x32x16 (mlp_lp.hip).  Each reads its own stream of the packed weights; the two agree to the 16-bit
 * format's rounding.  Exists for A/B measurements (models/nerf_mlp.py:67-100 is what both replace).  Every other value -- 2, a
 * retired kernel, included -- is NSOS_ERR_UNSUPPORTED and leaves the selection as it was.  NSOS_LP_KERNEL=lp16|lp4 in the
 * environment sets the initial selection; with any other value nsos_mlp_lp_selected_kernel and the 16-bit pack, forward, save and
 * nsos_mlp_save16_layout calls return NSOS_ERR_UNSUPPORTED until a kernel is selected here.
 * Whatever is selected, the fp32 operands of nsos_mlp_forward_rays_save_lp and launches of 2^31 points or more run on kernel 1. */
int32_t nsos_mlp_lp_select_kernel(int32_t kernel);
int32_t nsos_mlp_lp_selected_kernel(void);   /* 3 = mlp_lp16_kernel (default), 1 = mlp_lp_kernel, or NSOS_ERR_UNSUPPORTED */

/* ... and for the split-fp16 kernel (128-point tiles: more than 2 x 128 x (CU count) points).  scripts/phase_profile_x3.py. */
int32_t nsos_mlp_profile_rays_x3(const void* packed, int32_t sem_mode, const float* rays_o, const float* rays_d,
                                 const float* viewdirs, const float* z_vals, int64_t n_rays, int32_t n_samples,
                                 float* raw, uint64_t* stamps, void* stream);
int32_t nsos_mlp_profile_rays_lp(const void* packed, int32_t sem_mode, int32_t dtype, const float* rays_o,
                                 const float* rays_d, const float* viewdirs, const float* z_vals, int64_t n_rays,
                                 int32_t n_samples, float* raw, uint64_t* stamps, void* stream);

/* ---- K3: compositing ------------------------------------------------------------------------
 * VolumetricRenderer.forward (models/renderer.py:35-85): sigma->alpha, exclusive transmittance
 * product, weights, and the weighted sums.  noise (may be NULL) is the raw randn [R,S]; it is
 * scaled by noise_std in-kernel (models/renderer.py:47).  n_ch = 4 or 6.
 *   weights out [R,S]; rgb out [R,3]; sem out [R,n_ch-4] (NULL iff n_ch == 4); depth/acc/disp out [R]. */
int32_t nsos_composite(const float* raw, const float* z_vals, const float* rays_d, const float* noise,
                       float noise_std, int64_t n_rays, int32_t n_samples, int32_t n_ch, int32_t white_bkgd,
                       float* weights, float* rgb, float* sem, float* depth, float* acc, float* disp,
                       void* stream);

/* Backward of nsos_composite w.r.t. raw (autograd of models/renderer.py:35-85; z_vals, rays_d and the noise carry no
 * gradient in the reference).  Upstream gradients g_rgb [R,3], g_sem [R,C-4], g_depth [R], g_acc [R], g_disp [R],
 * g_weights [R,S] may each be NULL (= zero).  g_raw out [R,S,C], C = 4 .. 12 (4 + sem_dim).  alpha / transmittance / weights
 * are recomputed. */
int32_t nsos_composite_backward(const float* raw, const float* z_vals, const float* rays_d, const float* noise,
                                float noise_std, int64_t n_rays, int32_t n_samples, int32_t n_ch, int32_t white_bkgd,
                                const float* g_rgb, const float* g_sem, const float* g_depth, const float* g_acc,
                                const float* g_disp, const float* g_weights, float* g_raw, void* stream);

/* nsos_composite on the coarse samples followed by nsos_importance_sample on its weights, in ONE launch (models/nerf_net.py:98-113:
 * renderer -> importance_sampler): same device code, bit-identical outputs, one launch and one round trip of the weights
 * less per step.  n_coarse in [2, 64]. */
int32_t nsos_composite_importance(const float* raw, const float* z_vals, const float* rays_d, const float* noise, float noise_std,
                                  int64_t n_rays, int32_t n_coarse, int32_t n_ch, int32_t white_bkgd, float* weights, float* rgb,
                                  float* sem, float* depth, float* acc, float* disp, const float* u, int32_t n_importance,
                                  float* z_fine, float* z_samples, float* z_std, void* stream);

/* Train-mode random tensors of one ray chunk in ONE launch (optional; NeRFNet.rng = "philox").  The reference draws, in this
 * order, rand[R,S] (stratified jitter, models/sampler.py:61), randn[R,S] (coarse sigma noise, models/renderer.py:47),
 * rand[R,N] (importance u, models/sampler.py:103), randn[R,S+N] (fine sigma noise) from torch's global generator: four
 * launches.  Here a counter-based Philox4x32-10 stream keyed by `seed`, advanced by `call` (one value per chunk / step),
 * fills whichever of the four buffers is not NULL: element e of the padded concatenation is word e & 3 of block e >> 2; a uniform is
 * (k + 0.5) 2^-23 over its word's top 23 bits (never 0 or 1), normals are Box-Muller pairs of two such uniforms.  NOT torch's values: the default path keeps torch's generator so that
 * the reference's captured draws can be injected (tests/golden/end_to_end.npz). */
int32_t nsos_render_draws(uint64_t seed, uint64_t call, int64_t n_rays, int32_t n_coarse, int32_t n_importance,
                          float* t_rand, float* noise0, float* u, float* noise1, void* stream);
/* The same draws with the call counter in DEVICE memory: uses call = *calls_so_far + 1 and then advances *calls_so_far by one
 * (a second, one-thread launch), so that a captured HIP graph of a training step draws fresh numbers on every replay -- and
 * the same numbers as eager calls of nsos_render_draws with call = 1, 2, 3, ... under the same seed. */
int32_t nsos_render_draws_counted(uint64_t seed, uint64_t* calls_so_far, int64_t n_rays, int32_t n_coarse, int32_t n_importance,
                                  float* t_rand, float* noise0, float* u, float* noise1, void* stream);

/* ---- K4: hierarchical sampling ----------------------------------------------------------------
 * ImportanceSampler.forward / sample_pdf (models/sampler.py:91-167) + z_std (models/nerf_net.py:124):
 * pdf over the inner 62 coarse weights, cdf (fp64-accumulated), right-bisect search of u,
 * lerp inside the bin, merge-sort with the coarse depths, population std of the new samples.
 *   z_vals, weights [R,S] (2 <= S <= 512; S <= 64 -- every shipped config uses 64 -- is the tuned one-sample-per-lane kernel); u [R,N] or NULL (= det: linspace(0,1,N), perturb == 0);
 *   cdf_in [R,S-1] or NULL: if given it REPLACES the computed cdf (stage-wise index pinning);
 *   outputs: z_fine [R,S+N] ascending; z_samples [R,N]; z_std [R];
 *   optional outputs (NULL to skip): cdf_out [R,S-1], inds_out int64 [R,N] (the searchsorted result). */
int32_t nsos_importance_sample(const float* z_vals, const float* weights, const float* u, const float* cdf_in,
                               int64_t n_rays, int32_t n_coarse, int32_t n_importance, float* z_fine,
                               float* z_samples, float* z_std, float* cdf_out, int64_t* inds_out, void* stream);

/* ---- evaluation post-processing ---------------------------------------------
 * What engines/eval.py:44-57,79-86 computes on the host after copying every output off the device:
 *   sem_prob = softmax(semantics, -1); sem_pred = argmax(sem_prob, -1)   (first maximal index, int32)
 *   metrics[0] = img2mse(rgb, target) (utils/image.py:125-128), metrics[1] = mse2psnr(.) (utils/image.py:134-137)
 * semantics [R,sem_dim] may be NULL (no semantic outputs); rgb/target [R,3] may be NULL (no metrics);
 * sem_prob [R,sem_dim] / sem_pred [R] may each be NULL.  workspace: nsos_eval_workspace_bytes() bytes, 8-byte
 * aligned, contents undefined on return except ws[0] = the fp64 sum of per-ray mean squared errors.
 * The reduction order is fixed (no atomics): results are bit-identical run to run. */
size_t nsos_eval_workspace_bytes(void);
int32_t nsos_eval_postprocess(const float* semantics, const float* rgb, const float* target, int64_t n_rays,
                              int32_t sem_dim, float* sem_prob, int32_t* sem_pred, float* metrics, void* workspace,
                              void* stream);

/* ---- evaluation metrics: SSIM, k-means clustering, adjusted Rand index ---------------------------------------------
 * The rest of engines/eval.py:31-93 (eval_one_view) and of the trainer's i_print block (engines/trainer.py:172-195) on the device.
 * Every reduction runs in a fixed order (no float atomics): results are bitwise identical from run to run.
 *
 * nsos_ssim: utils/ssim.py:17-38 (_ssim) as reached through utils/image.py:139-147.  img1, img2 [batch, channels, height, width]
 * (NCHW, dense).  window_size odd, 1..31: the gaussian of sigma 1.5 normalised in fp32 (utils/ssim.py:7-9), applied separably
 * (its outer product) with zero padding window_size/2 per channel; C1 = 0.01^2, C2 = 0.03^2; moments and map in fp64.
 * window: HOST pointer to the window_size fp32 weights of that 1-D window (the reference's torch expression, whose fp32 sum order is
 * torch's), or NULL: the same gaussian normalised by its fp64-accumulated sum rounded to fp32.
 * out: size_average != 0 -> out[0] = mean over batch*channels*height*width; else out[batch] = per-image means.  ssim_map
 * [batch,channels,height,width] may be NULL.  workspace: nsos_ssim_workspace_bytes(...) bytes, 8-byte aligned. */
size_t nsos_ssim_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width);
int32_t nsos_ssim(const float* img1, const float* img2, int64_t batch, int64_t channels, int64_t height, int64_t width,
                  int32_t window_size, const float* window, int32_t size_average, float* out, float* ssim_map, void* workspace,
                  size_t workspace_bytes, void* stream);

/* nsos_adjusted_rand: sklearn.metrics.adjusted_rand_score (1.x, pair-confusion form) of labels_true vs labels_pred [n], both of
 * element type `dtype` (NSOS_LABEL_*; bool travels as UINT8).  Labels must be integers in [0, 64).  out (double [2]):
 * out[0] = ARI over all n, out[1] = ARI over the positions where labels_true == subset_label (engines/eval.py:67-69 `fg_idx`),
 * both from one contingency table.  Pair counts are exact (int64 sums, 128-bit products) and divided once in fp64; no
 * disagreeing pairs (n <= 1, empty subset, one class on both sides) gives exactly 1.0.  Any label outside [0, 64) or not an
 * integer makes both results NaN; their count is left in workspace word 4096 (uint64).  workspace:
 * nsos_adjusted_rand_workspace_bytes() bytes, 8-byte aligned (the uint64 contingency table [64][64] + that count).  n <= 2^31. */
enum { NSOS_LABEL_INT32 = 0, NSOS_LABEL_INT64 = 1, NSOS_LABEL_UINT8 = 2, NSOS_LABEL_FLOAT32 = 3 };
size_t nsos_adjusted_rand_workspace_bytes(void);
int32_t nsos_adjusted_rand(const void* labels_true, const void* labels_pred, int64_t n, int32_t dtype, int32_t subset_label,
                           double* out, void* workspace, void* stream);

/* nsos_kmeans: sklearn 1.x KMeans(algorithm="lloyd", n_init=1) on `batch` independent problems x [batch, n_points, n_features]
 * (utils/misc.py:40-52 segmap_cluster).  n_features <= 16, n_clusters <= 16, n_points >= n_clusters.
 *   - init_centers [batch, n_clusters, n_features] or NULL: greedy k-means++ (sklearn _kmeans_plusplus) with n_local_trials
 *     candidates per round (0: 2 + floor(ln n_clusters)); each draw is the exponential race argmin_i -ln(u_i) / w_i (w = 1 for the
 *     first center, D^2 after; ties to the lowest index) over the counter-based stream
 *     s = mix(mix(mix(seed) ^ problem) ^ (round << 8 | trial)), u_i = ((mix(s ^ i) >> 40) + 1) / 2^24, mix = splitmix64's finaliser,
 *     problem = problem_base + b / problems_per_stream (1: a stream per problem; batch: one stream shared by all, as per-slice
 *     calls with one random_state draw).  The candidate of lowest potential (first on ties) is kept.
 *   - Lloyd steps: nearest center (ties to the lowest index), fp64 per-cluster sums; an empty cluster takes the point farthest from
 *     its assigned center (largest first, ties to the lowest index).  Stops when no label changed (strict convergence), when the
 *     squared center shift <= tol * mean(var(x, axis=0)), or after max_iter steps; without strict convergence one more assignment
 *     makes the labels agree with the returned centers.  max_iter = 0: seeding only (sklearn.cluster.kmeans_plusplus): the
 *     centers are the seeds in draw order, labels the nearest seed, n_iter 0.
 *   - labels int32 [batch, n_points] in canonical order: cluster r is the r-th center in ascending lexicographic order.  centers
 *     [batch, n_clusters, n_features], inertia double [batch], n_iter int32 [batch] may each be NULL.
 * mode 0: automatic (workgroup regime for n_points <= NSOS_KMEANS_WG_MAX_POINTS), 1: workgroup, 2: grid.
 *   workgroup regime: one launch; one workgroup per problem runs seeding and every step.  Never synchronises.
 *   grid regime: one seeding launch, then per step an assignment pass over all 1024-point chunks and a one-workgroup finish that
 *   sets the problem's done word (later launches return at once); the host reads an all-done word after every 8 steps, so this
 *   call synchronises `stream` ceil(n_iter / 8) times (at most ceil(max_iter / 8) - 1 times).  Both regimes run the same arithmetic
 *   in the same order: bitwise-equal results.
 * workspace: nsos_kmeans_workspace_bytes(...) bytes, 16-byte aligned. */
#define NSOS_KMEANS_WG_MAX_POINTS 65536
size_t nsos_kmeans_workspace_bytes(int64_t batch, int64_t n_points, int32_t n_features, int32_t n_clusters);
int32_t nsos_kmeans(const float* x, int64_t batch, int64_t n_points, int32_t n_features, int32_t n_clusters, const float* init_centers,
                    uint64_t seed, int64_t problem_base, int64_t problems_per_stream, int32_t n_local_trials, int32_t max_iter, double tol, int32_t mode,
                    int32_t* labels, float* centers, double* inertia, int32_t* n_iter, void* workspace, size_t workspace_bytes,
                    void* stream);

/* Row-partitioned GeoCorrelationLoss for the ray/patch-sharded multi-GPU step (utils/image.py:448-487; call site
 * engines/trainer.py:159-160): every rank holds the WHOLE batch's depth / code / rays (sharding.all_gather_patches) but
 * evaluates the O(P^4) pair sets only for ITS OWN row patches `rows[0..n_rows)` (device int32, global patch ids).  The patches
 * are coupled through four global sums (mean(fd), mean(fd1) per pair set, utils/image.py:316-319) and through the gradient a
 * patch receives as the NEGATIVE of another rank's patch, so the call is split into phases with TWO sum-all-reduces in between:
 *   phase 0: prep + pass 1 + the row-mean residual of the own rows   -> all-reduce means[0..3]  (4 doubles)
 *   phase 1: passes 3, 4 + role sums of the gradient + the loss sums -> all-reduce sums (fp32: batch * n_points * 4 role sums, then the
 *            two loss sums as three fp32 terms each -- an exact split of the rank's fp64 partial -- + 2 spare: nsos_corr_exchange_floats)
 *   phase 2: loss (the batch-wide value, identical on every rank) and grad_code [B,C,H,W] for every patch.
 *   phase 3: phases 0..2 in one call, for a single process (nothing to reduce in between): fewer, merged finishing launches.
 * `means` / `sums` are the workspace's own slots (offsets from nsos_corr_workspace_slots; the workspace is
 * nsos_corr_workspace_bytes(1, ...)) unless exchange_means (8 doubles, 8-byte aligned; all 8 may be reduced) / exchange_sums
 * (nsos_corr_exchange_floats(batch, n_points) floats) are given: a training step hands every loss evaluation of the step a slice
 * of ONE buffer per reduction and issues one all-reduce per phase for all of them (sharding._losses_direct).
 * With rows = all patches and no reductions the phases equal nsos_geo_correlation_loss up to summation order (the loss sums'
 * split is exact; summed over ranks it carries fp32 rounding of each term, <= 1e-7 of the fp32 loss value). */
int64_t nsos_corr_exchange_floats(int32_t batch, int32_t n_points);
int32_t nsos_corr_workspace_slots(int32_t batch, int32_t n_points, int64_t* scal_offset_bytes, int64_t* gsum_offset_bytes,
                                  int64_t* gsum_floats);
int32_t nsos_geo_correlation_loss_rows(int32_t phase, float* depth, const float* code, const float* ray_o, const float* ray_d,
                                       const int64_t* neg_indx, const int32_t* rows, int32_t n_rows, int32_t batch,
                                       int32_t code_dim, int32_t height, int32_t width, float self_shift, float self_weight,
                                       float neg_shift, float neg_weight, float max_depth, int32_t filter_in_place, float* loss,
                                       float* grad_code, void* workspace, size_t workspace_bytes, double* exchange_means,
                                       float* exchange_sums, void* stream);
/* The training step's form of the row-partitioned call (engines/trainer.py:147-166 scores the coarse AND the fine semantic map
 * against the same geometry): TWO codes over ONE set of `batch` geometry patches, evaluated as the stacked batch of 2 * batch
 * patches [code0; code1] -- every term of the loss is a mean over the batch and the batch-wide quantities it subtracts depend
 * on the geometry only, so the result is (L(code0) + L(code1)) / 2 -- without materialising the stack (patch n reads geometry
 * n % batch and code n / batch).  neg_indx [2*batch] and rows index the STACKED batch (neg of patch batch+b = batch + neg of b).
 * channel_last != 0: code0/1 and grad_code0/1 are [batch,H,W,C], ray_o / ray_d [batch,H,W,3] -- the renderer's own tensors;
 * 0: [batch,C,H,W] / [batch,3,H,W].  depth [batch,H*W] is read only (values > max_depth are filtered on the fly).
 * workspace: nsos_corr_workspace_bytes(1, 2*batch, H*W, 0).  Phases and reductions as nsos_geo_correlation_loss_rows. */
int32_t nsos_geo_correlation_loss_pair(int32_t phase, const float* depth, const float* code0, const float* code1,
                                       const float* ray_o, const float* ray_d, const int64_t* neg_indx, const int32_t* rows,
                                       int32_t n_rows, int32_t batch, int32_t channel_last, int32_t code_dim, int32_t height,
                                       int32_t width, float self_shift, float self_weight, float neg_shift, float neg_weight,
                                       float max_depth, float* loss, float* grad_code0, float* grad_code1, void* workspace,
                                       size_t workspace_bytes, double* exchange_means, float* exchange_sums, void* stream);
/* CorrelationLoss (utils/image.py:335-370) row-partitioned the same way: phases 0..2 and the two reductions of
 * nsos_geo_correlation_loss_rows (one process: nsos_app_correlation_loss[_nhwc]).  A row patch needs only its own samples (coords1
 * of n, coords2 of neg[n]); its column gradient lands in patch neg[n], which another rank may own: `sums` carries that gradient for
 * every row (batch * S*S * 4 floats + the split loss sums), and phase 2 writes grad_code for the patches in `rows` only (zeros for
 * the others -- no rank needs them).  channel_last as nsos_app_correlation_loss_nhwc.  workspace: nsos_corr_workspace_bytes(0, ...);
 * rand1 / rand2 must hold the same draws on every rank. */
int32_t nsos_app_correlation_loss_rows(int32_t phase, const float* feats, const float* code, const int64_t* neg_indx,
                                       const float* rand1, const float* rand2, const int32_t* rows, int32_t n_rows, int32_t batch,
                                       int32_t channel_last, int32_t feat_dim, int32_t feat_h, int32_t feat_w, int32_t code_dim,
                                       int32_t code_h, int32_t code_w, int32_t feature_samples, float self_shift, float self_weight,
                                       float neg_shift, float neg_weight, float* loss, float* grad_code, void* workspace,
                                       size_t workspace_bytes, double* exchange_means, float* exchange_sums, void* stream);

/* ---- contrastive loss on the batch's class tokens (BASELINE configs[2]: "contrastive loss") ---------------
 * NeRFContrastive.forward with min_max_contrast=True (utils/image.py:192-218; call site engines/trainer.py:168-170,
 * `contrast_loss(cls_)`): sim = cosine_similarity of embeddings [n_tokens, dim] (each vector divided by max(|e|, 1e-8)
 * first), the off-diagonal entries' minimum and maximum (first occurrence in row-major order, like torch.argmin / argmax),
 * loss [1] = -log(max / (max + min)) -- NaN when max + min < 0, as in the reference.  grad_embeddings (may be NULL):
 * d loss / d embeddings [n_tokens, dim] (only the two picked pairs carry gradient).  2 <= n_tokens <= 120.  One
 * single-workgroup launch, deterministic. */
int32_t nsos_contrastive_loss(const float* embeddings, int32_t n_tokens, int32_t dim, float* loss, float* grad_embeddings,
                              void* stream);

/* The negatives of the correlation losses: similarity = F.cosine_similarity(x[None], x[:, None], dim=2) of the batch's class
 * tokens [n_tokens, dim] (get_similarity_matrix, utils/image.py:186-189; call site engines/trainer.py:125) and
 * negatives[j] = torch.min(similarity, dim=0)[1][j] (utils/image.py:354; first occurrence, a NaN wins) in ONE launch (torch:
 * thirteen).  similarity float [n_tokens, n_tokens] may be NULL.  negatives int64 [copies * n_tokens]: copy c holds
 * negatives + c * n_tokens (the stacked two-map evaluation of nsos_geo_correlation_loss_pair takes copies = 2).
 * 1 <= n_tokens <= 120. */
int32_t nsos_similarity_negatives(const float* tokens, int32_t n_tokens, int32_t dim, float* similarity, int64_t* negatives,
                                  int32_t copies, void* stream);

/* ---- correlation losses on the rendered patches --------------------------------
 * CorrelationLoss.forward (utils/image.py:335-370) and GeoCorrelationLoss.forward (utils/image.py:448-487) for one
 * batch of B patches, with the random choices made by the caller:
 *   neg_indx int64 [B]   the negative patch of each patch (reference: torch.min(sim_matrix, 0)[1], or a permutation)
 *   rand1, rand2 [B,S,S,2] the two torch.rand draws (values in [0,1); the kernel applies the reference's *2-1)
 * loss out [1].  grad_code out (may be NULL): d loss / d code, same shape as code -- the only input that carries
 * gradient in the reference (feats / depth sides are under no_grad).  Nothing of size (H*W)^2 is materialised for the
 * geometric loss.  workspace: nsos_corr_workspace_bytes(kind, B, n_points, feat_dim) bytes, 16-byte aligned
 * (kind 0 = appearance: n_points = S*S; kind 1 = geometric: n_points = H*W <= 4096, feat_dim ignored).
 * code_dim (sem_dim) <= 4.  Deterministic (fixed-order fp64 reductions, no atomics).
 * nsos_geo_correlation_loss: depth [B,1,H,W] is filtered as the reference does (values > max_depth become the
 * largest value < max_depth); with filter_in_place != 0 the filtered values are also written back, which is what
 * the reference does to the caller's tensor (utils/image.py:455). */
size_t nsos_corr_workspace_bytes(int32_t kind, int32_t batch, int32_t n_points, int32_t feat_dim);
int32_t nsos_app_correlation_loss(const float* feats, const float* code, const int64_t* neg_indx, const float* rand1,
                                  const float* rand2, int32_t batch, int32_t feat_dim, int32_t feat_h, int32_t feat_w,
                                  int32_t code_dim, int32_t code_h, int32_t code_w, int32_t feature_samples,
                                  float self_shift, float self_weight, float neg_shift, float neg_weight, float* loss,
                                  float* grad_code, void* workspace, size_t workspace_bytes, void* stream);
/* The same with code [B,Hc,Wc,C] and grad_code in that layout: the renderer's own `semantics` tensor as it is (no
 * permute().contiguous() copy on the way in, none of the gradient on the way out). */
int32_t nsos_app_correlation_loss_nhwc(const float* feats, const float* code, const int64_t* neg_indx, const float* rand1,
                                       const float* rand2, int32_t batch, int32_t feat_dim, int32_t feat_h, int32_t feat_w,
                                       int32_t code_dim, int32_t code_h, int32_t code_w, int32_t feature_samples,
                                       float self_shift, float self_weight, float neg_shift, float neg_weight, float* loss,
                                       float* grad_code, void* workspace, size_t workspace_bytes, void* stream);
int32_t nsos_geo_correlation_loss(float* depth, const float* code, const float* ray_o, const float* ray_d,
                                  const int64_t* neg_indx, int32_t batch, int32_t code_dim, int32_t height,
                                  int32_t width, float self_shift, float self_weight, float neg_shift,
                                  float neg_weight, float max_depth, int32_t filter_in_place, float* loss,
                                  float* grad_code, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DINO ViT-S/16 feature extractor (fp32; its backward: below) ----------------------------------------------------------
 * What engines/trainer.py:101-109 runs between the render and the losses: the rendered patches through a frozen DINO
 * ViT-S/16 (models/extractor.py:204-213 get_vit_attn_feat over models/vision_transformer.py vit_small(patch_size=16)).
 *   1. engines/trainer.py:103-106: channels first, F.interpolate(x, (h*stride, w*stride)) (nearest), (x - mean) / std;
 *   2. models/extractor.py:207-208: F.interpolate(x, size=(224,224)) (nearest), (x - mean) / std (again: kept);
 *      both resizes use torch's index rule min(floor(dst * (float)in / out), in - 1) with the product in fp32 and compose into one
 *      gather; subtract and divide are rounded separately (the prepared image is bit-equal to torch's);
 *   3. models/vision_transformer.py:196-215: 16x16 patch embedding, class token, + pos_embed, 12 blocks
 *      x += proj(attn(LN(x))); x += fc2(GELU(fc1(LN(x)))); LayerNorm eps 1e-6, 6 heads of 64, scale 1/8, erf GELU;
 *   4. models/extractor.py:109-117,209-212: block 11's output BEFORE the final norm: cls = x[:,0], feat = x[:,1:];
 *      attn = block 11's softmax, mean over the heads (h = 0..5 summed in that order, then / 6), row 0, columns 1..196.
 * Depth / width / heads are compile-time constants; the batch is a runtime argument (1..NSOS_DINO_MAX_BATCH).
 * Accumulation order (fixed: two runs give the same bits, and an image's result does not depend on the batch around it):
 * every GEMM output element is ONE fp32 fma chain over k = 0..K-1 ascending starting from 0 (v_mfma_f32_32x32x2_f32), then
 * + bias, then GELU, then + residual; q.k sums d = 0..63 ascending, softmax.v sums the keys 0..196 ascending (v_mfma_f32_16x16x4_f32);
 * LayerNorm / softmax row sums: six (four) strided elements per lane ascending, then an xor butterfly 32,16,8,4,2,1 over the wave. */
#define NSOS_DINO_DEPTH 12
#define NSOS_DINO_WIDTH 384
#define NSOS_DINO_HEADS 6
#define NSOS_DINO_TOKENS 197 /* 1 + 14*14 */
#define NSOS_DINO_IMAGE 224
#define NSOS_DINO_PATCH 16
#define NSOS_DINO_HIDDEN 1536
#define NSOS_DINO_MAX_BATCH 1024

/* DINO's checkpoint tensors (device fp32, nn.Linear / nn.Conv2d layout as in the state dict).  norm.weight / norm.bias are not
 * here: the final norm is never applied on this path. */
typedef struct nsos_dino_block_tensors {
    const float *norm1_w, *norm1_b; /* blocks.i.norm1.*       [384] */
    const float *qkv_w, *qkv_b;     /* blocks.i.attn.qkv.*    [1152,384] [1152] */
    const float *proj_w, *proj_b;   /* blocks.i.attn.proj.*   [384,384] [384] */
    const float *norm2_w, *norm2_b; /* blocks.i.norm2.*       [384] */
    const float *fc1_w, *fc1_b;     /* blocks.i.mlp.fc1.*     [1536,384] [1536] */
    const float *fc2_w, *fc2_b;     /* blocks.i.mlp.fc2.*     [384,1536] [384] */
} nsos_dino_block_tensors;
typedef struct nsos_dino_tensors {
    const float* cls_token;         /* [1,1,384] */
    const float* pos_embed;         /* [1,197,384] */
    const float *patch_w, *patch_b; /* patch_embed.proj.*     [384,3,16,16] [384] */
    nsos_dino_block_tensors blocks[NSOS_DINO_DEPTH];
} nsos_dino_tensors;

/* The frozen network is packed once into the stream the kernels read: every weight matrix transposed to [in,out] (the GEMM's
 * B operand, streamed row by row), biases and LayerNorm vectors as they are, pos_embed with row 0 replaced by cls_token + pos_embed[0].
 * `packed`: nsos_dino_packed_bytes() bytes, 16-byte aligned.  Call again whenever a parameter changes. */
size_t nsos_dino_packed_bytes(void);
int32_t nsos_dino_pack(const nsos_dino_tensors* tensors, void* packed, size_t packed_bytes, void* stream);

/* flags of nsos_dino_forward */
enum {
    NSOS_DINO_NHWC = 1,     /* input is [B,h,w,3] (the renderer's rgb) instead of [B,3,h,w] */
    NSOS_DINO_STEP1 = 2,    /* also do the trainer's step 1 (resize to (h*stride, w*stride) and normalise) before step 2 */
    NSOS_DINO_PREPARED = 4  /* input is an already prepared [B,3,224,224] image: steps 1-2 skipped (excludes the other two) */
};
/* workspace: nsos_dino_workspace_bytes(batch) bytes (0 for a batch outside 1..NSOS_DINO_MAX_BATCH), 16-byte aligned, contents
 * undefined on return.  Outputs, each optional (NULL to skip): feat [B,196,384], cls [B,384], attn [B,1,196],
 * prepared [B,3,224,224] (the image after steps 1-2), blocks [12,B,197,384] (every block's output: localises a difference).
 * Everything is validated before anything is launched or written.  No host synchronisation, no allocation: capturable.  The one-time
 * per-device kernel attribute (the attention kernel's dynamic LDS size) is set by nsos_dino_pack as well, so a forward call whose first
 * use is inside a stream capture has nothing left to configure; if setting it fails the positive hipError_t is returned. */
size_t nsos_dino_workspace_bytes(int32_t batch);
int32_t nsos_dino_forward(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                          const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn,
                          float* prepared, float* blocks, void* stream);
/* Host helper: the source index of each of the 224 output rows (or columns) of steps 1-2 for an input extent `in_size`
 * (patch_stride <= 0: step 2 alone), exactly the rule the prepare kernel evaluates.  idx: HOST int32 [224]. */
int32_t nsos_dino_resize_indices(int32_t in_size, int32_t patch_stride, int32_t* idx);

/* ---- DINO ViT-S/16, backward to the input (csrc/dino_vit_bwd.hip; fp32) ---------------------------------------------------------------
 * The gradient of sum(feat * g_feat) + sum(cls * g_cls) with respect to the image handed to nsos_dino_forward: the reference's
 * extractor is differentiable (engines/trainer.py:103-108 feeds the rendered rgb to it with autograd on), the weights are frozen, so
 * input gradients only.
 *   nsos_dino_forward_save  = nsos_dino_forward (same launches, bit-equal feat / cls / attn; no `prepared`, no `blocks`) that also keeps
 *     the input of every block: saved [12][B][197][384], nsos_dino_saved_bytes(batch) = 3.63 MB per image (0 for a batch outside
 *     1..NSOS_DINO_MAX_BATCH), 16-byte aligned.  Checks as nsos_dino_forward, `saved` joining the NULL and the alignment check.
 *   nsos_dino_pack_backward: the backward's own stream, nsos_dino_backward_packed_bytes() bytes, 16-byte aligned: 1536 zeros, then
 *     patch_embed.proj.weight and every block's qkv / proj / fc1 / fc2 matrix in the state dict's own [out,in] layout (the operand of
 *     dA[M,in] = dOut[M,out] . W[out,in] on the forward's GEMM tile).  Checks as nsos_dino_pack; sets the backward kernels' per-device
 *     attribute (and the forward's), so that a first nsos_dino_backward inside a stream capture has nothing left to configure.
 *   nsos_dino_backward: batch / in_h / in_w / patch_stride / flags as given to the forward; packed (nsos_dino_pack) and packed_bwd
 *     (nsos_dino_pack_backward) of the same checkpoint; saved from nsos_dino_forward_save of that call; g_feat [B,196,384] and g_cls [B,384],
 *     either may be NULL (= zeros, bit for bit), not both; workspace nsos_dino_backward_workspace_bytes(batch) bytes (4.25 MB per image, 0
 *     for a batch outside 1..NSOS_DINO_MAX_BATCH), 16-byte aligned; g_input: the input's shape and layout ([B,h,w,3] with
 *     NSOS_DINO_NHWC, else [B,3,h,w]), every element written -- a source pixel that no pixel of the 224 x 224 image reads (an input
 *     larger than 224) gets exactly 0.0; g_blocks (optional, NULL to skip): the residual-stream gradient at the INPUT of every block,
 *     [12][B][197][384], the mirror of `blocks`.
 *     Per block, 11..0: the block's forward is recomputed from its saved input with the forward's kernels (qkv, the residual midpoint,
 *     the MLP's pre-activation), then fc2 -> GELU' (exact erf form) -> fc1 -> LayerNorm' -> proj -> attention' (probabilities recomputed)
 *     -> qkv -> LayerNorm'; then the patch embedding and the two resizes as one gather, * 1/sd_c (1/sd_c^2 with NSOS_DINO_STEP1, 1 with
 *     NSOS_DINO_PREPARED).
 *     Check order: NULL pointer (packed, packed_bwd, saved, workspace, g_input, and g_feat and g_cls both NULL) -> then exactly
 *     nsos_dino_forward's: shape -> flag bits -> PREPARED -> STEP1 -> size limits -> alignment (16 bytes: packed, packed_bwd, saved,
 *     workspace; 4: g_feat, g_cls, g_input, g_blocks) -> workspace size.  Everything is validated before anything is launched or written.
 *     No host synchronisation, no allocation: capturable.
 *     Order (fixed; no atomics; an image's bits do not depend on its batch): every data-gradient GEMM output is one fp32 fma chain over
 *     the out-features ascending from 0 (v_mfma_f32_32x32x2_f32); LayerNorm' row sums as the forward's; attention (v_mfma_f32_16x16x4_f32):
 *     p as the forward, dP = dO.v over d ascending, delta = rowsum(dP*p) (four strided columns per lane ascending, then the butterfly),
 *     dQ over the keys ascending, dK and dV over the queries ascending in one workgroup per 32 keys; the input gather sums a pixel's
 *     preimage in ascending (y, x) order. */
size_t nsos_dino_saved_bytes(int32_t batch);
int32_t nsos_dino_forward_save(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                               const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn,
                               float* saved, void* stream);
size_t nsos_dino_backward_packed_bytes(void);
int32_t nsos_dino_pack_backward(const nsos_dino_tensors* tensors, void* packed_bwd, size_t packed_bytes, void* stream);
size_t nsos_dino_backward_workspace_bytes(int32_t batch);
int32_t nsos_dino_backward(int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags, const void* packed,
                           const void* packed_bwd, const float* saved, const float* g_feat, const float* g_cls, void* workspace,
                           size_t workspace_bytes, float* g_input, float* g_blocks, void* stream);

/* ---- DINO ViT-S/16, 16-bit operands (csrc/dino_vit16.hip) ---------------------------------------------------------------------
 * The same forward pass as nsos_dino_forward (same arguments, flags, outputs -- all fp32 -- and validation) with the two operands of
 * every matrix product (patch embedding, qkv, q.k^T, p.v, proj, fc1, fc2) in `precision` = NSOS_DTYPE_F16 or NSOS_DTYPE_BF16
 * (NSOS_DTYPE_F32 is refused with NSOS_ERR_UNSUPPORTED: that is nsos_dino_forward) and fp32 accumulation
 * (v_mfma_f32_16x16x32_{f16,bf16}).  Each operand is rounded ONCE, to nearest even, by whatever produces it: the weights at pack
 * time, the im2col tokens, the LayerNorm output, qkv, the probabilities (after the fp32 division), the attention output and the GELU
 * hidden by their kernels' epilogues.  fp32 throughout: the residual stream, LayerNorm (statistics and affine), softmax (row max,
 * expf, row sum, division), bias, GELU (erf), the residual add, feat / cls / attn (attn from the fp32 probabilities), `prepared`
 * (bit-equal to nsos_dino_forward's) and `blocks`.  fp16 has no range check: an operand beyond 65504 becomes infinity; use bf16
 * for a checkpoint whose activations are not known.
 * Packed stream (nsos_dino_packed16_bytes() = 43.6 MB, 16-byte aligned): an fp32 section (pos_embed with row 0 = cls_token +
 * pos_embed[0], every bias and LayerNorm vector), then every weight matrix in 16 bits in nn.Linear's own [out,in] layout (an MFMA
 * operand fragment is 16 contiguous bytes of a row).  A stream packed for one precision is read only with that precision.
 * Workspace: nsos_dino_workspace16_bytes(batch) bytes (0 outside 1..NSOS_DINO_MAX_BATCH), 16-byte aligned.
 * Order (fixed; an image's bits do not depend on the batch): every GEMM output is one fp32 chain over k ascending in steps of 32,
 * then + bias, GELU, + residual; q.k over d ascending, p.v over the keys ascending (32 at a time); row sums as nsos_dino_forward.
 * No attribute to configure, no host synchronisation, no allocation: capturable. */
size_t nsos_dino_packed16_bytes(void);
int32_t nsos_dino_pack16(const nsos_dino_tensors* tensors, int32_t precision, void* packed, size_t packed_bytes, void* stream);
size_t nsos_dino_workspace16_bytes(int32_t batch);
int32_t nsos_dino_forward16(const float* input, int32_t batch, int32_t in_h, int32_t in_w, int32_t patch_stride, int32_t flags,
                            int32_t precision, const void* packed, void* workspace, size_t workspace_bytes, float* feat, float* cls,
                            float* attn, float* prepared, float* blocks, void* stream);

/* ---- DINO's full-image path and find_fg (engines/eval.py:133-144 and :237-248) ---------------------------------------------
 * models/extractor.py:215-224 get_vit_attn_feat_noresize: x [B,3,H,W] (or [B,H,W,3] with NSOS_DINO_FULL_NHWC), (x - mean) / std
 * once (twice with NSOS_DINO_FULL_NORMALIZE: eval.py's normalize_batch first), no resize; a rows x cols = (H // 16) x (W // 16)
 * patch grid (the remainder pixels are never read), T = 1 + rows*cols tokens; every H, W >= 16 with rows*cols <= 16384.
 * Position embedding (models/vision_transformer.py:174-194): used as it is when rows*cols == 196 and H == W; otherwise the 14x14
 * patch part goes through ATen's upsample_bicubic2d (align_corners=False, A = -0.75, border taps clamped) with
 * scale_factor = ((rows + 0.1) / 14, (cols + 0.1) / 14) -- source coordinate (dst + 0.5) / scale_factor - 0.5 --, evaluated in fp64
 * and rounded once; the class position is prepended unchanged.  Then the same 12 blocks (same GEMM and LayerNorm kernels, same
 * orders as nsos_dino_forward) with a streaming attention: keys in tiles of 64, ascending, running max m and sum l per query row
 * (online softmax: per tile the row max / sum over a lane's four 16-key blocks in order, then an xor butterfly 1,2,4,8 over the
 * row's 16 lanes; o and l rescaled by exp(m_old - m_new); q.k over d = 0..63 ascending; p.v over the tile's keys ascending; o / l at
 * the end).  attn = block 11's softmax of query 0, exp(s - m) / l per head with that head's final (m, l), heads 0..5 summed in
 * order, / 6.  Outputs, each optional: feat [B,rows*cols,384], cls [B,384], attn [B,1,rows*cols], pos [T,384] (the table added to
 * the tokens).  Workspace: nsos_dino_full_workspace_bytes(batch, H, W) bytes, 16-byte aligned; 0 = refused (batch outside
 * 1..NSOS_DINO_MAX_BATCH, H or W < 16, over the token cap, batch*T over the GEMMs' grid, or a size past size_t).  Everything is
 * validated before anything is launched; no host synchronisation, no allocation: capturable. */
#define NSOS_DINO_FULL_MAX_PATCHES 16384
enum {
    NSOS_DINO_FULL_NHWC = 1,      /* input [B,H,W,3] (the renderer's rgb) instead of [B,3,H,W] */
    NSOS_DINO_FULL_NORMALIZE = 2  /* normalise twice: engines/eval.py:136 normalize_batch, then get_vit_attn_feat_noresize's own */
};
size_t nsos_dino_full_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int32_t nsos_dino_forward_full(const float* input, int32_t batch, int32_t h, int32_t w, int32_t flags, const void* packed,
                               void* workspace, size_t workspace_bytes, float* feat, float* cls, float* attn, float* pos, void* stream);
/* Host helper: the position table [1 + rows*cols][384] the forward adds, from a HOST pos_embed [197][384] (row 0 copied), by the
 * rule the kernel evaluates.  out: HOST float [(1 + rows*cols) * 384]. */
int32_t nsos_dino_interp_pos(const float* pos_embed, int32_t h, int32_t w, float* out);
/* find_fg (engines/eval.py:138-144) for one image: attn [rows*cols] (the forward's attn of that image) nearest-upsampled to H x W
 * by ATen's size= rule min(floor(dst * (float)rows / H), rows - 1); over labels [H*W] (int32, e.g. the k-means clustering
 * [H,W,1]) the sums of the upsampled attention and the pixel counts of clusters 0 and 1, in fp64: 256 fixed pixel ranges, each a
 * strided per-thread sum then a tree 128,64,..,1, then the same tree over the 256 partials.  mean = sum / count (an empty cluster
 * gives NaN); flipped = mean1 < mean0 (False with a NaN); out_labels = flipped ? 1 - labels : labels for every pixel (labels
 * outside {0,1} enter neither mean but are mapped: 2 -> -1).  Optional outputs: attn_up [H*W] fp32, means [2] fp64
 * (mean0, mean1), flipped [1] int32.  workspace: nsos_dino_find_fg_workspace_bytes(), 16-byte aligned.  No host synchronisation. */
size_t nsos_dino_find_fg_workspace_bytes(void);
int32_t nsos_dino_find_fg(const int32_t* labels, const float* attn, int32_t h, int32_t w, int32_t* out_labels, float* attn_up,
                          double* means, int32_t* flipped, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LPIPS v0.1, AlexNet (csrc/lpips.hip) ------------------------------------------------------------------------------------
 * utils/image.py:149-160 lpips(img1, img2, net='alex') as engines/eval.py:87 calls it: lpips.LPIPS(net='alex') with lpips=True,
 * spatial=False, in eval mode.  Forward only, fp32.  img0, img1 [N,3,H,W] (or [N,H,W,3] with NSOS_LPIPS_NHWC); with
 * NSOS_LPIPS_NORMALIZE each is first mapped 2x - 1 (the package's normalize=True).
 *   1. scaling layer: (x - shift[c]) / scale[c];
 *   2. features after each ReLU: conv 3->64 k11 s4 p2 | maxpool k3 s2, conv 64->192 k5 p2 | maxpool k3 s2, conv 192->384 k3 p1 |
 *      conv 384->256 k3 p1 | conv 256->256 k3 p1 (output extent (H + 4 - 11) / 4 + 1, pools (n - 3) / 2 + 1; H, W >= 31);
 *   3. per layer l and pixel n(f) = f / (sqrt(sum_c f^2) + 1e-10); d_l = mean_{h,w} sum_c lin_l[c] * (n(f0) - n(f1))^2;
 *   4. out[b] = d_0 + d_1 + d_2 + d_3 + d_4.
 * Layout: activations are pixel-major [image][y][x][channel] with image 2b = img0[b], image 2b + 1 = img1[b].  Every convolution is
 * one implicit GEMM (v_mfma_f32_32x32x2_f32): rows = the output pixels of all 2N images, columns = Cout, K index
 * k = (ky * ksize + kx) * Cin + c (channel fastest: a K slice of a row is contiguous in memory), a tap outside the image contributing
 * a = 0.  conv1's gather reads the images directly (either layout) and applies 2x - 1 and the scaling layer on the way.  The
 * max-pools are a kernel of their own.
 * Packed stream (nsos_lpips_packed_bytes() bytes = 4 * (8 + sum_l (Kp_l + 2) * Cout_l) with Kp = 384 (363 padded to the K tile of
 * 32), 1600, 1728, 3456, 2304; 16-byte aligned): shift[3] + 1 zero, scale[3] + 1 zero, then per layer Wt_l [Kp_l][Cout_l] (the
 * convolution weight transposed to the K order above, rows past K zero) and bias_l [Cout_l], then lin_0 .. lin_4.
 * Summation orders (fixed: an image's bits do not depend on the batch, and swapping img0 and img1 changes no bit):
 *   convolution: per output element, per K tile of 32 one fp32 fma chain over k ascending from zero; the tiles' partial sums are
 *   added in ascending order with the rounding error of each addition carried (two-sum: tot' = fl(tot + p), lo += (tot + p) - tot'),
 *   then fl(fl(tot + lo) + bias), then ReLU;
 *   max-pool: dy = 0..2 outer, dx = 0..2 inner;
 *   channel sums (sum f^2 and the lin-weighted sum; fp32): lane j of a wave adds channels j, j + 64, ... ascending, then an xor
 *   butterfly 32, 16, 8, 4, 2, 1 over the 64 lanes;
 *   pixels (fp64): per (layer, pair) NSOS_LPIPS_DIST_BLOCKS workgroups, workgroup g the pixels [g * chunk, (g + 1) * chunk) with
 *   chunk = ceil(P / NSOS_LPIPS_DIST_BLOCKS), wave v of its four every 4th pixel from g * chunk + v ascending, the workgroup
 *   ((v0 + v1) + v2) + v3; then the workgroups g ascending, / P, rounded to fp32 once; the five layers in order 0..4 in fp32.
 * Outputs: out [batch]; optional layers [batch][5] (the d_l) and feats: the ten post-ReLU feature maps, layer after layer, layer l
 * as [2 * batch][H_l][W_l][C_l] fp32 (pixel-major, image 2b = img0[b], 2b + 1 = img1[b]; C = 64, 192, 384, 256, 256; 16-byte aligned).
 * Workspace: nsos_lpips_workspace_bytes(batch, h, w) bytes (0 = refused: batch outside 1..NSOS_LPIPS_MAX_BATCH, h or w outside
 * 31..16384, or more than 2^31 GEMM rows), 16-byte aligned, contents undefined on return.
 * Validated before anything is launched: NULL -> -1; negative batch or h, w <= 0 -> -2; batch == 0 -> 0 with no launch; h or w < 31,
 * an unknown flag or a refused size -> -3; a misaligned pointer -> -5; a workspace too small -> -4.  No atomics, no host
 * synchronisation, no allocation, no attribute to configure: capturable. */
#define NSOS_LPIPS_LAYERS 5
#define NSOS_LPIPS_MIN_SIZE 31
#define NSOS_LPIPS_MAX_BATCH 1024
#define NSOS_LPIPS_DIST_BLOCKS 64
enum {
    NSOS_LPIPS_NHWC = 1,      /* inputs [N,H,W,3] (the renderer's rgb) instead of [N,3,H,W] */
    NSOS_LPIPS_NORMALIZE = 2  /* 2x - 1 first (inputs in [0,1] instead of [-1,1]) */
};
/* lpips.LPIPS's tensors (device fp32, nn.Conv2d layout as in the state dict) */
typedef struct nsos_lpips_tensors {
    const float *shift, *scale;            /* scaling_layer.shift / .scale            [1,3,1,1] */
    const float* conv_w[NSOS_LPIPS_LAYERS]; /* net.slice{1..5}.{0,3,6,8,10}.weight     [64,3,11,11] [192,64,5,5] [384,192,3,3] [256,384,3,3] [256,256,3,3] */
    const float* conv_b[NSOS_LPIPS_LAYERS]; /* ... .bias                               [Cout] */
    const float* lin_w[NSOS_LPIPS_LAYERS];  /* lin{0..4}.model.1.weight                [1,C,1,1] */
} nsos_lpips_tensors;
size_t nsos_lpips_packed_bytes(void);
int32_t nsos_lpips_pack(const nsos_lpips_tensors* tensors, void* packed, size_t packed_bytes, void* stream);
size_t nsos_lpips_workspace_bytes(int32_t batch, int32_t h, int32_t w);
int32_t nsos_lpips_forward(const float* img0, const float* img1, int32_t batch, int32_t h, int32_t w, int32_t flags, const void* packed,
                           float* out, float* layers, float* feats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CameraTransformer: learnable per-camera pose corrections (csrc/camera.hip) ----------------------------------------------
 * models/camera.py:81-143.  Per camera c a quaternion rvec[c] = (x, y, z, w) -- w LAST -- and an offset tvec[c]; ray n carries
 * the camera id c = cam_ids[n] (int32).  All tensors fp32, dense: rays_o, rays_d, out_o, out_d [n_rays,3]; rvec [n_cams,4];
 * tvec [n_cams,3].
 * Forward (camera.py:103-143), every operation rounded to fp32 on its own (no contraction), in the reference's order:
 *   theta = sqrt(1e-5 + ((x x + y y) + z z) + w w);  (a, b, c, w') = rvec[c] / theta    -- the epsilon sits INSIDE the root, so
 *   the normalised quaternion is not exactly unit and R below is not exactly orthogonal: the backward differentiates THIS map;
 *   R = [ (1 - 2 b b) - 2 c c    2 (a b - c w')        2 (a c + b w')
 *         2 (a b + c w')         (1 - 2 a a) - 2 c c   2 (b c - a w')
 *         2 (a c - b w')         2 (a w' + b c)        (1 - 2 a a) - 2 b b ];
 *   out_d[n][i] = (d[0] R[i][0] + d[1] R[i][1]) + d[2] R[i][2];   out_o[n] = o[n] + tvec[c]  (one rounded add).
 *   The identity (0,0,0,1) returns its input bit for bit (every product is by an exact 0 or 1).
 * Backward.  g_tvec[c] = sum_{n: id = c} g_out_o[n];  G[c] = sum_{n: id = c} g_out_d[n] (x) d[n]  (3x3);  g_qhat = the contraction of
 * G with dR / d(a, b, c, w') (R is quadratic: a 4-vector);  g_rvec[c] = g_qhat / theta - rvec[c] (rvec[c] . g_qhat) / theta^3;
 * and, when asked, g_rays_o[n] = g_out_o[n], g_rays_d[n] = R^T g_out_d[n] (fp32, j = 0, 1, 2 in order, the forward's R).
 * Reduction over the rays -- no atomics, a fixed order, two calls give the same bits; ids in any order:
 *   the batch is cut into K = min(NSOS_CAMERA_MAX_CHUNKS, ceil(n_rays / NSOS_CAMERA_CHUNK)) contiguous
 *   chunks of L = ceil(n_rays / K) rounded up to 256 rays.  One 256-thread workgroup per (camera c, chunk k) scans the chunk's ids:
 *   thread t takes rays k L + t, + 256, ... ascending and adds the 12 products of its rays with id == c in fp64 (each product of two
 *   fp32 numbers is exact in fp64); the 64 lanes of a wave are summed in six fixed pairing steps (nsos_wave_sum, every lane
 *   adding the same pairs): lane l with l ^ 1; with l ^ 2; inside each group of 8 lanes with its mirror 7 - (l % 8) (row_half_mirror);
 *   inside each row of 16 with its mirror 15 - (l % 16) (row_mirror); row r with row r ^ 1 (lane kept); half with half; the four
 *   waves as ((v0 + v1) + v2) + v3; partial [c][k][12] goes to the workspace.  A second kernel, one thread per camera, adds the K
 *   partials k ascending, contracts in fp64 (theta and the normalised quaternion recomputed in fp64 from the fp32 rvec) and rounds
 *   each output to fp32 once.  Hence camera c's gradient depends only on c's own rays and their POSITIONS in the batch: whatever
 *   the other rays hold, and whichever other camera they name, changes no bit of it.  A camera without a ray gets exact zeros.
 * Out-of-range ids (the reference raises an IndexError): nothing outside rvec / tvec is ever read.  A ray whose id is outside
 * [0, n_cams) gets NaN in out_o and out_d, enters no sum, and gets zeros in g_rays_o / g_rays_d.
 * workspace: nsos_camera_workspace_bytes(n_rays, n_cams) = 96 n_cams K bytes (0 for n_cams <= 0 or n_rays < 0), 8-byte aligned,
 * needed only when g_rvec or g_tvec is asked for; contents undefined on return.
 * Validated before anything is launched: a NULL input or output (backward: each of the four outputs may be NULL, not all of them;
 * the workspace may be NULL when neither g_rvec nor g_tvec is asked for) -> -1; n_cams <= 0 or n_rays < 0 -> -2; n_rays == 0 -> 0
 * with no launch; n_cams > NSOS_CAMERA_MAX_CAMS -> -3; a workspace too small -> -4.  Launches only, on `stream`: no host
 * synchronisation, no allocation: capturable. */
#define NSOS_CAMERA_CHUNK 2048
#define NSOS_CAMERA_MAX_CHUNKS 64
#define NSOS_CAMERA_MAX_CAMS 65535
size_t nsos_camera_workspace_bytes(int64_t n_rays, int32_t n_cams);
int32_t nsos_camera_transform(const float* rays_o, const float* rays_d, const int32_t* cam_ids, const float* rvec, const float* tvec,
                              int64_t n_rays, int32_t n_cams, float* out_o, float* out_d, void* stream);
int32_t nsos_camera_transform_backward(const float* g_out_o, const float* g_out_d, const float* rays_d, const int32_t* cam_ids,
                                       const float* rvec, int64_t n_rays, int32_t n_cams, void* workspace, size_t workspace_bytes,
                                       float* g_rvec, float* g_tvec, float* g_rays_o, float* g_rays_d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_SOS_HIP_H */
