// What the fp32 DINO forward (dino_vit.hip) and its backward (dino_vit_bwd.hip) share: the layout of the forward's packed stream and
// workspace, and the two host functions of dino_vit.hip that the backward calls to recompute a block with the forward's own kernels.
#pragma once
#include "dino_common.h"

namespace nsos {
namespace dino32 {

using namespace nsos::dino;

// ---- packed stream of nsos_dino_pack (floats) ------------------------------------------------------------------------------------
constexpr size_t P_POS = 0;                                  // [197][384], row 0 = cls_token + pos_embed[0]
constexpr size_t P_EMB_W = P_POS + (size_t)T * D;            // [768][384]  (patch_embed.proj.weight transposed)
constexpr size_t P_EMB_B = P_EMB_W + (size_t)KE * D;
constexpr size_t P_BLOCKS = P_EMB_B + D;
constexpr size_t B_LN1W = 0, B_LN1B = B_LN1W + D, B_QKVW = B_LN1B + D, B_QKVB = B_QKVW + (size_t)D * 3 * D, B_PROJW = B_QKVB + 3 * D,
                 B_PROJB = B_PROJW + (size_t)D * D, B_LN2W = B_PROJB + D, B_LN2B = B_LN2W + D, B_FC1W = B_LN2B + D,
                 B_FC1B = B_FC1W + (size_t)D * HID, B_FC2W = B_FC1B + HID, B_FC2B = B_FC2W + (size_t)HID * D, B_SIZE = B_FC2B + D;
constexpr size_t P_SIZE = P_BLOCKS + (size_t)NSOS_DINO_DEPTH * B_SIZE;
static_assert(P_EMB_W % 4 == 0 && P_BLOCKS % 4 == 0 && B_SIZE % 4 == 0 && B_QKVW % 4 == 0 && B_FC2W % 4 == 0, "float4 rows");

// ---- workspace of nsos_dino_forward (floats per image) ---------------------------------------------------------------------------
constexpr size_t W_X = 0, W_LN = W_X + (size_t)T * D, W_QKV = W_LN + (size_t)T * D, W_AO = W_QKV + (size_t)T * 3 * D,
                 W_HID = W_AO + (size_t)T * D, W_TOK = W_HID + (size_t)T * HID, W_ROW0 = W_TOK + (size_t)NP * KE,
                 W_SIZE = W_ROW0 + (size_t)HEADS * NP;
static_assert(W_SIZE % 4 == 0 && W_LN % 4 == 0 && W_QKV % 4 == 0 && W_TOK % 4 == 0, "16-byte aligned sections for every batch size");

// ---- dino_vit.hip, for the backward (hidden: not part of the C ABI) ---------------------------------------------------------------
// the forward attention kernel's dynamic-LDS attribute, once per device (NSOS_OK or the positive hipError_t)
__attribute__((visibility("hidden"))) int32_t configure();
// One block's forward from its input x_in [B*197,384] with the forward's own launches, up to the MLP's pre-activation:
//   ln <- LN1(x_in); qkv <- ln.Wqkv + b; ao <- attention(qkv); xmid <- x_in + ao.Wproj + b; ln <- LN2(xmid); hid <- ln.Wfc1 + b
// (no GELU).  `block` is the block's section of the packed stream.  qkv and xmid are bit-equal to what nsos_dino_forward held.
__attribute__((visibility("hidden"))) void recompute_block(const float* block, const float* x_in, float* xmid, float* ln, float* qkv,
                                                           float* ao, float* hid, int batch, hipStream_t st);

}  // namespace dino32
}  // namespace nsos
