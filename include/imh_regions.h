/* imh_regions.h -- the one entry of libimh_hip.so that regional image prompts add (csrc/xattn_regions.hip).  A companion of include/imh.h,
 * which it includes for the status codes and imh_dtype; conventions (pointers, streams, errors) as stated there. */
#ifndef IMH_REGIONS_H_
#define IMH_REGIONS_H_

#include "imh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fused QKV + cross-attention with N masked image prompts ------------------------------------------------------------------------
 * imh_cross_attention (include/imh.h) with the one image prompt replaced by n_img of them, each with its own softmax, a weight and a mask
 * over the query tokens (diffusers IPAdapterAttnProcessor2_0 with ip_adapter_masks and several images per adapter):
 *   q = attn.to_q(LN(x))
 *   O[b, q, h] = softmax(q K^T * scale) V + sum_{i < n_img} (g * w_i) * m_i[q] * softmax(q K2_i^T * scale) V2_i
 * g = scale2_tab ? scale2_tab[*step] : scale2 (today's gated IP scale), w_i = weights[i] (NULL: all 1), m_i[q] = mask[i * ldm + q].
 * Additive like imh_adapter_op: an entry and an argument struct of its own in this companion header; include/imh.h, every struct, enum and
 * existing entry stay as they were and the ABI stays at 13.  In a plan: kind IMH_OP_XATTN_REGIONS = 17, a #define like kinds 13 and 15
 * (kinds 12, 14 and 16 stay refused).
 *
 * Every field that imh_xattn_args has means here what it means there (X, Wq, the folded LayerNorm quadruple, the text K / Vt caches, O, the
 * shapes and leading dimensions, scale, scale2, scale2_tab, step, dtype, pf_ptr, pf_bytes).  Added:
 *   n_img           image prompts per batch entry, 1 .. 8
 *   K2 / Vt2        REQUIRED: the image-prompt caches in imh_xattn_args' K2 / Vt2 layouts (IMH_GF_VT_PERM included), image i of batch b at
 *                   rows (Vt2: columns) (b * n_img + i) * Lk2_pad -- what the K / V projection writes when the image tokens are handed to it
 *                   as a batch of B * n_img.  Lk2 (tokens per image) is the same for every image.
 *   mask            fp32 [n_img][ldm], ldm >= Lq: the same rows serve every batch entry and every head
 *   weights         fp32 [n_img], or NULL (all 1)
 * Arithmetic: after the text pass, image i = 0 .. n_img - 1 in order: the lane that owns query row q forms wq = (g * w_i) * m_i[q],
 *   inv = wq / l_tot (l_tot the image's softmax denominator), fin += o * inv.  With n_img == 1, w = 1 and m == 1 this is
 *   imh_cross_attention's two-pass arithmetic operation for operation (the same bits); a mask or gate of 0 leaves the text-only bits.
 * Kernel form: the one-head form only (one workgroup per (batch, head, 128 queries), half items as there); any Lq.  The wide five-head form
 *   is not built for regions: the entry never selects it and imh_debug_set key 3 has no influence on it.
 * Refused without a launch: null args / X / Wq / K / Vt / K2 / Vt2 / O / mask, ln_s without ln_c (or the reverse, or without ln_eps > 0 or
 *   ln_stats), mask or weights not 4-byte aligned, scale2_tab without step or step without scale2_tab (IMH_ERR_ARG); n_img outside 1 .. 8,
 *   ldm < Lq, Lk2 <= 0, Lk2_pad % 64, Lk2_pad < Lk2, and every shape rule of imh_cross_attention (IMH_ERR_SHAPE); another dtype
 *   (IMH_ERR_DTYPE).
 * Memory: reads what imh_cross_attention reads (rows [0, B*Lq) x columns [0, C) of X, all of Wq [C, C], ln_s / ln_c [C], ln_stats
 *   [B*Lq][ln_slots][2], the text caches padding included), K2 / Vt2 over B * n_img * Lk2_pad keys, mask[i][0 .. Lq) for i < n_img and
 *   weights[0 .. n_img); writes rows [0, B*Lq) x columns [0, C) of O.  Nothing else. */
#define IMH_OP_XATTN_REGIONS 17
#define IMH_REGIONS_MAX_IMAGES 8
typedef struct imh_xattn_regions_args {
    const void* X;
    const void* Wq;
    const float* ln_s;
    const float* ln_c;
    float ln_eps;
    const float* ln_stats;
    int32_t ln_slots;
    const void* K;
    const void* Vt;
    const void* K2;
    const void* Vt2;
    void* O;
    int32_t B, H, Lq, C;
    int32_t Lk, Lk_pad;
    int32_t Lk2, Lk2_pad;
    int32_t ldx, ldw, ldk, ldvt, ldk2, ldvt2, ldo;
    float scale;
    float scale2;
    const float* scale2_tab;
    const int32_t* step;
    int32_t dtype;
    const void* pf_ptr;
    uint32_t pf_bytes;
    int32_t n_img;
    const float* mask;
    int32_t ldm;
    const float* weights;
} imh_xattn_regions_args;
int imh_cross_attention_regions(const imh_xattn_regions_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMH_REGIONS_H_ */
