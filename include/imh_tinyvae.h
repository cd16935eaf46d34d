/* imh_tinyvae.h -- the one entry of libimh_hip.so that the tiny VAE decoder adds (csrc/tinyvae.hip).  A companion of include/imh.h, which it
 * includes for the status codes and imh_dtype; conventions (pointers, streams, errors) as stated there. */
#ifndef IMH_TINYVAE_H_
#define IMH_TINYVAE_H_

#include "imh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the 3x3 conv of diffusers' AutoencoderTiny decoder (TAESD / TAESDXL): 64 channels wide, ReLU, no normalisation ------------------
 * One launch per conv; 35 launches decode a latent (head, 33 body convs, tail) and nothing runs in between: the ReLU, the block's skip,
 * the nearest x2 upsampling, the latent's tanh clamp and the image's layout all live in this entry.  Additive like imh_adapter_op and
 * imh_lora_merge: an entry and an argument struct of their own in this companion header; include/imh.h, every struct, enum and existing
 * entry stay as they were and the ABI stays at 13.  Not a plan kind: the decoder runs eagerly.
 * T = bf16 / fp16 (dtype).  Weights are packed [Cout, 9 Cin] in T, tap-major (tap = 3 ky + kx), Cin fastest: the project's conv packing.
 * All convs are 3 x 3, stride 1, zero padding 1; products are exact and accumulated in fp32 (v_mfma_f32_32x32x16_*).
 *   body (flags without HEAD / TAIL)
 *       x T NHWC [B, H, W, 64], w T [64, 576], bias T [64] or NULL, residual T NHWC [B, Ho, Wo, 64] or NULL -> y T NHWC [B, Ho, Wo, 64]:
 *       y = round_T(act((acc + bias) + residual)), fp32 throughout, one rounding; act = max(., 0) under IMH_TINYVAE_RELU (after the
 *       residual), else the identity.  Ho = H, Wo = W.
 *   IMH_TINYVAE_UP2  (body only) the conv reads the nearest x2 upsampling of x: virtual pixel (Y, X) is x[Y >> 1, X >> 1], Ho = 2 H,
 *       Wo = 2 W; nothing is materialised in memory (the nine taps are summed at the output resolution).
 *   IMH_TINYVAE_HEAD x is the fp32 NCHW latent [B, 4, H, W]; the kernel forms round_T(3.0f * tanhf(x / 3.0f)), then conv 4 -> 64 with
 *       w T [64, 36], + bias, ReLU (always; IMH_TINYVAE_RELU may be set or not) -> y T NHWC [B, H, W, 64].
 *   IMH_TINYVAE_TAIL x T NHWC [B, H, W, 64], w T [3, 576], bias T [3] or NULL -> y fp32 NCHW [B, 3, H, W] = 2 (acc + bias) - 1, not rounded
 *       to T: the image in the layout AutoencoderKL.decode returns.
 * Kernel form: persistent workgroups of eight waves (at most one per CU) hold the whole packed weight in LDS and walk tiles of 16 x 32
 *   output pixels; a tile's 18 x 34 input patch is staged in LDS with zeros outside the image (the next tile's patch is fetched into
 *   registers while this one is multiplied).  Every global access sits behind its bounds test; the same bits on every call.
 * Refused without a launch: null args / x / w / y; x, w, y, bias or residual not 16-byte aligned (HEAD: x, w and TAIL: y, bias to 4 resp. 2
 *   bytes: see below); y overlapping x or residual (y == residual included); HEAD or TAIL combined with each other, with IMH_TINYVAE_UP2
 *   or with a residual; TAIL with IMH_TINYVAE_RELU; unknown flag bits (IMH_ERR_ARG); B, H or W <= 0, an operand of 2^31 elements or
 *   more (IMH_ERR_SHAPE); another dtype (IMH_ERR_DTYPE).
 *   Alignment: body x / w / y / bias / residual 16 bytes; HEAD x 4, w 2, bias 16, y 16; TAIL x 16, w 16, bias 2, y 4.
 * Memory: reads the B H W 64 (HEAD: B 4 H W) elements of x, the Cout x 9 Cin elements of w, the Cout of bias, the B Ho Wo 64 of residual;
 *   writes the B Ho Wo 64 (TAIL: B 3 H W) elements of y.  Nothing else. */
#define IMH_TINYVAE_RELU 1
#define IMH_TINYVAE_UP2 2
#define IMH_TINYVAE_HEAD 4
#define IMH_TINYVAE_TAIL 8
typedef struct imh_tinyvae_args {
    const void* x;
    const void* w;
    const void* bias;        /* or NULL */
    const void* residual;    /* or NULL */
    void* y;
    int32_t B, H, W;         /* the input's extents (the output's are 2 H x 2 W under IMH_TINYVAE_UP2) */
    int32_t flags;
    int32_t dtype;
} imh_tinyvae_args;
int imh_tinyvae_conv(const imh_tinyvae_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMH_TINYVAE_H_ */
