/* imh_adapter.h -- the one entry of libimh_hip.so that the SDXL T2I-Adapter adds (csrc/adapter.hip).  A companion of include/imh.h, which it
 * includes for the status codes and imh_dtype; conventions (pointers, streams, errors) as stated there. */
#ifndef IMH_ADAPTER_H_
#define IMH_ADAPTER_H_

#include "imh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the T2I-Adapter's three passes that are not convs ------------------------------------------------------------------------------
 * diffusers T2IAdapter (adapter_type "full_adapter_xl"): PixelUnshuffle in front of conv_in, AdapterResnetBlock's ReLU, the down block's
 * AvgPool2d(2, 2, ceil_mode=True).  They run eagerly, once per control image; T = bf16 / fp16 (dtype).  Additive like imh_control_add: an
 * entry and an argument struct of its own, declared in this companion header (the declarations of include/imh.h are pinned and stay as
 * they were); no struct, enum or existing entry changes and the ABI stays at 13.  The entry is not a plan kind (imh_plan_add refuses 16 as
 * it refuses 12 and 14); should it become one, its kind is the #define 16.
 *   IMH_ADAPTER_UNSHUFFLE  x fp32 NCHW [N, C, H, W] -> y T NHWC [N, H / f, W / f, Cp]: output channel c f^2 + dy f + dx of pixel (y, x) holds
 *                          x[n, c, y f + dy, x f + dx] rounded once to T (torch: F.pixel_unshuffle(x, f).permute(0, 2, 3, 1).to(T), the same
 *                          bits); Cp >= C f^2 a multiple of 8, channels [C f^2, Cp) are written as zeros.  H % f == 0, W % f == 0.
 *   IMH_ADAPTER_RELU       y[i] = x[i] > 0 ? x[i] : 0 over n elements of T (NaN -> 0); y == x (in place) is allowed, a partial overlap is not.
 *   IMH_ADAPTER_AVGPOOL2   x T NHWC [N, H, W, C] -> y [N, ceil(H / 2), ceil(W / 2), C], C % 8 == 0: the window of an edge pixel holds its
 *                          in-bounds pixels only (no padding); fp32 sum in raster order of the window, times the exact reciprocal of the
 *                          count (1, 1/2, 1/4), one rounding to T: torch's (((a.float() + b.float()) + c.float()) + d.float()).mul(0.25).to(T)
 *                          and its two- and one-pixel forms, the same bits.
 * Refused without a launch: null args / x / y, an unknown mode, x or y not 16-byte aligned (unshuffle: x 4-byte aligned), y overlapping x
 * (relu: other than y == x) (IMH_ERR_ARG); a non-positive extent, f < 1, H % f, W % f, Cp % 8, Cp < C f^2, C % 8 (avgpool2), an operand of
 * 2^31 elements or more (IMH_ERR_SHAPE); another dtype (IMH_ERR_DTYPE).
 * Memory: reads the elements of x, writes the elements of y (Cp per pixel for unshuffle).  Nothing else. */
#define IMH_ADAPTER_UNSHUFFLE 0
#define IMH_ADAPTER_RELU 1
#define IMH_ADAPTER_AVGPOOL2 2
typedef struct imh_adapter_args {
    const void* x;
    void* y;
    int64_t n;               /* relu: elements */
    int32_t mode;
    int32_t N, C, H, W;      /* unshuffle: the image [N, C, H, W]; avgpool2: the input [N, H, W, C] */
    int32_t f, Cp;           /* unshuffle: the factor and the padded channel count of y */
    int32_t dtype;
} imh_adapter_args;
int imh_adapter_op(const imh_adapter_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMH_ADAPTER_H_ */
