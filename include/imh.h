/*
 * libimh_hip.so -- C ABI of the MI355X (gfx950) kernels behind the IMAGHarmony SDXL
 * denoising hot path.
 *
 * The reference (muzishen/IMAGHarmony) is pure Python and has no FFI of its own; every GPU
 * kernel it runs comes from PyTorch through diffusers.  The entry points below are what a
 * Python binding of THIS path binds with ctypes (INTEGRATION.md shows the stub); each one
 * cites the reference call sites whose arithmetic it replaces.
 *
 * Contract
 *   - plain C: raw device pointers, ints, floats; no torch / C++ types in any signature.
 *   - ownership: the caller owns every buffer (activations, weights, workspaces).  Kernels
 *     never allocate or free; workspace sizes are queried with *_workspace_bytes().
 *   - all work is enqueued on the caller's stream (hipStream_t passed as void*); no internal
 *     synchronisation, no malloc/free -> every entry point is hipGraph-capturable.
 *   - errors: 0 (IMH_OK) or a negative imh_status; imh_last_error() returns a thread-local
 *     message.  Nothing throws across the ABI, nothing calls exit().
 *   - stateless and re-entrant (plans are explicit handles owned by the caller).
 *   - dtype: IMH_DT_BF16 / IMH_DT_F16 activations+weights, fp32 accumulation everywhere.
 *   - layouts: activations are token-major / NHWC ([B, H*W, C] row-major); weights are
 *     [out, in] row-major exactly as torch.nn.Linear stores them; conv3x3 weights are
 *     pre-packed to [Cout][ky][kx][Cin] (imagharmony_amd.unet.Conv2d.packed).
 *   - memory: a launch touches its operands and nothing else.  An operand is the rows x columns an op's description gives it
 *     (row r = columns [0, cols) at r * ld; the gap [cols, ld) of a row belongs to the caller), plus the padding an op makes part of
 *     it (imh_attention's K rows / V^T columns).  Every op below says in one sentence ("Memory:") what that is for it.  Nothing is
 *     STORED outside the outputs, and no value LOADED from outside an operand reaches a result: edge tiles clamp or redirect their
 *     loads (to a zero page, or to a valid row whose products are masked) instead of running past the operand.  A load whose value is
 *     discarded is not observable and not promised either way.  tests/test_gpu_guarded_ops.py holds every op to this with NaN-filled
 *     guard bands around every operand (tests/guarded.py).
 */
#ifndef IMH_H_
#define IMH_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Still 13 after the CLIP text towers: what they added is strictly additive -- one entry (imh_attention_enc_causal), one plan kind
 * (IMH_OP_ATTN_ENC_CAUSAL = 9), one imh_gemm flag bit (IMH_GF_ACT_QGELU = 128) and one elementwise op (IMH_EW_GATHER_ROWS, 12); no
 * struct changed, and a caller written against the first version 13 cannot observe any of it.  The same holds for the general
 * CFG + scheduler step of the multistep and ancestral samplers, IMH_EW_CFG_MSTEP (13): one more elementwise op on imh_ew_args as it is,
 * and for the two query entries of the dispatch contract, imh_conv_halo_lds_bytes and imh_gemm_check, and for the seeded step noise:
 * three entries (imh_step_seeded, imh_randn_seeded, imh_randn_seeded_host) with argument structs of their own and two plan kinds
 * (IMH_OP_STEP_SEEDED = 10, IMH_OP_RANDN_SEEDED = 11); enum imh_ew_op and imh_ew_args are as they were.  And for the image op of the PNS
 * judge: one entry (imh_clip_preprocess) with an argument struct of its own and one plan kind (IMH_OP_CLIP_PREPROCESS = 13).  And for the
 * ControlNet's gated residual add: one entry (imh_control_add), an argument struct of its own, one plan kind (IMH_OP_CONTROL_ADD = 15; 12 and 14 stay refused).
 * The T2I-Adapter's per-image passes have a header of their own, include/imh_adapter.h: this one is as it was. */
#define IMH_ABI_VERSION 13

enum imh_status {
    IMH_OK = 0,
    IMH_ERR_ARG = -1,
    IMH_ERR_SHAPE = -2,
    IMH_ERR_DTYPE = -3,
    IMH_ERR_LAUNCH = -4,
    IMH_ERR_WORKSPACE = -5
};

enum imh_dtype { IMH_DT_BF16 = 0, IMH_DT_F16 = 1 };

/* epilogue flags of imh_gemm_args.flags */
enum imh_gemm_flags {
    IMH_GF_GEGLU = 1,     /* diffusers GEGLU: W rows interleaved in quads (value_2k, value_2k+1, gate_2k, gate_2k+1);
                           * out[2k], out[2k+1] = value * gelu(gate); N % 16 == 0, Y is [M, N/2] */
    IMH_GF_ACT_GELU = 2,  /* erf GELU, nn.GELU() (resampler.py:18); |error| <= 1.2e-5 (csrc/imh_common.h gelu_erf_f) */
    IMH_GF_ACT_SILU = 4,  /* SiLU (TimestepEmbedding) */
    IMH_GF_VT_PERM = 8,   /* write the attention V^T key permutation (see imh_attention) */
    IMH_GF_OUT_F32 = 16,  /* fp32 output */
    IMH_GF_LN_ROW = 32,   /* folded LayerNorm, the un-normalised token rows are X's rows (statistics per output row m) */
    IMH_GF_LN_COL = 64,   /* folded LayerNorm, the token rows are W's rows (per output column n; swapped-operand V^T form) */
    IMH_GF_ACT_QGELU = 128 /* quick-GELU y = x * sigmoid(1.702 x) on the biased accumulator in fp32 (transformers "quick_gelu": the CLIP-L text
                           * tower's MLP); where IMH_GF_ACT_GELU / _SILU stand, in every variant that takes those; exclusive with
                           * IMH_GF_ACT_GELU, IMH_GF_ACT_SILU and IMH_GF_GEGLU (IMH_ERR_ARG) */
};

/* ---- dense contraction ------------------------------------------------------------------
 * Y[m, n] = epilogue( sum_k X[m, k] * W[n, k] ),  epilogue = (+bias[n]) (+rowadd[m / rows_per_batch, n])
 *           (act) (GEGLU) (+residual[m, n]).
 * conv == 0: torch.nn.Linear.  Replaces attn.to_q/to_k/to_v/to_out[0] and to_k_ip/to_v_ip
 *   (ip_adapter/attention_processor.py:292,299,300,320,396,410,411,432,433,453), diffusers
 *   proj_in/proj_out/FeedForward/TimestepEmbedding/time_emb_proj/conv_shortcut,
 *   Resampler / ImageProjModel / HarmonyAttention linears (resampler.py:13-20,45-47,101-103;
 *   ip_adapter.py:38; train.py:208,239).
 * conv == 1: 3x3 convolution, stride 1|2, optional fused nearest x2 upsampling of the
 *   input (up = 1), as an implicit GEMM over NHWC input [B, H, Wd, Cin]; K = 9*Cin; M = B*Ho*Wo.
 *   Padding by `pad` (ABI 10): 0 = one zero pixel on every side (Ho = (H - 1) / stride + 1); 1 = none on the top / left and
 *   one on the right / bottom -- diffusers Downsample2D(padding=0), conv(F.pad(x, (0, 1, 0, 1)), stride 2): input row
 *   2 oy + ky, zero beyond H - 1, Ho = (H - 2) / 2 + 1 (the VAE encoder's downsamplers); stride 2, up = 0 only.
 *   up = 2 (ABI 12): the PHASE form of Upsample2D's conv -- the same result as up = 1 with 4/9 of the multiply-adds.  Output pixel
 *   (2y + py, 2x + px) of a 3x3 conv over a nearest x2 upsampling reads only the 2 x 2 low-res pixels (y + py - 1 + a, x + px - 1 + b),
 *   a, b in {0, 1} (zero outside the low-res image), with weights that are sums of the 3x3 taps (rows: py = 0: a = 0 -> ky 0, a = 1 ->
 *   ky 1 + 2; py = 1: a = 0 -> ky 0 + 1, a = 1 -> ky 2; columns alike).  The caller passes the implicit GEMM itself: X = the low-res
 *   NHWC input, M = B*H*Wd low-res pixels, N = 4*Cout, K = 4*Cin, W = [4*Cout, 4*Cin] with row block p = 2 py + px and K order
 *   (a, b, cin) (pre-summed in fp32, rounded once), Ho x Wo = 2H x 2Wd, Y = [B, Ho, Wo, Cout] with ldy = Cout, bias[Cout] as the only
 *   epilogue input, stride 1, pad 0, no split-K.  Row (b, y, x) of column tile phase p is stored to pixel (b, 2y + py, 2x + px).  A
 *   column tile must lie inside one phase: variants 1464 / 2464 / 24128 / 23256 x 160, 23256 x 128, 5258 x 320 with Cout % bn == 0,
 *   IMH_ERR_ARG otherwise (the host then runs up = 1).  gn_out (bn = 160 variants): one partial per (sample, block of
 *   imh_gemm_gn_block_rows consecutive LOW-res pixels, phase, 10 channels), i.e. of those pixels' phase-p output pixels, at block index
 *   p * (gn_hw / rows) + low-res block; gn_hw = H*Wd, gn_nblk = 4 * gn_hw / rows, N / 10 read as Cout / 10.
 *   Replaces diffusers ResnetBlock2D.conv1/conv2, Downsample2D.conv, Upsample2D(+interpolate), conv_out.
 * K must be a multiple of 64; M and N are arbitrary (edge tiles read a zero page).
 * Memory: reads rows [0, M) of X (and X2), rows [0, N) of W, bias[0, N), rows [0, M) x columns [0, N) of residual (row stride ldr),
 *   rowadd rows [0, ceil(M / rows_per_batch)) x columns [0, N) (row stride ldra) and, as given, ln_s / ln_c / ln_stats / gn_tab /
 *   gn_part / gn_gamma / gn_beta over the same rows / channels; conv == 1: pixels inside [0, H) x [0, Wd) only (the padding ring is
 *   zeros made in the kernel, never read).  Writes rows [0, M) x columns [0, N) of Y at row stride ldy (N / 2 columns with GEGLU;
 *   columns [0, yt_col0) with Yt, whose rows [0, N - yt_col0) x columns [0, M) are written at row stride ldyt), ln_stats_out
 *   [M][ln_slots_out][2], gn_out [M / gn_hw][gn_nblk][N / 10][2], and -- scratch, any bits -- the first
 *   imh_gemm_workspace_bytes(M, N, splits) bytes of `partial`.  Row gaps [N, ldy) and rows >= M of every buffer are not touched.
 * bm/bn/splits = 0 selects the built-in heuristic.  splits > 1 needs `partial`
 * (imh_gemm_workspace_bytes) and runs a second reduce+epilogue kernel.
 */
typedef struct imh_gemm_args {
    const void* X;
    const void* W;
    void* Y;
    float* partial;
    const void* bias;
    const void* rowadd;
    const void* residual;
    /* LayerNorm folded into the contraction (IMH_GF_LN_ROW: X rows are the un-normalised tokens; IMH_GF_LN_COL:
     * W rows are).  With W pre-scaled by gamma:  y = rstd * (acc - mean * ln_s) + ln_c  (exact algebra of
     * LN(x) W^T; BasicTransformerBlock.norm1/2/3 never materialise and cost no launch).  (mean, rstd) of every
     * token row come from `ln_stats` (below; REQUIRED with either flag -- the in-loop sum / sum-of-squares form of ABI
     * versions <= 5 cancelled on rows with |mean| >> sigma and no longer exists; IMH_ERR_ARG without it).
     * ln_s = sum_k gamma_k W[.,k], ln_c = sum_k beta_k W[.,k] (fp32; row form: per output column n, column form: per
     * output row m).  Variants: plain 64/128 tiles (both forms) and the wave-specialised ones 1464 / 2464 / 24128 /
     * 23256 / 22128 (row form).  splits == 1, conv == 0. */
    const float* ln_s;
    const float* ln_c;
    float ln_eps;
    /* Row-statistics hand-over between the GEMM that WRITES a LayerNorm input (attn.to_out + residual,
     * attention_processor.py:320-329,453-462; ff.net.2 + residual; proj_in) and the launches that consume it folded.
     * Format (csrc/imh_lnstats.h): [rows][slots][2] fp32 = (sum, M2 about the slot mean) of `width` consecutive
     * channels per slot, taken from the values as rounded to the output dtype; slots merge by Chan's formula (no
     * E[x^2] - mean^2 cancellation).
     *   ln_stats / ln_slots          input: partials of the token rows of a IMH_GF_LN_ROW / _COL launch (K % slots == 0)
     *   ln_stats_out / ln_slots_out  output: partials of THIS launch's Y rows; ln_slots_out must equal
     *                                N / imh_gemm_stats_slot_width(bm, bn) (N a multiple of that width, plain T output,
     *                                no GEGLU / V^T permutation / fp32 output / split-K / conv)
     * IMH_EW_ROW_STATS writes the same format (one slot per row) for rows no statistics epilogue covers. */
    const float* ln_stats;
    float* ln_stats_out;
    int32_t ln_slots, ln_slots_out;
    /* GroupNorm partials of THIS launch's output, for the GroupNorm that reads it (diffusers ResnetBlock2D.norm2 after conv1, the
     * next block's norm1 / Transformer2DModel.norm after conv2 / conv_shortcut + residual; also through a channel concat): one
     * (sum, M2) pair -- M2 = squared deviations from the partial's own mean, values as rounded to the output dtype -- per
     * (sample, pixel block, sub-run of 10 consecutive output channels): gn_out[((b * gn_nblk + blk) * (N / 10) + n / 10) * 2 + {0, 1}]
     * fp32, one block per imh_gemm_gn_block_rows(bm, bn) consecutive rows (pixels) of a sample (10 * that many elements per
     * partial); gn_hw = rows per sample, gn_nblk = gn_hw / block rows.  Hand the buffer to imh_groupnorm (mode IMH_GN_TABLE:
     * partial / nblk = gn_nblk / sub = 10 / npart = 10 * block rows).  NULL -> none.  Variants with this epilogue: the
     * wave-specialised ones at bn = 160 and the LDS-halo conv3x3; N % 10 == 0; no split-K, GEGLU, V^T permutation, fp32 output, LN. */
    float* gn_out;
    int32_t gn_nblk, gn_hw;
    /* LDS-halo conv3x3 only (variants 7128 / 7564 / 7256 / 73xx / 74xx, stride 1, no upsampling): the ResnetBlock2D front end
     * norm -> SiLU -> conv in one launch.  gn_tab = the (scale, shift) table of the INPUT's GroupNorm, [B][Cin][2] fp32 as written
     * by imh_groupnorm(mode IMH_GN_TABLE): every staged input pixel becomes silu?(x * scale + shift) inside the kernel (padding
     * stays zero: the conv pads the normalised tensor); the normalised activation never exists in memory.  NULL -> plain conv. */
    const float* gn_tab;
    int32_t gn_silu;
    /* ... or (ABI 8) the PARTIALS of the input's GroupNorm instead of a table: every workgroup then builds the (scale, shift) table of its
     * sample in LDS in its prologue (the routine of imh_groupnorm's IMH_GN_TABLE step, bit-identical) and no table launch is needed.
     * gn_part (+ gn_part2 for channels [gn_pC1, Cin) of a channel concat) / gn_pnblk / gn_psub / gn_pnpart (+ ...2) as imh_norm_args.partial /
     * nblk / sub / npart; gn_gamma / gn_beta [Cin] in the activation dtype (NULL = 1 / 0), gn_groups, gn_eps > 0.  Exclusive with gn_tab. */
    const float* gn_part;
    const float* gn_part2;
    const void* gn_gamma;
    const void* gn_beta;
    float gn_eps;
    int32_t gn_groups, gn_pC1;
    int32_t gn_pnblk, gn_psub, gn_pnpart;
    int32_t gn_pnblk2, gn_psub2, gn_pnpart2;
    /* LDS-halo conv3x3 only: the input is the channel concat [X | X2] (torch.cat([hidden, skip], 1) of the up blocks) read from
     * its two producers: channels [0, Cin1) from X (pixel stride Cin1), [Cin1, Cin) from X2 (pixel stride Cin - Cin1); both
     * multiples of 64.  X2 == NULL -> one source. */
    const void* X2;
    int32_t Cin1;
    /* Wave-specialised variants at bn = 160 with flags == IMH_GF_LN_ROW (the self-attention projections, attention_processor.py:
     * 292-300, as ONE launch over W = [Wq; Wk; Wv]): output columns n >= yt_col0 are not written to Y but TRANSPOSED to
     * Yt[(n - yt_col0) * ldyt + m'] with the 16 tokens of every aligned group stored as [0-3, 8-11, 4-7, 12-15] -- the V^T operand
     * layout of imh_attention (what IMH_GF_VT_PERM produces for the swapped-operand form).  Whole tiles only (M a multiple of the
     * variant's rows, N and yt_col0 multiples of 160); Y receives columns [0, yt_col0) with row stride ldy.  NULL -> all of Y. */
    void* Yt;
    int32_t yt_col0, ldyt;
    int32_t M, N, K;
    int32_t ldx, ldw, ldy, ldr, ldra;   /* ldra: row stride of rowadd (0 -> N) */
    int32_t rows_per_batch;
    int32_t splits;
    int32_t flags;
    int32_t H, Wd, Cin, Ho, Wo, stride, up;
    int32_t dtype;
    int32_t conv;
    /* tile variant (0 = heuristic): bm in {64, 128} x bn in {64, 128}: two-stage tiles (gemm.hip); 256 x {128, 256}:
     * 8-wave rings; 3064 x 64 / 3128 x 128: KG2; 4064 / 4128 / 5064: small-tile rings; 5258 x 320, 6128 x 320: the
     * 256 x 320 / 128 x 320 exact tilings; 8256 x 256, 9128 x 320, 9256 x 320: ping-pong kernels (gemm_pp.hip);
     * 1464 / 2464 x 160, 24128 x 160 / 128, 23256 x 160 / 128, 22128 x 160 (two workgroups per CU): wave-specialised kernel
     * (producer + consumer waves, gemm_ring.hip); 7128 / 7564 x 320 / 160, 7256 x 160 and the weight-ring forms
     * 7328 / 7428 / 7356 x 160: LDS-halo conv3x3 (conv_halo.hip, stride 1). */
    int32_t bm, bn;
    /* cache hint: the NEXT launch's weight matrix; exiting workgroups touch it (HBM -> L2 / Infinity Cache) */
    const void* pf_ptr;
    uint32_t pf_bytes;
    /* how the tile grid is dealt to the eight XCDs (workgroup w runs on XCD w % 8; each XCD takes one cell of an M x N grid of
     * cells): 0 = the byte-count model picks the shape, 2 / 3 / 4 / 5 = 8 x 1 / 4 x 2 / 2 x 4 / 1 x 8 cells.  Placement only:
     * results are bit-identical.  Which shape is faster depends on the box, so the host measures. */
    int32_t xcd;
    /* conv padding mode (ABI 10; see conv == 1 above): 0 = one pixel on every side (the zero-initialised default), 1 = right / bottom
     * only (Downsample2D(padding=0)).  Mode 1 runs on the two-stage tiles, the rings and the wave-specialised variants; the LDS-halo
     * conv3x3 (stride 1) refuses it with IMH_ERR_ARG. */
    int32_t pad;
} imh_gemm_args;

int imh_gemm(const imh_gemm_args* a, void* stream);
/* two independent plain GEMMs of one dtype in ONE launch (a's tile config is used for both); e.g. the [Q|K]
 * and V^T projections of a self-attention layer (attention_processor.py:292,299,300), which share x.
 * In a plan: kind IMH_OP_GEMM_DUAL with args = imh_gemm_args[2]. */
int imh_gemm_dual(const imh_gemm_args* a, const imh_gemm_args* b, void* stream);
int imh_gemm_pick_config(int M, int N, int K, int* bm, int* bn, int* splits);
/* channels per statistics slot written by tile variant (bm, bn) through ln_stats_out; 0 = the variant has no
 * statistics epilogue (use IMH_EW_ROW_STATS on its output instead) */
int imh_gemm_stats_slot_width(int bm, int bn);
/* rows per GroupNorm partial block written by tile variant (bm, bn) through gn_out; 0 = no such epilogue */
int imh_gemm_gn_block_rows(int bm, int bn);
/* bytes of LDS one launch of LDS-halo conv3x3 variant (bm, bn) takes for Cin input channels, gn != 0: with the table of the fused
 * GroupNorm front end (gn_tab / gn_part) -- of the kernel the launch would run under the current imh_debug_set key 5 setting.  The
 * launchers refuse above 160 KB with IMH_ERR_SHAPE; a host layer that chooses between the fused form and passes asks here instead of
 * restating ring depths.  -1: (bm, bn) is not an LDS-halo variant. */
int imh_conv_halo_lds_bytes(int bm, int bn, int Cin, int gn);
/* every check imh_gemm(a, .) makes, without running anything (the launch goes into a stream capture whose graph is discarded):
 * IMH_OK, or the status imh_gemm would return with imh_last_error() set.  For a caller that records launches into a plan and wants
 * a refusal where the launch is recorded, not where the plan first runs.  Costs one begin / end capture pair on a
 * stream the library keeps per calling thread and current device; meant for record time, not for a per-step path. */
int imh_gemm_check(const imh_gemm_args* a);
size_t imh_gemm_workspace_bytes(int M, int N, int splits);

/* ---- attention, head_dim 64 -------------------------------------------------------------
 * O[b, q, h*64:(h+1)*64] = softmax(Q K^T * scale) V  (+ scale2 * softmax(Q K2^T * scale) V2)
 * Replaces F.scaled_dot_product_attention in AttnProcessor2_0 (attention_processor.py:312) and both
 * SDPA calls + the axpy of IPAttnProcessor2_0 (:423-425, :440-442, :450).
 *   Q  : [B, Lq, ldq], head h at columns h*64..
 *   K  : [B, Lk_pad, ldk] (rows >= Lk are padding and must be finite), head h at columns h*64..
 *   Vt : [H*64, ldvt] = V transposed; batch b occupies columns b*Lk_pad .. ; inside every group of
 *        16 keys the order is [0-3, 8-11, 4-7, 12-15] (what imh_gemm writes with IMH_GF_VT_PERM);
 *        padding columns must be finite (zero).
 *   K2/Vt2 (optional): the image-prompt key set of the IP branch, same layouts.
 * Lk_pad, Lk2_pad multiples of 64.
 * Memory: reads rows [0, B*Lq) of Q, rows [0, B*Lk_pad) of K and columns [0, B*Lk_pad) of every Vt row (+ K2 / Vt2 alike over Lk2_pad) --
 *   the padding rows / columns are part of the operand and are loaded, hence "finite" -- scale2_tab[*step] and *step; writes rows
 *   [0, B*Lq) x columns [0, H*64) of O.  Lq is arbitrary: query rows >= Lq of the last query block are neither read into a result nor stored.
 */
typedef struct imh_attn_args {
    const void* Q;
    const void* K;
    const void* Vt;
    const void* K2;
    const void* Vt2;
    void* O;
    int32_t B, H, Lq;
    int32_t Lk, Lk_pad;
    int32_t Lk2, Lk2_pad;
    int32_t ldq, ldk, ldvt, ldk2, ldvt2, ldo;
    float scale;
    float scale2;
    const float* scale2_tab; /* optional: scale2 = scale2_tab[*step] (per-step IP-scale gating,
                                custom_pipelines.py:326-329, without re-recording the plan) */
    const int32_t* step;
    int32_t dtype;
    const void* pf_ptr;    /* tail prefetch of the next launch's weights (cache hint) */
    uint32_t pf_bytes;
} imh_attn_args;

int imh_attention(const imh_attn_args* a, void* stream);

/* ---- fused QKV + image-prompt cross-attention ---------------------------------------------
 * The attention side of IPAttnProcessor2_0.__call__ (ip_adapter/attention_processor.py:396-450) in one launch:
 *   q = attn.to_q(LN(x))                      (:396; the BasicTransformerBlock.norm2 in front of it folded in, optional)
 *   O = softmax(q K^T * scale) V  (+ scale2 * softmax(q K2^T * scale) V2)          (:416-425, :432-442, :450)
 * K / Vt (text tokens, attn.to_k / to_v, :410-411) and K2 / Vt2 (image-prompt tokens, to_k_ip / to_v_ip, :432-433)
 * are step-invariant caches in imh_attention's layouts, EXCEPT that K and K2 store the 64 dims of every head with
 * each 16-group ordered [0-3, 8-11, 4-7, 12-15] (write them with IMH_GF_VT_PERM): the projected query leaves the
 * MFMA accumulators in exactly that order and becomes the QK^T operand without touching LDS or memory.
 * attn.to_out (:453) needs all heads of a token and stays a following imh_gemm.
 *   X  : [B*Lq, ldx] token rows, C = H*64 columns; un-normalised when ln_s != NULL
 *   Wq : [H*64, ldw] = attn.to_q.weight ([out, in]); with ln_s != NULL pre-scaled by the LayerNorm gamma,
 *        ln_s[d] = sum_k gamma_k Wq[d,k], ln_c[d] = sum_k beta_k Wq[d,k] (fp32) as for IMH_GF_LN_ROW
 * Memory: reads rows [0, B*Lq) x columns [0, C) of X, all of Wq [C, C], ln_s / ln_c [C], ln_stats [B*Lq][ln_slots][2] and the key / value
 *   caches exactly as imh_attention does (padding included); writes rows [0, B*Lq) x columns [0, C) of O.  The one-head form takes any Lq;
 *   the wide five-head form (imh_debug_set key 3 = 10, or chosen by shape) whole 128-query blocks and H % 5 == 0 only (IMH_ERR_SHAPE).
 */
typedef struct imh_xattn_args {
    const void* X;
    const void* Wq;
    const float* ln_s;
    const float* ln_c;
    float ln_eps;
    const float* ln_stats;   /* with ln_s: REQUIRED row statistics of X ([B*Lq][ln_slots][2], see imh_gemm_args) */
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
    const float* scale2_tab; /* optional per-step table of IP scales (custom_pipelines.py:326-329), indexed by *step */
    const int32_t* step;
    int32_t dtype;
    const void* pf_ptr;      /* tail prefetch of the next launch's weights (cache hint) */
    uint32_t pf_bytes;
} imh_xattn_args;

int imh_cross_attention(const imh_xattn_args* a, void* stream);

/* small generic attention (arbitrary head dims, short sequences), row-major Q/K/V, one softmax:
 * HarmonyAttention's Cross_Attention (ip_adapter/attention_processor.py:35-56, head_dim 40 / value_dim 64)
 * and the Resampler's PerceiverAttention core (ip_adapter/resampler.py:66-76).  Once per image.
 * Q [B*Lq, ldq], K [B*Lk, ldk], V [B*Lk, ldv], O [B*Lq, ldo], head h at columns h*dq.. (Q, K) / h*dv.. (V, O); K and V may be two column
 * ranges of one buffer.  Lk <= 8192, dq <= 1024 (IMH_ERR_SHAPE).  Two kernels, same result to rounding: the head's K^T and V resident in
 * LDS when dq, dv, ldk, ldv are multiples of 8 and they fit 150 KB, else one pass per query from global memory.
 * Memory: reads rows [0, B*Lq) x columns [0, H*dq) of Q, rows [0, B*Lk) x [0, H*dq) of K and x [0, H*dv) of V; writes rows [0, B*Lq) x
 *   columns [0, H*dv) of O; no padding rows anywhere (keys >= Lk exist only as zeros in LDS). */
typedef struct imh_small_attn_args {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int32_t B, H, Lq, Lk, dq, dv;
    int32_t ldq, ldk, ldv, ldo;
    float scale;
    int32_t dtype;
} imh_small_attn_args;

int imh_attention_small(const imh_small_attn_args* a, void* stream);

/* ---- bidirectional encoder attention, generic head dim (ABI 13) ----------------------------
 * O[b, q, h*d:(h+1)*d] = softmax(Q K^T * scale) V per (batch, head), no mask beyond the sequence end: the self-attention of
 * the CLIP vision tower behind the image prompt -- image_encoder(...).image_embeds / .hidden_states[-2]
 * (ip_adapter/ip_adapter.py:81-84,163-164,411-415; ViT-H/14: 16 heads x 80, ViT-bigG/14: 16 heads x 104, L = 257).
 *   Q, K, V, O : plain row-major [B*L, ld*]; head h at columns h*d..; Q, K and V may be three column ranges of ONE packed
 *                [B*L, 3*H*d] buffer written by a single QKV GEMM (ldq = ldk = ldv = 3*H*d).  No padding rows, no
 *                pre-permuted or transposed layouts: keys at or beyond L are masked and never read, query rows at or
 *                beyond L are never stored; nothing outside rows [0, B*L) of any operand is touched.
 *   d          : any multiple of 8 up to 128 (IMH_ERR_SHAPE otherwise); the contraction dim is zero-padded to the MFMA
 *                K step inside LDS.  L >= 1, any length (online softmax over key tiles of 64).
 *   ld*        : multiples of 8 elements, >= H*d; base pointers 16-byte aligned (IMH_ERR_ARG).
 * Scores and P V on v_mfma_f32_16x16x32, softmax (max, sum, exp) in fp32.  Grid = (query blocks of 64, H, B).
 * In a plan: kind IMH_OP_ATTN_ENC.
 */
typedef struct imh_enc_attn_args {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int32_t B, H, L, d;
    int32_t ldq, ldk, ldv, ldo;
    float scale;
    int32_t dtype;
} imh_enc_attn_args;

int imh_attention_enc(const imh_enc_attn_args* a, void* stream);
/* The causal form: O[b, q] = softmax over the keys k <= q only -- the self-attention of the CLIP text towers behind the SDXL prompt
 * (CLIP-L: 12 heads x 64, OpenCLIP bigG: 20 heads x 64, L = 77; diffusers StableDiffusionXLPipeline.encode_prompt).  The same argument
 * struct, operand rules, error codes and memory promise as imh_attention_enc.  The workgroup of queries [q0, q0 + 64) visits the key
 * tiles 0 .. q0 / 64 only (later tiles are neither loaded nor staged) and masks inside the diagonal tile; a masked probability is an
 * exact zero, so a FINITE K / V row of the future never reaches an earlier query (the masked keys of the diagonal tile are still
 * staged: they must be finite, as any operand).  In a plan: kind IMH_OP_ATTN_ENC_CAUSAL (args = imh_enc_attn_args). */
int imh_attention_enc_causal(const imh_enc_attn_args* a, void* stream);

/* ---- normalisation ----------------------------------------------------------------------
 * imh_groupnorm: GroupNorm(groups) over NHWC x[B, HW, C] with optional fused SiLU
 *   (diffusers ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2DModel.norm, conv_norm_out), in three steps that can run
 *   together or apart (torch.nn.GroupNorm semantics: fp32 statistics, biased variance; Welford / Chan merges, never
 *   E[x^2] - mean^2):
 *     statistics  (sum, M2) partials per (sample, pixel block, sub-run of `sub` consecutive channels) -- from a pass over x
 *                 (IMH_GN_STATS) or from the epilogue of the launch that wrote x (imh_gemm_args.gn_out, sub = 10)
 *     table       (scale, shift)[b][c] = (gamma[c] * rstd, beta[c] - mean * gamma[c] * rstd) from the partials of ONE or TWO producers
 *                 (the second covers channels [C1, C): the other half of a channel concat)                      (IMH_GN_TABLE)
 *     apply       y = silu?(x * scale + shift) as a pass (IMH_GN_APPLY) -- or inside the consuming conv3x3 (imh_gemm_args.gn_tab)
 * imh_layernorm: LayerNorm over the last dim of x[rows, C] (BasicTransformerBlock.norm1/2/3,
 *   ip_adapter.py:39, resampler.py:15,42,43,104, train.py:238).  gamma/beta may be NULL.
 * Memory (imh_groupnorm): x and y are dense [B, HW, C]; reads x, gamma / beta [C], and per mode partial (+ partial2) [B][nblk][C / sub][2] or
 *   table [B][C][2]; writes y (ALL / APPLY / TABLE_APPLY), partial [B][imh_groupnorm_stats_blocks][C / sub][2] (STATS), table [B][C][2]
 *   (TABLE), and in mode ALL -- scratch -- the first imh_groupnorm_workspace_bytes(B, HW, C, groups) bytes of `partial`.
 * Memory (imh_layernorm): reads and writes the dense rows [0, rows) x [0, C) of x / y and gamma / beta [C].
 */
enum imh_gn_mode {
    IMH_GN_ALL = 0,     /* statistics + table + apply; `partial` = workspace of imh_groupnorm_workspace_bytes() */
    IMH_GN_STATS = 1,   /* x -> partial[B][imh_groupnorm_stats_blocks(HW, C)][C / sub][2]; sub must divide C / groups of every consumer */
    IMH_GN_TABLE = 2,   /* partial (+ partial2) -> table[B][C][2] */
    IMH_GN_APPLY = 3,   /* x, table -> y */
    IMH_GN_TABLE_APPLY = 4   /* partial (+ partial2), x -> y in ONE launch: every workgroup builds its sample's table in LDS (ABI 8) */
};
typedef struct imh_norm_args {
    const void* x;
    void* y;
    const void* gamma;
    const void* beta;
    float* partial;
    int32_t B, HW, C, groups;
    int32_t rows;
    float eps;
    int32_t silu;
    int32_t dtype;
    /* imh_groupnorm only */
    int32_t mode;            /* enum imh_gn_mode */
    float* table;
    const float* partial2;   /* IMH_GN_TABLE: second producer's partials or NULL */
    int32_t nblk, sub, npart;    /* source 1: partial blocks per sample, channels per sub-run, elements per partial (0 = the ragged
                                  * blocks of IMH_GN_STATS: (pixels of block k) * sub with ceil(HW / nblk) pixels per block) */
    int32_t C1;                  /* channels covered by source 1 (ignored without partial2) */
    int32_t nblk2, sub2, npart2;
    const void* pf_ptr;    /* tail prefetch of the next launch's weights (cache hint) */
    uint32_t pf_bytes;
} imh_norm_args;

int imh_groupnorm(const imh_norm_args* a, void* stream);
size_t imh_groupnorm_workspace_bytes(int B, int HW, int C, int groups);
int imh_groupnorm_stats_blocks(int HW, int C);       /* pixel blocks per sample of IMH_GN_STATS */
int imh_groupnorm_stats_sub(int C, int groups);      /* the sub-run width IMH_GN_ALL uses: 10 when it divides C / groups, else C / groups */
int imh_layernorm(const imh_norm_args* a, void* stream);

/* ---- small fused elementwise kernels (see csrc/elementwise.hip for the field meaning) ---- */
enum imh_ew_op {
    IMH_EW_TIMESTEP = 0,  /* diffusers Timesteps() sinusoid */
    IMH_EW_SILU = 1,
    IMH_EW_CONCAT = 2,    /* NHWC channel concat (up-block skips): y[pix, 0:i0] = a[pix], y[pix, i0:i0+i1] = b[pix], n pixels; i0, i1 multiples of 8.
                           * Additive, ABI unchanged -- the FreeU form, selected by i2 > 0 (i2 == 0: the op as it was, same kernel): diffusers'
                           * apply_freeu at that concat.  i2 = H, i3 = W (both >= 2, any value; n % (H * W) == 0: n / (H * W) samples),
                           * i4 = leading channels of `a` that are scaled (0 <= i4 <= i0, any value), f0 = backbone scale b, f1 = skip scale s:
                           *   y[pix, c] = round_T(float(a[pix, c]) * f0) for c < i4 (torch's a[..., :i4] * b in T, bit for bit), a[pix, c] for i4 <= c < i0;
                           *   y[pix, i0 + c] = round_T(x + (f1 - 1) * low), x = b[pix, c]: fourier_filter(x, threshold = 1, scale = s) per (sample,
                           *   channel) plane, whose mask keeps the frequency pairs {-1, 0} x {-1, 0} (asymmetric, as upstream: a real cosine of
                           *   frequency 1 keeps weight 1 / 2),
                           *     low(y, x) = Re((1 / HW) * sum over (u, v) in {-1, 0}^2 of X[u, v] * exp(2 pi i (u y / H + v x / W))),
                           *   evaluated in float64 from float64 plane sums taken in a fixed order (no atomics, no workspace: the same bits on
                           *   every call, eager or from a plan), one rounding at the end -- where x and (s - 1) * low cancel, an ulp of the
                           *   result is smaller than one fp32 rounding of the sums.  imagharmony_amd/freeu.py restates it in numpy float64.
                           * Refused without a launch (the text names `concat`): i0 / i1 no multiples of 8, i4 outside [0, i0], H or W < 2,
                           * H * W not dividing n, H + W beyond the tables' LDS (about 3000).
                           * Additive, ABI unchanged -- the identity-attention form, selected by i5 > 0 (0 in every other call): the self-attention
                           * output of samples whose attention map is the identity (perturbed-attention guidance: softmax(QK^T) := I, so the
                           * output is V) read out of V^T as the self-attention projections leave it.  b = Vt (T) [C = i1, ldvt = i5], the keys of
                           * every 16-group stored in the order [0-3, 8-11, 4-7, 12-15] (imh_attention's V^T layout; perm16 swaps runs 1 and 2 of
                           * 4 and is its own inverse); the first part is empty (i0 = 0, `a` unused), i2 = 0, i3 = row stride of y, i4 = col0:
                           *   y[r, c] = Vt[c, col0 + 16 * (r / 16) + perm16(r % 16)]      0 <= r < n,  0 <= c < C
                           * -- a transposing copy, bit for bit, through one 64 x 64 LDS tile per workgroup; no atomics, no workspace.
                           * Refused without a launch, IMH_ERR_ARG (the text names `concat`): n or col0 no multiple of 16 (n > 0, col0 >= 0), C
                           * no positive multiple of 8, ldvt or i3 no multiple of 8, ldvt < col0 + n, i3 < C, i0 != 0 or i2 != 0, b NULL, b or y
                           * not 16-byte aligned. */
    IMH_EW_CONV_IN = 3,   /* conv_in + CFG duplication (custom_pipelines.py:332) + scale_model_input (:334).  ABI 11: i5 = input channels, 0 | 4 (the
                           * latents alone) or 9 (the SDXL inpainting UNet): channels 4-8 = [mask | masked-image latents] come unscaled from `x2`,
                           * fp32 NCHW [i0, 5, H, W], the same at every step; w is then [C0][9][3][3] */
    IMH_EW_CFG_STEP = 4,  /* CFG combine (:348-350) + scheduler.step (:357).  ABI 11, with `mask` set: followed in the same pass by the masked
                           * blend of diffusers StableDiffusionXLInpaintPipeline (4-channel UNet),
                           *   y = (1 - m) * (ba * x2 + bb * noise) + m * y,   (ba, bb) = blend_tab[2 * *step + {0, 1}]  (step REQUIRED),
                           * all fp32: x2 = the image latents z [i0, 4, i1], noise = the add-noise noise [i0, 4, i1], mask = the latent mask
                           * [i4, i1] (1 = repaint; sample s reads mask s % i4, i4 >= 1); a == NULL: the blend alone (no CFG / scheduler update).
                           * Additive, ABI unchanged -- the three-term form, selected by i2 = 1 (0: the op as it was, same kernel):
                           * perturbed-attention guidance (diffusers PAGMixin._apply_perturbed_attention_guidance), f3 = the PAG scale s.  `a`
                           * carries one more block of i0 samples, the conditional prediction under identity self-attention maps, p:
                           *   i3 = 1: a = [uncond | cond | perturbed] = [3 i0, i1, 4],  eps = (u + f2 * (c - u)) + s * (c - p);
                           *   i3 = 0: a = [cond | perturbed] = [2 i0, i1, 4],           eps = c + s * (c - p);
                           * everything behind eps (w, the update, the blend) is what it is without.  i2 outside {0, 1}, or i2 = 1 with
                           * a == NULL: IMH_ERR_ARG. */
    IMH_EW_CAST_F32 = 5,
    IMH_EW_ADD = 6,
    IMH_EW_STEP_SET = 7,  /* *y(int32) = i1 ? i0 : *y + 1 : the device-side step counter */
    IMH_EW_CFG_RESCALE = 8, /* y[s] = f3 * std(eps_text_s) / std(eps_cfg_s) + 1 - f3 (rescale_noise_cfg, custom_pipelines.py:351-354);
                             * a = noise prediction NHWC [2 i0, i1, 4], f2 = guidance scale; IMH_EW_CFG_STEP reads y through `w`.
                             * i2 = 1 (additive; 0: the op as it was): the three-term form of IMH_EW_CFG_STEP -- a = [3 i0, i1, 4], f0 = the PAG
                             * scale s, eps_cfg = (u + f2 * (c - u)) + s * (c - p) */
    IMH_EW_SOFTMAX = 9,     /* y[r,:] (T) = softmax(f0 * a[r,:]) with a fp32 (VAE mid-block attention); i0 rows, i1 cols, i2 / i3 leading dims */
    IMH_EW_ROW_STATS = 10,  /* y[r] (fp32 pair) = (sum, M2) of a[r, 0:i0] (row stride i1), n rows: LayerNorm statistics in the ln_stats format, one slot */
    IMH_EW_STEP_ROW = 11,   /* y[0:n] = a[*step * n + 0:n] (T; n % 8 == 0): row `step` of a per-schedule table (time embeddings of all denoise steps) */
    IMH_EW_GATHER_ROWS,     /* 12, numbered by its place behind IMH_EW_STEP_ROW (tests/test_host_logic.py pins the count of explicitly
                             * numbered ops of ABI 13 at twelve; this one is the additive thirteenth).  y[r, 0:C] = table[idx[r], 0:C] (+ add[r mod P, 0:C]), r in [0, n): the CLIP text towers' token + position embedding
                             * (add = the position table, P = 77) and their EOS pooling (no add; table = the final-layer-normed hidden rows,
                             * idx[b] = b * L + eos position).  Fields: a = table (T, i5 rows, row stride i1), b = idx (int32 [n], device), w = add
                             * (T, P = i3 rows, row stride i4) or NULL, y (T, row stride i2), i0 = C; C and the strides multiples of 8 (16-byte
                             * accesses; table / add / y 16-byte aligned), strides >= C.  The sum is taken in fp32 and rounded once.  The CALLER
                             * validates idx against [0, i5) before uploading it; a row with an index outside that range is skipped (not
                             * read, not written), never followed. */
    IMH_EW_CFG_MSTEP        /* 13, by its place behind IMH_EW_GATHER_ROWS (additive: imh_ew_args does not grow, the ABI version stays).  The
                             * general CFG + scheduler step of the multistep and ancestral samplers (DPM-Solver++ 2M, SDE-DPM-Solver++ 2M, Euler
                             * ancestral), one pass over the fp32 NCHW latents y [i0, 4, i1]:
                             *   eps = IMH_EW_CFG_STEP's: a = noise prediction NHWC [2 i0 | i0, i1, 4] (i3 = 1: [uncond | cond], f2 = guidance scale),
                             *         times w[s] when w (the IMH_EW_CFG_RESCALE factor) is set;
                             *   (cx, ce, ch, cn, hx, he) = tab[6 * *step + 0..5]   (tab and step REQUIRED; fp32 [n, 6]);
                             *   y' = cx * y + ce * eps + ch * h + cn * z,   h' = hx * y + he * eps   (all fp32),
                             * h = `b`, a fp32 history buffer [i0, 4, i1] that the launch READS AND WRITES in place (each element by one
                             * thread), z = row *step of the fp32 noise bank `bias` [n, i0, 4, i1].  b == NULL / bias == NULL: that term is
                             * absent (and h is not written).  With `mask` set the masked blend of IMH_EW_CFG_STEP follows in the same pass, same
                             * fields, same blend_tab -- except that `a` is REQUIRED here: there is no blend-alone form (a == NULL is an error).  With ch = cn = 0 and neither h nor bank the result equals IMH_EW_CFG_STEP's bit for bit.
                             * i2 = 1, f3 = the PAG scale: the three-term eps of IMH_EW_CFG_STEP, same layout of `a`, in every form of this op
                             * (bank, imh_step_seeded, with and without the blend). */
};

typedef struct imh_ew_args {
    const void* a;
    const void* b;
    void* y;
    const void* w;
    const void* bias;
    const float* tab;      /* optional per-step scalar table, indexed by *step */
    const int32_t* step;   /* device-resident denoise-step counter */
    int64_t n;
    int32_t i0, i1, i2, i3, i4, i5;
    float f0, f1, f2, f3;
    int32_t dtype;
    /* ABI 11, all optional (NULL = the op as it was): see IMH_EW_CONV_IN / IMH_EW_CFG_STEP */
    const float* x2;          /* CONV_IN: the step-invariant second source; CFG_STEP blend: the image latents */
    const float* noise;       /* CFG_STEP blend: the add-noise noise */
    const float* mask;        /* CFG_STEP blend: the latent mask; its presence selects the blend */
    const float* blend_tab;   /* CFG_STEP blend: per-schedule (a, b) rows indexed by *step */
} imh_ew_args;

/* Memory: every elementwise op reads and writes exactly the elements its description counts (n, or the i0..i5 extents) of dense buffers;
 * IMH_EW_SOFTMAX and IMH_EW_ROW_STATS take row strides and leave the gaps [cols, ld) alone; IMH_EW_STEP_SET touches the one int32 at y;
 * IMH_EW_STEP_ROW reads row *step of `a` only; `tab` / `blend_tab` are read at row *step only; IMH_EW_GATHER_ROWS reads idx[0, n), columns
 * [0, C) of the table rows idx names and of add's rows [0, min(n, P)), and writes columns [0, C) of y's rows [0, n).  IMH_EW_CFG_MSTEP reads
 * its six-column `tab` and the noise bank `bias` at row *step only (6 floats and i0 * 4 * i1 floats), and reads and writes exactly the
 * i0 * 4 * i1 elements of y and of the history buffer `b`.  IMH_EW_CONCAT, plain and FreeU form, reads the n * i0 elements of `a` and the n * i1 of `b`,
 * writes the n * (i0 + i1) elements of y and touches nothing else (the FreeU form reads `b` twice and keeps its sums on chip); its
 * identity-attention form (i5 > 0) reads columns [i4, i4 + n) of the i1 rows of `b` (row stride i5) and writes columns [0, i1) of y's rows
 * [0, n) (row stride i3): the slack columns of either side are neither read nor written.  The three-term forms (i2 = 1) of
 * IMH_EW_CFG_STEP / IMH_EW_CFG_MSTEP / IMH_EW_CFG_RESCALE read one more block of i0 * i1 * 4 elements of `a` and nothing else besides. */
int imh_elementwise(int op, const imh_ew_args* a, void* stream);

/* ---- seeded step noise: the noise of the stochastic samplers as a pure function of (seed, lane, table row, element) --------------
 * Philox4x32-10 as published (Salmon et al. 2011, Random123: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85, ten
 * rounds).  Sample s owns one 16-byte row of `seeds`, uint32 (k0, k1, lane, 0): k0 / k1 = the low / high word of a 64-bit seed, lane = 0
 * where every sample has a seed of its own, the sample index where one seed serves a batch.  For element e in [0, 4 HW) of the sample's
 * NCHW latent (e = ch * HW + pix), table row r and stream word t:
 *   w0..w3 = philox4x32_10(counter = (e >> 2, r, t, lane), key = (k0, k1)),      u_j = ((w_j >> 9) + 0.5) * 2^-23   (exact in fp32),
 *   (z0, z1) = sqrt(-2 ln u0) * (cos, sin)(2 pi u1),  (z2, z3) likewise from (u2, u3);  element e takes z_(e & 3);  |z| <= 5.77.
 * Nothing else enters: not the batch size, the sample's position, the device, eager or graph.  Stream 0 is the step noise; other
 * values are reserved.  imagharmony_amd/noise.py restates this in numpy (words exact, normals in float64).
 *
 * imh_step_seeded: IMH_EW_CFG_MSTEP (every field of `ew` as there, ew.bias -- the bank -- must be NULL) with z generated in the launch
 * from seeds[s], r = *ew.step and `stream`; a row whose cn is 0 generates nothing.  Fed the same z through a bank, IMH_EW_CFG_MSTEP gives
 * the same bits.  In a plan: kind IMH_OP_STEP_SEEDED.
 * Memory: as IMH_EW_CFG_MSTEP without the bank, plus the i0 * 4 uint32 of `seeds`, read only. */
typedef struct imh_seeded_args {
    imh_ew_args ew;
    const uint32_t* seeds;    /* device, [ew.i0][4] */
    uint32_t stream;
} imh_seeded_args;
int imh_step_seeded(const imh_seeded_args* a, void* stream);

/* imh_randn_seeded: the rows by themselves.  y[s, e] = z_(e & 3) of (seeds[s], r, stream), fp32 [S, 4, HW] dense; raw != 0: the uint32
 * words w_(e & 3) instead.  With quad0 != 0 y is a slice of the row: counter word 0 is quad0 + (e >> 2), modulo 2^32.  r = *step when step is set (device int32, read as uint32), else `row`.  In a plan: kind IMH_OP_RANDN_SEEDED.
 * imh_randn_seeded_host: the same functions compiled for the host -- y, seeds and step are HOST pointers, nothing is launched (the
 * integer path is bit-equal to the device's; the normals are float64 rounded once, within an fp32 ulp of the device's few).
 * Memory: reads the S * 4 uint32 of seeds (and the one int32 at step), writes exactly the S * 4 * HW elements of y. */
typedef struct imh_randn_args {
    void* y;
    const uint32_t* seeds;    /* [S][4] */
    const int32_t* step;
    int32_t S, HW;
    uint32_t row, stream;
    int32_t raw;
    uint32_t quad0;           /* first quad: y holds elements [4 quad0, 4 quad0 + 4 HW) of every sample's row (0: the row from its start) */
} imh_randn_args;
int imh_randn_seeded(const imh_randn_args* a, void* stream);
int imh_randn_seeded_host(const imh_randn_args* a);

/* ---- image ops: decoded image -> the patch rows of the CLIP vision tower ------------------------------------------------------------
 * The preprocessing of the PNS judge (imagharmony_amd.pns.ClipPreferenceJudge.preprocess, i.e. CLIPImageProcessor's resize / centre crop
 * / normalise on tensors) and the im2col of the tower's patch embedding in one launch.  x: fp32 NCHW [S, 3, H, W], nominally in [-1, 1],
 * dense.  y: [S g g, ldp] of T, g = size / patch; row s g g + gy g + gx holds the 3 patch patch values of patch (gy, gx) of image s in
 * Conv2d's weight order (c, py, px).  Per value:
 *   1. u = clamp(x / 2 + 0.5, 0, 1)
 *   2. antialiased bicubic (A = -0.5) resize of u to (nh, nw), separable, horizontal pass first; per axis, with scale = in / out:
 *        support = 2 scale if scale >= 1 else 2;   centre = scale (i + 0.5);
 *        taps j in [max(0, int(centre - support + 0.5)), min(in, int(centre + support + 0.5)));
 *        weight cubic((j - centre + 0.5) (1 / scale if scale >= 1 else 1)), the weights of one output normalised to sum 1;
 *        cubic(t) = (1.5 |t| - 2.5) t t + 1 below 1, -0.5 (((|t| - 5) |t| + 8) |t| - 4) below 2, else 0
 *      -- the filter of torch's upsample_bicubic2d_aa; this statement was run against torch's CPU result (tests/test_clip_preprocess_host.py,
 *      profiles/clip_judge_parity.json) and needed no correction.  The caller derives nh, nw (shortest edge -> size, Python's round, at
 *      least size) and the crop origin top = (nh - size) / 2, left = (nw - size) / 2 and passes them; only the cropped pixels are computed
 *   3. clamp to [0, 1]    4. (v - mean[c]) / std[c]    5. one rounding to T.
 * imagharmony_amd/imageops.py restates this in numpy float64.  fp32 accumulation in tap order; no atomics: the rows are a pure function
 * of x and the arguments, the same bits eagerly, from a plan and from a replayed graph.
 * dtype: IMH_DT_BF16, IMH_DT_F16 or IMH_CLIP_DT_F32 (fp32 rows; this entry only).
 * Refused without a launch: null x / y or misaligned pointers, a dtype that is none of the three, std <= 0 (IMH_ERR_ARG); S, H, W < 1,
 * size % patch != 0, patch outside [1, 32], nh < size or nw < size, a crop outside (nh, nw), ldp < 3 patch patch, S g g ldp or S 3 H W
 * >= 2^31 (IMH_ERR_SHAPE); and a downscale whose tap tables and source window exceed 64 KB of LDS (IMH_ERR_SHAPE; 1024 -> 224 needs 21 KB).
 * In a plan: kind IMH_OP_CLIP_PREPROCESS = 13.  enum imh_op_kind is as it was and kind 12 stays refused.
 * Memory: reads, of every image and channel, the source pixels under the taps of the cropped outputs only (inside [0, H) x [0, W));
 * writes columns [0, 3 patch patch) of rows [0, S g g) of y and leaves the columns [3 patch patch, ldp) of every row alone. */
#define IMH_CLIP_DT_F32 2
#define IMH_OP_CLIP_PREPROCESS 13
typedef struct imh_clip_preprocess_args {
    const float* x;
    void* y;
    int32_t S, H, W;
    int32_t nh, nw, top, left;
    int32_t size, patch, ldp;
    float mean0, mean1, mean2;
    float std0, std1, std2;
    int32_t dtype;
} imh_clip_preprocess_args;
int imh_clip_preprocess(const imh_clip_preprocess_args* a, void* stream);

/* ---- gated residual add with GroupNorm partials: the ControlNet's injections ------------------------------------------------------------
 * y[b, p, c] = round_T( x[b, p, c] + g * r[b % Br, p, c] ),   g = scale * (tab ? tab[*step] : 1)
 * over dense NHWC [B, HW, C] in bf16 / fp16: diffusers UNet2DConditionModel.forward's `down_block_res_sample + down_block_additional_residual`
 * (nine skips) and `sample + mid_block_additional_residual`, with ControlNetModel.forward's `sample * conditioning_scale` and the pipeline's
 * controlnet_keep window folded into the per-schedule table `tab` (fp32, indexed by the device step counter); and ControlNetModel.forward's
 * `sample + controlnet_cond` behind conv_in (Br = 1: one hint for every sample; g = 1).  B % Br == 0; C % 8 == 0, C <= 4096 (16-byte accesses;
 * x, r, y 16-byte aligned).  g * r and the sum are two separate fp32 operations, never contracted, so torch's
 * (x.float() + g * r.float()).to(T) gives the same bits; with g == 0 and finite r, y == x (a -0 in x becomes +0, as IEEE addition has it).
 * partial != NULL: the same launch writes the GroupNorm partials of y AS STORED in the IMH_GN_STATS format,
 * partial[B][imh_groupnorm_stats_blocks(HW, C)][C / sub][2] (ragged blocks: npart = 0), by the statistics routine of IMH_GN_STATS itself
 * (csrc/norm.hip gn_stats_block: same accumulation, same merge order) -- bit-equal to imh_groupnorm(IMH_GN_STATS) run over y, without
 * the pass.  sub must divide C.  No atomics: the same bits eagerly, from a plan and from a replayed graph.
 * Refused without a launch: null x / r / y, misaligned pointers, tab without step or step without tab, y overlapping x or r -- there is no
 * in-place form: the down path and the mid block of the UNet have read x -- (IMH_ERR_ARG); a non-positive extent, C % 8, C > 4096,
 * B % Br, B > 65535 (IMH_ERR_SHAPE); another dtype (IMH_ERR_DTYPE).
 * In a plan: kind IMH_OP_CONTROL_ADD = 15, a #define like kind 13: enum imh_op_kind is as it was, and kinds 12 and 14 stay refused (callers and
 * tests written against the first version 13 hold imh_plan_add to refusing both, so 15 is the next number that is free).
 * Memory: reads the B * HW * C elements of x, the Br * HW * C elements of r, *step and tab[*step]; writes the B * HW * C elements of y and,
 * when asked, the B * blocks * (C / sub) * 2 floats of partial.  Nothing else. */
#define IMH_OP_CONTROL_ADD 15
typedef struct imh_control_add_args {
    const void* x;
    const void* r;
    void* y;
    float* partial;          /* optional: the IMH_GN_STATS partials of y */
    const float* tab;        /* optional per-step gate table, indexed by *step (with step) */
    const int32_t* step;
    float scale;
    int32_t B, Br, HW, C, sub;
    int32_t dtype;
} imh_control_add_args;
int imh_control_add(const imh_control_add_args* a, void* stream);

/* ---- fp32 (reference-precision) kernels for the VAE decode tail -------------------------------
 * ip_adapter/custom_pipelines.py:365-377 upcasts the SDXL VAE to fp32 before `vae.decode` (it overflows in fp16): this entry keeps
 * fp32 activations, fp32 weights and fp32 arithmetic (v_mfma_f32_32x32x2_f32: exact products, fp32 accumulate).  All pointers fp32.
 *   IMH_F32_GEMM     Y[M, N] = X[M, K] W[N, K]^T (+ bias[n]) (+ residual[m, n]); K % 16 == 0.  conv == 1: 3x3, stride 1 | 2 (0 = 1),
 *                    padding mode `pad` as imh_gemm_args.pad (0: one pixel on every side; 1: right / bottom only, stride 2 -- the
 *                    encoder's Downsample2D), optional nearest x2 upsampling of the input (up = 1, stride 1), NHWC input [B, H, Wd, Cin],
 *                    weights [Cout][ky][kx][Cin], K = 9 Cin, Cin % 16 == 0, M = B Ho Wo.  Replaces diffusers AutoencoderKL's Conv2d /
 *                    Linear / Upsample2D / Downsample2D.
 *   IMH_F32_GN_STATS X [B, HW, C] -> ws [B, nblk, groups, 2] = (mean, M2) per pixel block and group   (diffusers GroupNorm(32, eps 1e-6))
 *   IMH_F32_GN_TABLE ws, gamma, beta -> Y [B, C, 2] = (gamma rstd, beta - mean gamma rstd), merged in double in a fixed order
 *   IMH_F32_GN_APPLY Y = silu?(X scale + shift), ws = the table
 *   IMH_F32_SOFTMAX  Y[r, 0:N] = softmax(scale X[r, 0:N]), M rows (the mid-block attention's materialised scores)
 *   IMH_F32_IMG2IMG_INIT  the initial latents of SDXL image-to-image (diffusers StableDiffusionXLImg2ImgPipeline.prepare_latents) in one
 *                    pass: X = the quant_conv moments [M, HW, 8] NHWC (mean = channels 0-3, logvar = 4-7), W = posterior noise [N, 4, HW],
 *                    residual = add-noise noise [B, 4, HW], Y = latents [B, 4, HW] (NCHW):
 *                      z = scale (mean + exp(0.5 clamp(logvar, -30, 20)) n1),  Y = add_a z + add_b n2
 *                    sample s reads moments s % M and posterior noise s % N (batch expansion by index: one encoded image feeds
 *                    several samples); (add_a, add_b) = (sqrt(abar_t), sqrt(1 - abar_t)) for DDIM, (1, sigma_t) for Euler
 */
enum imh_f32_op { IMH_F32_GEMM = 0, IMH_F32_GN_STATS = 1, IMH_F32_GN_TABLE = 2, IMH_F32_GN_APPLY = 3, IMH_F32_SOFTMAX = 4,
                  IMH_F32_IMG2IMG_INIT = 5 };

typedef struct imh_f32_args {
    const float* X;
    const float* W;
    float* Y;
    const float* bias;
    const float* residual;
    const float* gamma;
    const float* beta;
    float* ws;
    int32_t M, N, K, ldx, ldw, ldy, ldr;
    int32_t conv, H, Wd, Cin, Ho, Wo, up;
    int32_t B, HW, C, groups, nblk, silu;
    float eps, scale;
    int32_t stride, pad;     /* ABI 10: conv stride (0 = 1) and padding mode (as imh_gemm_args.pad) */
    float add_a, add_b;      /* ABI 10: IMH_F32_IMG2IMG_INIT's add-noise pair */
} imh_f32_args;

/* Memory: IMH_F32_GEMM as imh_gemm (rows [0, M) of X / residual / Y at ldx / ldr / ldy, rows [0, N) of W at ldw, any M, N; conv: pixels
 * inside the image only); the GroupNorm steps read / write dense [B, HW, C], ws [B][nblk][groups][2] and the table [B][C][2];
 * IMH_F32_SOFTMAX rows [0, M) x columns [0, N) at ldx / ldy (X == Y allowed); IMH_F32_IMG2IMG_INIT its four dense tensors. */
int imh_f32(int op, const imh_f32_args* a, void* stream);

/* ---- plans: a recorded sequence of the calls above, replayed from C++ (one UNet forward is
 * ~1000 launches; Python would be the bottleneck) and optionally captured into a hipGraph. ---- */
enum imh_op_kind { IMH_OP_GEMM = 0, IMH_OP_ATTN = 1, IMH_OP_GROUPNORM = 2, IMH_OP_LAYERNORM = 3, IMH_OP_EW = 4,
                   IMH_OP_ATTN_SMALL = 5, IMH_OP_GEMM_DUAL = 6, IMH_OP_XATTN = 7, IMH_OP_ATTN_ENC = 8, IMH_OP_ATTN_ENC_CAUSAL = 9,
                   IMH_OP_STEP_SEEDED = 10, IMH_OP_RANDN_SEEDED = 11 };

typedef struct imh_plan imh_plan;

imh_plan* imh_plan_create(void);
void imh_plan_destroy(imh_plan* p);
/* args points to the matching *_args struct (copied); ew_op only for IMH_OP_EW; tag is a small
 * caller-defined integer carried for profiling (e.g. which layer family). Returns op index or <0. */
int imh_plan_add(imh_plan* p, int kind, const void* args, int ew_op, int tag);
int imh_plan_size(const imh_plan* p);
/* in-place update of one recorded op's argument struct (per-step scalars such as the scheduler
 * coefficients); invalidates a captured graph. */
int imh_plan_update(imh_plan* p, int index, const void* args);
int imh_plan_run(imh_plan* p, void* stream);
/* run ops [first, last) */
int imh_plan_run_range(imh_plan* p, int first, int last, void* stream);
/* capture the whole plan into a hipGraph on `stream` (which must be a non-default stream) */
int imh_plan_capture(imh_plan* p, void* stream);
int imh_plan_replay(imh_plan* p, void* stream);
/* run once with a hipEvent pair around every op on `stream`; ms[i] receives op i's duration.
 * Synchronises the stream (measurement helper, not capturable). */
int imh_plan_time_ops(imh_plan* p, void* stream, float* ms, int n);
int imh_plan_get_tag(const imh_plan* p, int index);
int imh_plan_get_kind(const imh_plan* p, int index);

/* tuning / debugging knobs -- key 0: retired (attention workgroups are always 4 waves; accepted and ignored);
 * key 2: XCD tile placement (0 auto, 1 legacy row-major, 2..5 force the (8,1) (4,2) (2,4) (1,8) partition);
 * keys 3 / 4: cross- / self-attention kernel selection (3: 10 = the wide five-head form, 1 = one head per workgroup, 0 = by shape),
 * key 5: LDS-halo conv form (0 auto: conv_hws.hip for the 160-cout forms; 6: conv_halo.hip's lock-step kernels; 8: the K-split form
 * with the service waves transforming the whole halo), key 6: residual rows fetched before / after the K loop, key 7: ff.net.0's prefetch
 * of the next launch's weights inside (1) / behind (0) its K loop, key 9: the 256 x 320 ff.net.0 tile on eight (1) / sixteen (0) waves,
 * key 1: query -- 1 if the library was built with -DIMH_EXPERIMENTAL,
 * key 11: the phase form of the upsampler conv (imh_gemm_args.up == 2): 1 (default) accepted, 0 refused with IMH_ERR_ARG so that the host
 * runs the up = 1 form (A/B in one process); a negative value only queries; RETURNS the current value (not a status),
 * A/B and test use only: the values are process-wide plain ints read at launch time, not meant to change while another
 * thread is launching */
int imh_debug_set(int key, int value);

const char* imh_last_error(void);
int imh_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* IMH_H_ */
