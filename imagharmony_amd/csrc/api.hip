// C ABI of libimh_hip.so (include/imh.h): argument validation, dispatch to the kernel
// launchers, and the plan executor (recorded launch sequences + hipGraph capture).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/imh.h"
#include "../../include/imh_adapter.h"
#include "../../include/imh_regions.h"
#include "imh_common.h"
#include "imh_kernels.h"

namespace imh {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int experimental_refused(const char* what) {
    set_error("%s is compiled only with -DIMH_EXPERIMENTAL (IMH_EXPERIMENTAL=1 python -m imagharmony_amd.build): measured, not selected by any "
              "tuning.json entry or default mode", what);
    return IMH_ERR_ARG;
}
int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return IMH_ERR_LAUNCH;
    }
    return IMH_OK;
}

static GemmParams to_gemm(const imh_gemm_args* a) {
    GemmParams p;
    p.X = a->X; p.W = a->W; p.Y = a->Y; p.partial = a->partial; p.bias = a->bias; p.rowadd = a->rowadd;
    p.residual = a->residual; p.ln_s = a->ln_s; p.ln_c = a->ln_c; p.ln_eps = a->ln_eps;
    p.ln_stats = a->ln_stats; p.ln_stats_out = a->ln_stats_out; p.ln_slots = a->ln_slots; p.ln_slots_out = a->ln_slots_out;
    p.gn_out = a->gn_out; p.gn_nblk = a->gn_nblk; p.gn_hw = a->gn_hw;
    p.gn_tab = a->gn_tab; p.gn_silu = a->gn_silu; p.X2 = a->X2; p.Cin1 = a->X2 ? a->Cin1 : a->Cin;
    p.gn_src.partial = a->gn_part; p.gn_src.partial2 = a->gn_part2; p.gn_src.gamma = a->gn_gamma; p.gn_src.beta = a->gn_beta;
    p.gn_src.eps = a->gn_eps; p.gn_src.groups = a->gn_groups; p.gn_src.C = a->Cin; p.gn_src.C1 = a->gn_part2 ? a->gn_pC1 : a->Cin;
    p.gn_src.HW = a->H * a->Wd; p.gn_src.nblk = a->gn_pnblk; p.gn_src.sub = a->gn_psub; p.gn_src.npart = a->gn_pnpart;
    p.gn_src.nblk2 = a->gn_pnblk2; p.gn_src.sub2 = a->gn_psub2; p.gn_src.npart2 = a->gn_pnpart2; p.gn_src.dtype_f16 = a->dtype == IMH_DT_F16;
    p.Yt = a->Yt; p.yt_col0 = a->yt_col0; p.ldyt = a->ldyt;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.ldx = a->ldx; p.ldw = a->ldw; p.ldy = a->ldy; p.ldr = a->ldr; p.ldra = a->ldra > 0 ? a->ldra : a->N;
    p.rows_per_batch = a->rows_per_batch; p.splits = a->splits; p.flags = a->flags;
    p.H = a->H; p.Wd = a->Wd; p.Cin = a->Cin; p.Ho = a->Ho; p.Wo = a->Wo; p.stride = a->stride; p.up = a->up; p.pad_lo = a->pad == 1 ? 0 : 1;
    p.phase = 0; p.pN = 0;
    p.px = p.py = 1; p.tmx = p.tny = 0; p.xcd = a->xcd;
    p.pf_ptr = a->pf_ptr; p.pf_bytes = a->pf_bytes;
    p.early_res = g_ws_early;
    return p;
}

// IMH_GF_ACT_QGELU stands where the other activations stand: one of them at most
static bool qgelu_combined(int flags) {
    if ((flags & IMH_GF_ACT_QGELU) && (flags & (IMH_GF_ACT_GELU | IMH_GF_ACT_SILU | IMH_GF_GEGLU))) {
        set_error("gemm: IMH_GF_ACT_QGELU is exclusive with IMH_GF_ACT_GELU, IMH_GF_ACT_SILU and IMH_GF_GEGLU (flags=%d)", flags);
        return true;
    }
    return false;
}

static int do_gemm_dual(const imh_gemm_args* a, const imh_gemm_args* b, hipStream_t s) {
    if (!a || !b || !a->X || !a->W || !a->Y || !b->X || !b->W || !b->Y) { set_error("gemm_dual: null pointer argument"); return IMH_ERR_ARG; }
    if (a->conv || b->conv || a->dtype != b->dtype) { set_error("gemm_dual: both problems must be plain GEMMs of one dtype"); return IMH_ERR_ARG; }
    if (qgelu_combined(a->flags) || qgelu_combined(b->flags)) return IMH_ERR_ARG;
    int bm = a->bm, bn = a->bn;
    if (bm != 24128 && (bm <= 0 || bn <= 0 || bm > 128)) { bm = 128; bn = 64; }
    for (const imh_gemm_args* g : {a, b}) {
        if ((g->flags & (IMH_GF_LN_ROW | IMH_GF_LN_COL)) && (!g->ln_s || !g->ln_c || !(g->ln_eps > 0.f))) {
            set_error("gemm_dual: folded LayerNorm needs ln_s / ln_c / ln_eps > 0"); return IMH_ERR_ARG;
        }
        if (g->ln_stats_out || g->gn_out) { set_error("gemm_dual: no statistics epilogue"); return IMH_ERR_ARG; }
        if (g->ln_stats && (g->ln_slots <= 0 || g->K % g->ln_slots)) { set_error("gemm_dual: ln_slots=%d must divide K=%d", g->ln_slots, g->K); return IMH_ERR_ARG; }
    }
    if ((a->ln_stats == nullptr) != (b->ln_stats == nullptr) && ((a->flags | b->flags) & (IMH_GF_LN_ROW | IMH_GF_LN_COL))) {
        set_error("gemm_dual: both problems take their LayerNorm statistics the same way"); return IMH_ERR_ARG;
    }
    return gemm_dual_launch(to_gemm(a), to_gemm(b), a->dtype, bm, bn, s);
}

static int do_gemm(const imh_gemm_args* a, hipStream_t s) {
    if (!a || !a->X || !a->W || !a->Y) { set_error("gemm: null pointer argument"); return IMH_ERR_ARG; }
    if (qgelu_combined(a->flags)) return IMH_ERR_ARG;
    GemmParams p = to_gemm(a);
    if ((p.flags & (IMH_GF_LN_ROW | IMH_GF_LN_COL)) && (!p.ln_s || !p.ln_c || !(p.ln_eps > 0.f))) { set_error("gemm: folded LayerNorm needs ln_s / ln_c / ln_eps > 0"); return IMH_ERR_ARG; }
    if ((p.flags & IMH_GF_LN_ROW) && (p.flags & IMH_GF_LN_COL)) { set_error("gemm: IMH_GF_LN_ROW and IMH_GF_LN_COL are exclusive"); return IMH_ERR_ARG; }
    if (!(p.flags & (IMH_GF_LN_ROW | IMH_GF_LN_COL))) p.ln_stats = nullptr;
    if (p.ln_stats && (p.ln_slots <= 0 || p.K % p.ln_slots)) { set_error("gemm: ln_slots=%d must divide K=%d", p.ln_slots, p.K); return IMH_ERR_ARG; }
    int bm = a->bm, bn = a->bn;
    if (bm <= 0 || bn <= 0 || p.splits <= 0) {
        int hb, hn, hs;
        gemm_pick_config(p.M, p.N, p.K, &hb, &hn, &hs);
        if (bm <= 0) bm = hb;
        if (bn <= 0) bn = hn;
        if (p.splits <= 0) p.splits = p.partial ? hs : 1;
    }
    if ((p.flags & IMH_GF_VT_PERM) && p.splits == 1) bn = 128;   // the permutation lives in 16-column groups
    if (a->conv) {
        if (p.stride != 1 && p.stride != 2) { set_error("conv3x3: stride must be 1 or 2"); return IMH_ERR_ARG; }
        if (p.up != 0 && p.up != 1 && p.up != 2) { set_error("conv3x3: up must be 0, 1 or 2"); return IMH_ERR_ARG; }
        if (a->pad != 0 && a->pad != 1) { set_error("conv3x3: pad must be 0 or 1"); return IMH_ERR_ARG; }
        if (p.up == 2) {
            // phase form of Upsample2D's conv (include/imh.h): four 2 x 2-tap convs on the low-res input, W phase-packed [4 Cout, 4 Cin];
            // the kernels see a plain stride-1 conv geometry over the low-res pixels plus GemmParams.phase
            if (!g_up_phase) { set_error("conv3x3: the phase form (up = 2) is switched off (imh_debug_set key 11)"); return IMH_ERR_ARG; }
            if (p.stride != 1 || a->pad != 0 || p.H <= 0 || p.Wd <= 0 || p.Ho != 2 * p.H || p.Wo != 2 * p.Wd || p.M % (p.H * p.Wd) != 0 ||
                p.N <= 0 || p.N % 4 || p.K != 4 * p.Cin) {
                set_error("conv3x3: the phase form (up = 2) needs stride 1, pad 0, Ho x Wo = 2H x 2W, M = B*H*W low-res pixels, N = 4*Cout, "
                          "K = 4*Cin (H=%d W=%d Ho=%d Wo=%d M=%d N=%d K=%d Cin=%d stride=%d)", p.H, p.Wd, p.Ho, p.Wo, p.M, p.N, p.K, p.Cin, p.stride);
                return IMH_ERR_SHAPE;
            }
            p.phase = 1; p.pN = p.N / 4; p.up = 0; p.Ho = p.H; p.Wo = p.Wd;
            return gemm_launch(p, a->dtype, a->conv, bm, bn, s);
        }
        if (a->pad == 1) {
            // right / bottom padding (Downsample2D(padding=0)): stride 2 without upsampling, on the variants whose implicit-GEMM loaders
            // take pad_lo -- the LDS-halo conv3x3 (stride 1 only), the ping-pong and the sixteen-wave Linear forms do not
            if (p.stride != 2 || p.up || p.H < 2 || p.Wd < 2) {
                set_error("conv3x3: pad mode 1 needs stride 2, up 0 and an input of at least 2 x 2 (stride=%d up=%d H=%d W=%d)", p.stride, p.up, p.H, p.Wd);
                return IMH_ERR_ARG;
            }
            if (bm == 7128 || bm == 7564 || bm == 7328 || bm == 7428 || bm == 7256 || bm == 7356 || bm == 8256 || bm == 9128 || bm == 9256 ||
                bm == 26256) {
                set_error("conv3x3: pad mode 1 is not implemented by variant %d x %d", bm, bn);
                return IMH_ERR_ARG;
            }
        }
        const int Hv = p.H << p.up, Wv = p.Wd << p.up;
        const int span = a->pad == 1 ? 1 : 2;              // padded input minus the 3-tap window: (H + pad_total - 3)
        if (p.Ho != (Hv + span - 3) / p.stride + 1 || p.Wo != (Wv + span - 3) / p.stride + 1 || p.Ho <= 0 || p.Wo <= 0) {
            set_error("conv3x3: output size %dx%d inconsistent with input %dx%d up=%d stride=%d pad=%d", p.Ho, p.Wo, p.H, p.Wd, p.up, p.stride, a->pad);
            return IMH_ERR_SHAPE;
        }
        if (p.M % (p.Ho * p.Wo) != 0) { set_error("conv3x3: M must be B*Ho*Wo"); return IMH_ERR_SHAPE; }
    } else if (a->pad) {
        set_error("gemm: pad is a conv3x3 field (conv == 0)"); return IMH_ERR_ARG;
    }
    return gemm_launch(p, a->dtype, a->conv, bm, bn, s);
}

// the fields imh_attn_args, imh_xattn_args and imh_xattn_regions_args share under the same names; Q / ldq: the fused forms compute their queries
// in the launch.  split and defer_log2 are the launchers' to set (imh_kernels.h)
template <class A>
static void fill_attn(AttnParams& p, const A* a, const void* Q, int ldq) {
    p.Q = Q; p.K = a->K; p.Vt = a->Vt; p.K2 = a->K2; p.Vt2 = a->Vt2; p.O = a->O;
    p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.Lk_pad = a->Lk_pad; p.Lk2 = a->Lk2; p.Lk2_pad = a->Lk2_pad;
    p.ldq = ldq; p.ldk = a->ldk; p.ldvt = a->ldvt; p.ldk2 = a->ldk2; p.ldvt2 = a->ldvt2; p.ldo = a->ldo;
    p.scale = a->scale; p.scale2 = a->scale2; p.scale2_tab = a->scale2_tab; p.step = a->step;
    p.pf_ptr = a->pf_ptr; p.pf_bytes = a->pf_bytes; p.split = 0; p.defer_log2 = 0.f;
}

// ... and the fused to_q of imh_xattn_args and imh_xattn_regions_args: the statistics count only under a folded LayerNorm
template <class A>
static void fill_xattn(XAttnParams& x, const A* a) {
    fill_attn(x.a, a, nullptr, 0);
    x.X = a->X; x.Wq = a->Wq; x.ln_s = a->ln_s; x.ln_c = a->ln_c; x.ln_eps = a->ln_eps;
    x.ln_stats = a->ln_s ? a->ln_stats : nullptr; x.ln_slots = a->ln_slots;
    x.C = a->C; x.ldx = a->ldx; x.ldw = a->ldw; x.split = 0;
}

static int do_attn(const imh_attn_args* a, hipStream_t s) {
    if (!a || !a->Q || !a->K || !a->Vt || !a->O) { set_error("attention: null pointer argument"); return IMH_ERR_ARG; }
    if ((a->K2 == nullptr) != (a->Vt2 == nullptr)) { set_error("attention: K2 and Vt2 must come together"); return IMH_ERR_ARG; }
    AttnParams p;
    fill_attn(p, a, a->Q, a->ldq);
    return attention_launch(p, a->dtype, s);
}

static int do_xattn(const imh_xattn_args* a, hipStream_t s) {
    if (!a || !a->X || !a->Wq || !a->K || !a->Vt || !a->O) { set_error("cross_attention: null pointer argument"); return IMH_ERR_ARG; }
    if ((a->K2 == nullptr) != (a->Vt2 == nullptr)) { set_error("cross_attention: K2 and Vt2 must come together"); return IMH_ERR_ARG; }
    if ((a->ln_s == nullptr) != (a->ln_c == nullptr) || (a->ln_s && !(a->ln_eps > 0.f))) {
        set_error("cross_attention: folded LayerNorm needs ln_s, ln_c and ln_eps > 0"); return IMH_ERR_ARG;
    }
    if (a->C != a->H * 64) { set_error("cross_attention: C=%d must be H*64 (H=%d)", a->C, a->H); return IMH_ERR_SHAPE; }
    XAttnParams x;
    fill_xattn(x, a);
    if (x.ln_stats && (a->ln_slots <= 0 || a->C % a->ln_slots)) { set_error("cross_attention: ln_slots=%d must divide C=%d", a->ln_slots, a->C); return IMH_ERR_ARG; }
    return xattn_launch(x, a->dtype, s);
}

// imh_cross_attention_regions (include/imh_regions.h): the pointer / alignment rules here, the shape rules in the launcher
static int do_xattn_regions(const imh_xattn_regions_args* a, hipStream_t s) {
    const char* who = "cross_attention_regions";
    if (!a || !a->X || !a->Wq || !a->K || !a->Vt || !a->K2 || !a->Vt2 || !a->O || !a->mask) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if ((a->ln_s == nullptr) != (a->ln_c == nullptr) || (a->ln_s && !(a->ln_eps > 0.f))) {
        set_error("%s: folded LayerNorm needs ln_s, ln_c and ln_eps > 0", who); return IMH_ERR_ARG;
    }
    if (((uintptr_t)a->mask | (uintptr_t)a->weights) & 3) { set_error("%s: mask and weights must be 4-byte aligned", who); return IMH_ERR_ARG; }
    if ((a->scale2_tab == nullptr) != (a->step == nullptr)) { set_error("%s: scale2_tab and step come together", who); return IMH_ERR_ARG; }
    if (a->C != a->H * 64) { set_error("%s: C=%d must be H*64 (H=%d)", who, a->C, a->H); return IMH_ERR_SHAPE; }
    XRegionParams r;
    fill_xattn(r.x, a);
    if (a->ln_s && !a->ln_stats) { set_error("%s: the folded LayerNorm takes the token rows' statistics from ln_stats", who); return IMH_ERR_ARG; }
    if (r.x.ln_stats && (a->ln_slots <= 0 || a->C % a->ln_slots)) { set_error("%s: ln_slots=%d must divide C=%d", who, a->ln_slots, a->C); return IMH_ERR_ARG; }
    r.mask = a->mask; r.weights = a->weights; r.n_img = a->n_img; r.ldm = a->ldm;
    return xattn_regions_launch(r, a->dtype, s);
}

static int do_attn_small(const imh_small_attn_args* a, hipStream_t s) {
    if (!a || !a->Q || !a->K || !a->V || !a->O) { set_error("attention_small: null pointer argument"); return IMH_ERR_ARG; }
    SmallAttnParams p;
    p.Q = a->Q; p.K = a->K; p.V = a->V; p.O = a->O;
    p.B = a->B; p.H = a->H; p.Lq = a->Lq; p.Lk = a->Lk; p.dq = a->dq; p.dv = a->dv;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo; p.scale = a->scale;
    return attention_small_launch(p, a->dtype, s);
}

static int do_attn_enc(const imh_enc_attn_args* a, hipStream_t s, int causal = 0) {
    if (!a || !a->Q || !a->K || !a->V || !a->O) { set_error("attention_enc: null pointer argument"); return IMH_ERR_ARG; }
    EncAttnParams p;
    p.Q = a->Q; p.K = a->K; p.V = a->V; p.O = a->O;
    p.B = a->B; p.H = a->H; p.L = a->L; p.d = a->d;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo; p.scale = a->scale; p.causal = causal;
    return attention_enc_launch(p, a->dtype, s);
}

static NormParams to_norm(const imh_norm_args* a) {
    NormParams p;
    p.x = a->x; p.y = a->y; p.gamma = a->gamma; p.beta = a->beta; p.partial = a->partial;
    p.B = a->B; p.HW = a->HW; p.C = a->C; p.groups = a->groups; p.rows = a->rows; p.eps = a->eps; p.silu = a->silu;
    p.mode = a->mode; p.table = a->table; p.partial2 = a->partial2;
    p.nblk = a->nblk; p.sub = a->sub; p.npart = a->npart; p.C1 = a->C1; p.nblk2 = a->nblk2; p.sub2 = a->sub2; p.npart2 = a->npart2;
    p.dtype_f16 = 0;
    p.pf_ptr = a->pf_ptr; p.pf_bytes = a->pf_bytes;
    return p;
}

static EwParams to_ew(const imh_ew_args* a) {
    EwParams p;
    p.a = a->a; p.b = a->b; p.y = a->y; p.w = a->w; p.bias = a->bias; p.tab = a->tab; p.step = a->step; p.n = a->n;
    p.i0 = a->i0; p.i1 = a->i1; p.i2 = a->i2; p.i3 = a->i3; p.i4 = a->i4; p.i5 = a->i5;
    p.f0 = a->f0; p.f1 = a->f1; p.f2 = a->f2; p.f3 = a->f3;
    p.x2 = a->x2; p.noise = a->noise; p.mask = a->mask; p.blend_tab = a->blend_tab;
    return p;
}

static int do_groupnorm(const imh_norm_args* a, hipStream_t s) {
    if (!a) { set_error("groupnorm: null pointer argument"); return IMH_ERR_ARG; }
    return groupnorm_launch(to_norm(a), a->dtype, s);
}

static int do_layernorm(const imh_norm_args* a, hipStream_t s) {
    if (!a || !a->x || !a->y) { set_error("layernorm: null pointer argument"); return IMH_ERR_ARG; }
    return layernorm_launch(to_norm(a), a->dtype, s);
}

static int do_ew(int op, const imh_ew_args* a, hipStream_t s) {
    if (!a || !a->y) { set_error("elementwise: null pointer argument"); return IMH_ERR_ARG; }
    return ew_launch(op, to_ew(a), a->dtype, s);
}

// imh_step_seeded: IMH_EW_CFG_MSTEP's launch with the noise generated from the seed rows (elementwise.hip cfg_mstep_kernel<.., SEEDED>)
static int do_step_seeded(const imh_seeded_args* a, hipStream_t s) {
    if (!a || !a->ew.y) { set_error("imh_step_seeded: null pointer argument"); return IMH_ERR_ARG; }
    if (!a->seeds) { set_error("imh_step_seeded: null seeds (one uint32 row (k0, k1, lane, 0) per sample)"); return IMH_ERR_ARG; }
    if (a->ew.bias) { set_error("imh_step_seeded: bias (the noise bank of IMH_EW_CFG_MSTEP) must be NULL: the noise comes from seeds"); return IMH_ERR_ARG; }
    if ((uintptr_t)a->seeds & 3) { set_error("imh_step_seeded: seeds must be 4-byte aligned"); return IMH_ERR_ARG; }
    EwParams p = to_ew(&a->ew);                  // (bias, the noise bank, is null: checked above)
    p.seeds = a->seeds; p.noise_stream = a->stream;
    return ew_launch(IMH_EW_CFG_MSTEP, p, a->ew.dtype, s);
}

static int to_randn(const imh_randn_args* a, const char* who, RandnParams* p) {
    if (!a || !a->y) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if (!a->seeds) { set_error("%s: null seeds (one uint32 row (k0, k1, lane, 0) per sample)", who); return IMH_ERR_ARG; }
    if (a->S <= 0 || a->HW <= 0 || (long long)a->S * a->HW > 0x7fffffffLL / 4) { set_error("%s: S=%d HW=%d (both > 0, S * 4 * HW < 2^31)", who, a->S, a->HW); return IMH_ERR_SHAPE; }
    if (((uintptr_t)a->seeds | (uintptr_t)a->y | (uintptr_t)a->step) & 3) { set_error("%s: y, seeds and step must be 4-byte aligned", who); return IMH_ERR_ARG; }
    p->y = a->y; p->seeds = a->seeds; p->step = a->step; p->S = a->S; p->HW = a->HW; p->row = a->row; p->noise_stream = a->stream; p->raw = a->raw; p->quad0 = a->quad0;
    return IMH_OK;
}

static int do_randn_seeded(const imh_randn_args* a, hipStream_t s) {
    RandnParams p;
    const int rc = to_randn(a, "imh_randn_seeded", &p);
    return rc != IMH_OK ? rc : randn_seeded_launch(p, s);
}

static int do_clip_preprocess(const imh_clip_preprocess_args* a, hipStream_t s) {
    const char* who = "imh_clip_preprocess";
    if (!a || !a->x || !a->y) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if (a->dtype != IMH_DT_BF16 && a->dtype != IMH_DT_F16 && a->dtype != IMH_CLIP_DT_F32) {
        set_error("%s: dtype %d is none of IMH_DT_BF16, IMH_DT_F16, IMH_CLIP_DT_F32", who, a->dtype); return IMH_ERR_ARG;
    }
    if (((uintptr_t)a->x & 3) || ((uintptr_t)a->y & (a->dtype == IMH_CLIP_DT_F32 ? 3 : 1))) { set_error("%s: x / y must be aligned to their element size", who); return IMH_ERR_ARG; }
    if (!(a->std0 > 0.f) || !(a->std1 > 0.f) || !(a->std2 > 0.f)) { set_error("%s: std must be positive", who); return IMH_ERR_ARG; }
    if (a->S < 1 || a->H < 1 || a->W < 1) { set_error("%s: S=%d H=%d W=%d must be positive", who, a->S, a->H, a->W); return IMH_ERR_SHAPE; }
    if (a->patch < 1 || a->patch > 32 || a->size < a->patch || a->size % a->patch) {
        set_error("%s: size=%d must be a positive multiple of patch=%d (1 .. 32)", who, a->size, a->patch); return IMH_ERR_SHAPE;
    }
    if (a->nh < a->size || a->nw < a->size) { set_error("%s: the resized image %d x %d is smaller than the crop %d", who, a->nh, a->nw, a->size); return IMH_ERR_SHAPE; }
    if (a->top < 0 || a->left < 0 || a->top > a->nh - a->size || a->left > a->nw - a->size) {
        set_error("%s: crop (%d, %d) + %d lies outside the resized image %d x %d", who, a->top, a->left, a->size, a->nh, a->nw); return IMH_ERR_SHAPE;
    }
    if (a->ldp < 3 * a->patch * a->patch) { set_error("%s: ldp=%d is smaller than a row of 3 * %d * %d values", who, a->ldp, a->patch, a->patch); return IMH_ERR_SHAPE; }
    const long long g = a->size / a->patch;
    if ((long long)a->S * g * g * a->ldp > 0x7fffffffLL || (long long)a->S * 3 * a->H * a->W > 0x7fffffffLL || (long long)a->S * 3 * g * g > 0x7fffffffLL) {
        set_error("%s: S=%d H=%d W=%d size=%d ldp=%d: an operand of 2^31 elements or more", who, a->S, a->H, a->W, a->size, a->ldp); return IMH_ERR_SHAPE;
    }
    ClipPreParams p;
    p.x = a->x; p.y = a->y; p.S = a->S; p.H = a->H; p.W = a->W; p.nh = a->nh; p.nw = a->nw; p.top = a->top; p.left = a->left;
    p.size = a->size; p.patch = a->patch; p.ldp = a->ldp;
    p.mean[0] = a->mean0; p.mean[1] = a->mean1; p.mean[2] = a->mean2; p.std[0] = a->std0; p.std[1] = a->std1; p.std[2] = a->std2;
    p.ncols = p.ntx = p.nty = p.RC = 0;
    return clip_preprocess_launch(p, a->dtype, s);
}

static int do_control_add(const imh_control_add_args* a, hipStream_t s) {
    const char* who = "imh_control_add";
    if (!a || !a->x || !a->r || !a->y) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if (((uintptr_t)a->x | (uintptr_t)a->r | (uintptr_t)a->y) & 15) { set_error("%s: x, r and y must be 16-byte aligned", who); return IMH_ERR_ARG; }
    if (((uintptr_t)a->partial | (uintptr_t)a->tab | (uintptr_t)a->step) & 3) { set_error("%s: partial, tab and step must be 4-byte aligned", who); return IMH_ERR_ARG; }
    if ((a->tab == nullptr) != (a->step == nullptr)) { set_error("%s: tab and step come together", who); return IMH_ERR_ARG; }
    if (a->B <= 0 || a->HW <= 0 || a->C <= 0 || a->Br <= 0) { set_error("%s: B=%d Br=%d HW=%d C=%d must be positive", who, a->B, a->Br, a->HW, a->C); return IMH_ERR_SHAPE; }
    // y overlapping x or r (the in-place form included) is refused: the superseded tensor stays what its other readers saw
    const size_t yb = (size_t)a->B * a->HW * a->C * 2, rb = (size_t)a->Br * a->HW * a->C * 2;
    const uintptr_t y0 = (uintptr_t)a->y, x0 = (uintptr_t)a->x, r0 = (uintptr_t)a->r;
    if ((y0 < x0 + yb && x0 < y0 + yb) || (y0 < r0 + rb && r0 < y0 + yb)) { set_error("%s: y must not overlap x or r (no in-place form)", who); return IMH_ERR_ARG; }
    ControlAddParams p;
    p.x = a->x; p.r = a->r; p.y = a->y; p.partial = a->partial; p.tab = a->tab; p.step = a->step; p.scale = a->scale;
    p.B = a->B; p.Br = a->Br; p.HW = a->HW; p.C = a->C; p.sub = a->sub;
    return control_add_launch(p, a->dtype, s);
}

static int do_adapter_op(const imh_adapter_args* a, hipStream_t s) {
    const char* who = "imh_adapter_op";
    if (!a || !a->x || !a->y) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if (a->mode != IMH_ADAPTER_UNSHUFFLE && a->mode != IMH_ADAPTER_RELU && a->mode != IMH_ADAPTER_AVGPOOL2) {
        set_error("%s: unknown mode %d", who, a->mode); return IMH_ERR_ARG;
    }
    if (((uintptr_t)a->y & 15) || ((uintptr_t)a->x & (a->mode == IMH_ADAPTER_UNSHUFFLE ? 3 : 15))) {
        set_error("%s: y (and x, unshuffle: to 4 bytes) must be 16-byte aligned", who); return IMH_ERR_ARG;
    }
    if (a->dtype != IMH_DT_BF16 && a->dtype != IMH_DT_F16) { set_error("%s: unknown dtype %d", who, a->dtype); return IMH_ERR_DTYPE; }
    const long long lim = 0x7fffffffLL;
    long long xe, ye;                        // elements of x and of y
    if (a->mode == IMH_ADAPTER_RELU) {
        if (a->n <= 0 || a->n > lim) { set_error("%s: relu over n=%lld elements (0 < n < 2^31)", who, (long long)a->n); return IMH_ERR_SHAPE; }
        xe = ye = a->n;
    } else {
        if (a->N <= 0 || a->C <= 0 || a->H <= 0 || a->W <= 0) { set_error("%s: N=%d C=%d H=%d W=%d must be positive", who, a->N, a->C, a->H, a->W); return IMH_ERR_SHAPE; }
        xe = (long long)a->N * a->C;
        if (xe > lim || (xe *= a->H) > lim || (xe *= a->W) > lim) { set_error("%s: N=%d C=%d H=%d W=%d: an operand of 2^31 elements or more", who, a->N, a->C, a->H, a->W); return IMH_ERR_SHAPE; }
        if (a->mode == IMH_ADAPTER_UNSHUFFLE) {
            if (a->f < 1 || a->H % a->f || a->W % a->f) { set_error("%s: unshuffle of %d x %d by f=%d (f >= 1 divides both sides)", who, a->H, a->W, a->f); return IMH_ERR_SHAPE; }
            const long long K = (long long)a->C * a->f * a->f;
            if (a->Cp <= 0 || a->Cp % 8 || a->Cp < K) { set_error("%s: Cp=%d must be a multiple of 8 and at least C f^2 = %lld", who, a->Cp, K); return IMH_ERR_SHAPE; }
            ye = (long long)a->N * (a->H / a->f) * (a->W / a->f);
            if (ye > lim || (ye *= a->Cp) > lim) { set_error("%s: Cp=%d: an operand of 2^31 elements or more", who, a->Cp); return IMH_ERR_SHAPE; }
        } else {
            if (a->C % 8) { set_error("%s: avgpool2 over C=%d channels (a multiple of 8)", who, a->C); return IMH_ERR_SHAPE; }
            ye = (long long)a->N * ((a->H + 1) / 2) * ((a->W + 1) / 2) * a->C;
        }
    }
    const uintptr_t x0 = (uintptr_t)a->x, y0 = (uintptr_t)a->y;
    const size_t xb = (size_t)xe * (a->mode == IMH_ADAPTER_UNSHUFFLE ? 4 : 2), yb = (size_t)ye * 2;
    if (y0 < x0 + xb && x0 < y0 + yb && !(a->mode == IMH_ADAPTER_RELU && x0 == y0)) {
        set_error("%s: y must not overlap x (relu: except y == x)", who); return IMH_ERR_ARG;
    }
    AdapterParams p;
    p.x = a->x; p.y = a->y; p.n = a->n; p.mode = a->mode; p.N = a->N; p.C = a->C; p.H = a->H; p.W = a->W; p.f = a->f; p.Cp = a->Cp;
    return adapter_launch(p, a->dtype, s);
}

}  // namespace imh

using namespace imh;

struct imh_op {
    int kind;
    int ew_op;
    int tag;
    union {
        imh_gemm_args gemm;
        imh_attn_args attn;
        imh_norm_args norm;
        imh_ew_args ew;
        imh_small_attn_args sattn;
        imh_gemm_args gemm2[2];
        imh_xattn_args xattn;
        imh_enc_attn_args eattn;
        imh_seeded_args seeded;
        imh_randn_args randn;
        imh_clip_preprocess_args clip;
        imh_control_add_args cadd;
        imh_xattn_regions_args xregions;
    } u;
};

struct imh_plan {
    std::vector<imh_op> ops;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// the plan kinds: what imh_plan_add copies for each and what runs it.  A kind that is not here (12, 14 and 16 among them) is refused
struct op_entry {
    int kind;
    size_t size;
    int (*run)(const imh_op&, hipStream_t);
};
static const op_entry g_ops[] = {
    {IMH_OP_GEMM, sizeof(imh_gemm_args), [](const imh_op& o, hipStream_t s) { return do_gemm(&o.u.gemm, s); }},
    {IMH_OP_ATTN, sizeof(imh_attn_args), [](const imh_op& o, hipStream_t s) { return do_attn(&o.u.attn, s); }},
    {IMH_OP_GROUPNORM, sizeof(imh_norm_args), [](const imh_op& o, hipStream_t s) { return do_groupnorm(&o.u.norm, s); }},
    {IMH_OP_LAYERNORM, sizeof(imh_norm_args), [](const imh_op& o, hipStream_t s) { return do_layernorm(&o.u.norm, s); }},
    {IMH_OP_EW, sizeof(imh_ew_args), [](const imh_op& o, hipStream_t s) { return do_ew(o.ew_op, &o.u.ew, s); }},
    {IMH_OP_ATTN_SMALL, sizeof(imh_small_attn_args), [](const imh_op& o, hipStream_t s) { return do_attn_small(&o.u.sattn, s); }},
    {IMH_OP_GEMM_DUAL, 2 * sizeof(imh_gemm_args), [](const imh_op& o, hipStream_t s) { return do_gemm_dual(&o.u.gemm2[0], &o.u.gemm2[1], s); }},
    {IMH_OP_XATTN, sizeof(imh_xattn_args), [](const imh_op& o, hipStream_t s) { return do_xattn(&o.u.xattn, s); }},
    {IMH_OP_ATTN_ENC, sizeof(imh_enc_attn_args), [](const imh_op& o, hipStream_t s) { return do_attn_enc(&o.u.eattn, s); }},
    {IMH_OP_ATTN_ENC_CAUSAL, sizeof(imh_enc_attn_args), [](const imh_op& o, hipStream_t s) { return do_attn_enc(&o.u.eattn, s, 1); }},
    {IMH_OP_STEP_SEEDED, sizeof(imh_seeded_args), [](const imh_op& o, hipStream_t s) { return do_step_seeded(&o.u.seeded, s); }},
    {IMH_OP_RANDN_SEEDED, sizeof(imh_randn_args), [](const imh_op& o, hipStream_t s) { return do_randn_seeded(&o.u.randn, s); }},
    {IMH_OP_CLIP_PREPROCESS, sizeof(imh_clip_preprocess_args), [](const imh_op& o, hipStream_t s) { return do_clip_preprocess(&o.u.clip, s); }},
    {IMH_OP_CONTROL_ADD, sizeof(imh_control_add_args), [](const imh_op& o, hipStream_t s) { return do_control_add(&o.u.cadd, s); }},
    {IMH_OP_XATTN_REGIONS, sizeof(imh_xattn_regions_args), [](const imh_op& o, hipStream_t s) { return do_xattn_regions(&o.u.xregions, s); }},
};

static const op_entry* find_op(int kind) {
    for (const op_entry& e : g_ops)
        if (e.kind == kind) return &e;
    return nullptr;
}

static int run_op(const imh_op& o, hipStream_t s) {
    const op_entry* e = find_op(o.kind);
    if (!e) { set_error("plan: unknown op kind %d", o.kind); return IMH_ERR_ARG; }
    return e->run(o, s);
}

static void drop_graph(imh_plan* p) {
    if (p->exec) { hipGraphExecDestroy(p->exec); p->exec = nullptr; }
    if (p->graph) { hipGraphDestroy(p->graph); p->graph = nullptr; }
}

extern "C" {

int imh_abi_version(void) { return IMH_ABI_VERSION; }
int imh_debug_set(int key, int value) {
    if (key == 0) { g_attn_force_nw = value; return IMH_OK; }
    if (key == 1) {                               // query: was this library built with -DIMH_EXPERIMENTAL?
#ifdef IMH_EXPERIMENTAL
        return 1;
#else
        return 0;
#endif
    }
    if (key == 2) { g_xcd_mode = value; return IMH_OK; }
    if (key == 3) { g_xattn_mode = value; return IMH_OK; }
    if (key == 4) { g_attn_mode = value; return IMH_OK; }
    if (key == 5) { g_halo_mode = value; return IMH_OK; }
    if (key == 7) { g_w16_pf = value; return IMH_OK; }        // sixteen-wave ff.net.0 tile: 1 (default) = the next launch's weights prefetched inside the K loop, 0 = behind the epilogue
    if (key == 9) { g_w16_form = value; return IMH_OK; }      // the 256 x 320 ff.net.0 tile: 0 = sixteen waves of 64 x 80, 1 = eight waves of 128 x 80
    if (key == 10) { g_f32_exact = value; return IMH_OK; }    // imh_f32 GEMM / conv: 1 = the exact fp32 MFMA kernel for every launch, 0 (default) = bf16 hi / lo split where the K tile fits
    if (key == 11) { if (value >= 0) g_up_phase = value; return g_up_phase; }      // 0: up = 2 launches are refused (the host then runs the up = 1 form; A/B); value < 0: query
    if (key == 6) { g_ws_early = value; return IMH_OK; }      // 0: the residual rows of the wave-specialised launches fetched after the K loop (A/B)
    set_error("debug_set: unknown key %d", key);
    return IMH_ERR_ARG;
}
const char* imh_last_error(void) { return g_err; }

int imh_gemm(const imh_gemm_args* a, void* stream) { return do_gemm(a, (hipStream_t)stream); }
int imh_gemm_dual(const imh_gemm_args* a, const imh_gemm_args* b, void* stream) { return do_gemm_dual(a, b, (hipStream_t)stream); }
int imh_gemm_pick_config(int M, int N, int K, int* bm, int* bn, int* splits) {
    if (!bm || !bn || !splits) { set_error("pick_config: null output"); return IMH_ERR_ARG; }
    gemm_pick_config(M, N, K, bm, bn, splits);
    return IMH_OK;
}
size_t imh_gemm_workspace_bytes(int M, int N, int splits) { return gemm_workspace_bytes(M, N, splits); }
int imh_gemm_stats_slot_width(int bm, int bn) { return gemm_stats_slot_width(bm, bn); }
int imh_gemm_gn_block_rows(int bm, int bn) { return gemm_gn_block_rows(bm, bn); }
int imh_conv_halo_lds_bytes(int bm, int bn, int Cin, int gn) { return conv_halo_lds_bytes(bm, bn, Cin, gn); }

// every check of imh_gemm without the launch: the call is issued into a stream capture of its own whose graph is thrown away, so the
// validators that run are the launchers' own and nothing executes.  The capture stream belongs to the calling thread and to the device
// that is current at the call (one per device the thread ever checks on, created at the first check there and kept for the life of the
// thread); the cost is one begin / end capture pair per call, paid where a launch is recorded and never at replay
int imh_gemm_check(const imh_gemm_args* a) {
    static thread_local std::vector<hipStream_t> streams;          // [device]
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) { (void)hipGetLastError(); set_error("gemm_check: no current device"); return IMH_ERR_LAUNCH; }
    if ((size_t)dev >= streams.size()) streams.resize(dev + 1, nullptr);
    hipStream_t& cs = streams[dev];
    if (!cs && hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess) {
        cs = nullptr; (void)hipGetLastError();
        set_error("gemm_check: no stream to validate on"); return IMH_ERR_LAUNCH;
    }
    hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("gemm_check: begin: %s", hipGetErrorString(e)); return IMH_ERR_LAUNCH; }
    const int rc = do_gemm(a, cs);
    hipGraph_t g = nullptr;
    e = hipStreamEndCapture(cs, &g);
    if (g) hipGraphDestroy(g);
    if (rc != IMH_OK) { (void)hipGetLastError(); return rc; }
    if (e != hipSuccess) { (void)hipGetLastError(); set_error("gemm_check: end: %s", hipGetErrorString(e)); return IMH_ERR_LAUNCH; }
    return IMH_OK;
}

int imh_attention(const imh_attn_args* a, void* stream) { return do_attn(a, (hipStream_t)stream); }

int imh_cross_attention(const imh_xattn_args* a, void* stream) { return do_xattn(a, (hipStream_t)stream); }

int imh_cross_attention_regions(const imh_xattn_regions_args* a, void* stream) { return do_xattn_regions(a, (hipStream_t)stream); }

int imh_attention_small(const imh_small_attn_args* a, void* stream) { return do_attn_small(a, (hipStream_t)stream); }

int imh_attention_enc(const imh_enc_attn_args* a, void* stream) { return do_attn_enc(a, (hipStream_t)stream); }
int imh_attention_enc_causal(const imh_enc_attn_args* a, void* stream) { return do_attn_enc(a, (hipStream_t)stream, 1); }

int imh_groupnorm(const imh_norm_args* a, void* stream) { return do_groupnorm(a, (hipStream_t)stream); }
size_t imh_groupnorm_workspace_bytes(int B, int HW, int C, int groups) { return groupnorm_workspace_bytes(B, HW, C, groups); }
int imh_groupnorm_stats_blocks(int HW, int C) { return groupnorm_stats_blocks(HW, C); }
int imh_groupnorm_stats_sub(int C, int groups) { return groups > 0 && C % groups == 0 ? groupnorm_stats_sub(C, groups) : 0; }
int imh_layernorm(const imh_norm_args* a, void* stream) { return do_layernorm(a, (hipStream_t)stream); }

int imh_elementwise(int op, const imh_ew_args* a, void* stream) { return do_ew(op, a, (hipStream_t)stream); }

int imh_step_seeded(const imh_seeded_args* a, void* stream) { return do_step_seeded(a, (hipStream_t)stream); }
int imh_randn_seeded(const imh_randn_args* a, void* stream) { return do_randn_seeded(a, (hipStream_t)stream); }
int imh_clip_preprocess(const imh_clip_preprocess_args* a, void* stream) { return do_clip_preprocess(a, (hipStream_t)stream); }
int imh_control_add(const imh_control_add_args* a, void* stream) { return do_control_add(a, (hipStream_t)stream); }
int imh_adapter_op(const imh_adapter_args* a, void* stream) { return do_adapter_op(a, (hipStream_t)stream); }
int imh_randn_seeded_host(const imh_randn_args* a) {
    RandnParams p;
    const int rc = to_randn(a, "imh_randn_seeded_host", &p);
    return rc != IMH_OK ? rc : randn_seeded_host(p);
}

int imh_f32(int op, const imh_f32_args* a, void* stream) {
    if (!a) { set_error("imh_f32: null args"); return IMH_ERR_ARG; }
    F32Params p;
    p.X = a->X; p.W = a->W; p.Y = a->Y; p.bias = a->bias; p.residual = a->residual; p.gamma = a->gamma; p.beta = a->beta; p.ws = a->ws;
    p.M = a->M; p.N = a->N; p.K = a->K; p.ldx = a->ldx; p.ldw = a->ldw; p.ldy = a->ldy; p.ldr = a->ldr;
    p.conv = a->conv; p.H = a->H; p.Wd = a->Wd; p.Cin = a->Cin; p.Ho = a->Ho; p.Wo = a->Wo; p.up = a->up;
    p.B = a->B; p.HW = a->HW; p.C = a->C; p.groups = a->groups; p.nblk = a->nblk; p.silu = a->silu;
    p.eps = a->eps; p.scale = a->scale;
    if (a->pad != 0 && a->pad != 1) { set_error("imh_f32: pad must be 0 or 1"); return IMH_ERR_ARG; }
    p.stride = a->stride > 0 ? a->stride : 1; p.pad_lo = a->pad == 1 ? 0 : 1;
    p.add_a = a->add_a; p.add_b = a->add_b;
    return f32_launch(op, p, (hipStream_t)stream);
}

imh_plan* imh_plan_create(void) { return new (std::nothrow) imh_plan(); }
void imh_plan_destroy(imh_plan* p) {
    if (!p) return;
    drop_graph(p);
    delete p;
}
int imh_plan_add(imh_plan* p, int kind, const void* args, int ew_op, int tag) {
    if (!p || !args) { set_error("plan_add: null argument"); return IMH_ERR_ARG; }
    const op_entry* e = find_op(kind);
    if (!e) { set_error("plan_add: unknown kind %d", kind); return IMH_ERR_ARG; }
    imh_op o;
    memset(&o, 0, sizeof(o));
    o.kind = kind; o.ew_op = ew_op; o.tag = tag;
    memcpy(&o.u, args, e->size);
    p->ops.push_back(o);
    drop_graph(p);
    return (int)p->ops.size() - 1;
}
int imh_plan_size(const imh_plan* p) { return p ? (int)p->ops.size() : 0; }
int imh_plan_update(imh_plan* p, int index, const void* args) {
    if (!p || !args || index < 0 || index >= (int)p->ops.size()) { set_error("plan_update: bad index"); return IMH_ERR_ARG; }
    memcpy(&p->ops[index].u, args, find_op(p->ops[index].kind)->size);          // (imh_plan_add let no other kind in)
    drop_graph(p);
    return IMH_OK;
}
int imh_plan_run_range(imh_plan* p, int first, int last, void* stream) {
    if (!p || first < 0 || last > (int)p->ops.size() || first > last) { set_error("plan_run: bad range"); return IMH_ERR_ARG; }
    for (int i = first; i < last; ++i) {
        int rc = run_op(p->ops[i], (hipStream_t)stream);
        if (rc != IMH_OK) return rc;
    }
    return IMH_OK;
}
int imh_plan_run(imh_plan* p, void* stream) { return imh_plan_run_range(p, 0, p ? (int)p->ops.size() : 0, stream); }

int imh_plan_capture(imh_plan* p, void* stream) {
    if (!p) { set_error("plan_capture: null plan"); return IMH_ERR_ARG; }
    drop_graph(p);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { set_error("plan_capture: begin: %s", hipGetErrorString(e)); return IMH_ERR_LAUNCH; }
    int rc = imh_plan_run(p, stream);
    e = hipStreamEndCapture(s, &p->graph);
    if (rc != IMH_OK) { drop_graph(p); return rc; }
    if (e != hipSuccess) { set_error("plan_capture: end: %s", hipGetErrorString(e)); drop_graph(p); return IMH_ERR_LAUNCH; }
    e = hipGraphInstantiate(&p->exec, p->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { set_error("plan_capture: instantiate: %s", hipGetErrorString(e)); drop_graph(p); return IMH_ERR_LAUNCH; }
    return IMH_OK;
}
int imh_plan_replay(imh_plan* p, void* stream) {
    if (!p || !p->exec) { set_error("plan_replay: plan not captured"); return IMH_ERR_ARG; }
    hipError_t e = hipGraphLaunch(p->exec, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("plan_replay: %s", hipGetErrorString(e)); return IMH_ERR_LAUNCH; }
    return IMH_OK;
}
int imh_plan_time_ops(imh_plan* p, void* stream, float* ms, int n) {
    if (!p || !ms || n < (int)p->ops.size()) { set_error("plan_time_ops: bad arguments"); return IMH_ERR_ARG; }
    hipStream_t s = (hipStream_t)stream;
    const int cnt = (int)p->ops.size();
    std::vector<hipEvent_t> ev(cnt + 1);
    for (auto& e : ev) hipEventCreate(&e);
    int rc = IMH_OK;
    hipEventRecord(ev[0], s);
    for (int i = 0; i < cnt && rc == IMH_OK; ++i) {
        rc = run_op(p->ops[i], s);
        hipEventRecord(ev[i + 1], s);
    }
    hipStreamSynchronize(s);
    if (rc == IMH_OK)
        for (int i = 0; i < cnt; ++i) hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
    for (auto& e : ev) hipEventDestroy(e);
    return rc;
}
int imh_plan_get_tag(const imh_plan* p, int index) {
    return (p && index >= 0 && index < (int)p->ops.size()) ? p->ops[index].tag : -1;
}
int imh_plan_get_kind(const imh_plan* p, int index) {
    return (p && index >= 0 && index < (int)p->ops.size()) ? p->ops[index].kind : -1;
}

}  // extern "C"
