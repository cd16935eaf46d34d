// Fused QKV + cross-attention with N masked image prompts for gfx950 (include/imh_regions.h) -- diffusers' IPAdapterAttnProcessor2_0 with
// ip_adapter_masks and several images per adapter, in ONE launch:
//
//     q        = to_q( LayerNorm(x) )
//     O[b,q,h] = softmax(q K^T / 8) V  +  sum_{i < N}  (g * w_i) * m_i[q] * softmax(q K_i^T / 8) V_i
//
// xattn.hip's one-head form (one workgroup = (batch, head, 128 queries) = 4 waves x 32 queries, half items as there) with the second pass
// turned into a run-time loop over the N image prompts.  When an image's result is folded in, a lane owns ONE query row, so the mask is one
// fp32 value per lane and pass: wq = (g * w_i) * m_i[q], inv = wq / l_tot, fin += o * inv -- with N = 1, w = 1, m = 1 operation for
// operation what xattn_kernel<T, 2, LNQ> computes (the same bits; tests/test_gpu_ip_regions.py).
//
// The item decode and the to_q prologue below RESTATE xattn_kernel's (same staging map, same MFMA order, same folded LayerNorm).  They are a
// copy on purpose: calling one shared routine from xattn_kernel changed that kernel's generated code (DESIGN.md "Regional image prompts"),
// and the existing launches keep their instruction streams.
// The key phase is not attn_core's pass-by-pass ring: text tiles and image tiles form ONE sequence through a two-slot LDS-DMA ring
// (tile j + 1 in flight under tile j's arithmetic, also across the pass boundaries -- an image pass is a single 64-key tile holding 4 or 16
// valid keys, and a drained ring per pass would cost a full L2 round trip for every image).  Per tile the body is attn_tile (imh_attn_core.h),
// the resident-tile form the wide kernel of xattn.hip already runs bit-identically to attn_core.
#include "imh_attn_core.h"
#include "imh_lnstats.h"

namespace imh {

constexpr int XR_STAGE = 128 * 128 + 64 * 128;     // X tile (128 rows) + Wq tile (64 rows), 128 B per row
// items per XCD dealt as two 64-query halves (xattn.hip's rule; host and device agree on the grid: 8 * (per + split) workgroups)
__host__ __device__ __forceinline__ int xregions_split(const int per) { return (per > 32 && per < 64) ? per - 32 : 0; }

template <typename T, bool LNQ>
__global__ __launch_bounds__(256, 2) void xattn_regions_kernel(const XRegionParams rp) {
    constexpr int NW = 4;
    typedef typename Vec<T>::v8 v8;
    static_assert(2 * XR_STAGE <= ATT_STAGES * 2 * ATT_TILE_BYTES, "the projection stages alias the K / V^T ring");
    __shared__ __attribute__((aligned(16))) unsigned char smem[ATT_STAGES * 2 * ATT_TILE_BYTES];
    const XAttnParams& xp = rp.x;
    const AttnParams& p = xp.a;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    (void)hi;
    // ---- the item: XCD-aware head-major order, the items of an XCD beyond its 32nd dealt as 64-query halves (xattn_kernel) ----
    const int gx = (p.Lq + 32 * NW - 1) / (32 * NW);
    const int items = gx * p.H * p.B;
    const int per = (items + 7) >> 3;
    const int split = xp.split;
    const int jx = blockIdx.x >> 3;
    int item, qoff = 0, nq = 32 * NW;
    if (jx < per - split) item = (blockIdx.x & 7) * per + jx;
    else {
        const int k = jx - (per - split);
        if (k >= 2 * split) return;
        item = (blockIdx.x & 7) * per + (per - split) + (k >> 1);
        qoff = (k & 1) * 64; nq = 64;
    }
    if (item >= items) return;
    const int hb = item / gx, qblk = item - hb * gx;
    const int b = hb / p.H, h = hb - b * p.H;
    const int q0 = qblk * (32 * NW) + qoff;
    const bool act = wave * 32 < nq;           // (wave-uniform) the waves of a half item beyond its 64 queries only help staging

    // ---- prologue: Q^T = Wq_h X^T (xattn_kernel's, restated) ----
    const unsigned char* xsrc[4];
    const unsigned char* wsrc[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = xq_stage_xrow(i, wave, lane);
        const int ch = stage_chunk_x(row, lane);
        xsrc[i] = (const unsigned char*)((const T*)xp.X + ((size_t)b * p.Lq + min(q0 + row, p.Lq - 1)) * xp.ldx + ch * 8);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = xq_stage_wrow(i, wave, lane);
        const int ch = stage_chunk_x(row, lane);
        wsrc[i] = (const unsigned char*)((const T*)xp.Wq + ((size_t)h * 64 + row) * xp.ldw + ch * 8);
    }
    auto stage = [&](int buf, int kt) {
        unsigned char* xs = smem + buf * XR_STAGE;
        unsigned char* ws = xs + 128 * 128;
        if (act) {
#pragma unroll
            for (int i = 0; i < 4; ++i) glds16(xsrc[i] + (size_t)kt * 128, xs + (wave * 32 + i * 8) * 128);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(wsrc[i] + (size_t)kt * 128, ws + (wave * 16 + i * 8) * 128);
    };
    int xoff[4], woff[2][4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        xoff[ks] = xq_x_off(wave, lane, ks);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) woff[dt][ks] = 128 * 128 + xq_w_off(dt, lane, ks);
    }
    f32x16 qa[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) qa[dt][r] = 0.f;
    float st_s = 0.f, st_q = 0.f;

    const int nkt = xp.C / 64;
    stage(0, 0);
    if constexpr (LNQ) {           // precomputed row statistics (imh_lnstats.h): lane (q, hi) merges its query row's slots
        const f32x2s mr = merge_row_stats(xp.ln_stats, b * p.Lq + min(q0 + wave * 32 + (lane & 31), p.Lq - 1), xp.ln_slots, xp.C, xp.ln_eps);
        st_s = mr[0]; st_q = mr[1];
    }
    for (int kt = 0; kt < nkt; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's part of tile kt has landed
        __builtin_amdgcn_s_barrier();                         // ... everyone's has; tile kt-1 is fully consumed
        asm volatile("" ::: "memory");
        if (kt + 1 < nkt) stage((kt + 1) & 1, kt + 1);
        const unsigned char* sb = smem + (kt & 1) * XR_STAGE;
        if (act) {
            v8 xf[4], wf[2][4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                xf[ks] = *(const v8*)(sb + xoff[ks]);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) wf[dt][ks] = *(const v8*)(sb + woff[dt][ks]);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) qa[dt] = mfma32(wf[dt][ks], xf[ks], qa[dt]);
        }
        asm volatile("" ::: "memory");
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // every wave is done with the projection stages: the K / V^T ring may reuse them

    // ---- accumulators -> Q^T B-operand fragments of the key loop (xattn_kernel's hand-over) ----
    v8 qf[4];
    {
        float mean = 0.f, rstd = 1.f;
        if constexpr (LNQ) { mean = st_s; rstd = st_q; }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = qa[dt][rg * 4 + e];
                if constexpr (LNQ) {
                    const int d = h * 64 + att_o_dim(dt, rg * 4, hi);          // 4 consecutive head dims
                    const f32x4 s4 = *(const f32x4*)(xp.ln_s + d), c4 = *(const f32x4*)(xp.ln_c + d);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fma_nopk(rstd, fma_nopk(-mean, s4[e], v[e]), c4[e]);   // scalar on purpose (IMH_KERNEL note)
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) qf[xq_sd(dt, rg * 4 + e)][xq_slot(rg * 4 + e)] = from_f32<T>(v[e]);
            }
    }

    // ---- key phase: pass 0 = the text keys, pass 1 + i = image prompt i.  Tile j of the whole sequence sits in ring slot j & 1. ----
    const float c = p.scale * LOG2E;
    const float gate = p.scale2_tab ? p.scale2_tab[*p.step] : p.scale2;
    const int nt1 = (p.Lk + ATT_KV - 1) / ATT_KV;
    const int nt2 = (p.Lk2 + ATT_KV - 1) / ATT_KV;
    const int NT = nt1 + rp.n_img * nt2;
    // this lane's query row: the token-row clamp of the prologue, so the rows past Lq of a ragged block read mask[i][Lq - 1] (never stored)
    const int qrow = min(q0 + wave * 32 + (lane & 31), p.Lq - 1);
    auto stage_kv = [&](const int j) {
        unsigned char* ks = smem + (j & 1) * 2 * ATT_TILE_BYTES;
        if (j < nt1) {
            attn_stage_tile<T>((const T*)p.K, (const T*)p.Vt, p.Lk_pad, p.ldk, p.ldvt, b, h, j, ks, ks + ATT_TILE_BYTES, wave, lane);
        } else {
            const int i = (j - nt1) / nt2, t = (j - nt1) - i * nt2;
            attn_stage_tile<T>((const T*)p.K2, (const T*)p.Vt2, p.Lk2_pad, p.ldk2, p.ldvt2, b * rp.n_img + i, h, t, ks, ks + ATT_TILE_BYTES, wave, lane);
        }
    };
    f32x16 fin[2], o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { fin[dt][r] = 0.f; o[dt][r] = 0.f; }
    float m_run = NEG_BIG, l_run = 0.f;
    stage_kv(0);
    int pass = 0, t = 0;                     // tile j = tile t of pass `pass`
    // (g * w_i) and m_i[q] of the running image pass, and of the next one: fetched one tile ahead (the mask value with one ordinary vector
    // load per lane and pass), so that folding a pass in never waits for memory
    float wg = 1.f, mq = 1.f, wg_next = 1.f, mq_next = 1.f;
    for (int j = 0; j < NT; ++j) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's part of tile j has landed
        __builtin_amdgcn_s_barrier();                         // ... everyone's has; tile j - 1 is fully consumed
        asm volatile("" ::: "memory");
        const bool last = t + 1 == (pass == 0 ? nt1 : nt2);   // (wave-uniform) tile j completes its pass
        if (j + 1 < NT) {
            if (last) {                                       // tile j + 1 opens image `pass`
                mq_next = rp.mask[(size_t)pass * rp.ldm + qrow];
                wg_next = gate * (rp.weights ? rp.weights[pass] : 1.0f);
            }
            stage_kv(j + 1);
        }
        const unsigned char* ks = smem + (j & 1) * 2 * ATT_TILE_BYTES;
        attn_tile<T>(ks, ks + ATT_TILE_BYTES, qf, lane, t * ATT_KV, pass == 0 ? p.Lk : p.Lk2, c, o, m_run, l_run);
        asm volatile("" ::: "memory");
        ++t;
        if (last) {                                           // fold the pass in: the lane owns query row q, so the mask is one value
            const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
            const float wq = pass == 0 ? 1.0f : wg * mq;
            const float inv = wq / l_tot;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { fin[dt][r] += o[dt][r] * inv; o[dt][r] = 0.f; }
            m_run = NEG_BIG; l_run = 0.f;
            wg = wg_next; mq = mq_next;
            ++pass; t = 0;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // nobody reads the ring any more: its rows become the O staging rows
    if (act) attn_store<T, NW>(p, smem, fin, b, h, q0, wave, lane);
    tail_prefetch(p.pf_ptr, p.pf_bytes, item, items, tid, 64 * NW);
}

// shape rules of imh_cross_attention (xattn_launch) plus the regions' own; pointers and alignment are api.hip's
int xattn_regions_launch(const XRegionParams& rp, int dtype, hipStream_t stream) {
    const XAttnParams& xp = rp.x;
    const AttnParams& p = xp.a;
    const char* who = "cross_attention_regions";
    if (rp.n_img < 1 || rp.n_img > XR_MAX_IMAGES) { set_error("%s: n_img=%d must be 1 .. %d", who, rp.n_img, XR_MAX_IMAGES); return IMH_ERR_SHAPE; }
    if (p.Lk <= 0 || p.Lk_pad % ATT_KV != 0 || p.Lk_pad < p.Lk) {
        set_error("%s: Lk=%d Lk_pad=%d (pad must be a multiple of 64 and >= Lk)", who, p.Lk, p.Lk_pad);
        return IMH_ERR_SHAPE;
    }
    if (p.Lk2 <= 0 || p.Lk2_pad % ATT_KV != 0 || p.Lk2_pad < p.Lk2) { set_error("%s: Lk2=%d Lk2_pad=%d invalid", who, p.Lk2, p.Lk2_pad); return IMH_ERR_SHAPE; }
    if (xp.C <= 0 || xp.C % 64) { set_error("%s: C=%d must be a positive multiple of 64", who, xp.C); return IMH_ERR_SHAPE; }
    if ((xp.ldx & 7) || (xp.ldw & 7) || (p.ldk & 7) || (p.ldvt & 7) || (p.ldo & 7) || (p.ldk2 & 7) || (p.ldvt2 & 7)) {
        set_error("%s: leading dimensions must be multiples of 8 elements", who);
        return IMH_ERR_SHAPE;
    }
    if (p.B <= 0 || p.H <= 0 || p.Lq <= 0) { set_error("%s: empty problem", who); return IMH_ERR_SHAPE; }
    if (rp.ldm < p.Lq) { set_error("%s: ldm=%d is shorter than a mask row of Lq=%d values", who, rp.ldm, p.Lq); return IMH_ERR_SHAPE; }
    if (dtype != IMH_DT_BF16 && dtype != IMH_DT_F16) { set_error("%s: unknown dtype %d", who, dtype); return IMH_ERR_DTYPE; }
    const int items = ((p.Lq + 127) / 128) * p.H * p.B;
    const int per = (items + 7) / 8;
    XRegionParams rq = rp;
    rq.x.split = xregions_split(per);
    dim3 grid(8 * (per + rq.x.split));
#define IMH_XR(TT) do { \
        if (!xp.ln_s) hipLaunchKernelGGL((xattn_regions_kernel<TT, false>), grid, dim3(256), 0, stream, rq); \
        else hipLaunchKernelGGL((xattn_regions_kernel<TT, true>), grid, dim3(256), 0, stream, rq); } while (0)
    if (dtype == IMH_DT_BF16) IMH_XR(bf16_t);
    else IMH_XR(f16_t);
#undef IMH_XR
    return check_launch("xattn_regions_kernel");
}

}  // namespace imh
