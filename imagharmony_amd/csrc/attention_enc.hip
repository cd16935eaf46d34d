// Encoder attention with a generic head dim, bidirectional (include/imh.h imh_attention_enc) or causal (imh_attention_enc_causal):
// the CLIP vision towers behind the IP-Adapter image prompt (ViT-H/14: head dim 80, ViT-bigG/14: 104; 257 tokens) and the CLIP text
// towers behind the SDXL prompt (CLIP-L / OpenCLIP bigG: head dim 64, 77 tokens, causal), plain row-major Q / K / V with their own
// row strides -- e.g. three column ranges of the packed output of one QKV GEMM.
//
// One workgroup = 64 queries of one (batch, head): four waves of 16 queries each.  Keys go by in tiles of 64 through LDS with an
// online softmax, so any L runs.  Both products are computed TRANSPOSED on v_mfma_f32_16x16x32:
//   S^T[key][q] = K[key][:] . Q[q][:]       A = the K tile (LDS, row-major, head dim zero-padded to the K step of 32),
//                                           B = the wave's Q rows (registers for the whole kernel)
//   O^T[dv][q] += V^T[dv][key] P^T[key][q]  A = the V tile, transposed on its way into LDS, B = P^T
// S^T leaves the accumulators with the query on the lane (q = lane & 15) and 4 keys per 16-key block in the registers
// (key = 16 blk + 4 (lane >> 4) + reg).  That is already the B-operand layout of the second product up to the key order inside a
// 32-key step, so P never touches LDS: the V^T image stores key 32 s + 16 h + 4 g + r at column 32 s + 8 g + 4 h + r and both operands
// see the same order.  The softmax statistics of a query live in ONE lane group column (max / sum: registers, then two
// shuffles across lane >> 4), and the rescale of O^T by exp(m_old - m_new) is a per-lane scalar.
//
// CAUSAL (a compile-time parameter; the bidirectional instantiation is the kernel as it was): O[q] = softmax over keys <= q.  The
// workgroup of queries [q0, q0 + 64) visits the key tiles 0 .. q0 / 64 only -- later tiles are neither loaded nor staged -- and
// the mask key <= q bites in the last of them, the diagonal tile, alone (every key of an earlier tile is < q0 <= q).  A masked
// probability is an exact zero, so a finite K / V row of the future cannot reach an earlier query's result.
//
// Bounds: every global access is guarded -- keys and query rows at or beyond L and head dims at or beyond d are never loaded
// (zero-filled in LDS / registers, masked in the softmax) and never stored.
#include "imh_common.h"
#include "imh_kernels.h"

namespace imh {

constexpr int ENC_Q = 64;        // queries per workgroup (16 per wave)
constexpr int ENC_K = 64;        // keys per tile
constexpr int ENC_VLD = ENC_K + 8;   // row stride (elements) of the V^T image

// NKS = 32-wide contraction steps of Q K^T (head dim padded to 32 NKS with zeros), NDB = 16-wide blocks of output head dims
template <typename T, int NKS, int NDB, bool CAUSAL>
__global__ __launch_bounds__(256) void attn_enc_kernel(const EncAttnParams p) {
    // causal: key k0 = q0 of the diagonal tile is <= every query of the workgroup, so every visited tile has a valid first key for
    // every query and the running maximum is finite from the first tile on, as in the bidirectional form
    static_assert(ENC_Q == ENC_K, "the causal form relies on query blocks and key tiles of one size");
    typedef typename Vec<T>::v8 v8;
    typedef typename Vec<T>::v4 v4;
    constexpr int DP = 32 * NKS;          // padded contraction width
    constexpr int KLD = DP + 8;           // row stride (elements) of the K image
    constexpr int KCH = DP / 8;           // 16-B chunks per K row
    constexpr int KTASK = ENC_K * KCH / 256;   // K chunks per thread and tile (NKS)
    static_assert(ENC_K * KCH % 256 == 0, "whole rounds");
    __shared__ __attribute__((aligned(16))) T ks[ENC_K * KLD];
    __shared__ __attribute__((aligned(16))) T vt[NDB * 16 * ENC_VLD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * ENC_Q;
    const int L = p.L, d = p.d;
    const size_t row0 = (size_t)b * L;
    const T* Qg = (const T*)p.Q + h * d;
    const T* Kg = (const T*)p.K + h * d;
    const T* Vg = (const T*)p.V + h * d;

    // the wave's query rows as the B operand: lane (g, c) holds Q[q0 + 16 wave + c][32 s + 8 g .. + 8]
    v8 qf[NKS];
    {
        const int q = q0 + wave * 16 + c;
#pragma unroll
        for (int s = 0; s < NKS; ++s) {
            const int dc = 32 * s + 8 * g;
            v8 t = {};
            if (q < L && dc < d) t = *(const v8*)(Qg + (row0 + q) * p.ldq + dc);
            qf[s] = t;
        }
    }
    // V^T rows of the head dims in [d, 16 NDB) are never written by a tile: zero them once (they meet P in the MFMA)
    for (int i = tid; i < NDB * 16 * ENC_VLD / 8; i += 256) ((v8*)vt)[i] = v8{};

    // staging of one tile, global -> registers (guarded) and registers -> LDS
    v8 kr[KTASK];
    v8 vr[4];
    const int vquad = tid & 15, vch = tid >> 4;      // V task: keys 4 vquad .. + 4 of the tile, head dims 8 vch .. + 8
    const bool vtask = vch * 8 < d;
    auto load_tile = [&](const int k0) {
#pragma unroll
        for (int i = 0; i < KTASK; ++i) {
            const int t = tid + 256 * i, key = k0 + t / KCH, dc = (t % KCH) * 8;
            v8 x = {};
            if (key < L && dc < d) x = *(const v8*)(Kg + (row0 + key) * p.ldk + dc);
            kr[i] = x;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 4 * vquad + r;
            v8 x = {};
            if (vtask && key < L) x = *(const v8*)(Vg + (row0 + key) * p.ldv + vch * 8);
            vr[r] = x;
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KTASK; ++i) {
            const int t = tid + 256 * i;
            *(v8*)(ks + (t / KCH) * KLD + (t % KCH) * 8) = kr[i];
        }
        if (vtask) {
            // keys 4 vquad + r = 32 s + 16 hh + 4 gg + r  ->  column 32 s + 8 gg + 4 hh + r
            const int s = vquad >> 3, hh = (vquad >> 2) & 1, gg = vquad & 3;
            T* dst = vt + (vch * 8) * ENC_VLD + 32 * s + 8 * gg + 4 * hh;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v4 w;
                w[0] = vr[0][e]; w[1] = vr[1][e]; w[2] = vr[2][e]; w[3] = vr[3][e];
                *(v4*)(dst + e * ENC_VLD) = w;
            }
        }
    };

    f32x4 acc[NDB];
#pragma unroll
    for (int i = 0; i < NDB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -1e30f, lsum = 0.f;                    // running maximum (log2 domain) / this lane's share of the running sum
    const float sc2 = p.scale * 1.4426950408889634f;

    // causal: the tiles up to the diagonal one (q0 < L, so it exists); kend = one past the last key this lane's query sees -- below
    // min(L, q + 1) only inside the diagonal tile
    const int ntiles = CAUSAL ? (int)blockIdx.x + 1 : (L + ENC_K - 1) / ENC_K;
    int kend = L;
    if constexpr (CAUSAL) kend = min(L, q0 + wave * 16 + c + 1);
    load_tile(0);
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                             // the previous tile's readers are done (and the zero fill above)
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile((t + 1) * ENC_K);
        const int k0 = t * ENC_K;

        // S^T: four 16-key blocks
        f32x4 sacc[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NKS; ++s) {
                const v8 kf = *(const v8*)(ks + (16 * blk + c) * KLD + 32 * s + 8 * g);
                a = mfma16(kf, qf[s], a);
            }
            sacc[blk] = a;
        }
        // online softmax of query c over this tile's keys 16 blk + 4 g + r
        float mx = -1e30f;
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * blk + 4 * g + r;
                const float v = key < kend ? sacc[blk][r] * sc2 : -1e30f;
                sacc[blk][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(m, mx);             // finite from the first tile on: key 0 is always valid (and <= every query)
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        m = mnew;
        float ps = 0.f;
        v8 pf[2];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 16 * blk + 4 * g + r;
                const float e = key < kend ? __builtin_amdgcn_exp2f(sacc[blk][r] - mnew) : 0.f;
                ps += e;
                pf[blk >> 1][4 * (blk & 1) + r] = from_f32<T>(e);
            }
        lsum = lsum * alpha + ps;
#pragma unroll
        for (int i = 0; i < NDB; ++i) acc[i] *= alpha;
        // O^T += V^T P^T
#pragma unroll
        for (int i = 0; i < NDB; ++i)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const v8 vf = *(const v8*)(vt + (16 * i + c) * ENC_VLD + 32 * s + 8 * g);
                acc[i] = mfma16(vf, pf[s], acc[i]);
            }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
    const int q = q0 + wave * 16 + c;
    if (q < L) {
        T* Og = (T*)p.O + (row0 + q) * p.ldo + h * d;
#pragma unroll
        for (int i = 0; i < NDB; ++i) {
            const int dv = 16 * i + 4 * g;
            if (dv < d) {
                v4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = from_f32<T>(acc[i][r] * inv);
                *(v4*)(Og + dv) = w;
            }
        }
    }
}

template <typename T, int NDB>
static void enc_launch_one(const EncAttnParams& p, hipStream_t stream) {
    dim3 grid((p.L + ENC_Q - 1) / ENC_Q, p.H, p.B);
    if (p.causal) hipLaunchKernelGGL((attn_enc_kernel<T, (NDB + 1) / 2, NDB, true>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((attn_enc_kernel<T, (NDB + 1) / 2, NDB, false>), grid, dim3(256), 0, stream, p);
}

template <typename T>
static void enc_launch_t(const EncAttnParams& p, hipStream_t stream) {
    switch ((p.d + 15) / 16) {
        case 1: enc_launch_one<T, 1>(p, stream); break;
        case 2: enc_launch_one<T, 2>(p, stream); break;
        case 3: enc_launch_one<T, 3>(p, stream); break;
        case 4: enc_launch_one<T, 4>(p, stream); break;
        case 5: enc_launch_one<T, 5>(p, stream); break;
        case 6: enc_launch_one<T, 6>(p, stream); break;
        case 7: enc_launch_one<T, 7>(p, stream); break;
        default: enc_launch_one<T, 8>(p, stream); break;
    }
}

int attention_enc_launch(const EncAttnParams& p, int dtype, hipStream_t stream) {
    if (dtype != IMH_DT_BF16 && dtype != IMH_DT_F16) { set_error("attention_enc: unknown dtype %d", dtype); return IMH_ERR_DTYPE; }
    if (p.d <= 0 || p.d % 8 || p.d > 128) { set_error("attention_enc: head dim %d must be a multiple of 8 in [8, 128]", p.d); return IMH_ERR_SHAPE; }
    if (p.B <= 0 || p.H <= 0 || p.L <= 0 || p.B > 65535 || p.H > 65535) {
        set_error("attention_enc: unsupported shape B=%d H=%d L=%d", p.B, p.H, p.L); return IMH_ERR_SHAPE;
    }
    const int w = p.H * p.d;
    if (p.ldq < w || p.ldk < w || p.ldv < w || p.ldo < w || (p.ldq | p.ldk | p.ldv | p.ldo) % 8) {
        set_error("attention_enc: row strides (%d, %d, %d, %d) must be multiples of 8 and at least H*d=%d", p.ldq, p.ldk, p.ldv, p.ldo, w);
        return IMH_ERR_SHAPE;
    }
    if (((uintptr_t)p.Q | (uintptr_t)p.K | (uintptr_t)p.V | (uintptr_t)p.O) & 15) {
        set_error("attention_enc: Q / K / V / O must be 16-byte aligned"); return IMH_ERR_ARG;
    }
    if (dtype == IMH_DT_BF16) enc_launch_t<bf16_t>(p, stream);
    else enc_launch_t<f16_t>(p, stream);
    return check_launch("attn_enc_kernel");
}

}  // namespace imh
