// Small memory-/latency-bound kernels around the UNet forward and the denoise loop, gfx950.
//   EW_TIMESTEP   diffusers Timesteps(dim, flip_sin_to_cos=True, shift 0)      
//   EW_SILU       SiLU on the time embedding before time_emb_proj               (App. A ResnetBlock2D)
//   EW_CONCAT     channel concat of NHWC tensors (up-block skip connections)    (App. A.6); its FreeU form (the concat behind
//                 diffusers' apply_freeu) and its identity-attention form (perturbed-attention guidance: V rows out of V^T)
//   EW_CONV_IN    conv_in 3x3 (4 | 9 -> C0) reading NCHW fp32 latents, fusing CFG duplication
//                 (custom_pipelines.py:332) and scale_model_input (:334); writes NHWC; with 9 channels (the SDXL inpainting
//                 UNet) the last five, [mask | masked-image latents], come from a second, step-invariant buffer
//   EW_CFG_STEP   CFG combine (custom_pipelines.py:348-350) + linear scheduler update
//                 x' = cx*x + ce*eps (DDIM eta=0 / Euler), noise pred read
//                 NHWC, latents kept NCHW fp32 (custom_pipelines.py:357); optionally followed in the same pass by the
//                 masked blend of SDXL inpainting on a 4-channel UNet
//   EW_CFG_MSTEP  the same launch for the multistep and ancestral samplers (DPM-Solver++ 2M, its SDE variant, Euler ancestral):
//                 x' = cx*x + ce*eps + ch*h + cn*z and h' = hx*x + he*eps from one six-column table row, h a history slot,
//                 z the step's row of a host-filled noise bank -- or, in the seeded form (imh_step_seeded), generated in the launch by
//                 Philox4x32-10 from the sample's seed row, the table row and the element index (imh_philox.h): no bank, no host draw
//   randn_seeded  the generator's rows by themselves (imh_randn_seeded): normals or raw words, for tests and oracle comparisons
//                 -- all three step forms optionally with the third, perturbed block of perturbed-attention guidance (i2 = 1)
//   EW_CFG_RESCALE per-sample factor of rescale_noise_cfg (custom_pipelines.py:351-354; arXiv 2305.08891 3.4):
//                 phi * std(eps_text) / std(eps_cfg) + (1 - phi), consumed by EW_CFG_STEP through `w`
//   EW_SOFTMAX    row softmax of fp32 scores -> T probabilities (the VAE mid-block attention: one head of width
//                 512 over 4096-16384 tokens, materialised as GEMM -> softmax -> GEMM; once per image)
//   EW_ROW_STATS  (sum, M2) of token rows, the stand-alone LayerNorm-statistics producer (imh_lnstats.h)
//   EW_STEP_ROW   y[0:n] = a[*step * n + 0:n]: the denoise step's row of a per-schedule table (the stacked time-embedding projections,
//                 computed once per schedule for all steps instead of five launches per step)
//   EW_GATHER_ROWS y[r] = table[idx[r]] (+ add[r mod P]): the CLIP text towers' token + position embedding, and their EOS pooling
//   EW_CAST_F32   T -> fp32 copy (debug / host-side plumbing)
//   EW_STEP_SET   the device-resident step counter (lets 30 graph replays run with no host updates)
// Per-step scalars (timestep, scheduler coefficients, input scale) may come from device tables
// indexed by *step instead of the immediate f0..f2 fields.
#include <algorithm>

#include "imh_common.h"
#include "imh_kernels.h"
#include "imh_philox.h"

namespace imh {

enum : int { EW_TIMESTEP = 0, EW_SILU = 1, EW_CONCAT = 2, EW_CONV_IN = 3, EW_CFG_STEP = 4, EW_CAST_F32 = 5,
             EW_ADD = 6, EW_STEP_SET = 7, EW_CFG_RESCALE = 8, EW_SOFTMAX = 9, EW_ROW_STATS = 10, EW_STEP_ROW = 11, EW_GATHER_ROWS = 12,
             EW_CFG_MSTEP = 13 };

// a: fp32 values [n_vals]; y: T [n_vals, dim]; cos first, then sin.
template <typename T>
__global__ void timestep_kernel(const EwParams p) {
    const int dim = p.i0, half = dim >> 1;
    const long long total = p.n * half;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(i / half), j = (int)(i % half);
        const float t = p.step ? ((const float*)p.a)[*p.step] : ((const float*)p.a)[v];
        const float f = expf(-9.210340371976184f * (float)j / (float)half);   // ln(10000)
        const float a = t * f;
        T* y = (T*)p.y + (size_t)v * dim;
        y[j] = from_f32<T>(cosf(a));
        y[half + j] = from_f32<T>(sinf(a));
    }
}

template <typename T>
__global__ void silu_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    const long long nv = p.n >> 3;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        v8 v = ((const v8*)p.a)[i], o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(silu_f(to_f32(v[e])));
        ((v8*)p.y)[i] = o;
    }
}

template <typename T>
__global__ void add_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    const long long nv = p.n >> 3;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) {
        v8 u = ((const v8*)p.a)[i], v = ((const v8*)p.b)[i], o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(to_f32(u[e]) + to_f32(v[e]));
        ((v8*)p.y)[i] = o;
    }
}

// y[pix, 0:C1] = a[pix], y[pix, C1:C1+C2] = b[pix]   (n = pixels, C1 = i0, C2 = i1; multiples of 8)
template <typename T>
__global__ void concat_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    const int c1 = p.i0 >> 3, c2 = p.i1 >> 3, ct = c1 + c2;
    const long long total = p.n * ct;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long pix = i / ct;
        const int c = (int)(i - pix * ct);
        v8 v = c < c1 ? ((const v8*)p.a)[pix * c1 + c] : ((const v8*)p.b)[pix * c2 + (c - c1)];
        ((v8*)p.y)[i] = v;
    }
}

// EW_CONCAT, the FreeU form (imh.h; i2 = H > 0, i3 = W): diffusers' apply_freeu at the up blocks' torch.cat([hidden, skip], 1),
//   y[pix, c]      = round_T(a[pix, c] * f0)            c <  i4        (the backbone scale b on the leading hidden channels)
//   y[pix, c]      = a[pix, c]                          i4 <= c < C1
//   y[pix, C1 + c] = round_T(x + (f1 - 1) * low(x))     x = b[pix, c]  (fourier_filter(threshold = 1, scale = s = f1) of the skip)
// With threshold 1 the mask keeps the frequency pairs {-1, 0} x {-1, 0}, so per (sample, channel) plane, with t = 2 pi y / H and
// u = 2 pi x / W, low is the real part of four Fourier components and needs seven plane sums:
//   HW * low(y, x) = S + (Ac cos t + As sin t) + (Bc cos u + Bs sin u) + (Dc cos(t + u) + Ds sin(t + u)),
//   S = sum x, (Ac, As) = sum x (cos t, sin t), (Bc, Bs) = sum x (cos u, sin u), (Dc, Ds) = sum x (cos, sin)(t + u).
// One workgroup owns FREEU_LANES channel quads (32 bytes per pixel) of every pixel of one sample: four lanes per pixel, 256 pixels per
// sweep (8-byte loads, eight sweeps in flight).  Pass 1 sweeps the slab and keeps the 7 x 4 sums per lane; they are merged by a fixed butterfly inside the wave and in wave
// order across the workgroup through LDS (no atomics, no workspace: the bits depend on nothing but the operands).  Pass 2 reads the
// slab again -- from the XCD's L2, which the same CU has just filled; a slab is 32 B x HW, 32 to 512 KiB at the SDXL shapes -- and
// stores the filtered values.  cos / sin of t and u come from per-workgroup tables in LDS (H + W sincospi calls instead of two per
// pixel), cos / sin of t + u from the angle-sum identity.  The hidden channels are a scaled copy by the workgroups behind the slab
// owners.
// Sums, tables and the evaluation of low are float64, and the result is rounded to T once (through fp32 rounded to odd).  fp32 would
// not do: where x and (s - 1) * low cancel -- one element in 10^5 lands 2^-15 below |x| -- an ulp of the RESULT is 2^-23 |x| in bf16,
// the size of ONE fp32 rounding of the plane sums, and the launch is held to 1 ulp of the float64 statement
// (tests/test_gpu_freeu.py; an fp32 FFT is 89 ulp off at such an element).  At 14 fp64 multiply-adds per element the arithmetic
// stays below the launch's memory time.  LDS: 2 (H + W) + 1904 doubles (16.9 KiB at 64 x 64).
constexpr int FREEU_THREADS = 1024, FREEU_LANES = 4, FREEU_SUMS = 7;
constexpr int FREEU_COEF = FREEU_LANES * FREEU_SUMS * 4;                             // merged sums of a slab
constexpr int FREEU_RED = (FREEU_THREADS / 64 + 1) * FREEU_COEF;                     // per-wave partials, then the merged coefficients

static inline size_t freeu_lds_bytes(int H, int W) { return ((size_t)2 * (H + W) + FREEU_RED) * sizeof(double); }

// float64 -> T with ONE rounding: to fp32 rounded to odd (the inexact bit survives in the last place), then the usual nearest-even
template <typename T>
__device__ __forceinline__ T from_f64(double d) {
    const double ad = fabs(d);
    float af = (float)ad;
    if ((double)af != ad && !(__float_as_uint(af) & 1u)) af = __uint_as_float(__float_as_uint(af) + ((double)af < ad ? 1u : 0xffffffffu));
    return from_f32<T>(copysignf(af, (float)d));
}

template <typename T>
__global__ __launch_bounds__(FREEU_THREADS) void freeu_concat_kernel(const EwParams p, int slabs_per_sample, int nslab) {
    typedef typename Vec<T>::v8 v8;
    typedef typename Vec<T>::v4 v4;
    extern __shared__ double fl[];
    const int c1 = p.i0 >> 3, ct = (p.i0 + p.i1) >> 3;
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= nslab) {
        // the hidden half: channels [0, i4) scaled in fp32 and rounded once (torch's a[..., :i4] * b in T), the rest copied
        // (four vectors in flight per thread: these workgroups run at the filter's register budget, one per CU)
        const long long total = p.n * c1, nthr = (long long)(gridDim.x - nslab) * FREEU_THREADS;
        for (long long i0 = (long long)(blockIdx.x - nslab) * FREEU_THREADS + tid; i0 < total; i0 += 4 * nthr) {
            v8 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * nthr < total) v[u] = ((const v8*)p.a)[i0 + u * nthr];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long i = i0 + u * nthr;
                if (i >= total) break;
                const long long pix = i / c1;
                const int c = (int)(i - pix * c1) * 8;
                if (c < p.i4) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (c + e < p.i4) v[u][e] = from_f32<T>(to_f32(v[u][e]) * p.f0);
                }
                ((v8*)p.y)[pix * ct + (c >> 3)] = v[u];
            }
        }
        return;
    }
    const int H = p.i2, W = p.i3, HW = H * W;
    const int q2 = p.i1 >> 2, qt = (p.i0 + p.i1) >> 2;       // channel quads of the skip and of y
    double* cy = fl;
    double* sy = cy + H;
    double* cx = sy + H;
    double* sx = cx + W;
    double* red = sx + W;
    double* coef = red + (FREEU_THREADS / 64) * FREEU_COEF;
    for (int i = tid; i < H; i += FREEU_THREADS) sincospi(2.0 * (double)i / (double)H, sy + i, cy + i);
    for (int i = tid; i < W; i += FREEU_THREADS) sincospi(2.0 * (double)i / (double)W, sx + i, cx + i);
    __syncthreads();
    // slab order: workgroups that share an XCD (blockIdx % 8, as the dispatcher is observed to deal them; speed only) take neighbouring
    // slabs, so that the four slabs of a 128-byte line are fetched into one L2
    const int xcd = blockIdx.x & 7, chunk = nslab >> 3, rem = nslab & 7;
    const int slab = xcd * chunk + (xcd < rem ? xcd : rem) + (blockIdx.x >> 3);
    const int smp = slab / slabs_per_sample;
    const int q = tid & (FREEU_LANES - 1), quad = (slab - smp * slabs_per_sample) * FREEU_LANES + q;
    const bool live = quad < q2;                    // (the last slab of a sample may be narrower)
    const v4* src = (const v4*)p.b + (long long)smp * HW * q2 + quad;
    constexpr int PR = FREEU_THREADS / FREEU_LANES; // pixels per sweep
    double acc[FREEU_SUMS][4];
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = 0.0;
    if (live) {
#pragma unroll 8
        for (int px = tid / FREEU_LANES; px < HW; px += PR) {
            const v4 v = src[(long long)px * q2];
            const int yy = px / W, xx = px - yy * W;
            const double ct_ = cy[yy], st_ = sy[yy], cu = cx[xx], su = sx[xx];
            const double cd = ct_ * cu - st_ * su, sd = st_ * cu + ct_ * su;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double f = (double)to_f32(v[e]);
                acc[0][e] += f;
                acc[1][e] = fma(f, ct_, acc[1][e]);
                acc[2][e] = fma(f, st_, acc[2][e]);
                acc[3][e] = fma(f, cu, acc[3][e]);
                acc[4][e] = fma(f, su, acc[4][e]);
                acc[5][e] = fma(f, cd, acc[5][e]);
                acc[6][e] = fma(f, sd, acc[6][e]);
            }
        }
    }
    // lanes q, q + 4, .. of a wave hold the same channels: butterfly over the sixteen, then the waves in order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double v = acc[k][e];
#pragma unroll
            for (int o = FREEU_LANES; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
            acc[k][e] = v;
        }
    if (lane < FREEU_LANES) {
#pragma unroll
        for (int k = 0; k < FREEU_SUMS; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[((wave * FREEU_LANES + lane) * FREEU_SUMS + k) * 4 + e] = acc[k][e];
    }
    __syncthreads();
    if (tid < FREEU_COEF) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < FREEU_THREADS / 64; ++w) s += red[w * FREEU_COEF + tid];
        coef[tid] = s * (((double)p.f1 - 1.0) / (double)HW);
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int k = 0; k < FREEU_SUMS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[k][e] = coef[(q * FREEU_SUMS + k) * 4 + e];
    v4* dst = (v4*)p.y + (long long)smp * HW * qt + (p.i0 >> 2) + quad;
#pragma unroll 4
    for (int px = tid / FREEU_LANES; px < HW; px += PR) {
        const v4 v = src[(long long)px * q2];
        const int yy = px / W, xx = px - yy * W;
        const double ct_ = cy[yy], st_ = sy[yy], cu = cx[xx], su = sx[xx];
        const double cd = ct_ * cu - st_ * su, sd = st_ * cu + ct_ * su;
        v4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double low = acc[0][e] + (acc[1][e] * ct_ + acc[2][e] * st_) + (acc[3][e] * cu + acc[4][e] * su) + (acc[5][e] * cd + acc[6][e] * sd);
            o[e] = from_f64<T>((double)to_f32(v[e]) + low);
        }
        dst[(long long)px * qt] = o;
    }
}

// EW_CONCAT, the identity-attention form (imh.h; i5 = ldvt > 0, empty first part): the self-attention output of samples whose attention
// map is the identity (perturbed-attention guidance) is V itself, and V exists only transposed -- b = Vt [C = i1, ldvt], keys permuted
// inside every 16-group by vt_perm16 (imh_layout.h: runs 1 and 2 of 4 swapped).  So this is a transposing copy,
//   y[r, c] = Vt[c, col0 + 16 * (r / 16) + vt_perm16(r % 16)]      0 <= r < n, 0 <= c < C      (col0 = i4, y rows i3 elements apart)
// One workgroup moves a 64-key x 64-channel tile through LDS: 16-byte loads along the key axis (eight lanes cover a channel's 128
// bytes), each split into its two runs of four keys, which go to their LOGICAL place as 8-byte LDS writes (the un-permutation costs
// nothing: it is where the two halves are put); then every lane gathers the eight channels of one key as 16-bit LDS reads and stores
// 16 bytes along the channel axis (eight lanes cover a row's 128 bytes).  The tile is [channel][16 slots of four keys], 128-byte rows,
// slot s of channel c at s ^ (c >> 3) ^ ((c & 1) << 1) (idr_slot), which leaves neither side a bank conflict by the rules of the LDS
// (bank = dword mod 32 for the writes and for the 16-bit reads):
//   writes  a 16-lane group holds chunks j = 0..7 of channels c, c + 1 (c even, one c >> 3): per half its eight slots 4 (j >> 1) + (j & 1)
//           [+ 2] are distinct, the odd channel's are those XOR 2 -- a disjoint set -- so 16 lanes x 2 dwords fill the 32 banks once;
//   reads   a 32-lane group holds four keys of one slot x eight channel octets cc, and for element e reads channel 8 cc + e: slot
//           (r >> 2) ^ cc ^ ((e & 1) << 1), eight distinct slots = 16 distinct dwords, each read by the two lanes whose keys share it.
// Both dtypes are 16 bits wide and the launch never looks inside an element: one kernel.  Partial tiles (C % 64, n % 64) are guarded per
// 16-byte chunk on both sides (C % 8 == 0 and n % 16 == 0: a chunk is inside or outside as a whole).  8 KiB of LDS, no scratch.
constexpr int IDR_TILE = 64, IDR_THREADS = 256;

__device__ __forceinline__ int idr_slot(int c, int s) { return s ^ (c >> 3) ^ ((c & 1) << 1); }

__global__ __launch_bounds__(IDR_THREADS) void identity_rows_kernel(const EwParams p) {
    __shared__ uint2 tile[IDR_TILE][IDR_TILE / 4];
    const int C = p.i1, ldy = p.i3, col0 = p.i4, ldvt = p.i5, n = (int)p.n;
    const int k0 = blockIdx.x * IDR_TILE, c0 = blockIdx.y * IDR_TILE;
    const int tid = threadIdx.x, lo = tid & 7, hi = tid >> 3;
    const unsigned short* vt = (const unsigned short*)p.b;
    unsigned short* y = (unsigned short*)p.y;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int c = hi + it * 32;                         // lo = 16-byte chunk of the channel's 64 keys
        if (c0 + c < C && k0 + 8 * lo < n) {
            const uint4 v = *(const uint4*)(vt + (size_t)(c0 + c) * ldvt + col0 + k0 + 8 * lo);
            // stored runs (0, 1 | 2, 3) of a 16-group are the logical runs (0, 2 | 1, 3)
            const int s = 4 * (lo >> 1) + (lo & 1);
            tile[c][idr_slot(c, s)] = make_uint2(v.x, v.y);
            tile[c][idr_slot(c, s + 2)] = make_uint2(v.z, v.w);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int r = hi + it * 32;                         // lo = channel octet of the key's 64 channels
        if (k0 + r < n && c0 + 8 * lo < C) {
            unsigned int w[4];
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const int ca = 8 * lo + e, cb = ca + 1;
                const unsigned int a = ((const unsigned short*)&tile[ca][idr_slot(ca, r >> 2)])[r & 3];
                const unsigned int b = ((const unsigned short*)&tile[cb][idr_slot(cb, r >> 2)])[r & 3];
                w[e >> 1] = a | (b << 16);
            }
            *(uint4*)(y + (size_t)(k0 + r) * ldy + c0 + 8 * lo) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// conv_in: a = latents fp32 NCHW [S, 4, H, W]; w = weights T [C0][CIN][3][3]; bias T [C0];
// y = NHWC T [Bout, H, W, C0] with Bout = i4 (batch b reads latent b % S: CFG duplication).
// i0 = S, i1 = H, i2 = W, i3 = C0, f0 = input scale.  Eight threads per pixel, each 8 channels at a time.
// CIN = 9 (the SDXL inpainting UNet, diffusers StableDiffusionXLInpaintPipeline: cat([scaled latents, mask, masked_image_latents], 1)):
// channels 4-8 come from x2, fp32 NCHW [S, 5, H, W], NOT scaled (scale_model_input is applied before the concat) and rounded to T like
// the latents.  The weight tile stays fp32 in LDS, (81 + 1) * C0 * 4 B = 105 KB at C0 = 320 of the 160 KiB a workgroup may have -- one
// workgroup per CU instead of three, so it has 512 threads (two waves per SIMD, 256 VGPRs each: the 81 taps stay in registers); 16-bit weights in LDS would add a conversion per
// multiply-add to the inner loop of a VALU-bound kernel.  The CIN = 4 instantiation is the kernel as it was.
template <typename T, int CIN>
__global__ __launch_bounds__(CIN > 4 ? 512 : 256) void conv_in_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    constexpr int KT = CIN * 9;
    extern __shared__ float wl[];   // [KT][C0] transposed weights, then [C0] bias
    const int S = p.i0, H = p.i1, W = p.i2, C0 = p.i3, Bout = p.i4;
    const T* w = (const T*)p.w;
    for (int co = threadIdx.x; co < C0; co += blockDim.x) {      // one output channel (KT contiguous taps) per thread
#pragma unroll
        for (int k = 0; k < KT; ++k) wl[k * C0 + co] = to_f32(w[co * KT + k]);
    }
    for (int i = threadIdx.x; i < C0; i += blockDim.x) wl[KT * C0 + i] = p.bias ? to_f32(((const T*)p.bias)[i]) : 0.f;
    __syncthreads();
    const int cg = C0 >> 3;
    const float in_scale = p.tab ? p.tab[*p.step] : p.f0;
    // 8 threads per pixel: each fetches the pixel's KT taps once (all loads in flight together; the 8 copies hit
    // L1), then produces the channel octets l8, l8+8, .. -- the 8 threads of a pixel store 128 contiguous bytes
    const long long total = (long long)Bout * H * W * 8;
    const float* lat = (const float*)p.a;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int l8 = (int)(i & 7);
        const long long pix = i >> 3;
        const int x = (int)(pix % W);
        const int y = (int)((pix / W) % H);
        const int b = (int)(pix / ((long long)W * H));
        const float* src = lat + (size_t)(b % S) * 4 * H * W;
        float tap[KT];
#pragma unroll
        for (int ci = 0; ci < 4; ++ci)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int iy = y + ky - 1, ix = x + kx - 1;
                    const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
                    const float v = in ? src[((size_t)ci * H + iy) * W + ix] * in_scale : 0.f;
                    // the model sees the latent rounded to the compute dtype (pipeline casts latents)
                    tap[ci * 9 + ky * 3 + kx] = to_f32(from_f32<T>(v));
                }
        if constexpr (CIN > 4) {
            const float* src2 = p.x2 + (size_t)(b % S) * (CIN - 4) * H * W;
#pragma unroll
            for (int ci = 4; ci < CIN; ++ci)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int iy = y + ky - 1, ix = x + kx - 1;
                        const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
                        const float v = in ? src2[((size_t)(ci - 4) * H + iy) * W + ix] : 0.f;
                        tap[ci * 9 + ky * 3 + kx] = to_f32(from_f32<T>(v));
                    }
        }
        for (int c8 = l8; c8 < cg; c8 += 8) {
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = wl[KT * C0 + c8 * 8 + e];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                const float* wr = wl + k * C0 + c8 * 8;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += tap[k] * wr[e];
            }
            v8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(acc[e]);
            ((v8*)p.y)[pix * cg + c8] = o;
        }
    }
}

// The guided noise prediction of the step kernels below, np_ = the UNet's output NHWC [blocks * S, HW, 4]:
//   i3 = 1: [uncond | cond (| perturbed)],  eps = u + f2 * (c - u)            i3 = 0: [cond (| perturbed)],  eps = c
// PAG (imh.h: i2 = 1, the scale s in f3 -- IMH_EW_CFG_RESCALE: f0): perturbed-attention guidance, diffusers
// PAGMixin._apply_perturbed_attention_guidance -- a further block p, the conditional prediction with identity self-attention maps,
//   eps = (u + f2 * (c - u)) + s * (c - p)      |      eps = c + s * (c - p)
// The two-term part is the expression it always was and the third term is added to its result, so a perturbed block equal to the
// conditional one gives the bits of the launch without it; the PAG = false instantiations are the kernels as they were, instruction
// for instruction.

// BLEND (imh.h IMH_EW_CFG_STEP with `mask`): after the update, the masked blend of diffusers StableDiffusionXLInpaintPipeline.__call__
// (num_channels_unet == 4): latents = (1 - m) * add_noise(z, n, timesteps[i + 1]) + m * latents, with add_noise's pair read from
// blend_tab[*step] ((1, 0) in the last row that runs: the image latents themselves).  Same pass, same launch; a == NULL: the blend alone.
// The plain instantiation is the kernel as it was.
template <typename T, bool BLEND, bool PAG = false>
__global__ void cfg_step_kernel(const EwParams p) {
    const int S = p.i0, HW = p.i1;
    const long long total = (long long)S * HW * 4;
    const T* np_ = (const T*)p.a;
    float* lat = (float*)p.y;
    const float cx = p.tab ? p.tab[*p.step * 2] : p.f0;
    const float ce = p.tab ? p.tab[*p.step * 2 + 1] : p.f1;
    float ba = 0.f, bb = 0.f;
    if constexpr (BLEND) { ba = p.blend_tab[*p.step * 2]; bb = p.blend_tab[*p.step * 2 + 1]; }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const int ch = (int)((i / HW) % 4);
        const int s = (int)(i / ((long long)HW * 4));
        if (!BLEND || np_) {
            float eps;
            if (p.i3) {
                const float u = to_f32(np_[((size_t)s * HW + pix) * 4 + ch]);
                const float c = to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + ch]);
                eps = u + p.f2 * (c - u);
                if constexpr (PAG) eps = eps + p.f3 * (c - to_f32(np_[((size_t)(2 * S + s) * HW + pix) * 4 + ch]));
            } else {
                eps = to_f32(np_[((size_t)s * HW + pix) * 4 + ch]);
                if constexpr (PAG) eps = eps + p.f3 * (eps - to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + ch]));
            }
            if (p.w) eps *= ((const float*)p.w)[s];        // guidance_rescale factor of this sample (EW_CFG_RESCALE)
            if (p.b) ((float*)p.b)[i] = eps;
            lat[i] = cx * lat[i] + ce * eps;
        }
        if constexpr (BLEND) {
            const float m = p.mask[(size_t)(s % p.i4) * HW + pix];
            const float pv = ba * p.x2[i] + bb * p.noise[i];
            lat[i] = (1.0f - m) * pv + m * lat[i];
        }
    }
}

// EW_CFG_MSTEP (imh.h): the general step behind the multistep and ancestral samplers (schedulers.py DPMSolverMultistepScheduler,
// EulerAncestralDiscreteScheduler).  Same CFG combine, rescale factor and optional blend as cfg_step_kernel; the update reads one row of
// a six-column table, (cx, ce, ch, cn, hx, he) = tab[6 * *step ..]:
//   x' = cx * x + ce * eps + ch * h + cn * z,   h' = hx * x + he * eps
// h = p.b, fp32 [S, 4, HW], one history slot (the previous step's data prediction), read then overwritten by the same thread; z = row
// *step of the noise bank p.bias, fp32 [n, S, 4, HW].  Either may be NULL: the term is absent and h is not written.  All fp32; the
// first two terms are written as cfg_step_kernel writes them, so that with ch = cn = 0 and no h / bank the result has the same bits.
// SEEDED (imh.h imh_step_seeded): z is not read from a bank but generated here, a pure function of (seed row of the sample, table row,
// element): one Philox4x32-10 call (imh_philox.h) gives the normals of four consecutive elements of a sample, so the loop runs over quads
// of elements, e = 4 q .. 4 q + 3 of sample s (4 HW is a multiple of 4: a quad never leaves its sample; it may straddle a channel boundary
// when HW % 4 != 0).  The update is the expression of the bank form, term for term, so that fed the same z the bits are the same; a row
// with cn == 0 (every row of a deterministic sampler, the last row of Euler ancestral) generates nothing.  The SEEDED = false
// instantiations are the kernels as they were.
template <typename T, bool BLEND, bool SEEDED = false, bool PAG = false>
__global__ void cfg_mstep_kernel(const EwParams p) {
    const int S = p.i0, HW = p.i1;
    const long long total = (long long)S * HW * 4;
    const T* np_ = (const T*)p.a;
    float* lat = (float*)p.y;
    float* hist = (float*)p.b;
    const int row = *p.step;
    const float* c = p.tab + (size_t)row * 6;
    const float cx = c[0], ce = c[1], ch = c[2], cn = c[3], hx = c[4], he = c[5];
    const float* z = p.bias ? (const float*)p.bias + (size_t)row * (size_t)total : nullptr;
    float ba = 0.f, bb = 0.f;
    if constexpr (BLEND) { ba = p.blend_tab[row * 2]; bb = p.blend_tab[row * 2 + 1]; }
    if constexpr (SEEDED) {
        const bool gen = cn != 0.f;
        const long long quads = (long long)S * HW;
        for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
            const int s = (int)(q / HW);
            PhiloxNormals zn = {{0.f, 0.f, 0.f, 0.f}};
            if (gen) zn = seeded_normals(p.seeds + (size_t)s * 4, (uint32_t)(q - (long long)s * HW), (uint32_t)row, p.noise_stream);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long i = q * 4 + k;
                const int pix = (int)(i % HW);
                const int chn = (int)((i / HW) % 4);
                float eps;
                if (p.i3) {
                    const float u = to_f32(np_[((size_t)s * HW + pix) * 4 + chn]);
                    const float cnd = to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + chn]);
                    eps = u + p.f2 * (cnd - u);
                    if constexpr (PAG) eps = eps + p.f3 * (cnd - to_f32(np_[((size_t)(2 * S + s) * HW + pix) * 4 + chn]));
                } else {
                    eps = to_f32(np_[((size_t)s * HW + pix) * 4 + chn]);
                    if constexpr (PAG) eps = eps + p.f3 * (eps - to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + chn]));
                }
                if (p.w) eps *= ((const float*)p.w)[s];
                const float x = lat[i];
                float y = cx * x + ce * eps;
                if (hist) {
                    y += ch * hist[i];
                    hist[i] = hx * x + he * eps;
                }
                if (gen) y += cn * zn.z[k];
                if constexpr (BLEND) {
                    const float m = p.mask[(size_t)(s % p.i4) * HW + pix];
                    const float pv = ba * p.x2[i] + bb * p.noise[i];
                    y = (1.0f - m) * pv + m * y;
                }
                lat[i] = y;
            }
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int pix = (int)(i % HW);
        const int chn = (int)((i / HW) % 4);
        const int s = (int)(i / ((long long)HW * 4));
        float eps;
        if (p.i3) {
            const float u = to_f32(np_[((size_t)s * HW + pix) * 4 + chn]);
            const float cnd = to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + chn]);
            eps = u + p.f2 * (cnd - u);
            if constexpr (PAG) eps = eps + p.f3 * (cnd - to_f32(np_[((size_t)(2 * S + s) * HW + pix) * 4 + chn]));
        } else {
            eps = to_f32(np_[((size_t)s * HW + pix) * 4 + chn]);
            if constexpr (PAG) eps = eps + p.f3 * (eps - to_f32(np_[((size_t)(S + s) * HW + pix) * 4 + chn]));
        }
        if (p.w) eps *= ((const float*)p.w)[s];            // guidance_rescale factor of this sample (EW_CFG_RESCALE)
        const float x = lat[i];
        float y = cx * x + ce * eps;
        if (hist) {
            y += ch * hist[i];
            hist[i] = hx * x + he * eps;
        }
        if (z) y += cn * z[i];
        if constexpr (BLEND) {
            const float m = p.mask[(size_t)(s % p.i4) * HW + pix];
            const float pv = ba * p.x2[i] + bb * p.noise[i];
            y = (1.0f - m) * pv + m * y;
        }
        lat[i] = y;
    }
}

// imh_randn_seeded: the generator's rows by themselves, y[s, e] = z_{e & 3}(seed row s, quad e >> 2, row, stream) (raw: the uint32 words
// instead), fp32 [S, 4, HW]; one quad per thread and step.  For tests and for callers that want the rows (an oracle comparison).
__global__ void randn_seeded_kernel(const RandnParams p) {
    const int HW = p.HW;
    const uint32_t row = p.step ? (uint32_t)*p.step : p.row;
    const long long quads = (long long)p.S * HW;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
        const int s = (int)(q / HW);
        const uint32_t qs = p.quad0 + (uint32_t)(q - (long long)s * HW);
        if (p.raw) {
            const PhiloxWords w = seeded_words(p.seeds + (size_t)s * 4, qs, row, p.noise_stream);
            uint32_t* y = (uint32_t*)p.y + q * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = w.w[k];
        } else {
            const PhiloxNormals n = seeded_normals(p.seeds + (size_t)s * 4, qs, row, p.noise_stream);
            float* y = (float*)p.y + q * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = n.z[k];
        }
    }
}

// One workgroup per sample: unbiased std over (C, H, W) of the text-conditioned prediction and of the CFG
// combination (torch.std semantics, as diffusers' rescale_noise_cfg), double accumulation, fixed-order tree.
// a = noise prediction NHWC T [2S, HW, 4] ([uncond | cond]); y = fp32 [S]; f2 = guidance scale, f3 = guidance_rescale.
// PAG (i2 = 1, f0 = the PAG scale): a is [3S, HW, 4] ([uncond | cond | perturbed]) and the combination is the three-term one of guided_eps.
template <typename T, bool PAG = false>
__global__ __launch_bounds__(256) void cfg_rescale_kernel(const EwParams p) {
    __shared__ double red[4][256];
    const int S = p.i0, HW = p.i1, s = blockIdx.x;
    const long long n = (long long)HW * 4;
    const T* u = (const T*)p.a + (size_t)s * n;
    const T* c = (const T*)p.a + (size_t)(S + s) * n;
    double st = 0, st2 = 0, sc = 0, sc2 = 0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const float uu = to_f32(u[i]), cc = to_f32(c[i]);
        float g = uu + p.f2 * (cc - uu);
        if constexpr (PAG) g = g + p.f0 * (cc - to_f32(c[(size_t)S * n + i]));
        st += cc; st2 += (double)cc * cc; sc += g; sc2 += (double)g * g;
    }
    red[0][threadIdx.x] = st; red[1][threadIdx.x] = st2; red[2][threadIdx.x] = sc; red[3][threadIdx.x] = sc2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double N = (double)n;
        const double vt = (red[1][0] - red[0][0] * red[0][0] / N) / (N - 1.0);
        const double vc = (red[3][0] - red[2][0] * red[2][0] / N) / (N - 1.0);
        const double ratio = sqrt(fmax(vt, 0.0)) / sqrt(fmax(vc, 1e-300));
        ((float*)p.y)[s] = (float)(p.f3 * ratio + (1.0 - p.f3));
    }
}

// y[r, :] = softmax(f0 * a[r, :]) ; a fp32 [rows, ld_in], y T [rows, ld_out]; one workgroup per row, three passes
// over a row that stays in L2 (<= 64 KB).  i0 rows, i1 cols (multiple of 4), i2 ld_in, i3 ld_out.
template <typename T>
__global__ __launch_bounds__(256) void softmax_rows_kernel(const EwParams p) {
    __shared__ float red[4];
    const int cols = p.i1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* a = (const float*)p.a + (size_t)blockIdx.x * p.i2;
    T* y = (T*)p.y + (size_t)blockIdx.x * p.i3;
    const float c = p.f0 * 1.4426950408889634f;
    float m = -3.0e38f;
    for (int i = threadIdx.x * 4; i < cols; i += 1024) {
        const f32x4 v = *(const f32x4*)(a + i);
        m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    const float mc = m * c;       // f0 > 0: the maximum of the scaled row is the scaled maximum
    float s = 0.f;
    for (int i = threadIdx.x * 4; i < cols; i += 1024) {
        const f32x4 v = *(const f32x4*)(a + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += __builtin_amdgcn_exp2f(v[e] * c - mc);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float inv = 1.0f / ((red[0] + red[1]) + (red[2] + red[3]));
    for (int i = threadIdx.x * 4; i < cols; i += 1024) {
        const f32x4 v = *(const f32x4*)(a + i);
        typename Vec<T>::v4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(__builtin_amdgcn_exp2f(v[e] * c - mc) * inv);
        *(typename Vec<T>::v4*)(y + i) = o;
    }
}

template <typename T>
__global__ void step_row_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    const long long nv = p.n >> 3;
    const v8* src = (const v8*)p.a + (long long)(*p.step) * nv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (long long)gridDim.x * blockDim.x) ((v8*)p.y)[i] = src[i];
}

// EW_GATHER_ROWS: y[r, 0:C] = a[idx[r], 0:C] (+ w[r % P, 0:C]), r < n; a = table T [i5 rows, ld i1], b = idx int32 [n], w = add T [P = i3 rows,
// ld i4] or null, y T [n, ld i2], C = i0 (a multiple of 8: one 16-B chunk per thread and step).  The sum is taken in fp32 and rounded once.
// The host validates the indices before it uploads them; a row whose index is outside [0, i5) all the same is left unwritten -- never read.
template <typename T>
__global__ void gather_rows_kernel(const EwParams p) {
    typedef typename Vec<T>::v8 v8;
    const int cv = p.i0 >> 3;
    const long long total = p.n * cv;
    const int* idx = (const int*)p.b;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / cv;
        const int c = (int)(i - r * cv) * 8;
        const int src = idx[r];
        if ((unsigned)src >= (unsigned)p.i5) continue;
        v8 v = *(const v8*)((const T*)p.a + (size_t)src * p.i1 + c);
        if (p.w) {
            const v8 u = *(const v8*)((const T*)p.w + (size_t)(r % p.i3) * p.i4 + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = from_f32<T>(to_f32(v[e]) + to_f32(u[e]));
        }
        *(v8*)((T*)p.y + (size_t)r * p.i2 + c) = v;
    }
}

__global__ void step_set_kernel(int* step, int value, int set) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step = set ? value : *step + 1;
}

template <typename T>
__global__ void cast_f32_kernel(const EwParams p) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (long long)gridDim.x * blockDim.x)
        ((float*)p.y)[i] = to_f32(((const T*)p.a)[i]);
}

static inline int grid_for(long long work, int threads) {
    long long g = (work + threads - 1) / threads;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// EW_ROW_STATS: y[row] = (sum, M2 about the row mean) of a[row, 0:i0] (row stride i1 elements), ONE slot per row, in the
// format of imh_lnstats.h -- the stand-alone producer of LayerNorm statistics for token rows whose writing GEMM variant
// has no statistics epilogue (odd shapes / tiles).  One wave per row, two passes (the second hits L1).
template <typename T>
__global__ __launch_bounds__(256) void row_stats_kernel(const EwParams p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.n) return;
    const T* x = (const T*)p.a + row * p.i1;
    const int C = p.i0;
    float s = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const typename Vec<T>::v8 t = *(const typename Vec<T>::v8*)(x + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += to_f32(t[e]);
    }
    s = wave_sum(s);
    const float mean = s / (float)C;
    float m2 = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const typename Vec<T>::v8 t = *(const typename Vec<T>::v8*)(x + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = to_f32(t[e]) - mean; m2 = __builtin_fmaf(d, d, m2); }
    }
    m2 = wave_sum(m2);
    if (lane == 0) { float* y = (float*)p.y + row * 2; y[0] = s; y[1] = m2; }
}

template <typename T>
static int ew_typed(int op, const EwParams& p, hipStream_t stream) {
    switch (op) {
        case EW_TIMESTEP:
            if (p.i0 <= 0 || (p.i0 & 1)) { set_error("timestep: dim must be even"); return IMH_ERR_SHAPE; }
            hipLaunchKernelGGL((timestep_kernel<T>), dim3(grid_for(p.n * (p.i0 >> 1), 256)), dim3(256), 0, stream, p);
            break;
        case EW_SILU:
            if (p.n & 7) { set_error("silu: n must be a multiple of 8"); return IMH_ERR_SHAPE; }
            hipLaunchKernelGGL((silu_kernel<T>), dim3(grid_for(p.n >> 3, 256)), dim3(256), 0, stream, p);
            break;
        case EW_ADD:
            if (p.n & 7) { set_error("add: n must be a multiple of 8"); return IMH_ERR_SHAPE; }
            hipLaunchKernelGGL((add_kernel<T>), dim3(grid_for(p.n >> 3, 256)), dim3(256), 0, stream, p);
            break;
        case EW_CONCAT:
            if (p.i5 > 0) {         // the identity-attention form (imh.h): b = Vt [C = i1, ldvt = i5], y[r, c] = Vt[c, col0 + unpermuted r], i3 = ld of y, i4 = col0
                if (p.i0 != 0 || p.i2 != 0) { set_error("concat: the identity-rows form (i5 = ldvt = %d > 0) has an empty first part and no FreeU planes (i0 = %d, i2 = %d)", p.i5, p.i0, p.i2); return IMH_ERR_ARG; }
                if (p.n <= 0 || (p.n & 15) || p.n > 0x7fffffc0LL || p.i4 < 0 || (p.i4 & 15) || p.i1 <= 0 || (p.i1 & 7)) {
                    set_error("concat: identity rows n = %lld, col0 = %d (positive / non-negative multiples of 16), C = %d (a positive multiple of 8)", p.n, p.i4, p.i1); return IMH_ERR_ARG;
                }
                if ((p.i5 & 7) || p.i5 < p.i4 + p.n || (p.i3 & 7) || p.i3 < p.i1) {
                    set_error("concat: identity rows ldvt = %d (a multiple of 8, >= col0 + n = %lld), ld of y = %d (a multiple of 8, >= C = %d)", p.i5, p.i4 + p.n, p.i3, p.i1); return IMH_ERR_ARG;
                }
                if (!p.b || (((uintptr_t)p.b | (uintptr_t)p.y) & 15)) { set_error("concat: identity rows need Vt in b, and b and y 16-byte aligned"); return IMH_ERR_ARG; }
                hipLaunchKernelGGL(identity_rows_kernel, dim3((unsigned)((p.n + IDR_TILE - 1) / IDR_TILE), (unsigned)((p.i1 + IDR_TILE - 1) / IDR_TILE)), dim3(IDR_THREADS), 0, stream, p);
                break;
            }
            if ((p.i0 & 7) || (p.i1 & 7)) { set_error("concat: channel counts must be multiples of 8"); return IMH_ERR_SHAPE; }
            if (p.i2 > 0) {         // the FreeU form (imh.h): i2 = H, i3 = W, i4 = scaled hidden channels, f0 = b, f1 = s
                const long long hw = (long long)p.i2 * p.i3;
                if (p.i0 < 0 || p.i1 < 0 || p.i4 < 0 || p.i4 > p.i0) {
                    set_error("concat: FreeU scales i4 = %d leading channels of the %d hidden ones (0 <= i4 <= i0)", p.i4, p.i0); return IMH_ERR_SHAPE;
                }
                if (p.i2 < 2 || p.i3 < 2 || p.n < 0 || p.n % hw) {
                    set_error("concat: FreeU planes are H = %d x W = %d (both >= 2) and tile the n = %lld pixels", p.i2, p.i3, p.n); return IMH_ERR_SHAPE;
                }
                const size_t lds = freeu_lds_bytes(p.i2, p.i3);
                const int spb = ((p.i1 >> 2) + FREEU_LANES - 1) / FREEU_LANES;
                const long long nslab = p.n / hw * spb;
                if (hw > 0x7fffffffLL || lds > 64 * 1024 || nslab > 0x3fffffffLL) {
                    set_error("concat: FreeU planes of %d x %d over %lld pixels are beyond the launch (H + W <= 3000, H * W < 2^31)", p.i2, p.i3, p.n); return IMH_ERR_SHAPE;
                }
                if ((p.i0 && !p.a) || (p.i1 && !p.b)) { set_error("concat: null source"); return IMH_ERR_ARG; }
                const int ncopy = p.i0 ? std::min(grid_for((p.n * (p.i0 >> 3) + 3) / 4, FREEU_THREADS), 768) : 0;
                hipLaunchKernelGGL((freeu_concat_kernel<T>), dim3(std::max((int)nslab + ncopy, 1)), dim3(FREEU_THREADS), lds, stream, p, std::max(spb, 1), (int)nslab);
                break;
            }
            hipLaunchKernelGGL((concat_kernel<T>), dim3(grid_for(p.n * ((p.i0 + p.i1) >> 3), 256)), dim3(256), 0, stream, p);
            break;
        case EW_CONV_IN: {
            if (p.i3 & 7) { set_error("conv_in: C0 must be a multiple of 8"); return IMH_ERR_SHAPE; }
            const long long work = (long long)p.i4 * p.i1 * p.i2 * 8;
            if (p.i5 == 9) {
                // the 9-channel form (imh.h): (81 + 1) * C0 floats of LDS, above the 64 KB default from C0 = 200 on, within a workgroup's
                // 160 KiB up to C0 = 496; one persistent 512-thread workgroup per CU there, three while three fit
                static DynLdsOnce once;          // (per T: ew_typed is a template)
                const size_t lds = (size_t)(82 * p.i3) * sizeof(float);
                if (!p.x2 || p.i0 <= 0) { set_error("conv_in: 9 input channels need the second source x2 [S, 5, H, W]"); return IMH_ERR_ARG; }
                if (lds > 160 * 1024) { set_error("conv_in: C0 = %d needs %zu bytes of LDS at 9 input channels (160 KiB per workgroup)", p.i3, lds); return IMH_ERR_SHAPE; }
                if (lds > 64 * 1024) once.ensure((const void*)conv_in_kernel<T, 9>, 160 * 1024);
                hipLaunchKernelGGL((conv_in_kernel<T, 9>), dim3(std::min(grid_for(work, 512), lds > 53 * 1024 ? 256 : 768)), dim3(512), lds, stream, p);
                break;
            }
            if (p.i5 != 0 && p.i5 != 4) { set_error("conv_in: %d input channels (4 or 9)", p.i5); return IMH_ERR_ARG; }
            const size_t lds = (size_t)(37 * p.i3) * sizeof(float);
            // persistent workgroups (3 per CU by LDS): the 46 KB weight transpose is paid 768 times, not once per 1024 outputs
            hipLaunchKernelGGL((conv_in_kernel<T, 4>), dim3(std::min(grid_for(work, 256), 768)), dim3(256), lds, stream, p);
            break;
        }
        case EW_CFG_STEP:
            if (p.i2 != 0 && (p.i2 != 1 || !p.a)) { set_error("cfg_step: i2 = %d selects the three-term (PAG) form with 1 and needs the noise prediction", p.i2); return IMH_ERR_ARG; }
            if (p.mask) {
                if (!p.x2 || !p.noise || !p.blend_tab || !p.step || p.i4 < 1) {
                    set_error("cfg_step: the masked blend needs x2 (image latents), noise, blend_tab, step and i4 = mask batch >= 1");
                    return IMH_ERR_ARG;
                }
                if (p.i2) hipLaunchKernelGGL((cfg_step_kernel<T, true, true>), dim3(grid_for((long long)p.i0 * p.i1 * 4, 256)), dim3(256), 0, stream, p);
                else hipLaunchKernelGGL((cfg_step_kernel<T, true>), dim3(grid_for((long long)p.i0 * p.i1 * 4, 256)), dim3(256), 0, stream, p);
                break;
            }
            if (!p.a) { set_error("cfg_step: null noise prediction"); return IMH_ERR_ARG; }
            if (p.i2) hipLaunchKernelGGL((cfg_step_kernel<T, false, true>), dim3(grid_for((long long)p.i0 * p.i1 * 4, 256)), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((cfg_step_kernel<T, false>), dim3(grid_for((long long)p.i0 * p.i1 * 4, 256)), dim3(256), 0, stream, p);
            break;
        case EW_CFG_MSTEP:
            if (!p.a || !p.tab || !p.step || p.i0 <= 0 || p.i1 <= 0) {
                set_error("cfg_mstep: needs the noise prediction, the six-column table, step and S, HW > 0");
                return IMH_ERR_ARG;
            }
            if (p.i2 != 0 && p.i2 != 1) { set_error("cfg_mstep: i2 = %d selects the three-term (PAG) form with 1", p.i2); return IMH_ERR_ARG; }
            {
                const dim3 gq(grid_for((long long)p.i0 * p.i1, 256)), ge(grid_for((long long)p.i0 * p.i1 * 4, 256));
                if (p.mask) {
                    if (!p.x2 || !p.noise || !p.blend_tab || p.i4 < 1) {
                        set_error("cfg_mstep: the masked blend needs x2 (image latents), noise, blend_tab and i4 = mask batch >= 1");
                        return IMH_ERR_ARG;
                    }
                    if (p.i2) {
                        if (p.seeds) hipLaunchKernelGGL((cfg_mstep_kernel<T, true, true, true>), gq, dim3(256), 0, stream, p);
                        else hipLaunchKernelGGL((cfg_mstep_kernel<T, true, false, true>), ge, dim3(256), 0, stream, p);
                    } else if (p.seeds) hipLaunchKernelGGL((cfg_mstep_kernel<T, true, true>), gq, dim3(256), 0, stream, p);
                    else hipLaunchKernelGGL((cfg_mstep_kernel<T, true>), ge, dim3(256), 0, stream, p);
                    break;
                }
                if (p.i2) {
                    if (p.seeds) hipLaunchKernelGGL((cfg_mstep_kernel<T, false, true, true>), gq, dim3(256), 0, stream, p);
                    else hipLaunchKernelGGL((cfg_mstep_kernel<T, false, false, true>), ge, dim3(256), 0, stream, p);
                } else if (p.seeds) hipLaunchKernelGGL((cfg_mstep_kernel<T, false, true>), gq, dim3(256), 0, stream, p);
                else hipLaunchKernelGGL((cfg_mstep_kernel<T, false>), ge, dim3(256), 0, stream, p);
            }
            break;
        case EW_CFG_RESCALE:
            if (p.i0 <= 0 || p.i1 <= 0) { set_error("cfg_rescale: empty problem"); return IMH_ERR_SHAPE; }
            if (p.i2 != 0 && p.i2 != 1) { set_error("cfg_rescale: i2 = %d selects the three-term (PAG) form with 1", p.i2); return IMH_ERR_ARG; }
            if (p.i2) hipLaunchKernelGGL((cfg_rescale_kernel<T, true>), dim3(p.i0), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((cfg_rescale_kernel<T>), dim3(p.i0), dim3(256), 0, stream, p);
            break;
        case EW_SOFTMAX:
            if (p.i0 <= 0 || p.i1 <= 0 || (p.i1 & 3) || (p.i2 & 3) || (p.i3 & 3) || p.f0 <= 0.f) {
                set_error("softmax: rows=%d cols=%d ld=%d/%d (cols and lds must be multiples of 4, scale > 0)", p.i0, p.i1, p.i2, p.i3);
                return IMH_ERR_SHAPE;
            }
            hipLaunchKernelGGL((softmax_rows_kernel<T>), dim3(p.i0), dim3(256), 0, stream, p);
            break;
        case EW_CAST_F32:
            hipLaunchKernelGGL((cast_f32_kernel<T>), dim3(grid_for(p.n, 256)), dim3(256), 0, stream, p);
            break;
        case EW_ROW_STATS:
            if (p.n <= 0 || p.i0 <= 0 || (p.i0 & 7) || (p.i1 & 7) || !p.a) { set_error("row_stats: rows=%lld C=%d ld=%d (C and ld must be multiples of 8)", p.n, p.i0, p.i1); return IMH_ERR_SHAPE; }
            hipLaunchKernelGGL((row_stats_kernel<T>), dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, stream, p);
            break;
        case EW_STEP_ROW:
            if (p.n <= 0 || (p.n & 7) || !p.a || !p.step) { set_error("step_row: n=%lld must be a positive multiple of 8, a and step non-null", p.n); return IMH_ERR_ARG; }
            hipLaunchKernelGGL((step_row_kernel<T>), dim3(grid_for(p.n >> 3, 256)), dim3(256), 0, stream, p);
            break;
        case EW_GATHER_ROWS:
            if (!p.a || !p.b || p.n <= 0 || p.i0 <= 0 || (p.i0 & 7) || p.i1 < p.i0 || (p.i1 & 7) || p.i2 < p.i0 || (p.i2 & 7) || p.i5 <= 0 ||
                (p.w && (p.i3 <= 0 || p.i4 < p.i0 || (p.i4 & 7)))) {
                set_error("gather_rows: n=%lld C=%d ld=%d/%d table rows=%d add rows=%d ld=%d (table, idx non-null; C and the row strides multiples of 8, "
                          "strides >= C; table rows > 0; with add: rows > 0)", p.n, p.i0, p.i1, p.i2, p.i5, p.i3, p.i4);
                return IMH_ERR_SHAPE;
            }
            if ((((uintptr_t)p.a | (uintptr_t)p.y | (uintptr_t)p.w) & 15) || ((uintptr_t)p.b & 3)) {
                set_error("gather_rows: table / add / y must be 16-byte aligned, idx 4-byte aligned"); return IMH_ERR_ARG;
            }
            hipLaunchKernelGGL((gather_rows_kernel<T>), dim3(grid_for(p.n * (p.i0 >> 3), 256)), dim3(256), 0, stream, p);
            break;
        case EW_STEP_SET:
            hipLaunchKernelGGL(step_set_kernel, dim3(1), dim3(64), 0, stream, (int*)p.y, p.i0, p.i1);
            break;
        default:
            set_error("elementwise: unknown op %d", op);
            return IMH_ERR_ARG;
    }
    return check_launch("elementwise");
}

int randn_seeded_launch(const RandnParams& p, hipStream_t stream) {
    hipLaunchKernelGGL(randn_seeded_kernel, dim3(grid_for((long long)p.S * p.HW, 256)), dim3(256), 0, stream, p);
    return check_launch("randn_seeded");
}

int randn_seeded_host(const RandnParams& p) {
    const uint32_t row = p.step ? (uint32_t)*p.step : p.row;
    for (int s = 0; s < p.S; ++s)
        for (int q = 0; q < p.HW; ++q) {
            const size_t o = ((size_t)s * p.HW + q) * 4;
            if (p.raw) {
                const PhiloxWords w = seeded_words(p.seeds + (size_t)s * 4, p.quad0 + (uint32_t)q, row, p.noise_stream);
                for (int k = 0; k < 4; ++k) ((uint32_t*)p.y)[o + k] = w.w[k];
            } else {
                const PhiloxNormals n = seeded_normals(p.seeds + (size_t)s * 4, p.quad0 + (uint32_t)q, row, p.noise_stream);
                for (int k = 0; k < 4; ++k) ((float*)p.y)[o + k] = n.z[k];
            }
        }
    return IMH_OK;
}

int ew_launch(int op, const EwParams& p, int dtype, hipStream_t stream) {
    if (dtype == IMH_DT_BF16) return ew_typed<bf16_t>(op, p, stream);
    if (dtype == IMH_DT_F16) return ew_typed<f16_t>(op, p, stream);
    set_error("elementwise: unknown dtype %d", dtype);
    return IMH_ERR_DTYPE;
}

}  // namespace imh
