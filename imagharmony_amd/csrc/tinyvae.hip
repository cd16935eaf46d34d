// The 3 x 3 conv of diffusers' AutoencoderTiny decoder (include/imh_tinyvae.h imh_tinyvae_conv): 64 channels wide, so the whole packed
// weight (64 x 576 elements, 72 KiB) stays in a CU's LDS while pixel tiles stream past it.
//   GEMM view: D[cout][pixel] = sum_k W[cout][k] * P[k][pixel], k = tap * 64 + cin.  v_mfma_f32_32x32x16: A = the weight (32 couts x 16 k),
//   B = the patch (16 k x 32 pixels of one image row); D has the pixel on the lane (col = lane & 31) and the couts in the 16 registers.
//   The weight rows are stored PERMUTED in LDS so that register i of lane half h is cout 16 h + i of its block of 32: a lane then holds 16
//   consecutive output channels of its pixel, 32 contiguous bytes of the NHWC row, stored as two 16-byte pieces.
//   Workgroup = 8 waves, tile = 16 rows x 32 pixels; wave w owns rows 2 w, 2 w + 1 and all 64 couts: four 32 x 32 accumulators, and per k-step
//   two weight fragments + two patch fragments (ds_read_b128) feed four MFMAs; the reads run one k-step ahead of the MFMAs.
//   LDS: weight rows of 73 16-byte slots (72 + 1 pad), patch pixels of 9 slots (8 + 1 pad): both strides are odd in slots, so the 16 lanes of a
//   ds_read_b128 group (rows / pixels that differ mod 16, one lane half) hit 16 different slots of the 256-byte bank row: conflict-free.
//   74,752 + 88,128 = 162,880 bytes, one workgroup per CU.
//   The patch of the NEXT tile (ten 16-byte loads per lane) and this tile's residual are fetched into registers before this tile's MFMAs;
//   the patch is written to LDS behind them, and the tile's stores leave last, to drain under the next tile's MFMAs.
// HEAD (fp32 NCHW latent, tanh clamp, 4 -> 64) and TAIL (64 -> 3, fp32 NCHW image) are the same kernel: HEAD stages four channels + zeros and
// multiplies the first 16-channel k-step of each tap only, TAIL stages three weight rows + zeros and multiplies one block of 32 couts.
#include "../../include/imh_tinyvae.h"
#include "imh_common.h"

namespace imh {

constexpr int TV_THREADS = 512;
constexpr int TV_TH = 16, TV_TW = 32;                 // output pixels per tile
constexpr int TV_PH = TV_TH + 2, TV_PW = TV_TW + 2;   // the patch with its halo
constexpr int TV_PIX_B = 144;                         // bytes per patch pixel: 64 channels of T + one 16-byte pad slot
constexpr int TV_WROW_B = 1168;                       // bytes per weight row: 576 elements of T + one pad slot
constexpr int TV_W_BYTES = 64 * TV_WROW_B;
constexpr int TV_LDS_BYTES = TV_W_BYTES + TV_PH * TV_PW * TV_PIX_B;
enum { TV_BODY = 0, TV_HEAD = 1, TV_TAIL = 2 };

struct TinyVaeParams {
    const void* x;
    const void* w;
    const void* bias;
    const void* residual;
    void* y;
    int B, H, W, Ho, Wo;
    int tiles_x, tiles_y, ntiles;
    int up2, relu;
};

// LDS weight row r of a block of 32 holds this cout of the block (see the head of the file)
__device__ __forceinline__ int tv_row_cout(int r) { return 16 * ((r >> 2) & 1) + (r & 3) + 4 * (r >> 3); }

// RES: the launch has a residual (body only).  A compile-time switch, and the bias read through a pointer that falls back to a page of
// zeros: a run-time "load or not" around each epilogue load makes hipcc branch around it and wait for every load on its own -- sixteen
// dependent round trips per tile (measured: 140 -> 125 us per 1024^2 launch without them).
template <typename T, int MODE, bool RES>
__global__ __launch_bounds__(TV_THREADS) void tinyvae_conv_kernel(const TinyVaeParams p) {
    typedef typename Vec<T>::v8 v8;
    constexpr int SPP = MODE == TV_HEAD ? 2 : 8;                        // 16-byte slots staged per patch pixel
    constexpr int NITEMS = TV_PH * TV_PW * SPP;
    constexpr int NJ = (NITEMS + TV_THREADS - 1) / TV_THREADS;
    constexpr int KC = MODE == TV_HEAD ? 1 : 4;                         // k-steps of 16 channels per tap
    constexpr int MB = MODE == TV_TAIL ? 1 : 2;                         // blocks of 32 couts
    extern __shared__ __attribute__((aligned(16))) unsigned char tv_lds[];
    unsigned char* const wl = tv_lds;
    unsigned char* const pl = tv_lds + TV_W_BYTES;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const T zero = from_f32<T>(0.f);
    v8 z8;
#pragma unroll
    for (int e = 0; e < 8; ++e) z8[e] = zero;

    // ---- the weight, once per workgroup
    if (MODE == TV_HEAD) {            // [64, 36] -> per (row, tap): slot 0 = four channels + four zeros, slot 1 = zeros
        const T* w = (const T*)p.w;
#pragma unroll
        for (int j = 0; j < (64 * 9 + TV_THREADS - 1) / TV_THREADS; ++j) {
            const int i = tid + j * TV_THREADS;
            if (i >= 64 * 9) break;
            const int row = i / 9, tap = i - row * 9;
            const int cout = (row & 32) + tv_row_cout(row & 31);
            v8 v = z8;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = w[cout * 36 + tap * 4 + c];
            *(v8*)(wl + row * TV_WROW_B + tap * 128) = v;
            *(v8*)(wl + row * TV_WROW_B + tap * 128 + 16) = z8;
        }
    } else {
        const T* w = (const T*)p.w;
        constexpr int NWI = MB * 32 * 72, NWJ = (NWI + TV_THREADS - 1) / TV_THREADS;
        v8 wv[NWJ];
#pragma unroll
        for (int j = 0; j < NWJ; ++j) {           // every load first, then every LDS store: one wait for the lot
            const int i = tid + j * TV_THREADS;
            const int row = i / 72, s = i - row * 72;
            const int cout = (row & 32) + tv_row_cout(row & 31);
            wv[j] = z8;
            if (i < NWI && (MODE != TV_TAIL || cout < 3)) wv[j] = *(const v8*)(w + cout * 576 + s * 8);
        }
#pragma unroll
        for (int j = 0; j < NWJ; ++j) {
            const int i = tid + j * TV_THREADS;
            const int row = i / 72, s = i - row * 72;
            if (i < NWI) *(v8*)(wl + row * TV_WROW_B + s * 16) = wv[j];
        }
    }
    // TAIL: the three biases stay in registers; the other modes read the lane's sixteen per block of 32 couts in the epilogue
    float bt[3] = {0.f, 0.f, 0.f};
    if (MODE == TV_TAIL && p.bias) {
#pragma unroll
        for (int i = 0; i < 3; ++i) bt[i] = to_f32(((const T*)p.bias)[i]);
    }

    const int tiles_per_img = p.tiles_x * p.tiles_y;
    // one staged item = one 16-byte slot of one patch pixel; fetch() reads it from global memory (zeros outside the image)
    auto fetch = [&](int t, v8 (&st)[NJ]) {
        const int b = t / tiles_per_img, tr = t - b * tiles_per_img;
        const int Y0 = (tr / p.tiles_x) * TV_TH, X0 = (tr % p.tiles_x) * TV_TW;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int it = tid + j * TV_THREADS;
            const int pix = it / SPP, s = it - pix * SPP;
            const int py = pix / TV_PW, px = pix - py * TV_PW;
            const int Y = Y0 - 1 + py, X = X0 - 1 + px;                 // the (virtual) input pixel, at the output's resolution
            v8 v = z8;
            if (it < NITEMS && Y >= 0 && Y < p.Ho && X >= 0 && X < p.Wo) {
                if (MODE == TV_HEAD) {
                    if (s == 0) {
                        const float* x = (const float*)p.x;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float u = x[(((size_t)b * 4 + c) * p.H + Y) * p.W + X];
                            v[c] = from_f32<T>(3.0f * tanhf(u / 3.0f));
                        }
                    }
                } else {
                    const int ys = p.up2 ? Y >> 1 : Y, xs = p.up2 ? X >> 1 : X;
                    v = *(const v8*)((const T*)p.x + (((size_t)b * p.H + ys) * p.W + xs) * 64 + s * 8);
                }
            }
            st[j] = v;
        }
    };
    auto stage = [&](const v8 (&st)[NJ]) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int it = tid + j * TV_THREADS;
            const int pix = it / SPP, s = it - pix * SPP;
            if (it < NITEMS) *(v8*)(pl + pix * TV_PIX_B + s * 16) = st[j];
        }
    };

    // The tile loop.  The waves of the one workgroup on a CU move in lock step, so every global access of a tile is put in flight while
    // MFMAs run: the next tile's patch and this tile's residual are fetched into registers in front of the MFMAs, and this tile's stores
    // leave behind the next patch's LDS writes, so they drain under the next tile's MFMAs (the next wait on the memory counter is the
    // counted one in front of the next staging).  Measured against the form that loaded the residual and waited for the stores between
    // tiles: no difference beyond the spread (122 / 126 us at 1024^2) -- the launch is not bound there.
    v8 st[NJ];
    int t = blockIdx.x;
    if (t < p.ntiles) {
        fetch(t, st);
        stage(st);
    }
    __syncthreads();                      // the weight and the first patch are in LDS
    while (t < p.ntiles) {
        const int tn = t + gridDim.x;
        if (tn < p.ntiles) fetch(tn, st);
        // lane = pixel (Y0 + 2 wave + pb, X0 + n), couts mb * 32 + 16 h + i.  A lane outside the image reads the residual of the clamped
        // pixel (inside the operand) and stores nothing: no branch around a load.
        const int b = t / tiles_per_img, tr = t - b * tiles_per_img;
        const int Y0 = (tr / p.tiles_x) * TV_TH, X0 = (tr % p.tiles_x) * TV_TW;
        const int X = X0 + n;
        v8 bv[MB][2], rv[2][MB][2];
        size_t off[2];
        bool ok[2];
        if (MODE != TV_TAIL) {
            const T* const bias = p.bias ? (const T*)p.bias : (const T*)g_zero_page;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int q = 0; q < 2; ++q) bv[mb][q] = *(const v8*)(bias + mb * 32 + 16 * h + 8 * q);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int Y = Y0 + wave * 2 + pb;
                ok[pb] = Y < p.Ho && X < p.Wo;
                off[pb] = (((size_t)b * p.Ho + min(Y, p.Ho - 1)) * p.Wo + min(X, p.Wo - 1)) * 64 + 16 * h;
                if (RES) {
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int q = 0; q < 2; ++q) rv[pb][mb][q] = *(const v8*)((const T*)p.residual + off[pb] + mb * 32 + 8 * q);
                }
            }
        }

        f32x16 acc[MB][2];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[mb][pb][i] = 0.f;
        const unsigned char* const wa = wl + n * TV_WROW_B + h * 16;
        const unsigned char* const pa = pl + ((wave * 2) * TV_PW + n) * TV_PIX_B + h * 16;
        // k-step s = (tap, kc): the fragments of step s + 1 are read from LDS before the MFMAs of step s are issued, the order pinned
        // (hipcc alone sinks each read to the MFMA that uses it; at two waves per SIMD the two forms measured the same)
        constexpr int NS = 9 * KC;
        v8 fa[2][MB], fb[2][2];
        auto frags = [&](const int s, v8 (&a)[MB], v8 (&bq)[2]) {
            const int tap = s / KC, kc = s - tap * KC;
            const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) a[mb] = *(const v8*)(wa + mb * 32 * TV_WROW_B + tap * 128 + kc * 32);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) bq[pb] = *(const v8*)(pa + ((pb + dy) * TV_PW + dx) * TV_PIX_B + kc * 32);
        };
        frags(0, fa[0], fb[0]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s + 1 < NS) frags(s + 1, fa[(s + 1) & 1], fb[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) acc[mb][pb] = mfma32(fa[s & 1][mb], fb[s & 1][pb], acc[mb][pb]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();                  // every wave has read the patch: the next one may overwrite it
        if (tn < p.ntiles) stage(st);

        // ---- epilogue
        if (MODE == TV_TAIL) {
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) {
                const int Y = Y0 + wave * 2 + pb;
                if (h == 0 && Y < p.Ho && X < p.Wo) {
                    float* y = (float*)p.y;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        y[(((size_t)b * 3 + i) * p.Ho + Y) * p.Wo + X] = __fsub_rn(__fmul_rn(2.0f, __fadd_rn(acc[0][pb][i], bt[i])), 1.0f);
                }
            }
        } else {
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        v8 ov;
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float v = __fadd_rn(acc[mb][pb][8 * q + e], to_f32(bv[mb][q][e]));
                            if (RES) v = __fadd_rn(v, to_f32(rv[pb][mb][q][e]));
                            ov[e] = from_f32<T>(p.relu ? fmaxf(v, 0.f) : v);
                        }
                        if (ok[pb]) *(v8*)((T*)p.y + off[pb] + mb * 32 + 8 * q) = ov;
                    }
        }
        __syncthreads();                  // the next patch is in LDS
        t = tn;
    }
}

static bool tv_overlaps(uintptr_t a, size_t ab, uintptr_t b, size_t bb) { return ab && bb && a < b + bb && b < a + ab; }

template <typename T, int MODE, bool RES>
static void tinyvae_launch_r(const TinyVaeParams& p, int grid, hipStream_t s) {
    static DynLdsOnce once;
    once.ensure((const void*)tinyvae_conv_kernel<T, MODE, RES>, TV_LDS_BYTES);
    hipLaunchKernelGGL((tinyvae_conv_kernel<T, MODE, RES>), dim3(grid), dim3(TV_THREADS), TV_LDS_BYTES, s, p);
}
template <typename T, int MODE>
static void tinyvae_launch_t(const TinyVaeParams& p, int grid, hipStream_t s) {
    if constexpr (MODE == TV_BODY) {
        if (p.residual) { tinyvae_launch_r<T, MODE, true>(p, grid, s); return; }
    }
    tinyvae_launch_r<T, MODE, false>(p, grid, s);
}

static int tv_num_cus() {
    static thread_local int cus[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && cus[dev] > 0) return cus[dev];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) { (void)hipGetLastError(); n = 256; }
    if (dev >= 0 && dev < 64) cus[dev] = n;
    return n;
}

static int do_tinyvae_conv(const imh_tinyvae_args* a, hipStream_t s) {
    const char* who = "imh_tinyvae_conv";
    if (!a || !a->x || !a->w || !a->y) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    const int known = IMH_TINYVAE_RELU | IMH_TINYVAE_UP2 | IMH_TINYVAE_HEAD | IMH_TINYVAE_TAIL;
    if (a->flags & ~known) { set_error("%s: unknown flag bits in %d", who, a->flags); return IMH_ERR_ARG; }
    const bool head = a->flags & IMH_TINYVAE_HEAD, tail = a->flags & IMH_TINYVAE_TAIL, up2 = a->flags & IMH_TINYVAE_UP2;
    if (head && tail) { set_error("%s: HEAD and TAIL are exclusive", who); return IMH_ERR_ARG; }
    if ((head || tail) && (up2 || a->residual)) { set_error("%s: HEAD / TAIL take neither UP2 nor a residual", who); return IMH_ERR_ARG; }
    if (tail && (a->flags & IMH_TINYVAE_RELU)) { set_error("%s: TAIL has no ReLU", who); return IMH_ERR_ARG; }
    if (a->dtype != IMH_DT_BF16 && a->dtype != IMH_DT_F16) { set_error("%s: unknown dtype %d", who, a->dtype); return IMH_ERR_DTYPE; }
    const uintptr_t xa = head ? 3 : 15, wa = head ? 1 : 15, ba = tail ? 1 : 15, ya = tail ? 3 : 15;
    if (((uintptr_t)a->x & xa) || ((uintptr_t)a->w & wa) || ((uintptr_t)a->bias & ba) || ((uintptr_t)a->residual & 15) || ((uintptr_t)a->y & ya)) {
        set_error("%s: x, w, bias, residual and y must be 16-byte aligned (HEAD: x to 4, w to 2; TAIL: bias to 2, y to 4)", who); return IMH_ERR_ARG;
    }
    if (a->B <= 0 || a->H <= 0 || a->W <= 0) { set_error("%s: B=%d H=%d W=%d must be positive", who, a->B, a->H, a->W); return IMH_ERR_SHAPE; }
    const long long lim = 0x7fffffffLL;
    const long long Ho = up2 ? 2LL * a->H : a->H, Wo = up2 ? 2LL * a->W : a->W;
    const long long cx = head ? 4 : 64, cy = tail ? 3 : 64;
    long long xe = (long long)a->B * cx, ye = (long long)a->B * cy;
    if (xe > lim || (xe *= a->H) > lim || (xe *= a->W) > lim || ye > lim || (ye *= Ho) > lim || (ye *= Wo) > lim) {
        set_error("%s: B=%d H=%d W=%d: an operand of 2^31 elements or more", who, a->B, a->H, a->W); return IMH_ERR_SHAPE;
    }
    const size_t xb = (size_t)xe * (head ? 4 : 2), yb = (size_t)ye * (tail ? 4 : 2);
    if (tv_overlaps((uintptr_t)a->y, yb, (uintptr_t)a->x, xb) || (a->residual && tv_overlaps((uintptr_t)a->y, yb, (uintptr_t)a->residual, yb))) {
        set_error("%s: y must not overlap x or residual (no in-place form)", who); return IMH_ERR_ARG;
    }
    TinyVaeParams p;
    p.x = a->x; p.w = a->w; p.bias = a->bias; p.residual = a->residual; p.y = a->y;
    p.B = a->B; p.H = a->H; p.W = a->W; p.Ho = (int)Ho; p.Wo = (int)Wo;
    p.tiles_x = (int)((Wo + TV_TW - 1) / TV_TW); p.tiles_y = (int)((Ho + TV_TH - 1) / TV_TH);
    const long long nt = (long long)a->B * p.tiles_x * p.tiles_y;          // < 2^31: every tile holds an output pixel
    p.ntiles = (int)nt;
    p.up2 = up2; p.relu = head || (a->flags & IMH_TINYVAE_RELU);
    const int cus = tv_num_cus();
    const int grid = p.ntiles < cus ? p.ntiles : cus;
    const bool bf = a->dtype == IMH_DT_BF16;
    if (head) { if (bf) tinyvae_launch_t<bf16_t, TV_HEAD>(p, grid, s); else tinyvae_launch_t<f16_t, TV_HEAD>(p, grid, s); }
    else if (tail) { if (bf) tinyvae_launch_t<bf16_t, TV_TAIL>(p, grid, s); else tinyvae_launch_t<f16_t, TV_TAIL>(p, grid, s); }
    else { if (bf) tinyvae_launch_t<bf16_t, TV_BODY>(p, grid, s); else tinyvae_launch_t<f16_t, TV_BODY>(p, grid, s); }
    return check_launch("tinyvae_conv_kernel");
}

}  // namespace imh

extern "C" {
int imh_tinyvae_conv(const imh_tinyvae_args* a, void* stream) { return imh::do_tinyvae_conv(a, (hipStream_t)stream); }
}
