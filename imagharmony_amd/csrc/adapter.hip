// The three passes of the SDXL T2I-Adapter (diffusers T2IAdapter, adapter_type "full_adapter_xl") that are not convs (include/imh_adapter.h
// imh_adapter_op): the pixel-unshuffle of the fp32 control image into the NHWC rows conv_in reads, AdapterResnetBlock's ReLU and the
// down block's AvgPool2d(2, 2, ceil_mode=True).  Once per control image, eagerly; HBM-bound: one lane moves 16 bytes of T along C, so a
// wave's stores (and the loads of relu / avgpool2) are 1 KiB contiguous.  Every global access sits behind its bounds test.
#include "imh_common.h"
#include "imh_kernels.h"

namespace imh {

constexpr int AD_THREADS = 256;

// unshuffle: lane = (pixel (n, y, x) of the output, channel group cg of eight): output channel k = c f^2 + dy f + dx holds
// image[n, c, y f + dy, x f + dx]; k >= Cin f^2 (the padding up to Cp) holds zero.  VEC (f % 8 == 0, 16-byte aligned image, W % 4 == 0): the
// eight channels of a group are eight consecutive floats of one image row -> two 16-byte loads; else element by element.
template <typename T, bool VEC>
__global__ __launch_bounds__(AD_THREADS) void adapter_unshuffle_kernel(const AdapterParams p) {
    typedef typename Vec<T>::v8 v8;
    const long long CG = p.Cp >> 3;
    const int Ho = p.H / p.f, Wo = p.W / p.f;
    const long long total = (long long)p.N * Ho * Wo * CG;
    const long long idx = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % CG);
    const long long pix = idx / CG;
    const int x = (int)(pix % Wo);
    const int y = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((long long)Wo * Ho));
    const int f = p.f, ff = f * f, K = p.C * ff;
    const float* img = (const float*)p.x;
    v8 o;
    const int k0 = cg * 8;
    if (VEC && k0 < K) {           // f % 8 == 0: K % 8 == 0 too, the whole group lies inside one row of one channel
        const int c = k0 / ff, dy = (k0 % ff) / f, dx = k0 % f;
        const float* src = img + (((long long)n * p.C + c) * p.H + (long long)y * f + dy) * p.W + (long long)x * f + dx;
        const f32x4 a = *(const f32x4*)src;
        const f32x4 b = *(const f32x4*)(src + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = from_f32<T>(a[e]); o[4 + e] = from_f32<T>(b[e]); }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            float v = 0.f;
            if (k < K) {
                const int c = k / ff, dy = (k % ff) / f, dx = k % f;
                v = img[(((long long)n * p.C + c) * p.H + (long long)y * f + dy) * p.W + (long long)x * f + dx];
            }
            o[e] = from_f32<T>(v);
        }
    }
    *(v8*)((T*)p.y + pix * p.Cp + k0) = o;
}

// relu: y = max(x, 0) over n elements; lane i takes the i-th group of eight, the lanes i < n % 8 also one element of the tail each
template <typename T>
__global__ __launch_bounds__(AD_THREADS) void adapter_relu_kernel(const AdapterParams p) {
    typedef typename Vec<T>::v8 v8;
    const T* x = (const T*)p.x;
    T* y = (T*)p.y;
    const long long nv = p.n >> 3;
    const long long idx = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (idx < nv) {
        const v8 v = *(const v8*)(x + idx * 8);
        v8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = to_f32(v[e]) > 0.f ? v[e] : from_f32<T>(0.f);
        *(v8*)(y + idx * 8) = o;
    }
    const long long t = nv * 8 + idx;
    if (idx < 8 && t < p.n) {
        const T v = x[t];
        y[t] = to_f32(v) > 0.f ? v : from_f32<T>(0.f);
    }
}

// avgpool2: AvgPool2d(2, 2, ceil_mode=True), no padding: the window of output pixel (oy, ox) is the in-bounds part of rows 2 oy, 2 oy + 1 x
// columns 2 ox, 2 ox + 1; fp32 sum in raster order, times the exact reciprocal of the count (1, 1/2, 1/4), one rounding to T.  The adds and
// the multiply are separate fp32 operations (nothing to contract them with).
template <typename T>
__global__ __launch_bounds__(AD_THREADS) void adapter_avgpool2_kernel(const AdapterParams p) {
    typedef typename Vec<T>::v8 v8;
    const long long CG = p.C >> 3;
    const int Ho = (p.H + 1) >> 1, Wo = (p.W + 1) >> 1;
    const long long total = (long long)p.N * Ho * Wo * CG;
    const long long idx = (long long)blockIdx.x * AD_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % CG);
    const long long pix = idx / CG;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((long long)Wo * Ho));
    const T* x = (const T*)p.x;
    float s[8];
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int iy = 2 * oy + dy, ix = 2 * ox + dx;
            if (iy < p.H && ix < p.W) {
                const v8 v = *(const v8*)(x + (((long long)n * p.H + iy) * p.W + ix) * p.C + cg * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e] = cnt ? __fadd_rn(s[e], to_f32(v[e])) : to_f32(v[e]);
                ++cnt;
            }
        }
    }
    const float r = cnt == 4 ? 0.25f : (cnt == 2 ? 0.5f : 1.f);      // (cnt is 1, 2 or 4: the window loses a whole row and / or a whole column)
    v8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(__fmul_rn(s[e], r));
    *(v8*)((T*)p.y + pix * p.C + cg * 8) = o;
}

template <typename T>
static void adapter_launch_t(const AdapterParams& p, long long lanes, bool vec, hipStream_t stream) {
    const dim3 grid((unsigned)((lanes + AD_THREADS - 1) / AD_THREADS)), block(AD_THREADS);
    if (p.mode == IMH_ADAPTER_UNSHUFFLE) {
        if (vec) hipLaunchKernelGGL((adapter_unshuffle_kernel<T, true>), grid, block, 0, stream, p);
        else hipLaunchKernelGGL((adapter_unshuffle_kernel<T, false>), grid, block, 0, stream, p);
    } else if (p.mode == IMH_ADAPTER_RELU) {
        hipLaunchKernelGGL(adapter_relu_kernel<T>, grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL(adapter_avgpool2_kernel<T>, grid, block, 0, stream, p);
    }
}

// the caller (api.hip do_adapter_op) has validated the pointers and the extents; lanes = 16-byte groups the launch covers
int adapter_launch(const AdapterParams& p, int dtype, hipStream_t stream) {
    long long lanes;
    bool vec = false;
    if (p.mode == IMH_ADAPTER_UNSHUFFLE) {
        lanes = (long long)p.N * (p.H / p.f) * (p.W / p.f) * (p.Cp >> 3);
        vec = p.f % 8 == 0 && p.W % 4 == 0 && ((uintptr_t)p.x & 15) == 0;
    } else if (p.mode == IMH_ADAPTER_RELU) {
        lanes = (p.n >> 3) > 8 ? (p.n >> 3) : 8;        // (the tail's lanes are the first eight)
    } else {
        lanes = (long long)p.N * ((p.H + 1) >> 1) * ((p.W + 1) >> 1) * (p.C >> 3);
    }
    if (dtype == IMH_DT_BF16) adapter_launch_t<bf16_t>(p, lanes, vec, stream);
    else adapter_launch_t<f16_t>(p, lanes, vec, stream);
    return check_launch("adapter_op");
}

}  // namespace imh
