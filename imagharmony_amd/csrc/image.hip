// Image ops (include/imh.h imh_clip_preprocess): decoded image [S, 3, H, W] fp32 -> the patch rows of the CLIP vision tower's first GEMM.
//
// One workgroup computes one (image, patch), channel after channel: 3 x patch x patch outputs, the patch's whole row.  It
//   1. builds the tap tables of its `patch` output columns and `patch` output rows in LDS (first tap, count, normalised fp32 weights),
//   2. per channel walks its source window [y0, y1) x [x0, x1) in chunks of RC rows: stages a chunk once (coalesced along x, first clamp applied),
//      filters it horizontally into LDS (RC x patch), and every output thread adds the chunk's rows under its vertical taps in row order
//      -- the sum of an output is taken in tap order whatever RC is,
//   3. clamps, normalises, rounds once and stores.
// At 1024^2 -> 224 a window is ~83 x 83 source pixels and a tap table 14 x 20; upsampling has 4-5 taps.  Every global access is inside
// the image / the row's 3 patch^2 columns by construction AND guarded.  No atomics.
#include <stdint.h>

#include "imh_common.h"
#include "imh_kernels.h"

namespace imh {

namespace {

constexpr float CUBIC_A = -0.5f;

__device__ __forceinline__ float cubic_aa(float x) {
    x = fabsf(x);
    if (x < 1.f) return ((CUBIC_A + 2.f) * x - (CUBIC_A + 3.f)) * x * x + 1.f;
    if (x < 2.f) return (((x - 5.f) * x + 8.f) * x - 4.f) * CUBIC_A;
    return 0.f;
}

struct AxisTaps {
    int first, count;
};

// taps of output index i of an axis resized n_in -> n_out; weights (normalised) to w[0 .. count), count <= cap.
// With scale = n_in / n_out every quantity of the filter is a ratio of integers, and is taken as one: centre = n_in (2 i + 1) / (2 n_out),
// so int(centre -+ support + 0.5) are floor divisions and the argument of tap j, (j - centre + 0.5) / max(scale, 1), is
// ((2 j + 1) n_out - (2 i + 1) n_in) / (2 max(n_in, n_out)) -- one fp32 rounding, where the textbook form in fp32 loses the position of a
// tap near coordinate 1000 to 6e-5 (an ulp of the centre).
__device__ __forceinline__ AxisTaps axis_taps(int n_in, int n_out, int i, float* w, int cap) {
    const long long ni = n_in, no = n_out;
    const long long c2 = ni * (2LL * i + 1);                       // centre * 2 n_out
    const long long s2 = ni >= no ? 4 * ni : 4 * no;               // support * 2 n_out
    const long long a = c2 - s2 + no, b = c2 + s2 + no;            // (centre -+ support + 0.5) * 2 n_out
    long long lo = a <= 0 ? 0 : a / (2 * no);
    long long hi = b <= 0 ? 0 : b / (2 * no);
    hi = hi > ni ? ni : hi;
    int n = (int)(hi - lo);
    n = n > cap ? cap : n;          // (never: cap is the launcher's bound 2 support + 2; keeps the table inside its LDS whatever happens)
    n = n < 0 ? 0 : n;
    const float den = (float)(2 * (ni >= no ? ni : no));
    float total = 0.f;
    for (int j = 0; j < n; ++j) {
        const long long num = (2 * (lo + j) + 1) * no - c2;
        const float v = cubic_aa((float)num / den);
        w[j] = v;
        total += v;
    }
    const float r = total != 0.f ? total : 1.f;
    for (int j = 0; j < n; ++j) w[j] = w[j] / r;
    AxisTaps t;
    t.first = (int)lo;
    t.count = n;
    return t;
}

template <typename T>
__global__ void __launch_bounds__(1024) clip_preprocess_kernel(ClipPreParams p) {
    extern __shared__ float lds[];
    const int P = p.patch, g = p.size / p.patch;
    // LDS: wx [P][ntx] | wy [P][nty] | src [RC][ncols] | hc [RC][P] | taps: xfirst, xcount, yfirst, ycount [P] each
    float* wx = lds;
    float* wy = wx + P * p.ntx;
    float* src = wy + P * p.nty;
    float* hc = src + p.RC * p.ncols;
    int* xfirst = (int*)(hc + p.RC * P);
    int* xcount = xfirst + P;
    int* yfirst = xcount + P;
    int* ycount = yfirst + P;

    const int tid = threadIdx.x, nthr = blockDim.x;
    int b = blockIdx.x;
    const int gx = b % g; b /= g;
    const int gy = b % g;
    const int s = b / g;
    if (s >= p.S) return;

    if (tid < P) {
        const AxisTaps t = axis_taps(p.W, p.nw, p.left + gx * P + tid, wx + tid * p.ntx, p.ntx);
        xfirst[tid] = t.first; xcount[tid] = t.count;
    } else if (tid >= 64 && tid < 64 + P) {      // (a second wave: the two axes' serial tap loops run side by side)
        const int k = tid - 64;
        const AxisTaps t = axis_taps(p.H, p.nh, p.top + gy * P + k, wy + k * p.nty, p.nty);
        yfirst[k] = t.first; ycount[k] = t.count;
    }
    __syncthreads();

    const int x0 = xfirst[0], y0 = yfirst[0];
    int x1 = xfirst[P - 1] + xcount[P - 1], y1 = yfirst[P - 1] + ycount[P - 1];
    x1 = x1 > p.W ? p.W : x1;
    y1 = y1 > p.H ? p.H : y1;
    int ncol = x1 - x0;
    ncol = ncol > p.ncols ? p.ncols : ncol;       // (never: ncols is the launcher's bound of the window)

    const int py = tid / P, px = tid - py * P;
    const bool out_thr = tid < P * P;
    const int yf = out_thr ? yfirst[py] : 0, yn = out_thr ? ycount[py] : 0;

    // the three channels share the tap tables and the window geometry: built once above, used three times
    for (int c = 0; c < 3; ++c) {
    const float* img = p.x + ((size_t)s * 3 + c) * (size_t)p.H * p.W;
    float acc = 0.f;

    for (int r0 = y0; r0 < y1; r0 += p.RC) {
        const int rows = (y1 - r0) < p.RC ? (y1 - r0) : p.RC;
        // stage: a wave takes a row, its lanes consecutive columns
        for (int rr = tid >> 6; rr < rows; rr += nthr >> 6) {
            const float* row = img + (size_t)(r0 + rr) * p.W;
            for (int cc = tid & 63; cc < ncol; cc += 64) {
                const int xs = x0 + cc;
                float v = 0.f;
                if (r0 + rr < p.H && xs < p.W) v = row[xs];
                v = v * 0.5f + 0.5f;
                src[rr * p.ncols + cc] = fminf(fmaxf(v, 0.f), 1.f);
            }
        }
        __syncthreads();
        // horizontal: (row, output column) -> hc
        for (int idx = tid; idx < rows * P; idx += nthr) {
            const int rr = idx / P, ox = idx - rr * P;
            const float* w = wx + ox * p.ntx;
            const float* sp = src + rr * p.ncols + (xfirst[ox] - x0);
            const int n = xcount[ox];
            int lim = ncol - (xfirst[ox] - x0);   // (taps beyond the staged columns cannot occur; the bound keeps the reads inside the chunk)
            lim = n < lim ? n : lim;
            float t = 0.f;
            for (int j = 0; j < lim; ++j) t += sp[j] * w[j];
            hc[idx] = t;
        }
        __syncthreads();
        // vertical: this chunk's rows under the output's taps, in row order
        if (out_thr) {
            int ra = yf > r0 ? yf : r0;
            int rb = yf + yn < r0 + rows ? yf + yn : r0 + rows;
            const float* w = wy + py * p.nty;
            for (int r = ra; r < rb; ++r) acc += hc[(r - r0) * P + px] * w[r - yf];
        }
        __syncthreads();
    }

    if (out_thr) {
        const float mean = c == 0 ? p.mean[0] : c == 1 ? p.mean[1] : p.mean[2];
        const float sd = c == 0 ? p.std[0] : c == 1 ? p.std[1] : p.std[2];
        const float v = (fminf(fmaxf(acc, 0.f), 1.f) - mean) / sd;
        const size_t row = (size_t)s * g * g + (size_t)gy * g + gx;
        const int col = c * P * P + tid;
        if (col < p.ldp) ((T*)p.y)[row * (size_t)p.ldp + col] = (T)v;
    }
    }   // channels (the chunk loop ends on a barrier: the next channel may overwrite src / hc)
}

}  // namespace

// upper bounds of one axis: (columns of the source window of `patch` consecutive outputs, taps of one output)
static void axis_bounds(int n_in, int n_out, int patch, long long* cols, long long* taps) {
    const double scale = (double)n_in / (double)n_out;
    const double support = scale >= 1.0 ? 2.0 * scale : 2.0;
    *cols = (long long)((patch - 1) * scale + 2.0 * support) + 2;
    *taps = (long long)(2.0 * support) + 2;
}

int clip_preprocess_launch(ClipPreParams p, int dtype, hipStream_t stream) {
    const int P = p.patch, g = p.size / p.patch;
    long long ncols, ntx, nrows, nty;
    axis_bounds(p.W, p.nw, P, &ncols, &ntx);
    axis_bounds(p.H, p.nh, P, &nrows, &nty);
    if (ncols > p.W) ncols = p.W;
    if (nrows > p.H) nrows = p.H;
    // chunk rows: the staged chunk takes at most 16 KB (or one row)
    long long RC = 4096 / ncols;
    RC = RC < 1 ? 1 : RC > nrows ? nrows : RC;
    const long long floats = (long long)P * (ntx + nty) + RC * ncols + RC * P + 4 * P;
    if (floats * 4 > 64 * 1024) {
        set_error("clip_preprocess: resizing %d x %d to %d x %d needs %lld bytes of LDS for its tap tables and source window (64 KB at most)",
                  p.H, p.W, p.nh, p.nw, floats * 4);
        return IMH_ERR_SHAPE;
    }
    p.ncols = (int)ncols; p.ntx = (int)ntx; p.nty = (int)nty; p.RC = (int)RC;
    int threads = (P * P + 63) / 64 * 64;
    threads = threads < 256 ? 256 : threads;
    const dim3 grid((unsigned)(p.S * g * g)), block((unsigned)threads);
    const size_t lds = (size_t)floats * 4;
    if (dtype == IMH_DT_BF16) hipLaunchKernelGGL(clip_preprocess_kernel<bf16_t>, grid, block, lds, stream, p);
    else if (dtype == IMH_DT_F16) hipLaunchKernelGGL(clip_preprocess_kernel<f16_t>, grid, block, lds, stream, p);
    else if (dtype == IMH_CLIP_DT_F32) hipLaunchKernelGGL(clip_preprocess_kernel<float>, grid, block, lds, stream, p);
    else { set_error("clip_preprocess: unknown dtype %d", dtype); return IMH_ERR_ARG; }
    return check_launch("clip_preprocess");
}

}  // namespace imh
