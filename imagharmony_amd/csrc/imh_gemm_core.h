// Shared pieces of the LDS-DMA GEMM / implicit-conv kernels of gemm.hip and gemm_ring.hip: the split-K range, the accumulator clear, the
// fragment-read + MFMA loop over one landed K tile, the fp32 split-K slab store, and the host's launch sequence.  The device functions are
// __forceinline__; a kernel takes one only where its compiled resources (registers, scratch, spills) come out exactly as with the code
// written in place -- which is why the operand staging and the conv gather stay with each kernel.
#pragma once
#include "imh_common.h"
#include "imh_kernels.h"
#include "imh_gemm_epilogue.h"

namespace imh {

// K tiles [kt0, kt1) of split z (empty for the last splits of a short K)
__device__ __forceinline__ void split_k_range(const GemmParams& p, const int z, int& kt0, int& kt1) {
    const int nkt = p.K / GEMM_BK;
    const int per = (nkt + p.splits - 1) / p.splits;
    kt0 = z * per;
    kt1 = min(nkt, kt0 + per);
}

template <int FM, int FN>
__device__ __forceinline__ void acc_zero(f32x4 (&acc)[FM][FN]) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// one landed K tile: both k steps' fragment reads (token fragment i adds 16 rows, weight fragment j adds 4) and FM x FN MFMAs each,
// the weight fragment as the MFMA A operand
template <typename T, int FM, int FN>
__device__ __forceinline__ void mma_ktile(const unsigned char* xs, const unsigned char* ws, const int (&xoff)[2], const int (&woff)[2],
                                          f32x4 (&acc)[FM][FN]) {
    typedef typename Vec<T>::v8 v8;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        v8 xf[FM], wf[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) xf[i] = *(const v8*)(xs + xoff[kk] + i * 16 * GEMM_ROW_BYTES);
#pragma unroll
        for (int j = 0; j < FN; ++j) wf[j] = *(const v8*)(ws + woff[kk] + j * 4 * GEMM_ROW_BYTES);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(wf[j], xf[i], acc[i][j]);
    }
}

// split-K: the lane's NV consecutive fp32 partial sums of row m, columns nb .., into slab z (vector path; ragged right edge by element).
// (gemm.hip only: behind this function the wave-specialised conv kernels and the 256 x 320 ring of gemm_ring.hip allocate registers
// differently, so that file keeps the same store written in place.)
template <int NV>
__device__ __forceinline__ void store_partial(const GemmParams& p, const int z, const int m, const int nb, const float* v) {
    float* o = p.partial + ((size_t)z * p.M + m) * p.N + nb;
    if (nb + NV <= p.N && (p.N & 3) == 0) {
#pragma unroll
        for (int q0 = 0; q0 < NV; q0 += 4) *(f32x4*)(o + q0) = f32x4{v[q0], v[q0 + 1], v[q0 + 2], v[q0 + 3]};
    } else {
#pragma unroll
        for (int q = 0; q < NV; ++q) if (nb + q < p.N) o[q] = v[q];
    }
}

// ---- host: one launch of a GEMM-family kernel KERN over the BM x BN tiles of p (grid y = the K splits): XCD partition, dynamic-LDS
// opt-in (lds_optin: once per kernel and device; the plain tiles without a statistics area stay inside the 64 KB every kernel may have
// and skip it), launch, status
template <auto KERN>
static int launch_gemm(const GemmParams& p, int BM, int BN, int threads, size_t lds, bool lds_optin, const char* name, hipStream_t stream) {
    GemmParams q = p;
    int tiles;
    xcd_partition(q, BM, BN, &tiles);
    static DynLdsOnce once;
    if (lds_optin) once.ensure((const void*)KERN, (int)lds);
    hipLaunchKernelGGL(KERN, dim3(tiles, p.splits, 1), dim3(threads), lds, stream, q);
    return check_launch(name);
}
// ... and of a two-problem kernel: workgroups [0, grid_a) run a on BMa x BNa tiles, the rest b
template <auto KERN>
static int launch_gemm_pair(const GemmParams& a, int BMa, int BNa, const GemmParams& b, int BMb, int BNb, int threads, size_t lds,
                            bool lds_optin, const char* name, hipStream_t stream) {
    GemmParams qa = a, qb = b;
    int ga, gb;
    xcd_partition(qa, BMa, BNa, &ga);
    xcd_partition(qb, BMb, BNb, &gb);
    static DynLdsOnce once;
    if (lds_optin) once.ensure((const void*)KERN, (int)lds);
    hipLaunchKernelGGL(KERN, dim3(ga + gb), dim3(threads), lds, stream, qa, qb, ga);
    return check_launch(name);
}

}  // namespace imh
