// The grouped low-rank merge of include/imh_lora.h: dst = round_T(fp32(base) + U (g * D)) for every adapted weight of a model in ONE launch.
// One workgroup per 128 x 128 tile of an item [N, K]; the grid is the sum of the items' tiles and a workgroup finds its item by a 256-way
// search of a device prefix array.  The rank axis is walked in tiles of 16 through LDS (U transposed to [j][n], D scaled by g on its way in), the
// products run on v_mfma_f32_32x32x2_f32: exact fp32 products, one rounding per accumulate, ascending j -- bitwise an fmaf chain
// (cdna_hip_programming.md 3), so the result does not depend on the tiling.  4 waves x (64 x 64 = 2 x 2 MFMA blocks).
// The two column blocks of a wave are INTERLEAVED: block jb of lane l holds column 2 (l & 31) + jb, so a lane owns two neighbouring
// elements of a weight row and -- where the item's pointers and leading dimensions allow it (4-byte aligned, even) -- reads and writes them
// as one 32-bit access: 32 lanes cover 128 contiguous bytes of a row.  Otherwise element by element.
// Roofline: per tile 32 KB of base read + 32 KB of dst written against 2 * 128 * 128 * R FLOP at the fp32 matrix rate (64 FLOP / clk / SIMD):
// HBM-bound up to R ~ 50, MFMA-bound beyond; the factors are re-read by every tile of a row / column strip and stay in L2.
// Loads past an edge are clamped into the operand (n < N, k < K, j < R: no branch around a load), stores sit behind their bounds test; the
// base tile is requested before the rank loop, so it arrives under the MFMAs.  Measured (tools/lora_time.py, the whole UNet's 722 Linears, 8.8 GB of weight traffic): 6.9 ms at rank 16, 9.9 ms at rank 64
// -- about 1.3 TB/s, a fifth of what the HBM sustains: the kernel is bound by neither of its floors yet, and what does bound it has not been found.
#include "../../include/imh_lora.h"
#include "imh_common.h"

namespace imh {

constexpr int LM_BN = 128, LM_BK = 128, LM_BR = 16, LM_LD = 132;      // +4 floats: the transposing writes of U spread over the banks

static inline int lora_tiles(long long N, long long K) {
    if (N < 1 || K < 1) return 0;
    const long long t = ((N + LM_BN - 1) / LM_BN) * ((K + LM_BK - 1) / LM_BK);
    return t > 0x7fffffffLL ? 0x7fffffff : (int)t;
}

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_kernel(const imh_lora_item* __restrict__ items, const int32_t* __restrict__ tile_start,
                                                         const int n_items) {
    typedef typename Pk2<T>::t T2;
    __shared__ float Us[LM_BR][LM_LD];                                   // [j][n]
    __shared__ __attribute__((aligned(16))) float Ds[LM_BR][LM_LD];      // [j][k], already times g[j]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int hi = lane >> 5, l31 = lane & 31;
    // the item of this workgroup: the last i with tile_start[i] <= blockIdx.x (tile_start[0] = 0, tile_start[n_items] = the grid)
    // A 256-way search, one probe per thread and round: one round up to 256 items, two up to 65536, where a bisection makes ~10 dependent
    // loads.  (Measured at 722 items: the launch takes the same time either way, 6.9 against 6.7 ms at rank 16 -- the search is not what
    // bounds this kernel.)
    __shared__ int cnt[4];
    const int bid = blockIdx.x;
    int lo = 0, up = n_items;                                            // tile_start[lo] <= bid < tile_start[up] throughout
    while (up - lo > 1) {
        const int S = (up - lo + 255) >> 8;
        const int idx = lo + tid * S;
        const bool le = idx < up && tile_start[idx] <= bid;              // monotone in tid, true for tid == 0
        const int c = __builtin_popcountll(__ballot(le));
        if (lane == 0) cnt[wave] = c;
        __syncthreads();
        const int m = cnt[0] + cnt[1] + cnt[2] + cnt[3];                 // probes that are <= bid: the last of them starts the next range
        __syncthreads();
        lo = __builtin_amdgcn_readfirstlane(lo + (m - 1) * S);
        up = min(up, lo + S);
    }
    const imh_lora_item it = items[lo];
    const int N = it.N, K = it.K, R = it.R;
    const int t = bid - tile_start[lo];
    const int tk = (K + LM_BK - 1) / LM_BK;
    const int n0 = (t / tk) * LM_BN, k0 = (t % tk) * LM_BK;             // (a prefix that disagrees with the items gives n0 >= N: all masked)
    // the table's pointers are global memory: said so, the accesses are global_load / global_store instead of flat ones
    typedef const T __attribute__((address_space(1)))* gT;
    typedef const T2 __attribute__((address_space(1)))* gT2;
    typedef const float __attribute__((address_space(1)))* gF;
    const gT base = (gT)it.base;
    const gF gU = (gF)it.U, gD = (gF)it.D, gG = (gF)it.g;
    const bool pk_in = (((uintptr_t)it.base & 3) | (it.ld_base & 1)) == 0 && K >= 2;
    const bool pk_out = (((uintptr_t)it.dst & 3) | (it.ld_dst & 1)) == 0;

    // the base tile, requested first.  D-matrix map of a 32 x 32 block: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
    // No branch around a load: rows and columns past the edge are CLAMPED into the operand (their values are never stored).
    const int kc = k0 + wn * 64 + 2 * l31;                               // this lane's column pair (even)
    const bool ok0 = kc < K, ok1 = kc + 1 < K;
    T bv[2][16][2];
    if (pk_in) {                                                         // (workgroup-uniform)
        const int kp = ok1 ? kc : 0;                                     // a pair that lies inside the row
        const int kl = min(kc, K - 1);                                   // odd K: the lane that owns the last column alone reads it by itself
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = min(n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, N - 1);
                const T2 v = *(gT2)(base + (size_t)n * it.ld_base + kp);
                bv[i][r][0] = v[0]; bv[i][r][1] = v[1];
                if (K & 1) {
                    const T l = base[(size_t)n * it.ld_base + kl];
                    if (!ok1) bv[i][r][0] = l;
                }
            }
    } else {
        const int ka = min(kc, K - 1), kb = min(kc + 1, K - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = min(n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi, N - 1);
                bv[i][r][0] = base[(size_t)n * it.ld_base + ka];
                bv[i][r][1] = base[(size_t)n * it.ld_base + kb];
            }
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][jb][r] = 0.f;

    // loaders.  U: thread -> rank column tid & 15 of tile rows (tid >> 4) + 16 e; D: thread -> column tid & 127 of rank rows (tid >> 7) + 2 e
    const int uj = tid & 15, un = tid >> 4;
    const int dk = tid & 127, dj = tid >> 7;
    for (int j0 = 0; j0 < R; j0 += LM_BR) {
        float uv[8], dv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int n = n0 + un + 16 * e, ju = j0 + uj;                // clamped loads, then the mask (R >= 1 in here)
            const float u = gU[(size_t)min(n, N - 1) * it.ldu + min(ju, R - 1)];
            uv[e] = (n < N && ju < R) ? u : 0.f;
            const int jd = j0 + dj + 2 * e, k = k0 + dk, jc = min(jd, R - 1);
            const float gd = __fmul_rn(gG[jc], gD[(size_t)jc * it.ldd + min(k, K - 1)]);
            dv[e] = (jd < R && k < K) ? gd : 0.f;
        }
        __syncthreads();                                                 // every wave is past its reads of the previous rank tile
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            Us[uj][un + 16 * e] = uv[e];
            Ds[dj + 2 * e][dk] = dv[e];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < LM_BR / 2; ++kk) {                         // ascending j: rank 2 kk (lanes 0-31), then 2 kk + 1 (lanes 32-63)
            float a[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = Us[2 * kk + hi][wm * 64 + i * 32 + l31];      // A[i = lane & 31][k = lane >> 5]
            const float2 b = *(const float2*)&Ds[2 * kk + hi][wn * 64 + 2 * l31];            // B[k = lane >> 5][columns 2 (lane & 31) + jb]
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b.x, acc[i][0], 0, 0, 0);
                acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b.y, acc[i][1], 0, 0, 0);
            }
        }
    }

    // dst = round(base + sum); a zero sum keeps base's bits
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (n >= N) continue;
            T o[2];
#pragma unroll
            for (int jb = 0; jb < 2; ++jb) {
                const float s = acc[i][jb][r];
                o[jb] = s == 0.f ? bv[i][r][jb] : from_f32<T>(__fadd_rn(to_f32(bv[i][r][jb]), s));
            }
            T __attribute__((address_space(1)))* p = (T __attribute__((address_space(1)))*)it.dst + (size_t)n * it.ld_dst + kc;
            if (pk_out && ok1) {
                T2 v;
                v[0] = o[0]; v[1] = o[1];
                *(T2 __attribute__((address_space(1)))*)p = v;
            } else {
                if (ok0) p[0] = o[0];
                if (ok1) p[1] = o[1];
            }
        }
}

static bool overlaps(uintptr_t a, size_t ab, uintptr_t b, size_t bb) { return ab && bb && a < b + bb && b < a + ab; }

static int do_lora_merge(const imh_lora_merge_args* a, hipStream_t s) {
    const char* who = "imh_lora_merge";
    if (!a || !a->items_host || !a->items_dev || !a->tile_start_dev) { set_error("%s: null pointer argument", who); return IMH_ERR_ARG; }
    if (a->dtype != IMH_DT_BF16 && a->dtype != IMH_DT_F16) { set_error("%s: unknown dtype %d", who, a->dtype); return IMH_ERR_DTYPE; }
    if (a->n_items <= 0) { set_error("%s: n_items=%d must be positive", who, a->n_items); return IMH_ERR_SHAPE; }
    const long long lim = 0x7fffffffLL;
    long long tiles = 0;
    for (int i = 0; i < a->n_items; ++i) {
        const imh_lora_item& it = a->items_host[i];
        if (!it.base || !it.dst || (it.R > 0 && (!it.U || !it.D || !it.g))) { set_error("%s: item %d: null pointer", who, i); return IMH_ERR_ARG; }
        if (((uintptr_t)it.base & 1) || ((uintptr_t)it.dst & 1) || ((uintptr_t)it.U & 3) || ((uintptr_t)it.D & 3) || ((uintptr_t)it.g & 3)) {
            set_error("%s: item %d: base / dst must be 2-byte aligned, U / D / g 4-byte aligned", who, i); return IMH_ERR_ARG;
        }
        if (it.N <= 0 || it.K <= 0 || it.R < 0 || it.ld_base < it.K || it.ld_dst < it.K || it.ldu < it.R || it.ldd < it.K) {
            set_error("%s: item %d: N=%d K=%d R=%d ld_base=%d ld_dst=%d ldu=%d ldd=%d (N, K >= 1, R >= 0, ld_base, ld_dst, ldd >= K, ldu >= R)", who, i,
                      it.N, it.K, it.R, it.ld_base, it.ld_dst, it.ldu, it.ldd);
            return IMH_ERR_SHAPE;
        }
        if ((long long)it.N * it.ld_base > lim || (long long)it.N * it.ld_dst > lim || (long long)it.N * it.ldu > lim || (long long)it.R * it.ldd > lim) {
            set_error("%s: item %d: an operand of 2^31 elements or more", who, i); return IMH_ERR_SHAPE;
        }
        const uintptr_t d0 = (uintptr_t)it.dst;
        const size_t db = ((size_t)(it.N - 1) * it.ld_dst + it.K) * 2;
        const size_t bb = ((size_t)(it.N - 1) * it.ld_base + it.K) * 2;
        const size_t ub = it.R ? ((size_t)(it.N - 1) * it.ldu + it.R) * 4 : 0, gb = (size_t)it.R * 4;
        const size_t Db = it.R ? ((size_t)(it.R - 1) * it.ldd + it.K) * 4 : 0;
        if (overlaps(d0, db, (uintptr_t)it.base, bb) || overlaps(d0, db, (uintptr_t)it.U, ub) || overlaps(d0, db, (uintptr_t)it.D, Db) ||
            overlaps(d0, db, (uintptr_t)it.g, gb)) {
            set_error("%s: item %d: dst must not overlap base, U, D or g (no in-place form)", who, i); return IMH_ERR_ARG;
        }
        tiles += lora_tiles(it.N, it.K);
        if (tiles > lim) { set_error("%s: 2^31 tiles or more", who); return IMH_ERR_SHAPE; }
    }
    if (tiles != a->total_tiles) {
        set_error("%s: total_tiles=%d, the items have %lld (imh_lora_merge_tiles per item)", who, a->total_tiles, tiles); return IMH_ERR_SHAPE;
    }
    const dim3 grid((unsigned)tiles), block(256);
    if (a->dtype == IMH_DT_BF16) hipLaunchKernelGGL(lora_merge_kernel<bf16_t>, grid, block, 0, s, a->items_dev, a->tile_start_dev, a->n_items);
    else hipLaunchKernelGGL(lora_merge_kernel<f16_t>, grid, block, 0, s, a->items_dev, a->tile_start_dev, a->n_items);
    return check_launch("lora_merge_kernel");
}

}  // namespace imh

extern "C" {
int imh_lora_merge_tiles(int N, int K) { return imh::lora_tiles(N, K); }
int imh_lora_merge(const imh_lora_merge_args* a, void* stream) { return imh::do_lora_merge(a, (hipStream_t)stream); }
}
