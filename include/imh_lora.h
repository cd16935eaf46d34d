/* imh_lora.h -- the two entries of libimh_hip.so that LoRA adds (csrc/lora.hip).  A companion of include/imh.h, which it includes for the
 * status codes and imh_dtype; conventions (pointers, streams, errors) as stated there. */
#ifndef IMH_LORA_H_
#define IMH_LORA_H_

#include "imh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- grouped low-rank merge: every adapted weight of a model in ONE launch ----------------------------------------------------------
 * Per item (one adapted Linear or conv weight, flattened to [N, K] in the master layout's own order):
 *   dst[n, k] = round_T( fp32(base[n, k]) + sum_{j < R} U[n, j] * (g[j] * D[j, k]) )          n < N, k < K
 * base is the pristine snapshot of the weight, dst the live weight (T = bf16 / fp16, dtype); U [N, R] holds the `up` factors of every
 * adapter that touches the weight, concatenated along the rank, D [R, K] the `down` factors stacked the same way, g [R] the strength
 * adapter_weight * alpha / rank of the adapter that owns column j (0: an inactive adapter).  U, D and g are fp32: an fp16, bf16 or fp32 LoRA
 * file loses nothing.  A conv weight [Cout, Cin, k, k] with a LoCon pair (down [r, Cin, k, k], up [Cout, r, 1, 1]) is the same item with
 * K = Cin * k * k.  Additive like imh_adapter_op: entries and structs of their own in this companion header; include/imh.h, every struct,
 * enum and existing entry stay as they were and the ABI stays at 13.  Not a plan kind: the merge runs eagerly, between denoises.
 * Arithmetic: gd = g[j] * D[j, k] is one fp32 multiply; the products U[n, j] * gd are exact and accumulated in fp32 in ascending j from 0
 *   (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain); the sum is added to fp32(base) and rounded once to T (nearest even).  Where the sum is
 *   zero -- R == 0, g == 0 -- dst gets base's bits (a -0 stays -0).  No atomics, no split over j: the same bits on every call.
 * Kernel form: one workgroup per 128 x 128 tile of an item; the grid is the sum of the items' tiles, imh_lora_merge_tiles(N, K) each,
 *   and a workgroup finds its item by a 256-way search of tile_start_dev (one probe per thread and round).  Edge
 *   tiles clamp their loads into the operand and mask their stores element by element.
 * The item table and the prefix live in device memory (the caller uploads them); the entry validates items_host, which must hold the same
 *   values as items_dev, and launches with items_dev.  tile_start_dev: int32 [n_items + 1], entry i = the sum of imh_lora_merge_tiles over
 *   the items before i (entry n_items = total_tiles).  The entry enqueues on `stream` and allocates nothing.
 * Refused without a launch: null args / items_host / items_dev / tile_start_dev, an item's null base / dst (or U / D / g with R > 0), base or
 *   dst not 2-byte aligned, U / D / g not 4-byte aligned, dst overlapping the item's base, U, D or g (IMH_ERR_ARG); n_items <= 0, N <= 0,
 *   K <= 0, R < 0, ld_base < K, ld_dst < K, ldu < R, ldd < K, an operand of 2^31 elements or more (N * ld, R * ldd), a tile total of 2^31 or
 *   more or other than total_tiles (IMH_ERR_SHAPE); another dtype (IMH_ERR_DTYPE).  The dst ranges of different items must not overlap
 *   each other (not checked).
 * Memory: reads rows [0, N) x columns [0, K) of base, rows [0, N) x columns [0, R) of U, rows [0, R) x columns [0, K) of D, g[0 .. R), the
 *   n_items entries of items_dev and the n_items + 1 of tile_start_dev; writes rows [0, N) x columns [0, K) of dst.  The gaps
 *   [K, ld_dst) are not touched.  Nothing else. */
typedef struct imh_lora_item {
    const void* base;        /* T [N, ld_base]: the snapshot */
    void* dst;               /* T [N, ld_dst]: the live weight */
    const float* U;          /* fp32 [N, ldu] */
    const float* D;          /* fp32 [R, ldd] */
    const float* g;          /* fp32 [R] */
    int32_t N, K, R;
    int32_t ld_base, ld_dst, ldu, ldd;
    int32_t pad;
} imh_lora_item;
typedef struct imh_lora_merge_args {
    const imh_lora_item* items_host;
    const imh_lora_item* items_dev;
    const int32_t* tile_start_dev;
    int32_t n_items;
    int32_t total_tiles;
    int32_t dtype;
} imh_lora_merge_args;
int imh_lora_merge_tiles(int N, int K);      /* workgroups of an [N, K] item (0 unless N, K >= 1) */
int imh_lora_merge(const imh_lora_merge_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IMH_LORA_H_ */
