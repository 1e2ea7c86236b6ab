// bamd_moe_batch_mfma.h — what the grouped matrix-core mat-muls of a mixture-of-experts prompt micro-batch share (bamd_moe_batch_mfma.hip: Q4_K / Q5_K / Q6_K experts;
// bamd_moe_batch_kq_mfma.hip / bamd_moe_batch_xs_mfma.hip: Q3_K / Q2_K / IQ4_XS; bamd_moe_batch_b32_mfma.hip: the 32-weight block types): the kernel arguments, the
// bounded reads of the tile table and the pair lists that moe_group_kernel (bamd_moe_batch.hip) wrote with tt = 64, and, for the K-quant kernels, the gathered
// record offset and the scattered row-of-four store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bamd_device.h"
#include "bamd_mfma_common.h"

enum { MOE_GATE = 0, MOE_UP = 1, MOE_DOWN = 2 };
struct bamd_moe_mma_args {
    const uint8_t * w; size_t wstride;              // expert 0's wave stream, bytes between experts
    const uint8_t * aux; size_t astride, ch_off;    // expert 0's side table, bytes between tables, offset of a table's consumer part (K-quants)
    const uint8_t * blob16;                         // f16 activation records: [T] rows of K = E (gate / up), [T * n_used] rows of K = F (down)
    const int32_t * lists, * tiles;                 // what moe_group_kernel wrote with tt = 64
    float * out; const float * wgt;                 // [npairs][nrows]: h (gate / up) or prod (down); down: w[pair]
    int K, nrows, npairs, n_used, n_expert;
};

// tile `tile` of the table: false = past the table.  Entries bounded as moe_group_mm_kernel bounds them
__device__ __forceinline__ bool moe_tile(const bamd_moe_mma_args & a, uint32_t tile, int & ex, int & first, int & nt) {
    if ((int) tile >= __builtin_amdgcn_readfirstlane(a.tiles[0])) return false;
    const int32_t * te = a.tiles + 4 + 4 * tile;
    ex = __builtin_amdgcn_readfirstlane(te[0]); first = __builtin_amdgcn_readfirstlane(te[1]); nt = __builtin_amdgcn_readfirstlane(te[2]);
    ex = ex < 0 ? 0 : ex; ex = ex < a.n_expert ? ex : a.n_expert - 1;
    nt = nt < 1 ? 1 : nt; nt = nt < 64 ? nt : 64; nt = nt < a.npairs ? nt : a.npairs;
    first = first < 0 ? 0 : first; first = first <= a.npairs - nt ? first : a.npairs - nt;
    return true;
}
// the launch of one grouped mat-mul for a 32-weight block type (bamd_moe_batch_b32_mfma.hip); mode: MOE_GATE / MOE_UP / MOE_DOWN, tile_bound: tiles the table can hold
void bamd_launch_moe_mma_b32(const bamd_moe_mma_args & a, int type, int mode, int tile_bound, hipStream_t s);
// the same for Q3_K / Q2_K (bamd_moe_batch_kq_mfma.hip) and IQ4_XS (bamd_moe_batch_xs_mfma.hip, which the former forwards to), and 1 when the device takes
// their kernels' LDS size (asked by bamd_prefill_mfma_supported)
void bamd_launch_moe_mma_kq(const bamd_moe_mma_args & a, int type, int mode, int tile_bound, hipStream_t s);
void bamd_launch_moe_mma_xs(const bamd_moe_mma_args & a, int mode, int tile_bound, hipStream_t s);
int  bamd_moe_mma_kq_supported(void);
int  bamd_moe_mma_xs_supported(void);
// pair id of slot u of the tile (slots past the count: the last pair again)
__device__ __forceinline__ int moe_pair(const bamd_moe_mma_args & a, int first, int nt, int u) {
    int p = a.lists[first + (u < nt ? u : nt - 1)];
    p = p < 0 ? 0 : p; return p < a.npairs ? p : a.npairs - 1;
}
// x_rec_off of the gathered tile: byte offset into blob16 of record chunk idx (slot idx / 38, its chunk idx % 38)
template <int MODE>
__device__ __forceinline__ uint32_t moe_rec_off(const bamd_moe_mma_args & a, int first, int nt, int idx, size_t b16) {
    const int u = idx / BAMD_B16_Q, q = idx - u * BAMD_B16_Q, p = moe_pair(a, first, nt, u);
    return (uint32_t) ((size_t) (MODE == MOE_DOWN ? p : p / a.n_used) * b16 + (size_t) q * 16);
}
// rows row0 .. row0 + 3 of pair p: 16 consecutive, 16-byte aligned bytes (nrows is a multiple of 256)
template <int MODE>
__device__ __forceinline__ void moe_store(const bamd_moe_mma_args & a, int p, int row0, const float (&val)[4]) {
    float * o = a.out + (size_t) p * a.nrows + row0;
    bamd_f4 y = { val[0], val[1], val[2], val[3] };
    if (MODE == MOE_UP) {
        const bamd_f4 r = *(const bamd_f4 *) o;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = v_silu(r[i]) * val[i];
    }
    if (MODE == MOE_DOWN) {
        const float wp = a.wgt[p];
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = val[i] * wp;
    }
    *(bamd_f4 *) o = y;
}
