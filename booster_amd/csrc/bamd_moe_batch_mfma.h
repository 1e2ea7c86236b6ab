// bamd_moe_batch_mfma.h — what the grouped matrix-core mat-muls of a mixture-of-experts prompt micro-batch share (bamd_moe_batch_mfma.hip: Q4_K / Q5_K / Q6_K experts;
// bamd_moe_batch_b32_mfma.hip: the 32-weight block types): the kernel arguments and the bounded reads of the tile table and the pair lists that moe_group_kernel
// (bamd_moe_batch.hip) wrote with tt = 64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
// pair id of slot u of the tile (slots past the count: the last pair again)
__device__ __forceinline__ int moe_pair(const bamd_moe_mma_args & a, int first, int nt, int u) {
    int p = a.lists[first + (u < nt ? u : nt - 1)];
    p = p < 0 ? 0 : p; return p < a.npairs ? p : a.npairs - 1;
}
