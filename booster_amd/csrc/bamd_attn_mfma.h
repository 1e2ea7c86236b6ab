// bamd_attn_mfma.h — what the matrix-core batched-attention kernels share (bamd_attention_mfma.hip: head_dim 128, gq 1 / 2 / 4 / 8 / 16;
// bamd_attention_mfma_ext.hip: head_dim 64 and the ratios 3 / 5 / 6 / 7): the workgroup shape, the LDS map of the score rows, the scratch block's order.
#pragma once
#include "bamd_device.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));
#define BAMD_AM_NW 4                           /* waves per workgroup: FOUR, at <= 256 VGPRs and <= 56 KB of LDS, so that TWO workgroups share a CU — one workgroup is a chain of
                                                  dependent phases (q / K requests, scores, softmax, V requests, P.V: ~19 us of latency even for a short sequence, measured
                                                  phase by phase), and only a second resident workgroup fills the matrix pipe while the first one waits */
#define BAMD_AM_VROW 144                       /* bytes per staged V^T row (64 positions x f16 = 128 B, padded: 36 dwords -> 16 rows on 16 distinct banks) */
#define BAMD_AM_RBYTES 1024                    /* column maxima per wave + 1 / sum per column */
#define BAMD_AM_MAXPOS 512                     /* positions whose score rows stay in LDS (64 B each: 32 KB); beyond: global scratch + chunks (LONG) */
#define BAMD_AM_CHUNK 512                      /* LONG: positions staged through LDS at a time in the P.V pass */

// score / probability storage [position][column] in LDS, laid out for the three access patterns (64 banks of 4 bytes):
//   row(p) = the positions of a group of 32 reordered as [p & 7][(p >> 3) & 3]: the four positions p, p + 8, p + 16, p + 24 that the four k-groups of a
//            P.V MFMA read together sit in rows with different (row & 3) = different quarters of the banks;
//   column n of a row is stored at n ^ ((row >> 2) & 15): consecutive positions of one column (the softmax pass) hit distinct banks.
__device__ __forceinline__ int am_sidx(int p, int n) {
    const int row = (p & ~31) | ((p & 7) << 2) | ((p >> 3) & 3);
    return row * 16 + (n ^ ((row >> 2) & 15));
}
// LONG: the scratch block of a workgroup holds its 16 score rows as [position / 4][column][4]: the four consecutive positions a lane of pass 1 produces for
// its column are one 16-byte store, and the 16 columns of a position quad are 256 contiguous bytes
__device__ __forceinline__ size_t am_gidx(int p, int n) { return ((size_t) (p >> 2) * 16 + n) * 4 + (p & 3); }
__device__ __forceinline__ float h2f_lo(uint32_t w) { return __half2float(__ushort_as_half((unsigned short) (w & 0xffffu))); }
__device__ __forceinline__ float h2f_hi(uint32_t w) { return __half2float(__ushort_as_half((unsigned short) (w >> 16))); }
