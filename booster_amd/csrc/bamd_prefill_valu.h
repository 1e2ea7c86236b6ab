// bamd_prefill_valu.h — the integer-dot batched prompt mat-mul, the part every weight family shares: the ring loop of a segment, the kernel body (tile staging, slot
// walk, segment loop) and the host geometry.  What a family adds is a ROW POLICY per type and a TYPE LIST; the K-quant ones are in bamd_prefill.hip, those of the
// 32-weight block formats in bamd_prefill_b32.h (bamd_b32_device.h stays out of the K-quant unit).  The kernels keep their names and translation units.
//
// A row policy P supplies
//   P::Rec, P::RECB        the wave-stream record of the type and its bytes
//   P::NULL_TAIL           what is requested behind a wave's last chunk: true = the zero-record descriptor (null_rsrc: fetches nothing), false = the row's last
//                          record again with step 0.  Both forms are kept: they differ in what is fetched
//   P::Acc                 the type of an accumulator.  A token has three, a0 a1 a2; a policy uses those it needs and ignores the rest
//   P::Work                the type of a temporary of one step.  A step has three, w0 w1 w2, on the same terms
//   P::zero(a0, a1, a2)    a token's accumulators at the start of a row
//   P::step(R, ci, lane, au, nb, a0, a1, a2, w0, w1, w2)   block ci of the row (record R) times the token's activation image au, into the token's accumulators
//   P::finish(a0, a1, a2)  the row's value for the token
// The storage is declared by valu_segment, as plain arrays in its own body, and only handed to the policy.  That is deliberate (profiles/prefill_valu_unify.txt):
// a float array that stands alone becomes one vector value per array (float acc[4] is a <4 x float> in the optimised IR), the same array as a member of a struct
// does not (pairs of floats: 214 -> 135 VGPRs in matmul_batch_b32_kernel<false, 0, 4>, other instructions in every instance), and temporaries declared inside
// the policy's step gave the instances with a minimum 20 to 76 bytes of scratch.  An array that nobody reads costs nothing.
// A type list maps a segment's run-time type to valu_segment<P, D, EPI, TT> and picks the ring depth D: see BAMD_VALU_MM_KERNEL_BODY.
#pragma once
#include "bamd_device.h"

template <typename P, int D, int EPI, int TT>
__device__ __forceinline__ void valu_segment(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                             float * __restrict__ out, const float * __restrict__ res, int ldo, int t0, int nt,
                                             const unsigned char * acts, size_t bb, int nvalid) {
    constexpr int RECB = P::RECB; static_assert(RECB > 0, "no wave-stream record for this type");     // bamd_record_bytes
    constexpr bool NULL_TAIL = P::NULL_TAIL;
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int NPARTS = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = PAIR ? weight_rsrc(wB) : rsA, rsN = NULL_TAIL ? null_rsrc(wA) : rsA;
    const int rgb = nb * RECB, rg_step = stride * rgb;
    const int chunks = nb / D;
    typename P::Rec ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val[TT];
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool last = !(PAIR && part == 0) && r + 1 >= count;
            bool after_b; int after_off;                         // behind the part's last chunk: matrix B? and the record
            if constexpr (NULL_TAIL) {
                after_b = PAIR && part == 0;
                after_off = (PAIR && part == 0) ? rowoff : rowoff + rg_step;
            } else {
                after_b = (PAIR && part == 0) || (last && part == 1);
                after_off = (PAIR && part == 0) ? rowoff : (last ? rowoff + (nb - 1) * RECB : rowoff + rg_step);
            }
            typename P::Acc a0[TT], a1[TT], a2[TT];
#pragma unroll
            for (int u = 0; u < TT; ++u) P::zero(a0[u], a1[u], a2[u]);
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                bamd_rsrc nrs; int nxt, step;
                if constexpr (NULL_TAIL) {
                    const bool tail = !inrow && last;            // behind the wave's last chunk: the zero-record descriptor
                    nrs = tail ? rsN : (inrow ? part == 1 : after_b) ? rsB : rsA;
                    nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
                    step = RECB;
                } else {                                         // behind the wave's last chunk: the row's last record again, with step 0
                    nrs = (inrow ? part == 1 : after_b) ? rsB : rsA;
                    nxt = inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
                    step = (inrow || !last) ? RECB : 0;
                }
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
#pragma unroll
                    for (int u = 0; u < TT; ++u) {               // tokens beyond nt read the last token's copy and are never stored
                        typename P::Work w0, w1, w2;
                        P::step(ring[s], c * D + s, lane, acts + (size_t) u * bb, nb, a0[u], a1[u], a2[u], w0, w1, w2);
                    }
                    load_rec(ring[s], nrs, nxt + s * step, lane);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < TT; ++u) {
                const float val = P::finish(a0[u], a1[u], a2[u]);
                if (PAIR && part == 0) { gate_val[u] = val; continue; }
                if ((lane & 7) == 0 && row < nvalid && u < nt) {
                    const size_t o = (size_t) (t0 + u) * ldo + row;
                    float y = val;
                    if (PAIR) y = v_silu(gate_val[u]) * val;
                    if (EPI == BAMD_EPI_ADD) y = val + res[o];
                    out[o] = y;
                }
            }
        }
    }
}

// The body of a kernel `template <.., int EPI, int TT> __global__ void __launch_bounds__(512) NAME(bamd_mm_args a)`.
// grid (token tiles, row slots): consecutive workgroups share the weights (L2) and differ in the token tile.  TT tokens per tile: BAMD_TT = 8 while their
// activation images fit the LDS (K <= 17920), 4 beyond (K <= 35840: the 70B ffn_down at K = 28672); every activation form has the stride of the Q8_K blobs.
// A macro, not a function, for the reason bamd_matvec_b32.h gives for its kernel: inlined from a function of its own the same statements read the workgroup size
// the long way and every instance comes out different.  TYPES, the kernel's type list, is a macro too: TYPES(SEG) is the chain of ifs over the segment's type t
// that picks the ring depth D from nb and calls SEG(D, policy).  A list that is a function — handed the segment's arguments, or a lambda of the kernel — loads
// out / res / ldo once in front of the chain, not in the branch of each type, or reaches the kernel's arguments through a reference; both change every instance
#define BAMD_VALU_SEG(D, ...) valu_segment<__VA_ARGS__, D, EPI, TT>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a.ldo, t0, nt, smem, bb, nv)
#define BAMD_VALU_MM_KERNEL_BODY(TYPES) \
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; \
    const int nb = a.K >> 8; \
    const size_t bb = BAMD_BLOB_BYTES(nb); \
    const int t0 = blockIdx.x * TT; \
    const int nt = a.T - t0 < TT ? a.T - t0 : TT; \
    {   /* this tile's activations -> LDS (rows past T: repeat the last token; results discarded) */ \
        const int n16 = (int) (bb / 16); \
        for (int i = threadIdx.x; i < n16 * TT; i += blockDim.x) { \
            const int u = i / n16, k = i - u * n16; \
            const int tu = t0 + (u < nt ? u : nt - 1); \
            ((uint4 *) smem)[(size_t) u * n16 + k] = ((const uint4 *) (a.blob + (size_t) tu * bb))[k]; \
        } \
    } \
    __syncthreads(); \
    const int wave = wave_id(), nwaves = blockDim.x >> 6; \
    const int slot = blockIdx.y + gridDim.y * wave, stride = gridDim.y * nwaves; \
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL; \
    int off = 0; \
    const int nseg = PAIR ? 1 : a.nseg; \
    for (int s = 0; s < nseg; ++s) { \
        const int nrg = a.seg[s].nrows >> 3; \
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride; \
        const int g0 = slot + k0 * stride; \
        const int count = g0 < off + nrg ? (off + nrg - 1 - g0) / stride + 1 : 0; \
        if (count > 0) { \
            const int t = a.seg[s].type; \
            const uint8_t * wA = (const uint8_t *) a.seg[s].w; \
            const uint8_t * wB = PAIR ? (const uint8_t *) a.seg[1].w : wA; \
            const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows; \
            TYPES(BAMD_VALU_SEG); \
        } \
        off += nrg; \
    }

// host: tokens per tile (8 while their activations fit the LDS, else 4), the LDS bytes and the grid of a launch.  false: K > 35840, which would need a K-split
// of the activation tile
struct valu_mm_geom { int tt; size_t lds; dim3 grid; };
static inline bool valu_mm_geometry(const bamd_mm_args & a, int epi, int n_cu, valu_mm_geom & g) {
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3; else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    g.tt = (size_t) BAMD_TT * BAMD_BLOB_BYTES(a.K >> 8) <= 160 * 1024 ? BAMD_TT : 4;
    g.lds = (size_t) g.tt * BAMD_BLOB_BYTES(a.K >> 8);
    if (g.lds > 160 * 1024) return false;
    const int tiles = (a.T + g.tt - 1) / g.tt;
    // row slots: enough workgroups to fill the chip a few times over, at least one row-group per wave
    int gy = (4 * (n_cu > 0 ? n_cu : 256) + tiles - 1) / tiles;
    if (gy * 8 > nrg) gy = (nrg + 7) / 8;
    if (gy < 1) gy = 1;
    g.grid = dim3(tiles, gy);
    return true;
}
