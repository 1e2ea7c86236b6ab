// bamd_attention_gs.hip — batched prefill attention on the VALU with its score / probability rows in a global scratch block: what runs beyond the LDS bound
// (two rows of ld floats no longer fit BAMD_ATTN_LDS_MAX: ld > 18432) where the LONG matrix-core kernel (bamd_attention_mfma.hip) does not take the shape.
// A translation unit of its own: the decode step's code objects (bamd_attention.hip, embedded for the own-queue replay) do not change with it.
#include "bamd_attn_batch.h"

// attn_batch_body (bamd_attn_batch.h) — the code attn_batch_kernel (bamd_attention.hip) runs — for sequences whose rows no longer fit BAMD_ATTN_LDS_MAX: the
// fallback of the LONG matrix-core kernel and the only path of the head shapes that kernel declines (head_dim 64 / 192 / 256, GQA ratios 3, 5, 6, 7).  One
// workgroup per (KV head, token) computes ALL GQ query heads of the KV head — no ladder: nothing here is sized by the LDS — so every K row and V^T chunk is
// fetched once for the GQ heads.  Its rows [GQ][ld] sit at workgroup index x GQ x ld floats of a.batch_scratch (AttnRowsGlobal).
// tok0: first token of this launch's slice of the micro-batch (grid.y = tokens of the slice).
template <int GQ>
__global__ void __launch_bounds__(512) attn_batch_gs_kernel(bamd_attn_args a, int tok0) {
    const int ld = a.lds_ld ? a.lds_ld : a.n_ctx;                            // scratch row length
    const int hk = blockIdx.x;
    attn_batch_body<GQ>(a, hk, hk * GQ, tok0 + (int) blockIdx.y, AttnRowsGlobal{a.batch_scratch + ((size_t) blockIdx.y * gridDim.x + blockIdx.x) * GQ * (size_t) ld});
}

// tokens [t0, t0 + Ts) of the micro-batch (after the KV store); a.batch_scratch holds Hkv x Ts x gq x ld floats (bamd_attention_batch_plan)
void bamd_launch_attention_batch_gs(const bamd_attn_args & a, int gq, int t0, int Ts, hipStream_t s) {
    const dim3 grid(a.Hkv, Ts);
    switch (gq) {
#define CASE(G) case G: BAMD_LAUNCH((attn_batch_gs_kernel<G>), grid, dim3(512), 0, s, a, t0); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    }
}
