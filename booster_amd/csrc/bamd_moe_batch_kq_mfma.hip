// bamd_moe_batch_kq_mfma.hip — the grouped, gathered expert mat-muls of a mixture-of-experts prompt micro-batch on the matrix cores for Q3_K, Q2_K and IQ4_XS experts:
// launches 4 (gate, then up) and 6 (down) of bamd_moe_batch.hip.  Taken while BAMD_PREFILL_MOE is on AND the type's own family switch (BAMD_PREFILL_LOWBIT for
// Q3_K / Q2_K, BAMD_PREFILL_XS for IQ4_XS) is on; all default off (bamd_prefill_family.h).  The kernel, moe_mfma2_kernel<MODE, F> (bamd_moe_batch_kq_mfma.h), joins
// two things that existed: the dense eight-wave body under its policies X2LowBit<false> (Q3_K), X2LowBit<true> (Q2_K) and X2IQ4XS, and the grouping of
// moe_mfma2_q6k_kernel (bamd_moe_batch_mfma.hip): tile table with tt = 64, pair lists, gathered staging, scattered epilogues, per-tensor routing on the host.  Nine
// instances; the six low-bit ones here, the three IQ4_XS ones in bamd_moe_batch_xs_mfma.hip, which is built without packed-f32 instructions as the dense IQ4_XS
// file is (booster_amd/build.py).
//
// Arithmetic: the dense body's (matmul_mfma2_kernel, bamd_prefill2_body.h), instruction for instruction per (row, pair): the half step, NFRAG
// v_mfma_f32_16x16x32_f16 chained through the accumulator (one for Q3_K / Q2_K, two for IQ4_XS's split scale), the chain one iteration behind (LATE_CHAIN, all
// three policies), X2Hdr<MINS> with Q2_K's min term in front of the dot term into the same accumulator, x_hsum8.  Per (row, pair) the bits are those of the grouped
// integer-dot kernel (moe_group_mm_kernel), of the routed decode launches and of llm_build_moe_ffn.
//
// Grouping: moe_tile / moe_pair / moe_rec_off<MODE> / moe_store<MODE> (bamd_moe_batch_mfma.h), XStage with gathered record sources, weights from w + expert x
// wstride, the side table from aux + expert x astride with its consumer part at ch_off.  Grid (npairs / 64 + n_expert, nrows / 64); a workgroup past tiles[0]
// exits before its first barrier; every table and list entry is bounded again where it becomes an address.
//
// Where it differs from the Q6_K grouped kernel, and what was decided:
//   * Clamps at the end of K.  The Q3_K / Q2_K / IQ4_XS side tables carry no slack (x_slack = 0) and an expert's table is followed by the next expert's, the last
//     one's by nothing: the clamps of the dense body on load_set (the last half steps load the last super-block again, into registers nobody builds from) and on
//     stage (the last super-block is staged once more into the block nobody reads again) are kept as they are.  The prologue's load_set<1>(1) is half step 1 of
//     super-block 0: in range for K = 256.
//   * IQ4_XS's weight sets.  load_set<0> copies set 0 to set 1 and fetches one 16-byte piece per super-block, load_set<1> fetches nothing, PH_SB is one set for
//     both half steps — all inside the policy, which the kernel calls exactly as the dense body does (same order, same clamped arguments), so the copy carries
//     across super-blocks as there.
//   * Q2_K's bsum16.  The dot of the mins reads bytes 576..607 of the GATHERED record in LDS: chunks 36 and 37 of the 38 that the stage copies per slot, so they
//     are covered.  For MOE_DOWN the records are the rows of h that launch 5 writes: bamd_launch_quantize_batch in the Q8_K form writes the f16 records with the
//     bsum16 field for every K-quant alike (quantize_batch_kernel), whatever the down type.  The llama.cpp recipes never put Q2_K into ffn_down; the op test does.
//   * Dead slot tiles.  A wave owns slot tiles 2 tp and 2 tp + 1, sixteen pairs each; a short prompt gives tiles of 1 to 3 pairs, where seven of eight slot tiles
//     hold no pair.  A wave skips the B operand reads, the MFMAs and the chain of a slot tile whose first slot is at or past nt (and, with no live tile, the A
//     fragment and header reads).  The condition is wave-uniform (nt and tp are scalars) and picks one of three compile-time copies of the K loop, so the copy with
//     both tiles live is the dense half step without a branch in it.  The wave keeps every duty it has for others: staging, weight loads, fragment building, and
//     EVERY barrier — each copy holds the same barriers.  The result is unchanged: those slots are never stored.
//   * Policies.  X2LowBit and X2IQ4XS moved to bamd_prefill2_lowbit.h / bamd_prefill2_xs.h; the dense kernels keep their code objects
//     (profiles/moe_kq_mfma_codeobj.txt, which also has registers, LDS and scratch — none — of the nine instances).
#include "bamd_prefill2_lowbit.h"
#include "bamd_moe_batch_kq_mfma.h"
#include "bamd_kernels.h"

void bamd_launch_moe_mma_kq(const bamd_moe_mma_args & a, int type, int mode, int tile_bound, hipStream_t s) {
    if (type == BAMD_IQ4_XS)    bamd_launch_moe_mma_xs(a, mode, tile_bound, s);
    else if (type == BAMD_Q2_K) moe_mfma2_launch<X2LowBit<true>>(a, mode, tile_bound, s);
    else                        moe_mfma2_launch<X2LowBit<false>>(a, mode, tile_bound, s);
}
int bamd_moe_mma_kq_supported(void) { return moe_mfma2_supported<X2LowBit<false>>() && moe_mfma2_supported<X2LowBit<true>>() && bamd_moe_mma_xs_supported(); }
