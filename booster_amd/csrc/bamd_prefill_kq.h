// bamd_prefill_kq.h — the row policy of a K-quant for the integer-dot batched prompt mat-muls: bamd_prefill.hip (dense: valu_segment, bamd_prefill_valu.h) and
// bamd_moe_batch.hip (the grouped, gathered mat-muls of a mixture-of-experts layer).
#pragma once
#include "bamd_device.h"

// the row policy of a K-quant: block_terms / chain_step / finish_row of the decode path over the Q8_K image q8 | S | yd; one accumulator (a pair of chains), no
// temporaries.  Behind a wave's last chunk the row's last record is read again (step 0)
// (the unnamed RowAcc & and kq_none & parameters: valu_segment hands every policy three accumulators and three temporaries, because the storage of the 32-weight
// block types has to be declared there for their kernels to stay what they are, bamd_prefill_valu.h; a K-quant needs one accumulator, the rest is never touched)
struct kq_none {};
template <int TYPE, typename REC> struct KqRow {
    typedef REC Rec;
    typedef RowAcc Acc;
    typedef kq_none Work;
    static constexpr int RECB = BAMD_RECB_OF(TYPE);
    static constexpr bool NULL_TAIL = false;
    static __device__ __forceinline__ void zero(RowAcc & A, RowAcc &, RowAcc &) { A.acc = 0.f; A.accm = 0.f; }
    static __device__ __forceinline__ void step(const REC & R, int ci, int lane, const unsigned char * au, int nb, RowAcc & A, RowAcc &, RowAcc &, kq_none &, kq_none &, kq_none &) {
        const uint32_t * q8 = (const uint32_t *) au; const int * S = (const int *) (q8 + nb * 64); const float * yd = (const float *) (S + nb * 8);
        const Terms T = block_terms(R, ci, lane, q8, S, yd);
        chain_step<TYPE>(A, T.d, T.fs, T.dmin, T.pm);
    }
    static __device__ __forceinline__ float finish(const RowAcc & A, const RowAcc &, const RowAcc &) { return finish_row<TYPE>(A); }
};
