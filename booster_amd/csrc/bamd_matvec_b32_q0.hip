// bamd_matvec_b32_q0.hip — the mat-vec kernels of bamd_matvec_b32.h for Q8_0 / Q4_0 / Q5_0 (split-K among them), and the one entry point of all three type lists
#include "bamd_matvec_b32.h"

void bamd_launch_quantize_q80_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) { launch_quantize_q8_test<false>(x, nw, eps, K, norm, out, s); }
// the family of segment 0 decides; without a minimum, a launch with an IQ4_NL segment anywhere takes the kernel that has the type
int bamd_launch_matvec_b32(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    if (a.nseg > 0 && bamd_is_q1(a.seg[0].type)) return bamd_launch_matvec_b32_q1(a, pro, epi, n_cu, s);
    for (int i = 0; i < a.nseg; ++i) if (a.seg[i].type == BAMD_IQ4_NL) return bamd_launch_matvec_b32_nl(a, pro, epi, n_cu, s);
    return launch_matvec_b32<B32_FAM_Q0>(a, pro, epi, n_cu, s);
}
