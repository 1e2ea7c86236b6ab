// bamd_matvec_b32_q0.hip — the mat-vec kernels of bamd_matvec_b32.h for Q8_0 / Q4_0 / Q5_0 (split-K among them), and the one entry point of both families
#include "bamd_matvec_b32.h"

void bamd_launch_quantize_q80_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) { launch_quantize_q8_test<false>(x, nw, eps, K, norm, out, s); }
// the family of segment 0 decides
int bamd_launch_matvec_b32(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    return a.nseg > 0 && bamd_is_q1(a.seg[0].type) ? bamd_launch_matvec_b32_q1(a, pro, epi, n_cu, s) : launch_matvec_b32<false>(a, pro, epi, n_cu, s);
}
