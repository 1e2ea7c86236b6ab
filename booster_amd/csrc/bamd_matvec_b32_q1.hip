// bamd_matvec_b32_q1.hip — the mat-vec kernels of bamd_matvec_b32.h for Q4_1 / Q5_1; callers go through bamd_launch_matvec_b32 (bamd_matvec_b32_q0.hip)
#include "bamd_matvec_b32.h"

void bamd_launch_quantize_q81_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) { launch_quantize_q8_test<true>(x, nw, eps, K, norm, out, s); }
int bamd_launch_matvec_b32_q1(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) { return launch_matvec_b32<B32_FAM_Q1>(a, pro, epi, n_cu, s); }
