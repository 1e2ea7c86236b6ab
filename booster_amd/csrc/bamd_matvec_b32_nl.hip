// bamd_matvec_b32_nl.hip — the mat-vec kernel of bamd_matvec_b32.h whose type list is Q8_0 / Q4_0 / Q5_0 and IQ4_NL: the launches with at least one IQ4_NL segment.
// A code object of its own, so that the kernels of bamd_matvec_b32_q0.hip / _q1.hip stay what they are; callers go through bamd_launch_matvec_b32 (bamd_matvec_b32_q0.hip)
#define BAMD_B32_MV_KERNEL matvec_b32_nl_kernel
#define BAMD_B32_MV_NL 1
#include "bamd_matvec_b32.h"

int bamd_launch_matvec_b32_nl(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) { return launch_matvec_b32<B32_FAM_NL>(a, pro, epi, n_cu, s); }
