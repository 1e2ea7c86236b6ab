// bamd_prefill_b32_nl.hip — the batched prompt mat-mul kernel of bamd_prefill_b32.h whose type list is Q8_0 / Q4_0 / Q5_0 and IQ4_NL: the launches with at least one
// IQ4_NL segment (two chains per (row, token) for those segments); callers go through bamd_launch_matmul_batch_b32 (bamd_prefill_b32.hip)
#define BAMD_B32_MM_KERNEL matmul_batch_b32_nl_kernel
#define BAMD_B32_MM_NL 1
#include "bamd_prefill_b32.h"

int bamd_launch_matmul_batch_b32_nl(const bamd_mm_args & a, int epi, int n_cu, hipStream_t s) { return launch_matmul_batch_b32<>(a, epi, n_cu, s); }
