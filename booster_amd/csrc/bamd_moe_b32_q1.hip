// bamd_moe_b32_q1.hip — the routed mixture-of-experts decode launches of bamd_moe_b32.h for Q4_1 / Q5_1 experts (Q8_1 activations, the second chain per row)
#include "bamd_moe_b32.h"

int bamd_launch_moe_gate_up_b32_q1(const bamd_moe_args & a, int tiles, hipStream_t s) { return launch_moe_b32_gate_up<BAMD_Q4_1, BAMD_Q5_1>(a, tiles, s); }
int bamd_launch_moe_down_b32_q1(const bamd_moe_args & a, hipStream_t s) { return launch_moe_b32_down<BAMD_Q4_1, BAMD_Q5_1>(a, s); }
