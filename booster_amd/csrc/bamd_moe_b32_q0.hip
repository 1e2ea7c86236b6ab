// bamd_moe_b32_q0.hip — the routed mixture-of-experts decode launches of bamd_moe_b32.h for Q8_0 / Q4_0 / Q5_0 experts; callers go through bamd_launch_moe_gate_up / bamd_launch_moe_down (bamd_moe.hip)
#include "bamd_moe_b32.h"

int bamd_launch_moe_gate_up_b32_q0(const bamd_moe_args & a, int tiles, hipStream_t s) { return launch_moe_b32_gate_up<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0>(a, tiles, s); }
int bamd_launch_moe_down_b32_q0(const bamd_moe_args & a, hipStream_t s) { return launch_moe_b32_down<BAMD_Q8_0, BAMD_Q4_0, BAMD_Q5_0>(a, s); }
