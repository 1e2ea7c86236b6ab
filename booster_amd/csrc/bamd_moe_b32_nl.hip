// bamd_moe_b32_nl.hip — the routed mixture-of-experts decode launches of bamd_moe_b32.h for IQ4_NL experts (Q8_0 activations, two accumulators per lane)
#include "bamd_moe_b32.h"

int bamd_launch_moe_gate_up_b32_nl(const bamd_moe_args & a, int tiles, hipStream_t s) { return launch_moe_b32_gate_up<BAMD_IQ4_NL>(a, tiles, s); }
int bamd_launch_moe_down_b32_nl(const bamd_moe_args & a, hipStream_t s) { return launch_moe_b32_down<BAMD_IQ4_NL>(a, s); }
