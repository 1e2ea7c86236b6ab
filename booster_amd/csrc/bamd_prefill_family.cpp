// bamd_prefill_family.cpp — state of the prompt matrix-core family switches (bamd_prefill_family.h: the table and what is derived from it), their exported
// setters and the sentences of the load-time message.
#include "bamd_prefill_family.h"
#include "bamd_kernels.h"
#include <array>
#include <stdlib.h>

#define BAMD_API extern "C" __attribute__((visibility("default")))
static const bamd_prefill_family_row * const R = bamd_prefill_families;

// the switches, read from the environment at first use (a function-local static: no translation unit's initialisers run before it is ready)
static int * family_state() {
    static std::array<int, BAMD_PF_COUNT> on = [] {
        std::array<int, BAMD_PF_COUNT> v;
        for (int f = 0; f < BAMD_PF_COUNT; ++f) { const char * e = R[f].env ? getenv(R[f].env) : "1"; v[f] = (e && e[0] == '1') ? 1 : 0; }
        return v; }();
    return on.data();
}
int  bamd_prefill_family_on(int f) { return family_state()[f]; }
void bamd_prefill_family_set(int f, int on) { family_state()[f] = on ? 1 : 0; }
uint32_t bamd_prefill_types_on(bool table) {
    const int * on = family_state(); uint32_t m = 0;
    for (int f = 0; f < BAMD_PF_COUNT; ++f) if (on[f] && R[f].table == table) m |= R[f].types;
    return m;
}
bool bamd_prefill_reads_act16(int form) {
    for (int t = 0; t < 32; ++t) if (bamd_prefill_mfma_type(t) && bamd_act_form_of(t) == form) return true;
    return false;
}
BAMD_API void bamd_set_prefill_lowbit(int on) { bamd_prefill_family_set(BAMD_PF_LOWBIT, on); }
BAMD_API void bamd_set_prefill_q0(int on) { bamd_prefill_family_set(BAMD_PF_Q0, on); }
BAMD_API void bamd_set_prefill_q1(int on) { bamd_prefill_family_set(BAMD_PF_Q1, on); }
BAMD_API void bamd_set_prefill_nl(int on) { bamd_prefill_family_set(BAMD_PF_NL, on); }
BAMD_API void bamd_set_prefill_flt(int on) { bamd_prefill_family_set(BAMD_PF_FLT, on); }
BAMD_API void bamd_set_prefill_bf16(int on) { bamd_prefill_family_set(BAMD_PF_BF16, on); }
BAMD_API unsigned long long bamd_prefill_bf16_fallback_tiles(void) { return bamd_bf16_fallback_tiles_all(); }

// Called for a matrix without a side table (bamd_prefill_aux_bytes = 0).  With every switch off the sentences read as they did before the switches existed.  The
// composed ones name the family's switch only where a sibling among the 32-weight block families (Q0 / Q1 / NL) is on — somebody switched one on and not this one;
// the first such sibling in table order is named.  A type whose own family is on comes here only with a shape its kernel does not take (the load refuses those)
#define INT_DOT "side tables are all-or-nothing per model, so every prompt mat-mul runs on the integer-dot kernel (token by token where K > 35840)"
std::string bamd_prefill_reason(int type) {
    if (bamd_is_flt(type))      // (with FLT on, F32 / F16 need no table: only BF16 gets here — and BF16 itself not while its own switch, BAMD_PREFILL_BF16, is on)
        return bamd_prefill_family_on(BAMD_PF_FLT) ? "the model holds a BF16 matrix: these have no matrix-core kernel (BAMD_PREFILL_FLT covers F32 / F16 only), and side tables are all-or-nothing per model, so every prompt mat-mul of the other types runs on the VALU kernels"
                                                   : "the model holds an F32 / F16 / BF16 matrix: these have no matrix-core kernel, and side tables are all-or-nothing per model, so every prompt mat-mul runs on the VALU kernels";
    if (type == BAMD_IQ4_NL) return "the model holds an IQ4_NL matrix: these have no matrix-core kernel (BAMD_PREFILL_Q0 covers Q4_0 / Q5_0 / Q8_0 only), and " INT_DOT "; BAMD_PREFILL_NL, the switch of the IQ4_NL matrix-core kernel, is off";
    if (type == BAMD_IQ4_XS) return "the model holds an IQ4_XS matrix: these have no matrix-core kernel, and " INT_DOT;      // (in no family: no matrix-core kernel is built for the type)
    int own = 0;
    while (own < BAMD_PF_COUNT && !bamd_prefill_type_in(R[own].types, type)) ++own;
    if (own == BAMD_PF_COUNT || !R[own].names || bamd_prefill_family_on(own)) return "a matrix type / shape without a matrix-core kernel";
    const std::string head = std::string("the model holds a ") + R[own].names + " matrix";
    for (int g = BAMD_PF_Q0; g <= BAMD_PF_NL && bamd_is_b32(type); ++g) if (g != own && bamd_prefill_family_on(g))
        return head + " and " + R[own].env + " is off (" + R[g].env + " covers only its " + R[g].names + " matrices" +
               (g != BAMD_PF_NL ? "; a Q4_0 / Q5_0 file made with an importance matrix needs both switches" : "") + "): " INT_DOT;
    return head + ": these have no matrix-core kernel, and " INT_DOT;
}

// tests/test_prefill_family.py: what build_prefill_aux decides for a matrix of `type` under the current switches (no device needed; not part of include/bamd.h)
BAMD_API const char * bamd_prefill_reason_test(int type) {
    static thread_local std::string s;
    s = bamd_prefill_aux_bytes(type, 64, 256) > 0 ? "tables" : bamd_prefill_mfma_type_notable(type) ? "no table needed" : bamd_prefill_reason(type);
    return s.c_str();
}
