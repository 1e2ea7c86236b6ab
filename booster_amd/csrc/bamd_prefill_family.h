// bamd_prefill_family.h — the ONE description of the weight families with a matrix-core prompt mat-mul (host only; state and sentences: bamd_prefill_family.cpp).
// Switches, routing, the batch quantiser's f16 records and the load-time message are all derived from the table below.
//
// A family is a set of weight types that share a process-wide switch: an environment variable read once (on iff its value begins with '1'; every switch
// defaults to off) and an exported setter, bamd_set_prefill_<family> (include/bamd.h), for tests and tools.  The switches are independent of one another.
//   K       Q4_K / Q5_K (sixteen-wave kernel) and Q6_K (eight-wave kernel), bamd_prefill2.hip: always on
//   LOWBIT  Q3_K / Q2_K: the eight-wave kernel of bamd_prefill2.hip with a policy struct of their own
//   Q0, Q1  Q8_0 / Q4_0 / Q5_0 and Q4_1 / Q5_1: one kernel template, bamd_prefill2_b32.hip
//   NL      IQ4_NL: the Q4_0 record and side table; the same template with two accumulator sets and a 16-token tile
//   FLT     F32 / F16 (bamd_prefill2_flt.hip)
//   BF16    BF16 (bamd_prefill2_bf16.hip): fma chains where exponent ranges prove every product exact, the two-rounding VALU step per workgroup otherwise
// Families WITH A SIDE TABLE are asked three times: when a model builds its tables at load (all or nothing per model: one matrix without a table and every prompt
// mat-mul stays on the integer-dot kernel — llama.cpp writes Q4_0 / Q5_0 files made with an importance matrix with Q4_1 / Q5_1 ffn_down matrices in their first
// layers, so such a file needs BOTH Q0 and Q1), at each launch (a table built earlier is ignored while its family is off) and by the batch quantiser (the f16
// activation records of the 32-weight block kernels are written only while a family reads them).  FLT and BF16 have no table: their kernels read the resident
// weight stream and the f32 / bf16 activation rows as they are, so they are asked at each launch only and apply to models loaded before.
// To add a family: its row here, its kernel's branch in the launcher (bamd_launch_matmul_mfma2 / bamd_batch_mm), its literal sentence in bamd_prefill_reason if the
// composed one does not fit, its exported setter and the Python wrapper of that (booster_amd/__init__.py).
#pragma once
#include <string>
#include "bamd_formats.h"

enum bamd_prefill_family { BAMD_PF_K = 0, BAMD_PF_LOWBIT, BAMD_PF_Q0, BAMD_PF_Q1, BAMD_PF_NL, BAMD_PF_FLT, BAMD_PF_BF16, BAMD_PF_COUNT };
// env: the switch's environment variable (null: always on); types: bit t = bamd_type t belongs to the family (every type is < 32); table: its kernels read a
// load-time side table (bamd_prefill_aux_bytes); names: the types as the load-time message names them (null: the family has no composed sentence)
struct bamd_prefill_family_row { const char * env; uint32_t types; bool table; const char * names; };
static const bamd_prefill_family_row bamd_prefill_families[BAMD_PF_COUNT] = {
    { nullptr,               1u << BAMD_Q4_K | 1u << BAMD_Q5_K | 1u << BAMD_Q6_K, true,  nullptr },
    { "BAMD_PREFILL_LOWBIT", 1u << BAMD_Q3_K | 1u << BAMD_Q2_K,                   true,  "Q2_K / Q3_K" },
    { "BAMD_PREFILL_Q0",     1u << BAMD_Q8_0 | 1u << BAMD_Q4_0 | 1u << BAMD_Q5_0, true,  "Q4_0 / Q5_0 / Q8_0" },
    { "BAMD_PREFILL_Q1",     1u << BAMD_Q4_1 | 1u << BAMD_Q5_1,                   true,  "Q4_1 / Q5_1" },
    { "BAMD_PREFILL_NL",     1u << BAMD_IQ4_NL,                                   true,  "IQ4_NL" },
    { "BAMD_PREFILL_FLT",    1u << BAMD_F32 | 1u << BAMD_F16,                     false, nullptr },
    { "BAMD_PREFILL_BF16",   1u << BAMD_BF16,                                     false, nullptr },
};
int  bamd_prefill_family_on(int f);
void bamd_prefill_family_set(int f, int on);
uint32_t bamd_prefill_types_on(bool table);      // the types of the families that are on now, with (table = true) or without a side table: seven compares per call
static inline bool bamd_prefill_type_in(uint32_t mask, int type) { return type >= 0 && type < 32 && (mask >> type & 1u); }
// "this weight type has a matrix-core prompt mat-mul with a side table now": side-table sizes, the launcher and the engine's routing ask here
static inline bool bamd_prefill_mfma_type(int type) { return bamd_prefill_type_in(bamd_prefill_types_on(true), type); }
// "this weight type has a matrix-core prompt mat-mul WITHOUT a side table now" (F32 / F16 while FLT is on, BF16 while BF16 is on)
static inline bool bamd_prefill_mfma_type_notable(int type) { return bamd_prefill_type_in(bamd_prefill_types_on(false), type); }
// "a family that is on reads the f16 activation records of this activation form" (Q8_0 form: Q0 or NL; Q8_1 form: Q1)
bool bamd_prefill_reads_act16(int form);
// why a matrix of `type` has no side table under the current switches: the sentence of the load-time message (BAMD_PREFILL_VERBOSE=1)
std::string bamd_prefill_reason(int type);
