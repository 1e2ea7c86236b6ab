// bamd_formats.h — GGUF K-quant block formats (as they sit in the file) and the MI355X "wave-stream"
// layout they are repacked into at load time.
//
// File formats follow the reference's block definitions (cpp/ggml/src/ggml-common.h:267-316):
//   Q4_K 144 B = {f16 d, f16 dmin, u8 scales[12], u8 qs[128]}
//   Q5_K 176 B = {f16 d, f16 dmin, u8 scales[12], u8 qh[32], u8 qs[128]}
//   Q6_K 210 B = {u8 ql[128], u8 qh[64], i8 scales[16], f16 d}
//   Q2_K  84 B = {u8 scales[16] (low nibble scale, high nibble min), u8 qs[64], f16 d, f16 dmin}      (ggml-common.h:234-261)
//   Q3_K 110 B = {u8 hmask[32], u8 qs[64], u8 scales[12], f16 d}
//   Q8_K 292 B = {f32 d, i8 qs[256], i16 bsums[16]}   (activations only; never stored in HBM here)
// and the 32-weight block formats (ggml-common.h:140-190), whose activations are Q8_0 blocks themselves:
//   Q4_0  18 B = {f16 d, u8 qs[16]}             element i: low nibble of qs[i] (i < 16), high nibble of qs[i - 16]; value = nibble - 8
//   Q5_0  22 B = {f16 d, u8 qh[4], u8 qs[16]}   nibbles as Q4_0; bit i of qh = bit 4 of element i; value = 5 bits - 16
//   Q8_0  34 B = {f16 d, i8 qs[32]}
// and their "_1" siblings, whose quants are UNSIGNED with a per-block minimum m and whose activations are Q8_1 blocks {f16 d, f16 s = d * sum(qs), i8 qs[32]}:
//   Q4_1  20 B = {f16 d, f16 m, u8 qs[16]}             nibbles as Q4_0; value = nibble * d + m
//   Q5_1  24 B = {f16 d, f16 m, u8 qh[4], u8 qs[16]}   nibbles and qh as Q5_0; value = (5 bits) * d + m
// and IQ4_NL (ggml-common.h block_iq4_nl), byte for byte the geometry of Q4_0, its nibble an index into a table of 16 signed values; Q8_0 activations:
//   IQ4_NL 18 B = {f16 d, u8 qs[16]}            nibbles as Q4_0; value = kvalues_iq4nl[nibble] * d, the table -127 .. 113 (ggml-quants.c:3548; here b32_iq4nl_values and, by index, iq4nl_value: bamd_device.h)
// and IQ4_XS (ggml-common.h:393-398), the same table under K-quant clothes: a 256-weight super-block of eight 32-blocks with 6-bit scales, Q8_K activations:
//   IQ4_XS 136 B = {f16 d, u16 scales_h, u8 scales_l[4], u8 qs[128]}   32-block ib: ls = (scales_l[ib/2] >> 4*(ib%2) & 0xf) | (scales_h >> 2*ib & 3) << 4, used as ls - 32;
//                                               qs[16 ib + j]: low nibble = weight 32 ib + j, high nibble = weight 32 ib + 16 + j (each 32-block a Q4_0 / IQ4_NL block)
//
// Wave-stream layout (our design; the GGUF file itself is untouched).  A matrix [nrows][K] is cut into
// row-groups of 8 rows; for each row-group the K/256 super-blocks follow one another as RECORDS, and a record
// holds the same super-block index of all 8 rows, arranged so that wave lane (r*8 + e) — row r of the group,
// SIMD-lane e of the reference's 256-bit AVX2 registers — finds its bytes at lane*16:
//
//   Q4_K record 1152 B: [qs   : lane*16 -> 4 dwords j=0..3 = file qs[32j+4e .. +3]      ] 1024 B
//                       [hdr  : r*16    -> file bytes 0..15 (d, dmin, scales[12])       ]  128 B
//   Q5_K record 1408 B: [qs 1024 B as Q4_K][qh: lane*4 -> file qh[4e..4e+3] 256 B][hdr 128 B]
//   (BAMD_XSCALES = 1, an experiment kept behind the macro: hdr = {d | dmin<<16, sc[0..3], sc[4..7], mn[0..3]} + 32 B of mn[4..7])
//   Q6_K record 1680 B: [ql   : lane*16 -> 4 dwords j=0..3 = file ql[32j+4e .. +3]      ] 1024 B
//                       [qh   : lane*8  -> 2 dwords m=0,1 = file qh[32m+4e .. +3]      ]  512 B
//                       [sc   : r*16    -> byte hi*8+c = file scales[2c+hi]             ]  128 B
//                       [d    : r*2     -> f16 d                                        ]   16 B
//   Q3_K record  880 B: [qs   : lane*8  -> 2 dwords j=0,1 = file qs[32j+4e .. +3]       ]  512 B
//                       [hmask: lane*4  -> file hmask[4e .. 4e+3]                        ]  256 B
//                       [sc   : r*12    -> file scales[12] (packed 6-bit, as in the file)]   96 B
//                       [d    : r*2     -> f16 d                                        ]   16 B
//   Q2_K record  672 B: [qs   : lane*8  -> 2 dwords j=0,1 = file qs[32j+4e .. +3]       ]  512 B
//                       [sc   : r*16    -> file scales[16]                              ]  128 B
//                       [dd   : r*4     -> f16 d, f16 dmin                              ]   32 B
//   Q8_0 / Q4_0 / Q5_0: a record is still 8 rows x 256 weights = eight 32-blocks c = 0..7 per row; lane (r, e) covers bytes 4e .. 4e+3 of every block
//   (SIMD lane e of the reference's 256-bit accumulator, sgemm.cpp:711-759)
//   Q8_0 record 2176 B: [qs   : h*1024 + lane*16 -> 4 dwords j=0..3 = block c=4h+j, file qs[4e .. 4e+3]   ] 2048 B (h = 0, 1)
//                       [d    : r*16    -> eight f16 d, block c = 0..7                  ]  128 B
//   Q4_0 record 1152 B: [qs   : (r*4 + (e&3))*32 -> 8 dwords c=0..7 = file qs[4(e&3) .. +3]: lanes e and e+4 read the SAME 32 bytes, low / high nibbles] 1024 B
//                       [d    : r*16    -> eight f16 d                                  ]  128 B
//   Q5_0 record 1408 B: [qs 1024 B as Q4_0][qh: lane*4 -> one dword, bit 8t + c = bit 4e + t of block c's qh   ] 256 B [d 128 B]
//   Q4_1 record 1280 B: [qs 1024 B as Q4_0][dm: r*32 -> eight f16 d, then eight f16 m, block c = 0..7    ] 256 B
//   Q5_1 record 1536 B: [qs 1024 B as Q4_0][qh 256 B as Q5_0][dm 256 B as Q4_1]
//   IQ4_NL record 1152 B: the Q4_0 record, written by the Q4_0 repack (bamd_launch_repack)
//   F32 / F16 / BF16 (unquantised): a record is 8 rows x 256 weights too, and every lane's share of it is whole 16-byte loads, request q of a record at q*1024 + lane*16
//   F32  record 8192 B: lane (r, j) owns w[r][8i + j], i = 0..31 (lane j of the reference's 8-lane accumulator, sgemm.cpp:408-432): request q = 0..7 holds i = 4q .. 4q+3
//   F16  record 4096 B: the same ownership, request q = 0..3 holds i = 8q .. 8q+7 (eight halves)
//   BF16 record 4096 B: a row has 32 chain lanes c = 8a + j (accumulator a = 0..3, lane j of ggml_vec_dot_bf16's AVX2 branch, ggml.c:2007-2026), chain lane c owns
//                       w[r][32i + c], i = 0..7: request q = 0..3 holds rows 2q (wave lanes 0-31) and 2q + 1 (lanes 32-63), eight bf16 per lane
//   IQ4_XS record 1088 B: [qs  : (r*4 + (e&3))*32 -> 8 dwords c=0..7 = file qs[16c + 4(e&3) .. +3]: the Q4_0 geometry, lanes e and e+4 read the SAME 32 bytes ] 1024 B
//                       [hdr  : r*8     -> file bytes 0..7 (d, scales_h, scales_l[4]): one 8-byte load per lane        ]   64 B
//   (Q3_K / Q2_K: 3.4375 / 2.625 bits per weight leave a lane 8 B of qs per super-block, so its widest load is 8 bytes; records are 16-byte multiples)
//
// Record bytes = 8 x file block bytes, so HBM traffic per weight is exactly the GGUF's bits per weight, every
// wave load instruction is one contiguous, 16-byte-per-lane kilobyte, and consecutive records of a row-group
// are consecutive in memory (a pure sequential stream per wave).
#pragma once
#include <stdint.h>
#include <stddef.h>

#define BAMD_QK_K 256
#ifdef __HIPCC__
#define BAMD_HD __host__ __device__
#else
#define BAMD_HD
#endif

enum bamd_type { BAMD_F32 = 0, BAMD_F16 = 1, BAMD_BF16 = 30, BAMD_Q4_0 = 2, BAMD_Q4_1 = 3, BAMD_Q5_0 = 6, BAMD_Q5_1 = 7, BAMD_Q8_0 = 8, BAMD_Q2_K = 10, BAMD_Q3_K = 11, BAMD_Q4_K = 12, BAMD_Q5_K = 13, BAMD_Q6_K = 14, BAMD_IQ4_NL = 20, BAMD_IQ4_XS = 23 };

BAMD_HD static inline int bamd_is_q0(int t) { return t == BAMD_Q8_0 || t == BAMD_Q4_0 || t == BAMD_Q5_0; }       // 32-weight blocks, Q8_0 activations
// the same family by record geometry and activation form, IQ4_NL included: what everything but the matrix-core prompt kernels and split-K asks (those two have
// no IQ4_NL instance and keep asking bamd_is_q0)
BAMD_HD static inline int bamd_takes_q8_0(int t) { return bamd_is_q0(t) || t == BAMD_IQ4_NL; }
BAMD_HD static inline int bamd_is_q1(int t) { return t == BAMD_Q4_1 || t == BAMD_Q5_1; }                               // 32-weight blocks with a minimum, Q8_1 activations
BAMD_HD static inline int bamd_is_b32(int t) { return bamd_takes_q8_0(t) || bamd_is_q1(t); }                         // any 32-weight block type: Q8_0 / Q4_0 / Q5_0, IQ4_NL, Q4_1 / Q5_1
BAMD_HD static inline int bamd_is_flt(int t) { return t == BAMD_F32 || t == BAMD_F16 || t == BAMD_BF16; }               // unquantised weights: f32 activations (F32 / F16) or bf16 ones (BF16)
// the form a launch quantises its activations to for weights of type t; one launch has one form (0 = a type without a mat-vec kernel)
enum bamd_act_form { BAMD_ACT_NONE = 0, BAMD_ACT_Q8_K = 1, BAMD_ACT_Q8_0 = 2, BAMD_ACT_Q8_1 = 3, BAMD_ACT_F32 = 4, BAMD_ACT_BF16 = 5 };
// (the load-time repack kernel asks the first of the two: IQ4_NL reaches it as Q4_0, bamd_launch_repack)
BAMD_HD static inline int bamd_block_bytes_repack(int t) {
    return t == BAMD_Q4_1 ? 20 : t == BAMD_Q5_1 ? 24 : t == BAMD_Q4_K ? 144 : t == BAMD_Q5_K ? 176 : t == BAMD_Q6_K ? 210 : t == BAMD_Q3_K ? 110 : t == BAMD_Q2_K ? 84 : t == BAMD_IQ4_XS ? 136 : t == BAMD_Q8_0 ? 34 : t == BAMD_Q4_0 ? 18 : t == BAMD_Q5_0 ? 22 : 0;
}
BAMD_HD static inline int bamd_block_bytes(int t) { return t == BAMD_IQ4_NL ? 18 : bamd_block_bytes_repack(t); }
BAMD_HD static inline int bamd_block_weights(int t) { return bamd_takes_q8_0(t) || bamd_is_q1(t) ? 32 : BAMD_QK_K; }
#ifndef BAMD_XSCALES
#define BAMD_XSCALES 0          /* 0: the file's 12 packed scale bytes per row (records of 1152 / 1408 B = 8 x the GGUF block); 1: unpacked scales and
                                   mins, a byte each (1184 / 1440 B) — measured SLOWER on the MI355X in round 2 (gate/up 14.8 vs 13.2 us, decode 649 vs
                                   666 tok/s): 9 vector instructions saved per record do not pay for +2.8 % bytes, a third request per record and
                                   records that no longer start on a 128-byte line */
#endif
#define BAMD_RECB_Q4K (BAMD_XSCALES ? 1184 : 1152)
#define BAMD_RECB_Q5K (BAMD_XSCALES ? 1440 : 1408)
#define BAMD_RECB_Q6K 1680
#define BAMD_RECB_Q3K 880
#define BAMD_RECB_Q2K 672
#define BAMD_RECB_IQ4XS 1088
#define BAMD_RECB_Q80 2176
#define BAMD_RECB_Q40 1152
#define BAMD_RECB_Q50 1408
#define BAMD_RECB_Q41 1280
#define BAMD_RECB_Q51 1536
#define BAMD_RECB_F32 8192
#define BAMD_RECB_F16 4096
#define BAMD_RECB_BF16 4096
// record bytes as a constant expression of a kernel's TYPE template argument; a type without a record does not compile
#define BAMD_RECB_OF(T_) ((T_) == BAMD_Q4_K ? BAMD_RECB_Q4K : (T_) == BAMD_Q5_K ? BAMD_RECB_Q5K : (T_) == BAMD_Q6_K ? BAMD_RECB_Q6K : (T_) == BAMD_Q3_K ? BAMD_RECB_Q3K : (T_) == BAMD_Q2_K ? BAMD_RECB_Q2K : (T_) == BAMD_IQ4_XS ? BAMD_RECB_IQ4XS : (T_) == BAMD_Q8_0 ? BAMD_RECB_Q80 : (T_) == BAMD_Q4_0 ? BAMD_RECB_Q40 : (T_) == BAMD_Q5_0 ? BAMD_RECB_Q50 : (T_) == BAMD_Q4_1 ? BAMD_RECB_Q41 : (T_) == BAMD_Q5_1 ? BAMD_RECB_Q51 : (T_) == BAMD_IQ4_NL ? BAMD_RECB_Q40 : -1)
BAMD_HD static inline int bamd_record_bytes_quant(int t) { return t == BAMD_Q4_K ? BAMD_RECB_Q4K : t == BAMD_Q5_K ? BAMD_RECB_Q5K : t == BAMD_Q6_K ? BAMD_RECB_Q6K : t == BAMD_Q3_K ? BAMD_RECB_Q3K : t == BAMD_Q2_K ? BAMD_RECB_Q2K : t == BAMD_IQ4_XS ? BAMD_RECB_IQ4XS : t == BAMD_Q8_0 ? BAMD_RECB_Q80 : t == BAMD_Q4_0 ? BAMD_RECB_Q40 : t == BAMD_Q5_0 ? BAMD_RECB_Q50 : t == BAMD_Q4_1 ? BAMD_RECB_Q41 : t == BAMD_Q5_1 ? BAMD_RECB_Q51 : 0; }   // the quantised types only (what the load-time repack of bamd_matvec.hip asks)
BAMD_HD static inline int bamd_record_bytes_repack(int t) { return t == BAMD_F32 ? BAMD_RECB_F32 : t == BAMD_F16 ? BAMD_RECB_F16 : t == BAMD_BF16 ? BAMD_RECB_BF16 : bamd_record_bytes_quant(t); }   // (what the repack of bamd_matvec_flt.hip asks)
BAMD_HD static inline int bamd_record_bytes(int t) { return t == BAMD_IQ4_NL ? BAMD_RECB_Q40 : bamd_record_bytes_repack(t); }   // wave-stream record: 8 rows x 256 weights
// bytes of the wave-stream copy of a quantised matrix [nrows_pad (multiple of 8)][K]
BAMD_HD static inline size_t bamd_stream_bytes(int t, int64_t k, int64_t nrows_pad) { return (size_t) (nrows_pad / 8) * (size_t) (k / BAMD_QK_K) * (size_t) bamd_record_bytes(t); }
// the 256-weight super-block types with Q8_K activations; IQ4_XS is one of them by record, activation form and chain (it has no dmin, no side table and no
// matrix-core prompt kernel: whoever means one of those asks for the type, bamd_prefill_family.h)
BAMD_HD static inline int bamd_is_kquant(int t) { return t == BAMD_Q4_K || t == BAMD_Q5_K || t == BAMD_Q6_K || t == BAMD_Q3_K || t == BAMD_Q2_K || t == BAMD_IQ4_XS; }
BAMD_HD static inline size_t bamd_row_bytes(int t, int64_t k) {
    return t == BAMD_F32 ? (size_t) k * 4 : t == BAMD_F16 || t == BAMD_BF16 ? (size_t) k * 2 : (size_t) (k / bamd_block_weights(t)) * bamd_block_bytes(t);
}
BAMD_HD static inline int bamd_has_record(int t) { return bamd_is_kquant(t) || bamd_takes_q8_0(t) || bamd_is_q1(t) || bamd_is_flt(t); }     // has a wave-stream record (rows of K % 256 == 0)
BAMD_HD static inline int bamd_act_form_of(int t) { return bamd_is_kquant(t) ? BAMD_ACT_Q8_K : bamd_takes_q8_0(t) ? BAMD_ACT_Q8_0 : bamd_is_q1(t) ? BAMD_ACT_Q8_1 : t == BAMD_BF16 ? BAMD_ACT_BF16 : bamd_is_flt(t) ? BAMD_ACT_F32 : BAMD_ACT_NONE; }
// the float family holds its whole activation vector in the LDS of a CU (4 bytes per element as f32, 2 as bf16, beside 256 bytes of reduction slots): the longest row a mat-vec of type t takes
BAMD_HD static inline int bamd_flt_max_k(int t) { return t == BAMD_BF16 ? 65536 : 40704; }
// bytes of one token's activations in form f for the batched prompt mat-muls of the float family (the quantised forms: bamd_blob_bytes)
BAMD_HD static inline size_t bamd_flt_act_bytes(int form, int64_t k) { return form == BAMD_ACT_F32 ? (size_t) k * 4 : form == BAMD_ACT_BF16 ? (size_t) k * 2 : 0; }
