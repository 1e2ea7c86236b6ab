// bamd_prefill2_b32.h — what the two matrix-core prompt kernels of the 32-weight block formats share: the dense one (bamd_prefill2_b32.hip, where the arithmetic,
// the lane maps and the reasons for the tile are written down) and the grouped, gathered one of the mixture-of-experts micro-batch (bamd_moe_batch_b32_mfma.hip).
// The tile of a type, the lane's weight pieces of half a record, and their unpack to unsigned bytes.
#pragma once
#include <type_traits>
#include "bamd_b32_device.h"
#include "bamd_mfma_common.h"

typedef float bamd_f16v __attribute__((ext_vector_type(16)));
typedef float bamd_f2 __attribute__((ext_vector_type(2)));
typedef _Float16 bamd_h2q __attribute__((ext_vector_type(2)));
union bamd_h2qu { uint32_t u; bamd_h2q h; };

#define Y_ROWS 64                                          /* rows of a workgroup: four waves x 16 */
#define Y_QSTR 528                                         /* LDS bytes between the quants of consecutive tokens */
// the tile of a type: a wave owns NT token tiles of 16 and NP accumulator sets per output, NT * NP = 2 either way (64 accumulator registers)
template <int TYPE> struct YTile {
    static constexpr int NP = b32_two_acc(TYPE) ? 2 : 1;      // accumulator sets per output: by block parity
    static constexpr int NT = b32_two_acc(TYPE) ? 1 : 2;      // token tiles of a wave
    static constexpr int TOK = 16 * NT;                       // tokens of a workgroup
    static constexpr int XD_OFF = TOK * Y_QSTR;               // d_x of the stage: [block c][token] f32
    static constexpr int XS_OFF = XD_OFF + 8 * TOK * 4;       // MIN: s_x of the stage, the same shape
    static constexpr int STAGE = b32_has_min(TYPE) ? XS_OFF + 8 * TOK * 4 : XS_OFF;     // 17 920 B, MIN 18 944 B, two sets 8 960 B
};
// a BAMD_B16_REC record in this form uses 544 bytes: element 4e + k of block c as f16 at half c * 32 + (e & 3) * 8 + (e >> 2) * 4 + k (the A operands of both
// e-halves of an MFMA lane are 16 consecutive bytes), then the eight d_x as f32 at byte 512; MIN: 576 bytes, the eight s_x as f32 at byte 544
static_assert(BAMD_B16_REC >= 512 + 32 + 32, "the f16 activation record holds the quants, eight d_x and eight s_x");

// the lane's pieces of HALF a record (blocks c = 4h .. 4h+3) for its two chunks e = g and g + 4
template <int TYPE> struct HalfB32 { uint4 q[TYPE == BAMD_Q8_0 ? 2 : 1]; uint32_t qh[2]; };
// (r by reference for the two-set type, by value for the others: either form for all six moves the address arithmetic of the other group's prologue — with r by
//  value the IQ4_NL side-table pointer becomes a float index, its prologue is scheduled in another order and loses one v_mov_b32; profiles/b32_mfma_unify.txt)
template <int TYPE> using y_row_arg = std::conditional_t<b32_two_acc(TYPE), const int &, int>;
template <int TYPE> __device__ __forceinline__ void load_half(HalfB32<TYPE> & H, const uint8_t * rec, int h, y_row_arg<TYPE> r, int g) {
    if (TYPE == BAMD_Q8_0) {
        H.q[0] = *(const uint4 *) (rec + h * 1024 + (r * 8 + g) * 16); H.q[1] = *(const uint4 *) (rec + h * 1024 + (r * 8 + g + 4) * 16);
    } else {
        H.q[0] = *(const uint4 *) (rec + (r * 4 + g) * 32 + h * 16);             // chunks g and g + 4 share the bytes: low / high nibbles
        if (b32_has_qh(TYPE)) { H.qh[0] = *(const uint32_t *) (rec + 1024 + (r * 8 + g) * 4); H.qh[1] = *(const uint32_t *) (rec + 1024 + (r * 8 + g + 4) * 4); }
    }
}
// the four weights of block 4h + cl, chunk 4 eh + g, as unsigned bytes u = weight + offset (128 / 8 / 16; MIN: b32_weights' bytes, no offset)
template <int TYPE> __device__ __forceinline__ uint32_t half_bytes(const HalfB32<TYPE> & H, int h, int cl, int eh) {
    if (TYPE == BAMD_Q8_0) return BAMD_B32_COMP(H.q[eh], cl) ^ 0x80808080u;
    const uint32_t nib = (BAMD_B32_COMP(H.q[0], cl) >> (eh * 4)) & 0x0f0f0f0fu;
    if (TYPE == BAMD_IQ4_NL) return b32_iq4nl_values(nib) ^ 0x80808080u;     // value + 128 (1 .. 241): the table stands in bamd_b32_device.h only
    if (!b32_has_qh(TYPE)) return nib;
    return nib | (((H.qh[eh] >> (4 * h + cl)) & 0x01010101u) << 4);
}
// the f16 constant that takes 0x6400 | u = 1024 + u back to the weight: -(1024 + offset), exact in f16
template <int TYPE> __device__ __forceinline__ _Float16 y_kzero() {
    return b32_has_min(TYPE) ? (_Float16) -1024.f : TYPE == BAMD_Q8_0 || TYPE == BAMD_IQ4_NL ? (_Float16) -1152.f : TYPE == BAMD_Q4_0 ? (_Float16) -1032.f : (_Float16) -1040.f;
}
