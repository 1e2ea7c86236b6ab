// bamd_bf16_range.h — the exponent range of a set of bf16 values as one word, and the guard of the BF16 matrix-core prompt kernel over two of them
// (bamd_prefill2_bf16.hip states what the guard decides and why; host and device).
// A word: bits 0-15 = the lowest, bits 16-31 = the highest max(E, 1) over the set's NONZERO values, E = (h >> 7) & 0xff the exponent field of pattern h.
// A set without a nonzero value is BAMD_BF16_RANGE_NONE (lowest 0x1ff, highest 0); an infinity or NaN shows as highest = 255.
#pragma once
#include <stdint.h>
#include "bamd_formats.h"

#define BAMD_BF16_RANGE_NONE 0x000001ffu
#define BAMD_BF16_RANGE_UNKNOWN 0x00ff0001u                /* a set nobody measured: never safe */
// one more pattern (the low 16 bits of h) into lo / hi
BAMD_HD static inline void bamd_bf16_range_add(uint32_t & lo, uint32_t & hi, uint32_t h) {
    if (!(h & 0x7fffu)) return;
    uint32_t e = (h >> 7) & 0xffu;
    e = e ? e : 1u;
    lo = e < lo ? e : lo; hi = e > hi ? e : hi;
}
BAMD_HD static inline void bamd_bf16_range_add2(uint32_t & lo, uint32_t & hi, uint32_t two) { bamd_bf16_range_add(lo, hi, two & 0xffffu); bamd_bf16_range_add(lo, hi, two >> 16); }
// the union of two words
BAMD_HD static inline uint32_t bamd_bf16_range_join(uint32_t a, uint32_t b) {
    const uint32_t lo = (a & 0xffffu) < (b & 0xffffu) ? (a & 0xffffu) : (b & 0xffffu), hi = (a >> 16) > (b >> 16) ? (a >> 16) : (b >> 16);
    return lo | hi << 16;
}
// every product of a value of set w and a value of set x is exact in f32: with e = max(E, 1) - 127, emin_w + emin_x >= -135 and emax_w + emax_x <= 126
// (biased: >= 119 and <= 380), no E == 255 on either side; a side without a nonzero value is safe
BAMD_HD static inline bool bamd_bf16_ranges_safe(uint32_t w, uint32_t x) {
    const uint32_t wl = w & 0xffffu, wh = w >> 16, xl = x & 0xffffu, xh = x >> 16;
    if (wh >= 255u || xh >= 255u) return false;
    if (wh == 0u || xh == 0u) return true;
    return wl + xl >= 119u && wh + xh <= 380u;
}
