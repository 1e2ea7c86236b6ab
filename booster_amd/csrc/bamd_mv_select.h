// bamd_mv_select.h — what the mat-vec launch files (bamd_matvec.hip, bamd_matvec_fast_a.hip, bamd_matvec_fast_b.hip, bamd_colaunch.hip) share about
// CHOOSING a kernel instance and sizing its LDS: the run-time -> compile-time dispatchers, the switches, the generic split-K kernel's shape table and the
// layout of the dynamic LDS behind the activations.  Each of these facts is written here once; the selection itself is pinned by
// tests/test_launch_selection.py.  Included behind bamd_device.h (bamd_matvec_core.h).
#pragma once
#include <stdlib.h>
#include <type_traits>

// ---- switches: read once per process (static initialisers of the launch files).  on by default: off with NAME=0; off by default: on with NAME=1 ----
inline bool env_flag(const char * name, bool dflt) { const char * e = getenv(name); return dflt ? !(e && e[0] == '0') : (e && e[0] == '1'); }
inline int env_int(const char * name, int dflt) { const char * e = getenv(name); return e ? atoi(e) : dflt; }

// ---- run-time value -> compile-time constant --------------------------------------------------------------------------------------------------
// with_const(consts<A, B, ..>(), v, f): f(std::integral_constant<int, X>()) for the entry X == v; with_pair(pairs<cpair<A, B>, ..>(), x, y, f): f(cpair<A, B>())
// for the entry (A, B) == (x, y).  f returns "launched"; false = no such entry (or f declined): never a fall-through to another type.  The lists ARE the
// tables of which instances exist: every entry instantiates what f launches for it, in list order (a LEFT fold: hipcc expands a right fold last entry first,
// and the kernels of a code object are laid out in instantiation order).
template <int... VS> struct consts {};
template <int A, int B> struct cpair { static constexpr int a = A, b = B; };
template <typename... PS> struct pairs {};
template <int... VS, typename F> inline bool with_const(consts<VS...>, int v, F && f) { return (... || (v == VS && f(std::integral_constant<int, VS>()))); }
template <typename... PS, typename F> inline bool with_pair(pairs<PS...>, int x, int y, F && f) { return (... || (x == PS::a && y == PS::b && f(PS()))); }
typedef consts<BAMD_Q4_K, BAMD_Q5_K, BAMD_Q6_K, BAMD_Q3_K, BAMD_Q2_K, BAMD_IQ4_XS> kquants_all;      // (new types at the END: kernels are laid out in instantiation order)
typedef consts<BAMD_Q4_K, BAMD_Q5_K, BAMD_Q6_K> kquants_456;       // the families the low-bit types and IQ4_XS have no instance of
template <typename F> inline bool with_kquant(int type, F && f) { return with_const(kquants_all(), type, f); }

// fast kernels: row-groups per wave slot (mode A) / per workgroup (mode B), quotient and remainder
inline void mv_set_counts(bamd_mv_args & a, int nrg, int slots) { a.cnt_q = nrg / slots; a.cnt_r = nrg % slots; }

// ---- the generic split-K kernel's shapes ------------------------------------------------------------------------------------------------------
// K / 256 = nb super-blocks over the 8 waves of a workgroup -> records per wave and row-group (uneven: the larger share), row-groups per batch (the prefetch
// depth), term buffers.  nb a multiple of 8 with 1, 2, 4 or 7 records per wave; or uneven shares of 2-3, 5-6, 6-7 records (17..23, 41..47, 49..55
// super-blocks: Llama-2-13B's n_embd 5120, Llama-2-7B's n_ff 11008, Llama-2-13B's n_ff 13824).  (9..15 super-blocks — Llama-3.2-3B's n_embd 3072 — measured
// no faster split than with one wave per row-group: 6.9 / 4.8 us against 6.2 / 5.1 for its QKV / wo.)  K = 14336 with M = 2 (all of ffn_down's work per
// workgroup in flight from the first instruction, single-buffered) measured no better for Q4_K and 14 % worse for Q6_K than M = 1: the kernel is
// instruction-issue bound, not latency bound.  m == 0: no entry (mode A takes the launch)
struct SplitShape {
    int nbw, m, nbuf; bool uneven;
    constexpr bool operator==(const SplitShape & o) const { return nbw == o.nbw && m == o.m && nbuf == o.nbuf && uneven == o.uneven; }
};
constexpr SplitShape split_shape(int nb) {
    const int nbw = nb >> 3;
    if (nb & 7) return nbw == 5 ? SplitShape{6, 1, 2, true} : nbw == 6 ? SplitShape{7, 1, 2, true} : nbw == 2 ? SplitShape{3, 2, 2, true} : SplitShape{0, 0, 0, true};
    return nbw == 2 ? SplitShape{2, 4, 2, false} : nbw == 7 ? SplitShape{7, 1, 2, false} : nbw == 4 ? SplitShape{4, 2, 2, false} : nbw == 1 ? SplitShape{1, 8, 2, false}
                                                                                                                                  : SplitShape{0, 0, 0, false};
}
// term buffers of the fast split-K kernels: double-buffered while 2 x M x K/256 KiB fit the LDS (compact records: always two)
constexpr int split_fast_nbuf(int nbw, int m, bool compact) { return compact ? 2 : nbw * m > 8 ? 1 : 2; }

// ---- dynamic LDS of a mat-vec workgroup, byte offsets from its start ---------------------------------------------------------------------------
//   [0, BAMD_ACT_RED_OFF)             the Q8_K activations (carve_lds)
//   [BAMD_ACT_RED_OFF, mv_terms_off)  16 doubles of reduction scratch
//   [mv_terms_off, mv_park_off)       16 arg-max slots (mode A)          | split-K kernels: their term buffers start HERE (no arg-max epilogue) and run
//   [mv_park_off, ..)                 the gate/up kernels' park areas    | to mv_lds_terms: `row_groups` parked row-groups of nb records each
#define BAMD_LDS_CU_BYTES (160 * 1024)                                     /* one gfx950 CU */
constexpr size_t mv_terms_off(int nb) { return BAMD_ACT_RED_OFF(nb) + 16 * sizeof(double); }
constexpr size_t mv_park_off(int nb) { return act_lds_bytes(nb << 8); }
// a parked record: one float4 {d, fs, dmin, pm} per lane (1024 bytes), or compact {fs, pm} per lane + {d, dmin} per row (576 bytes)
constexpr size_t mv_term_rec_bytes(bool compact) { return compact ? 576 : 1024; }
constexpr size_t mv_term_floats(int nb, bool compact = false) { return (size_t) nb * (mv_term_rec_bytes(compact) / sizeof(float)); }      // per parked row-group
constexpr size_t mv_lds_terms(int nb, int row_groups, bool compact = false) { return mv_park_off(nb) + 16 + (size_t) row_groups * nb * mv_term_rec_bytes(compact); }
// gate/up with seven pairs per workgroup: park[3 pairs][gate | up][nb / 4][64 lanes] float4, then 4 flag words; with fourteen: [2 half pairs][8 rows] floats, 2 flag words
constexpr size_t mv_gu7_park_bytes(int nb) { return (size_t) 3 * 2 * (nb / 4) * 64 * 16; }
constexpr size_t mv_lds_gu7(int nb) { return mv_park_off(nb) + mv_gu7_park_bytes(nb) + 16; }
constexpr size_t mv_lds_gu14(int nb) { return mv_park_off(nb) + 16 * sizeof(float) + 2 * sizeof(int) + 8; }
// the co-launch: the wo role's term buffers, or the attention role's score + probability rows (ld floats each) where those are larger
constexpr size_t mv_lds_colaunch(int nb, int row_groups, int ld) { return mv_lds_terms(nb, row_groups) > (size_t) ld * 8 ? mv_lds_terms(nb, row_groups) : (size_t) ld * 8; }
