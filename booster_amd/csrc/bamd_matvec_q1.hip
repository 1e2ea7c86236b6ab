// bamd_matvec_q1.hip — single-token mat-vec for the 32-weight block formats with a minimum, Q4_1 / Q5_1 (bamd_formats.h): the Q8_1 activation prologue and
// one wave per row-group.  A launch whose segments are all of this family comes here (bamd_launch_mv, bamd_kernels.h); the K-quant and Q8_0-family kernels
// are not touched by these types.  There is no split-K kernel: it measured slower than one wave per row-group for the whole Q8_0 family
// (profiles/legacy_matvec.txt), and a request for it (mode 2) is refused by the caller in words.
//
// Numerics, records and the two chains: bamd_q1_device.h.
#include "bamd_matvec_core.h"
#include "bamd_q1_device.h"

struct Q1Lds { uint32_t * q8; float * ys; double * red; };
__device__ __forceinline__ Q1Lds carve_lds_q1(const bamd_mv_args & a, unsigned char * smem) {
    const ProArgs pa = carve_lds(a, smem);
    Q1Lds l; l.q8 = pa.q8; l.ys = (float *) pa.S; l.red = pa.red;
    return l;
}

// the streaming loop of q0_stream (bamd_matvec_q0.hip): a ring of D records, the loader one chunk ahead; beside the lane's chain the row's scalar chain
template <int TYPE, int D, int EPI, bool NORM>
__device__ __forceinline__ void q1_stream(const uint8_t * __restrict__ wA, const uint8_t * __restrict__ wB, int nb, int first, int count, int stride,
                                          float * __restrict__ out, const float * __restrict__ res, const bamd_mv_args & a, const Q1Lds & L, bool do_pro,
                                          unsigned long long & best, int nvalid) {
    constexpr int RECB = BAMD_RECB_OF(TYPE);
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    constexpr int NPARTS = PAIR ? 2 : 1;
    const int lane = threadIdx.x & 63;
    const bamd_rsrc rsA = weight_rsrc(wA), rsB = PAIR ? weight_rsrc(wB) : rsA, rsN = null_rsrc(wA);
    const int rgb = nb * RECB;
    const int rg_step = stride * rgb;
    const int chunks = nb / D;
    ActProQ0<NORM> ap;
    if (do_pro) ap.issue(a.x, a.normw, a.K, wave_id());     // activation loads go out first
    RecQ1<TYPE> ring[D];
#pragma unroll
    for (int s = 0; s < D; ++s) load_rec(ring[s], rsA, first * rgb + s * RECB, lane);
    if (do_pro) ap.template finish_q0<true>(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red);
    for (int r = 0; r < count; ++r) {
        const int rg = first + r * stride;
        const int row = rg * 8 + (lane >> 3);
        const int rowoff = rg * rgb;
        float gate_val = 0.f;
#pragma unroll
        for (int part = 0; part < NPARTS; ++part) {
            const bool last = !(PAIR && part == 0) && r + 1 >= count;
            const bool after_b = PAIR && part == 0;
            const int after_off = (PAIR && part == 0) ? rowoff : rowoff + rg_step;
            float resv = 0.f;
            if (EPI == BAMD_EPI_ADD && row < nvalid) resv = ik_ld(res + row);
            float acc = 0.f, summs = 0.f;
            for (int c = 0; c < chunks; ++c) {
                const bool inrow = c + 1 < chunks;
                const bool tail = !inrow && last;            // behind the wave's last chunk: the zero-record descriptor (returns 0, fetches nothing)
                const bamd_rsrc nrs = tail ? rsN : (inrow ? part == 1 : after_b) ? rsB : rsA;
                const int nxt = tail ? 0 : inrow ? rowoff + (c + 1) * (D * RECB) : after_off;
#pragma unroll
                for (int s = 0; s < D; ++s) {
                    pin_rec(ring[s]);
                    float sc[8], fd[8], ms[8];
                    q1_terms(ring[s], c * D + s, lane, L.q8, L.ys, sc, fd, ms);
                    q0_chain8(acc, sc, fd);
                    q1_summs8(summs, ms);
                    load_rec(ring[s], nrs, nxt + s * RECB, lane);
                    if ((s & (BAMD_SCHED_GROUP - 1)) == BAMD_SCHED_GROUP - 1) __builtin_amdgcn_sched_barrier(0);
                }
            }
            const float val = q1_finish_row(acc, summs);
            if (PAIR) {
                if (part == 0) gate_val = val;
                else if ((lane & 7) == 0 && row < nvalid) ik_st(out + row, v_silu(gate_val) * val);
            } else if ((lane & 7) == 0 && row < nvalid) {
                float o = val;
                if (EPI == BAMD_EPI_ADD) o = val + resv;
                ik_st(out + row, o);
                if (EPI == BAMD_EPI_ARGMAX) { const unsigned long long k = argmax_key(o, row); best = k > best ? k : best; }
            }
        }
    }
}
template <int TYPE, int EPI, bool NORM>
__device__ __forceinline__ void q1_stream_depth(const uint8_t * wA, const uint8_t * wB, int nb, int first, int count, int stride, float * out, const float * res,
                                                const bamd_mv_args & a, const Q1Lds & L, bool do_pro, unsigned long long & best, int nvalid) {
    if ((nb & 3) == 0)      q1_stream<TYPE, 4, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
    else if ((nb & 1) == 0) q1_stream<TYPE, 2, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
    else                    q1_stream<TYPE, 1, EPI, NORM>(wA, wB, nb, first, count, stride, out, res, a, L, do_pro, best, nvalid);
}

template <int PRO, int EPI>
__global__ void __launch_bounds__(512) matvec_q1_kernel(bamd_mv_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool NORM = PRO == BAMD_PRO_NORM;
    const int nb = a.K >> 8;
    const Q1Lds L = carve_lds_q1(a, smem);
    const int wave = wave_id(), nwaves = blockDim.x >> 6;
    const int slot = blockIdx.x + gridDim.x * wave;          // consecutive row-groups land on different CUs
    const int stride = gridDim.x * nwaves;
    unsigned long long best = 0ull;
    constexpr bool PAIR = EPI == BAMD_EPI_SILU_MUL;
    bool pro_done = false;
    int off = 0;
    const int nseg = PAIR ? 1 : a.nseg;
    for (int s = 0; s < nseg; ++s) {
        const int nrg = a.seg[s].nrows >> 3;
        const int k0 = off <= slot ? 0 : (off - slot + stride - 1) / stride;
        const int g0 = slot + k0 * stride;
        const int count = g0 < off + nrg ? (off + nrg - 1 - g0) / stride + 1 : 0;
        if (count > 0) {
            const int t = a.seg[s].type;
            const uint8_t * wA = (const uint8_t *) a.seg[s].w;
            const uint8_t * wB = PAIR ? (const uint8_t *) a.seg[1].w : wA;
            const int nv = a.seg[s].nvalid > 0 ? a.seg[s].nvalid : a.seg[s].nrows;
            if (t == BAMD_Q4_1)      q1_stream_depth<BAMD_Q4_1, EPI, NORM>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, best, nv);
            else if (t == BAMD_Q5_1) q1_stream_depth<BAMD_Q5_1, EPI, NORM>(wA, wB, nb, g0 - off, count, stride, a.seg[s].out, a.res, a, L, !pro_done, best, nv);
            else __builtin_trap();                           // unreachable: bamd_launch_matvec_q1 refuses any other type on the host
            pro_done = true;
        }
        off += nrg;
    }
    if (!pro_done) { ActProQ0<NORM> ap; ap.issue(a.x, a.normw, a.K, wave); ap.template finish_q0<true>(a.x, a.normw, a.eps, a.K, L.q8, L.ys, L.red); }   // idle waves still owe the block its barriers
    if (EPI == BAMD_EPI_ARGMAX) {
        for (int o = 32; o; o >>= 1) { const unsigned long long ob = __shfl_xor(best, o); best = ob > best ? ob : best; }
        __syncthreads();
        unsigned long long * wb = (unsigned long long *) smem;
        if ((threadIdx.x & 63) == 0) wb[wave] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long b = 0ull;
            for (int w = 0; w < nwaves; ++w) b = wb[w] > b ? wb[w] : b;
            if (b) atomicMax(a.best_key, b);
        }
    }
}

// test entry: standard block_q8_1 bytes {f16 d, f16 s, i8 qs[32]} out of the prologue (parity with quantize_row_q8_1)
__global__ void __launch_bounds__(512) quantize_q81_test_kernel(const float * x, const float * nw, float eps, int K, int norm, uint8_t * out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int nb = K >> 8;
    uint32_t * q8 = (uint32_t *) smem; float * ys = (float *) (q8 + nb * 64);
    double * red = (double *) (smem + BAMD_ACT_RED_OFF(nb));
    if (norm) { ActProQ0<true> ap; ap.issue(x, nw, K, wave_id()); ap.template finish_q0<true>(x, nw, eps, K, q8, ys, red); }
    else { ActProQ0<false> ap; ap.issue(x, nw, K, wave_id()); ap.template finish_q0<true>(x, nw, eps, K, q8, ys, red); }
    for (int i = threadIdx.x; i < nb * 64; i += blockDim.x) {
        const int blk = i >> 6, e = (i >> 3) & 7, c = i & 7;
        const uint32_t w = q8[i];
        uint8_t * o = out + ((size_t) blk * 8 + c) * 36;
        for (int t = 0; t < 4; ++t) o[4 + 4 * e + t] = (uint8_t) (w >> (8 * t));
    }
    for (int i = threadIdx.x; i < nb * 8; i += blockDim.x) {
        const uint32_t ds = ((const uint32_t *) ys)[i];      // {f16 d, f16 s} as the block holds them
        for (int t = 0; t < 4; ++t) out[(size_t) i * 36 + t] = (uint8_t) (ds >> (8 * t));
    }
}

// ===========================================================================================================
// launchers
// ===========================================================================================================
void bamd_launch_quantize_q81_test(const float * x, const float * nw, float eps, int K, int norm, void * out, hipStream_t s) {
    BAMD_LAUNCH(quantize_q81_test_kernel, dim3(1), dim3(512), act_lds_bytes(K), s, x, nw, eps, K, norm, (uint8_t *) out);
}

// every segment Q4_1 / Q5_1.  One wave per row-group for every shape; 2 = split-K was asked for (mode 2): these types have none
int bamd_launch_matvec_q1(const bamd_mv_args & a, int pro, int epi, int n_cu, hipStream_t s) {
    for (int i = 0; i < a.nseg; ++i) if (!bamd_is_q1(a.seg[i].type)) return 1;
    if ((a.mode & 15) == 2) return 2;
    int nrg = 0;
    if (epi == BAMD_EPI_SILU_MUL) nrg = a.seg[0].nrows >> 3;
    else for (int i = 0; i < a.nseg; ++i) nrg += a.seg[i].nrows >> 3;
    const int cus = n_cu > 0 ? n_cu : 256;
    const int grid = nrg < 1 ? 1 : nrg < cus ? nrg : cus;
    typedef consts<BAMD_PRO_NORM, BAMD_PRO_PLAIN> pros;
    return with_const(pros(), pro, [&](auto P) -> bool { return with_const(consts<BAMD_EPI_STORE, BAMD_EPI_ADD, BAMD_EPI_SILU_MUL, BAMD_EPI_ARGMAX>(), epi, [&](auto E) -> bool {
        BAMD_LAUNCH((matvec_q1_kernel<decltype(P)::value, decltype(E)::value>), dim3(grid), dim3(512), act_lds_bytes(a.K), s, a); return true; }); }) ? 0 : 1;
}
