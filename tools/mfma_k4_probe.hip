// tools/mfma_k4_probe.hip — the K = 4 multi-block MFMAs on gfx950 (sibling of mfma_chain_probe.hip): the lane maps of v_mfma_f32_16x16x4_4b_f16 and
// v_mfma_f32_32x32x4_2b_f16, checked with exact integer data, and what one such instruction costs a SIMD — back to back, with the f32 chain FMAs of the
// Q8_0 / Q4_0 / Q5_0 prompt mat-mul beside it (acc = fma(S, result, acc) on the PREVIOUS instruction's results), and with its operands read from LDS.
//   build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -Wno-unused-value -mllvm -amdgpu-mfma-vgpr-form=1 -o tools/mfma_k4_probe tools/mfma_k4_probe.hip
//   run:   tools/mfma_k4_probe
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x32 __attribute__((ext_vector_type(32)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ---- lane maps: one instruction on given operands, every result register of every lane written out ---------------------------------------------
template <int WIDE>
__global__ void __launch_bounds__(64) map_kernel(const _Float16 * a, const _Float16 * b, float * d) {
    const int lane = threadIdx.x;
    h4 A, B;
    for (int k = 0; k < 4; ++k) { A[k] = a[lane * 4 + k]; B[k] = b[lane * 4 + k]; }
    if (WIDE) {
        f32x32 z; for (int v = 0; v < 32; ++v) z[v] = 0.f;
        const f32x32 r = __builtin_amdgcn_mfma_f32_32x32x4f16(A, B, z, 0, 0, 0);
        for (int v = 0; v < 32; ++v) d[lane * 32 + v] = r[v];
    } else {
        f32x16 z; for (int v = 0; v < 16; ++v) z[v] = 0.f;
        const f32x16 r = __builtin_amdgcn_mfma_f32_16x16x4f16(A, B, z, 0, 0, 0);
        for (int v = 0; v < 16; ++v) d[lane * 16 + v] = r[v];
    }
}

// ---- timing.  KIND 0: v_mfma_f32_32x32x4_2b_f16, 1: v_mfma_i32_32x32x4_2b_i8, 2: v_mfma_f32_16x16x4_4b_f16 (NR = 32 / 32 / 16 results per lane).  NF chain FMAs
//      (elements per lane) per MFMA on the previous result, PK: written as float2 (v_pk_fma_f32), LDS: the A / B operands and the scales re-read from LDS -----
template <int KIND, int NF, bool PK, bool LDS>
__global__ void __launch_bounds__(256) probe(float * out, int iters, const float * dsrc) {
    constexpr int NR = KIND == 2 ? 16 : 32;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 8192];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    h4 A, B;
    for (int i = 0; i < 4; ++i) { A[i] = (_Float16) (float) ((lane + i) & 7); B[i] = (_Float16) (float) ((lane * 3 + i) & 3); }
    unsigned char * my = smem + wave * 8192;
    for (int e = 0; e < 4; ++e) *(h4 *) (my + e * 512 + lane * 8) = e & 1 ? B : A;
    for (int i = 0; i < 16; ++i) ((float *) (my + 4096))[i * 64 + lane] = dsrc[(lane + i) & 15];
    __syncthreads();
    f2 acc[32];
    for (int i = 0; i < 32; ++i) acc[i] = (f2) { 0.f, 0.f };
    float S[16]; for (int i = 0; i < 16; ++i) S[i] = dsrc[(lane + i) & 15];
    float prev[NR]; for (int v = 0; v < NR; ++v) prev[v] = 0.f;
    f32x32 c0, c1; for (int v = 0; v < 32; ++v) { c0[v] = 0.f; c1[v] = 0.f; }
    i32x32 ic0, ic1; for (int v = 0; v < 32; ++v) { ic0[v] = 0; ic1[v] = 0; }
    f32x16 q0, q1; for (int v = 0; v < 16; ++v) { q0[v] = 0.f; q1[v] = 0.f; }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            union { h4 h; unsigned long long u; int i[2]; } oa, ob; oa.h = A; ob.h = B;
            asm volatile("" : "+v"(oa.u), "+v"(ob.u));        // opaque: the MFMA is not loop-invariant
            if (LDS) {
                oa.h = *(const volatile h4 *) (my + (u & 1) * 1024 + lane * 8); ob.h = *(const volatile h4 *) (my + 512 + (u & 1) * 1024 + lane * 8);
                if (u == 0) { for (int i = 0; i < 16; i += 4) { const f4 s = *(const volatile f4 *) (my + 4096 + ((it + i) & 15) * 256 + (lane >> 5) * 16); S[i] = s[0]; S[i + 1] = s[1]; S[i + 2] = s[2]; S[i + 3] = s[3]; } }
            }
            const h4 a = oa.h, b = ob.h;
            if (NF == 0) {                                    // back to back: two independent accumulators
                if (KIND == 0) { if (u & 1) c1 = __builtin_amdgcn_mfma_f32_32x32x4f16(a, b, c1, 0, 0, 0); else c0 = __builtin_amdgcn_mfma_f32_32x32x4f16(a, b, c0, 0, 0, 0); }
                if (KIND == 1) { if (u & 1) ic1 = __builtin_amdgcn_mfma_i32_32x32x4i8(oa.i[0], ob.i[0], ic1, 0, 0, 0); else ic0 = __builtin_amdgcn_mfma_i32_32x32x4i8(oa.i[0], ob.i[0], ic0, 0, 0, 0); }
                if (KIND == 2) { if (u & 1) q1 = __builtin_amdgcn_mfma_f32_16x16x4f16(a, b, q1, 0, 0, 0); else q0 = __builtin_amdgcn_mfma_f32_16x16x4f16(a, b, q0, 0, 0, 0); }
                continue;
            }
            float r[NR];
            if (KIND == 0) { f32x32 z; for (int v = 0; v < 32; ++v) z[v] = 0.f; const f32x32 t = __builtin_amdgcn_mfma_f32_32x32x4f16(a, b, z, 0, 0, 0); for (int v = 0; v < NR; ++v) r[v] = t[v]; }
            if (KIND == 1) { i32x32 z; for (int v = 0; v < 32; ++v) z[v] = 0; const i32x32 t = __builtin_amdgcn_mfma_i32_32x32x4i8(oa.i[0], ob.i[0], z, 0, 0, 0); for (int v = 0; v < NR; ++v) r[v] = (float) t[v]; }
            if (KIND == 2) { f32x16 z; for (int v = 0; v < 16; ++v) z[v] = 0.f; const f32x16 t = __builtin_amdgcn_mfma_f32_16x16x4f16(a, b, z, 0, 0, 0); for (int v = 0; v < NR; ++v) r[v] = t[v]; }
            __builtin_amdgcn_sched_barrier(0);
            if (PK) {
#pragma unroll
                for (int k = 0; k < NF; k += 2) {
                    const f2 s = { S[k & 15], S[(k + 1) & 15] }, p = { prev[k % NR], prev[(k + 1) % NR] };
                    acc[k >> 1] = __builtin_elementwise_fma(s, p, acc[k >> 1]);
                }
            } else {
#pragma unroll
                for (int k = 0; k < NF; ++k) { float t = acc[k >> 1][k & 1]; t = __builtin_fmaf(S[k & 15], prev[k % NR], t); asm volatile("" : "+v"(t)); acc[k >> 1][k & 1] = t; }      // (the empty asm keeps the halves apart)
            }
            for (int v = 0; v < NR; ++v) prev[v] = r[v];
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    float s = prev[0];
    for (int i = 0; i < 32; ++i) s += acc[i][0] + acc[i][1];
    for (int v = 0; v < 32; ++v) s += c0[v] + c1[v] + (float) (ic0[v] + ic1[v]);
    for (int v = 0; v < 16; ++v) s += q0[v] + q1[v];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int KIND, int NF, bool PK, bool LDS> static void run(const char * name, float * out, const float * dsrc, int ncu) {
    const int iters = 20000;
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL((probe<KIND, NF, PK, LDS>), dim3(ncu), dim3(256), 0, 0, out, 16, dsrc);
    hipDeviceSynchronize();
    hipEventRecord(a);
    hipLaunchKernelGGL((probe<KIND, NF, PK, LDS>), dim3(ncu), dim3(256), 0, 0, out, iters, dsrc);
    hipEventRecord(b); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    printf("%-100s %8.1f\n", name, ms * 1e-3 * 2.4e9 / ((double) iters * 4));
    fflush(stdout);
}

// hypothesis (both forms): A lane = NI block + i, B lane = NI block + j, the four k in the lane's halves; D register v of lane l: block v / RPB, column j = l % NI,
// row i = 4 (l / NI) + (v & 3) for 16 x 16 (RPB = 4) and 8 ((v % 16) >> 2) + 4 (l >> 5) + (v & 3) for 32 x 32 (RPB = 16)
template <int WIDE> static void check_map() {
    constexpr int NI = WIDE ? 32 : 16, NBLK = WIDE ? 2 : 4, NR = WIDE ? 32 : 16, NC = NBLK * NI * NI;
    std::vector<_Float16> ha(256), hb(256); std::vector<float> hd(64 * NR);
    _Float16 * da, * db; float * dd; hipMalloc(&da, 512); hipMalloc(&db, 512); hipMalloc(&dd, 64 * NR * 4);
    std::vector<char> alive((size_t) 64 * NR * NC, 1);
    int bad = 0;
    for (int trial = 0; trial < 6; ++trial) {
        srand(17 + trial);
        for (int i = 0; i < 256; ++i) { ha[i] = (_Float16) (float) (rand() % 255 - 127); hb[i] = (_Float16) (float) (rand() % 255 - 127); }
        hipMemcpy(da, ha.data(), 512, hipMemcpyHostToDevice); hipMemcpy(db, hb.data(), 512, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(map_kernel<WIDE>, dim3(1), dim3(64), 0, 0, da, db, dd);
        hipMemcpy(hd.data(), dd, 64 * NR * 4, hipMemcpyDeviceToHost);
        auto ref = [&](int blk, int i, int j) { float s = 0; for (int k = 0; k < 4; ++k) s += (float) ha[(blk * NI + i) * 4 + k] * (float) hb[(blk * NI + j) * 4 + k]; return s; };
        for (int l = 0; l < 64; ++l) for (int v = 0; v < NR; ++v) {
            const float got = hd[l * NR + v];
            const int blk = WIDE ? v >> 4 : v >> 2, i = WIDE ? 8 * ((v & 15) >> 2) + 4 * (l >> 5) + (v & 3) : 4 * (l >> 4) + (v & 3), j = l % NI;
            if (got != ref(blk, i, j)) ++bad;
            for (int c = 0; c < NC; ++c) if (alive[(size_t) (l * NR + v) * NC + c] && ref(c / (NI * NI), (c / NI) % NI, c % NI) != got) alive[(size_t) (l * NR + v) * NC + c] = 0;
        }
    }
    printf("lane map of %s (A / B lane = %d block + row / column, four k per lane; D register v: block v / %d, column lane %% %d): %s\n",
           WIDE ? "v_mfma_f32_32x32x4_2b_f16" : "v_mfma_f32_16x16x4_4b_f16", NI, WIDE ? 16 : 4, NI, bad ? "DOES NOT HOLD" : "holds on six sets of exact integer data");
    if (bad) {
        for (int l : { 0, 1, 15, 16, 31, 32, 63 }) for (int v : { 0, 1, 3, 4, 15 }) {
            printf("  lane %2d reg %2d:", l, v);
            int n = 0; for (int c = 0; c < NC && n < 4; ++c) if (alive[(size_t) (l * NR + v) * NC + c]) { printf(" (block %d, i %d, j %d)", c / (NI * NI), (c / NI) % NI, c % NI); ++n; }
            printf("\n");
        }
    }
}

int main() {
    hipDeviceProp_t p; hipGetDeviceProperties(&p, 0);
    const int ncu = p.multiProcessorCount;
    check_map<0>();
    check_map<1>();
    float * out, * dsrc; hipMalloc(&out, (size_t) ncu * 256 * 4); hipMalloc(&dsrc, 64);
    std::vector<float> h(16); for (int i = 0; i < 16; ++i) h[i] = 1.0f + i * 0.125f;
    hipMemcpy(dsrc, h.data(), 64, hipMemcpyHostToDevice);
    printf("cycles per MFMA per SIMD (2.4 GHz assumed), %d CUs, one wave per SIMD; chain FMAs are on the previous MFMA's results\n", ncu);
    run<2, 0, false, false>("v_mfma_f32_16x16x4_4b_f16 (4096 MAC) back to back, two accumulators", out, dsrc, ncu);
    run<0, 0, false, false>("v_mfma_f32_32x32x4_2b_f16 (8192 MAC) back to back", out, dsrc, ncu);
    run<1, 0, false, false>("v_mfma_i32_32x32x4_2b_i8  (8192 MAC) back to back", out, dsrc, ncu);
    run<2, 16, false, false>("16x16x4_4b_f16 (C = 0) + 16 v_fma_f32 (every result chained)", out, dsrc, ncu);
    run<2, 32, false, false>("16x16x4_4b_f16 (C = 0) + 32 v_fma_f32", out, dsrc, ncu);
    run<2, 16, true, false>("16x16x4_4b_f16 (C = 0) +  8 v_pk_fma_f32 (every result chained: the kernel's ratio)", out, dsrc, ncu);
    run<2, 32, true, false>("16x16x4_4b_f16 (C = 0) + 16 v_pk_fma_f32", out, dsrc, ncu);
    run<2, 64, true, false>("16x16x4_4b_f16 (C = 0) + 32 v_pk_fma_f32", out, dsrc, ncu);
    run<2, 16, true, true>("16x16x4_4b_f16 (C = 0) +  8 v_pk_fma_f32 + A, B (ds_read_b64) and scales from LDS", out, dsrc, ncu);
    run<0, 32, true, false>("32x32x4_2b_f16 (C = 0) + 16 v_pk_fma_f32 (every result chained)", out, dsrc, ncu);
    run<1, 32, true, false>("32x32x4_2b_i8  (C = 0) + 32 v_cvt_f32_i32 + 16 v_pk_fma_f32", out, dsrc, ncu);
    return 0;
}
