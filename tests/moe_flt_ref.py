"""F16 / F32 / BF16 EXPERT matrices: a numpy restatement of what ggml_compute_forward_mul_mat_id (ggml.c:12494) computes for a row of one.

It never calls llamafile_sgemm: the activations go through from_float of the type's vec_dot_type and each output is the type's vec_dot of a whole row.
  F16   x rounded to f16 (ggml_fp32_to_fp16_row, F16C: nearest even, overflow to inf, subnormals kept); ggml_vec_dot_f16 (ggml.c:2038): four 8-lane f32
        accumulators, lane j of accumulator a takes k = 32i + 8a + j, one fma per step; GGML_F32x8_REDUCE: (s0 + s2) + (s1 + s3), lo + hi halves, two hadd_ps,
        i.e. (t0 + t1) + (t2 + t3) — not the (t0 + t2) + (t1 + t3) of the sgemm hsum
  F32   x as it is; ggml_vec_dot_f32 (ggml.c:1931): the same 4 x 8 fma structure and the same reduce
  BF16  float_ref.vec_dot_bf16_rows, unchanged
Held to the genuine reference's answers in tests/golden/moe_flt_kats.npz (tests/golden/gen_moe_flt_kats.py, tests/test_moe_flt_ref.py)."""
import numpy as np

from float_ref import BF16, ESIZE, F16, F32, bf16_bits, to_f32, vec_dot_bf16_rows
from lowbit_ref import fma32


def act(t, x):
    """from_float of the type's vec_dot_type: what the dot reads, widened back to f32 (BF16: the uint16 bits)"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(all="ignore"):
        return x if t == F32 else x.astype(np.float16).astype(np.float32) if t == F16 else bf16_bits(x)


def vec_dot_rows(w, x):
    """ggml_vec_dot_f16 / ggml_vec_dot_f32, AVX2: w f32 [rows][K], x f32 [K] (both already widened) -> f32 [rows]"""
    rows, K = w.shape
    acc = np.zeros((rows, 4, 8), np.float32)
    with np.errstate(all="ignore"):
        for i in range(K // 32):
            acc = fma32(w[:, 32 * i:32 * i + 32].reshape(rows, 4, 8), x[32 * i:32 * i + 32].reshape(1, 4, 8), acc)
        s = (acc[:, 0] + acc[:, 2]) + (acc[:, 1] + acc[:, 3])
        t = s[:, 0:4] + s[:, 4:8]
        return ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])).astype(np.float32)


def mul_mat_id_rows(t, raw, rows, K, x, chunk=2048):
    """y = W . x for ONE expert matrix of type t as mul_mat_id computes it (x: the f32 activation row)"""
    w = to_f32(t, np.asarray(raw, np.uint8)[:rows * K * ESIZE[t]]).reshape(rows, K)
    a = act(t, x)
    dot = vec_dot_bf16_rows if t == BF16 else vec_dot_rows
    return np.concatenate([dot(w[r:r + chunk], a) for r in range(0, rows, chunk)])
