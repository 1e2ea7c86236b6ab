"""CPU: the slice plan of a micro-batch's attention (bamd_attention_batch_plan) with set_attn_mfma_ext on — head_dim 64 and the ratios 3 / 5 / 6 / 7 in
matrix-core tiles of 16 // gq tokens, 16 scratch columns per workgroup beyond 512 positions — and the same call with it off again.  No device is opened."""
import os

import pytest

import booster_amd


@pytest.mark.parametrize("args,want", [
    ((2, 3, 128, 37, 1024, 2), (40, 1, 2 * 8 * 16 * 1024 * 4)),       # gq 3: eight tiles of 5 tokens
    ((1, 4, 64, 37, 576, 2), (40, 1, 10 * 16 * 576 * 4)),             # head_dim 64, gq 4: ten tiles of 4 tokens
    ((1, 7, 64, 5, 512, 2), (6, 1, 0)),                               # up to 512 positions the rows are in LDS: no block
    ((2, 3, 128, 37, 512, 0), (40, 1, 0)),
    ((2, 3, 192, 37, 1024, 2), None),                                 # head_dim 192 / 256 stay on the VALU
    ((2, 4, 256, 37, 1024, 2), None),
])
def test_plan_with_the_switch_on(args, want):
    from booster_amd import build
    build.build()
    booster_amd.set_attn_mfma_ext(True)
    try:
        assert booster_amd.attention_batch_plan(*args) == want
    finally:
        booster_amd.set_attn_mfma_ext(os.environ.get("BAMD_ATTN_MFMA_EXT", "")[:1] == "1")
    if os.environ.get("BAMD_ATTN_MFMA_EXT", "")[:1] != "1":
        assert booster_amd.attention_batch_plan(2, 3, 128, 37, 1024, 2) is None
