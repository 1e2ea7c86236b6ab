// bamd_moe_batch_xs_mfma.hip — the IQ4_XS instances of the grouped eight-wave matrix-core kernel (bamd_moe_batch_kq_mfma.h; the design: bamd_moe_batch_kq_mfma.hip's
// head), reached through bamd_launch_moe_mma_kq.  A translation unit of its own because it is built without packed-f32 instructions, as the dense IQ4_XS kernel
// of bamd_prefill2_xs.hip is (booster_amd/build.py: NO_PACKED_F32); the Q3_K / Q2_K instances keep the flags of bamd_prefill2.hip.
#include "bamd_prefill2_xs.h"
#include "bamd_moe_batch_kq_mfma.h"
#include "bamd_kernels.h"

void bamd_launch_moe_mma_xs(const bamd_moe_mma_args & a, int mode, int tile_bound, hipStream_t s) { moe_mfma2_launch<X2IQ4XS>(a, mode, tile_bound, s); }
int bamd_moe_mma_xs_supported(void) { return moe_mfma2_supported<X2IQ4XS>(); }
