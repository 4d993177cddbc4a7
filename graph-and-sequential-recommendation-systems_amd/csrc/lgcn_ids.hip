// lgcn_ids.hip -- the fused step called the way the reference calls it: BPRLoss.stageOne(users, pos, neg) with torch.long (int64) id
// tensors (main.py:217-225, utils.py:53-64).  The kernels of the step read int32 ids; converting the three tensors in the caller
// costs three launches and three allocations per step (measured: 6 208 vs 6 598 steps/s on Gowalla).  Here ONE launch narrows all
// three into a caller-owned scratch buffer and the step follows on the same stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgcn_hip.h"
#include "lgcn_internal.h"

// an id outside int32 becomes -1: the step flags it (cfg.err) and voids its triplet, as it does any out-of-range id
__global__ void __launch_bounds__(256) k_ids_to_i32(const int64_t *u, const int64_t *p, const int64_t *n, int32_t B, int32_t *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 3 * B) return;
    const int c = i / B, b = i - c * B;
    const int64_t v = (c == 0 ? u : c == 1 ? p : n)[b];
    out[i] = (v < 0 || v > 0x7fffffffLL) ? -1 : (int32_t)v;
}

extern "C" int lgcn_train_step_i64(lgcn_ctx *ctx, const int64_t *users, const int64_t *pos, const int64_t *neg, int32_t B,
                                   int32_t *ids_scratch, float *loss_out, void *stream) {
    if (!ctx || !users || !pos || !neg || !ids_scratch || B <= 0) { lgcn_set_error("lgcn_train_step_i64: invalid argument"); return 3; }
    if (int rc = lgcn_refuse_loss(ctx, "lgcn_train_step_i64")) return rc;       // refused before the scratch buffer is written
    hipLaunchKernelGGL(k_ids_to_i32, dim3((unsigned)((3 * (int64_t)B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, users, pos, neg, B, ids_scratch);
    return lgcn_train_step(ctx, ids_scratch, ids_scratch + B, ids_scratch + 2 * (int64_t)B, B, loss_out, stream);
}
