// Host-side entry points of csrc/rank16_mfma.hip for the C-ABI functions of linear.hip / linear_fused.hip: each returns
// true when it took the launch (bf16 activations, f32 factor, aligned rows, hook enabled; rank 9..64 for the row product,
// the rank update and the column reduction, 9..16 for bwd_g), false when the caller's VALU kernel has to run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lora_amd {

extern int g_r16_mfma;
extern int g_cr_mfma;   // lora_amd_colreduce_mfma: the column reduction's own switch, ANDed with g_r16_mfma

// The predicate r16_rowdot (op 0, cols = C), r16_rank_update (op 1, cols = N) and r16_colreduce (op 2, cols = K) decide by;
// lora_amd_rank16_mfma_takes exposes ops 0 and 1, lora_amd_colreduce_mfma_takes op 2, lora_amd_rank_update_rowscale_mfma_takes
// op 1 for the row-table form.
bool r16_takes(int op, const void *rows, int64_t ld, int64_t M, int cols, int r, int act_dtype, int fdt, bool has_sel);
bool r16_rowdot(const void *x, int64_t ldx, const void *f, int fdt, int layout, float *t_out, int64_t M, int C, int r,
                int act_dtype, float scale, float p, uint64_t seed, uint64_t offset, const uint64_t *offset_dev, hipStream_t st,
                bool has_sel = false);
// row_scale != nullptr: the row-table form (lora_amd_rank_update_rowscale): row m's T row times
// row_scale[((m / rps) % nsel) * r + j] as it is staged; same predicate, same geometry.
bool r16_rank_update(void *y, int64_t ldy, const float *t, int nparts, int64_t part_stride, const void *f, int fdt, int layout,
                     int64_t M, int N, int r, int act_dtype, float scale, float p, uint64_t seed, uint64_t offset,
                     const uint64_t *offset_dev, hipStream_t st, const float *row_scale = nullptr, int nsel = 1,
                     int64_t rps = 1);
// colreduce (op 2, cols = K): launches stage 1; *fold_blocks row-block partials [fold_blocks][r][K] at the head of
// `workspace` are left for the caller's colreduce_stage2_kernel (beta = 1, scale = 1) to add to D; 0: D is complete.
bool r16_colreduce(const void *x, int64_t ldx, const float *t, float *d, int64_t M, int K, int r, int act_dtype, int out_layout,
                   float scale, float beta, float p, uint64_t seed, uint64_t offset, const uint64_t *offset_dev, void *workspace,
                   size_t workspace_bytes, hipStream_t st, int64_t *fold_blocks);
bool r16_bwd_g(const void *g, int64_t ldg, const float *t, const void *up, int fdt, float *gt_part, float *up_part, int64_t M,
               int N, int r, int log_ct8, int nct, int rows_per_block, int64_t nrb, int act_dtype, float scale, float p,
               uint64_t seed, uint64_t offset, const uint64_t *offset_dev, hipStream_t st, float *gt_out = nullptr,
               unsigned *counters = nullptr);

}  // namespace lora_amd
