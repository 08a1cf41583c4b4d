// Launch forms of the CONTEXT-FOLDED cross-attention (fd_gemm_desc.softmax_group; include/flexdiffuse_hip.h), part of gemm.hip's translation
// unit (included behind launch_mode / launch_epi):
//   launch 1  P = softmax_per_head(LN-fold(h) K'[b])   -- k_gemm_f16_dma with EPI 14 (gemm_epilogue_softmax) on a 64x160 or 128x160 tile,
//                                                        3 LDS stages, 32x80 wave tiles: one wave column = one head of 80 keys;
//   launch 2  out = P V'[b] + bo + residual             -- the ordinary statistics + residual epilogue (EPI 8 / 9); only the 8x8 map with
//                                                        per-sample weights (64 rows per launch slice) needs a tile of its own, 64x160.
// tests/test_gpu_xattn_fold.py holds their reference tests.
#pragma once


// Everything the softmax form cannot run is refused here -- the caller asks fd_gemm_plan first and keeps its unfolded launches for a refused shape
static int xfold_check(const fd_gemm_desc* d, GemmArgs& g, int batch) {
    FD_CHECK_ARG(d->ln_stats && !d->conv && !d->trans_out && d->act == FD_ACT_NONE && !d->residual && !d->out_f32 && !d->K2 && !d->ln_stats_out &&
                     !d->gn_out && !d->gn_part_out && !d->trans_n0 && !d->residual_rows && d->split_k <= 1,
                 FD_EINVAL, "fd_gemm_f16: softmax_group needs a plain LayerNorm-fold linear GEMM (ln_stats; act NONE, fp16 output, no residual / appended operand / "
                            "statistics or GroupNorm output / transposed store / split-K)");
    FD_CHECK_ARG(d->softmax_group == 80 && d->softmax_valid >= 1 && d->softmax_valid <= 80, FD_ESHAPE,
                 "fd_gemm_f16: softmax_group must be 80 with 1 <= softmax_valid <= 80 keys (got group %d, %d keys)", d->softmax_group, d->softmax_valid);
    FD_CHECK_ARG(d->N % 160 == 0 && (d->ldc & 7) == 0, FD_ESHAPE, "fd_gemm_f16: softmax_group needs N %% 160 == 0 (two heads per tile) and ldc %% 8 == 0");
    // (the rows of one launch slice -- one sample with per-sample weights -- must be whole tiles: no tile of two samples' rows)
    FD_CHECK_ARG(d->M % 64 == 0, FD_ESHAPE, "fd_gemm_f16: softmax_group: M=%d rows per launch slice is not a multiple of the 64-row tile (a tile would straddle two samples)", d->M);
    FD_CHECK_ARG(batch == 1 || (d->bias && d->batch_stride_c == (int64_t)d->M * d->ldc), FD_ESHAPE,
                 "fd_gemm_f16: softmax_group with batch > 1 needs a bias and batch_stride_c == M * ldc");
    const GemmExtents ext = gemm_extents(g, false);
    FD_CHECK_ARG(ext.dma_ok() && GemmExtents::below_2gib(ext.c), FD_ESHAPE, "fd_gemm_f16: softmax_group: operands >= 2 GiB");
    FD_CHECK_ARG(gemm_lean_dma_path(), FD_ESHAPE, "fd_gemm_f16: softmax_group needs the LDS-DMA path with the lean epilogue and LDS-staged biases");
    FD_CHECK_ARG(d->tile == 0 || d->tile == 24 || (d->tile == 25 && d->M % 128 == 0), FD_ESHAPE,
                 "fd_gemm_f16: softmax_group runs on tile 24 (64x160) or 25 (128x160, M %% 128 == 0), not %d", d->tile);
    g.sm_valid = d->softmax_valid;
    return FD_OK;
}

// 24: 64 x 160, 4 waves; 25: 128 x 160, 8 waves (both 32x80 wave tiles, 3 LDS stages).  The 128-row tile from 128 workgroups on: at the 16x16 level
// of the bench forward (16 x 256 rows, 128 against 256 workgroups) it takes 19.8 us against 22.5 us (tools/ab_xattn_fold.py)
static int xfold_rule(const fd_gemm_desc* d, int batch) {
    return d->tile ? d->tile : ((d->M % 128 == 0 && (long long)(d->M / 128) * (d->N / 160) * batch >= 128) ? 25 : 24);
}

static int xfold_launch_probs(GemmArgs& g, int batch, int stile, hipStream_t st2) {
    return stile == 25 ? launch_mode<128, 160, false, false, 4, 3, 2, 14>(g, batch, st2) : launch_mode<64, 160, false, false, 2, 3, 2, 14>(g, batch, st2);
}

// tile 26: 64 x 160, 4 waves, 32x80 wave tiles, statistics (+ residual) epilogue only (fd_stats_plan picks it for batched launches of 64 rows)
static int xfold_launch_out64(GemmArgs& g, int batch, hipStream_t st) { return launch_epi<64, 160, 2, 2, 2, 256>(g, batch, st); }
