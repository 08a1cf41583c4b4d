// Context-folded cross-attention (fd_gemm_desc.softmax_group, include/flexdiffuse_hip.h): the once-per-context helper beside the two GEMM
// launches -- the folded operands themselves are small batched fd_gemm_f16 launches (ops.xattn_fold).
#include "common.h"

// ---- context-folded cross-attention (fd_gemm_desc.softmax_group): the two fp32 rows per sample beside the folded keys ----------------
// One wave per (sample, folded key row n = h * 80 + l): the sum of the row's C fp16 values (the LayerNorm fold's colsum) and the dot
// product of the folded q bias with the cached key (the fold's bias); lane partials in a fixed order, then a butterfly over the wave.
__global__ __launch_bounds__(256) void k_xattn_fold_rows(const half_t* __restrict__ kf, const half_t* __restrict__ K, const float* __restrict__ bq,
                                                         float* __restrict__ rows, int total, int n_keys, int heads, int dh, int C, int ldk) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total) return;
    const int N = heads * 80, s = row / N, n = row - s * N, h = n / 80, l = n - h * 80;
    const half_t* src = kf + (size_t)row * C;
    float cs = 0.f;
    for (int c = lane * 8; c < C; c += 512) {
        const half8 v = *reinterpret_cast<const half8*>(src + c);
#pragma unroll
        for (int k = 0; k < 8; ++k) cs += (float)v[k];
    }
    float bs = 0.f;
    if (l < n_keys) {
        const half_t* kr = K + ((size_t)s * n_keys + l) * ldk + h * dh;
        for (int j = lane; j < dh; j += 64) bs = fmaf(bq[h * dh + j], (float)kr[j], bs);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        cs += __shfl_xor(cs, o, 64);
        bs += __shfl_xor(bs, o, 64);
    }
    if (lane == 0) {
        rows[(size_t)s * 2 * N + n] = cs;
        rows[(size_t)s * 2 * N + N + n] = bs;
    }
}

extern "C" int fd_xattn_fold_rows_f32(const void* kf, const void* K, const float* bias_q, float* rows, int samples, int n_keys, int heads,
                                      int head_dim, int C, int ldk, void* stream) {
    FD_PLAN(fd_xattn_fold_rows_f32(kf, K, bias_q, rows, samples, n_keys, heads, head_dim, C, ldk, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(4u, __LINE__));
    FD_CHECK_ARG(kf && K && bias_q && rows && samples > 0 && heads > 0, FD_EINVAL, "fd_xattn_fold_rows_f32: args");
    FD_CHECK_ARG(n_keys >= 1 && n_keys <= 80 && head_dim > 0 && head_dim % 8 == 0 && C > 0 && C % 8 == 0 && ldk >= heads * head_dim &&
                     (uintptr_t)kf % 16 == 0 && (long long)samples * heads * 80 < (1ll << 30),
                 FD_ESHAPE, "fd_xattn_fold_rows_f32: 1..80 keys, head_dim %% 8 == 0, C %% 8 == 0, ldk >= heads * head_dim, kf 16-byte aligned (got %d keys, %d x %d, C %d, ldk %d)",
                 n_keys, heads, head_dim, C, ldk);
    const int total = samples * heads * 80;
    hipLaunchKernelGGL(k_xattn_fold_rows, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const half_t*)kf, (const half_t*)K, bias_q, rows,
                       total, n_keys, heads, head_dim, C, ldk);
    FD_CHECK_LAUNCH("k_xattn_fold_rows");
    return FD_OK;
}
