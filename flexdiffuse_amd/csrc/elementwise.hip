// Small HBM-bound kernels around the MFMA path: layout conversion between the pipeline's
// NCHW fp32 latents and the kernels' NHWC fp16 activations, im2col for the few convs whose
// input-channel count is below one K tile (conv_in 4ch, VAE conv_in, CLIP patch embed),
// channel concat for the UNet skip connections, CLIP token/position embedding gathers, the
// sinusoidal timestep embedding and the CompositeGuide region blend.  (The fused
// classifier-free-guidance + scheduler update of the latents is step.hip.)
#include "latent_step.h"

// ---- NCHW fp32 -> NHWC fp16 (optionally replicated `rep` times along batch: CFG) ---------
// y = half_rn(x * scale): ONE fp32 product, ONE rounding to half.  The product is kept an fp32 value of its own (the empty asm): the
// compiler otherwise folds product and conversion into v_fma_mixlo_f16 (x * scale + 0), whose +0 addend turns a product of -0 into +0.
__device__ __forceinline__ half_t fd_scale_to_half(float x, float scale) {
    float p = x * scale;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    return (half_t)p;
}

__global__ void k_nchw_to_nhwc(const float* __restrict__ x, half_t* __restrict__ y, int B, int C,
                               int HW, int rep, int Cpad, float scale) {
    const size_t total = (size_t)B * HW * Cpad;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int c = e % Cpad;
        const size_t r = e / Cpad;
        const int p = r % HW;
        const int b = r / HW;
        const half_t v = c < C ? fd_scale_to_half(x[((size_t)b * C + c) * HW + p], scale) : (half_t)0.f;
        for (int k = 0; k < rep; ++k) y[((size_t)(k * B + b) * HW + p) * Cpad + c] = v;
    }
}

extern "C" int fd_nchw_f32_to_nhwc_f16(const float* x, void* y, int B, int C, int HW, int rep,
                                       int c_pad, float scale, void* stream) {
    FD_PLAN(fd_nchw_f32_to_nhwc_f16(x, y, B, C, HW, rep, c_pad, scale, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && y && B > 0 && C > 0 && HW > 0 && rep > 0 && c_pad >= C, FD_EINVAL,
                 "fd_nchw_f32_to_nhwc_f16: args");
    const size_t total = (size_t)B * HW * c_pad;
    const int blocks = fd_grid1d(total, 4096);
    hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x,
                       (half_t*)y, B, C, HW, rep, c_pad, scale);
    FD_CHECK_LAUNCH("k_nchw_to_nhwc");
    return FD_OK;
}

// ---- 3x3 / stride 1 / pad 1 convolution of a NARROW input (<= 4 channels) read from the fp32 NCHW tensor: the UNet's conv_in ---------------
// (4 latent channels -> 320).  As a GEMM the layer is 0.75 GFLOP behind three memory passes (layout change, explicit im2col with K padded
// 36 -> 128, a 64x64-tile GEMM) and, under CFG, a fourth that replicates the output for the decoder's skip connection.  Here one workgroup
// makes one output row of one sample: the 3 x (W + 2) x 4 input strip (fp16, as fd_nchw_f32_to_nhwc_f16 rounds it) in LDS, a thread's
// 8 output channels' 36 taps in registers as fp16 pairs, v_dot2_f32_f16 products (exact fp16 x fp16, fp32 accumulation -- the MFMA path's
// arithmetic in another summation order), 16-byte NHWC stores to the output and to its replicas.  HBM-write-bound: 21 MB per copy.
template <int CPT>   // output channels per thread (8: one 16-byte store)
__global__ __launch_bounds__(256) void k_conv3x3_narrow(const float* __restrict__ x, const half_t* __restrict__ w, const float* __restrict__ bias,
                                                        half_t* __restrict__ y, int ldy, half_t* __restrict__ y2, int ldy2, int rep2,
                                                        int B, int Cin, int H, int W, int Cout, float scale) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char sm_c3[];
    half_t* xs = reinterpret_cast<half_t*>(sm_c3);          // [3][W + 2][4]
    const int row = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int WP = W + 2;
    for (int i = tid; i < 3 * WP * 4; i += 256) {
        const int ci = i & 3, col = (i >> 2) % WP, r = (i >> 2) / WP;
        const int yy = row + r - 1, xx = col - 1;
        float v = 0.f;
        if (ci < Cin && yy >= 0 && yy < H && xx >= 0 && xx < W) v = x[((size_t)(b * Cin + ci) * H + yy) * W + xx] * scale;
        xs[i] = (half_t)v;
    }
    const int nchunk = Cout / CPT, npg = 256 / nchunk;       // pixel groups that fit the workgroup
    const int c = tid % nchunk, pg = tid / nchunk;
    const bool live = pg < npg;
    // this thread's weights: CPT channels x 36 taps, (ky, kx, ci) order = the order of a pixel's 3 x 12 strip values
    half2v wr[CPT][18];
    float bs[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int co = c * CPT + k;
        const half2v* src = reinterpret_cast<const half2v*>(w + (size_t)(live ? co : 0) * 36);
#pragma unroll
        for (int t = 0; t < 18; ++t) wr[k][t] = src[t];
        bs[k] = bias ? bias[live ? co : 0] : 0.f;
    }
    __syncthreads();
    if (!live) return;
    const size_t rowbase = ((size_t)b * H + row) * W;
    for (int p = pg; p < W; p += npg) {
        half2v xv[18];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const half2v* src = reinterpret_cast<const half2v*>(xs + ((size_t)r * WP + p) * 4);   // 12 consecutive values: columns p .. p+2, 4 channels
#pragma unroll
            for (int t = 0; t < 6; ++t) xv[r * 6 + t] = src[t];
        }
        typedef half_t halfN __attribute__((ext_vector_type(CPT)));
        halfN o;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            float acc = bs[k];
#pragma unroll
            for (int t = 0; t < 18; ++t) acc = __builtin_amdgcn_fdot2(xv[t], wr[k][t], acc, false);
            o[k] = (half_t)acc;
        }
        *reinterpret_cast<halfN*>(y + (rowbase + p) * ldy + c * CPT) = o;
        for (int r = 0; r < rep2; ++r)
            *reinterpret_cast<halfN*>(y2 + ((size_t)r * B * H * W + rowbase + p) * ldy2 + c * CPT) = o;
    }
#endif
}

extern "C" int fd_conv3x3_narrow_f16(const float* x, const void* w, const float* bias, void* y, int ldy, void* y2, int ldy2, int rep2,
                                     int B, int Cin, int H, int W, int Cout, float scale, void* stream) {
    FD_PLAN(fd_conv3x3_narrow_f16(x, w, bias, y, ldy, y2, ldy2, rep2, B, Cin, H, W, Cout, scale, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && w && y && B > 0 && H > 0 && W > 0 && rep2 >= 0 && (rep2 == 0 || y2), FD_EINVAL, "fd_conv3x3_narrow_f16: args");
    FD_CHECK_ARG(Cin >= 1 && Cin <= 4 && Cout % 8 == 0 && Cout >= 8 && Cout <= 2048 && 256 / (Cout / 8) >= 1 && W <= 1024 && B <= 65535, FD_ESHAPE,
                 "fd_conv3x3_narrow_f16: Cin=%d (<= 4), Cout=%d (a multiple of 8, <= 2048), W=%d (<= 1024)", Cin, Cout, W);
    FD_CHECK_ARG(ldy >= Cout && ldy % 8 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)w % 4 == 0 &&
                     (rep2 == 0 || (ldy2 >= Cout && ldy2 % 8 == 0 && (uintptr_t)y2 % 16 == 0)), FD_ESHAPE,
                 "fd_conv3x3_narrow_f16: row strides must be multiples of 8 and >= Cout, outputs 16-byte aligned");
    const size_t lds = (size_t)3 * (W + 2) * 4 * sizeof(half_t);
    hipLaunchKernelGGL((k_conv3x3_narrow<8>), dim3(H, B), dim3(256), lds, (hipStream_t)stream, x, (const half_t*)w, bias, (half_t*)y, ldy,
                       (half_t*)y2, ldy2, rep2, B, Cin, H, W, Cout, scale);
    FD_CHECK_LAUNCH("k_conv3x3_narrow");
    return FD_OK;
}

// ---- NHWC fp32 [B][HW][ld] -> NCHW fp32 [B][C][HW]: y = clamp(x*a + b) -------------------
__global__ void k_nhwc_to_nchw(const float* __restrict__ x, float* __restrict__ y, int B, int C,
                               int HW, int ld, float a, float bofs, int clamp01) {
    const size_t total = (size_t)B * C * HW;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int p = e % HW;
        const size_t r = e / HW;
        const int c = r % C;
        const int b = r / C;
        float v = x[((size_t)b * HW + p) * ld + c] * a + bofs;
        if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
        y[e] = v;
    }
}

extern "C" int fd_nhwc_f32_to_nchw_f32(const float* x, float* y, int B, int C, int HW, int ld,
                                       float a, float b, int clamp01, void* stream) {
    FD_PLAN(fd_nhwc_f32_to_nchw_f32(x, y, B, C, HW, ld, a, b, clamp01, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && y && B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL,
                 "fd_nhwc_f32_to_nchw_f32: args");
    const size_t total = (size_t)B * C * HW;
    const int blocks = fd_grid1d(total, 4096);
    hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, B, C,
                       HW, ld, a, b, clamp01);
    FD_CHECK_LAUNCH("k_nhwc_to_nchw");
    return FD_OK;
}

// ---- im2col (NHWC fp16) for convs with Cin < 64: out[m][k], k=(kh*KW+kw)*Cin+ci, zero pad --
__global__ void k_im2col(const half_t* __restrict__ x, half_t* __restrict__ y, int B, int Hi, int Wi,
                         int Cin, int Ho, int Wo, int KH, int KW, int stride, int pad_t, int pad_l,
                         int Kpad) {
    const size_t total = (size_t)B * Ho * Wo * Kpad;
    const int K = KH * KW * Cin;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int k = e % Kpad;
        const size_t m = e / Kpad;
        half_t v = (half_t)0.f;
        if (k < K) {
            const int ci = k % Cin, tap = k / Cin;
            const int kh = tap / KW, kw = tap % KW;
            const int ox = m % Wo;
            const size_t r = m / Wo;
            const int oy = r % Ho;
            const int b = r / Ho;
            const int iy = oy * stride + kh - pad_t, ix = ox * stride + kw - pad_l;
            if (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi)
                v = x[(((size_t)b * Hi + iy) * Wi + ix) * Cin + ci];
        }
        y[e] = v;
    }
}

extern "C" int fd_im2col_f16(const void* x, void* y, int B, int Hi, int Wi, int Cin, int Ho,
                             int Wo, int KH, int KW, int stride, int pad_t, int pad_l, int k_pad,
                             void* stream) {
    FD_PLAN(fd_im2col_f16(x, y, B, Hi, Wi, Cin, Ho, Wo, KH, KW, stride, pad_t, pad_l, k_pad, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && y && B > 0 && Hi > 0 && Wi > 0 && Cin > 0 && Ho > 0 && Wo > 0, FD_EINVAL,
                 "fd_im2col_f16: args");
    FD_CHECK_ARG(KH > 0 && KW > 0 && stride > 0 && pad_t >= 0 && pad_l >= 0, FD_EINVAL,
                 "fd_im2col_f16: KH=%d, KW=%d, stride=%d must be positive, pad=(%d, %d) non-negative", KH, KW, stride, pad_t, pad_l);
    FD_CHECK_ARG(k_pad >= 8 && k_pad % 8 == 0 && (int64_t)KH * KW * Cin <= k_pad, FD_ESHAPE, "fd_im2col_f16: k_pad");
    const size_t total = (size_t)B * Ho * Wo * k_pad;
    const int blocks = fd_grid1d(total, 8192);
    hipLaunchKernelGGL(k_im2col, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x,
                       (half_t*)y, B, Hi, Wi, Cin, Ho, Wo, KH, KW, stride, pad_t, pad_l, k_pad);
    FD_CHECK_LAUNCH("k_im2col");
    return FD_OK;
}

// ---- channel concat of two row-major fp16 matrices: out[m] = [a[m] | b[m]] ---------------
__global__ void k_concat(const uint4* __restrict__ a, const uint4* __restrict__ b,
                         uint4* __restrict__ out, size_t M, int ca8, int cb8) {
    const int ct = ca8 + cb8;
    const size_t total = M * ct;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int c = e % ct;
        const size_t m = e / ct;
        out[e] = c < ca8 ? a[m * ca8 + c] : b[m * cb8 + (c - ca8)];
    }
}

extern "C" int fd_concat_channels_f16(const void* a, const void* b, void* out, int64_t M, int Ca,
                                      int Cb, void* stream) {
    FD_PLAN(fd_concat_channels_f16(a, b, out, M, Ca, Cb, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(a && b && out && M > 0, FD_EINVAL, "fd_concat_channels_f16: args");
    FD_CHECK_ARG(Ca >= 0 && Cb >= 0 && (int64_t)Ca + Cb > 0, FD_EINVAL, "fd_concat_channels_f16: Ca=%d, Cb=%d (>= 0, not both 0)", Ca, Cb);
    FD_CHECK_ARG(Ca % 8 == 0 && Cb % 8 == 0, FD_ESHAPE, "fd_concat_channels_f16: C %% 8");
    FD_CHECK_ARG(((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) % 16 == 0, FD_ESHAPE,
                 "fd_concat_channels_f16: the pointers must be 16-byte aligned");
    const size_t total = (size_t)M * ((size_t)(Ca + Cb) / 8);
    const int blocks = fd_grid1d(total, 8192);
    hipLaunchKernelGGL(k_concat, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)a,
                       (const uint4*)b, (uint4*)out, (size_t)M, Ca / 8, Cb / 8);
    FD_CHECK_LAUNCH("k_concat");
    return FD_OK;
}

// ---- strided 2-D copy of fp16 rows (16-byte granules): dst[r][0..cols) = src[r][0..cols) ---------
// The CFG fan-out of the shared UNet prefix (B samples -> rep*B) and the skip tensors copied into
// their concat buffers; a library launch (not a torch op) so that a launch plan records it.
__global__ void k_copy2d(const uint4* __restrict__ src, size_t lds8, uint4* __restrict__ dst, size_t ldd8,
                         size_t rows, int cols8) {
    const size_t total = rows * cols8;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (size_t)gridDim.x * blockDim.x) {
        const int c = e % cols8;
        const size_t r = e / cols8;
        dst[r * ldd8 + c] = src[r * lds8 + c];
    }
}

// dst[r * rows + i][0..cols) = src[i][0..cols) for r < rep: the CFG fan-out (B samples -> rep * B) in ONE launch -- every source granule
// is read once and stored rep times (round 6: three launches and three boundaries less per forward than rep separate copies)
__global__ void k_repeat_rows(const uint4* __restrict__ src, size_t lds8, uint4* __restrict__ dst, size_t ldd8, size_t rows, int cols8, int rep) {
    const size_t total = rows * cols8;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = e % cols8;
        const size_t r = e / cols8;
        const uint4 v = src[r * lds8 + c];
        for (int k = 0; k < rep; ++k) dst[((size_t)k * rows + r) * ldd8 + c] = v;
    }
}

extern "C" int fd_repeat_rows_f16(const void* src, int lds, void* dst, int ldd, int64_t rows, int cols, int rep, void* stream) {
    FD_PLAN(fd_repeat_rows_f16(src, lds, dst, ldd, rows, cols, rep, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(src && dst && rows > 0 && cols > 0 && rep >= 1 && lds >= cols && ldd >= cols, FD_EINVAL, "fd_repeat_rows_f16: args");
    FD_CHECK_ARG(cols % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0, FD_ESHAPE,
                 "fd_repeat_rows_f16: cols / strides must be multiples of 8 and the pointers 16-byte aligned");
    const size_t total = (size_t)rows * (cols / 8);
    const int blocks = fd_grid1d(total, 8192);
    hipLaunchKernelGGL(k_repeat_rows, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, (size_t)(lds / 8), (uint4*)dst,
                       (size_t)(ldd / 8), (size_t)rows, cols / 8, rep);
    FD_CHECK_LAUNCH("k_repeat_rows");
    return FD_OK;
}

extern "C" int fd_copy2d_f16(const void* src, int lds, void* dst, int ldd, int64_t rows, int cols,
                             void* stream) {
    FD_PLAN(fd_copy2d_f16(src, lds, dst, ldd, rows, cols, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(src && dst && rows > 0 && cols > 0 && lds >= cols && ldd >= cols, FD_EINVAL,
                 "fd_copy2d_f16: args");
    FD_CHECK_ARG(cols % 8 == 0 && lds % 8 == 0 && ldd % 8 == 0 && (uintptr_t)src % 16 == 0 &&
                     (uintptr_t)dst % 16 == 0,
                 FD_ESHAPE, "fd_copy2d_f16: cols / strides must be multiples of 8 and the pointers 16-byte aligned");
    const size_t total = (size_t)rows * (cols / 8);
    const int blocks = fd_grid1d(total, 8192);
    hipLaunchKernelGGL(k_copy2d, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)src,
                       (size_t)(lds / 8), (uint4*)dst, (size_t)(ldd / 8), (size_t)rows, cols / 8);
    FD_CHECK_LAUNCH("k_copy2d");
    return FD_OK;
}

// ---- out = a*x + b*y (fp32): add_noise, latent scaling, VAE sampling helper ----------------
__global__ void k_axpby(const float* __restrict__ x, const float* __restrict__ y,
                        float* __restrict__ out, size_t n, float a, float b, int exp_half_x) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (size_t)gridDim.x * blockDim.x) {
        float xv = x[e];
        if (exp_half_x) xv = expf(0.5f * xv);  // std = exp(0.5 logvar)
        const float yv = y ? y[e] : 0.f;
        out[e] = exp_half_x ? __fmul_rn(__fmul_rn(xv, yv), b) : __fadd_rn(__fmul_rn(a, xv), __fmul_rn(b, yv));
    }
}

extern "C" int fd_axpby_f32(const float* x, const float* y, float* out, int64_t n, float a,
                            float b, int exp_half_x, void* stream) {
    FD_PLAN(fd_axpby_f32(x, y, out, n, a, b, exp_half_x, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && out && n > 0, FD_EINVAL, "fd_axpby_f32: args");
    const int blocks = fd_grid1d((size_t)n, 2048);
    hipLaunchKernelGGL(k_axpby, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y, out,
                       (size_t)n, a, b, exp_half_x);
    FD_CHECK_LAUNCH("k_axpby");
    return FD_OK;
}

// ---- CLIP text embeddings: out[b][l] = tok[ids[b][l]] + pos[l] --------------------------------
// (an id outside [0, vocab) is clamped to the nearest valid row: 0 or vocab - 1)
__global__ void k_embed_tokens(const long long* __restrict__ ids, const half_t* __restrict__ tok,
                               const half_t* __restrict__ pos, half_t* __restrict__ out, int L,
                               int D, int vocab) {
    const int row = blockIdx.x;
    const int l = row % L;
    long long id = ids[row];
    if (id < 0) id = 0;
    if (id >= vocab) id = vocab - 1;
    for (int d = threadIdx.x; d < D; d += blockDim.x)
        out[(size_t)row * D + d] =
            (half_t)((float)tok[(size_t)id * D + d] + (float)pos[(size_t)l * D + d]);
}

extern "C" int fd_embed_tokens_f16(const int64_t* ids, const void* tok_emb, const void* pos_emb,
                                   void* out, int B, int L, int D, int vocab, void* stream) {
    FD_PLAN(fd_embed_tokens_f16(ids, tok_emb, pos_emb, out, B, L, D, vocab, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(ids && tok_emb && pos_emb && out && B > 0 && L > 0 && D > 0 && vocab > 0, FD_EINVAL,
                 "fd_embed_tokens_f16: args");
    hipLaunchKernelGGL(k_embed_tokens, dim3(B * L), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)ids, (const half_t*)tok_emb, (const half_t*)pos_emb,
                       (half_t*)out, L, D, vocab);
    FD_CHECK_LAUNCH("k_embed_tokens");
    return FD_OK;
}

// ---- ViT embeddings: out[b][0] = cls + pos[0]; out[b][1+p] = patch[b][p] + pos[1+p] ----------
__global__ void k_vit_assemble(const half_t* __restrict__ patches, const half_t* __restrict__ cls,
                               const half_t* __restrict__ pos, half_t* __restrict__ out, int T,
                               int D) {
    const int row = blockIdx.x;  // b*T + t
    const int t = row % T, b = row / T;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const float v = t == 0 ? (float)cls[d] : (float)patches[((size_t)b * (T - 1) + t - 1) * D + d];
        out[(size_t)row * D + d] = (half_t)(v + (float)pos[(size_t)t * D + d]);
    }
}

extern "C" int fd_vit_assemble_f16(const void* patches, const void* cls, const void* pos, void* out,
                                   int B, int T, int D, void* stream) {
    FD_PLAN(fd_vit_assemble_f16(patches, cls, pos, out, B, T, D, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(patches && cls && pos && out && B > 0 && T > 1 && D > 0, FD_EINVAL,
                 "fd_vit_assemble_f16: args");
    hipLaunchKernelGGL(k_vit_assemble, dim3(B * T), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)patches, (const half_t*)cls, (const half_t*)pos, (half_t*)out,
                       T, D);
    FD_CHECK_LAUNCH("k_vit_assemble");
    return FD_OK;
}

// ---- sinusoidal timestep embedding (flip_sin_to_cos, shift 0): [cos | sin] -> fp16 -----------
__global__ void k_timestep_embedding(const float* __restrict__ t, int t_stride, half_t* __restrict__ out,
                                     int dim) {
    const int b = blockIdx.x;
    const int half_dim = dim / 2;
    const float tv = t[(size_t)b * t_stride];
    for (int i = threadIdx.x; i < half_dim; i += blockDim.x) {
        const float freq = expf(-9.210340371976184f * (float)i / (float)half_dim);
        const float a = tv * freq;
        out[(size_t)b * dim + i] = (half_t)cosf(a);
        out[(size_t)b * dim + half_dim + i] = (half_t)sinf(a);
    }
}

extern "C" int fd_timestep_embedding_f16(const float* t, int t_stride, void* out, int B, int dim,
                                         void* stream) {
    FD_PLAN(fd_timestep_embedding_f16(t, t_stride, out, B, dim, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(t && out && B > 0 && dim > 0 && dim % 2 == 0 && (t_stride == 0 || t_stride == 1),
                 FD_EINVAL, "fd_timestep_embedding_f16: args");
    hipLaunchKernelGGL(k_timestep_embedding, dim3(B), dim3(256), 0, (hipStream_t)stream, t, t_stride,
                       (half_t*)out, dim);
    FD_CHECK_LAUNCH("k_timestep_embedding");
    return FD_OK;
}

// ---- fp32 -> fp16 cast of a contiguous buffer (weights upload, embeddings) -------------------
__global__ void k_cast(const float* __restrict__ x, half_t* __restrict__ y, size_t n) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (size_t)gridDim.x * blockDim.x)
        y[e] = (half_t)x[e];
}

extern "C" int fd_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream) {
    FD_PLAN(fd_cast_f32_to_f16(x, y, n, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && y && n > 0, FD_EINVAL, "fd_cast_f32_to_f16: args");
    const int blocks = fd_grid1d((size_t)n, 4096);
    hipLaunchKernelGGL(k_cast, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (half_t*)y,
                       (size_t)n);
    FD_CHECK_LAUNCH("k_cast");
    return FD_OK;
}

__global__ void k_cast_back(const half_t* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
         e += (size_t)gridDim.x * blockDim.x)
        y[e] = (float)x[e];
}

extern "C" int fd_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream) {
    FD_PLAN(fd_cast_f16_to_f32(x, y, n, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && y && n > 0, FD_EINVAL, "fd_cast_f16_to_f32: args");
    const int blocks = fd_grid1d((size_t)n, 4096);
    hipLaunchKernelGGL(k_cast_back, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)x, y, (size_t)n);
    FD_CHECK_LAUNCH("k_cast_back");
    return FD_OK;
}

// ---- out = a + w (b - a) on fp16 buffers: the per-step blend of two cached context projections (UNet2DConditionModel.blend_context) ------
// Per element: half_rn(fd_lerp(float(a), float(b), w)) -- three separately rounded fp32 operations, one rounding to half.  w == 0 stores
// a's bits and w == 1 stores b's bits (a + 1 * (b - a) is not b in fp32 when |a| >> |b|).  a == b therefore gives a for every w (a zero of
// either sign gives +0 when 0 != w != 1).  HBM-bound: 16-byte accesses (8 halves per lane) when the three bases allow it.
__device__ __forceinline__ half_t fd_lerp_h(half_t a, half_t b, float w) {
    return w == 0.f ? a : w == 1.f ? b : (half_t)fd_lerp((float)a, (float)b, w);
}

template <int V>   // halves per lane and trip: 8 (all three bases 16-byte aligned) or 1
__global__ __launch_bounds__(256) void k_lerp_f16(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ out,
                                                   size_t n, float w) {
    const size_t nv = n / V;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < nv; e += (size_t)gridDim.x * blockDim.x) {
        if constexpr (V == 8) {
            const half8 av = *reinterpret_cast<const half8*>(a + e * 8), bv = *reinterpret_cast<const half8*>(b + e * 8);
            half8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = fd_lerp_h(av[i], bv[i], w);
            *reinterpret_cast<half8*>(out + e * 8) = o;
        } else {
            out[e] = fd_lerp_h(a[e], b[e], w);
        }
    }
    if constexpr (V == 8) {     // the tail: fewer than 8 halves, one lane each
        const size_t t = nv * 8 + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (t < n) out[t] = fd_lerp_h(a[t], b[t], w);
    }
}

extern "C" int fd_lerp_f16(const void* a, const void* b, void* out, int64_t n, float w, void* stream) {
    FD_PLAN(fd_lerp_f16(a, b, out, n, w, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(a && b && out && n > 0, FD_EINVAL, "fd_lerp_f16: args");
    FD_CHECK_ARG(out != a && out != b, FD_EINVAL, "fd_lerp_f16: out may alias neither input");
    const bool vec = ((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) % 16 == 0;
    if (vec) {
        const int blocks = fd_grid1d((size_t)n / 8 + 8, 2048);
        hipLaunchKernelGGL(k_lerp_f16<8>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)a, (const half_t*)b, (half_t*)out,
                           (size_t)n, w);
    } else {
        const int blocks = fd_grid1d((size_t)n, 2048);
        hipLaunchKernelGGL(k_lerp_f16<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)a, (const half_t*)b, (half_t*)out,
                           (size_t)n, w);
    }
    FD_CHECK_LAUNCH("k_lerp_f16");
    return FD_OK;
}

// ---- rectangular blend of one latent tensor onto another (CompositeGuide, reference
// composition/guide.py:86-98): dst[:, oy:oy+sh, ox:ox+sw] += blend * (src - dst) on NCHW fp32
__global__ void k_region_blend(float* __restrict__ dst, const float* __restrict__ src, int C, int H,
                               int W, int oy, int ox, int sh, int sw, float blend) {
    const int total = C * sh * sw;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int x = e % sw, y = (e / sw) % sh, c = e / (sw * sh);
        const size_t i = ((size_t)c * H + oy + y) * W + ox + x;
        dst[i] = fd_lerp(dst[i], src[i], blend);
    }
}

extern "C" int fd_region_blend_f32(float* dst, const float* src, int C, int H, int W, int oy, int ox,
                                   int sh, int sw, float blend, void* stream) {
    FD_PLAN(fd_region_blend_f32(dst, src, C, H, W, oy, ox, sh, sw, blend, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(dst && src && C > 0 && H > 0 && W > 0, FD_EINVAL, "fd_region_blend_f32: args");
    // the host resolves Python's slice semantics (a negative start counts from the end of the
    // axis: composition/guide.py:86-98) before calling; here only the clip at the far edge remains
    FD_CHECK_ARG(oy >= 0 && ox >= 0, FD_EINVAL, "fd_region_blend_f32: negative box origin (%d, %d)", oy, ox);
    if (oy + sh > H) sh = H - oy;
    if (ox + sw > W) sw = W - ox;
    if (sh <= 0 || sw <= 0) return FD_OK;
    const int total = C * sh * sw;
    hipLaunchKernelGGL(k_region_blend, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       dst, src, C, H, W, oy, ox, sh, sw, blend);
    FD_CHECK_LAUNCH("k_region_blend");
    return FD_OK;
}
