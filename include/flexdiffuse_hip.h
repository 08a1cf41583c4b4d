/*
 * libflexdiffuse_hip.so -- C ABI of the MI355X (gfx950) hot path of flexdiffuse.
 *
 * The reference (tim-speed/flexdiffuse) has no FFI of its own: its boundary is three
 * duck-typed Python protocols (guidance.py:315-474 `Guide`, pipeline/guide.py:8-72
 * `GuideBase`, pipeline/flex.py:46-310 `FlexPipeline`).  The host side of this
 * project keeps those protocols in Python (package `flexdiffuse_amd`) and binds the
 * entry points below with ctypes (flexdiffuse_amd/hip.py).  INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *  - every function returns FD_OK (0) or a negative FD_E* code; the message for the
 *    calling thread is available from fd_last_error();
 *  - all pointers are BORROWED DEVICE pointers (caller owns all memory; the library
 *    never allocates device memory) unless a parameter says "host";
 *  - `stream` is a hipStream_t passed as void*; every launch is asynchronous;
 *  - activations are NHWC / row-major fp16 ("h"), accumulation and statistics fp32;
 *  - no global state except the thread-local error string and the optional
 *    kernel-timing recorder (fd_prof_*).
 */
#ifndef FLEXDIFFUSE_HIP_H
#define FLEXDIFFUSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FD_OK 0
#define FD_EINVAL (-1) /* bad argument value */
#define FD_ESHAPE (-2) /* unsupported shape / alignment */
#define FD_EHIP (-3)   /* HIP runtime error */

#define FD_ABI_VERSION 12

int fd_abi_version(void);
const char* fd_last_error(void);
/* CU count, max engine clock (kHz), total HBM bytes and gcnArchName of `device`. */
int fd_device_info(int device, int* cu_count, int* clock_khz, int64_t* hbm_bytes,
                   char* arch, int arch_len);

/* Optional per-launch timing of a kernel family with HIP events recorded on the launch
 * stream (bench.py roofline leg).  Families: */
#define FD_FAMILY_GEMM 0      /* implicit-GEMM conv / GEMM MFMA kernel */
#define FD_FAMILY_ATTENTION 1 /* flash attention MFMA kernel */
#define FD_FAMILY_GROUPNORM 2 /* GroupNorm(+SiLU) statistics + apply */
#define FD_FAMILY_OTHER 3     /* (ABI 11) every other launch of the library: layout / elementwise / LayerNorm statistics / guidance */
int fd_prof_enable(int on);
/* Record events around every `stride`-th launch of each family only (default 1 = all): a pair of
 * event records costs ~6.6 us of stream time, which at one pair per launch is ~10 % of the pass
 * being measured.  fd_prof_collect then sums over the sampled launches. */
int fd_prof_set_stride(int stride);
/* Synchronises the recorded events of `family`, returns summed elapsed ms, declared work
 * (FLOPs for MFMA families, algorithmic bytes for HBM families) and launch count, and
 * forgets those records. Host pointers. */
int fd_prof_collect(int family, double* total_ms, double* total_work, int64_t* launches);
/* (ABI 9) the same plus `total_executed`: the work the kernels really issued -- equal to the declared work except
 * where a launch implements an op with fewer MACs than its definition (parity-decomposed upsample convolution: 4/9).
 * The hardware roofline is `executed` / time; `work` / time is the algorithmic-equivalent rate. */
int fd_prof_collect2(int family, double* total_ms, double* total_work, double* total_executed, int64_t* launches);
/* (ABI 11) Every recorded bracket one by one, in launch order: family, tag (an identity of the launch's shape and kernel choice; 0 =
 * none), elapsed ms, declared and executed work; then forgets all records.  Host arrays of `cap` entries, *n = entries written.
 * bench.py's roofline leg (the measurement of the `unet(...)` call of reference pipeline/guide.py:56-58) takes the MEDIAN per
 * (family, tag, work) group x the group's launch count, so one host stall inside one bracket cannot move a family's total. */
int fd_prof_drain(int32_t* family, uint32_t* tag, float* ms, double* work, double* executed, int64_t cap, int64_t* n);
/* Mean elapsed ms of an EMPTY event bracket (`pairs` back-to-back record pairs on `stream`);
 * subtract it per sampled launch to turn bracket time into kernel time. Host pointer. */
int fd_prof_calibrate(int pairs, double* ms_per_empty_pair, void* stream);

/* ------------------------------------------------------------------------------------
 * Launch plan.  The denoising loop (reference pipeline/flex.py:262-287) calls the UNet with the
 * same shapes at every step: the ~430 launches of a forward differ only in the CONTENTS of the
 * latent and timestep buffers.  While a thread records (fd_plan_record_begin .. _end) every launch
 * entry point of this library, besides launching, appends a by-value copy of its own call to the
 * plan; fd_plan_replay issues the recorded calls again on `stream` as ordinary eager launches
 * (same kernels, order and tile choices; none of the host front's per-op work).  The caller keeps
 * every recorded device address alive and unchanged and refreshes the input buffers between
 * replays.  Recording is per thread; a plan may be replayed from any ONE thread at a time.
 * ---------------------------------------------------------------------------------- */
typedef struct fd_plan fd_plan;
int fd_plan_create(fd_plan** out);
int fd_plan_destroy(fd_plan* plan);
int fd_plan_record_begin(fd_plan* plan); /* clears the plan; the calling thread records */
int fd_plan_record_end(fd_plan* plan);
int fd_plan_size(const fd_plan* plan, int* launches); /* recorded entry-point calls */
int fd_plan_replay(const fd_plan* plan, void* stream);

/* ------------------------------------------------------------------------------------
 * Guidance: CLIP image<->text token alignment and tween  (reference guidance.py)
 * ---------------------------------------------------------------------------------- */
#define FD_ORDER_TEXT 0   /* guidance.py:18 GUIDE_ORDER_TEXT   */
#define FD_ORDER_ALIGN 1  /* guidance.py:19 GUIDE_ORDER_ALIGN  */
#define FD_ORDER_DIRECT 2 /* guidance.py:20 GUIDE_ORDER_DIRECT */

/* Scratch floats needed by fd_guidance_map / fd_guidance_tween: B*N*L. */
int64_t fd_guidance_workspace_floats(int B, int N, int L);

/* Replaces guidance.py:23-85 `_map_emb` for B prompts at once.
 *   alt  [Balt][N][D] f32 guide tokens (alt_batched=0: one guide shared by all prompts)
 *   txt  [B][L][D]    f32 text tokens
 *   idx  [B][L] i32, s [B][L] f32 : row j = (guide index, similarity) of text column
 *        j+1, exactly as the reference's (L,2) array (last row stays (0,0)).
 * D % 32 == 0, L <= 96, N*(L|1)*4 <= 150 KiB. */
int fd_guidance_map(const float* alt, const float* txt, float* ws, int32_t* idx, float* s,
                    int B, int alt_batched, int N, int L, int D, int order, int reuse,
                    void* stream);

typedef struct fd_tween_params {
    double threshold_floor; /* guidance.py:205 */
    double threshold_mult;  /* guidance.py:206 */
    double clustered;       /* guidance.py:209 */
    double max_guidance;    /* guidance.py:210 */
    double header_max;      /* guidance.py:211 */
    int32_t order;          /* guidance.py:212 align_mode */
    int32_t reuse;          /* guidance.py:213 mapping_reuse */
} fd_tween_params;

/* Replaces guidance.py:215-272 `Tweener.tween` for B prompts at once (map + weights +
 * blend in two launches, no host round trip).
 *   base   [B][L][D] f32 text embeddings; alt as in fd_guidance_map
 *   lin_w  [L] f32 = torch.linspace(linear_start, linear_end, L) (guidance.py:231-233;
 *          computed by the host exactly as the reference does)
 *   out    [B][L][D] f32 tweened embeddings
 *   weights[B][L] f32 blend weights after the header cap (the vector the reference
 *          prints at guidance.py:255); idx/s as in fd_guidance_map
 *   status [B] i32: 0 ok, 1 = adjacent equal similarity peaks (the reference raises
 *          ZeroDivisionError at guidance.py:112; out is then the un-tweened base). */
int fd_guidance_tween(const float* base, const float* alt, const float* lin_w, float* ws,
                      float* out, float* weights, int32_t* idx, float* s, int32_t* status,
                      int B, int alt_batched, int N, int L, int D,
                      const fd_tween_params* p, void* stream);

/* Replaces guidance.py:288-312 `ConceptMapper.map`: for text row j, c = ct_idx[j];
 * if c >= 1 and ct_s[j] > 0.9: out[j+1] = guide[cm_idx[c-1]].  guide [N][D], out [L][D]. */
int fd_guidance_concept_override(const float* guide, const int32_t* cm_idx,
                                 const int32_t* ct_idx, const float* ct_s, float* out,
                                 int N, int L, int D, void* stream);

/* guidance.py:467-472 pure-image path: out[b][0][:] += (hdr[:] - out[b][0][:]) * 0.85 */
int fd_guidance_header_pull(float* out, const float* hdr, int B, int L, int D, void* stream);

/* ------------------------------------------------------------------------------------
 * Dense contractions: fp16 MFMA GEMM / implicit-GEMM convolution with fused epilogue.
 * Replaces the cuDNN/cuBLAS kernels diffusers/transformers launch inside
 * `unet(...)` (reference pipeline/guide.py:56-58), `vae.decode/encode`
 * (pipeline/flex.py:118,189) and the CLIP towers (encode/clip.py:64,86-100).
 * ---------------------------------------------------------------------------------- */
#define FD_ACT_NONE 0
#define FD_ACT_SILU 1
#define FD_ACT_QUICK_GELU 2 /* x * sigmoid(1.702 x)  (CLIP) */
#define FD_ACT_GELU 3       /* exact erf GELU */
#define FD_ACT_GEGLU 4      /* value * gelu(gate); weight rows interleaved 16 value / 16 gate */

typedef struct fd_gemm_desc {
    const void* A;        /* fp16: linear [M][lda]; conv: NHWC input [B][in_h][in_w][in_c], pixel stride lda halfs (0 = in_c; >= in_c, % 8) */
    const void* W;        /* fp16 [N][ldw], K contiguous (conv: [Cout][kh][kw][Cin]) */
    void* C;              /* fp16 (or fp32 if out_f32) [M][ldc]; GEGLU: [M][N/2] */
    const float* bias;    /* [N] or NULL */
    const float* bias2;   /* per-sample bias [M/rows_per_sample][ld_bias2] or NULL */
    const void* residual; /* fp16 [M][ldr] added after the activation, or NULL */
    int32_t M, N, K;
    int32_t lda, ldw, ldc, ldr, ld_bias2;
    int32_t rows_per_sample; /* rows of A per sample (H*W or tokens); 0 = M */
    int32_t act;             /* FD_ACT_* */
    int32_t out_f32;
    float alpha;             /* scales the accumulator before bias; 0 means 1 */
    /* implicit-GEMM convolution (conv != 0): in_c % 64 == 0, K = kh*kw*in_c.
     * upsample2x: 1 = the input is read through a fused nearest-2x upsample (in_h / in_w are the LOW-resolution size).
     * 2 = PHASE-DECOMPOSED upsample convolution: diffusers' Upsample2D (nearest 2x, then conv3x3; inside `unet(...)`,
     * reference pipeline/guide.py:56-58, and `vae.decode`, pipeline/flex.py:118) computed as four 2x2 convolutions of the
     * low-resolution input, one per output-pixel parity (py, px) = (z >> 1, z & 1) with batch = 4: W is [4][N][2*2*in_c]
     * (batch_stride_w = N * ldw), the 3x3 taps that fall on the same source pixel pre-summed per parity (4/9 of the MACs,
     * same sums); M = B * in_h * in_w rows of the low-resolution grid, out_h = in_h, out_w = in_w, kh = kw = 2, and C is the
     * FULL-resolution [B][2 in_h][2 in_w][ldc] map into which slice z writes the pixels (2y + py, 2x + px).
     * Ranges (FD_ESHAPE outside them, before any launch): upsample2x 0..2; stride, kh, kw >= 1; pad_t, pad_l 0..16; the input view
     * (in_h, in_w; doubled under upsample2x == 1) and (out - 1) * stride + k at most 16384 in each direction. */
    int32_t conv, in_h, in_w, in_c, out_h, out_w, kh, kw, stride, pad_t, pad_l, upsample2x;
    /* transposed store: C is [sample][N][trans_ld] (row n, column m within the sample) */
    int32_t trans_out, trans_ld;
    int64_t trans_sample_stride;
    /* batched GEMM over blockIdx.z: element strides per batch */
    int32_t batch;
    int64_t batch_stride_a, batch_stride_w, batch_stride_c, batch_stride_res;
    /* scheduling: tile 0 = auto, 1 = 128x128, 2 = 128x160, 3 = 128x64, 4 = 64x64, 5 = 256x160 and
     * 6 = 256x128 (8 waves), 7/8 = the same with 3 LDS stages, 9 = 128x160 and 10 = 128x128 with
     * 8 waves, 11 = 128x64 with 8 waves, 12 = 128x160, 13 = 256x160 and 14 = 256x128 with 16 waves; 30 = 256x320, 31 = 256x256, 32 = 128x320, 33 = 256x160 on
     * the deep-pipelined ping-pong loop (csrc/gemm_pp.hip: 8 waves, full tiles and K % 64 == 0 only, FD_ESHAPE otherwise);
     * split_k 0 =
     * auto (needs `workspace`, fp32 [split_k][M][N]), 1 = off. Results are deterministic for
     * a given (shape, tile, split_k). */
    int32_t tile, split_k;
    void* workspace;
    int64_t workspace_bytes;
    /* LayerNorm folded into the GEMM (replaces the separate LayerNorm launch diffusers' BasicTransformerBlock
     * runs before attn1 / attn2 / ff inside `unet(...)`, reference pipeline/guide.py:56-58).  A holds the
     * UN-normalised rows x, W the weights pre-multiplied by the LayerNorm gain (W' = W diag(gamma), fp16),
     * bias = b + W beta, ln_colsum[n] = sum_k W'[n][k] (of the fp16 values), ln_stats[m] = (rstd_m,
     * -mean_m rstd_m) from fd_ln_row_stats_f16:
     *   C[m][n] = act(rstd_m (x W'^T)[m][n] - rstd_m mean_m ln_colsum[n] + bias[n])  ==  act(LN(x) W^T + b).
     * Linear GEMMs only; act NONE or GEGLU; works with trans_out.  NULL = off. */
    const float* ln_stats;  /* fp32 [M][2] */
    const float* ln_colsum; /* fp32 [N] */
    /* Producer side of the fold: also write ln_stats_out[m] = (rstd_m, -mean_m rstd_m) of the OUTPUT rows
     * (LayerNorm over the N columns, eps ln_eps, statistics of the fp16-rounded values), so that the next
     * GEMM can take them as its ln_stats without a separate statistics pass.  N == 320, M % 256 == 0: one workgroup
     * tile spans the row and writes the finished pair.  N a larger multiple of 160, M % 128 == 0: ln_stats_out is
     * [N / 160][M][2] RAW partial sums (sum, sum of squares per 160-column tile), to be combined by
     * fd_ln_finalize_stats_f32.  fd_gemm_can_emit_row_stats returns the slab count (0: not possible, 1: finished).
     * Linear, plain or residual epilogue. NULL = off. */
    float* ln_stats_out;
    float ln_eps;
    /* APPENDED phase: after the K columns of the GEMM / convolution the same K loop runs K2 more columns over the plain
     * rows of a second operand A2 [M][lda2] against W[:, K .. K+K2):
     *   C = epilogue( A-part(A, W[:, :K]) + A2 W[:, K:]^T ).
     * Two uses inside `unet(...)` (reference pipeline/guide.py:56-58), both weight folds done once at model construction:
     * a ResBlock's 1x1 shortcut convolution rides in conv2's accumulation (diffusers ResnetBlock2D.conv_shortcut: no
     * shortcut launch, no shortcut tensor written and re-read as the residual); and a transformer block's proj_out is
     * folded THROUGH the feed-forward output layer, proj_out(ff2(f) + h) = f (Wp W2)^T + h Wp^T + (bp + Wp b2): one GEMM
     * with A = f, A2 = h instead of two.  W is [N][ldw] with ldw >= K + K2; K % 64 == 0, K2 % 64 == 0; LDS-DMA path only. */
    const void* A2;
    int32_t lda2, K2;
    /* (ABI 8) batch > 1: `bias` advances by this many floats per batch (0: one bias for every batch).  With per-batch
     * weights (batch_stride_w) this is the GroupNorm fold of fd_groupnorm_fold_linear_f16: sample b's rows are
     * multiplied by ITS weights and get ITS bias.  LDS-DMA path with LDS-staged biases only.  With batch > 1,
     * ln_stats_out needs batch_stride_c == M * ldc (row index = batch * M + m). */
    int64_t batch_stride_bias;
    /* (ABI 11) GroupNorm(+SiLU) of the OUTPUT fused into the split-K finish pass: gn_out [M][N] (contiguous fp16) =
     * act(GroupNorm_{gn_groups}(C; gn_gamma, gn_beta, gn_eps)) over the rows_per_sample rows x N / gn_groups channels of each
     * (sample, group), statistics of the fp16-rounded values of C -- bit for bit what fd_groupnorm_nhwc_f16 gives on C.  Inside
     * `unet(...)` (reference pipeline/guide.py:56-58) a ResBlock's conv1 feeds nothing but norm2 + SiLU (diffusers ResnetBlock2D):
     * at the 16x16 / 8x8 levels, where the convolution is split over K, the pass that sums the fp32 partial slabs normalises the
     * tile it has just summed -- one launch less, and with gn_skip_c the convolution's own output never goes to HBM (C may then be
     * NULL).  Only honoured by split-K launches (ask fd_gemm_plan for the split, fd_gemm_can_fuse_groupnorm for the shape);
     * FD_ESHAPE otherwise.  act NONE, fp16 output, batch 1; residual row stride % 8 == 0; not together with residual_rows (FD_EINVAL:
     * this finish pass adds residual row m, it does not wrap).  NULL = off. */
    void* gn_out;
    const float* gn_gamma; /* [N] */
    const float* gn_beta;  /* [N] */
    int32_t gn_groups, gn_silu;
    float gn_eps;
    int32_t gn_skip_c;
    /* (ABI 11) GroupNorm PARTIAL SUMS of the output from the epilogue of the producing launch: gn_part_out
     * [M / rows_per_sample][chunks][gn_groups][2] fp32 = (sum, sum of squares) of the fp16-rounded outputs of each (sample, row
     * chunk, group) -- the layout fd_groupnorm_apply_parts_f16 / fd_groupnorm_fold_linear_parts_f16 consume, `chunks` =
     * fd_gemm_gn_parts_chunks(desc).  At the 64x64 level of `unet(...)` (reference pipeline/guide.py:56-58) the GroupNorms behind a
     * convolution (norm2 behind conv1, the transformer's input norm behind conv2) then need no statistics pass over the tensor the
     * convolution has just written.  Honoured where one tile spans the row and lies in one sample (N == 320, the 256x320 / 128x320
     * tiles, lean epilogue, act NONE, batch 1, no split-K); FD_ESHAPE otherwise -- ask fd_gemm_gn_parts_chunks first.  Uses gn_groups.
     * gn_part_chunks: the chunk count the buffer was sized for (what fd_gemm_gn_parts_chunks answered); a launch whose tile would write
     * another count -- a forced `tile` -- is refused instead of writing past the buffer.  NULL = off. */
    float* gn_part_out;
    int32_t gn_part_chunks;
    /* (ABI 11) TRANSPOSED TAIL: columns n >= trans_n0 of the output are stored transposed into C2 -- [sample][N - trans_n0][trans_ld]
     * (row n - trans_n0, column m within the sample; trans_ld / trans_sample_stride as for trans_out) -- while columns n < trans_n0 go to C
     * [M][ldc] as usual.  The self-attention of diffusers' BasicTransformerBlock.attn1 inside `unet(...)` (reference pipeline/guide.py:56-58)
     * projects q, k and v from the same LayerNorm'd rows: with the weights stacked [q | k | v] this is ONE launch that reads the hidden
     * states once and writes q|k row-major and V^T in the layout fd_attention_f16 takes, instead of two launches over the same rows.
     * Linear GEMM with the LayerNorm fold (ln_stats), act NONE, no residual / bias2 / batch; M %% 128 == 0, N and trans_n0 multiples of
     * 160, rows_per_sample %% 32 == 0, trans_ld %% 8 == 0.  0 = off. */
    int32_t trans_n0;
    void* C2;
    /* (ABI 11, EXPERIMENTAL: measured and left off) in-launch split-K reduction on the ping-pong tiles: sk_sync =
     * 2 x (output tiles) zero-initialised uint32 (arrival / departure counters, left zero by every launch).  Each K-slice workgroup publishes its
     * fp32 slab, arrives (agent-scope release), waits for the tile's other slices (acquire, bounded spin) and finishes 1/split_k of the tile's rows
     * in the fixed slice order -- the bits of the finish launch, without it.  Needs every workgroup of the launch RESIDENT at once
     * (tiles x split_k <= CUs, one per CU: refused otherwise) and nothing else competing for the CUs: two such launches from two processes
     * sharing a GPU can starve each other, which is why the product does not use it.  NULL = the finish launch. */
    void* sk_sync;
    /* (ABI 11) LayerNorm fold fed with the producer's PARTIAL sums: ln_stats_parts = k in {2, 4, 8} > 0 makes ln_stats the raw slabs
     * [k][ln_stats_rows][2] (sum, sum of squares per 160-column tile) that a producer GEMM wrote through ln_stats_out, instead of the finished
     * (rstd, -mean rstd) pairs: every tile of this launch finalises its own rows into LDS (the arithmetic of fd_ln_finalize_stats_f32, bit for
     * bit, over K columns with ln_fold_eps) -- the finalise launch between a transformer block's producer and consumer GEMMs inside `unet(...)`
     * (reference pipeline/guide.py:56-58) disappears.  One-tile LDS-DMA and ping-pong kernels (the persistent form is not used then). 0 = off. */
    int32_t ln_stats_parts, ln_stats_rows;
    float ln_fold_eps; /* 0 = 1e-5 */
    /* (ABI 12) residual_rows > 0: output row m adds residual row m %% residual_rows -- the residual of a GEMM whose rows are `rep` replicas of
     * a shared prefix (the classifier-free-guidance fan-out inside `unet(...)`, reference pipeline/guide.py:56-58: both halves of the batch read
     * the same hidden states until the first cross-attention) without materialising the replicas.  Linear GEMM, batch 1,
     * M %% residual_rows == 0 and residual_rows a multiple of the tile's rows (256 covers every tile but the 288-row one).  Not together
     * with gn_out (FD_EINVAL: the GroupNorm finish pass does not wrap the residual rows).  0 = row m. */
    int32_t residual_rows;
    /* (additive; FD_ABI_VERSION stays 12) PER-HEAD SOFTMAX of the output: the N columns are `N / softmax_group` groups of softmax_group = 80
     * base-2 logits, of which the first softmax_valid (1..80) are real keys; C[m][group] = softmax over those, stored normalised fp16, the pad
     * columns as 0.  This is launch 1 of the CONTEXT-FOLDED cross-attention of `unet(...)` (reference pipeline/guide.py:56-58; diffusers
     * BasicTransformerBlock.attn2): the text context is fixed over the denoising loop, so to_q and K fold into K'_h = Wq_h K_h^T once per
     * context and  P = softmax_h(LN(x) K')  is one LayerNorm-fold GEMM (ln_stats / ln_stats_parts) against per-sample weights -- batch = samples,
     * batch_stride_w, and batch_stride_bias then advances `bias` AND `ln_colsum` (both [batch][N] fp32); the statistics of batch z are rows
     * z * M .. of ln_stats (ln_stats_rows >= batch * M).  Launch 2 is an ordinary residual GEMM  P V' + bo + x  with V'_h = V_h Wo_h as its
     * per-sample weights.  A wave tile is one head (80 columns): the softmax never leaves the wave.  Needs N %% 160 == 0, M %% 64 == 0 (rows per
     * launch slice: a tile never holds rows of two samples), ldc %% 8 == 0, operands < 2 GiB, the LDS-DMA path; FD_ESHAPE otherwise -- ask
     * fd_gemm_plan (tile 24: 64x160, 25: 128x160) and keep the unfolded launches for a refused shape.  0 = off. */
    int32_t softmax_group, softmax_valid;
} fd_gemm_desc;

int fd_gemm_f16(const fd_gemm_desc* desc, void* stream);
/* > 0 when fd_gemm_f16 will honour ln_stats_out for an [M][N] fp16 output (row stride ldc, residual row stride ldr
 * or 0) with the library's current settings: 1 = the finished (rstd, -mean rstd) pairs, k > 1 = k slabs of partial
 * sums for fd_ln_finalize_stats_f32; 0: run fd_ln_row_stats_f16 on the output instead. */
int fd_gemm_can_emit_row_stats(int M, int N, int K, int ldc, int ldr);
/* The tile id and split-K factor fd_gemm_f16 would launch `d` with -- the same argument checks and cost model (reference call
 * site: every linear / convolution behind pipeline/guide.py:56-58), nothing launched, no HIP call: usable without a device.
 * Tile ids as in fd_gemm_desc.tile (30..33: the ping-pong kernels of gemm_pp.hip; -7: the 128x128 generic kernel with the
 * LayerNorm fold compiled in).  Pointers are only tested for NULL / alignment. */
int fd_gemm_plan(const fd_gemm_desc* d, int* tile, int* split_k);
/* (ABI 11) 1 when a split-K launch of an [M][N] output with `rows_per_sample` rows per sample and split factor `split_k` can take
 * fd_gemm_desc.gn_out with `groups` groups (the slab of one sample x a few groups fits the finish kernel's registers); 0: run
 * fd_groupnorm_nhwc_f16 on the output instead.  Host logic only. */
int fd_gemm_can_fuse_groupnorm(int M, int N, int rows_per_sample, int groups, int split_k);
/* (ABI 11) Row chunks per sample of fd_gemm_desc.gn_part_out for `d` (with d->gn_groups set): > 0 when fd_gemm_f16 will honour it with the
 * tile the rule picks, 0: run the statistics pass on the output instead.  Host logic only. */
int fd_gemm_gn_parts_chunks(const fd_gemm_desc* d);
/* (additive; FD_ABI_VERSION stays 12) The two fp32 rows per sample that launch 1 of the context-folded cross-attention (fd_gemm_desc.softmax_group)
 * takes beside the folded keys kf [samples][heads * 80][C] fp16 (row h * 80 + l = Wq'^T K_{h,l}, pad rows zero):
 *   rows[s][0][n] = sum_c kf[s][n][c]                              (ln_colsum: of the ROUNDED values, so a row mean cancels exactly)
 *   rows[s][1][h * 80 + l] = sum_j bias_q[h * d + j] K[s * n_keys + l][h * d + j]   for l < n_keys, 0 for the pad keys   (bias)
 * K [samples * n_keys][ldk] fp16 is the cached key projection, bias_q [heads * head_dim] fp32 the folded q bias.  Fixed summation order.
 * C %% 8 == 0, head_dim %% 8 == 0, n_keys <= 80. */
int fd_xattn_fold_rows_f32(const void* kf, const void* K, const float* bias_q, float* rows, int samples, int n_keys, int heads, int head_dim,
                           int C, int ldk, void* stream);

/* Flash attention forward (scores never leave registers).  Q [B][n_q][ldq], K [B][n_k][ldk]
 * with head h at column h*head_dim; Vt [B][heads*head_dim][ldvt] is V transposed (keys
 * contiguous; columns n_k..ldvt-1 must be finite, e.g. zero); O [B][n_q][ldo].
 * head_dim % 8 == 0, <= 160.  scale <= 0 means head_dim^-0.5.  causal: key <= query.
 * q_prescaled != 0: Q already carries scale*log2(e) (e.g. folded into the q projection's
 * weights), so K.Q^T is used directly as the base-2 logit and `scale` is ignored (head_dim <= 80
 * or 160 only). */
typedef struct fd_attention_desc {
    const void* Q;
    const void* K;
    const void* Vt;
    void* O;
    int64_t q_sample_stride, k_sample_stride, vt_sample_stride, o_sample_stride;
    int32_t ldq, ldk, ldvt, ldo;
    int32_t batch, heads, n_q, n_k, head_dim;
    int32_t causal;
    float scale;
    int32_t q_prescaled;
} fd_attention_desc;

int fd_attention_f16(const fd_attention_desc* desc, void* stream);

/* Fused front half of the UNet's cross-attention at the 64x64 level (8 heads x 40 channels, 256-row
 * tiles) and at the 32x32 level (8 heads x 80 channels, 128-row tiles, two 320-column n-tiles): the
 * LayerNorm-fold q projection and softmax(Q K^T) V over the step-invariant text context (65..80
 * keys) in ONE launch -- replaces the q-projection fd_gemm_f16 launch and the fd_attention_f16
 * launch of diffusers' BasicTransformerBlock.attn2 inside `unet(...)` (reference
 * pipeline/guide.py:56-58); the query matrix never goes to HBM.  Other shapes are refused (FD_ESHAPE).
 * fd_xattn_pack_kv_f16 packs the context's K [samples][n_keys][ldk] / V^T [samples][heads*head_dim][ldvt]
 * (the outputs of the to_k / to_v projections, computed once per context; 1..80 keys, ldk >= heads*head_dim,
 * ldvt >= n_keys; K rows and V^T columns >= n_keys are never read) into per-sample "images"
 * in MFMA fragment order, fd_xattn_image_bytes(heads, head_dim) bytes each: 61440 at 8 x 40, 102400 at
 * 8 x 80, 0 = unsupported shape.  Every byte of an image is written; key slots >= n_keys are zero. */
int64_t fd_xattn_image_bytes(int heads, int head_dim);
int fd_xattn_pack_kv_f16(const void* K, const void* Vt, void* k_image, void* v_image, int samples, int n_keys,
                         int heads, int head_dim, int ldk, int ldvt, int64_t k_sample_stride,
                         int64_t vt_sample_stride, void* stream);
typedef struct fd_xattn_desc {
    const void* x;          /* fp16 [M][ldx] UN-normalised hidden states */
    const void* wq;         /* fp16 [C][ldw] q weights with the LayerNorm gain and head_dim^-0.5 log2(e) folded in */
    const float* bias;      /* [C] folded bias (W beta), see fd_gemm_desc.ln_stats */
    const float* ln_colsum; /* [C] */
    const float* ln_stats;  /* [M][2] (rstd, -mean rstd) of the rows of x */
    const void* k_image;    /* [n_rep * M / rows_per_sample] images: replica r of sample b at index r * (M / rows_per_sample) + b */
    const void* v_image;
    void* out;              /* fp16 [n_rep * M][ldo]: attention output (heads concatenated), replica-major */
    int32_t M, ldx, ldw, ldo; /* M: a multiple of the row tile; ldx, ldw multiples of 8, ldo of 4, all >= heads * head_dim; x, wq 16-byte, out 8-byte aligned */
    int32_t rows_per_sample; /* query rows per sample; a multiple of the row tile (256 at head_dim 40, 128 at head_dim 80) that divides M */
    int32_t n_rep;           /* context replicas sharing the same queries (CFG fan-out of a shared prefix); >= 1 */
    int32_t n_keys, heads, head_dim;
    /* (ABI 12) ln_stats_parts = k in {2, 4, 8}: ln_stats holds the k partial slabs [k][M][2] (sum, sum of squares per 160-column tile) that the
     * producer GEMM wrote through fd_gemm_desc.ln_stats_out; every tile finalises its own rows (fd_ln_finalize_stats_f32's arithmetic, bit for
     * bit, over heads * head_dim columns with ln_fold_eps) -- as fd_gemm_desc.ln_stats_parts does for the GEMM consumers.  0 = finished pairs. */
    int32_t ln_stats_parts;
    float ln_fold_eps;       /* 0 = 1e-5 */
} fd_xattn_desc;
int fd_xattn_q_f16(const fd_xattn_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------
 * Normalisation / softmax (HBM-bound)
 * ---------------------------------------------------------------------------------- */
int64_t fd_groupnorm_workspace_floats(int B, int G);
/* GroupNorm(G, eps) [+ SiLU] on NHWC fp16 x [B][HW][C] -> y (may alias x). ws: scratch. */
int fd_groupnorm_nhwc_f16(const void* x, void* y, const float* gamma, const float* beta,
                          float* ws, int B, int HW, int C, int G, float eps, int silu,
                          void* stream);
/* Same with a row stride ldx >= C (in elements) on the INPUT: x is a column slice of a wider
 * [B*HW][ldx] matrix (the UNet writes skip tensors straight into the decoder's concatenation
 * buffers, pipeline/flex.py's UNet call -> diffusers' torch.cat of the skip connections). y is
 * contiguous [B][HW][C] and must not alias x. */
int fd_groupnorm_nhwc_ld_f16(const void* x, int ldx, void* y, const float* gamma, const float* beta,
                             float* ws, int B, int HW, int C, int G, float eps, int silu,
                             void* stream);
/* (ABI 11) The apply pass alone, from partial sums parts [B][chunks][G][2] that the PRODUCER of x wrote (fd_gemm_desc.gn_part_out):
 * y = GroupNorm(x)(+SiLU) without the statistics pass over x. */
int fd_groupnorm_apply_parts_f16(const void* x, int ldx, void* y, const float* gamma, const float* beta, const float* parts,
                                 int chunks, int B, int HW, int C, int G, float eps, int silu, void* stream);
/* GroupNorm folded into the linear layer that consumes it (the transformer block's norm -> proj_in, diffusers
 * Transformer2DModel.norm / proj_in inside the `unet(...)` call of reference pipeline/guide.py:56-58):
 *   proj_in(GN(x))[m][n] = sum_c w_out[b][n][c] x[m][c] + (bias[n] + (W beta)[n] - sum_g mean_{b,g} sum_{c in g} w_out[b][n][c]),
 *   w_out[b][n][c] = fp16(W[n][c] gamma_c rstd_{b,g(c)})
 * One statistics pass over x [B][HW][ldx] (the first launch of fd_groupnorm_nhwc_ld_f16), then per sample b the scaled
 * weights w_out [B][N][C] fp16 and bias_out [B][N] fp32 from the model constants wg = W diag(gamma) (fp16 [N][C]) and
 * biasf = bias + W beta (fp32 [N]).  (ABI 9) the mean term is summed over the ROUNDED w_out, so a group mean cancels
 * exactly whatever its size relative to the group's spread.  The normalised activation is never written: the consumer is
 * fd_gemm_f16 with batch = B, batch_stride_w = N * C, batch_stride_bias = N on x itself. */
int fd_groupnorm_fold_linear_f16(const void* x, int ldx, float* ws, int B, int HW, int C, int G, float eps,
                                 const void* wg, const float* biasf, int N,
                                 void* w_out, float* bias_out, void* stream);
/* (ABI 11) The same from the producer's partial sums (fd_gemm_desc.gn_part_out), without reading x at all. */
int fd_groupnorm_fold_linear_parts_f16(const float* parts, int chunks, int B, int HW, int C, int G, float eps,
                                       const void* wg, const float* biasf, int N, void* w_out, float* bias_out, void* stream);
/* LayerNorm over the last dim of fp16 x [rows][ldx] -> fp16 (or fp32) y [rows][ldy]. */
int fd_layernorm_f16(const void* x, void* y, const float* gamma, const float* beta, int rows,
                     int C, int ldx, int ldy, float eps, int out_f32, void* stream);
/* Per-row LayerNorm statistics of fp16 x [rows][ldx] (exact two-pass, fp32): stats[row] = (rstd,
 * -mean * rstd) with rstd = 1 / sqrt(var + eps); consumed by fd_gemm_desc.ln_stats. */
int fd_ln_row_stats_f16(const void* x, float* stats, int rows, int C, int ldx, float eps, void* stream);
/* partials [n_tiles][M][2] (fd_gemm_desc.ln_stats_out of an N > 320 producer) -> stats [M][2] = (rstd, -mean rstd)
 * over the N columns, eps as fd_ln_row_stats_f16 (one-pass E[x^2] - mean^2 in fp32, fixed summation order). */
int fd_ln_finalize_stats_f32(const float* partials, float* stats, int M, int N, int n_tiles, float eps, void* stream);
/* In-place softmax(scale * x) over the first N columns of fp16 x [rows][ld]. */
int fd_softmax_rows_f16(void* x, int rows, int N, int ld, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Layout / elementwise helpers
 * ---------------------------------------------------------------------------------- */
/* NCHW fp32 [B][C][HW] * scale -> NHWC fp16 [rep*B][HW][c_pad] (channels >= C are +0, the rep replicas identical).
 * Per element half_rn(x * scale): ONE fp32 product and ONE rounding to half (round to nearest even; -0 stays -0). */
int fd_nchw_f32_to_nhwc_f16(const float* x, void* y, int B, int C, int HW, int rep, int c_pad,
                            float scale, void* stream);
/* NHWC fp32 [B][HW][ld] -> NCHW fp32 [B][C][HW]: y = x*a + b, optionally clamped to [0,1].  The affine MAY BE FUSED (one FMA or a
 * product and a sum rounded separately): |y - (x a + b)| <= 2^-24 (|x a| + |x a + b|) either way; the clamp follows the affine, so
 * 0 <= y <= 1 exactly.  Columns C .. ld-1 of x are never read. */
int fd_nhwc_f32_to_nchw_f32(const float* x, float* y, int B, int C, int HW, int ld, float a,
                            float b, int clamp01, void* stream);
/* (ABI 12) 3x3 / stride 1 / pad 1 convolution of a NARROW input (Cin <= 4) read straight from the fp32 NCHW tensor -- the UNet's conv_in
 * (reference pipeline/guide.py:56-58, the first layer of `unet(...)`; diffusers UNet2DConditionModel.conv_in):
 *   y[(b H + i) W + j][co] = bias[co] + sum_{ky, kx, ci} half(x[b][ci][i + ky - 1][j + kx - 1] * scale) * w[co][ky][kx][ci]
 * (fp16 x fp16 products, fp32 accumulation, fp16 NHWC rows of stride ldy).  w: [Cout][3][3][4] fp16, channels >= Cin zero.  rep2 > 0 also
 * writes `rep2` replicas of the output to y2 (row stride ldy2, replica r at rows r B H W ...): the classifier-free-guidance fan-out's copy
 * of the first skip tensor.  One launch instead of fd_nchw_f32_to_nhwc_f16 + fd_im2col_f16 + fd_gemm_f16 (+ fd_repeat_rows_f16). */
int fd_conv3x3_narrow_f16(const float* x, const void* w, const float* bias, void* y, int ldy, void* y2, int ldy2, int rep2,
                          int B, int Cin, int H, int W, int Cout, float scale, void* stream);
/* im2col for convolutions with fewer than 64 input channels: NHWC fp16 x [B][Hi][Wi][Cin] -> out [B*Ho*Wo][k_pad] with
 * out[(b Ho + oy) Wo + ox][(kh KW + kw) Cin + ci] = x[b][oy stride + kh - pad_t][ox stride + kw - pad_l][ci], +0 for taps outside the
 * image and in columns KH KW Cin .. k_pad-1.  KH, KW, stride > 0, pads >= 0 (FD_EINVAL); k_pad >= KH KW Cin, a multiple of 8. */
int fd_im2col_f16(const void* x, void* y, int B, int Hi, int Wi, int Cin, int Ho, int Wo, int KH,
                  int KW, int stride, int pad_t, int pad_l, int k_pad, void* stream);
/* out[m] = [a[m] | b[m]] for dense fp16 rows: a [M][Ca], b [M][Cb], out [M][Ca + Cb].  Ca, Cb >= 0 and multiples of 8, not both 0
 * (a zero-width half is legal; its pointer must still be non-NULL); all three pointers 16-byte aligned (FD_ESHAPE). */
int fd_concat_channels_f16(const void* a, const void* b, void* out, int64_t M, int Ca, int Cb,
                           void* stream);
/* Classifier-free guidance (pipeline/guide.py:59-63) fused with the DDIM update the
 * reference obtains from scheduler.step (pipeline/flex.py:280-285), eta = 0:
 *   eps = u + g (t - u); x0 = (x - c1 eps)/c2; x <- c3 x0 + c4 eps
 * with c1 = sqrt(1-a_t), c2 = sqrt(a_t), c3 = sqrt(a_prev), c4 = sqrt(1-a_prev).
 * x: NCHW fp32 [B][C][HW] updated in place when do_step; eps_nhwc: UNet output
 * [(cfg?2:1)*B][HW][ld] fp32 (unconditional half first); eps_out (optional) NCHW fp32.
 * This entry point, fd_cfg_ddim_masked_step_f32 and fd_cfg_multistep_step_f32 are ONE kernel (k_latent_step,
 * csrc/step.hip) over one statement of the arithmetic (csrc/latent_step.h, every operation a separately rounded fp32
 * one), so they are bit-equal wherever they compute the same thing; float4 along the NCHW planes when HW % 4 == 0 and
 * the NCHW pointers are 16-byte aligned, scalar otherwise -- the same bits either way. */
int fd_cfg_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, int B, int C, int HW,
                         int ld, int cfg, float guidance, float c1, float c2, float c3, float c4,
                         int v_prediction, int do_step, void* stream);
/* out = a*x + b*y; with exp_half_x: out = exp(0.5 x) * y * b (VAE posterior sampling).  Plain form: the two products and the sum
 * are three SEPARATELY ROUNDED fp32 operations (no FMA), so the result has the bits of the same three host operations; y == NULL
 * stands for y = 0 (a x = -0 then gives +0 for b >= 0).  out may be x itself (same base, in place): every element is read before it
 * is written, by the same thread; a partial overlap is not supported. */
int fd_axpby_f32(const float* x, const float* y, float* out, int64_t n, float a, float b,
                 int exp_half_x, void* stream);
/* CLIP text embeddings: out[b][l] = half_rn(float(tok_emb[ids[b][l]]) + float(pos_emb[l])), tok_emb [vocab][D], pos_emb [L][D].
 * An id outside [0, vocab) is CLAMPED: a negative id reads row 0, an id >= vocab reads row vocab-1.  vocab > 0 (FD_EINVAL). */
int fd_embed_tokens_f16(const int64_t* ids, const void* tok_emb, const void* pos_emb, void* out,
                        int B, int L, int D, int vocab, void* stream);
/* ViT embeddings: out[b][0] = half_rn(cls + pos[0]), out[b][1 + p] = half_rn(patches[b (T-1) + p] + pos[1 + p]) (fp32 sums);
 * patches [B (T-1)][D], cls [D], pos [T][D], out [B T][D]; T > 1. */
int fd_vit_assemble_f16(const void* patches, const void* cls, const void* pos, void* out, int B,
                        int T, int D, void* stream);
/* diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0): t fp32 -> fp16 [B][dim]; sample b reads
 * t[b * t_stride], t_stride 1 (one timestep per sample) or 0 (one device scalar for the batch: the
 * denoising loop's timestep, refreshed between replays of a launch plan). */
int fd_timestep_embedding_f16(const float* t, int t_stride, void* out, int B, int dim, void* stream);
/* dst[r][0..cols) = src[r][0..cols) for fp16 matrices with row strides lds / ldd (elements);
 * cols, lds, ldd multiples of 8, pointers 16-byte aligned.  The CFG fan-out copies of the UNet. */
int fd_copy2d_f16(const void* src, int lds, void* dst, int ldd, int64_t rows, int cols, void* stream);
/* (ABI 11) dst[r * rows + i][0..cols) = src[i][0..cols) for r < rep, one launch: the CFG fan-out of the shared UNet prefix (B samples -> rep * B;
 * the reference feeds the replicated batch from the start, pipeline/guide.py:46-58).  Same alignment rules as fd_copy2d_f16. */
int fd_repeat_rows_f16(const void* src, int lds, void* dst, int ldd, int64_t rows, int cols, int rep, void* stream);
/* CompositeGuide region blend (reference composition/guide.py:86-98), NCHW fp32 [C][H][W]:
 * dst[:, oy:oy+sh, ox:ox+sw] += blend * (src - dst) on the same box.  oy, ox >= 0: the host
 * resolves Python's slice semantics (negative starts count from the end of the axis) first;
 * the box is clipped to the canvas (nothing left, or sh / sw <= 0: FD_OK and no launch).  Per element d + blend (s - d) as three
 * separately rounded fp32 operations; src is read inside the clipped box only. */
int fd_region_blend_f32(float* dst, const float* src, int C, int H, int W, int oy, int ox, int sh,
                        int sw, float blend, void* stream);
/* CompositeGuide on the device loop, one launch per step: the region blend of composition/guide.py:86-98
 * with a per-cell weight, the CFG combine of pipeline/guide.py:59-63 and, with do_step, the DDIM update of
 * fd_cfg_ddim_step_f32 (same coefficients, eps- or v-prediction).  eps_nhwc: UNet output, E = cfg + 1 + n
 * blocks of B samples in rep-major order ([uncond] [background] [entity 0] ... [entity n-1]); row
 * (r * B + b) * HW + p, row stride ld.  weights: fp32 [n][HW] (shared by the B samples), 0 outside an
 * entity's box.  Per (b, c, p): v = bg; for each k with w_k(p) != 0: v += w_k(p) * (ent_k - v); with cfg
 * v = u + g (v - u).  eps_out (optional): NCHW fp32 [B][C][HW]; x: NCHW fp32, updated in place when do_step. */
int fd_composite_step_f32(float* x, const float* eps_nhwc, const float* weights, float* eps_out, int B, int C,
                          int HW, int ld, int n_entities, int cfg, float guidance, float c1, float c2, float c3,
                          float c4, int v_prediction, int do_step, void* stream);
/* Masked img2img (inpainting) on the device loop, one launch per step: outside the mask the latents are put back on
 * the clean init latents z0, re-noised with the call's noise to the level of the step's output.  Per NCHW element,
 * with m = mask[p] (fp32 [HW], shared by the C channels and the B samples):
 *   known = k1 z0 + k2 noise ;  x <- x' where m == 1, known where m == 0, known + m (x' - known) otherwise
 * (fp32, every operation rounded separately; the two exact branches make an all-ones mask give the unmasked step's
 * bits and an all-zeros mask those of fd_axpby_f32(z0, noise, k1, k2)).  eps_nhwc != NULL (fused form): x' is the
 * CFG + DDIM (eta = 0) update of fd_cfg_ddim_step_f32 with do_step -- same arguments, same bits -- of the x read.
 * eps_nhwc == NULL (blend only): x' is x as it stands (any scheduler, any guide); ld, cfg, guidance, c1..c4 and
 * v_prediction are ignored.  x, z0, noise: NCHW fp32 [B][C][HW]; x is updated in place and may alias neither. */
int fd_cfg_ddim_masked_step_f32(float* x, const float* eps_nhwc, const float* z0, const float* noise, const float* mask,
                                int B, int C, int HW, int ld, int cfg, float guidance, float c1, float c2, float c3,
                                float c4, int v_prediction, float k1, float k2, void* stream);
/* DPM-Solver++ (2M) on the device loop, one launch per step (additive, ABI 12): replaces the CFG combine of
 * pipeline/guide.py:59-63 (fd_cfg_ddim_step_f32 without do_step) and the chain of fd_axpby_f32 launches a multistep
 * `scheduler.step` would issue (x0, the update, one per history term), plus the blend-only launch of
 * fd_cfg_ddim_masked_step_f32 for a masked request.  Per NCHW element, every operation a separately rounded fp32 one:
 *   e = u + g (t - u) (cfg) ;  m0 = p x + q e -> m0_out ;  x' = a x + w0 m0 ;  x' = x' + w1 m1 (m1 != NULL)
 *   mask != NULL: known = k1 z0 + k2 noise ;  x <- x' where m == 1, known where m == 0, known + m (x' - known) otherwise
 * x: NCHW fp32 [B][C][HW], updated in place.  eps_nhwc: the UNet output [(cfg ? 2 : 1) * B][HW][ld] fp32, unconditional
 * half first, as fd_cfg_ddim_step_f32 reads it (an NCHW eps: B * C one-channel planes, C = 1, ld = 1).  m0_out, m1: NCHW
 * fp32 history slots (this step's data prediction x0 and the previous step's; m1 == NULL is the first-order step);
 * m0_out may alias neither x nor m1.  (p, q): x0 from (x, eps) -- (1/alpha_s, -sigma_s/alpha_s) for eps-prediction,
 * (alpha_s, -sigma_s) for v-prediction.  mask: fp32 [HW] with z0, noise NCHW fp32 that do not alias x (mask == NULL: z0,
 * noise, k1, k2 are ignored). */
int fd_cfg_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1, const float* z0,
                              const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                              float p, float q, float a, float w0, float w1, float k1, float k2, void* stream);
/* PLMS and K-LMS on the device loop, one launch per step (additive; FD_ABI_VERSION stays 12): replaces, for the scheduler the
 * reference's Runner passes its pipeline (utils.py:70: PNDM in its PLMS form) and for LMSDiscreteScheduler, the CFG combine
 * of pipeline/guide.py:59-63 (fd_cfg_ddim_step_f32 without do_step), the chain of fd_axpby_f32 launches of
 * `scheduler.step` (pipeline/flex.py:280-285), K-LMS's sigma input scaling (pipeline/flex.py:270-274) and the blend-only
 * launch of a masked request.  Per NCHW element, every operation a separately rounded fp32 one, every scalar the float the
 * fd_axpby_f32 call it replaces received:
 *   e = u + g (t - u) (cfg; otherwise the one eps row)
 *   form 0, PLMS (history rows h1..h3: earlier guided eps, newest first; n_prev of them are read):
 *     h_out <- e (h_out != NULL) ;  x_keep_out <- x (x_keep_out != NULL) ;  xs = x_src ? x_src : x
 *     E = e (n_prev == 0) | w0 e + w1 h1, then E = 1 E + wk hk for k = 2..n_prev ;  x' = a0 xs + a1 E     (a0, a1) = (cs, ce)
 *     (PLMS's second call on the repeated timestep: n_prev = 1, (w0, w1) = (0.5, 0.5), h_out NULL, x_src the kept sample)
 *   form 1, K-LMS (history rows: earlier derivatives), (a0, a1, a2) = (-sigma, 1/sigma, -1/sigma), (w0..w3) = c0..c3:
 *     x0 = 1 x + a0 e ;  d = a1 x + a2 x0 ;  h_out <- d ;  x' = 1 x + w0 d, then x' = 1 x' + wk hk for k = 1..n_prev
 *   mask != NULL: known = k1 z0 + k2 noise ;  x <- x' where m == 1, known where m == 0, known + m (x' - known) otherwise
 *   x_scaled_out <- scale x + 0 0 (x_scaled_out != NULL: fd_axpby_f32(x, NULL, scale, 0), the next K-LMS model input)
 * x: NCHW fp32 [B][C][HW], updated in place; every other row has its shape.  eps_nhwc as fd_cfg_ddim_step_f32 reads it.
 * FD_EINVAL before any launch: x or eps_nhwc NULL; n_prev outside 0..3; one of the first n_prev history rows NULL; h_out or
 * x_keep_out aliasing x, each other or a row that is read (h1..h3, x_src, z0, noise); x_scaled_out aliasing x; form 1 with
 * x_src, with x_keep_out or without h_out; the mask rules of fd_cfg_multistep_step_f32. */
int fd_cfg_linear_multistep_step_f32(float* x, const float* eps_nhwc, int form, int n_prev, const float* h1, const float* h2,
                                     const float* h3, float* h_out, float* x_keep_out, const float* x_src,
                                     float* x_scaled_out, const float* z0, const float* noise, const float* mask, int B, int C,
                                     int HW, int ld, int cfg, float guidance, float w0, float w1, float w2, float w3, float a0,
                                     float a1, float a2, float scale, float k1, float k2, void* stream);
/* Stochastic sampling on the device loop (additive; FD_ABI_VERSION stays 12): the step noise the reference's
 * scheduler draws when `eta` is forwarded to it (pipeline/flex.py:247-251) comes from a counter-based normal stream
 * generated inside the step kernel, never from a tensor.  Value z of flat element i of a launch:
 *   key = (seed & 0xffffffff, seed >> 32) ;  sample = sample_offset + i / per ;  j = i % per
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (j >> 2, sample, draw, stream), key)      (Salmon et al. 2011)
 *   (wa, wb) = (w0, w1) for j % 4 in {0, 1}, (w2, w3) for j % 4 in {2, 3}
 *   u = ((wa >> 8) + 1) 2^-24 ;  f = (wb >> 8) 2^-23 ;  r = sqrt(-2 log u) ;  z = r cospi(f) (j even) | r sinpi(f) (j odd)
 * in fp32 (u, f exact; log, sincospi the accurate library functions; the products and the root separately rounded), so
 * |z| < 5.77.  `per` is the number of elements of one sample (C * HW of the real latent) whatever (B, C) view the call
 * uses; it must divide B * C * HW; sample_offset >= 0 is the global index of the call's first sample (a rank's or a
 * batch's offset), draw >= 0 the step's index in the scheduler's timestep list; stream 0 is the step noise, stream 1 the
 * stand-alone fill.  A value does not depend on the vector width, the batch split or the view.
 * fd_philox_normal_f32: out[0..n) = z (n need not be a multiple of per; any alignment). */
int fd_philox_normal_f32(float* out, int64_t n, int per, uint64_t seed, int64_t sample_offset, int draw, int noise_stream,
                         void* stream);
/* fd_cfg_ddim_masked_step_f32's fused form with the mask trio optional (mask == NULL: z0, noise, k1, k2 ignored) and
 * DDIM's eta > 0 term: x' = c3 x0 + c4 e ;  x' = x' + sigma z (skipped when sigma == 0: the bits of the entry points
 * above) ;  then the blend.  c4 = sqrt(1 - a_prev - sigma^2) comes from the host.  eps_nhwc must not be NULL. */
int fd_cfg_ddim_noise_step_f32(float* x, const float* eps_nhwc, const float* z0, const float* noise, const float* mask,
                               int B, int C, int HW, int ld, int cfg, float guidance, float c1, float c2, float c3,
                               float c4, int v_prediction, float k1, float k2, float sigma, uint64_t seed,
                               int64_t sample_offset, int per, int draw, void* stream);
/* fd_cfg_multistep_step_f32 plus the SDE-DPM-Solver++ term: ... x' = a x + w0 m0 (+ w1 m1) ;  x' = x' + sn z (skipped
 * when sn == 0) ;  m0_out holds m0 ;  then the blend. */
int fd_cfg_multistep_noise_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1, const float* z0,
                                    const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg,
                                    float guidance, float p, float q, float a, float w0, float w1, float k1, float k2,
                                    float sn, uint64_t seed, int64_t sample_offset, int per, int draw, void* stream);
/* Guidance rescale on the device loop (additive; FD_ABI_VERSION stays 12): replaces diffusers' `rescale_noise_cfg` (Lin et
 * al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", sec. 3.4) applied to the CFG combine of the
 * reference's pipeline/guide.py:59-63 -- several torch reductions per step -- by one launch that also is the step.  CFG is
 * implied: eps_nhwc has 2 * B * HW rows (unconditional half first), row stride ld >= C; the ld - C padding columns are
 * never read.  Per sample b, over its n = C * HW elements, t the conditional value and e = u + g (t - u) the separately
 * rounded fp32 value of the entry points above:
 *   M2(v) = sum v^2 - (sum v)^2 / n  (the four sums in fp64) ;  f_b = float(rescale sqrt(max(M2(t), 0) / M2(e)) + (1 - rescale))
 * evaluated in fp64 and rounded once; f_b = 1 when rescale == 0 or M2(e) <= 0.  The n - 1 of the two unbiased standard
 * deviations cancels, so f_b is diffusers' factor.  Then, per element:  e = f_b e (one fp32 product) -> eps_out ;  the
 * update ;  + sigma z ;  the blend ;  -> x -- everything after the product the arithmetic of the entry points above, so
 * rescale == 0 gives their bits.  One workgroup per sample computes the statistics and runs the step (k_latent_step_rescale,
 * csrc/step.hip): no atomics, no workspace, the same bits on every run.  scale_out (optional): fp32 [B], receives f_b.
 * rescale outside [0, 1] is FD_EINVAL.
 * fd_cfg_rescale_ddim_step_f32: the plain, masked (mask != NULL: z0, noise, k1, k2 as fd_cfg_ddim_masked_step_f32) and
 * stochastic (sigma != 0: z as fd_cfg_ddim_noise_step_f32 with per = C * HW) DDIM steps.  do_step == 0 is the combine-only
 * form: f_b e -> eps_out (required), x may be NULL, mask must be NULL and sigma 0. */
int fd_cfg_rescale_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* scale_out, const float* z0,
                                 const float* noise, const float* mask, int B, int C, int HW, int ld, float guidance,
                                 float rescale, float c1, float c2, float c3, float c4, int v_prediction, int do_step,
                                 float k1, float k2, float sigma, uint64_t seed, int64_t sample_offset, int draw,
                                 void* stream);
/* fd_cfg_multistep_step_f32 / fd_cfg_multistep_noise_step_f32 (sn != 0, per = C * HW) on the rescaled e: DPM-Solver++ (2M)
 * and its SDE form. */
int fd_cfg_rescale_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1, float* scale_out,
                                      const float* z0, const float* noise, const float* mask, int B, int C, int HW, int ld,
                                      float guidance, float rescale, float p, float q, float a, float w0, float w1,
                                      float k1, float k2, float sn, uint64_t seed, int64_t sample_offset, int draw,
                                      void* stream);
/* Region composition under every scheduler, one launch per step (additive; FD_ABI_VERSION stays 12): the steps of
 * fd_cfg_ddim_noise_step_f32, fd_cfg_multistep_noise_step_f32 and fd_cfg_linear_multistep_step_f32 with the entity blend of
 * fd_composite_step_f32 as the source of the guided e -- the same kernel (k_latent_step, csrc/step.hip), the arguments of the
 * sibling plus `weights, n_entities`.  eps_nhwc holds (cfg + 1 + n_entities) * B * HW rows, row stride ld >= C, in
 * fd_composite_step_f32's rep-major order ([uncond] [background] [entity 0] ...: block r, sample b, pixel p -> row
 * (r * B + b) * HW + p); weights: fp32 [n_entities][HW], shared by the B samples.  With first = cfg ? 1 : 0 and
 * blk = B * HW * ld, element (b, c, p), row = (b * HW + p) * ld + c, every operation a separately rounded fp32 one:
 *   v = eps[first * blk + row]
 *   for k = 0 .. n_entities - 1, ascending:  w = weights[k * HW + p] ;  w != 0:  v = v + w (eps[(first + 1 + k) * blk + row] - v)
 *   e = cfg ? u + g (v - u), u = eps[row] : v
 * (no exact branch for w == 1: the lerp is the contract, as in fd_composite_step_f32), then everything the sibling does with
 * its e.  n_entities == 0 (weights ignored): the sibling's kernel and bits.  float4 accesses need HW % 4 == 0 and 16-byte
 * bases, weights included; otherwise the scalar kernel runs.  FD_EINVAL before any launch: the sibling's cases, n_entities < 0,
 * weights NULL with n_entities > 0.
 * fd_composite_ddim_step_f32: DDIM; eps_out (optional, NCHW fp32) receives e; mask != NULL: the known-region blend (z0, noise,
 * k1, k2 as fd_cfg_ddim_masked_step_f32); sigma != 0: x' += sigma z from the stream at (seed, sample_offset, per, draw), which
 * are checked only then.  sigma == 0 and mask == NULL: the bits of fd_composite_step_f32 with do_step. */
int fd_composite_ddim_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities, float* eps_out,
                               const float* z0, const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg,
                               float guidance, float c1, float c2, float c3, float c4, int v_prediction, float k1, float k2,
                               float sigma, uint64_t seed, int64_t sample_offset, int per, int draw, void* stream);
/* DPM-Solver++ (2M), orders 1 (m1 == NULL) and 2; sn == 0 is the ODE form (per and draw are checked as the sibling checks them). */
int fd_composite_multistep_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities, float* m0_out,
                                    const float* m1, const float* z0, const float* noise, const float* mask, int B, int C,
                                    int HW, int ld, int cfg, float guidance, float p, float q, float a, float w0, float w1,
                                    float k1, float k2, float sn, uint64_t seed, int64_t sample_offset, int per, int draw,
                                    void* stream);
/* PLMS (form 0) and K-LMS (form 1), n_prev 0..3, every row and rule of fd_cfg_linear_multistep_step_f32. */
int fd_composite_linear_multistep_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities, int form,
                                           int n_prev, const float* h1, const float* h2, const float* h3, float* h_out,
                                           float* x_keep_out, const float* x_src, float* x_scaled_out, const float* z0,
                                           const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg,
                                           float guidance, float w0, float w1, float w2, float w3, float a0, float a1, float a2,
                                           float scale, float k1, float k2, void* stream);
/* UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"; additive;
 * FD_ABI_VERSION stays 12): the corrector of the previous step's sample and the predictor of the next one in ONE launch of
 * k_latent_step (csrc/step.hip), with the coefficients of UniPCMultistepScheduler.step_coefficients.  x, eps_nhwc, z0, noise,
 * mask, B, C, HW, ld, cfg, guidance, k1, k2 as fd_cfg_multistep_step_f32.  h1, h2, h3: the x0 rows of the earlier steps, newest
 * first (NCHW fp32); x_last: the corrected sample the previous step's predictor started from.  Per element, every operation a
 * separately rounded fp32 one, every sum in the order written:
 *   e = the guided eps -> eps_out (optional, NCHW fp32)
 *   m = p x + q e -> m_out                                          (x: the sample the model saw)
 *   xc = cx x_last + cn m, then xc += c_k h_k for k = 1..c_order     (c_order == 0: no corrector, xc = x)
 *   xc -> x_keep_out
 *   x' = ax xc + w0 m, then x' += w_k h_k for k = 1..p_order - 1
 *   the known-region blend (mask != NULL) -> x
 * A row is read only at k <= max(c_order, p_order - 1) and x_last only with c_order >= 1; what is not read may be NULL, hold
 * anything and have any alignment.  The kept sample is updated in place: x_keep_out may be x_last (a thread reads and writes
 * only its own elements); no other output may be a buffer the launch reads or another output.  At c_order == 0 and
 * p_order <= 2 the bits are fd_cfg_multistep_step_f32's on (p, q, ax, w0, w1).  FD_EINVAL before any launch: c_order outside
 * 0..3, p_order outside 1..3, a NULL row at a used order, NULL x, eps_nhwc, m_out or x_keep_out, NULL x_last with a corrector,
 * the aliasing above, the size and mask rules of the siblings. */
int fd_cfg_unipc_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* m_out, const float* h1, const float* h2,
                          const float* h3, const float* x_last, float* x_keep_out, const float* z0, const float* noise,
                          const float* mask, int B, int C, int HW, int ld, int cfg, float guidance, int c_order, int p_order,
                          float p, float q, float cx, float cn, float c1, float c2, float c3, float ax, float w0, float w1,
                          float w2, float k1, float k2, void* stream);
/* ... with guidance rescale (CFG implied; one workgroup per sample, as fd_cfg_rescale_multistep_step_f32): e = f_b e before m.
 * rescale == 0: the bits of fd_cfg_unipc_step_f32 with cfg. */
int fd_cfg_rescale_unipc_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* m_out, const float* h1,
                                  const float* h2, const float* h3, const float* x_last, float* x_keep_out, float* scale_out,
                                  const float* z0, const float* noise, const float* mask, int B, int C, int HW, int ld,
                                  float guidance, float rescale, int c_order, int p_order, float p, float q, float cx, float cn,
                                  float c1, float c2, float c3, float ax, float w0, float w1, float w2, float k1, float k2,
                                  void* stream);
/* ... with the entity blend of the composite forms above as the source of e.  n_entities == 0: fd_cfg_unipc_step_f32's kernel
 * and bits. */
int fd_composite_unipc_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities, float* eps_out,
                                float* m_out, const float* h1, const float* h2, const float* h3, const float* x_last,
                                float* x_keep_out, const float* z0, const float* noise, const float* mask, int B, int C, int HW,
                                int ld, int cfg, float guidance, int c_order, int p_order, float p, float q, float cx, float cn,
                                float c1, float c2, float c3, float ax, float w0, float w1, float w2, float k1, float k2,
                                void* stream);
/* Context schedules (additive; FD_ABI_VERSION stays 12): out[i] = half_rn(a[i] + w * (b[i] - a[i])) on contiguous fp16 buffers of n
 * elements -- the subtraction, the product and the sum three separately rounded fp32 operations (no FMA), one rounding to half.
 * w == 0 stores a's bits, w == 1 stores b's bits; a[i] == b[i] gives a[i] for every w (a zero of either sign: +0 unless w is 0 or 1).
 * The cross-attention projections are linear, so the K, V^T and packed images of a blended context are this blend of the
 * cached projections of its keyframes (UNet2DConditionModel.blend_context).  16-byte accesses when a, b and out are all 16-byte
 * aligned, a scalar kernel otherwise; out may alias neither input (FD_EINVAL, as are NULL pointers and n <= 0). */
int fd_lerp_f16(const void* a, const void* b, void* out, int64_t n, float w, void* stream);
/* Windowed (MultiDiffusion, Bar-Tal et al. 2023) sampling on the device loop (additive; FD_ABI_VERSION stays 12): a canvas
 * latent (B, C, H, W) is covered by ny x nx overlapping windows (h, w) of the model's own size, the UNet runs on all of them
 * as one batch, and the guided predictions are averaged where windows overlap before one step on the canvas.  The grid is
 * plain ints: along an axis of extent S, window s, stride d (1 <= d <= s <= S) there are n = ceil((S - s) / d) + 1 <= 16
 * windows at offsets o_i = min(i d, S - s) (the last snapped to the edge); ny, nx must be those counts.  Window (iy, ix) is
 * w = iy nx + ix of Wn = ny nx; sample b, window w is row b Wn + w of the window batch.  Anything else is FD_EINVAL.
 * fd_window_gather_f32: windows (B Wn, C, h, w) NCHW fp32 <- the canvas cells under each window. */
int fd_window_gather_f32(const float* canvas, float* windows, int B, int C, int H, int W, int h, int w, int stride_y,
                         int stride_x, int ny, int nx, void* stream);
/* One launch per step after the UNet.  eps_nhwc: the UNet output, fp32, row ((r B Wn + b Wn + w) h w + p), r = 0
 * unconditional / 1 conditional (r = 0 only without cfg), p = ly w + lx, row stride ld >= C.  Per canvas cell (b, y, x) and
 * channel, every operation a separately rounded fp32 one:
 *   acc = 0, wsum = 0 ;  for every window covering the cell, in ascending (iy, ix) order:
 *     g_w = u_w + guidance (t_w - u_w) (cfg; otherwise the one row)
 *     blend 0 (uniform): acc = acc + g_w ;  blend 1 (tent): wgt = min(ly + 1, h - ly) min(lx + 1, w - lx) (an exact integer),
 *     acc = acc + wgt g_w, wsum = wsum + wgt
 *   e = g_w where exactly one window covers the cell (an exact branch), else acc / count (uniform) | acc / wsum (tent)
 *   eps_out (optional, NCHW fp32 [B][C][H][W]) <- e ;  do_step: x <- x' = the DDIM (eta = 0) update of fd_cfg_ddim_step_f32
 *   (same coefficients, eps- or v-prediction) ;  windows_out (optional, needs do_step) <- x' in the cell of every covering
 *   window -- the next step's UNet input; each window cell has one source, so there are no atomics.
 * do_step == 0 is the combine-only form: eps_out is required and windows_out must be NULL.  On a one-window grid the uniform
 * form gives the bits of fd_cfg_ddim_step_f32. */
int fd_window_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out, int B, int C, int ld, int H,
                       int W, int h, int w, int stride_y, int stride_x, int ny, int nx, int blend, int cfg, float guidance,
                       float c1, float c2, float c3, float c4, int v_prediction, int do_step, void* stream);
/* The other schedulers, the step noise and the mask of a windowed request in that same one launch (additive; FD_ABI_VERSION
 * stays 12).  Both are fronts of fd_window_step_f32's kernel and take its grid, eps_nhwc, blend, cfg and guidance; per canvas
 * cell (b, y, x) and channel, o the NCHW canvas element ((b C + c) H + y) W + x, every operation a separately rounded fp32 one:
 *   e as fd_window_step_f32 (-> eps_out, fd_window_ddim_step_f32 only, optional)
 *   the update: DDIM (fd_cfg_ddim_step_f32's, c1..c4 of step_coefficients(t, eta)) | multistep (fd_cfg_multistep_step_f32's:
 *     d0 = p x + q e ;  x' = a x + w0 d0 (+ w1 m1[o], m1 != NULL: order 2))
 *   x' = x' + sn z (sigma | sn != 0): z the counter-based normal stream (fd_philox_normal_f32) of CANVAS element o --
 *     per = C H W, sample = sample_offset + b, draw, stream 0.  The noise is a function of the canvas element and never of the
 *     window grid: it equals the fill of a (B, C, H, W) tensor at that element.  sigma | sn == 0: no noise stage, seed,
 *     sample_offset and draw are ignored.
 *   m0_out[o] = d0 (multistep; the history holds the noise-free data prediction; m0_out and m1 are canvas-shaped)
 *   mask != NULL ([H][W] over the canvas, shared by the samples; needs z0 and noise, canvas-shaped):
 *     x' = the known-region blend of fd_cfg_ddim_masked_step_f32 on (x', z0[o], noise[o], mask[y W + x], k1, k2)
 *   x[o] = x' ;  windows_out (optional) <- the same, blended value in the cell of every covering window
 * With neither mask nor sigma fd_window_ddim_step_f32 gives the bits of fd_window_step_f32(do_step = 1); on a one-window grid
 * both give the bits of fd_cfg_ddim_noise_step_f32 / fd_cfg_multistep_[noise_]step_f32 on the same operands; either equals the
 * combine-only form followed by that non-windowed step on B C one-channel planes and fd_window_gather_f32.
 * FD_EINVAL: the grid's errors; NULL x, eps_nhwc or m0_out; m0_out aliasing x or m1; mask without z0 / noise; z0 / noise
 * aliasing x; eps_out aliasing x; windows_out aliasing any other buffer of the call; with noise, C H W past 2^31, a negative
 * sample_offset or draw, or sample_offset + B past 2^32. */
int fd_window_ddim_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out, const float* z0,
                            const float* noise, const float* mask, int B, int C, int ld, int H, int W, int h, int w,
                            int stride_y, int stride_x, int ny, int nx, int blend, int cfg, float guidance, float c1, float c2,
                            float c3, float c4, int v_prediction, float k1, float k2, float sigma, uint64_t seed,
                            int64_t sample_offset, int draw, void* stream);
int fd_window_multistep_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* m0_out, const float* m1,
                                 const float* z0, const float* noise, const float* mask, int B, int C, int ld, int H, int W,
                                 int h, int w, int stride_y, int stride_x, int ny, int nx, int blend, int cfg, float guidance,
                                 float p, float q, float a, float w0, float w1, float k1, float k2, float sn, uint64_t seed,
                                 int64_t sample_offset, int draw, void* stream);
/* Region composition over windows, one launch per step (additive; FD_ABI_VERSION stays 12): the fronts above with the entity
 * blend of fd_composite_step_f32 as the source of the guided prediction of every covering window -- the same kernel
 * (k_window_step, csrc/window.hip), the arguments of the sibling plus `weights, n_entities`.  Entities live on the CANVAS:
 * weights is fp32 [n_entities][H][W] over the canvas latent, shared by the B samples, read at the canvas cell (y, x); a cell's
 * weight does not depend on the window grid.  The UNet batch is the window batch (B Wn latent rows, sample b, window w at row
 * b Wn + w) under E = cfg + 1 + n_entities context blocks in rep-major order ([uncond] [background] [entity 0] ...): in
 * eps_nhwc block r, sample b, window w, local cell (ly, lx) is row ((r B + b) Wn + w) h w + ly w + lx, row stride ld >= C.
 * With first = cfg ? 1 : 0, per canvas cell (b, y, x) and channel, every operation a separately rounded fp32 one:
 *   for every window covering the cell, in ascending (iy, ix) order, R_r its row in block r:
 *     v = eps[R_first]
 *     for k = 0 .. n_entities - 1, ascending:  wk = weights[(k H + y) W + x] ;  wk != 0:  v = v + wk (eps[R_(first + 1 + k)] - v)
 *       (the wk == 0 skip is an exact branch and there is none for wk == 1: the lerp is the contract, as in
 *       fd_composite_step_f32)
 *     g_w = cfg ? u + guidance (v - u), u = eps[R_0] : v
 *     acc, wsum as fd_window_step_f32 (uniform | tent)
 *   e = g_w where exactly one window covers the cell, else acc / count | acc / wsum, as fd_window_step_f32
 *   then every stage of the sibling in its order: eps_out, the update, + sigma z at the canvas element, m0_out, the
 *   known-region blend, x, and the cell of every covering window in windows_out.
 * Blend and CFG are linear and the weights do not depend on the window, so this equals averaging each block first and blending
 * afterwards up to rounding; per window first keeps one accumulator set instead of E.  The rows of an (entity, window) pair
 * that do not intersect are read nowhere (weight 0).  n_entities == 0 (weights ignored): the sibling's kernel and bits.  A
 * one-window grid gives the bits of fd_composite_ddim_step_f32 / fd_composite_multistep_step_f32; an entity that is 0 on the
 * whole canvas those of the call without its block.  float4 loads along the channels under the sibling's rule (C % 4 == 0,
 * ld % 4 == 0, eps_nhwc 16-byte aligned); the weights of a cell are scalar loads, once per cell.
 * FD_EINVAL before any launch: the sibling's cases; n_entities < 0 or above 16; weights NULL with n_entities > 0; weights
 * aliasing windows_out, x, eps_out or m0_out.
 * fd_window_composite_step_f32 replaces fd_window_step_f32 and fd_window_ddim_step_f32 for a composition: do_step == 0 is the
 * combine-only form (eps_out required, windows_out, mask NULL and sigma 0; x may be NULL); do_step == 1 the DDIM step with the
 * optional sigma z term and the optional known-region blend. */
int fd_window_composite_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out, const float* weights,
                                 int n_entities, const float* z0, const float* noise, const float* mask, int B, int C, int ld,
                                 int H, int W, int h, int w, int stride_y, int stride_x, int ny, int nx, int blend, int cfg,
                                 float guidance, float c1, float c2, float c3, float c4, int v_prediction, float k1, float k2,
                                 float sigma, uint64_t seed, int64_t sample_offset, int draw, int do_step, void* stream);
/* fd_window_composite_multistep_step_f32 replaces fd_window_multistep_step_f32 for a composition: DPM-Solver++ (2M), orders 1
 * (m1 == NULL) and 2, sn == 0 the ODE form. */
int fd_window_composite_multistep_step_f32(float* x, float* windows_out, const float* eps_nhwc, const float* weights,
                                           int n_entities, float* m0_out, const float* m1, const float* z0, const float* noise,
                                           const float* mask, int B, int C, int ld, int H, int W, int h, int w, int stride_y,
                                           int stride_x, int ny, int nx, int blend, int cfg, float guidance, float p, float q,
                                           float a, float w0, float w1, float k1, float k2, float sn, uint64_t seed,
                                           int64_t sample_offset, int draw, void* stream);
/* Tiled VAE decode / encode (additive; FD_ABI_VERSION stays 12): the VAE runs on a batch of overlapping tiles of the model's
 * own size -- the grid of fd_window_gather_f32, same rule, same batch order -- and this one launch puts the tile outputs
 * together.  tiles: NHWC fp32, the row of (sample b, tile t = iy nx + ix, ly, lx) is ((b ny nx + t) h + ly) w + lx, row
 * stride ld >= C.  out: (B, C, H, W) NCHW fp32.  All extents are in the units of out (pixels for a decode, latent cells for an
 * encode).  Per canvas element (b, c, y, x), every operation a separately rounded fp32 one:
 *   acc = 0, wsum = 0 ;  for every tile covering the element, in ascending (iy, ix) order, v its value there:
 *     wgt = r_y(ly) r_x(lx),  r(l) = min(l + 1, E - l, F), E the tile extent and F the feather of that axis (small integers:
 *     the weight is exact) ;  acc = acc + wgt v ;  wsum = wsum + wgt
 *   u = v where exactly one tile covers the element (an exact branch), else acc / wsum
 *   y = u a + b (a product, then a sum) ;  clamp01: y = min(max(y, 0), 1)
 * F = 1 is the plain average, F >= E / 2 the full tent.  With a a power of two a one-tile grid gives the bits of
 * fd_nhwc_f32_to_nchw_f32.  One thread owns one canvas pixel and its C channels; a tile pixel is read as float4 loads when
 * ld % 4 == 0 and tiles is 16-byte aligned, as scalars otherwise.  No atomics: every element of out is written exactly once.
 * FD_EINVAL: the grid's errors; NULL tiles or out; ld < C; a feather below 1; out overlapping tiles. */
int fd_tile_blend_f32(const float* tiles, float* out, int B, int C, int ld, int H, int W, int h, int w, int stride_y,
                      int stride_x, int ny, int nx, int feather_y, int feather_x, float a, float b, int clamp01, void* stream);
/* Hires two-pass sampling, the bridge between the passes (additive; FD_ABI_VERSION stays 12; csrc/resample.hip): ONE launch
 * resamples low-resolution latents onto a canvas, noises them to the start level of the second pass and, on a windowed canvas,
 * writes the first window batch.  src: (src_samples, C, hs, ws) NCHW fp32, src_samples 1 (one latent shared by the B samples,
 * each with its own noise) or B.  x: (B, C, H, W) NCHW fp32, H >= hs and W >= ws (FD_ESHAPE otherwise: downscaling would need
 * the antialias filter widened).  Per canvas cell (b, y, x) and channel, o = ((b C + c) H + y) W + x, every operation a
 * separately rounded fp32 one:
 *   r = sum over the row taps jy (ascending) of wy[jy] (sum over the column taps jx (ascending) of wx[jx] src[b mod src_samples][c][jy][jx]),
 *       each sum starting at its first product (no zero seed)
 *   z = noise[o] (noise != NULL) | the counter-based normal (fd_philox_normal_f32) of canvas element o: per = C H W,
 *       sample = sample_offset + b, draw, noise_stream -- the fill of a (B, C, H, W) tensor at that element | 0 when k2 == 0
 *       (no noise stage: noise, seed, sample_offset, draw and noise_stream are ignored)
 *   x[o] = k1 r + k2 z (two products, one sum): the bits of fd_axpby_f32(r, z, k1, k2), which is scheduler.add_noise
 *   windows_out (optional) <- the same value in the cell of every covering window of the grid (h, w, stride_y, stride_x, ny, nx):
 *       fd_window_gather_f32's rule, checks and layout; each window cell has one source, so there are no atomics.  With
 *       windows_out == NULL the six grid ints are ignored.
 * The taps of output index i along an axis n_in -> n_out (align_corners = False conventions):
 *   n_out == n_in: the one tap j = i with weight 1 (an exact branch: the identity in every mode)
 *   mode 0 (nearest): the one tap j = ((2 i + 1) n_in) / (2 n_out) in integer arithmetic, weight 1
 *   mode 1 (bilinear, S = 1, f the triangle 1 - |t|) and mode 2 (bicubic, S = 2, f the Keys cubic with a = -0.5:
 *   ((1.5 t - 2.5) t) t + 1 for |t| < 1, (((t - 5) t + 8) t - 4) (-0.5) for |t| < 2, else 0): the filters of torch's
 *   interpolate(..., antialias=True), which is the reference's composition/guide.py:27-29 --
 *     c = (n_in / n_out) (i + 0.5) ;  j in [max(0, floor(c - S + 0.5)), min(n_in, floor(c + S + 0.5))) ;  f_j = f(j - c + 0.5)
 *     w_j = f_j / (f_lo + ... + f_hi-1)   (taps that fall off the axis are dropped, not clamped; at most 2 | 4 taps)
 *   c is the ratio of the integers m = n_in (2 i + 1) and d = 2 n_out: the two floors are exact integer divisions and the
 *   filter argument is the ONE rounded quotient (d j + n_out - m) / d of two exact integers, so a weight is accurate to an ulp
 *   of its argument whatever the extent of the axis (torch's own fp32 c loses ulp(c)).  The filter's Horner steps, the sum
 *   of the f_j (from f_lo on) and the quotients are separately rounded.
 *   NOT torch's non-antialiased bicubic (a = -0.75, clamped indices).
 * A cell's value depends on neither the grid nor the launch shape.  One thread owns one canvas cell and its C channels.
 * FD_EINVAL: NULL src or x; non-positive sizes; src_samples not in {1, B}; an unknown mode; the grid's errors when windows_out is
 * given; src, x, windows_out, noise overlapping; H or W past 2^24, cells past 2^31; with in-kernel noise (k2 != 0, noise == NULL) C H W past 2^31,
 * a negative sample_offset, draw or noise_stream, or sample_offset + B past 2^32. */
int fd_latent_upscale_noise_f32(const float* src, float* x, float* windows_out, const float* noise, int B, int src_samples,
                                int C, int hs, int ws, int H, int W, int h, int w, int stride_y, int stride_x, int ny, int nx,
                                int mode, float k1, float k2, uint64_t seed, int64_t sample_offset, int draw, int noise_stream,
                                void* stream);
/* Contiguous casts: fp32 -> fp16 rounds to nearest even (overflow to inf from 65520 on), fp16 -> fp32 is exact. */
int fd_cast_f32_to_f16(const float* x, void* y, int64_t n, void* stream);
int fd_cast_f16_to_f32(const void* x, float* y, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FLEXDIFFUSE_HIP_H */
