/*
 * npm_hip.h -- C ABI of the MI355X (gfx950) layer forward/backward hot path.
 *
 * This is the drop-in boundary.  The reference
 * (levendlee/np-modeling) is pure NumPy: it has no FFI, so every entry point below
 * replaces a NumPy call site instead of a native symbol; the site is cited as
 * reference file:line.  A maintainer binds these with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every function returns 0 on success or a
 *     non-zero hipError_t / NPM_E_* code, and npm_last_error() describes the failure.
 *   - One process drives one GPU: npm_init(device) binds the process to a device and
 *     creates the compute stream all launches go to.  Launches are asynchronous;
 *     npm_sync() / npm_d2h() are the synchronisation points.
 *   - ONE host thread per process: the library keeps process-global state (the device, its one compute
 *     stream, the caching pool, the math mode and tuning knobs, npm_last_error / npm_last_math /
 *     npm_last_attn_kernel) without locks.  Calls from several threads must be serialised by the caller;
 *     parallelism across GPUs is one process per GPU (np_modeling_amd/launch.py, include/npm_comm.h).
 *   - All tensors are fp32, row-major; "ld" is the row pitch in elements.
 *   - Device pointers come from npm_malloc (a stream-ordered caching pool).
 */
#ifndef NPM_HIP_H
#define NPM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NPM_ABI_VERSION 2      /* 2: npm_mha_core gained tile_summary .. summary_all_offset, npm_comm_exchange_stats last_allreduce_ms / dropped */

enum {
    NPM_OK = 0,
    NPM_E_NOT_INITIALIZED = 10001,
    NPM_E_BAD_ARGUMENT = 10002,
    NPM_E_UNSUPPORTED = 10003,
    NPM_E_NO_DEVICE = 10004
};

/* ---- runtime ------------------------------------------------------------ */
int npm_abi_version(void);
const char *npm_last_error(void);
int npm_device_count(int *count);
int npm_init(int device);                 /* idempotent for the same device */
int npm_shutdown(void);
int npm_device_name(char *buf, int len);
void *npm_stream(void);                   /* the hipStream_t launches go to */
int npm_sync(void);                       /* hipStreamSynchronize(compute stream) */

/* ---- memory: caching pool over hipMalloc --------------------------------- */
int npm_malloc(void **ptr, size_t bytes);
int npm_free(void *ptr);                  /* returns the block to the pool (stream-ordered reuse) */
int npm_pool_stats(size_t *bytes_in_use, size_t *bytes_reserved);
int npm_pool_trim(void);                  /* hipFree every cached block */
int npm_h2d(void *dst, const void *src, size_t bytes);   /* ordered after prior launches; returns when done */
int npm_d2h(void *dst, const void *src, size_t bytes);   /* ditto */
int npm_d2d(void *dst, const void *src, size_t bytes);   /* async on the compute stream */
int npm_fill_f32(float *dst, float value, size_t n);

/* ---- events (HIP events on the compute stream; used by bench.py) ---------- */
int npm_event_create(void **event);
int npm_event_destroy(void *event);
int npm_event_record(void *event);
int npm_event_sync(void *event);
int npm_event_elapsed_ms(void *start, void *stop, float *ms);

/* ---- GEMM: C = epilogue(alpha * op(A) op(B)) ------------------------------
 * Replaces np.matmul in layers/mlp.py:23,35,36 and every np.einsum contraction in
 * layers/attentions.py:88-117,129-188 (each is a flat or batched GEMM view).
 * fp32 operands on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulate.
 *
 *   trans_a == 0 : A is [M,K] (pitch lda)      trans_a == 1 : A is stored [K,M]
 *   trans_b == 0 : B is [K,N] (pitch ldb)      trans_b == 1 : B is stored [N,K]
 * Batches are indexed z = z0 * batch1 + z1 with operand offset z0*stride0 + z1*stride1
 * (lets [B,S,H,D] head slices be addressed without a transpose).
 */
enum {
    NPM_EPI_BIAS = 1,        /* + bias[n]                                  (mlp.py:24) */
    NPM_EPI_RESIDUAL = 2,    /* + residual[m,n] (may alias C: accumulate)  (transformer.py:39,53) */
    NPM_EPI_RELU_SAVE = 4,   /* aux[m,n] = v; C = max(v,0)                 (activations.py:14-15) */
    NPM_EPI_RELU_MASK = 8,   /* C = aux[m,n] >= 0 ? v : 0                  (activations.py:19) */
    NPM_EPI_RELU = 16,       /* C = max(v,0), pre-activation not kept (inference) */
    NPM_EPI_SOFTMAX_BWD = 32,/* C = alpha * aux[m,n] * (acc - rowvec[m]): softmax backward with the row term
                                sum_j dP_ij P_ij = dctx_i . ctx_i precomputed (activations.py:32-45, attentions.py:150-155) */
    NPM_EPI_ROWDOT = 128     /* C = acc (stored as is) AND rowdot[(n / 128) * m_total + i] += rowdot_scale * sum over the 128 columns
                                j of column block n / 128 of C[i, j] * aux[i, j]: the row term delta_i = dctx_i . ctx_i of the attention
                                backward (attentions.py:150-155, the Jacobian-vector product of Softmax.backward) per head of size
                                128, taken where dctx = dy wo is produced (attentions.py:136) instead of by a pass over dctx and
                                ctx.  `rowdot` ([n / 128, m]) must be ZERO on entry (two partial sums per element are added with
                                float atomics: commutative, so bitwise reproducible).  Plain product only: no other epilogue flag,
                                no batch, no split-K, n % 128 == 0, the LDS-DMA kernel's alignment rules; else NPM_E_UNSUPPORTED. */
};

typedef struct npm_gemm {
    int32_t trans_a, trans_b;
    int32_t m, n, k;
    int32_t batch0, batch1;              /* >= 1 each */
    const float *a; int64_t lda, stride_a0, stride_a1;
    const float *b; int64_t ldb, stride_b0, stride_b1;
    float *c;       int64_t ldc, stride_c0, stride_c1;
    float alpha;
    int32_t epilogue;                    /* NPM_EPI_* bit set */
    const float *bias;                   /* [n] */
    const float *residual; int64_t ldr;  /* same batch strides as C */
    float *aux; int64_t ldaux;           /* same batch strides as C */
    int32_t split_k;                     /* 0 = choose automatically, 1 = never split */
    const float *rowvec;                 /* [batch, m] per-row term of NPM_EPI_SOFTMAX_BWD */
    float *colsum;                       /* optional [batch1, n]: colsum[z1, j] = sum over z0 and rows of the stored C
                                            (the bias gradient np.sum(dy, axis=0), mlp.py:34 / attentions.py:190-197,
                                            taken in the producing GEMM's epilogue; fixed summation order) */
    float *bsum;                         /* optional [n]: bsum[j] = sum over k of B[k, j] -- the column sums of the
                                            second operand of a weight-gradient product x^T dy, i.e. the bias gradient
                                            that goes with it (mlp.py:34-35, attentions.py:129-135,190-197), taken from
                                            the B tiles the GEMM stages anyway.  Needs trans_b = 0, batch0 = batch1 = 1. */
    float *asum;                         /* optional [m]: asum[i] = sum over k of A[k, i] for a transposed A (trans_a = 1,
                                            stored [k, m]): the same for products written dproj^T x, whose bias gradient
                                            sums the FIRST operand (attentions.py:167-197).  Not together with bsum. */
    float *rowdot; float rowdot_scale;   /* NPM_EPI_ROWDOT (ABI version 2) */
} npm_gemm;

int npm_sgemm(const npm_gemm *g);

/* Tuning knobs for A/B experiments in one process (tools/gemm_bench.py --tune, NPM_TUNE=knob=value,...).
 * Defaults are the shipped configuration: LDS-DMA pipeline (2), tile-row groups of 8, buffer epilogue on,
 * convolution DMA on.  NPM_TUNE_GEMM_ABLATE is a timing-only diagnostic: it skips work and breaks results. */
enum {
    NPM_TUNE_GEMM_PIPELINE = 0,      /* 0 register-staged 2 barriers, 1 register-staged double buffer, 2 LDS-DMA */
    NPM_TUNE_GEMM_GROUP_M = 2,
    NPM_TUNE_GEMM_BUF_EPILOGUE = 3,
    NPM_TUNE_CONV_DMA = 4,
    NPM_TUNE_GEMM_WIDE_TILE = 5,     /* 128 x 256 block tile (8 waves) where n % 256 == 0: 0 never (default), 1 always, 2 NN / NT, 3 NT only */
    NPM_TUNE_LN_BWD_BLOCKS = 6,      /* blocks per CU of the LayerNorm backward grid (default 4) */
    NPM_TUNE_EW_GRID_CAP = 7,        /* max blocks of the grid-stride elementwise kernels (default 2^20) */
    NPM_TUNE_CONV_WGRAD_BLOCKS = 8,  /* grad_w split-K blocks per CU: 0 (default) best of 3 and 4, 3 / 4 pinned, 6 / 9 / 12 several generations of shorter K ranges (measured at C3: 14.44 -> 14.6-15.0 ms), -1 unbalanced ceil(3 CUs / tiles) */
    NPM_TUNE_GEMM_WAVE_PRIO = 9,     /* s_setprio 3 in the GEMM / conv block prologue (bit 0) and epilogue (bit 1) */
    NPM_TUNE_GEMM_MATH = 10,         /* same as npm_set_math */
    NPM_TUNE_ATTN_STAGGER = 11,      /* attention forward: bits 0-7 s_sleep(127) units one of the two blocks of a CU waits at its start (default 1; read by mha_fwd_kernel only: mha_fwd8_kernel, the default, does not sleep); bit 8 set: no pairing of query tiles under a tile summary */
    NPM_TUNE_CONV_WGRAD_FUSED = 13,  /* npm_conv2d_bwd_w_relu: 1 (default) ReLU backward inside the grad_w kernel, tile height picked (k*k*C0 of exactly three 192-row tiles: one block of twelve waves sharing the masked dy tile); 2 / 3 the same with 128- / 192-row tiles in four-wave blocks; 0 two passes */
    NPM_TUNE_ATTN_BWD16 = 14,        /* attention backward: 2 (default) mha_bwd8_kernel (8 waves on the 16x16x4 MFMA, one barrier per tile, every head size, both score modes, tile skipping) except head size 128 with saved scores and no tile summary, which runs mha_bwd16_kernel; 3 mha_bwd8_kernel always; 1 round 3's choice (mha_bwd16_kernel for head size 128 with saved scores, the 4-wave 32x32x2 kernel otherwise); 0 the 4-wave kernel always */
    NPM_TUNE_KSYNC = 15,             /* K tiles between the soft rendezvous of the co-resident split-K blocks of the fused Conv2D filter gradient: a power of two, default 128; 0 off */
    NPM_TUNE_CONV_KORDER = 16,       /* Conv2D forward / grad_x K loop: 1 (default) the k k taps of one 16-channel chunk back to back (the lines a tap fetched are still in L2 when its neighbour wants them: grad_x of C3 reads 13.8 instead of 82 GB past the L2s, +4 %), 0 taps outermost (kk = tap C + c) */
    NPM_TUNE_ATTN_FWD8 = 17,         /* attention forward: 2 mha_fwd8_kernel (8 waves per block on the 16x16x4 MFMA, four waves per SIMD) for every head size; 1 below head size 128 only; 0 the 4-wave 32x32x2 mha_fwd_kernel always */
    NPM_TUNE_GEMM_SPLIT_GENS = 18,   /* split-K of tall-K products (weight gradients): 1 (default) for A-heavy products that also sum A's columns, a K range longer than 768 K tiles is cut further when that makes whole generations of resident blocks (3 x 4 per CU: the packed q/k/v weight gradient 6.00 -> 5.71 ms); 0 one generation of three blocks per CU always (round 3) */
    NPM_TUNE_STREAM_NT = 12,         /* 1 (default): the HBM-bound kernels move tensors of >= 32 MB with the nontemporal cache hint; 0: default policy */
    NPM_TUNE_LN_NT_SPLIT = 19,       /* LayerNorm at d in (512, 1024]: backward mode + 4 * forward mode; a mode: 0 nontemporal hint on loads and stores, 1 on the loads only, 2 on the stores only.  Default 5: loads only in both (dx and z are read at once by the GEMMs behind them; measured inside the encoder step, profiles/r05_ln_nt_split.log) */
    NPM_TUNE_DECODE_SPLITS = 20,     /* npm_mha_decode_fwd: blocks the keys of one (batch, K / V head) are split over: 0 (default) automatic (npm_mha_decode_splits), n in 1 .. NPM_DECODE_MAX_SPLITS forced -- more splits than 16-key tiles leaves empty splits, which is allowed */
    NPM_TUNE_DECODE_NT = 21,         /* npm_mha_decode_fwd, the cache hint of the K / V loads (each byte is read once): 0 (default) nontemporal when the valid part of K is at least 32 MB (NPM_TUNE_STREAM_NT's rule), 1 always, 2 never; measured in tools/decode_bench.py */
    NPM_TUNE_SKINNY_SPLITS = 22,     /* npm_sgemm_skinny: blocks the K range of one 64-column strip is split over: 0 (default) automatic (npm_sgemm_skinny_splits), n in 1 .. NPM_SKINNY_MAX_SPLITS forced -- more splits than 16-k chunks leaves empty splits, which is allowed */
    NPM_TUNE_SKINNY_NT = 23,         /* npm_sgemm_skinny, the cache hint of the weight loads (each byte is read once): 0 (default) nontemporal when the weights are at least 32 MB (NPM_TUNE_STREAM_NT's rule), 1 always, 2 never; measured in tools/skinny_gemm_bench.py */
    NPM_TUNE_PREFIX_SPLITS = 24,     /* npm_mha_prefix_splits: blocks the keys of a shared prefix are split over: 0 (default) automatic, n in 1 .. NPM_PREFIX_MAX_SPLITS forced -- more splits than 16-key tiles leaves empty splits, which is allowed */
    NPM_TUNE_GEMM_ABLATE = 99
};
int npm_set_tuning(int knob, int value);

/* Arithmetic of the matrix products (GEMM and convolution kernels).  Inputs, outputs and accumulators are fp32 in
 * every mode; what changes is the instruction that forms the products:
 *   NPM_MATH_F32          v_mfma_f32_32x32x2_f32: exact fp32 products, bit-equal to a k-ordered fmaf chain (default).
 *   NPM_MATH_BF16X3       each operand is split in registers into three bf16 parts (hi rounded, mid, lo: 24 mantissa
 *                         bits, the parts add up to the fp32 value) and the product is formed as the six largest
 *                         cross terms on v_mfma_f32_32x32x16_bf16, the five small terms in accumulators of their own.
 *                         Error against fp64 is at or below the f32 mode's (tools/math_bias.py);
 *                         results are NOT bit-equal to the f32 mode.  Non-finite operands: an infinity (or a
 *                         value that rounds to one in bf16, |a| > 3.389e38) splits into inf + (inf - inf) and gives
 *                         NaN where the f32 mode gives inf; operands below 2^-110 lose their low parts to underflow.
 *   NPM_MATH_BF16X3_FAST  the same six terms into one accumulator: fewer registers, faster; the matrix pipe cuts
 *                         small addends against a large accumulator, which leaves a bias of about -0.5 ulp per
 *                         4096 accumulated terms (visible in column checksums, not per element).
 *   NPM_MATH_F16X2        two-way fp16 split with ROW SCALING on v_mfma_f32_32x32x16_f16, three MFMAs per product: every
 *                         row of op(A) and column of op(B) is scaled by a power of two that brings its largest magnitude
 *                         along K to [2^13, 2^14), split into hi + lo (11 + 11 bits), and the product is
 *                         (hi hi + hi lo + lo hi) / (s_a s_b).  The error is fp32-class ROW-NORMWISE (rms 1.4e-7 of the
 *                         output row's largest element at K = 4096, below a k-ordered fp32 fma chain's 3.8e-7) rather
 *                         than elementwise: an operand element more than 2^17 below its row's maximum keeps fewer than
 *                         22 bits (absolute loss <= 2^-39 of that maximum).  inf / nan anywhere in a row or column
 *                         make the whole output row / column nan.  Runs for single (un-batched) products on 16-byte
 *                         aligned operands with K % 16 == 0; every other launch (batched attention products,
 *                         convolutions, epilogue column sums) takes the bf16 split: npm_last_math() tells which ran. */
enum { NPM_MATH_F32 = 0, NPM_MATH_BF16X3_FAST = 1, NPM_MATH_BF16X3 = 2, NPM_MATH_F16X2 = 3 };
/* The parity contract of a mode: what a layer computed under it may differ from the NumPy reference evaluated in fp64 on
 * the same inputs, on every configuration of BASELINE.json (C1 .. C5) at full width.  north_star's bound is "1e-4 rel";
 * fp32 contractions reorder sums, so it is read as
 *   REL     max |got - ref| / |ref|       over the elements with |ref| >= 0.1 max |ref|   (elementwise relative), and
 *   SCALED  max |got - ref| / max |ref|   over all elements                               (tensor-scaled).
 * tests/test_gpu_parity.py asserts both for every mode that has a line here (np_modeling_amd/_C.py reads the numbers from
 * this header), and bench.py reports a throughput line only for such a mode: a mode that fails its bound on any
 * configuration loses its line.  Measured worst cases (profiles/r06_parity_relative_error.log): f32 6.2e-5 / 6.7e-6,
 * bf16x3 1.9e-5 / 2.0e-6, f16x2 2.0e-5 / 2.1e-6 -- the weight gradient dwq of C4 each time.  NPM_MATH_BF16X3_FAST has no
 * line: its documented accumulation bias is outside the contract and bench.py does not report it. */
#define NPM_PARITY_REL_F32        1e-4
#define NPM_PARITY_SCALED_F32     1e-5
#define NPM_PARITY_REL_BF16X3     1e-4
#define NPM_PARITY_SCALED_BF16X3  1e-5
#define NPM_PARITY_REL_F16X2      1e-4
#define NPM_PARITY_SCALED_F16X2   1e-5
int npm_set_math(int mode);
int npm_get_math(void);                  /* the mode REQUESTED with npm_set_math */
/* The mode the most recent npm_sgemm / npm_conv2d_* / npm_mha_core_* launch actually RAN.  The split-bf16 modes exist
 * on the LDS-DMA pipelines with the 128 x 128 tile; a launch that cannot take them (operands not 16-byte aligned, K not a
 * multiple of 16, the epilogue column sums `colsum`, the 128 x 256 tile, the fused attention core) runs the exact-f32
 * MFMA and says so here -- results are then bit-equal to NPM_MATH_F32. */
int npm_last_math(void);
/* Diagnostics: when buf != NULL every block of the LDS-DMA GEMM writes 8 words (hardware id, XCC id, s_memtime at
 * start / first tile landed / loop end / after the epilogue stores) to buf[blockIdx*8 ..]; NULL switches it off. */
int npm_debug_gemm_trace(long long *buf);

/* ---- elementwise ---------------------------------------------------------- */
int npm_relu_fwd(const float *x, float *y, size_t n);                      /* activations.py:15 */
int npm_relu_bwd(const float *x_pre, const float *dy, float *dx, size_t n);/* activations.py:19 (x >= 0) */
int npm_add(const float *a, const float *b, float *out, size_t n);          /* transformer.py:39,53,78,90 */
int npm_add3(const float *a, const float *b, const float *c, float *out, size_t n); /* transformer.py:85 */
int npm_axpy(float *y, const float *x, float alpha, size_t n);              /* y += alpha*x; optimizer.py:32 */
int npm_scale(const float *x, float *y, float alpha, size_t n);
int npm_colsum(const float *x, float *out, int64_t rows, int64_t cols, int64_t ld); /* mlp.py:34 */
/* dx = (x_pre >= 0 ? dy : 0) on a contiguous [rows, cols] matrix and colsum[c] = sum_r dx[r, c] in the same
 * pass: the ReLU backward and the bias gradient of conv.py:54-55 / mlp.py:34,74 (one read of x_pre and dy). */
int npm_relu_bwd_colsum(const float *x_pre, const float *dy, float *dx, float *colsum, int64_t rows, int64_t cols);

/* ---- row kernels (one wavefront per row) ---------------------------------- */
/* out[(b*H + h)*S + s] = sum_d a[b,s,h,d] * b[b,s,h,d]: the row term of the fused softmax backward */
int npm_attn_rowdot(const float *a, const float *b, float *out, int64_t batch, int64_t seq, int64_t heads, int64_t dim);
/* y = softmax(scale * x) over the last axis                    (activations.py:26-29, attentions.py:104) */
int npm_softmax_fwd(const float *x, float *y, int64_t rows, int64_t n, float scale);
/* dx = scale * y * (dy - sum(dy*y)): closed form of the Jacobian einsum (activations.py:32-45, attentions.py:155) */
int npm_softmax_bwd(const float *y, const float *dy, float *dx, int64_t rows, int64_t n, float scale);
/* z = gamma*(x-mean)*rstd + beta; saves mean and rstd = 1/sqrt(var+eps), biased var (normalizations.py:45-48) */
int npm_layernorm_fwd(const float *x, const float *gamma, const float *beta, float eps,
                      int64_t rows, int64_t d, float *z, float *mean, float *rstd);
/* dx = rstd*(g - mean(g) - yhat*mean(g*yhat)) [+ residual], g = dz*gamma;
 * dgamma = sum dz*yhat, dbeta = sum dz (normalizations.py:50-75) */
int npm_layernorm_bwd(const float *dz, const float *x, const float *mean, const float *rstd,
                      const float *gamma, const float *residual, int64_t rows, int64_t d,
                      float *dx, float *dgamma, float *dbeta);
/* LayerNormalization of DropOut's output without ever storing it -- in the reference's encoder / decoder a DropOut always sits
 * directly in front of a LayerNormalization (transformer.py:35-36,40-41,49-50,55-56):
 *   forward   xd = mask ? x / keep_prob : 0 (normalizations.py:21-23) on the way in, then npm_layernorm_fwd's arithmetic on xd;
 *   backward  the same xd again from x and mask, npm_layernorm_bwd's arithmetic, then DropOut.backward on the way out
 *             (normalizations.py:27-30): dx = mask ? dxd / keep_prob : 0 [+ residual].
 * mask: one byte per element (0 = dropped), 4-byte aligned.  Equal to npm_mask_scale + npm_layernorm_fwd / npm_layernorm_bwd +
 * npm_mask_scale (+ npm_add) to rounding (the same operations in the same order; the compiler contracts the row sums of products
 * into fused multiply-adds per kernel instance: single ulps in a few per cent of dx).  Rows with d % 4 != 0 or d > 4096 are NPM_E_UNSUPPORTED: compose the calls above. */
int npm_layernorm_dropout_fwd(const float *x, const unsigned char *mask, float keep_prob, const float *gamma, const float *beta,
                              float eps, int64_t rows, int64_t d, float *z, float *mean, float *rstd);
int npm_layernorm_dropout_bwd(const float *dz, const float *x, const unsigned char *mask, float keep_prob, const float *mean,
                              const float *rstd, const float *gamma, const float *residual, int64_t rows, int64_t d,
                              float *dx, float *dgamma, float *dbeta);
/* RMSNorm over the last axis: LayerNorm without the mean and without beta, as kernels of their own in the same width grid (a row
 * in registers with 1 / 2 / 4 / 8 / 16 float4 per lane for d % 4 == 0, d <= 4096 and 16-byte aligned x, z / dz, dx, residual and
 * gamma; a generic kernel takes every other d or alignment).
 *   forward   ms = sum(x^2) / d, rstd = 1 / sqrtf(ms + eps), z = gamma * (x * rstd); rstd [rows] is saved.  The sum is a plain
 *             fp32 sum of the squares as they are: no rescaling by the row's largest element, so an |x| above about 1.8e19
 *             overflows it (ms = inf, rstd = 0, z = 0) -- activations are far from that, and the rescaling costs a second pass.
 *   backward  xh = x * rstd, g = dz * gamma, m2 = sum(g * xh) / d, dx = rstd * (g - xh * m2) [+ residual] (residual may be
 *             NULL), dgamma = sum over rows of dz * xh.
 * dgamma is reproducible, as npm_layernorm_bwd's: waves walk rows grid-stride (NPM_TUNE_LN_BWD_BLOCKS blocks per CU), one partial
 * row per block added in wave order, one fixed-order column sum over the block partials; no float atomics.  A row's z and dx do
 * not depend on the other rows nor on the row's position.  Tensors of >= 32 MB move with the nontemporal hint (NPM_TUNE_STREAM_NT);
 * at d in (512, 1024] the hint is on the loads only, npm_layernorm's placement (NPM_TUNE_LN_NT_SPLIT) for npm_layernorm's reason:
 * a GEMM reads z and dx at once.  rows == 0: the forward is a no-op, the backward writes dgamma = 0. */
int npm_rmsnorm_fwd(const float *x, const float *gamma, float eps, int64_t rows, int64_t d, float *z, float *rstd);
int npm_rmsnorm_bwd(const float *dz, const float *x, const float *rstd, const float *gamma, const float *residual /* may be NULL */,
                    int64_t rows, int64_t d, float *dx, float *dgamma);
/* The gate of a gated-SiLU ("SwiGLU") feed-forward.  pre [rows, 2 units] with a pitch of ld floats is the output of the packed
 * gate | up projection: gate columns [0, units), up columns [units, 2 units).
 *   forward   h[r, c] = (gate * sigma(gate)) * up                                                  h [rows, units], pitch ldh
 *   backward  dgate = dh * up * sigma(gate) * (1 + gate * (1 - sigma(gate))),  dup = dh * (gate * sigma(gate))
 *             dpre [rows, 2 units], pitch lddpre, laid out as pre; sigma is recomputed from pre: nothing else is stored.
 * sigma in the overflow-free two-branch form: t = expf(-|gate|), sigma = gate >= 0 ? 1 / (1 + t) : t / (1 + t); 1 - sigma is the
 * other branch, so neither cancels.  16-byte loads and stores when units % 4 == 0, every pitch is a multiple of 4 and every base is
 * 16-byte aligned; one element per thread otherwise.  Grid-stride under NPM_TUNE_EW_GRID_CAP; nontemporal instances when pre has
 * at least 32 MB (8 rows units bytes; NPM_TUNE_STREAM_NT).  An inf or NaN in an element of pre or dh reaches that element's
 * outputs only; nothing faults on any value.  The outputs may not overlap the inputs.  Error against exact arithmetic on the
 * fp32 inputs (u = 2^-24; expf within 1 ulp, correctly rounded division): forward 6 u |h|; backward 8 u T1 + 13 u T2 for dgate
 * with T1 = |dh up sigma| and T2 = |dh up gate sigma (1 - sigma)| -- relative to the terms, not to their sum, which has a root near
 * gate = -1.2785 -- and 6 u |dup|; plus absolute terms of a few 2^-126 (|gate| + 1) times the other factors where sigma or 1 - sigma
 * is below the smallest normal number (|gate| above about 87.3).  tests/test_gpu_swiglu.py derives and asserts them.
 * NPM_E_BAD_ARGUMENT: units < 1, a pitch below its row, rows outside 0 .. 2^31 - 1, a NULL pointer with rows > 0.  rows == 0 is a
 * no-op. */
int npm_swiglu_fwd(const float *pre, int64_t ld, int64_t rows, int64_t units, float *h, int64_t ldh);
int npm_swiglu_bwd(const float *pre, int64_t ld, const float *dh, int64_t lddh, int64_t rows, int64_t units, float *dpre,
                   int64_t lddpre);

/* ---- Conv2D: NHWC x HWIO, SAME, stride 1, odd k (layers/conv.py:74-194) ----
 * Implicit-im2col GEMM on the fp32 MFMA; the im2col matrix is never materialised. */
typedef struct npm_conv2d {
    int32_t n, h, w, c_in, c_out, ksize;
    const float *x;        /* [n,h,w,c_in] */
    const float *filt;     /* [k,k,c_in,c_out] */
    const float *bias;     /* [c_out] or NULL */
    float *y;              /* [n,h,w,c_out] */
    float *pre;            /* optional pre-activation output when relu != 0 */
    int32_t relu;
} npm_conv2d;
int npm_conv2d_fwd(const npm_conv2d *c);                                           /* conv.py:44-48,97-105 */
/* dx = conv(dy, flip+transpose(filt))  (conv.py:130,153) */
int npm_conv2d_bwd_x(const float *dy, const float *filt, float *dx,
                     int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t ksize);
/* dw[i,j] = shifted(x)^T dy  (conv.py:185-194) */
int npm_conv2d_bwd_w(const float *dy, const float *x, float *dw,
                     int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t ksize);
/* Conv2D.backward's first three lines in one call (conv.py:54-56 with the layer's ReLU, activations.py:19):
 *   g = where(pre >= 0, dy, 0)  [n,h,w,c_out], written out (the grad_x convolution reads it: npm_conv2d_bwd_x(g, ...))
 *   db = sum over n, h, w of g  [c_out]
 *   dw[i,j] = shifted(x)^T g    [k,k,c_in,c_out]
 * The mask is applied where the grad_w kernel stages its dy tiles, so no separate ReLU-backward pass over the
 * activation-sized tensors runs; results are bitwise reproducible (fixed-order slab and column reductions). */
int npm_conv2d_bwd_w_relu(const float *dy, const float *pre, const float *x, float *g, float *dw, float *db,
                          int32_t n, int32_t h, int32_t w, int32_t c_in, int32_t c_out, int32_t ksize);
/* What the most recent of the four calls above launched; "" before the first one.  A call that fails its argument check leaves
 * the string as it was.  "none" for the empty calls (n == 0; no pixels: dw and db are zero-filled).  Otherwise
 *   "<family> vec=<0|1> tall=<0|1> math=<0|1|2> korder=<0|1> buf=<0|1> splits=<s> kper=<k> wr=<0|2|3> trio=<0|1> ksync=<0|e>"
 * family  conv_fwd (register-staged forward / grad_x kernel), conv_fwd_glds (LDS-DMA), conv_wgrad, conv_wgrad_glds,
 *         conv_wgrad_relu (the fused filter gradient);
 * vec     16-byte loads (the register-staged kernels' float4 instance; every LDS-DMA kernel);
 * tall    the 256 x 64 block tile of conv_fwd_glds;
 * math    the arithmetic that ran, as NPM_TUNE_GEMM_MATH counts it with the f16 mode folded into 2 (0 on every
 *         register-staged kernel and on the fused one);
 * korder  the K walk of conv_fwd_glds (NPM_TUNE_CONV_KORDER); 0 elsewhere: taps outermost;
 * buf     the accumulators leave through buffer stores (write_tile_buf, or the fused kernel's own), not write_tile;
 * splits  split-K blocks per output tile, kper the K range of one of them (pixels for the filter gradients, k*k*c_in for
 *         forward / grad_x);
 * wr      the fused kernel's tile height in 64-row units (2: 128 rows, 3: 192), trio: its twelve-wave form, ksync: the K
 *         rendezvous interval in K tiles when it is engaged, else 0.
 * npm_conv2d_bwd_w_relu on a shape the fused kernel does not take reports "two_pass " followed by what its
 * npm_conv2d_bwd_w reported. */
const char *npm_last_conv_kernel(void);

/* ---- fused attention core (layers/attentions.py:103-112 forward, :146-162 backward) ----
 * ctx[b, i, h, :] = sum_j softmax_j(scale * q[b, i, h, :] . k[b, j, h, :]) v[b, j, h, :] in ONE kernel: the
 * [B, H, Sq, Skv] probabilities never go to memory (online softmax, as derived in the reference's
 * layers/attentions_test.py:158-265); the forward saves lse[b, h, i] = log sum_j exp(scale * q.k) and the backward
 * recomputes the probabilities from it.  q/k/v/ctx and the gradients are [B, S, H, D] with a row pitch (H * D, or
 * 3 * H * D inside a packed qkv buffer); head_dim in {16, 32, 64, 128}, else NPM_E_UNSUPPORTED (callers then
 * compose the same math from npm_sgemm + npm_softmax_*).  mask (optional): bytes, element (b, h, i, j) at
 * mask[b * stride_b + h * stride_h + i * stride_q + j], 0 = excluded (np.where(mask, scaled, -inf),
 * attentions.py:105-107); the backward treats excluded positions as P = 0 (the reference raises NotImplementedError
 * there, attentions.py:152-153).  scores (optional, [B, H, Sq, Skv]): when given, the forward also stores the raw
 * masked scores q.k and the backward reads them instead of recomputing q.k (trades 4 B/element of traffic each way
 * for one of the five matrix products).  fp32 MFMA only (npm_set_math does not apply to this kernel). */
typedef struct npm_mha_core {
    int32_t batch, heads, seq_q, seq_kv, head_dim;
    float scale;                                   /* 1 / sqrt(Dk), > 0 */
    const float *q; int64_t q_pitch;
    const float *k; int64_t k_pitch;
    const float *v; int64_t v_pitch;
    const uint8_t *mask; int64_t mask_stride_b, mask_stride_h, mask_stride_q;
    float *ctx; int64_t ctx_pitch;                 /* forward: out; backward: in (the forward's result) */
    float *lse;                                    /* [B, H, Sq]; forward: out; backward: in */
    float *scores;                                 /* optional [B, H, Sq, Skv]; forward: out; backward: in */
    const float *dctx; int64_t dctx_pitch;         /* backward only from here */
    float *dq; int64_t dq_pitch;
    float *dk; int64_t dk_pitch;
    float *dv; int64_t dv_pitch;
    /* Optional, with `mask`: the mask's tile summary from npm_mha_mask_summary -- one byte per (query tile of 32, key block
     * of 128), bit w set when some position of the 32 x 16 sub-tile (keys 16 w .. 16 w + 15 of the block) is allowed; byte
     * (qt, kb) of plane (b, h) at tile_summary[b * summary_stride_b + h * summary_stride_h + qt * ceil(seq_kv / 128) + kb]
     * (a stride of 0 broadcasts, like the mask's).  Forward and backward then skip tiles without an allowed position: the
     * results are the same as without it -- including the NaNs of a query row with NO allowed key (np.where(mask, s, -inf) then
     * softmax: that row of ctx and dq, and through P = NaN every dk / dv row of its (batch, head)): npm_mha_mask_summary marks
     * every tile of a mask plane that has such a row as "visit", so such planes are simply not skipped.  Positions of `scores`
     * inside skipped tiles are left unwritten (the backward never reads them).  Used for seq_q, seq_kv <= 2048; longer
     * sequences run unskipped. */
    const uint8_t *tile_summary; int64_t summary_stride_b, summary_stride_h;
    int64_t summary_all_offset;   /* bytes from a tile's "some position allowed" byte to its "every position allowed" byte (the second
                                     half of what npm_mha_mask_summary writes: planes_b * planes_h * tiles bytes later); 0 = not given.
                                     Tiles whose every position is allowed run without reading the mask. */
    /* Optional, backward: the row terms MINUS scale * (dctx_i . ctx_i) already computed by the caller (the NPM_EPI_ROWDOT
     * epilogue of the GEMM that produced dctx -- which exists at head_dim 128 only, but any head size is taken here), element
     * (b, h, i) at neg_delta[b * stride_b + h * stride_h + i], 16-byte aligned, strides multiples of 4; npm_mha_core_bwd then
     * does not read dctx and ctx for them.  Honoured by the eight-wave kernels (mha_bwd16_kernel, mha_bwd8_kernel) when
     * seq_q % 4 == 0 (they fetch four row terms per load); otherwise -- and on the four-wave kernel (NPM_TUNE_ATTN_BWD16 = 0
     * or 1) -- it is ignored and the terms are recomputed from dctx and ctx: same results. */
    const float *neg_delta; int64_t neg_delta_stride_b, neg_delta_stride_h;
} npm_mha_core;
int npm_mha_core_supported(int head_dim);          /* 1 when npm_mha_core_fwd/bwd take this head dimension */
int npm_mha_core_fwd(const npm_mha_core *c);
int npm_mha_core_bwd(const npm_mha_core *c);
/* Grouped-query attention (the reference's gqa_fwd, layers/attentions_test.py:267-358): c->heads query heads share kv_heads
 * key / value heads, and query head h reads K / V head h % kv_heads.  k, v, dk and dv are [B, Skv, kv_heads, D] with their own
 * pitches (>= kv_heads * D; a packed [B, S, heads + 2 kv_heads, D] buffer works); everything per query head (q, ctx, lse, mask,
 * tile summary, scores, neg_delta, dq) is laid out as in npm_mha_core_fwd / _bwd.  The backward writes one dK / dV partial per
 * query head into pooled scratch and sums each group in a fixed order (bitwise reproducible, no atomics).  kv_heads < 1 or
 * heads % kv_heads != 0: NPM_E_BAD_ARGUMENT; kv_heads == heads is the ungrouped call exactly. */
int npm_mha_core_fwd_grouped(const npm_mha_core *c, int32_t kv_heads);
int npm_mha_core_bwd_grouped(const npm_mha_core *c, int32_t kv_heads);
/* A plane (b, h) with a query row that has no allowed key at all gets 0xFF in every "some position allowed" byte (see above).
 * summary[2][plane_b][plane_h][ceil(seq_q / 32)][ceil(seq_kv / 128)] (first the "some position allowed" bytes, then, in the
 * same order, the "every position inside the tensors allowed" bytes) of a byte mask laid out like npm_mha_core's (element
 * (b, h, i, j) at mask[b * stride_b + h * stride_h + i * stride_q + j]); planes_b / planes_h = how many distinct planes the
 * mask has along batch and head (1 where it broadcasts).  np.where(mask, scaled, -inf) of attentions.py:105-107 skips
 * nothing; this is what lets the fused kernels skip the tiles such a mask empties (half of a causal mask's). */
int npm_mha_mask_summary(const uint8_t *mask, int64_t stride_b, int64_t stride_h, int64_t stride_q, int32_t planes_b,
                         int32_t planes_h, int32_t seq_q, int32_t seq_kv, uint8_t *summary);
/* Which kernel the most recent npm_mha_core_fwd / npm_mha_core_bwd call launched, as "<kernel> D=<head_dim> mask=<0|1>
 * scores=<0|1>" (e.g. "mha_bwd16_kernel D=128 mask=0 scores=1"), followed by " kv_heads=<n>" for a grouped call with fewer
 * K / V heads than query heads; "" before the first call.  Tests use it to assert that
 * a comparison exercised the kernel it names. */
const char *npm_last_attn_kernel(void);
/* Diagnostics: when buf != NULL every block of the stamped kernel instances writes 16 words of s_memtime stamps of ONE of its
 * tiles (backward phase boundaries: tile start, after S, dP, dV, dK, the dS barrier, dQ, the dQ stores; words 9 .. 13: the
 * block's start and end) to buf[blockIdx * 16 ..]; NULL switches it off.  The stamped instances: mha_bwd16_kernel (a backward
 * at head size 128 with saved scores and no tile summary runs it while buf is set, whatever NPM_TUNE_ATTN_BWD16 says) and
 * the four-wave forward mha_fwd_kernel at head size 128 without a mask (such a forward runs it while buf is set, whatever
 * NPM_TUNE_ATTN_FWD8 says).  Every other call runs its normal kernel and leaves buf alone. */
int npm_debug_attn_trace(long long *buf);

/* ---- incremental decoding: attention over a key / value cache (inference; the reference has none: "# TODO: support cache",
 * layers/transformer.py:120) ----
 * T = new_tokens query tokens per sequence attend to the first L = kv_len rows of a cache [B, capacity, kv_heads, D]:
 *   ctx[b, t, h, :] = sum_j softmax_j(scale * q[b, t, h, :] . k[b, j, h % kv_heads, :]) v[b, j, h % kv_heads, :]
 *   j < L when causal == 0; j <= L - T + t when causal != 0 (the T new tokens are the LAST T keys of the cache, already appended).
 * Rows L .. capacity - 1 of the cache are never part of a result, whatever they hold (NaN included); capacity itself is not an
 * argument: the kernel reads no row at or past L.  One block serves the heads / kv_heads query heads that share a K / V head (so
 * K and V are read once per group), the keys are split over several blocks whose partial results a second kernel merges in
 * split order (no atomics: bitwise reproducible; the split count is npm_mha_decode_splits, a function of the shape and of
 * NPM_TUNE_DECODE_SPLITS only).  fp32 in and out, exact-fp32 MFMA (npm_set_math does not apply).  head_dim in {16, 32, 64, 128} and
 * group_rows = (heads / kv_heads) * new_tokens <= NPM_DECODE_MAX_ROWS, else NPM_E_UNSUPPORTED (callers then use npm_mha_core_fwd_grouped
 * with a causal mask, or the GEMM composition).  NPM_E_BAD_ARGUMENT: kv_len < new_tokens, heads % kv_heads != 0, a pointer that
 * is not 16-byte aligned, a pitch or batch stride that is not a multiple of 4 floats or is narrower than its row. */
#define NPM_DECODE_MAX_ROWS 32
#define NPM_DECODE_MAX_SPLITS 1024
typedef struct npm_mha_decode {
    int32_t batch, heads, kv_heads, new_tokens, kv_len, head_dim;   /* kv_len = L: valid cache rows, the new tokens included */
    int32_t causal;                                /* 0: every row sees keys 0 .. L - 1; else row t sees keys 0 .. L - T + t */
    float scale;                                   /* 1 / sqrt(Dk), > 0 */
    const float *q; int64_t q_pitch;               /* [B, T, heads, D]; pitch = floats between consecutive (b, t) rows */
    const float *k; int64_t k_pitch, k_stride_b;   /* cache [B, capacity, kv_heads, D]: floats between rows / between batch entries */
    const float *v; int64_t v_pitch, v_stride_b;
    float *ctx; int64_t ctx_pitch;                 /* out [B, T, heads, D] */
    float *lse;                                    /* optional out [B, heads, T]: log sum_j exp(scale * q.k) over the visible keys */
} npm_mha_decode;
int npm_mha_decode_supported(int head_dim, int group_rows);      /* group_rows = (heads / kv_heads) * new_tokens */
int npm_mha_decode_fwd(const npm_mha_decode *d);
/* The number of key splits npm_mha_decode_fwd uses for this shape under the current NPM_TUNE_DECODE_SPLITS. */
int npm_mha_decode_splits(int batch, int kv_heads, int kv_len);
/* cache[b, at + t, 0 .. row_len - 1] = src[b * new_tokens + t, 0 .. row_len - 1] for every b < batch, t < new_tokens: the freshly
 * projected K (or V) rows of T tokens per sequence into cache rows at .. at + T - 1.  src_pitch: floats between consecutive
 * (b, t) rows of the source (a packed [B, T, heads + 2 kv_heads, D] projection is read in place); cache_pitch / cache_stride_b as
 * k_pitch / k_stride_b above.  The caller checks at + new_tokens against the capacity.  16-byte accesses: row_len, pitches and
 * the stride multiples of 4 floats, pointers 16-byte aligned, else NPM_E_BAD_ARGUMENT. */
int npm_kv_append(const float *src, int64_t src_pitch, float *cache, int64_t cache_pitch, int64_t cache_stride_b,
                  int32_t batch, int32_t new_tokens, int32_t row_len, int32_t at);
/* What the most recent npm_mha_decode_fwd launched: "<kernel> D=<head_dim> rows=<group_rows> splits=<n> causal=<0|1>"; "" before
 * the first call.  After npm_mha_decode_fwd_varlen: the same string followed by " varlen=1"; after npm_mha_decode_fwd_paged: that
 * followed by " paged=<page_rows>". */
const char *npm_last_decode_kernel(void);

/* ---- ragged batches: one length per sequence (device arrays of batch int32 each; they are read by the kernels, never on the host) ----
 * npm_mha_decode_fwd with L_b = kv_lens[b] valid cache rows for sequence b (this call's new tokens included) and n_b = new_lens[b]
 * new tokens (NULL: all d->new_tokens); x is padded on the right to T = d->new_tokens rows.  Row t of sequence b sees keys
 *   j < (t < n_b ? (causal ? L_b - n_b + t + 1 : L_b) : 0).
 * A row that sees no key (a padded token t >= n_b, or L_b = 0) gets ctx = 0 and lse = -inf by selection, never 0 / 0; nothing at or
 * past row L_b of the cache enters a result, whatever it holds.  d->kv_len is an upper bound of kv_lens known to the host: it sizes
 * the grid, the split count (npm_mha_decode_splits(batch, kv_heads, d->kv_len)) and the key range of every split, so with all
 * kv_lens[b] == d->kv_len and all new_lens[b] == d->new_tokens the result is bitwise that of npm_mha_decode_fwd.  A block whose key
 * range starts at or past L_b returns before it loads any key: the cost follows the sum of the lengths, not batch * d->kv_len.
 * The caller guarantees 0 <= new_lens[b] <= d->new_tokens, 0 <= kv_lens[b] <= d->kv_len and, when causal, new_lens[b] <= kv_lens[b]
 * (the new tokens are among the valid rows; a frozen cross-attention cache may be shorter than the query).  NPM_E_BAD_ARGUMENT for
 * kv_lens == NULL; otherwise the argument checks of npm_mha_decode_fwd except kv_len >= new_tokens (kv_len >= 0 here). */
int npm_mha_decode_fwd_varlen(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens);
/* npm_kv_append per sequence: cache[b, at_lens[b] + t, 0 .. row_len - 1] = src[b * new_tokens + t, 0 .. row_len - 1] for
 * t < new_lens[b] (NULL: every t < new_tokens); no other cache row is written.  The caller checks at_lens[b] + new_lens[b] against
 * the capacity on the host.  Alignment rules as npm_kv_append. */
int npm_kv_append_varlen(const float *src, int64_t src_pitch, float *cache, int64_t cache_pitch, int64_t cache_stride_b,
                         int32_t batch, int32_t new_tokens, int32_t row_len, const int32_t *at_lens, const int32_t *new_lens);
/* out[b, j, 0 .. row_len - 1] = j < lens[b] ? cache[b, j, 0 .. row_len - 1] : 0 for every b < batch, j < rows; out is
 * [batch, rows, row_len], contiguous: the valid rows of a ragged cache for a kernel that addresses K / V without a batch stride,
 * with ZEROS behind them (the fused forward multiplies P = 0 by whatever V holds there).  Cache rows at and past lens[b] are not
 * read.  One launch.  Alignment rules as npm_kv_append. */
int npm_kv_gather_varlen(const float *cache, int64_t cache_pitch, int64_t cache_stride_b, float *out, int32_t batch, int32_t rows,
                         int32_t row_len, const int32_t *lens);

/* ---- paged caches: K / V rows in a pool of pages, one block table per sequence ----
 * npm_mha_decode_fwd_varlen over a paged cache.  d->k / d->v are page pools [pages, page_rows, kv_heads, D]: d->k_pitch / v_pitch the
 * row pitch inside a page, d->k_stride_b / v_stride_b the PAGE stride (>= page_rows * pitch).  Key j of sequence b is row
 * (j & (page_rows - 1)) of page block_table[b * table_pitch + (j >> log2 page_rows)]; block_table is a device array of
 * batch * table_pitch int32 with table_pitch * page_rows >= d->kv_len.  page_rows is a power of two >= 16 (the kernel's key tile),
 * so a tile never straddles a page and paging is one wave-uniform table lookup per tile in front of the varlen kernel's own
 * arithmetic: split count, tile partition, load policy and every floating-point operation are those of npm_mha_decode_fwd_varlen
 * with the same d->kv_len, and the result is BITWISE that call's on a contiguous cache holding the same rows.  Table entries at and
 * past ceil(kv_lens[b] / page_rows) may hold anything: they are never read (the look-ahead index is clamped to the page of key
 * kv_lens[b] - 1).  The caller guarantees that every entry before that names a page of the pool.  NPM_E_BAD_ARGUMENT for kv_lens or
 * block_table == NULL and for a page_rows that is not a power of two >= 16; otherwise the checks of npm_mha_decode_fwd_varlen.
 * npm_last_decode_kernel() afterwards: the varlen string followed by " paged=<page_rows>". */
int npm_mha_decode_fwd_paged(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                             int32_t table_pitch, int32_t page_rows);
/* npm_kv_append_varlen into a page pool: row at_lens[b] + t of sequence b, addressed through the block table as above, =
 * src[b * new_tokens + t] for t < new_lens[b] (NULL: every t).  The caller has put a page into the table for every row written.
 * row_pitch / page_stride: floats between rows of a page / between pages.  Alignment rules as npm_kv_append; at_lens or block_table
 * == NULL or a bad page_rows: NPM_E_BAD_ARGUMENT. */
int npm_kv_append_paged(const float *src, int64_t src_pitch, float *pool, int64_t row_pitch, int64_t page_stride, int32_t batch,
                        int32_t new_tokens, int32_t row_len, const int32_t *at_lens, const int32_t *new_lens,
                        const int32_t *block_table, int32_t table_pitch, int32_t page_rows);
/* npm_kv_gather_varlen out of a page pool: out[b, j] = j < lens[b] ? row j of sequence b : 0 for j < rows; out is
 * [batch, rows, row_len], contiguous.  Neither a row at or past lens[b] nor its table entry is read. */
int npm_kv_gather_paged(const float *pool, int64_t row_pitch, int64_t page_stride, float *out, int32_t batch, int32_t rows,
                        int32_t row_len, const int32_t *lens, const int32_t *block_table, int32_t table_pitch, int32_t page_rows);

/* ---- prefill: any number of new tokens straight over the cache (a prompt, a chunk of one, a sequence admitted into a batch) ----
 * The contract of npm_mha_decode_fwd / _varlen / _paged on the same descriptor, without the limit on (heads / kv_heads) * new_tokens:
 *   kv_lens == NULL      every sequence has L = d->kv_len valid rows and brings T = d->new_tokens (needs kv_len >= new_tokens);
 *   kv_lens != NULL      L_b = kv_lens[b], n_b = new_lens[b] (NULL: T) as in npm_mha_decode_fwd_varlen; d->kv_len is the host's
 *                        upper bound and changes no result;
 *   block_table == NULL  the cache is contiguous (d->k_stride_b the batch stride); otherwise d->k / d->v are page pools as in
 *                        npm_mha_decode_fwd_paged (kv_lens is then required).
 * Row t < n_b sees keys j <= L_b - n_b + t when causal and j < L_b otherwise; a row with no visible key (t >= n_b, L_b == 0) is
 * stored as ctx = 0, lse = -inf by selection; lse is optional.  Nothing at or past row L_b of the cache enters a result, whatever it
 * holds; table entries at and past ceil(L_b / page_rows) are not read.
 * The kernel (csrc/npm_prefill.hip): a block covers 64 query rows -- (query head of the group, token) pairs -- of ONE K / V head,
 * so K / V are read once per group; its four waves share every 16-key tile through LDS; it walks key tiles only up to the largest
 * limit of its own rows (the causal upper triangle and everything past L_b are skipped), and a block whose tokens are all padding
 * returns before it loads anything.  No mask, no gather, no [T, L] object: causality and lengths are arithmetic on (t, j, L_b, n_b)
 * read on the device.  Keys are NOT split over blocks, so a valid row of sequence b depends only on that sequence's q, rows, L_b,
 * n_b and d->new_tokens.  Hence, BITWISE: the paged result is the contiguous one on the same rows; kv_lens == NULL is the call
 * with all lengths equal; sequence b in a batch is that sequence at batch 1 with the same new_tokens, whatever d->kv_len bounds.
 * Exact fp32 MFMA (npm_set_math does not apply), no atomics.  head_dim in {16, 32, 64, 128}, else NPM_E_UNSUPPORTED.  Argument
 * checks and error codes are those of the decode entry point of the same layout; a refused call launches nothing.
 * npm_last_prefill_kernel(): "mha_prefill_kernel D=<head_dim> T=<new_tokens> rows=<query rows per block> causal=<0|1>", then
 * " varlen=1" with kv_lens and " paged=<page_rows>" with a block table; "" before the first call. */
int npm_mha_prefill_supported(int head_dim);
int npm_mha_prefill_fwd(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                        int32_t table_pitch, int32_t page_rows);
const char *npm_last_prefill_kernel(void);

/* ---- half-precision cache: K / V rows stored as IEEE fp16 (opt-in; everything above is unchanged) ----
 * The cache holds halves; q, ctx, lse, the rows handed to an append and the rows a gather returns stay fp32.  A row is converted
 * ONCE, by the append, with round to nearest even -- bit for bit NumPy's astype(float16), subnormal results included; |x| >= 65520
 * becomes +-inf (there is NO clamp: a projection that large is the caller's to scale) -- and converted back exactly wherever it is
 * read.  Scores, softmax, accumulators and outputs are the fp32 ones: npm_mha_decode_fwd_f16 is BITWISE the fp32 entry point of the
 * same layout on a cache that holds the rounded values as floats (same split count, tile partition and order of every sum), at
 * half the bytes per key.  The load policy (NPM_TUNE_DECODE_NT = 0) counts the bytes of the valid part of K, so the fp16 call
 * switches to nontemporal loads at twice the keys.
 * One entry point per operation; NULL selects the simpler layout, as in npm_mha_prefill_fwd:
 *   at_lens / kv_lens == NULL   the uniform call (npm_kv_append at ``at`` / npm_mha_decode_fwd); otherwise the per-sequence one
 *                               (``at`` is ignored);
 *   block_table == NULL         a contiguous cache (cache_stride / k_stride_b the batch stride); otherwise a page pool as in the
 *                               _paged entry points (the stride is the page stride; lengths are then required).
 * A gather always takes lens (zeros at and past lens[b]; neither such a row nor its table entry is read).
 * Units and alignment: cache pointers (cache, d->k, d->v) are 16-byte aligned; cache_pitch, cache_stride, d->k_pitch, d->k_stride_b
 * and the v_ pair count HALVES and are multiples of 8; row_len % 8 == 0; the fp32 side (src, src_pitch, out, q, ctx) keeps the
 * rules of the fp32 entry points.  npm_mha_decode itself is unchanged: d->k / d->v carry the addresses of the fp16 data.  Head
 * sizes and the row limit are those of npm_mha_decode_supported (else NPM_E_UNSUPPORTED); a block table without lengths, a bad
 * page_rows, kv_len < new_tokens on the uniform call and every other violation return what the fp32 entry point of that layout
 * returns (NPM_E_BAD_ARGUMENT); a refused call launches nothing and writes nothing.
 * npm_last_decode_kernel() after npm_mha_decode_fwd_f16: the fp32 string of the same layout followed by " kv=f16". */
int npm_kv_append_f16(const float *src, int64_t src_pitch, void *cache, int64_t cache_pitch, int64_t cache_stride, int32_t batch,
                      int32_t new_tokens, int32_t row_len, int32_t at, const int32_t *at_lens, const int32_t *new_lens,
                      const int32_t *block_table, int32_t table_pitch, int32_t page_rows);
int npm_kv_gather_f16(const void *cache, int64_t cache_pitch, int64_t cache_stride, float *out, int32_t batch, int32_t rows,
                      int32_t row_len, const int32_t *lens, const int32_t *block_table, int32_t table_pitch, int32_t page_rows);
int npm_mha_decode_fwd_f16(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                           int32_t table_pitch, int32_t page_rows);
/* npm_mha_prefill_fwd over an fp16 cache: the same arguments, layouts (kv_lens / block_table NULL or not), refusals and error codes,
 * except that d->k / d->v point at halves, their pitches and strides (the page stride d->k_stride_b included) count HALVES and are
 * multiples of 8 (the fp32 entry point: 4 floats), and every pointer is 16-byte aligned.  The kernel (mha_prefill_f16_kernel, the
 * same body as mha_prefill_kernel) loads 8 halves per 16-byte piece and converts them exactly on the way into LDS, which then
 * holds the fp32 tiles of the fp32 kernel in the same layout; everything behind that is the same code.  Hence the call is BITWISE
 * npm_mha_prefill_fwd of the same layout on a cache that holds the rounded values as floats, ctx and lse, and inherits its
 * identities (paged = contiguous, a sequence in a batch = that sequence alone, kv_lens == NULL = all lengths equal).  Nothing at or
 * past row L_b is read into a result; a block without a live row loads nothing.  head_dim as npm_mha_prefill_supported.
 * npm_last_prefill_kernel() afterwards: the fp32 string of the same layout followed by " kv=f16". */
int npm_mha_prefill_fwd_f16(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                            int32_t table_pitch, int32_t page_rows);

/* ---- sliding-window (local) causal attention over a cache (opt-in; everything above is unchanged) ----
 * window = W >= 1: a query at absolute position p sees keys max(0, p - W + 1) .. p, itself included.  Row t < n_b of sequence b
 * has the upper limit of the causal calls above, limit = L_b - n_b + t + 1, and sees keys floor <= j < limit with
 * floor = max(0, limit - W).  Nothing below a row's floor enters its result, whatever those cache rows hold (the rule rows >= L_b
 * have): such a key gets score -inf by selection, V rows below the smallest floor of a tile's users are zeroed by selection, a
 * tile wholly below that floor is never loaded and its block-table entry never read -- the pages there may have been given back.
 * Per-sequence layouts only, arguments as the _f16 entry points take them: kv_lens is required; block_table == NULL is a
 * contiguous cache, else a page pool; kv_f16 != 0: d->k / d->v point at halves, pitches and strides count halves.  Refusals are
 * those of the entry point of the same layout and storage type; in addition NPM_E_BAD_ARGUMENT for window < 1, d->causal == 0
 * and kv_lens == NULL.  A refused call launches nothing.
 * npm_mha_decode_fwd_window (rows <= NPM_DECODE_MAX_ROWS): the key walk of sequence b starts at its first live tile
 * lo_b = max(0, L_b - n_b + 1 - W) / 16 and the split partition is laid over the window: with keys_bound = min(d->kv_len,
 * W + new_tokens - 1) the split count is npm_mha_decode_splits(batch, kv_heads, keys_bound) (= npm_mha_decode_window_splits),
 * tiles_per_split covers the most 16-key tiles an interval of keys_bound keys can touch, split s takes tiles lo_b + s *
 * tiles_per_split ..; scratch, grid and the load policy follow keys_bound.  W >= d->kv_len: BITWISE the unwindowed entry point of
 * the same layout and storage type.  Paged is bitwise contiguous on the same rows, fp16 bitwise the fp32 call on the rounded
 * values; a row without a visible key is ctx = 0, lse = -inf by selection.
 * npm_mha_prefill_fwd_window (any number of rows): a block's walk starts at the tile of the smallest floor of its live rows and a
 * wave skips tiles wholly below its own rows' smallest floor; keys are not split, so the identities of npm_mha_prefill_fwd[_f16]
 * carry over bitwise, and W >= every L_b is bitwise that call.
 * npm_last_decode_kernel() / npm_last_prefill_kernel() afterwards: the string of the same layout and storage type followed by
 * " window=<W>". */
int npm_mha_decode_fwd_window(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                              int32_t table_pitch, int32_t page_rows, int32_t window, int32_t kv_f16);
int npm_mha_prefill_fwd_window(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens, const int32_t *block_table,
                               int32_t table_pitch, int32_t page_rows, int32_t window, int32_t kv_f16);
int npm_mha_decode_window_splits(int batch, int kv_heads, int kv_len, int new_tokens, int window);

/* ---- shared key / value prefixes: pages named by several sequences (opt-in; everything above is unchanged) ----
 * npm_kv_copy_pages, the copy of copy-on-write: for i < n, rows 0 .. rows[i] - 1 of page dst_pages[i] of the pool become those of
 * page src_pages[i]; rows at and past rows[i] of the destination are not written.  ONE launch for all pairs.  The pool is bytes
 * here: page_stride_bytes between pages, the rows of a page back to back at row_bytes each, both multiples of 16 and the pool
 * 16-byte aligned, so f32 and f16 pools take the same call.  src_pages, dst_pages, rows: device arrays of n int32; the caller
 * guarantees pages of the pool, src_pages[i] != dst_pages[i], distinct destinations and rows[i] * row_bytes <= page_stride_bytes.
 * n == 0 or row_bytes == 0: NPM_OK, nothing launched.  NPM_E_BAD_ARGUMENT for a NULL pointer, a negative count or a misaligned size.
 *
 * npm_mha_prefix_fwd: the R = d->batch * d->new_tokens query rows of ALL sequences (row b * new_tokens + t of d->q, pitch
 * d->q_pitch) attend, NOT causally, to the same prefix_rows = P keys: those of the ONE sequence whose block-table row is
 * prefix_table (device, P / page_rows int32).  d->k / d->v are the page pools with the pitches and page strides of
 * npm_mha_decode_fwd_paged (kv_f16 != 0: halves, counted in halves, multiples of 8); d->kv_len, d->causal, d->ctx and d->lse are
 * not read.  P is a positive multiple of page_rows, a power of two >= 16: every 16-key tile is full, so there are no lengths, no
 * masked score and no redirected load.  A block covers 64 (head of the group, row) pairs of one K / V head, the batch folded into
 * the row index, and its four waves share every tile through LDS as in npm_mha_prefill_fwd; the KEYS are split over `splits`
 * blocks in contiguous ranges of ceil(P / 16 / splits) tiles (a split past the last tile is empty, which is allowed).  Every
 * (split s, row r, head h) with t < new_lens[b] (NULL: every row) writes
 *   part_ctx[((s * R + r) * heads + h) * head_dim ..]   softmax-weighted V over the split's keys, normalised within the split
 *   part_lse[(s * R + r) * heads + h]                   log sum exp of the split's scaled scores (-inf and ctx 0 for an empty split)
 * and other rows read no q and write nothing.  The caller provides splits * R * heads * (head_dim + 1) floats, part_ctx 16-byte
 * aligned.  Exact fp32 MFMA, no atomics; a row's partials depend on its q, the prefix and `splits` only (bitwise the same at any
 * batch); the f16 call is bitwise the f32 call on the rounded values.  head_dim in {16, 32, 64, 128}, else NPM_E_UNSUPPORTED.
 * npm_last_prefix_kernel(): "mha_prefix_kernel D=<head_dim> R=<rows> rows=64 prefix=<P> splits=<splits> paged=<page_rows>", then
 * " kv=f16"; "" before the first call.
 * npm_mha_prefix_splits: the split count for this shape (rows = R) under NPM_TUNE_PREFIX_SPLITS: row tiles x kv_heads x splits
 * of about two blocks per compute unit, no split shorter than 128 keys.  Shape arguments and the knob only.
 *
 * npm_attn_combine: for every row with t < new_lens[b] (NULL: every row) and every head, the `splits` partials in split order and
 * then, LAST, the result the caller's suffix call left in ctx [B, T, heads, head_dim] (pitch ctx_pitch) and lse [B, heads, T]:
 *   M = max lse_i,  w_i = exp(lse_i - M) (0 by selection for lse_i = -inf, whose ctx is not read),
 *   ctx = (sum w_i ctx_i) / sum w_i, summed in that order,  lse = M + log sum w_i (stored when store_lse != 0).
 * The suffix call is the paged entry point of the cache with block_table + P / page_rows, lengths max(kv_lens[b] - P, 0) and
 * d->kv_len less P: a row's causal limit is the same number in suffix coordinates.  Rows with t >= new_lens[b] are stored as
 * ctx = 0 (lse = -inf with store_lse), by selection.  lse is required: it carries the suffix weights in. */
#define NPM_PREFIX_MAX_SPLITS 1024
int npm_kv_copy_pages(void *pool, int64_t page_stride_bytes, int64_t row_bytes, const int32_t *src_pages, const int32_t *dst_pages,
                      const int32_t *rows, int32_t n);
/* npm_kv_copy_pages_planes: npm_kv_copy_pages in `planes` pools at once.  Plane p is the pool at pool + p * plane_stride_bytes (a
 * multiple of 16; at least one page with more than one plane) with the page stride and row bytes of the call, and the SAME n pairs
 * are copied in every plane by one launch: the K and V pools of all layers of a layered cache, which share one block table.
 * Everything else is npm_kv_copy_pages, which is unchanged; planes == 0 is NPM_OK and nothing is launched. */
int npm_kv_copy_pages_planes(void *pool, int64_t page_stride_bytes, int64_t row_bytes, const int32_t *src_pages,
                             const int32_t *dst_pages, const int32_t *rows, int32_t n, int32_t planes, int64_t plane_stride_bytes);
int npm_mha_prefix_supported(int head_dim);
int npm_mha_prefix_fwd(const npm_mha_decode *d, const int32_t *new_lens, const int32_t *prefix_table, int32_t page_rows,
                       int32_t prefix_rows, int32_t splits, float *part_ctx, float *part_lse, int32_t kv_f16);
int npm_mha_prefix_splits(int rows, int heads, int kv_heads, int prefix_rows);
const char *npm_last_prefix_kernel(void);
int npm_attn_combine(const float *part_ctx, const float *part_lse, int32_t splits, float *ctx, int64_t ctx_pitch, float *lse,
                     int32_t batch, int32_t new_tokens, int32_t heads, int32_t head_dim, const int32_t *new_lens, int32_t store_lse);

/* ---- rotary position embedding (RoPE), in place ----
 * Rotates the first `heads` heads of every row b * tokens + t (b < batch, t < tokens) of x: head h of a row is the head_dim floats
 * at x[row * pitch + h * head_dim]; whatever lies behind them in the row (the V heads of a packed [B, T, H + 2 Hkv, D] projection,
 * when heads = H + Hkv) is not touched.  With half = head_dim / 2 (head_dim even), element i < half is paired with element
 * i + half ("rotate-half"), and for the row's position p = (at_lens ? at_lens[b] : at) + t
 *   c = cos[p * half + i], s = sin[p * half + i]      (fp32 tables [table_rows, half] made by the caller: the angle of (p, i) is
 *                                                      p * base ** (-i / half); no trigonometry is computed on the device)
 *   inverse == 0:  y[i] = x[i] * c - x[i + half] * s    y[i + half] = x[i + half] * c + x[i] * s
 *   inverse != 0:  y[i] = x[i] * c + x[i + half] * s    y[i + half] = x[i + half] * c - x[i] * s     (the transpose: for gradients)
 * Every product and every sum is rounded to fp32 on its own (no fused multiply-add): bitwise what NumPy gives for these
 * expressions on float32 arrays.  at_lens: device array of batch int32, read by the kernel (NULL: the scalar `at`).  A row whose
 * position is outside 0 .. table_rows - 1 is left untouched, and nothing past a table is read, whatever at_lens holds; with the
 * scalar, at < 0 or at + tokens > table_rows is NPM_E_BAD_ARGUMENT.  NPM_E_BAD_ARGUMENT too for an odd head_dim, a size < 1,
 * pitch < heads * head_dim and a NULL x, cos or sin.  head_dim % 8 == 0, pitch % 4 == 0 and 16-byte aligned x, cos and sin move
 * 16 bytes per access; everything else takes a scalar kernel with the same arithmetic and the same bits. */
int npm_rope(float *x, int64_t pitch, int32_t batch, int32_t tokens, int32_t heads, int32_t head_dim, const float *cos,
             const float *sin, int32_t table_rows, int32_t at, const int32_t *at_lens, int32_t inverse);

/* npm_rope_kv_append: npm_rope and the two appends of a self-attention step in ONE launch (a decode step is launch-bound).  qkv is
 * the packed projection of the step, rows b * tokens + t of (heads + 2 kv_heads) * head_dim floats with row pitch `pitch`: the q
 * heads, then the k heads, then the v heads.
 *  1. The first heads + kv_heads heads of every row are rotated in place, exactly as
 *       npm_rope(qkv, pitch, batch, tokens, heads + kv_heads, head_dim, cos, sin, table_rows, at, at_lens, 0)
 *     leaves them: padded rows t >= new_lens[b] too, a row whose position is outside the table untouched.  cos == sin == NULL: no
 *     rotation, and q is not touched at all.
 *  2. For t < new_lens[b] (NULL: every t) the k heads, as step 1 left them, and the v heads are stored at row at_b + t of sequence b
 *     of k_cache and v_cache, at_b = at_lens ? at_lens[b] : at.  Both caches have the row pitch cache_pitch and the stride
 *     cache_stride, in elements of the cache: between sequences, or with block_table (device int32 [batch, table_pitch], page_rows a
 *     power of two >= 16) between pages, as npm_kv_append_paged has it.  kv_f16 != 0: the caches hold IEEE halves, converted as
 *     npm_kv_append_f16 converts (round to nearest even).  These are exactly the bytes npm_kv_append / _varlen / _paged / _f16 store
 *     from that buffer; no other byte of a cache is written.
 * Bit for bit the three launches: every product and sum of the rotation is rounded on its own.  head_dim % 8 == 0 and 16-byte
 * aligned qkv, cos and sin move 16 bytes per access (8 per store into an fp16 cache); everything else takes a scalar instance with
 * the same bits.  Argument errors are those of the calls it fuses: with tables npm_rope's (a NULL cos or sin alone, sizes < 1, an odd
 * head_dim, a scalar `at` outside the table); then the appends' -- a negative size or `at`, NPM_OK and nothing launched for
 * batch == 0 or tokens == 0, a NULL pointer, k / v parts of qkv or caches that are not 16-byte aligned, pitch % 4, kv_heads *
 * head_dim or a cache pitch / stride that is not a multiple of 4 (8 for halves), pitch < (heads + 2 kv_heads) * head_dim,
 * cache_pitch < kv_heads * head_dim, and with a block_table a NULL at_lens, a bad page_rows or cache_stride < page_rows *
 * cache_pitch -- all NPM_E_BAD_ARGUMENT.  Its own: head_dim is even with or without tables (elements move in pairs).
 * npm_last_rope_append_kernel(): "rope_kv_append_kernel D=<head_dim> vec=<0|1> rope=<0|1> varlen=<0|1> paged=<page_rows or 0>
 * kv=<f32|f16>"; "" before the first launch. */
int npm_rope_kv_append(float *qkv, int64_t pitch, int32_t batch, int32_t tokens, int32_t heads, int32_t kv_heads, int32_t head_dim,
                       const float *cos, const float *sin, int32_t table_rows, int32_t at, const int32_t *at_lens,
                       const int32_t *new_lens, void *k_cache, void *v_cache, int64_t cache_pitch, int64_t cache_stride,
                       const int32_t *block_table, int32_t table_pitch, int32_t page_rows, int32_t kv_f16);
const char *npm_last_rope_append_kernel(void);

/* ---- skinny-M GEMM: the matrix products of a decode step (inference) ----
 * C[M, N] = epilogue(alpha * A[M, K] op(B)) for 1 <= M <= NPM_SKINNY_MAX_M rows, described by the same npm_gemm as npm_sgemm.  These
 * are the products np.matmul / np.einsum make at M = B T rows of new tokens: the q / k / v and output projections of
 * layers/attentions.py:88-100,114-117 (B stored [N, K]: trans_b = 1) and x @ w + b of layers/mlp.py:23-24 with the ReLU of
 * activations.py:14-15 and the residual additions of transformer.py:39,53 (B stored [K, N]: trans_b = 0).  npm_sgemm runs them on
 * its 128-row tiles with ceil(N / 128) blocks that each walk all of K; here the weights are the stream: every weight element is
 * loaded once, by one wave, straight into registers; a block owns 64 columns and a range of K, and the ranges of a column strip are
 * merged in a fixed order by a second kernel (no atomics: bitwise reproducible).  The split count and the order in which the k
 * terms of an output element are added depend on (N, K, trans_b) and NPM_TUNE_SKINNY_SPLITS only, never on M or on the row's
 * position: row r of an M-row call is bitwise the M = 1 call on that row.  Rows >= M of A's buffer, rows >= N of a [N, K] B and
 * columns >= N of a [K, N] B are never read.
 * Exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) whatever npm_set_math says; npm_last_math() is left alone.
 * Supported: trans_a = 0, batch0 = batch1 = 1, n and k multiples of 16 (>= 16), a / b / c (and bias / residual / aux when used) 16-byte
 * aligned, lda / ldb / ldc / ldr / ldaux multiples of 4 floats and at least the row widths, epilogue any of NPM_EPI_BIAS,
 * NPM_EPI_RESIDUAL and one of NPM_EPI_RELU / NPM_EPI_RELU_SAVE, colsum = bsum = asum = rowdot = NULL, split_k = 0.  Everything else is
 * NPM_E_UNSUPPORTED before anything is launched or written (callers then use npm_sgemm). */
#define NPM_SKINNY_MAX_M 64
#define NPM_SKINNY_MAX_SPLITS 64
int npm_sgemm_skinny(const npm_gemm *g);
/* 1 when npm_sgemm_skinny takes this call, else 0; never sets an error. */
int npm_sgemm_skinny_supported(const npm_gemm *g);
/* The number of K splits npm_sgemm_skinny uses for this shape under the current NPM_TUNE_SKINNY_SPLITS: shape arguments only. */
int npm_sgemm_skinny_splits(int n, int k, int trans_b);
/* What the most recent npm_sgemm_skinny launched: "sgemm_skinny_kernel <NT|NN> M=<m> N=<n> K=<k> rb=<16-row blocks> splits=<n>
 * nt=<0|1>" (nt: nontemporal weight loads); "" before the first call. */
const char *npm_last_skinny_kernel(void);

/* ---- half-precision weight copies for the skinny-M GEMM (opt-in; everything above is unchanged) ----
 * A decode step is a stream over its weights, so the six matrices it reads may be kept a second time as IEEE fp16 and streamed at
 * half the bytes.  The pattern is the fp16 cache's: convert ONCE (npm_cvt_f32_f16), read in place, accumulate in fp32.
 *
 * npm_cvt_f32_f16 converts a pitched 2-D array (rows x cols; each pitch counts elements of its own side's type and is >= cols) with
 * round to nearest even -- bit for bit NumPy's astype(float16), subnormal results kept; |x| >= 65520 becomes +-inf: there is NO
 * clamp, as in npm_kv_append_f16 -- and npm_cvt_f16_f32 is the exact way back.  Row kernels: 16-byte accesses when cols and the
 * fp16 pitch are multiples of 8, the fp32 pitch is a multiple of 4 and both pointers are 16-byte aligned, else one element per
 * thread with the same bits.  rows == 0 or cols == 0 returns NPM_OK whatever the pointers are; a negative size, a pitch below
 * cols or a NULL pointer is NPM_E_BAD_ARGUMENT.
 *
 * npm_sgemm_skinny_w16 is npm_sgemm_skinny -- the same descriptor, rules, epilogues, split count (npm_sgemm_skinny_splits), combine
 * kernel and refusals -- except that g->b points at halves: ldb counts halves and is a multiple of 8, b is 16-byte aligned.  A, C,
 * bias, residual, aux and alpha stay fp32.  Each weight element is converted exactly in registers (v_cvt_f32_f16) and enters the
 * same v_mfma_f32_16x16x4_f32 chain, contraction off.  The kernel keeps the lane-to-k mapping of the fp32 instance (a lane's
 * 16-byte weight load becomes an 8-byte one), so the call is BITWISE
 * npm_sgemm_skinny on a B that holds the rounded values as floats, and inherits its identities: row r of an M-row call is the
 * M = 1 call on that row, two identical calls and either load hint give the same bits, nothing outside the operands is read.  The
 * nontemporal rule (NPM_TUNE_SKINNY_NT = 0) counts the bytes stored, 2 N K.  npm_last_skinny_kernel() afterwards: the fp32 string
 * followed by " w=f16".  Measured on one MI355X (tools/skinny_w16_bench.py): at d 1024 / hidden 4096 the six products
 * of a decode step are bound by their two launches, not by weight bytes -- w16 / fp32 is 0.85 - 0.88 on dense2 (K 4096) and 0.93 - 0.94
 * on dense1 at M <= 16, within the spread elsewhere; a decode step was 1 - 3 % slower on the variant with four chunks per step and has not been measured on
 * the shipped instance.  What the copies buy today is the rounded
 * model; they cost 2 N K more bytes of memory. */
int npm_cvt_f32_f16(const float *src, int64_t src_pitch, void *dst, int64_t dst_pitch, int64_t rows, int64_t cols);
int npm_cvt_f16_f32(const void *src, int64_t src_pitch, float *dst, int64_t dst_pitch, int64_t rows, int64_t cols);
int npm_sgemm_skinny_w16(const npm_gemm *g);
/* 1 when npm_sgemm_skinny_w16 takes this call, else 0; never sets an error. */
int npm_sgemm_skinny_w16_supported(const npm_gemm *g);

/* ---- token generation: rows by index, the gradient of that lookup, and sampling on the device ----
 * npm_take_rows: dst[r, :] = src[idx[r], :] for r < n, both sides with a row pitch in floats (>= cols); idx: device array of n int32.
 * An index below 0 or >= src_rows gives a row of zeros and the source is not read for it (a finished sequence carries token -1 and
 * the decoder wants finite padding).  The embedding lookup, and picking the last row of every sequence of a ragged chunk so that
 * the vocabulary projection runs on B rows.  cols % 4 == 0, pitches % 4 == 0 and 16-byte aligned src and dst move 16 bytes per
 * access, everything else one float per thread: a copy, the same bits.  n == 0 or cols == 0 returns NPM_OK whatever the pointers
 * are; a negative size, a pitch below cols or a NULL pointer is NPM_E_BAD_ARGUMENT.
 *
 * npm_embedding_bwd: the gradient of the lookup without atomics.  The caller sorts the rows of dy stably by token: order[j] is the
 * j-th row of dy in that order, segment s = starts[s] .. starts[s + 1] - 1 (starts has distinct + 1 entries, every segment at least
 * one row) holds the rows of token tokens[s], in ascending row order.  dw[tokens[s], c] = ((dy[order[first], c] + dy[order[first
 * + 1], c]) + ...) in fp32, in that order: deterministic, bit for bit a NumPy float32 loop.  Rows of dw that no segment names are
 * not written (the caller zeroes dw first).  One block per segment and chunk of 256 columns.  All arrays are device arrays;
 * nothing is checked on the device: order must name rows of dy and tokens rows of dw. */
int npm_take_rows(const float *src, int64_t src_pitch, int64_t src_rows, const int32_t *idx, float *dst, int64_t dst_pitch, int64_t n,
                  int64_t cols);
int npm_embedding_bwd(const float *dy, int64_t dy_pitch, const int32_t *order, const int32_t *starts, const int32_t *tokens,
                      int32_t distinct, float *dw, int64_t dw_pitch, int64_t cols);

/* npm_sample_rows: one launch samples one token per row of a [batch, vocab] fp32 logit matrix; every row has its own parameters
 * (the sequences of a continuous batch do not share them).  All pointers are device pointers.  One row, with z its logits:
 *  1. A row that holds a NaN or +inf, or whose every logit is -inf, is invalid: token = -1, kept = 0, prob = 0; it never faults.
 *     So is a row whose temperature is not >= 0 or whose top_p is not > 0.  -inf logits are otherwise legal (a masked
 *     vocabulary); such tokens are never kept.
 *  2. Order: i comes before j when z_i > z_j, or when z_i == z_j and i < j; -0.0 == 0.0.
 *  3. Greedy: temperature == 0 or top_k == 1 (or a temperature so small that 1 / t is not finite in fp32): the token is the first
 *     in that order, kept = 1, prob = 1.
 *  4. Otherwise K1 is the first min(top_k, finite count) tokens in order; top_k <= 0: every finite token.  Exact: logits only.
 *  5. Weights: w_i = floor(q_i * 2^32) as an unsigned 64-bit integer, q_i = exp((z_i - zmax) * (1 / t)) with the difference, the
 *     reciprocal, the product and the exponential each in fp32; the largest logit has w = 2^32 exactly.  Every mass after this
 *     point is an integer sum of w: no result depends on the order in which anything is added.
 *  6. Top-p: K2 is the shortest prefix of K1 in order whose mass reaches max(1, floor((double)top_p * (double)W1)), W1 the mass
 *     of K1; top_p >= 1: K2 = K1.  kept = |K2|, Wk its mass.
 *  7. Draw: u24 = word0 >> 8, word0 the first word of Philox4x32-10 with counter (draw lo, draw hi, 0, 0) and key (seed lo, seed
 *     hi).  target = floor(Wk * u24 / 2^24), exact in integers.  The token is the first i of K2 IN INDEX ORDER whose running mass
 *     S_i exceeds target.  prob = (float)((double)w_token / (double)Wk).
 *  8. Then draw[b] += 1 for every active row: greedy and invalid rows included.  With active != NULL and active[b] == 0 the row is
 *     left alone: no logit of it is loaded, draw[b] stays, token = -1, kept = 0, prob = 0.
 * Hence a row's result depends on nothing outside that row, the launch is bitwise reproducible, and row b of a batch is the
 * batch-1 call on that row with the same seed and counter.
 * One block per row; a row of at most NPM_SAMPLE_LDS_ROW logits is kept in LDS, a longer one is read again from L2.  A 16-byte
 * aligned `logits` with pitch % 4 == 0 is loaded 16 bytes per lane, anything else one float per lane, with the same results.
 * NPM_E_BAD_ARGUMENT before anything is launched: s == NULL, batch < 1, vocab outside 1 .. NPM_SAMPLE_MAX_VOCAB, pitch < vocab, a
 * NULL logits, temperature, top_k, top_p, seed, draw or token (active, kept and prob may be NULL). */
#define NPM_SAMPLE_LDS_ROW 32768
#define NPM_SAMPLE_MAX_VOCAB (1 << 20)
typedef struct npm_sample {
    const float *logits; int64_t pitch;          /* row b starts at logits + b * pitch, pitch >= vocab */
    int32_t batch, vocab;                        /* 1 <= vocab <= 1 << 20 */
    const float *temperature;                    /* [batch], >= 0; 0 = greedy */
    const int32_t *top_k;                        /* [batch], <= 0 = off */
    const float *top_p;                          /* [batch], (0, 1]; >= 1 = off */
    const uint64_t *seed; uint64_t *draw;        /* [batch]; draw[b] is advanced by 1 for every active row */
    const int32_t *active;                       /* NULL = all, or [batch]: 0 = leave the row alone */
    int32_t *token;                              /* [batch] out; -1 for an inactive or invalid row */
    int32_t *kept; float *prob;                  /* [batch] out, either may be NULL */
} npm_sample;
int npm_sample_rows(const npm_sample *s);
/* What the most recent npm_sample_rows or npm_verify_rows launched: "sample_rows_kernel <vec|scalar> B=<batch> V=<vocab>
 * row=<lds|global>", or "verify_rows_kernel <vec|scalar> B=<batch> rows=<rows> V=<vocab> row=<lds|global> history=<0|1>"; ""
 * before the first call. */
const char *npm_last_sample_kernel(void);

/* ---- speculative decoding: drafts by prompt lookup, verified by sampling ----
 * npm_verify_rows: a speculative step fed every slot b its last token and up to T = rows - 1 drafted tokens, and the model
 * returned rows = T + 1 logit rows per slot, row (b, r) at logits + (b * rows + r) * pitch.  Row r is what follows the r-th
 * drafted token, so it counts only while every drafted token before it was the token sampled.  All pointers are device pointers.
 * Per slot b, with n = n_draft[b] (0 .. rows - 1 drafted tokens; below 0: the slot is inactive; above rows - 1 is read as
 * rows - 1):
 *  1. For r = 0 .. n, s[r] is what npm_sample_rows returns for that logit row with slot b's temperature, top_k, top_p and seed
 *     and the counter draw[b] + r (64 bits: the carry into the high word counts) -- the same device function samples the row in
 *     both entry points.  Rows r > n are not loaded.
 *  2. a is the smallest r in 0 .. n with r == n or s[r] != draft[b * draft_pitch + r].  An invalid row has s[r] = -1 and a draft
 *     entry below 0 never matches, so acceptance stops there.
 *  3. token[b, 0 .. a] = s[0 .. a] with their kept and prob; token[b, r > a] = -1 with kept 0 and prob 0 (token, kept and prob are
 *     [batch, rows], dense); accepted[b] = a; draw[b] += a + 1.
 *  4. With history != NULL: the tokens token[b, 0 .. a] that are >= 0 are written to history[b * history_pitch + history_len[b]
 *     ...] in order and history_len[b] grows by their number.  Nothing is written at or past history_cap: a token that does not
 *     fit is dropped and history_len[b] stops at history_cap (the caller checks the room before the launch).
 *  5. An inactive slot: token -1, kept 0, prob 0 in every column, accepted 0; draw[b] and history_len[b] stay and no logit of
 *     the slot is read.
 * Hence the tokens a slot emits over any number of calls are the tokens npm_sample_rows gives it from the same logit rows one
 * call at a time, seed for seed and counter for counter, whatever was drafted.  Two launches: one block of 1024 threads per
 * (slot, row), then one thread per slot for steps 2 - 4; integers only between them, so the call is bitwise reproducible and
 * slot b of a batch is the batch-1 call on that slot.
 * NPM_E_BAD_ARGUMENT before anything is launched: v == NULL, batch < 1, rows outside 1 .. NPM_VERIFY_MAX_ROWS, vocab outside
 * 1 .. NPM_SAMPLE_MAX_VOCAB, pitch < vocab, batch * rows >= 2^31, a NULL logits, temperature, top_k, top_p, seed, draw, n_draft,
 * token or accepted, with rows > 1 a NULL draft or draft_pitch < rows - 1, with a history a NULL history_len, history_cap < 1 or
 * history_pitch < history_cap (kept, prob and history may be NULL). */
#define NPM_VERIFY_MAX_ROWS 64
typedef struct npm_verify {
    const float *logits; int64_t pitch;          /* row (b, r) starts at logits + (b * rows + r) * pitch, pitch >= vocab */
    int32_t batch, rows, vocab, history_cap;     /* rows = T + 1 in 1 .. 64 */
    const float *temperature;                    /* the five per-slot vectors of npm_sample, [batch] each */
    const int32_t *top_k;
    const float *top_p;
    const uint64_t *seed; uint64_t *draw;        /* draw[b] is advanced by accepted[b] + 1 for every active slot */
    const int32_t *draft; int64_t draft_pitch;   /* [batch, >= rows - 1]: the drafted tokens the rows were computed behind */
    const int32_t *n_draft;                      /* [batch], -1 .. rows - 1; below 0 = inactive */
    int32_t *token, *accepted;                   /* out: [batch, rows] and [batch] */
    int32_t *kept; float *prob;                  /* [batch, rows] out, either may be NULL */
    int32_t *history; int64_t history_pitch;     /* NULL, or [batch, history_cap] with a row pitch: the tokens of every slot so far */
    int32_t *history_len;                        /* [batch], advanced by the tokens appended */
} npm_verify;
int npm_verify_rows(const npm_verify *v);

/* npm_ngram_draft: the draft of every slot from its own token history h = history[b * history_pitch ...] of L = history_len[b]
 * tokens (read as min(L, history_cap)), by prompt lookup.  T = max_draft, m_max = min(T, limit[b]) (limit NULL: T); a slot with
 * L <= 0 or limit[b] < 0 is inactive.  Exact, integers only:
 *  1. n walks from nmax down to nmin; an n with L < n + 1 is skipped.
 *  2. Its candidates are the j in 0 .. L - n - 1 with h[j + i] == h[L - n + i] for every i < n: earlier occurrences of the last n
 *     tokens (they may overlap the last one).  The first n that has a candidate is used.
 *  3. Among them the LARGEST j with j + n + m_max <= L -- the most recent occurrence followed by a whole draft -- else the
 *     SMALLEST candidate, which has the longest continuation.  m = min(m_max, L - (j + n)).
 *  4. No candidate at any n, or m_max <= 0: m = 0.
 *  5. chunk[b, 0] = h[L - 1], chunk[b, 1 + i] = h[j + n + i] for i < m, -1 behind that (chunk is [batch, T + 1], dense);
 *     n_new[b] = 1 + m.  An inactive slot gets a row of -1 and n_new[b] = 0.
 * chunk is what the model is fed; chunk + 1 with pitch T + 1 is npm_verify's draft and n_new[b] - 1 its n_draft[b].  One block
 * of 256 threads per slot; the history is read once per n.  NPM_E_BAD_ARGUMENT before the launch: batch < 1, max_draft outside
 * 0 .. NPM_VERIFY_MAX_ROWS - 1, nmin < 1, nmax < nmin, nmax > NPM_DRAFT_MAX_NGRAM, history_cap < 1, history_pitch < history_cap,
 * a NULL history, history_len, chunk or n_new. */
#define NPM_DRAFT_MAX_NGRAM 8
int npm_ngram_draft(const int32_t *history, int64_t history_pitch, int32_t history_cap, const int32_t *history_len,
                    const int32_t *limit, int32_t batch, int32_t max_draft, int32_t nmax, int32_t nmin, int32_t *chunk,
                    int32_t *n_new);
/* What the most recent npm_ngram_draft launched: "ngram_draft_kernel B=<batch> T=<max_draft> ngram=<nmax>..<nmin> cap=<cap>". */
const char *npm_last_draft_kernel(void);

/* ---- beam search: the best 2 W of W x V continuations per prompt, and the split, on the device ----
 * npm_beam_step: slots are `groups` groups of `width` beams, slot g W + w, 1 <= W <= NPM_BEAM_MAX_WIDTH, C = 2 W candidates per
 * group.  logits: fp32 [G W, vocab] with a row pitch; cum: fp32 [G W], the beams' running scores, -inf for a dead beam, updated in
 * place; eos: the end-of-sequence token, below 0 for none.  All pointers are device pointers.
 *  1. A dead row (cum == -inf, or NaN) is NOT READ and contributes nothing.
 *  2. A live row that holds a NaN or +inf, or whose every logit is -inf, is invalid: it contributes nothing and never faults.
 *     -inf logits are otherwise legal (a masked token) and never candidates.
 *  3. Row order is npm_sample_rows': i before j when z_i > z_j, or z_i == z_j and i < j; -0.0 == 0.0.
 *  4. The row normaliser is npm_sample_rows' mass at temperature 1: W1 = sum over the finite tokens of floor(expf(z_i - zmax) *
 *     2^32), difference and exponential in fp32, as an unsigned 64-bit INTEGER sum: nothing depends on the order in which lanes,
 *     waves or LDS atomics add.
 *  5. n = log((double)W1 * 2^-32) in fp64; lse = (float)((double)zmax + n), a zmax of -0.0 read as 0.0.
 *  6. Candidate (w, i) has score s = (float)((((double)cum_w - (double)zmax_w) - n_w) + (double)z_i): fp64 throughout, in that
 *     order, ONE rounding to fp32.  Rounding is monotone, so a row's candidates in row order have non-increasing scores.
 *  7. The candidates of a group are totally ordered: the larger score first, then the smaller beam w, then row order.  Hence only
 *     the first min(C, finite count) tokens of a row can matter.
 *  8. cand_slot (g W + w), cand_token and cand_score, [G, C] each, are the first C candidates of every group in that order;
 *     -1 / -1 / -inf behind the last candidate that exists.
 *  9. The split: walking the C candidates in order, one whose token is eos is FINISHED when its position is below W and ignored
 *     otherwise -- either way it never becomes a beam; the others become the next beams 0, 1, ... in order until W are placed.  (A
 *     row holds eos once, so C = 2 W candidates always hold W others when they exist.)  eos < 0: no candidate is finished.
 * 10. Per slot g W + j of the NEXT step: parent (the slot beam j continues; -1: dead), ids (its token; -1: dead -- npm_take_rows
 *     turns that into a row of zeros), cum (written in place: its score; -inf: dead).  lse [G W] belongs to the rows of THIS
 *     step: the log-sum-exp of row g W + w, NaN for a dead or invalid row; z_i - lse is token i's log-probability.
 * 11. The caller chooses where the seven results live: np_modeling_amd/beam.py puts them in one allocation, one host copy a step.
 * 12. Hence a group's results depend on nothing outside its own W rows and cum entries, group g of a batch is the groups = 1 call
 *     on that group, and a launch is bitwise reproducible.
 * Two launches: one block of 1024 threads per row (npm_sample_rows' passes -- the row in LDS up to NPM_SAMPLE_LDS_ROW logits,
 * 16-byte loads for a 16-byte aligned `logits` with pitch % 4 == 0, else one float per lane with the same results -- then the at
 * most C survivors ranked by one wavefront), which leaves each row's list in `workspace`; then one block per group merges W
 * lists and splits.  workspace: NPM_BEAM_WORKSPACE_BYTES(groups, width) bytes, 4-byte aligned, contents unspecified before and
 * after.  NPM_E_BAD_ARGUMENT before anything is launched: s == NULL, groups < 1, width outside 1 .. NPM_BEAM_MAX_WIDTH, vocab
 * outside 1 .. NPM_SAMPLE_MAX_VOCAB, pitch < vocab, groups * width * C >= 2^31, a NULL pointer, a workspace that is too small or
 * misaligned. */
#define NPM_BEAM_MAX_WIDTH 32
#define NPM_BEAM_WORKSPACE_BYTES(groups, width) ((int64_t)4 * (groups) * (width) * (1 + 4 * (int64_t)(width)))
typedef struct npm_beam {
    const float *logits; int64_t pitch;          /* row g W + w starts at logits + (g W + w) * pitch, pitch >= vocab */
    int32_t groups, width, vocab, eos;
    float *cum;                                  /* [G W] in and out */
    int32_t *cand_slot, *cand_token; float *cand_score;   /* [G, 2 W] out */
    int32_t *parent, *ids;                       /* [G W] out: the next step's slots */
    float *lse;                                  /* [G W] out: this step's rows */
    void *workspace; int64_t workspace_bytes;
} npm_beam;
int npm_beam_step(const npm_beam *s);
/* What the most recent npm_beam_step launched: "beam_rows_kernel <vec|scalar> G=<groups> W=<width> V=<vocab> row=<lds|global>"
 * (npm_logprob_rows: "logprob_rows_kernel <vec|scalar> R=<rows> V=<vocab> top=<top_n> row=<lds|global>"); "" before the first call. */
const char *npm_last_beam_kernel(void);

/* npm_logprob_rows: clauses 2 - 6 of npm_beam_step with cum = 0, per row and without the beam bookkeeping -- the same kernel,
 * instantiated without the workspace.  logits: fp32 [rows, vocab] with a row pitch.  Per row r, with zmax, W1 and
 * n = log((double)W1 * 2^-32) as npm_beam_step defines them:
 *  1. lse[r] = (float)((double)zmax + n): npm_beam_step's lse of the same row bit for bit.
 *  2. Token i's log-probability is (float)(((0.0 - (double)zmax) - n) + (double)z_i); that of a -inf token is -inf.
 *  3. top_token / top_logprob [rows, top_n], top_n in 0 .. 64: the first min(top_n, finite count) tokens in the sampler's order
 *     with their log-probabilities, -1 / -inf behind them.
 *  4. With ids != NULL: chosen[r] is the log-probability of ids[r], NaN when that id is >= vocab.  It is the expression of 2, so a
 *     chosen token among the top n equals that entry bit for bit.
 *  5. With ids != NULL a row with ids[r] < 0 is NOT LOADED: lse NaN, chosen NaN, top -1 / -inf (the rows a verify step rejected,
 *     the inactive slots).  An invalid row (a NaN or +inf, or every logit -inf) gives the same outputs and never faults.
 * One launch, one block of 1024 threads per row; bitwise reproducible; a row depends on nothing outside it.
 * NPM_E_BAD_ARGUMENT before the launch: p == NULL, rows < 1, vocab outside 1 .. NPM_SAMPLE_MAX_VOCAB, pitch < vocab, top_n outside
 * 0 .. 64, a NULL logits or lse, ids without chosen, top_n > 0 without top_token or top_logprob. */
typedef struct npm_logprob {
    const float *logits; int64_t pitch;          /* row r starts at logits + r * pitch, pitch >= vocab */
    int32_t rows, vocab, top_n;
    const int32_t *ids;                          /* NULL, or [rows]: the token whose log-probability chosen reports; < 0: skip the row */
    float *lse, *chosen;                         /* [rows] out; chosen may be NULL when ids is */
    int32_t *top_token; float *top_logprob;      /* [rows, top_n] out; may be NULL when top_n == 0 */
} npm_logprob;
int npm_logprob_rows(const npm_logprob *p);

/* ---- logit processors: penalties, bias, bans and the minimum length, applied in place before sampling ----
 * npm_logits_process edits the logit rows npm_sample_rows (rows = 1) or npm_verify_rows (rows = T + 1) is about to read: row (b, r)
 * starts at logits + (b * rows + r) * pitch.  All pointers are device pointers.  Per slot b:
 *   L = history_len[b] clipped to 0 .. history_cap (history == NULL: 0); P = prompt_len[b] clipped to 0 .. L (NULL: 0);
 *   n = 0 with n_draft == NULL (rows must be 1), else min(n_draft[b], rows - 1).
 * A slot with active != NULL and active[b] == 0, or with n_draft[b] < 0, is inactive: none of its logits is read or written.
 * Rows r > n of an active slot are not touched.  For an active slot and r in 0 .. n:
 *   S_r = history[b, 0 .. L) followed by draft[b, 0 .. r); an id outside 0 .. vocab - 1 anywhere in it is ignored;
 *   seen_i: token i occurs in S_r; c_i: its occurrences at positions >= P of S_r (draft positions always count);
 *   gen_r = (L - P) + r.
 * The row's logits z change as follows, every operation rounded to fp32 on its own (no contraction; the division is IEEE):
 *  1. Repetition: where seen_i and repetition[b] is finite, positive and != 1: z_i = z_i > 0 ? z_i / rep : z_i * rep.
 *  2. Frequency and presence: where c_i > 0, unless frequency[b] and presence[b] are both zero:
 *     z_i = z_i - frequency[b] * (float)c_i, then z_i = z_i - presence[b].
 *  3. Bias: for each of the first min(bias_count[b], bias_cap) entries whose index lies in the vocabulary: z_i = z_i + bias_value.
 *     -inf bans the token.  An index listed twice takes the entry with the smallest position only.
 *  4. Minimum length: when 0 <= eos[b] < vocab and gen_r < min_new[b]: z_eos = -inf.
 * Every other logit, the pitch padding and everything outside the rows are NOT WRITTEN.  NULL parameter vectors: repetition 1,
 * presence and frequency 0, eos or min_new NULL: no rule 4.  A neutral slot (no rule applies: rep 1, both penalties 0, no bias
 * entry, no eos rule with gen_0 < min_new) returns before its first load of a logit.
 * Any int32 content of history, draft, bias_index and eos is legal and leads to no access outside the slot's rows and its
 * workspace row.  workspace: int32 [batch, vocab], ALL ZERO on entry and all zero again when the call's work has finished.
 * Hence a row's result is a pure function of the row and the slot's own history, draft and parameters; the launch is bitwise
 * reproducible (integer atomics only); slot b of a batch is the batch-1 call on that slot; row r of a chunk is the rows = 1 call
 * on that row with draft[b, 0 .. r) appended to the history.  Calling twice applies the rules twice.
 * One launch, one block per slot; O(L + distinct tokens * (n + 1) + bias entries) work per slot, nothing O(vocab).
 * NPM_E_BAD_ARGUMENT before anything is launched: p == NULL, a NULL logits or workspace, batch < 1, rows outside
 * 1 .. NPM_VERIFY_MAX_ROWS, vocab outside 1 .. NPM_SAMPLE_MAX_VOCAB, pitch < vocab, batch * rows >= 2^31, rows > 1 without draft or
 * n_draft or with draft_pitch < rows - 1, a history without history_len or with history_cap < 1 or history_pitch < history_cap,
 * bias_cap outside 0 .. NPM_LOGITS_MAX_BIAS, bias_cap > 0 with a NULL bias_index, bias_value or bias_count. */
#define NPM_LOGITS_MAX_BIAS 256
typedef struct npm_logits {
    float *logits; int64_t pitch;                /* edited in place */
    int32_t batch, rows, vocab, history_cap;
    const int32_t *history; int64_t history_pitch;   /* NULL, or [batch, history_cap] with a row pitch (NgramDrafter's layout) */
    const int32_t *history_len;                  /* [batch] */
    const int32_t *prompt_len;                   /* NULL = 0, or [batch] */
    const int32_t *draft; int64_t draft_pitch;   /* as in npm_verify */
    const int32_t *n_draft;                      /* NULL (rows == 1), or [batch]; below 0 = inactive */
    const int32_t *active;                       /* NULL = all, or [batch]: 0 = leave the slot alone */
    const float *repetition, *presence, *frequency;  /* [batch] each, or NULL */
    const int32_t *eos, *min_new;                /* [batch] each, or NULL */
    const int32_t *bias_index; const float *bias_value;  /* [batch, bias_cap] */
    const int32_t *bias_count;                   /* [batch] */
    int32_t bias_cap;                            /* 0 = no list */
    int32_t *workspace;                          /* [batch, vocab], zero before and after */
} npm_logits;
int npm_logits_process(const npm_logits *p);
/* One token behind every slot's history: when (active == NULL or active[b] != 0), ids[b] >= 0 and history_len[b] (clipped at 0) is
 * below history_cap, ids[b] is written to history[b * history_pitch + history_len[b]] and history_len[b] advances -- step 4 of
 * npm_verify_rows for a plain sampling loop.  One thread per slot.  NPM_E_BAD_ARGUMENT: batch < 1, history_cap < 1, history_pitch <
 * history_cap, a NULL history, history_len or ids. */
int npm_history_append(int32_t *history, int64_t history_pitch, int32_t history_cap, int32_t *history_len, const int32_t *ids,
                       const int32_t *active, int32_t batch);
/* What the most recent of the two launched: "logits_process_kernel B=<batch> rows=<rows> V=<vocab> history=<0|1> bias=<bias_cap>"
 * or "history_append_kernel B=<batch> cap=<history_cap>"; "" before the first call. */
const char *npm_last_logits_kernel(void);

/* ---- around the path ("next" rows of SURVEY.md section 8f): keeps a Trainer step on the device ---- */
/* Adam as the reference computes it (optimizer.py:53-67), operation for operation: (1 - beta1) * g and (1 - beta2) * (g * g) are
 * float32 products (the gradient is float32 and the scalars do not widen it), the moments m, v are fp64 (device buffers of n
 * doubles, zero-initialised with npm_fill_f64; beta * moment + term without contraction), bias correction with step >= 1 (step < 1:
 * NPM_E_BAD_ARGUMENT), epsilon inside the sqrt, the subtraction in fp64 and ONE rounding to the float32 parameter.  The moments are
 * the reference's bit for bit; the parameter is, up to ties of the fp64 divide / root.  npm_fill_f64: value 0.0
 * only (anything else NPM_E_UNSUPPORTED). */
int npm_adam_step(float *var, const float *grad, double *m, double *v, size_t n, double lr, double beta1,
                  double beta2, double eps, int step);
int npm_fill_f64(double *dst, double value, size_t n);
/* ---- AdamW with global-norm gradient clipping: a language-model training step with no host round trip ----
 * Three calls: the fp64 sum of squares of the gradients, one thread that turns it into a clip factor in HBM, and an AdamW
 * step that reads the factor from there.  All pointers are device pointers; the npm_ranges struct itself is host memory.
 *
 * npm_sumsq_ranges: *acc += sum over ranges[0 .. count) of (double)x * (double)x.  Every square is exact in fp64 (a product of
 * two float32 has 48 significant bits) and every addition is an fp64 addition: no float atomics, no fp32 accumulator, no fp32
 * square.  Range r is cut into ceil(n[r] / NPM_SUMSQ_TILE) tiles of NPM_SUMSQ_TILE elements (the last one shorter); one block
 * of 256 threads sums one tile in a fixed order into partials[tile] (it finds its range by walking the at most
 * NPM_SUMSQ_MAX_RANGES tile counts, which are the same for the whole block), and a second launch of ONE block adds the partials
 * in index order with a fixed tree and adds the total to *acc.  The result is a function of the ranges (addresses and lengths),
 * their order and NPM_SUMSQ_TILE only: not of the grid, the number of compute units or any tuning knob; a repeated call gives
 * the same bits, and two calls accumulate in stream order.  ptr[r] is 4-byte aligned: a tile loads 16 bytes at a time over its
 * 16-byte aligned interior and peels up to 3 elements in front and behind with 4-byte loads.  Nothing outside the ranges is
 * read.  count == 0 or every n[r] == 0: nothing is launched.  NPM_E_BAD_ARGUMENT: ranges or acc NULL, count outside
 * 0 .. NPM_SUMSQ_MAX_RANGES, a NULL ptr[r] with n[r] > 0, a ptr[r] that is not 4-byte aligned, more than
 * 2^31 - 1 tiles in all. */
#define NPM_SUMSQ_TILE 16384        /* elements per tile: 256 lanes x 64 */
#define NPM_SUMSQ_MAX_RANGES 32
typedef struct npm_ranges {
    const float *ptr[32];
    uint64_t n[32];
    int32_t count;
} npm_ranges;
int npm_sumsq_ranges(const npm_ranges *ranges, double *acc);
/* state = 4 doubles [sumsq, norm, scale, ok].  One thread: norm = sqrt(sumsq); a norm that is not finite gives scale = 0 and
 * ok = 0; otherwise scale = (double)(float)min(1.0, max_norm / (norm + 1e-6)) -- the ratio in fp64, rounded ONCE to float32, so
 * scale is exactly a float -- and ok = 1.  max_norm = +inf gives scale 1: the norm is reported and nothing is clipped.
 * NPM_E_BAD_ARGUMENT: state NULL, max_norm <= 0 or NaN. */
int npm_clip_finish(double *state, double max_norm);
/* AdamW (Loshchilov and Hutter; what torch.optim.AdamW computes) on fp64 moments, every operation rounded on its own (no
 * contraction).  omb1 = 1 - beta1, omb2 = 1 - beta2, c1 = 1 - beta1^step, c2 = 1 - beta2^step and lw = lr * weight_decay are
 * computed on the host in fp64.  clip_state is NULL or the 4 doubles of npm_clip_finish.  Per element:
 *     if clip_state and clip_state[3] == 0: nothing at all is written (var, m, v keep their bits)
 *     g    = clip_state ? (float)clip_state[2] * grad[i] : grad[i]           one fp32 product; exact when scale == 1
 *     G    = (double)g
 *     m'   = beta1 * m + omb1 * G;    v' = beta2 * v + omb2 * (G * G)        fp64
 *     d    = (double)var - lw * (double)var                                  fp64 product, fp64 difference
 *     var' = (float)(d - lr * ((m' / c1) / (sqrt(v' / c2) + eps)))           epsilon OUTSIDE the root; ONE rounding to fp32
 * This is deliberately NOT the arithmetic of npm_adam_step, which stays as it is: that one is the reference's Adam operation
 * for operation (float32 gradient products, epsilon INSIDE the root, no decay), this one is the update other frameworks
 * compute -- hyper-parameters ported from them (epsilon 1e-8, weight decay 0.01 .. 0.1) assume the outside epsilon and the
 * decoupled decay, and an epsilon inside the root is a different regulariser by orders of magnitude (sqrt(1e-8) = 1e-4).
 * The same grid-stride launch as npm_adam_step, a kernel of its own.  n == 0: nothing is launched.
 * NPM_E_BAD_ARGUMENT: step < 1, weight_decay < 0 or NaN, a NULL var, grad, m or v with n > 0. */
int npm_adamw_step(float *var, const float *grad, double *m, double *v, size_t n, double lr, double beta1, double beta2,
                   double eps, int step, double weight_decay, const double *clip_state);
/* ---- gradient accumulation over micro-batches (csrc/npm_accum.hip) ----
 * npm_accumulate_ranges: dst[r][i] = dst[r][i] + src[r][i] for every range r and element i -- ONE float32 addition and nothing else;
 * an inf or a NaN stays in its own element.  src is not written.  The two tables are host memory, their pointers device pointers.
 * The grid is the tiling of npm_sumsq_ranges laid over the dst ranges: range r is ceil(n[r] / NPM_SUMSQ_TILE) tiles, one block of
 * 256 threads a tile, found by the same scalar walk of the tile counts.  Inside a tile the elements follow dst's alignment as they
 * do there: up to 3 head elements on lanes 0 .. 2, aligned groups of four with group q on lane q % 256 in ascending order, up to
 * 3 tail elements.  dst is read and written 16 bytes at a time over its aligned interior; src is read 16 bytes at a time where it
 * has dst's 16-byte phase and with four 4-byte loads where it has not -- the same bits either way.
 * sumsq_acc == NULL: one launch, no reduction.  sumsq_acc != NULL: the same launch also squares every NEW dst value exactly in
 * fp64, adds the squares per lane in the order above, reduces with the fixed 256-lane tree into one partial per tile; a second
 * launch of one block adds the partials in index order with the same tree, and *sumsq_acc = *sumsq_acc + total.
 * CONTRACT: after the call *sumsq_acc holds the bits that npm_sumsq_ranges(dst, sumsq_acc) would have produced on the updated
 * buffers from the same starting value -- the pass over the gradients that the norm costs disappears into the last fold.
 * count == 0 or every n[r] == 0: nothing is launched.  NPM_E_BAD_ARGUMENT, with nothing written: dst or src NULL, count outside
 * 0 .. NPM_SUMSQ_MAX_RANGES, dst->count != src->count, dst->n[r] != src->n[r], a NULL pointer with n[r] > 0, a pointer that is not
 * 4-byte aligned, a dst range that overlaps another dst range or any src range, more than 2^31 - 1 tiles in all. */
int npm_accumulate_ranges(const npm_ranges *dst, const npm_ranges *src, double *sumsq_acc);
/* npm_clip_finish for gradients that are still to be multiplied by grad_scale (1 / micro-batches, 1 / counted tokens): the norm
 * reported and clipped is the norm of the SCALED gradient, and the factor npm_adamw_step multiplies with carries the scale.
 * state = 4 doubles [sumsq, norm, scale, ok], sumsq over the unscaled gradients.  One thread, every operation rounded on its own:
 *     norm = grad_scale * sqrt(sumsq);  state[1] = norm
 *     norm not finite:  state[2] = state[3] = 0
 *     otherwise:        ratio = max_norm / (norm + 1e-6);  c = ratio < 1 ? ratio : 1
 *                       state[2] = (double)(float)(grad_scale * c);  state[3] = 1
 * max_norm = +inf: no clipping, the factor is (float)grad_scale.  grad_scale == 1.0: the four doubles of npm_clip_finish, bit
 * for bit.  NPM_E_BAD_ARGUMENT: state NULL, max_norm <= 0 or NaN, grad_scale <= 0, NaN or inf. */
int npm_clip_finish_scaled(double *state, double max_norm, double grad_scale);
/* MSELoss (loss.py:21-29): loss = sum((y-t)^2)/n (fp64 accumulation, returned to the host); dy = 2 (y-t) / n */
int npm_mse_fwd(const float *y, const float *targets, size_t n, double *loss);
int npm_mse_bwd(const float *y, const float *targets, float *dy, size_t n);
/* CrossEntropyLoss (loss.py:33-39): loss = -sum(t log y); dy = -t / y */
int npm_xent_fwd(const float *y, const float *targets, size_t n, double *loss);
int npm_xent_bwd(const float *y, const float *targets, float *dy, size_t n);
/* ---- softmax cross-entropy from logits and token ids: what training a language model needs ----
 * npm_softmax_xent_rows replaces CrossEntropyLoss (loss.py:33-39) composed with Softmax (activations.py:26-45) over a dense
 * one-hot [rows, vocab] float tensor -- five passes over [rows, vocab] and log(0) = -inf for an underflowed probability -- by one
 * launch that reads every logit once and, with a gradient, writes every gradient once.  logits: fp32 [rows, vocab], row r at
 * logits + r * ld; targets: int32 [rows]; dlogits: NULL (no gradient) or fp32 [rows, vocab] with the pitch ldd; row_loss, row_lse:
 * fp32 [rows], row_lse may be NULL; all of these device pointers.  loss_sum: HOST pointer.  e = smoothing in [0, 1), V = vocab.
 * Per row r with t = targets[r]:
 *  1. t < 0: the row is ignored (the padding convention of npm_take_rows): its logits are NOT READ, row_loss = 0, the gradient
 *     row is all zeros, row_lse is NaN.
 *  2. t >= V: row_loss, row_lse and the whole gradient row are NaN; nothing outside the row is touched.
 *  3. Otherwise, with m = max_j z_j, s = sum_j exp(z_j - m), lse = m + log(s):
 *       row_lse  = lse
 *       row_loss = lse - (1 - e) z_t - (e / V) sum_j z_j           (the last term only when e != 0)
 *       dlogits[r, j] = grad_scale * (exp(z_j - lse) - (1 - e) [j == t] - e / V)
 *  4. A -inf logit is a masked token: it adds 0 to s and its gradient is 0, the target included.  With e != 0 a -inf logit makes
 *     row_loss +inf, as the formula says; a -inf target logit makes it +inf for every e.
 *  5. A row that holds a NaN or +inf, or whose every logit is -inf, gives NaN row_loss, row_lse and gradient row; it never faults.
 *  6. dlogits may be exactly logits with ldd == ld: the gradient then overwrites the logits.  Any other overlap of the two
 *     [rows, vocab] extents is NPM_E_BAD_ARGUMENT.
 *  7. *loss_sum = the fp64 sum of row_loss[0 .. rows) in a fixed order (a second launch of one block, no atomics; one 8-byte copy
 *     to the host, as npm_mse_fwd).  rows == 0 is legal: *loss_sum = 0 and nothing is launched.
 *  8. Every reduction has a fixed thread-to-token mapping and a fixed tree, the same on the 16-byte and the scalar path: a launch is
 *     bitwise reproducible, and a row's results depend neither on rows, on the row's position, on the pitches nor on the alignment.
 * Instances, by vocab alone: "xent_wave" (V <= 1024: one wavefront per row), "xent_block256" (V <= 8192) and "xent_block1024"
 * (V <= 32768 = NPM_SAMPLE_LDS_ROW): one block per row; these three read the row once and keep it in registers;
 * "xent_block1024_global" (larger: the second and third pass re-read the row).  16-byte loads and stores when logits (and dlogits) are 16-byte
 * aligned with ld % 4 == 0 (ldd % 4 == 0), else 4-byte ones.  A [rows, vocab] of at least 32 MB moves with the nontemporal hint
 * (NPM_TUNE_STREAM_NT): the gradient stores and every load that is the last use of a logit.
 * Arithmetic: m exact; z_j - m and expf in fp32; s and sum_j z_j accumulated in fp64, the target's own term joining s after the
 * tree, so that the target's gradient is grad_scale * (float)(e (1 - 1 / V) - s_excl / s) in fp64 -- a quotient of sums, accurate
 * relative to 1 - p_t however close p_t is to 1; lse and row_loss in fp64 with fp64 log, ONE rounding to fp32 each; the other
 * gradients are grad_scale * (expf(z_j - m) * (float)(1 / s) - (float)(e / V)), each operation rounded to fp32, no contraction
 * (the same expf value that entered s: the register instances keep it, the re-reading one computes it again).
 * Error bound against exact arithmetic on the same fp32 inputs, for a row of clause 3 with finite results.  u = 2^-24; expf is
 * within 1 ulp <= 2 u (the documented accuracy of the device library's expf), the fp64 log within 2^-52; d_j = m - z_j;
 * p_j = exp(z_j - lse); A = sum_j p_j d_j (the mean distance below the maximum under the row's own distribution; A <= ln V):
 *   - a term of s: u d_j from the subtraction, 2 u from expf, so |ds| / s <= (A + 2) u to first order, 1.01 covering the rest;
 *   - the fp64 sums run through chains of at most 32 + V / 1024 tokens per thread, then the log2(64) = 6 butterfly levels of a
 *     wavefront, the at most 16 wave partials in order and the target's term, 23 more additions: gamma = (55 + V / 1024) 2^-53
 *     relative to the sum of magnitudes -- the summation term; it is below u / 512 for every legal V;
 *   |row_lse  - lse|  <= u (|lse|  + 1.01 (A + 2)) + gamma (1 + |m|)
 *   |row_loss - loss| <= u (|loss| + 1.01 (A + 2)) + gamma (1 + |m| + |z_t| + e mean_j |z_j|)
 *   |dlogits[r, j] - g_j| <= 1.01 u |grad_scale| (q_j + e / V + 2 |g_j / grad_scale|) + 2^-125 |grad_scale|
 *     j != t: q_j = p_j (d_j + 1.01 A + 6.1)       (subtraction, expf, s, the rounding of 1 / s, the product: then the
 *                                                   subtraction of e / V and the scaling round once each)
 *     j == t: q_t = (A - p_t d_t) + 2 (1 - p_t) + 1.01 (1 - p_t) (A + 2)        (the error of s_excl and of s in s_excl / s)
 *   2^-125: a probability below the smallest normal number may be flushed to zero.
 * tests/test_gpu_xent.py asserts these three bounds on every case of tests/xent_cases.py; DESIGN.md 4.5k records the worst
 * observed fraction of each.
 * NPM_E_BAD_ARGUMENT before anything is launched: loss_sum == NULL, rows outside 0 .. 2^31 - 1, vocab outside 1 .. 2^30,
 * ld < vocab, smoothing outside [0, 1), and for rows > 0 a NULL logits, targets or row_loss, dlogits with ldd < vocab, dlogits ==
 * logits with ldd != ld, a partial overlap. */
int npm_softmax_xent_rows(const float *logits, int64_t ld, const int32_t *targets, int64_t rows, int64_t vocab, float smoothing,
                          float grad_scale, float *dlogits, int64_t ldd, float *row_loss, float *row_lse, double *loss_sum);
/* What the most recent npm_softmax_xent_rows launched: "<instance> V=<vocab> grad=<0|1> inplace=<0|1> vec=<0|1> nt=<0|1>" with the
 * instance names above, "xent_none rows=0" for an empty call; "" before the first call. */
const char *npm_last_xent_kernel(void);
/* DropOut (normalizations.py:14-30): y = mask ? x / keep_prob : 0 with a host-drawn byte mask */
int npm_mask_scale(const float *x, const unsigned char *mask, float *y, size_t n, float keep_prob);
/* The same with the mask drawn ON THE DEVICE: element i keeps its value when word (i & 3) of
 * Philox4x32-10(counter = (i / 4, offset), key = seed) is below keep_prob * 2^32; the byte mask is written too (the layer's
 * `_mask` stays readable).  Deterministic in (seed, offset); not the host generator's stream -- seeded parity with the
 * reference needs the host-drawn path above.  x == y == NULL: only the mask is drawn (its consumer applies it:
 * npm_layernorm_dropout_fwd / _bwd). */
int npm_dropout_philox(const float *x, float *y, unsigned char *mask, size_t n, float keep_prob, uint64_t seed, uint64_t offset);

#ifdef __cplusplus
}
#endif
#endif /* NPM_HIP_H */
