// Skinny-M GEMM for decode steps (include/npm_hip.h: npm_sgemm_skinny): C[M, N] = epilogue(alpha A[M, K] op(B)) for 1 <= M <= 64 in
// exact fp32, un-batched.  op(B) is a weight matrix that is read ONCE: B [N, K] (NT: wq / wk / wv / wo and the packed q/k/v
// projection) or B [K, N] (NN: Dense / Linear).  At these M the product is a stream over the weights (56 MB per decoder layer at
// d 1024 / hidden 4096 against at most 1 MB of activations), so the kernel is shaped around that stream, as mha_decode_kernel
// (npm_decode.hip) is shaped around K / V:
//   * every weight element is loaded once, by one wave, with a 16-byte load straight into VGPRs (no LDS round trip), a step of
//     32 k ahead of the MFMAs that use it;
//   * a block owns a strip of 64 columns and a range of K; its four waves take consecutive quarters of that range and merge
//     their accumulators through LDS in wave order; the K ranges of a column strip (gridDim.y SPLITS) leave [M, 64] partial sums
//     in pooled scratch and sgemm_skinny_combine_kernel adds them in a fixed order: no atomics, bitwise reproducible.  The
//     epilogue runs where the final sum is formed (the block itself when there is one split);
//   * the activation fragment of 16 k (16 bytes per lane and 16-row block, L2-resident) is loaded once per wave and K chunk and
//     reused in registers over the FOUR 16-column tiles of the wave's strip, so A costs RB / 4 of the weight traffic in L2
//     requests and nothing in LDS (DESIGN.md 4.1b has the choice against staging A in LDS).
//
// MFMA orientation (v_mfma_f32_16x16x4_f32: lane l supplies A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; register w
// of the result is row m = 4 (l >> 4) + w, column n = l & 15).  The OUTPUT ROW is on the lane (the MFMA's B operand is the
// activation, its A operand the weights), so rows >= M are whole lanes whose results are never stored.  With c = l & 15, g = l >> 4
// and a K chunk of 16 starting at k0:
//   activation   lane (r = c, g) loads A[r][k0 + 4 g .. + 3] (16 bytes); component i is the B operand of step i
//   NT           tile t: lane loads B[n0 + 16 t + c][k0 + 4 g .. + 3]; step e contracts k = {k0 + 4 g' + e} (the permuted
//                contraction index of the decode kernel's K operand); register w of tile t is column n0 + 16 t + 4 g + w
//   NN           lane loads B[k0 + 4 g + w][n0 + 4 c .. + 3] for w = 0 .. 3 (16 lanes cover 256 contiguous bytes of one k row: the
//                decode kernel's V operand); step w contracts k = {k0 + 4 g' + w}; component e of the load feeds output block e
//                whose register w' is column n0 + 16 g + 4 w' + e
// Either way a lane ends with four consecutive columns of one row per 16-byte store.
//
// The order in which the k terms of an output element are added is a function of (K, the split count) alone: chunk after chunk
// inside a wave, waves 0 .. 3, then the splits in the combine kernel's fixed tree.  The row-block count RB only says how many
// lanes' worth of rows ride along, so row r of an M-row call is bitwise the M = 1 call on that row.  Nothing outside the operands is read: rows >= M of A are zeros by
// selection (their loads are redirected to row 0), rows >= N of an NT B and columns >= N of an NN B are redirected to valid ones
// and their results never stored, and a K chunk past a wave's range is neither loaded past K nor multiplied.
// Floating-point contraction is off in these kernels: each fma is written out.
//
// Half-precision weights (npm_sgemm_skinny_w16): the same kernel template with WT = _Float16.  B holds IEEE halves (ldb counts
// halves); a lane loads the SAME four elements as the float instance -- 8 bytes instead of 16 -- and converts them exactly
// (v_cvt_f32_f16) when the step is consumed, so the MFMA operands, the chunk order and every sum are those of the float instance on
// the rounded weights: the result is bitwise npm_sgemm_skinny's on a B of rounded floats, and every identity above carries over.
// Halving the load width halves the bytes in flight per wave, which is what cost the fp16 KV cache its 2x.  Loading
// FOUR chunks per step instead of two (the same bytes in flight, twice the load instructions) was built and measured: it is the
// slower one, because a wave of these products has two to four chunks in all and a step of four leaves nothing to overlap
// (DESIGN.md 4.1c has the numbers), so the halves instance keeps the float instance's step.  A 16-byte load of halves would need
// another lane-to-k mapping (8 k per lane in NT) or 128-column strips (8 columns per lane in NN); it was not built.
#include <algorithm>
#include <cstring>

#include "npm_internal.h"

namespace {

constexpr int WAVES = 4;          // per block
constexpr int STRIP = 64;         // columns per block
constexpr int CHUNK = 16;         // k per MFMA group
constexpr int STEP = 2;           // chunks loaded together, one step ahead
constexpr int AUTO_MAX_SPLITS = 16;   // the automatic rule's ceiling (NPM_TUNE_SKINNY_SPLITS may force up to NPM_SKINNY_MAX_SPLITS)

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

int g_splits = 0;                 // NPM_TUNE_SKINNY_SPLITS: 0 automatic, n > 0 forced
int g_nt = 0;                     // NPM_TUNE_SKINNY_NT: 0 by size (npm::stream_nt_enabled of the weight bytes), 1 always, 2 never
char g_last[112] = "";

struct SkinnyArgs {
    const float *a, *b;
    long lda, ldb;
    float *c;
    long ldc;
    const float *bias, *residual;
    long ldr;
    float *aux;
    long ldaux;
    float *part;                  // splits > 1: [splits, m, n]
    float alpha;
    int m, n, chunks;             // chunks = k / 16
    int per_split, per_wave;      // chunks per split and per wave of a split
    int relu;
};

template <bool NT>
__device__ __forceinline__ f32x4v ld_w(const float *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(p));
    return *reinterpret_cast<const f32x4v *>(p);
}

// The same four elements of a weight matrix stored as halves (npm_sgemm_skinny_w16): one 8-byte load, kept as loaded until use
template <bool NT>
__device__ __forceinline__ f16x4v ld_w(const _Float16 *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f16x4v *>(p));
    return *reinterpret_cast<const f16x4v *>(p);
}

// four weights as the MFMA takes them: as they are, or converted exactly (v_cvt_f32_f16; subnormals are kept)
__device__ __forceinline__ f32x4v widen(f32x4v w) { return w; }
__device__ __forceinline__ f32x4v widen(f16x4v w) { return __builtin_convertvector(w, f32x4v); }

// alpha, bias, residual (may alias C: read before the store of the same thread), saved pre-activation, ReLU -- npm_sgemm's order
__device__ __forceinline__ void epilogue_store(const SkinnyArgs &a, f32x4v v, int row, int col) {
#pragma clang fp contract(off)
    v = v * a.alpha;
    if (a.bias) v = v + *reinterpret_cast<const f32x4v *>(a.bias + col);
    if (a.residual) v = v + *reinterpret_cast<const f32x4v *>(a.residual + (long)row * a.ldr + col);
    if (a.aux) *reinterpret_cast<f32x4v *>(a.aux + (long)row * a.ldaux + col) = v;
    if (a.relu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.f);
    }
    *reinterpret_cast<f32x4v *>(a.c + (long)row * a.ldc + col) = v;
}

// RB: 16-row blocks (M <= 16 RB); TB: B is [N, K] (NT layout); NT: nontemporal weight loads; WT: a.b holds floats, or halves
// (behind the float pointer; ldb then counts halves) that are converted exactly on their way into the MFMAs -- the lane-to-k
// mapping, the chunk order and every sum are those of the float instance, so the result is bitwise the float instance's on the
// rounded weights
template <int RB, bool TB, bool NT, typename WT = float>
__global__ void __launch_bounds__(WAVES * 64, 2)
sgemm_skinny_kernel(const SkinnyArgs a) {
#pragma clang fp contract(off)
    typedef WT wvec __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) float s_acc[WAVES][16][STRIP + 4];

    const int n0 = blockIdx.x * STRIP, split = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;

    // this wave's chunks [q_begin, q_end): a quarter of the split's range, wave-uniform
    const int s_begin = split * a.per_split;
    const int s_end = min(s_begin + a.per_split, a.chunks);
    const int q_begin = min(s_begin + wave * a.per_wave, s_end);
    const int q_end = min(q_begin + a.per_wave, s_end);

    const float *ap[RB];
    bool live[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = rb * 16 + c;
        live[rb] = r < a.m;
        ap[rb] = a.a + (long)(live[rb] ? r : 0) * a.lda + 4 * g;
    }
    // TB: bp[t] is row n0 + 16 t + c of B (a tile at or past N: row N - 1, never stored); else bp[0] is column n0 + 4 c of k row
    // 4 g (a column at or past N: column 0, never stored)
    const WT *const b = reinterpret_cast<const WT *>(a.b);
    const WT *bp[4];
    if (TB) {
#pragma unroll
        for (int t = 0; t < 4; ++t) bp[t] = b + (long)min(n0 + 16 * t + c, a.n - 1) * a.ldb + 4 * g;
    } else {
        const int col = n0 + 4 * c;
        bp[0] = b + (col < a.n ? col : 0) + (long)(4 * g) * a.ldb;
    }

    f32x4v acc[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[rb][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

    wvec wr[STEP][4];
    f32x4v ar[STEP][RB];
    // chunk q + j of a step (clamped to the last chunk of K: the odd chunk behind a wave's range is loaded in bounds, never used)
    auto load_step = [&](int q, wvec (&w)[STEP][4], f32x4v (&x)[STEP][RB]) {
#pragma unroll
        for (int j = 0; j < STEP; ++j) {
            const long k0 = (long)CHUNK * min(q + j, a.chunks - 1);
#pragma unroll
            for (int t = 0; t < 4; ++t) w[j][t] = TB ? ld_w<NT>(bp[t] + k0) : ld_w<NT>(bp[0] + (k0 + t) * a.ldb);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) x[j][rb] = *reinterpret_cast<const f32x4v *>(ap[rb] + k0);
        }
    };

    if (q_begin < q_end) load_step(q_begin, wr, ar);
    for (int q = q_begin; q < q_end; q += STEP) {
        f32x4v wc[STEP][4], xc[STEP][RB];
#pragma unroll
        for (int j = 0; j < STEP; ++j) {
#pragma unroll
            for (int t = 0; t < 4; ++t) wc[j][t] = widen(wr[j][t]);
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) xc[j][rb] = live[rb] ? ar[j][rb] : f32x4v{0.f, 0.f, 0.f, 0.f};
        }
        if (q + STEP < q_end) load_step(q + STEP, wr, ar);
#pragma unroll
        for (int j = 0; j < STEP; ++j) {
            if (q + j < q_end) {                  // wave-uniform
                // the outer index is the contraction step, the inner ones run over 4 RB independent accumulators
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int rb = 0; rb < RB; ++rb) {
                            if (TB) acc[rb][t] = MFMA16(wc[j][t][i], xc[j][rb][i], acc[rb][t]);     // step e = i of tile t
                            else acc[rb][t] = MFMA16(wc[j][i][t], xc[j][rb][i], acc[rb][t]);        // step w = i of block e = t
                        }
            }
        }
    }

    // merge the four waves in wave order, one row block at a time; then the epilogue (one split) or this split's partial sums
    const int row = threadIdx.x >> 4, col4 = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        if (rb) __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int w = 0; w < 4; ++w) s_acc[wave][c][TB ? 16 * t + 4 * g + w : 16 * g + 4 * w + t] = acc[rb][t][w];
        __syncthreads();
        f32x4v o = *reinterpret_cast<const f32x4v *>(&s_acc[0][row][col4]);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) o = o + *reinterpret_cast<const f32x4v *>(&s_acc[w][row][col4]);
        const int r = rb * 16 + row, col = n0 + col4;
        if (r < a.m && col < a.n) {
            if (a.part) *reinterpret_cast<f32x4v *>(a.part + ((long)split * a.m + r) * a.n + col) = o;
            else epilogue_store(a, o, r, col);
        }
    }
}

// COMBINE_LANES consecutive lanes per (row, four columns): lane j adds the partial sums of splits j, j + 8, j + 16, ... in that
// order, then the eight lane sums are added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) by three exchanges (both partners of an
// exchange form the same commutative sum, so every lane ends with the same bits); lane 0 runs the epilogue.  A lane without a
// split adds 0.  The order is a function of the split count alone.
constexpr int COMBINE_LANES = 8;

__global__ void __launch_bounds__(256)
sgemm_skinny_combine_kernel(const SkinnyArgs a, int splits) {
#pragma clang fp contract(off)
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = tid / COMBINE_LANES, j = tid % COMBINE_LANES;
    const int n4 = a.n / 4;
    const bool valid = i < a.m * n4;                  // whole groups of eight lanes: the exchanges below never leave a group
    const int r = valid ? i / n4 : 0, col = valid ? (i % n4) * 4 : 0;
    const float *p = a.part + (long)r * a.n + col;
    const long plane = (long)a.m * a.n;
    f32x4v o{0.f, 0.f, 0.f, 0.f};
    for (int s = j; s < splits; s += COMBINE_LANES) o = o + *reinterpret_cast<const f32x4v *>(p + s * plane);
#pragma unroll
    for (int step = 1; step < COMBINE_LANES; step *= 2)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = o[e] + __shfl_xor(o[e], step);
    if (valid && j == 0) epilogue_store(a, o, r, col);
}

template <int RB, bool TB, typename WT>
void launch_nt(const SkinnyArgs &a, dim3 grid, bool nt, hipStream_t s) {
    if (nt) hipLaunchKernelGGL((sgemm_skinny_kernel<RB, TB, true, WT>), grid, dim3(WAVES * 64), 0, s, a);
    else hipLaunchKernelGGL((sgemm_skinny_kernel<RB, TB, false, WT>), grid, dim3(WAVES * 64), 0, s, a);
}

template <bool TB, typename WT>
void launch_rb(const SkinnyArgs &a, dim3 grid, int rb, bool nt, hipStream_t s) {
    switch (rb) {
        case 1: launch_nt<1, TB, WT>(a, grid, nt, s); break;
        case 2: launch_nt<2, TB, WT>(a, grid, nt, s); break;
        case 3: launch_nt<3, TB, WT>(a, grid, nt, s); break;
        default: launch_nt<4, TB, WT>(a, grid, nt, s); break;
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

const int EPI_OK = NPM_EPI_BIAS | NPM_EPI_RESIDUAL | NPM_EPI_RELU | NPM_EPI_RELU_SAVE;

// w16: g->b points at halves (npm_sgemm_skinny_w16): ldb counts halves and a 16-byte row start takes a multiple of 8 of them
bool supported(const npm_gemm *g, bool w16 = false) {
    if (g == nullptr) return false;
    if (g->trans_a != 0 || (g->trans_b != 0 && g->trans_b != 1)) return false;
    if (g->batch0 != 1 || g->batch1 != 1) return false;
    if (g->m < 1 || g->m > NPM_SKINNY_MAX_M) return false;
    if (g->n < 16 || g->n % 16 || g->k < 16 || g->k % 16) return false;
    if (g->a == nullptr || g->b == nullptr || g->c == nullptr) return false;
    if (!aligned16(g->a) || !aligned16(g->b) || !aligned16(g->c)) return false;
    if (g->lda % 4 || g->ldb % (w16 ? 8 : 4) || g->ldc % 4) return false;
    if (g->lda < g->k || g->ldb < (g->trans_b ? g->k : g->n) || g->ldc < g->n) return false;
    if (g->epilogue & ~EPI_OK) return false;
    if ((g->epilogue & NPM_EPI_RELU) && (g->epilogue & NPM_EPI_RELU_SAVE)) return false;
    if ((g->epilogue & NPM_EPI_BIAS) && (g->bias == nullptr || !aligned16(g->bias))) return false;
    if ((g->epilogue & NPM_EPI_RESIDUAL) && (g->residual == nullptr || !aligned16(g->residual) || g->ldr % 4 || g->ldr < g->n))
        return false;
    if ((g->epilogue & NPM_EPI_RELU_SAVE) && (g->aux == nullptr || !aligned16(g->aux) || g->ldaux % 4 || g->ldaux < g->n))
        return false;
    if (g->colsum || g->bsum || g->asum || g->rowdot || g->split_k != 0) return false;
    return true;
}

}  // namespace

extern "C" int npm_skinny_set_splits(int value) {
    if (value < 0 || value > NPM_SKINNY_MAX_SPLITS)
        return npm::fail(NPM_E_BAD_ARGUMENT, "npm_set_tuning: NPM_TUNE_SKINNY_SPLITS takes 0 .. %d", NPM_SKINNY_MAX_SPLITS);
    g_splits = value;
    return NPM_OK;
}

extern "C" int npm_skinny_set_nt(int value) {
    if (value < 0 || value > 2) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_set_tuning: NPM_TUNE_SKINNY_NT takes 0, 1 or 2");
    g_nt = value;
    return NPM_OK;
}

extern "C" int npm_sgemm_skinny_supported(const npm_gemm *g) { return supported(g) ? 1 : 0; }

extern "C" int npm_sgemm_skinny_splits(int n, int k, int trans_b) {
    if (n < 1 || k < 1) return 1;
    if (g_splits > 0) return g_splits;
    // Fill the chip: about two blocks per compute unit of the 256 over the 64-column strips, but never fewer than 128 k (two
    // 16-k chunks per wave) per split and never more than 16 splits -- beyond either the partial sums and their combine cost
    // more than the idle units (tools/skinny_gemm_bench.py; DESIGN.md 4.1b has the sweep).  Shape arguments only: both layouts
    // split alike (trans_b is part of the signature so that a rule may tell them apart).
    (void)trans_b;
    const long strips = (n + STRIP - 1) / STRIP;
    const long want = (512 + strips - 1) / strips;
    const long by_k = std::max<long>(1, k / 128);
    return (int)std::max<long>(1, std::min<long>(std::min(want, by_k), AUTO_MAX_SPLITS));
}

extern "C" const char *npm_last_skinny_kernel(void) { return g_last; }

namespace {

// npm_sgemm_skinny and npm_sgemm_skinny_w16 behind their argument checks: WT is what g->b points at
template <typename WT>
int run(const npm_gemm *g) {
    const int splits = npm_sgemm_skinny_splits(g->n, g->k, g->trans_b);
    const int rb = (g->m + 15) / 16;
    SkinnyArgs a{};
    a.a = g->a; a.b = g->b; a.lda = g->lda; a.ldb = g->ldb;
    a.c = g->c; a.ldc = g->ldc;
    a.bias = (g->epilogue & NPM_EPI_BIAS) ? g->bias : nullptr;
    a.residual = (g->epilogue & NPM_EPI_RESIDUAL) ? g->residual : nullptr;
    a.ldr = g->ldr;
    a.aux = (g->epilogue & NPM_EPI_RELU_SAVE) ? g->aux : nullptr;
    a.ldaux = g->ldaux;
    a.relu = (g->epilogue & (NPM_EPI_RELU | NPM_EPI_RELU_SAVE)) != 0;
    a.alpha = g->alpha;
    a.m = g->m; a.n = g->n; a.chunks = g->k / CHUNK;
    a.per_split = (a.chunks + splits - 1) / splits;
    a.per_wave = (a.per_split + WAVES - 1) / WAVES;

    hipStream_t s = npm::ctx().stream;
    npm::Scratch part;
    if (splits > 1) {
        if (int rc = part.alloc(sizeof(float) * (size_t)splits * g->m * g->n)) return rc;
        a.part = static_cast<float *>(part.ptr);
    }
    // Each weight byte is read once by one wave: the project's rule for streaming tensors (NPM_TUNE_STREAM_NT, 32 MB) on the
    // weight bytes as stored, NPM_TUNE_SKINNY_NT to force either way.
    const bool nt = g_nt == 1 || (g_nt == 0 && npm::stream_nt_enabled(sizeof(WT) * (size_t)g->n * g->k));
    const dim3 grid((g->n + STRIP - 1) / STRIP, splits);
    if (g->trans_b) launch_rb<true, WT>(a, grid, rb, nt, s);
    else launch_rb<false, WT>(a, grid, rb, nt, s);
    NPM_CHECK_LAUNCH();
    if (splits > 1) {
        const int total = g->m * (g->n / 4) * COMBINE_LANES;
        hipLaunchKernelGGL(sgemm_skinny_combine_kernel, dim3((total + 255) / 256), dim3(256), 0, s, a, splits);
        NPM_CHECK_LAUNCH();
    }
    snprintf(g_last, sizeof g_last, "sgemm_skinny_kernel %s M=%d N=%d K=%d rb=%d splits=%d nt=%d%s", g->trans_b ? "NT" : "NN", g->m,
             g->n, g->k, rb, splits, nt ? 1 : 0, sizeof(WT) == 2 ? " w=f16" : "");
    return NPM_OK;
}

}  // namespace

extern "C" int npm_sgemm_skinny(const npm_gemm *g) {
    NPM_REQUIRE_INIT();
    NPM_ARG(g != nullptr);
    if (!supported(g))
        return npm::fail(NPM_E_UNSUPPORTED, "npm_sgemm_skinny: not supported (trans_a = 0, no batch, 1 <= m <= %d, n and k multiples "
                         "of 16, 16-byte aligned operands, pitches multiples of 4 floats and at least the widths, epilogue of "
                         "bias / residual / ReLU / saved ReLU only, no colsum / bsum / asum / rowdot / split_k)", NPM_SKINNY_MAX_M);
    return run<float>(g);
}

extern "C" int npm_sgemm_skinny_w16_supported(const npm_gemm *g) { return supported(g, true) ? 1 : 0; }

extern "C" int npm_sgemm_skinny_w16(const npm_gemm *g) {
    NPM_REQUIRE_INIT();
    NPM_ARG(g != nullptr);
    if (!supported(g, true))
        return npm::fail(NPM_E_UNSUPPORTED, "npm_sgemm_skinny_w16: not supported (what npm_sgemm_skinny takes, with b pointing at "
                         "halves: ldb a multiple of 8 halves and at least the width, b 16-byte aligned; 1 <= m <= %d)", NPM_SKINNY_MAX_M);
    return run<_Float16>(g);
}
