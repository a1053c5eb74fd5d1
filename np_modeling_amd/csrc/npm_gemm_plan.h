// The launch plans of the GEMM (npm_gemm.hip) and of the Conv2D entry points (npm_conv.hip): which kernel instance a call takes,
// its tiling, split-K and what the epilogue does, as pure functions of explicit inputs.  Plain C++17, no HIP, no globals and no
// pointer dereferenced: a host program can include it (tests/test_gemm_plan_host.py pins the tables below).
//
// ---- GEMM: gemm_plan ---------------------------------------------------------------------------------------------------------
//   a_kmaj, b_kmaj  A stored [M, K] (trans_a == 0), B stored [N, K] (trans_b != 0); NN, NT and TN are the three layouts
//   vec       both bases 16-byte aligned, lda, ldb and the four operand batch strides % 4 == 0, and the contiguous extent of
//             each operand % 4 == 0 (K where it is K-major, else M resp. N)
//   wide      NPM_TUNE_GEMM_WIDE_TILE 1, or 2 and a_kmaj, or 3 and NT; pipeline knob 2, vec, k % 16 == 0, n % 256 == 0, no colsum /
//             bsum / asum, 256 * ldb * 4 < 2^30.  Tile 128 x 256 instead of 128 x 128
//   buf_ok    NPM_TUNE_GEMM_BUF_EPILOGUE on and (256 * ld + n) * 4 < 2^31 for ldc, n, and ldr / ldaux where the epilogue reads them
//   linear    no RELU_SAVE / RELU_MASK / RELU / SOFTMAX_BWD / ROWDOT in the epilogue
//   splits    split_k > 1: that many.  split_k == 0, linear, tiles_m * tiles_n * batch < 2 * CUs and ceil(k / 32) >= 16:
//             pick_splits with 4 / 3 / 2 resident blocks for math 0 / 1 / 2 and 3, and its several-generations rule when
//             math == 0, NPM_TUNE_GEMM_SPLIT_GENS is on, asum is wanted and tiles_m > tiles_n.  Otherwise 1.
//             A non-linear epilogue forces 1, so does colsum.  Then split_ranges over ceil(k / 32) K tiles of 32
//             (k == 0: one split, k_per_split 32).
//   dma       pipeline knob 2, vec, k % 16 == 0 and both operand panels of a block below 2^31 bytes:
//             K-major (tile rows * ld + k) * 4, else (k_per_split * ld + tile rows) * 4
//   dma_path  dma && buf_ok
//   math      NPM_TUNE_GEMM_MATH; 3 (f16x2) counts as 2 wherever the f16x2 kernel does not run
//
//   first row that applies                                     | kernel                           | block | reported math
//   -----------------------------------------------------------+----------------------------------+-------+--------------
//   math == 3, dma_path, batch == 1, !wide, no colsum, k > 0,  | F16X2 (bsum / asum ride in its   | 256   | 3
//     no diagnostics (ablate, trace)                           |   scale passes)                  |       |
//   !dma, !vec                                                 | STAGED_SCALAR                    | 256   | 0
//   !dma, vec, pipeline knob 1                                 | STAGED_VEC_2BUF                  | 256   | 0
//   !dma, vec                                                  | STAGED_VEC                       | 256   | 0
//   bsum / asum wanted, dma_path, TN, k > 0                    | DMA_KSUM (operand 1 B / 2 A,     | 256   | math
//                                                              |   x math 0 / 1 / 2)              |       |
//   wide                                                       | DMA_WIDE                         | 512   | 0
//   colsum wanted, dma_path                                    | DMA_COLSUM                       | 256   | 0
//   math 1 / 2                                                 | DMA_MATH1 / DMA_MATH2            | 256   | math
//   ROWDOT                                                     | DMA_ROWDOT                       | 256   | 0
//   otherwise                                                  | DMA                              | 256   | 0
//
// Quirks, kept:
//   * dma && !buf_ok runs the DMA kernels with the plain epilogue (buf_ok false in the plan); colsum then takes the pass over
//     the stored C and bsum / asum the pass over the operand, as they do on the staged kernels.
//   * the k-sum partial rows are splits * min(blocks sharing the operand tile, 16): tiles_m for bsum, tiles_n for asum.
//   * k_per_split % 16 == 0 always (a multiple of BK = 32), so dma does not test it.
// Refusals, first that applies: the grid (tiles * splits >= 2^31 blocks), WIDE_SPANS (wide && !dma_path), ROWDOT (off its one
// instance: dma_path, NN, !wide, batch == 1, one split, n % 128 == 0, math knob 0, no diagnostics).
//
// ---- Conv2D -----------------------------------------------------------------------------------------------------------------
//   vec   both channel counts % 4 == 0 and the gathered tensors 16-byte aligned;  halo = pad * w + pad, pad = ks / 2
//   buf   NPM_TUNE_CONV_DMA on and (256 * n + n) * 4 < 2^31 (n = output channels); reported only with dma
//   math  NPM_TUNE_GEMM_MATH as the conv kernels count it (0 / 1 / 2); reported, and run, only by the DMA kernels
//
//   conv_gemm_plan (forward: c = c_in, n = c_out; grad_x: c = c_out, n = c_in), K = ks * ks * c, never split
//     dma     knob on, vec, c % 16 == 0, (256 + 2 halo) * c * 4 < 2^30 and K * n * 4 < 2^31
//     tall    dma, n <= 64, n % 16 == 0, knob != 2: 256 x 64 tiles instead of 128 x 128
//     kernel  TALL, DMA (conv_fwd_glds, korder reported), else VEC, else SCALAR (conv_fwd); refused at 2^31 blocks
//   conv_wgrad_plan: M = ks * ks * c_in, N = c_out, K = pixels, K tiles of 32
//     splits  tiles < 2 * CUs and nkt >= 16: NPM_TUNE_CONV_WGRAD_BLOCKS < 0: min(ceil(3 CUs / tiles), nkt / 8); else pick_splits
//             with that value as the pinned blocks per CU and 4 / 3 / 2 resident blocks by math.  Then split_ranges
//     dma     knob on, vec, pixels % 16 == 0, (k_per_split + 2 halo + 16) * c_in * 4 < 2^30 and k_per_split * c_out * 4 < 2^30
//     kernel  DMA (conv_wgrad_glds), else VEC, else SCALAR (conv_wgrad)
//   conv_wgrad_fused_plan (npm_conv2d_bwd_w_relu): K tiles of 16
//     fused   knob on, math 0, NPM_TUNE_CONV_WGRAD_FUSED != 0, both channel counts % 4 == 0, pixels % 16 == 0, w >= 16, all four
//             tensors aligned, M * c_out * 4 < 2^31; and, after the split, the wgrad span limits above and tiles * splits < 2^31.
//             Anything else: the two-pass form (ReLU backward, then conv_wgrad_plan)
//     rows    192 (3 resident blocks) when FUSED == 3, or FUSED != 2 and 192-row tiles pad M less than 128-row ones; else 128 (4)
//     splits  tiles < 2 * CUs and nkt >= 16: pick_splits, pinned by WGRAD_BLOCKS when that is > 0.  Then split_ranges
//     trio    192 rows, exactly 3 tile rows, splits > 1, FUSED != 3: one block of twelve waves per (column tile, split)
//     ksync   K rendezvous every `ksync_every` tiles: !trio, splits > 1, grid <= resident * CUs, ksync_every > 0 and
//             kt_per >= 2 * ksync_every; epochs = (nkt - (splits - 1) * kt_per - 1) / ksync_every
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "npm_hip.h"

namespace npm {

constexpr int BM = 128;
constexpr int BN = 128;
constexpr int BK = 32;
constexpr int GK = 16;                         // K step of the DMA pipeline
static_assert(BK % GK == 0, "a split of whole BK tiles is a split of whole GK tiles");

// Split-K factor for a grid of `tiles` output tiles over `nkt` K tiles.  All blocks of such a launch are
// resident at once (`resident` fit a CU: 4 with the f32 MFMA, 3 / 2 with the split-bf16 modes) and run equally
// long, so the launch lasts as long as the fullest CU: cost(s) = ceil(tiles * s / CUs) / s.  Candidates leave the
// fullest CU with `resident` or `resident - 1` blocks (fewer cannot keep the matrix pipe busy, more would queue a
// second generation).  `force_per_cu` > 0 pins the blocks-per-CU target.
inline int pick_splits(long tiles, int nkt, long cus, int force_per_cu = 0, int resident = 4, int generations = 0) {
    const long max_s = nkt / 8;
    if (force_per_cu > resident) {                       // several generations of `resident` blocks, pinned (experiments)
        const long s = (long)force_per_cu * cus / tiles;
        return (int)(s < 1 ? 1 : s > max_s ? max_s : s);
    }
    int best = 1;
    double best_cost = 1e30;
    // candidates in order of preference: 3 blocks per CU where that many fit (measured on the FFN weight gradients,
    // f32 math: 768 blocks 7.57 ms, 1024 blocks 8.15 ms), then the other neighbour of `resident`
    const int first = resident < 3 ? resident : 3;
    const int second = first == resident ? resident - 1 : resident;
    const int order[2] = {first, second < 2 ? first : second};
    for (int c = 0; c < 2; ++c) {
        const int per_cu = order[c];
        if (force_per_cu > 0 && force_per_cu <= resident && per_cu != force_per_cu) continue;
        long s = per_cu * cus / tiles;
        if (s > max_s) s = max_s;
        if (s < 1) s = 1;
        const double cost = (double)((tiles * s + cus - 1) / cus) / (double)s;
        if (cost < best_cost * (1.0 - 1e-6)) { best_cost = cost; best = (int)s; }
    }
    // Long K ranges (round 4, `generations` > 0): the blocks of one generation stream the same operand panels through their XCD's
    // L2 and drift apart over a thousand K tiles (the packed q/k/v weight gradient, 192 tiles x 4 splits of 1024 K tiles of 32:
    // 6.00 ms; x 16 splits of 256: 5.71 ms).  When the chosen range is longer than 768 K tiles and an exact number of FULL
    // generations (`resident` blocks on every CU, 3 then 2 of them) exists with at least 128 K tiles per block, take that.
    if (generations > 0 && force_per_cu == 0 && nkt / best > 768) {
        for (int gens = 3; gens >= 2; --gens) {
            const long blocks = (long)resident * gens * cus;
            if (blocks % tiles) continue;
            const long s = blocks / tiles;
            if (s <= best || s > max_s || nkt / s < 128) continue;
            return (int)s;
        }
    }
    return best;
}

// `splits` ranges of whole K tiles over `nkt` tiles of `k_tile`: the count clamped to 1 .. nkt, every range ceil(nkt / splits)
// tiles long, and the count lowered until no range is empty.  nkt == 0 (a GEMM with k == 0): one range of one tile.
struct SplitRanges {
    int splits, kt_per, k_per_split;
};
inline SplitRanges split_ranges(int splits, int nkt, int k_tile) {
    splits = std::max(1, std::min(splits, nkt));
    const int kt_per = std::max(1, (nkt + splits - 1) / splits);
    return {nkt > 0 ? (nkt + kt_per - 1) / kt_per : 1, kt_per, kt_per * k_tile};
}

inline int resident_blocks(int math) { return math >= 2 ? 2 : math == 1 ? 3 : 4; }      // of the LDS-DMA kernels, per CU

// ---- GEMM ------------------------------------------------------------------------------------------------------------------------
struct GemmShape {                  // what npm_sgemm reads of its descriptor
    int m, n, k, batch0, batch1;
    int64_t lda, ldb, ldc, ldr, ldaux;
    int64_t stride_a0, stride_a1, stride_b0, stride_b1;
    bool trans_a, trans_b;
    int epilogue;                   // NPM_EPI_*
    bool a_aligned, b_aligned;      // the operands' bases sit on 16 bytes
    int split_k;
    bool colsum, bsum, asum;        // wanted
    bool diagnostics;               // NPM_TUNE_GEMM_ABLATE or a trace buffer is set
};

struct GemmKnobs {                  // NPM_TUNE_GEMM_PIPELINE, _WIDE_TILE, _BUF_EPILOGUE, _MATH, _SPLIT_GENS
    int pipe = 2, wide_tile = 0, buf_epilogue = 1, math = 0, split_gens = 1;
};

enum class GemmKernel { F16X2, STAGED_SCALAR, STAGED_VEC_2BUF, STAGED_VEC, DMA_KSUM, DMA_WIDE, DMA_COLSUM, DMA_MATH1, DMA_MATH2, DMA_ROWDOT, DMA };
enum class GemmRefusal { NONE, GRID, WIDE_SPANS, ROWDOT };

struct GemmPlan {
    GemmRefusal refusal;
    GemmKernel kernel;
    int block;                      // threads
    int64_t grid;                   // blocks: tiles_m * tiles_n * batch * splits
    int tiles_m, tiles_n, splits, k_per_split;
    bool wide, buf_ok;
    int math;                       // NPM_MATH_* the kernel runs: what npm_last_math reports
    int ksum_op;                    // DMA_KSUM: 1 sums B's tiles over k, 2 A's; else 0
    int64_t ksum_rows;              // partial rows the k-sum kernel writes
    bool colsum_fused;              // colsum rides in the epilogue (DMA_COLSUM); else it takes the pass over the stored C
};

inline GemmPlan gemm_plan(const GemmShape &s, const GemmKnobs &kn, int num_cus) {
    GemmPlan p{};
    const bool a_kmaj = !s.trans_a, b_kmaj = s.trans_b;
    const int epi = s.epilogue;
    const bool want_ksum = s.bsum || s.asum;
    bool vec = s.a_aligned && s.b_aligned && s.lda % 4 == 0 && s.ldb % 4 == 0 && s.stride_a0 % 4 == 0 && s.stride_a1 % 4 == 0 &&
               s.stride_b0 % 4 == 0 && s.stride_b1 % 4 == 0;
    vec = vec && (a_kmaj ? s.k : s.m) % 4 == 0 && (b_kmaj ? s.k : s.n) % 4 == 0;
    p.wide = (kn.wide_tile == 1 || (kn.wide_tile == 2 && a_kmaj) || (kn.wide_tile == 3 && a_kmaj && b_kmaj)) && kn.pipe == 2 && vec &&
             s.k % GK == 0 && s.n % 256 == 0 && !s.colsum && !want_ksum && 256 * s.ldb * 4 < ((int64_t)1 << 30);
    const int tile_n = p.wide ? 256 : BN;
    p.tiles_m = (s.m + BM - 1) / BM;
    p.tiles_n = (s.n + tile_n - 1) / tile_n;
    // the buffer epilogue addresses one block (<= 256 rows) at a time: its row pitches must keep that below 2^31
    auto fits = [&](int64_t ld) { return (256 * ld + s.n) * 4 < ((int64_t)1 << 31); };
    p.buf_ok = kn.buf_epilogue && fits(s.ldc) && (!(epi & NPM_EPI_RESIDUAL) || fits(s.ldr)) &&
               (!(epi & (NPM_EPI_RELU_SAVE | NPM_EPI_RELU_MASK | NPM_EPI_SOFTMAX_BWD | NPM_EPI_ROWDOT)) || fits(s.ldaux)) && fits(s.n);

    // Split-K: only for the linear epilogues, when the grid cannot fill 256 CUs x 2-3 blocks.
    const int64_t batch = (int64_t)s.batch0 * s.batch1;
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n * batch;
    const int nkt = (s.k + BK - 1) / BK;
    const bool linear = !(epi & (NPM_EPI_RELU_SAVE | NPM_EPI_RELU_MASK | NPM_EPI_RELU | NPM_EPI_SOFTMAX_BWD | NPM_EPI_ROWDOT));
    int splits = 1;
    if (s.split_k > 1) {
        splits = s.split_k;
    } else if (s.split_k == 0 && linear && tiles < 2L * num_cus && nkt >= 16) {
        // (several generations of shorter K ranges: measured to pay for the A-heavy products that also sum A's columns -- the packed
        //  q/k/v weight gradient [3F, F] -- and to cost 0.3 ms per step on the FFN weight gradients, which sum B's: profiles/r04_splitk_sweep.log)
        const bool more_generations = kn.math == 0 && kn.split_gens && s.asum && p.tiles_m > p.tiles_n;
        splits = pick_splits(tiles, nkt, num_cus, 0, resident_blocks(kn.math), more_generations ? 1 : 0);
    }
    if (!linear || s.colsum) splits = 1;
    const SplitRanges r = split_ranges(splits, nkt, BK);
    p.splits = r.splits;
    p.k_per_split = r.k_per_split;
    p.grid = tiles * p.splits;

    const int64_t a_span = (a_kmaj ? (int64_t)BM * s.lda + s.k : (int64_t)p.k_per_split * s.lda + BM) * 4;
    const int64_t b_span = (b_kmaj ? (int64_t)tile_n * s.ldb + s.k : (int64_t)p.k_per_split * s.ldb + tile_n) * 4;
    const bool dma = kn.pipe == 2 && vec && s.k % GK == 0 && a_span < ((int64_t)1 << 31) && b_span < ((int64_t)1 << 31);
    const bool dma_path = dma && p.buf_ok;
    const bool rowdot = (epi & NPM_EPI_ROWDOT) != 0;
    if (p.grid >= ((int64_t)1 << 31)) p.refusal = GemmRefusal::GRID;
    else if (p.wide && !dma_path) p.refusal = GemmRefusal::WIDE_SPANS;
    else if (rowdot && !(dma_path && a_kmaj && !b_kmaj && !p.wide && batch == 1 && p.splits == 1 && s.n % 128 == 0 && kn.math == 0 &&
                         !s.diagnostics))
        p.refusal = GemmRefusal::ROWDOT;

    const int math = kn.math == NPM_MATH_F16X2 ? NPM_MATH_BF16X3 : kn.math;      // where the f16x2 kernel does not apply: the bf16 split
    p.block = 256;
    if (kn.math == NPM_MATH_F16X2 && dma_path && batch == 1 && !p.wide && !s.colsum && s.k > 0 && !s.diagnostics) {
        p.kernel = GemmKernel::F16X2;
        p.math = NPM_MATH_F16X2;
    } else if (!dma) {
        p.kernel = !vec ? GemmKernel::STAGED_SCALAR : kn.pipe == 1 ? GemmKernel::STAGED_VEC_2BUF : GemmKernel::STAGED_VEC;
    } else if (want_ksum && dma_path && !a_kmaj && !b_kmaj && s.k > 0) {
        p.kernel = GemmKernel::DMA_KSUM;
        p.math = math;
        p.ksum_op = s.bsum ? 1 : 2;
        p.ksum_rows = (int64_t)p.splits * std::min(s.bsum ? p.tiles_m : p.tiles_n, GK);
    } else if (p.wide) {
        p.kernel = GemmKernel::DMA_WIDE;
        p.block = 512;
    } else if (s.colsum && dma_path) {
        p.kernel = GemmKernel::DMA_COLSUM;
        p.colsum_fused = true;
    } else if (math != 0) {
        p.kernel = math == 1 ? GemmKernel::DMA_MATH1 : GemmKernel::DMA_MATH2;
        p.math = math;
    } else {
        p.kernel = rowdot ? GemmKernel::DMA_ROWDOT : GemmKernel::DMA;
    }
    return p;
}

// ---- Conv2D ----------------------------------------------------------------------------------------------------------------------
struct ConvKnobs {                  // NPM_TUNE_CONV_DMA, _CONV_KORDER, NPM_TUNE_GEMM_MATH (0 / 1 / 2), _CONV_WGRAD_BLOCKS, _CONV_WGRAD_FUSED; npm::ksync_every()
    int dma = 1, korder = 1, math = 0, wgrad_blocks = 0, wgrad_fused = 1, ksync_every = 128;
};

enum class ConvKernel { SCALAR, VEC, DMA, TALL };

// What npm_last_conv_kernel reports (include/npm_hip.h).
struct ConvReport {
    const char *family;
    bool vec, tall;
    int math, korder;
    bool buf;
    int splits, kper, wr;
    bool trio;
    int ksync;
};
inline void format_conv_report(char *out, size_t size, const ConvReport &r) {
    snprintf(out, size, "%s vec=%d tall=%d math=%d korder=%d buf=%d splits=%d kper=%d wr=%d trio=%d ksync=%d", r.family, (int)r.vec,
             (int)r.tall, r.math, r.korder, (int)r.buf, r.splits, r.kper, r.wr, (int)r.trio, r.ksync);
}

struct ConvGemmPlan {               // forward and grad_x: the pixels are the rows
    ConvKernel kernel;
    bool fits;                      // the grid is below 2^31 blocks
    int64_t grid;
    int k, tiles_m, tiles_n;
    bool buf_ok;
    int math;                       // what runs: the knob on the DMA kernels, else 0
    ConvReport report;
};

inline ConvGemmPlan conv_gemm_plan(int64_t pixels, int w, int c, int n_out, int ks, bool aligned, const ConvKnobs &kn) {
    ConvGemmPlan p{};
    p.k = ks * ks * c;
    const int64_t pad = ks / 2, halo = pad * w + pad;
    const bool vec = c % 4 == 0 && n_out % 4 == 0 && aligned;
    p.buf_ok = kn.dma && (256L * n_out + n_out) * 4 < ((int64_t)1 << 31);
    const bool dma = kn.dma && vec && c % GK == 0 && (256 + 2 * halo) * c * 4 < ((int64_t)1 << 30) &&
                     (int64_t)p.k * n_out * 4 < ((int64_t)1 << 31);
    const bool tall = dma && n_out <= 64 && n_out % 16 == 0 && kn.dma != 2;
    p.kernel = tall ? ConvKernel::TALL : dma ? ConvKernel::DMA : vec ? ConvKernel::VEC : ConvKernel::SCALAR;
    p.tiles_m = (int)((pixels + (tall ? 255 : BM - 1)) / (tall ? 256 : BM));
    p.tiles_n = (n_out + (tall ? 63 : BN - 1)) / (tall ? 64 : BN);
    p.grid = (int64_t)p.tiles_m * p.tiles_n;
    p.fits = p.grid < ((int64_t)1 << 31);
    p.math = dma ? kn.math : 0;
    p.report = {dma ? "conv_fwd_glds" : "conv_fwd", vec, tall, p.math, dma ? kn.korder : 0, dma && p.buf_ok, 1, p.k, 0, false, 0};
    return p;
}

struct ConvWgradPlan {              // the filter gradient: the pixels are K
    ConvKernel kernel;              // SCALAR, VEC or DMA
    int m, tiles_m, tiles_n, splits, k_per_split, grid;
    bool buf_ok;
    int math;
    ConvReport report;
};

inline ConvWgradPlan conv_wgrad_plan(int64_t pixels, int w, int c_in, int c_out, int ks, bool aligned, const ConvKnobs &kn, int num_cus) {
    ConvWgradPlan p{};
    p.m = ks * ks * c_in;
    p.tiles_m = (p.m + BM - 1) / BM;
    p.tiles_n = (c_out + BN - 1) / BN;
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n;
    const int nkt = (int)((pixels + BK - 1) / BK);
    int splits = 1;
    // 5 tiles x 154 splits = 770 blocks left a quarter of the CUs with 4 blocks and the rest with 3 (19.9 ms at C3);
    // pick_splits keeps every CU equally full.
    if (tiles < 2L * num_cus && nkt >= 16) {
        if (kn.wgrad_blocks < 0) splits = (int)std::min<int64_t>((3L * num_cus + tiles - 1) / tiles, nkt / 8);
        else splits = pick_splits(tiles, nkt, num_cus, kn.wgrad_blocks, resident_blocks(kn.math));
    }
    const SplitRanges r = split_ranges(splits, nkt, BK);
    p.splits = r.splits;
    p.k_per_split = r.k_per_split;
    p.grid = (int)(tiles * p.splits);
    const int64_t pad = ks / 2, halo = pad * w + pad;
    const bool vec = c_in % 4 == 0 && c_out % 4 == 0 && aligned;
    p.buf_ok = kn.dma && (256L * c_out + c_out) * 4 < ((int64_t)1 << 31);
    const bool dma = kn.dma && vec && pixels % GK == 0 && (p.k_per_split + 2 * halo + GK) * c_in * 4 < ((int64_t)1 << 30) &&
                     (int64_t)p.k_per_split * c_out * 4 < ((int64_t)1 << 30);
    p.kernel = dma ? ConvKernel::DMA : vec ? ConvKernel::VEC : ConvKernel::SCALAR;
    p.math = dma ? kn.math : 0;
    p.report = {dma ? "conv_wgrad_glds" : "conv_wgrad", vec, false, p.math, 0, dma && p.buf_ok, p.splits, p.k_per_split, 0, false, 0};
    return p;
}

struct ConvWgradFusedPlan {         // npm_conv2d_bwd_w_relu
    bool fused;                     // false: the two-pass form, nothing else is meaningful
    int m, rows, resident;          // tile height 128 (4 blocks per CU) or 192 (3)
    int tiles_m, tiles_n, nkt, splits, kt_per, k_per_split;
    bool trio;
    int parts_m;                    // column-sum partial rows per split
    int grid, block;
    int ksync_every, ksync_epochs;  // the K rendezvous, 0 when it does not engage
    ConvReport report;              // ksync as planned: the entry point reports 0 when the runtime has no counters to give
};

inline ConvWgradFusedPlan conv_wgrad_fused_plan(int64_t pixels, int w, int c_in, int c_out, int ks, bool aligned, const ConvKnobs &kn,
                                                int num_cus) {
    ConvWgradFusedPlan p{};
    p.m = ks * ks * c_in;
    const int64_t pad = ks / 2, halo = pad * w + pad;
    if (!(kn.dma && kn.math == 0 && kn.wgrad_fused && c_in % 4 == 0 && c_out % 4 == 0 && pixels % GK == 0 && w >= GK && aligned &&
          (int64_t)p.m * c_out * 4 < ((int64_t)1 << 31)))
        return p;
    // tile height: the one that pads k*k*C0 least (192-row tiles: 3 blocks per CU, 128-row tiles: 4)
    const int64_t pad128 = (int64_t)((p.m + 127) / 128) * 128, pad192 = (int64_t)((p.m + 191) / 192) * 192;
    const bool tall = kn.wgrad_fused == 3 || (kn.wgrad_fused != 2 && pad192 < pad128);
    p.rows = tall ? 192 : 128;
    p.resident = tall ? 3 : 4;
    p.tiles_m = (p.m + p.rows - 1) / p.rows;
    p.tiles_n = (c_out + BN - 1) / BN;
    const int64_t tiles = (int64_t)p.tiles_m * p.tiles_n;
    p.nkt = (int)(pixels / GK);
    int splits = 1;
    if (tiles < 2L * num_cus && p.nkt >= 16) splits = pick_splits(tiles, p.nkt, num_cus, kn.wgrad_blocks > 0 ? kn.wgrad_blocks : 0, p.resident);
    const SplitRanges r = split_ranges(splits, p.nkt, GK);
    p.splits = r.splits;
    p.kt_per = r.kt_per;
    p.k_per_split = r.k_per_split;
    if (!((p.k_per_split + 2 * halo + GK) * c_in * 4 < ((int64_t)1 << 30) && (int64_t)p.k_per_split * c_out * 4 < ((int64_t)1 << 30) &&
          tiles * p.splits < ((int64_t)1 << 31)))
        return p;
    p.fused = true;
    // TRIO: the three tile rows of a split in one block of twelve waves (NPM_TUNE_CONV_WGRAD_FUSED = 3 keeps the four-wave blocks)
    p.trio = tall && p.tiles_m == 3 && p.splits > 1 && kn.wgrad_fused != 3;
    p.parts_m = p.trio ? 1 : p.tiles_m;
    p.grid = (int)((p.trio ? p.tiles_n : tiles) * p.splits);
    p.block = p.trio ? 768 : 256;
    // K rendezvous: all blocks resident at once (3 or 4 per CU), every split long enough
    if (!p.trio && p.splits > 1 && p.grid <= (int64_t)p.resident * num_cus && kn.ksync_every > 0 && p.kt_per >= 2 * kn.ksync_every) {
        p.ksync_every = kn.ksync_every;
        p.ksync_epochs = (p.nkt - (p.splits - 1) * p.kt_per - 1) / p.ksync_every;
    }
    p.report = {"conv_wgrad_relu", true, false, 0, 0, true, p.splits, p.k_per_split, tall ? 3 : 2, p.trio, p.ksync_every};
    return p;
}

}  // namespace npm
