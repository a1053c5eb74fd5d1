"""CPU: the launch plans of the GEMM and the Conv2D entry points (np_modeling_amd/csrc/npm_gemm_plan.h) as a host program sees them.

The header is plain C++17, so a stand-alone program includes it, reads one request per line and prints the plan.  Two kinds of test:

* literal pins -- expectations worked out by hand from the routing tables in the header's comment, never computed by the code under
  test, at the smallest shapes on each side of each rule.  Which instance a GEMM call ran changes speed and nothing else, so this is
  where its routing is pinned;
* agreement with the restatements the GPU suite vouches for: every case of every list of tests/conv_cases.py and
  tests/gemm_epilogue_cases.py, under that case's knobs, against ``route`` / ``fused_plan`` / ``pick_splits`` resp.
  ``takes_dma_kernel`` / ``takes_wide_tile`` / ``expected_math`` / ``grid_blocks``.  No case is left out.

All pins: 256 CUs and the default knobs unless the case says otherwise; operands aligned, pitches the row widths."""

import os
import shutil
import subprocess

import pytest

import conv_cases as CC
import gemm_epilogue_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'np_modeling_amd', 'csrc')

PROGRAM = r'''#include <cstdio>
#include <cstring>
#include "npm_gemm_plan.h"
using namespace npm;
static long long v[40];
static bool read(int n) {
    for (int i = 0; i < n; ++i)
        if (std::scanf("%lld", &v[i]) != 1) return false;
    return true;
}
int main() {
    static const char *const kernels[] = {"F16X2", "STAGED_SCALAR", "STAGED_VEC_2BUF", "STAGED_VEC", "DMA_KSUM", "DMA_WIDE", "DMA_COLSUM",
                                          "DMA_MATH1", "DMA_MATH2", "DMA_ROWDOT", "DMA"};
    static const char *const refusals[] = {"NONE", "GRID", "WIDE_SPANS", "ROWDOT"};
    char tag[8], text[192];
    while (std::scanf("%7s", tag) == 1) {
        if (!std::strcmp(tag, "gemm")) {
            if (!read(30)) return 1;
            GemmShape s{};
            s.m = (int)v[0]; s.n = (int)v[1]; s.k = (int)v[2]; s.batch0 = (int)v[3]; s.batch1 = (int)v[4];
            s.lda = v[5]; s.ldb = v[6]; s.ldc = v[7]; s.ldr = v[8]; s.ldaux = v[9];
            s.stride_a0 = v[10]; s.stride_a1 = v[11]; s.stride_b0 = v[12]; s.stride_b1 = v[13];
            s.trans_a = v[14] != 0; s.trans_b = v[15] != 0; s.epilogue = (int)v[16];
            s.a_aligned = v[17] != 0; s.b_aligned = v[18] != 0; s.split_k = (int)v[19];
            s.colsum = v[20] != 0; s.bsum = v[21] != 0; s.asum = v[22] != 0; s.diagnostics = v[23] != 0;
            GemmKnobs kn;
            kn.pipe = (int)v[24]; kn.wide_tile = (int)v[25]; kn.buf_epilogue = (int)v[26]; kn.math = (int)v[27]; kn.split_gens = (int)v[28];
            const GemmPlan p = gemm_plan(s, kn, (int)v[29]);
            std::printf("kernel=%s block=%d grid=%lld tiles_m=%d tiles_n=%d splits=%d kper=%d wide=%d buf=%d math=%d ksum_op=%d ksum_rows=%lld "
                        "colsum_fused=%d refusal=%s\n", kernels[(int)p.kernel], p.block, (long long)p.grid, p.tiles_m, p.tiles_n, p.splits,
                        p.k_per_split, (int)p.wide, (int)p.buf_ok, p.math, p.ksum_op, (long long)p.ksum_rows, (int)p.colsum_fused,
                        refusals[(int)p.refusal]);
        } else if (!std::strcmp(tag, "fwd") || !std::strcmp(tag, "wgrad") || !std::strcmp(tag, "fused")) {
            if (!read(13)) return 1;      // pixels w c0 c1 ks aligned | dma korder math blocks fused ksync | cus
            ConvKnobs kn;
            kn.dma = (int)v[6]; kn.korder = (int)v[7]; kn.math = (int)v[8]; kn.wgrad_blocks = (int)v[9]; kn.wgrad_fused = (int)v[10];
            kn.ksync_every = (int)v[11];
            if (tag[1] == 'w') {
                const ConvGemmPlan p = conv_gemm_plan(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5] != 0, kn);
                format_conv_report(text, sizeof(text), p.report);
                std::printf("%s | grid=%lld fits=%d tiles_m=%d tiles_n=%d\n", text, (long long)p.grid, (int)p.fits, p.tiles_m, p.tiles_n);
            } else if (tag[0] == 'w') {
                const ConvWgradPlan p = conv_wgrad_plan(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5] != 0, kn, (int)v[12]);
                format_conv_report(text, sizeof(text), p.report);
                std::printf("%s | grid=%d\n", text, p.grid);
            } else {
                const ConvWgradFusedPlan p = conv_wgrad_fused_plan(v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5] != 0, kn, (int)v[12]);
                if (!p.fused) { std::printf("two_pass\n"); continue; }
                format_conv_report(text, sizeof(text), p.report);
                std::printf("%s | rows=%d tiles_m=%d tiles_n=%d nkt=%d splits=%d kt_per=%d kper=%d trio=%d ksync=%d last_rows=%d grid=%d block=%d "
                            "epochs=%d parts_m=%d\n", text, p.rows, p.tiles_m, p.tiles_n, p.nkt, p.splits, p.kt_per, p.k_per_split, (int)p.trio,
                            p.ksync_every, p.m - (p.tiles_m - 1) * p.rows, p.grid, p.block, p.ksync_epochs, p.parts_m);
            }
        } else if (!std::strcmp(tag, "pick")) {
            if (!read(6)) return 1;
            std::printf("%d\n", pick_splits((long)v[0], (int)v[1], (long)v[2], (int)v[3], (int)v[4], (int)v[5]));
        } else if (!std::strcmp(tag, "ranges")) {
            if (!read(3)) return 1;
            const SplitRanges r = split_ranges((int)v[0], (int)v[1], (int)v[2]);
            std::printf("%d %d %d\n", r.splits, r.kt_per, r.k_per_split);
        } else {
            return 2;
        }
    }
    return 0;
}
'''

MATH = {'f32': 0, 'bf16x3_fast': 1, 'bf16x3': 2, 'f16x2': 3}          # npm_set_math mode -> NPM_MATH_*
RELU, ROWDOT = 16, 128                                                # include/npm_hip.h NPM_EPI_*


# ---- requests ------------------------------------------------------------------------------------------------------------------------------
def gemm(layout, m, n, k, batch=(1, 1), lda=None, ldb=None, ldc=None, ldr=None, ldaux=None, sa=(0, 0), sb=(0, 0), epi=0, aligned=(True, True),
         split_k=1, colsum=False, bsum=False, asum=False, diagnostics=False, pipe=2, wide=0, buf=1, math=0, gens=1, cus=256):
    """One request line for gemm_plan.  Pitches default to the row widths as stored: A [M, K] (TN: [K, M]), B [K, N] (NT: [N, K])."""
    lda = (m if layout == 'TN' else k) if lda is None else lda
    ldb = (k if layout == 'NT' else n) if ldb is None else ldb
    ldc, ldr, ldaux = (n if ld is None else ld for ld in (ldc, ldr, ldaux))
    words = [m, n, k, batch[0], batch[1], lda, ldb, ldc, ldr, ldaux, sa[0], sa[1], sb[0], sb[1], layout == 'TN', layout == 'NT', epi,
             aligned[0], aligned[1], split_k, colsum, bsum, asum, diagnostics, pipe, wide, buf, math, gens, cus]
    return 'gemm ' + ' '.join(str(int(w)) for w in words)


def conv(entry, pixels, w, c0, c1, ks, aligned=True, dma=1, korder=1, math=0, blocks=0, fused=1, ksync=128, cus=256):
    """entry: 'fwd' (conv_gemm_plan: c0 gathered, c1 out), 'wgrad' (conv_wgrad_plan) or 'fused' (conv_wgrad_fused_plan)."""
    return entry + ' ' + ' '.join(str(int(x)) for x in (pixels, w, c0, c1, ks, aligned, dma, korder, math, blocks, fused, ksync, cus))


def conv_of(entry, shape, kn: CC.Knobs, cus, aligned):
    """The request of one conv_cases case: its knobs as the entry points see them (NPM_TUNE_KSYNC through set_ksync_every)."""
    n, h, w, c0, c1, k = shape
    if entry == 'bwd_x':
        c0, c1 = c1, c0
    return conv({'fwd': 'fwd', 'bwd_x': 'fwd', 'bwd_w': 'wgrad', 'bwd_w_relu': 'fused'}[entry], n * h * w, w, c0, c1, k, aligned, kn.dma, kn.korder,
                CC.CONV_MATH[kn.math][0], kn.blocks, kn.fused, CC.ksync_every(kn.ksync), cus)


# ---- literal pins: GEMM --------------------------------------------------------------------------------------------------------------------
def F(**fields):
    return fields


G = gemm
PINS = {}
PINS['alignment_and_pipeline'] = [
    (G('NN', 128, 128, 32), F(kernel='DMA', block=256, grid=1, buf=1, math=0, splits=1, kper=32, refusal='NONE')),
    (G('NN', 128, 128, 72), F(kernel='STAGED_VEC', grid=1, kper=96)),                     # K % 16 != 0
    (G('NN', 128, 128, 30), F(kernel='STAGED_SCALAR')),                                   # K-major A with K % 4 != 0
    (G('NN', 128, 130, 32), F(kernel='STAGED_SCALAR', tiles_n=2, grid=2)),                # B [K, N] with N % 4 != 0
    (G('NN', 128, 130, 32, ldb=132), F(kernel='STAGED_SCALAR')),                          # ... whatever the pitch
    (G('TN', 130, 128, 32), F(kernel='STAGED_SCALAR', tiles_m=2)),                        # A [K, M] with M % 4 != 0
    (G('TN', 130, 128, 32, lda=132), F(kernel='STAGED_SCALAR')),
    (G('TN', 132, 128, 32), F(kernel='DMA', grid=2)),
    (G('NT', 129, 129, 32), F(kernel='DMA', tiles_m=2, tiles_n=2, grid=4)),               # K-major operands: any M and N
    (G('NN', 128, 128, 32, lda=34), F(kernel='STAGED_SCALAR')),                           # a pitch that is no multiple of 4
    (G('NN', 128, 128, 32, batch=(2, 1), sa=(4098, 0)), F(kernel='STAGED_SCALAR', grid=2)),   # a batch stride that is none
    (G('NN', 128, 128, 32, batch=(2, 1), sa=(4096, 0)), F(kernel='DMA', grid=2)),
    (G('NN', 128, 128, 32, aligned=(False, True)), F(kernel='STAGED_SCALAR')),
    (G('NN', 128, 128, 32, aligned=(True, False)), F(kernel='STAGED_SCALAR')),
    (G('NN', 128, 128, 32, pipe=0), F(kernel='STAGED_VEC', math=0)),
    (G('NN', 128, 128, 32, pipe=1), F(kernel='STAGED_VEC_2BUF', math=0)),
    (G('NN', 128, 130, 32, pipe=1), F(kernel='STAGED_SCALAR')),
    (G('NN', 128, 128, 32, pipe=1, math=2), F(kernel='STAGED_VEC_2BUF', math=0)),         # the staged kernels are exact f32 only
    (G('NN', 128, 128, 32, buf=0), F(kernel='DMA', buf=0)),                               # the DMA kernel with the plain epilogue
    # buf_ok: (256 * ld + n) * 4 < 2^31 <=> ld <= 2097151 at n = 128; ldr / ldaux only where the epilogue reads them
    (G('NN', 128, 128, 32, ldc=2097151), F(kernel='DMA', buf=1)),
    (G('NN', 128, 128, 32, ldc=2097152), F(kernel='DMA', buf=0)),
    (G('NN', 128, 128, 32, ldr=2097152), F(buf=1)),
    (G('NN', 128, 128, 32, ldr=2097152, epi=2), F(buf=0)),
    (G('NN', 128, 128, 32, ldaux=2097152, epi=1), F(buf=1)),
    (G('NN', 128, 128, 32, ldaux=2097152, epi=8), F(buf=0)),
    # operand panels of a block below 2^31 bytes: K-major A (128 * lda + k) * 4, lda % 4 == 0
    (G('NN', 128, 128, 32, lda=4194300), F(kernel='DMA')),
    (G('NN', 128, 128, 32, lda=4194304), F(kernel='STAGED_VEC')),
]
PINS['every_instance'] = (
    # the fused k-sums: TN, operand 1 (bsum) and 2 (asum) under each math mode; 3 x 2 tiles: min(3, 16) resp. min(2, 16) partial rows
    [(G('TN', 384, 256, 32, bsum=True, math=mode), F(kernel='DMA_KSUM', ksum_op=1, ksum_rows=3, math=mode, block=256, grid=6)) for mode in (0, 1, 2)]
    + [(G('TN', 384, 256, 32, asum=True, math=mode), F(kernel='DMA_KSUM', ksum_op=2, ksum_rows=2, math=mode)) for mode in (0, 1, 2)]
    + [(G('TN', 2176, 128, 64, bsum=True, split_k=2), F(kernel='DMA_KSUM', ksum_rows=32, splits=2)),          # 17 sharing blocks: 16 rows a split
       (G('TN', 384, 256, 72, bsum=True), F(kernel='STAGED_VEC', ksum_op=0, ksum_rows=0)),                    # off the DMA path: a pass over B
       (G('TN', 384, 256, 32, bsum=True, buf=0), F(kernel='DMA', buf=0, ksum_op=0)),
       (G('TN', 384, 256, 0, asum=True), F(kernel='DMA', ksum_op=0)),                                         # k == 0: nothing to sum
       (G('NN', 128, 128, 32, math=1), F(kernel='DMA_MATH1', math=1)),
       (G('NT', 128, 128, 32, math=2), F(kernel='DMA_MATH2', math=2)),
       (G('TN', 128, 128, 32, math=2, buf=0), F(kernel='DMA_MATH2', math=2, buf=0))]
    # the wide tile: knob 1 always, 2 NN / NT, 3 NT only
    + [(G(layout, 128, 256, 32, wide=knob), F(kernel='DMA_WIDE', block=512, wide=1, tiles_n=1, grid=1, math=0) if is_wide else F(kernel='DMA', block=256, wide=0, tiles_n=2, grid=2))
       for knob, wide_layouts in ((1, 'NN NT TN'), (2, 'NN NT'), (3, 'NT'), (0, '')) for layout in ('NN', 'NT', 'TN') for is_wide in [layout in wide_layouts.split()]]
    + [(G('NN', 128, 384, 32, wide=1), F(kernel='DMA', wide=0, tiles_n=3)),                                   # N % 256 != 0
       (G('NN', 128, 512, 32, wide=1), F(kernel='DMA_WIDE', tiles_n=2, grid=2)),
       (G('NN', 128, 256, 72, wide=1), F(kernel='STAGED_VEC', wide=0, refusal='NONE')),                       # off the DMA kernel: no wide tile
       (G('NN', 128, 256, 32, wide=1, colsum=True), F(kernel='DMA_COLSUM', wide=0)),
       (G('TN', 128, 256, 32, wide=1, bsum=True), F(kernel='DMA_KSUM', wide=0)),
       (G('NN', 128, 256, 32, wide=1, math=1), F(kernel='DMA_WIDE', math=0)),                                 # exact f32 whatever the mode
       (G('NN', 128, 256, 32, wide=1, ldb=1048572), F(kernel='DMA_WIDE')),                                    # 256 * ldb * 4 < 2^30
       (G('NN', 128, 256, 32, wide=1, ldb=1048576), F(kernel='DMA', wide=0)),
       (G('NN', 128, 128, 32, colsum=True), F(kernel='DMA_COLSUM', colsum_fused=1, math=0, splits=1)),
       (G('NN', 128, 128, 32, colsum=True, math=2), F(kernel='DMA_COLSUM', colsum_fused=1, math=0)),
       (G('NN', 128, 128, 32, colsum=True, buf=0), F(kernel='DMA', colsum_fused=0)),                          # the pass over the stored C
       (G('NN', 128, 128, 32, colsum=True, buf=0, math=1), F(kernel='DMA_MATH1', colsum_fused=0, math=1)),
       (G('NN', 128, 128, 72, colsum=True), F(kernel='STAGED_VEC', colsum_fused=0)),
       (G('NN', 128, 128, 32, epi=ROWDOT), F(kernel='DMA_ROWDOT', math=0, refusal='NONE')),
       (G('NN', 128, 128, 32, math=3), F(kernel='F16X2', math=3, block=256, grid=1)),
       (G('TN', 128, 128, 32, math=3, asum=True), F(kernel='F16X2', math=3, ksum_op=0)),                      # the sums ride in its scale passes
       # f16x2 lost: the request becomes the bf16 split -- which the wide tile and the epilogue column sums do not run either
       (G('NN', 128, 128, 32, math=3, batch=(2, 1)), F(kernel='DMA_MATH2', math=2)),
       (G('NN', 128, 128, 0, math=3), F(kernel='DMA_MATH2', math=2)),
       (G('NN', 128, 128, 32, math=3, buf=0), F(kernel='DMA_MATH2', math=2)),
       (G('NN', 128, 128, 32, math=3, diagnostics=True), F(kernel='DMA_MATH2', math=2)),
       (G('TN', 128, 128, 0, math=3, asum=True), F(kernel='DMA_MATH2', math=2, ksum_op=0)),
       (G('NN', 128, 256, 32, math=3, wide=1), F(kernel='DMA_WIDE', math=0)),
       (G('NN', 128, 128, 32, math=3, colsum=True), F(kernel='DMA_COLSUM', math=0)),
       (G('NN', 128, 128, 72, math=3), F(kernel='STAGED_VEC', math=0))])
TALL_K = 131072                                                                   # 4096 K tiles of 32
PINS['split_k'] = [
    (G('NN', 128, 128, 4096, split_k=4), F(splits=4, kper=1024, grid=4)),
    (G('NN', 128, 128, 128, split_k=3), F(splits=2, kper=64)),                    # 4 K tiles in ranges of 2
    (G('NN', 128, 128, 128, split_k=100), F(splits=4, kper=32)),                  # clamped to the K tiles
    (G('NN', 128, 128, 100, split_k=8), F(splits=4, kper=32, kernel='STAGED_VEC')),
    (G('NN', 128, 128, 0, split_k=4), F(splits=1, kper=32, grid=1)),              # k == 0
    (G('NN', 128, 128, 4096, split_k=4, epi=RELU), F(splits=1, kper=4096)),       # a non-linear epilogue
    (G('NN', 128, 128, 4096, split_k=0, epi=RELU), F(splits=1, kper=4096)),
    (G('NN', 128, 128, 4096, split_k=4, colsum=True), F(splits=1, kper=4096, kernel='DMA_COLSUM')),
    (G('NN', 128, 128, 4096, split_k=1), F(splits=1, kper=4096)),
    # automatic (split_k = 0).  64 tiles: 3 per CU -> 12, cost 3 / 12; 4 per CU -> 16, cost 4 / 16: no better.  ceil(4096 / 12) = 342
    (G('TN', 1024, 1024, TALL_K, split_k=0), F(splits=12, kper=10944, grid=768, kernel='DMA')),
    (G('TN', 1024, 1024, TALL_K, split_k=0, bsum=True), F(splits=12, kper=10944, ksum_rows=96)),
    # 3 resident blocks (math 1): 3 -> 12, 2 -> 8 at the same cost; 2 resident (math 2, 3): 2 -> 8
    (G('TN', 1024, 1024, TALL_K, split_k=0, math=1), F(splits=12, kernel='DMA_MATH1')),
    (G('TN', 1024, 1024, TALL_K, split_k=0, math=2), F(splits=8, kper=16384, kernel='DMA_MATH2')),
    (G('TN', 1024, 1024, TALL_K, split_k=0, math=3), F(splits=8, kper=16384, kernel='F16X2')),
    # 100 tiles: 3 per CU -> 7, cost 3 / 7; 4 -> 10, cost 4 / 10: better.  With 3 resident: 2 -> 5, cost 2 / 5, better than 3 / 7
    (G('TN', 1280, 1280, TALL_K, split_k=0), F(splits=10, kper=13120)),
    (G('TN', 1280, 1280, TALL_K, split_k=0, math=1), F(splits=5, kper=26240)),
    (G('TN', 1280, 1280, TALL_K, split_k=0, math=2), F(splits=5, kper=26240)),
    # several generations: 24 x 8 tiles, 3 per CU -> 4 splits of 1024 K tiles > 768; 4 x 3 x 256 blocks / 192 tiles = 16
    (G('TN', 3072, 1024, TALL_K, split_k=0, asum=True), F(splits=16, kper=8192, grid=3072, kernel='DMA_KSUM', ksum_rows=128)),
    (G('TN', 3072, 1024, TALL_K, split_k=0, asum=True, gens=0), F(splits=4, kper=32768)),
    (G('TN', 3072, 1024, TALL_K, split_k=0), F(splits=4)),                        # only beside asum,
    (G('TN', 1024, 3072, TALL_K, split_k=0, asum=True), F(splits=4)),             # with more tile rows than columns,
    (G('TN', 3072, 1024, TALL_K, split_k=0, asum=True, math=1), F(splits=4)),     # in exact f32: 3 resident, 3 -> 4, 2 -> 2 no better
    # 384 tiles are split in two (3 per CU: 2, cost 3 / 2), 512 = 2 x CUs are not; 128 tiles at 64 CUs likewise
    (G('TN', 2048, 3072, TALL_K, split_k=0), F(splits=2, kper=65536, grid=768)),
    (G('TN', 2048, 4096, TALL_K, split_k=0), F(splits=1, kper=TALL_K, grid=512)),
    (G('TN', 1024, 1024, TALL_K, split_k=0, batch=(8, 1)), F(splits=1, grid=512)),
    (G('TN', 1024, 1024, TALL_K, split_k=0, cus=64), F(splits=3, kper=43712)),    # 3 per CU: 192 / 64 = 3; ceil(4096 / 3) = 1366
    (G('TN', 1024, 2048, TALL_K, split_k=0, cus=64), F(splits=1)),
    # fewer than 16 K tiles are not split; 16 are, nkt / 8 = 2 at most
    (G('TN', 128, 128, 480, split_k=0), F(splits=1, kper=480)),
    (G('TN', 128, 128, 512, split_k=0), F(splits=2, kper=256)),
]
PINS['refusals'] = [
    # the wide tile off the buffer-epilogue DMA kernel: B [K, N] panel (k_per_split * ldb + 256) * 4 at ldb = 2^19
    (G('NN', 128, 256, 992, wide=1, ldb=524288), F(kernel='DMA_WIDE', refusal='NONE')),
    (G('NN', 128, 256, 1024, wide=1, ldb=524288), F(wide=1, refusal='WIDE_SPANS')),
    (G('NN', 128, 256, 32, wide=1, buf=0), F(wide=1, refusal='WIDE_SPANS')),
    # row-dot off its one instance
    (G('NT', 128, 128, 32, epi=ROWDOT), F(refusal='ROWDOT')),
    (G('TN', 128, 128, 32, epi=ROWDOT), F(refusal='ROWDOT')),
    (G('NN', 128, 192, 32, epi=ROWDOT), F(refusal='ROWDOT')),
    (G('NN', 128, 256, 32, epi=ROWDOT), F(kernel='DMA_ROWDOT', refusal='NONE', grid=2)),
    (G('NN', 128, 256, 32, epi=ROWDOT, wide=1), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 72, epi=ROWDOT), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 32, epi=ROWDOT, buf=0), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 32, epi=ROWDOT, batch=(1, 2)), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 32, epi=ROWDOT, math=1), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 32, epi=ROWDOT, diagnostics=True), F(refusal='ROWDOT')),
    (G('NN', 128, 128, 64, epi=ROWDOT, split_k=2), F(kernel='DMA_ROWDOT', splits=1, refusal='NONE')),     # not linear: never split
    # 2^31 blocks: 2^15 x 2^15 batches of one tile, two splits
    (G('NN', 4, 4, 64, batch=(32768, 32767), split_k=2), F(grid=2 ** 31 - 65536, refusal='NONE')),
    (G('NN', 4, 4, 64, batch=(32768, 32768), split_k=2), F(grid=2 ** 31, refusal='GRID')),
    (G('NN', 4, 4, 64, batch=(65536, 32768), epi=ROWDOT), F(grid=2 ** 31, refusal='GRID')),               # the grid first
]


# ---- literal pins: Conv2D ------------------------------------------------------------------------------------------------------------------
def report(family, vec, tall=0, math=0, korder=0, buf=0, splits=1, kper=0, wr=0, trio=0, ksync=0):
    return '%s vec=%d tall=%d math=%d korder=%d buf=%d splits=%d kper=%d wr=%d trio=%d ksync=%d' % (
        family, vec, tall, math, korder, buf, splits, kper, wr, trio, ksync)


GLDS = dict(vec=1, korder=1, buf=1)
CONV_PINS = {}
CONV_PINS['forward'] = [
    # 240 pixels of a 12-wide image, 3 x 3: K = 9 c
    (conv('fwd', 240, 12, 3, 5, 3), report('conv_fwd', 0, kper=27) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    (conv('fwd', 240, 12, 4, 8, 3), report('conv_fwd', 1, kper=36) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    (conv('fwd', 240, 12, 4, 8, 3, aligned=False), report('conv_fwd', 0, kper=36) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    (conv('fwd', 240, 12, 20, 12, 3), report('conv_fwd', 1, kper=180) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),          # c % 16 != 0
    (conv('fwd', 240, 12, 16, 132, 3), report('conv_fwd_glds', kper=144, **GLDS) + ' | grid=4 fits=1 tiles_m=2 tiles_n=2'),
    (conv('fwd', 240, 12, 16, 16, 3), report('conv_fwd_glds', tall=1, kper=144, **GLDS) + ' | grid=1 fits=1 tiles_m=1 tiles_n=1'),
    (conv('fwd', 240, 12, 16, 64, 3), report('conv_fwd_glds', tall=1, kper=144, **GLDS) + ' | grid=1 fits=1 tiles_m=1 tiles_n=1'),
    (conv('fwd', 257, 12, 16, 48, 3), report('conv_fwd_glds', tall=1, kper=144, **GLDS) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    (conv('fwd', 240, 12, 16, 40, 3), report('conv_fwd_glds', kper=144, **GLDS) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),    # N % 16 != 0
    (conv('fwd', 240, 12, 16, 80, 3), report('conv_fwd_glds', kper=144, **GLDS) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),    # N > 64
    (conv('fwd', 240, 12, 16, 16, 3, dma=2), report('conv_fwd_glds', kper=144, **GLDS) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),   # never tall
    (conv('fwd', 240, 12, 16, 16, 3, dma=0), report('conv_fwd', 1, kper=144) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    (conv('fwd', 240, 12, 16, 16, 3, korder=0), report('conv_fwd_glds', 1, tall=1, buf=1, kper=144) + ' | grid=1 fits=1 tiles_m=1 tiles_n=1'),
    (conv('fwd', 240, 12, 16, 132, 3, math=2), report('conv_fwd_glds', math=2, kper=144, **GLDS) + ' | grid=4 fits=1 tiles_m=2 tiles_n=2'),
    (conv('fwd', 240, 12, 16, 16, 3, math=1), report('conv_fwd_glds', tall=1, math=1, kper=144, **GLDS) + ' | grid=1 fits=1 tiles_m=1 tiles_n=1'),
    (conv('fwd', 240, 12, 4, 8, 3, math=2), report('conv_fwd', 1, kper=36) + ' | grid=2 fits=1 tiles_m=2 tiles_n=1'),
    # the halo: (256 + 2 (w + 1)) * 16 * 4 < 2^30 <=> w <= 8388478
    (conv('fwd', 8388478, 8388478, 16, 132, 3), report('conv_fwd_glds', kper=144, **GLDS) + ' | grid=131070 fits=1 tiles_m=65535 tiles_n=2'),
    (conv('fwd', 8388479, 8388479, 16, 132, 3), report('conv_fwd', 1, kper=144) + ' | grid=131070 fits=1 tiles_m=65535 tiles_n=2'),
    # the filter: K * n * 4 < 2^31 at K = 9 * 4096
    (conv('fwd', 240, 12, 4096, 14560, 3), report('conv_fwd_glds', kper=36864, **GLDS) + ' | grid=228 fits=1 tiles_m=2 tiles_n=114'),
    (conv('fwd', 240, 12, 4096, 14564, 3), report('conv_fwd', 1, kper=36864) + ' | grid=228 fits=1 tiles_m=2 tiles_n=114'),
    # the output pitch of the buffer epilogue: (256 n + n) * 4 < 2^31 <=> n <= 2088991 (c = 16, 1 x 1: K * n * 4 stays below 2^31)
    (conv('fwd', 128, 12, 16, 2088988, 1), report('conv_fwd_glds', kper=16, **GLDS) + ' | grid=16321 fits=1 tiles_m=1 tiles_n=16321'),
    (conv('fwd', 128, 12, 16, 2088992, 1), report('conv_fwd_glds', 1, korder=1, buf=0, kper=16) + ' | grid=16321 fits=1 tiles_m=1 tiles_n=16321'),
    # 2^31 blocks: 2^23 tile rows x 256 tile columns
    (conv('fwd', 2 ** 30 - 128, 12, 4, 32768, 1), report('conv_fwd', 1, kper=4) + ' | grid=2147483392 fits=1 tiles_m=8388607 tiles_n=256'),
    (conv('fwd', 2 ** 30, 12, 4, 32768, 1), report('conv_fwd', 1, kper=4) + ' | grid=2147483648 fits=0 tiles_m=8388608 tiles_n=256'),
]
MANY = (16384, 64, 64, 16, 7)                    # 25 x 1 tiles over 512 K tiles of 32
CONV_PINS['filter_gradient'] = [
    # NPM_TUNE_CONV_WGRAD_BLOCKS: 0 -> pick_splits 30 -> ranges of 18: 29; 3 the same; -1 -> ceil(768 / 25) = 31 -> ranges of 17: 31;
    # 4 -> 40 -> ranges of 13: 40; 6 -> 6 * 256 / 25 = 61 -> ranges of 9: 57
    (conv('wgrad', *MANY, blocks=0), report('conv_wgrad_glds', 1, buf=1, splits=29, kper=576) + ' | grid=725'),
    (conv('wgrad', *MANY, blocks=3), report('conv_wgrad_glds', 1, buf=1, splits=29, kper=576) + ' | grid=725'),
    (conv('wgrad', *MANY, blocks=-1), report('conv_wgrad_glds', 1, buf=1, splits=31, kper=544) + ' | grid=775'),
    (conv('wgrad', *MANY, blocks=4), report('conv_wgrad_glds', 1, buf=1, splits=40, kper=416) + ' | grid=1000'),
    (conv('wgrad', *MANY, blocks=6), report('conv_wgrad_glds', 1, buf=1, splits=57, kper=288) + ' | grid=1425'),
    # 2 resident blocks (math 2): 2 per CU -> 20 -> ranges of 26: 20
    (conv('wgrad', *MANY, math=2), report('conv_wgrad_glds', 1, math=2, buf=1, splits=20, kper=832) + ' | grid=500'),
    # 16 K tiles split in two, 15 do not
    (conv('wgrad', 496, 31, 16, 20, 3), report('conv_wgrad_glds', 1, buf=1, splits=2, kper=256) + ' | grid=4'),
    (conv('wgrad', 480, 30, 16, 20, 3), report('conv_wgrad_glds', 1, buf=1, splits=1, kper=480) + ' | grid=2'),
    # the DMA predicate
    (conv('wgrad', 429, 13, 8, 12, 3), report('conv_wgrad', 1, kper=448) + ' | grid=1'),                       # pixels % 16 != 0
    (conv('wgrad', 496, 31, 3, 5, 3), report('conv_wgrad', 0, splits=2, kper=256) + ' | grid=2'),
    (conv('wgrad', 496, 31, 16, 20, 3, aligned=False), report('conv_wgrad', 0, splits=2, kper=256) + ' | grid=4'),
    (conv('wgrad', 496, 31, 16, 20, 3, dma=0), report('conv_wgrad', 1, splits=2, kper=256) + ' | grid=4'),
    (conv('wgrad', 496, 31, 16, 20, 3, math=1), report('conv_wgrad_glds', 1, math=1, buf=1, splits=2, kper=256) + ' | grid=4'),
    (conv('wgrad', 496, 31, 16, 20, 3, dma=0, math=1), report('conv_wgrad', 1, splits=2, kper=256) + ' | grid=4'),
    # 512 tile rows (1 x 1, 65536 channels): never split; (k_per_split + 16) * 65536 * 4 < 2^30 <=> k_per_split < 4080
    (conv('wgrad', 4064, 16, 65536, 4, 1), report('conv_wgrad_glds', 1, buf=1, kper=4064) + ' | grid=512'),
    (conv('wgrad', 4080, 16, 65536, 4, 1), report('conv_wgrad', 1, kper=4096) + ' | grid=512'),
    # ... and k_per_split * 65536 * 4 < 2^30 on the dy side
    (conv('wgrad', 4064, 16, 4, 65536, 1), report('conv_wgrad_glds', 1, buf=1, kper=4064) + ' | grid=512'),
    (conv('wgrad', 4080, 16, 4, 65536, 1), report('conv_wgrad', 1, kper=4096) + ' | grid=512'),
]
RDV = (16384, 64, 64, 128, 3)                    # 3 x 1 tiles of 192 rows over 1024 K tiles of 16: 128 splits of 8


def fused(rows, tiles_m, tiles_n, nkt, splits, kt_per, trio=0, ksync=0, last_rows=None, epochs=0):
    """What the program prints for a fused plan: the report, then the fields."""
    last_rows = rows if last_rows is None else last_rows
    grid = (tiles_n if trio else tiles_m * tiles_n) * splits
    return (report('conv_wgrad_relu', 1, buf=1, splits=splits, kper=kt_per * 16, wr=rows // 64, trio=trio, ksync=ksync)
            + ' | rows=%d tiles_m=%d tiles_n=%d nkt=%d splits=%d kt_per=%d kper=%d trio=%d ksync=%d last_rows=%d grid=%d block=%d epochs=%d parts_m=%d'
            % (rows, tiles_m, tiles_n, nkt, splits, kt_per, kt_per * 16, trio, ksync, last_rows, grid, 768 if trio else 256, epochs,
               1 if trio else tiles_m))


CONV_PINS['fused'] = [
    # tile height by padding: M = 72 -> 128 (192 pads more); 144 -> 192 (256 against 192); 576 -> 3 x 192 (640 against 576)
    (conv('fused', 496, 31, 8, 20, 3), fused(128, 1, 1, 31, 3, 11, last_rows=72)),
    (conv('fused', 496, 31, 16, 20, 3), fused(192, 1, 1, 31, 3, 11, last_rows=144)),
    (conv('fused', 496, 31, 16, 20, 3, fused=2), fused(128, 2, 1, 31, 3, 11, last_rows=16)),
    (conv('fused', 496, 31, 8, 20, 3, fused=3), fused(192, 1, 1, 31, 3, 11, last_rows=72)),
    # exactly three 192-row tile rows and splits: the twelve-wave block; NPM_TUNE_CONV_WGRAD_FUSED = 3 keeps four-wave blocks
    (conv('fused', 496, 31, 64, 20, 3), fused(192, 3, 1, 31, 3, 11, trio=1)),
    (conv('fused', 496, 31, 64, 132, 3), fused(192, 3, 2, 31, 3, 11, trio=1)),
    (conv('fused', 496, 31, 64, 20, 3, fused=3), fused(192, 3, 1, 31, 3, 11)),
    (conv('fused', 496, 31, 64, 20, 3, fused=2), fused(128, 5, 1, 31, 3, 11, last_rows=64)),
    (conv('fused', 240, 16, 64, 20, 3), fused(192, 3, 1, 15, 1, 15)),                      # 15 K tiles: one split, no trio
    (conv('fused', 256, 16, 64, 20, 3), fused(192, 3, 1, 16, 2, 8, trio=1)),               # 16: nkt / 8 = 2
    # M = 3136: 25 x 128 pads less than 17 x 192.  NPM_TUNE_CONV_WGRAD_BLOCKS: -1 counts as 0 here -> 30 -> ranges of 35: 30;
    # 4 -> 40 -> ranges of 26: 40; 6 -> 6 * 256 / 25 = 61 -> ranges of 17: 61
    (conv('fused', 16384, 64, 64, 16, 7, blocks=-1), fused(128, 25, 1, 1024, 30, 35, last_rows=64)),
    (conv('fused', 16384, 64, 64, 16, 7, blocks=0), fused(128, 25, 1, 1024, 30, 35, last_rows=64)),
    (conv('fused', 16384, 64, 64, 16, 7, blocks=4), fused(128, 25, 1, 1024, 40, 26, last_rows=64)),
    (conv('fused', 16384, 64, 64, 16, 7, blocks=6), fused(128, 25, 1, 1024, 61, 17, last_rows=64)),
    # the K rendezvous: four-wave blocks, splits, the grid resident (384 <= 3 * 256), ranges of at least two intervals
    (conv('fused', *RDV, fused=3, ksync=2), fused(192, 3, 1, 1024, 128, 8, ksync=2, epochs=3)),
    (conv('fused', *RDV, fused=3, ksync=4), fused(192, 3, 1, 1024, 128, 8, ksync=4, epochs=1)),
    (conv('fused', *RDV, fused=3, ksync=8), fused(192, 3, 1, 1024, 128, 8)),               # 8 < 2 * 8
    (conv('fused', *RDV, fused=3, ksync=0), fused(192, 3, 1, 1024, 128, 8)),
    (conv('fused', *RDV, fused=1, ksync=2), fused(192, 3, 1, 1024, 128, 8, trio=1)),       # not in the twelve-wave block
    (conv('fused', *RDV, fused=3, ksync=2, cus=64), fused(192, 3, 1, 1024, 64, 16, ksync=2, epochs=7)),
    (conv('fused', *RDV, fused=3, ksync=2, blocks=6), fused(192, 3, 1, 1024, 128, 8, ksync=2, epochs=3)),     # 6 * 256 / 3 = 512 -> nkt / 8 = 128 all the same
    (conv('fused', *RDV, fused=3, ksync=2, cus=32), fused(192, 3, 1, 1024, 32, 32, ksync=2, epochs=15)),       # 96 blocks on 32 CUs
    (conv('fused', 16384, 64, 64, 132, 3, fused=3, ksync=2), fused(192, 3, 2, 1024, 128, 8, ksync=2, epochs=3)),      # 768 blocks fit 256 CUs;
    (conv('fused', *RDV, fused=3, ksync=2, blocks=6, cus=64), fused(192, 3, 1, 1024, 128, 8)),                 # 384 do not fit 64
    # each reason for the two-pass form
    (conv('fused', 480, 15, 8, 20, 3), 'two_pass'),                                        # w < 16
    (conv('fused', 85, 17, 8, 20, 3), 'two_pass'),                                         # pixels % 16 != 0
    (conv('fused', 496, 31, 6, 20, 3), 'two_pass'),
    (conv('fused', 496, 31, 8, 5, 3), 'two_pass'),
    (conv('fused', 496, 31, 16, 20, 3, math=1), 'two_pass'),
    (conv('fused', 496, 31, 16, 20, 3, math=2), 'two_pass'),
    (conv('fused', 496, 31, 16, 20, 3, dma=0), 'two_pass'),
    (conv('fused', 496, 31, 16, 20, 3, fused=0), 'two_pass'),
    (conv('fused', 496, 31, 16, 20, 3, aligned=False), 'two_pass'),
    # M * c_out * 4 < 2^31 at M = 65536 (1 x 1): 512 x 64 tiles of 128 rows, never split
    (conv('fused', 496, 31, 65536, 8188, 1), fused(128, 512, 64, 31, 1, 31)),
    (conv('fused', 496, 31, 65536, 8192, 1), 'two_pass'),
    # the span limits after the split, as for the two-pass filter gradient
    (conv('fused', 4064, 16, 65536, 4, 1), fused(128, 512, 1, 254, 1, 254)),
    (conv('fused', 4080, 16, 65536, 4, 1), 'two_pass'),
    (conv('fused', 4080, 16, 4, 65536, 1), fused(128, 1, 512, 255, 1, 255, last_rows=4)),
    (conv('fused', 4096, 16, 4, 65536, 1), 'two_pass'),
]

# pick_splits(tiles, nkt, cus, force_per_cu, resident, generations) and split_ranges(splits, nkt, k_tile), by hand
FUNCTION_PINS = [
    ('pick 2 16 256 0 4 0', '2'), ('pick 25 512 256 0 4 0', '30'), ('pick 25 512 256 4 4 0', '40'), ('pick 25 512 256 6 4 0', '61'),
    ('pick 25 512 256 12 4 0', '64'), ('pick 25 512 256 0 2 0', '20'), ('pick 3 1024 256 0 3 0', '128'), ('pick 600 512 256 0 4 0', '1'),
    ('pick 192 4096 256 0 4 0', '4'), ('pick 192 4096 256 0 4 1', '16'), ('pick 64 4096 256 0 4 1', '12'),
    ('ranges 30 512 32', '29 18 576'), ('ranges 61 512 32', '57 9 288'), ('ranges 3 4 32', '2 2 64'), ('ranges 100 4 32', '4 1 32'),
    ('ranges 0 31 16', '1 31 496'), ('ranges 1 0 32', '1 1 32'), ('ranges 4 0 32', '1 1 32'), ('ranges 4 33 16', '4 9 144'),
]


# ---- agreement with the Python restatements --------------------------------------------------------------------------------------------------
CUS = (256, 304, 64)


def conv_agreement():
    """(request, expected line prefix, expected fused fields or None) for every case of every list tests/test_conv_host.py walks, at
    its CU counts; the forward and filter-gradient lists under every math mode as there."""
    out = []
    for cus in CUS:
        for case in CC.FWD_PLAIN + CC.FWD_DMA + CC.FWD_KNOBS + CC.FWD_PRIO + CC.FWD_MISALIGNED:
            for mode in CC.CONV_MATH:
                kn = case.knobs._replace(math=mode)
                for entry in ('fwd', 'bwd_x'):
                    out.append((conv_of(entry, case.shape, kn, cus, not case.offset), CC.route(entry, *case.shape, kn, cus, aligned=not case.offset), None))
        for case in CC.WGRAD_DMA + CC.WGRAD_PLAIN:
            for mode in CC.CONV_MATH:
                kn = case.knobs._replace(math=mode)
                out.append((conv_of('bwd_w', case.shape, kn, cus, not case.offset), case.route(cus, mode), None))
        rendezvous = [CC.FusedCase('rendezvous', *CC.RENDEZVOUS_SHAPE, CC.Knobs(fused=f, ksync=every)) for every in CC.RENDEZVOUS_KSYNC for f in (3, 1)]
        for case in CC.FUSED + CC.FUSED_FALLBACK + rendezvous:
            want = case.route(cus)
            plan = CC.fused_plan(*case.shape, case.knobs, cus, aligned=not case.offset)
            assert (plan is None) == want.startswith('two_pass ')
            out.append((conv_of('bwd_w_relu', case.shape, case.knobs, cus, not case.offset), 'two_pass' if plan is None else want, plan))
            if plan is None:         # the two-pass form reports the filter gradient's own plan
                out.append((conv_of('bwd_w', case.shape, case.knobs, cus, not case.offset), want[len('two_pass '):], None))
    return out


def gemm_of(case: GC.Case, **knobs):
    d, fam = GC.describe(case), GC.FAMILY[case.family]
    return gemm(case.layout, case.m, case.n, case.k, case.batch, d.lda, d.ldb, d.ldc, d.ldr, d.ldaux, d.sa, d.sb, epi=fam.flags,
                split_k=case.split_k, colsum=fam.colsum, **knobs)


def gemm_lists():
    grid = [c for family, layout in GC.GRID for c in GC.cases(family, layout)]
    tile_map = [c for kind in GC.TILE_MAP_KINDS for c in GC.tile_map_cases(kind)]
    wide = [c for family in GC.WIDE_FAMILIES for layout in GC.WIDE_LAYOUTS for c in GC.wide_cases(family, layout)]
    staged = [c for family in GC.PIPELINE_FAMILIES for layout in GC.LAYOUTS for c in GC.pipeline_cases(family, layout)]
    return dict(grid=grid, tile_map=tile_map, wide=wide, staged=staged)


DMA_KERNELS = {'F16X2', 'DMA_KSUM', 'DMA_WIDE', 'DMA_COLSUM', 'DMA_MATH1', 'DMA_MATH2', 'DMA_ROWDOT', 'DMA'}
MODE_OF = {v: k for k, v in MATH.items()}


def gemm_agreement():
    """(request, {field: expected}) for every case of every list of tests/gemm_epilogue_cases.py.  ``dma_path`` is "an LDS-DMA kernel
    (the f16x2 kernel has the same predicate) with the buffer epilogue"."""
    out = []
    for name, listed in gemm_lists().items():
        for case in listed:
            dma = GC.takes_dma_kernel(case)
            for pipe, buf in ((2, 1), (0, 1), (1, 1), (2, 0)):
                out.append((gemm_of(case, pipe=pipe, buf=buf), dict(dma_path=GC.takes_dma_kernel(case, pipeline=pipe, buf_epilogue=buf))))
            out.append((gemm_of(case), dict(grid=GC.grid_blocks(case), wide=0)))
            is_wide = GC.takes_wide_tile(case)
            out.append((gemm_of(case, wide=1), dict(wide=int(is_wide), dma_path=dma)))
            for mode, value in MATH.items():
                out.append((gemm_of(case, math=value), dict(mode=GC.expected_math(case, mode, dma=dma))))
                out.append((gemm_of(case, math=value, wide=1), dict(mode=GC.expected_math(case, mode, wide=is_wide, dma=dma))))
                for pipe in (0, 1):                   # test_register_staged_kernels: exact f32 whatever the mode
                    out.append((gemm_of(case, math=value, pipe=pipe), dict(mode='f32')))
                if dma:                               # test_epilogue_instance_at_tile_edges: the DMA kernel with the plain epilogue
                    out.append((gemm_of(case, math=value, buf=0), dict(mode='bf16x3' if mode == 'f16x2' else mode, colsum_fused=0)))
    return out


# ---- one compile, one run ------------------------------------------------------------------------------------------------------------------
def all_requests():
    reqs = [r for group in PINS.values() for r, _ in group] + [r for group in CONV_PINS.values() for r, _ in group]
    reqs += [r for r, _ in FUNCTION_PINS] + [r for r, _, _ in conv_agreement()] + [r for r, _ in gemm_agreement()]
    return list(dict.fromkeys(reqs))


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    """Every request's printed plan, keyed by the request line: one compile and one run for the module."""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    tmp = tmp_path_factory.mktemp('gemm_plan')
    src, exe = str(tmp / 'gemm_plan.cpp'), str(tmp / 'gemm_plan')
    with open(src, 'w') as f:
        f.write(PROGRAM)
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', CSRC, '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
    reqs = all_requests()
    lines = subprocess.run([exe], input='\n'.join(reqs) + '\n', check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(reqs)
    return dict(zip(reqs, lines))


def gemm_fields(line):
    out = {}
    for word in line.split():
        key, value = word.split('=')
        out[key] = int(value) if value.lstrip('-').isdigit() else value
    out['dma_path'] = out['kernel'] in DMA_KERNELS and out['buf'] == 1
    out['mode'] = MODE_OF[out['math']]
    return out


@pytest.mark.parametrize('group', sorted(PINS))
def test_gemm_plan(plans, group):
    for request, want in PINS[group]:
        got = gemm_fields(plans[request])
        assert {key: got[key] for key in want} == want, request


def test_gemm_pins_name_every_instance_and_refusal():
    kernels = {want['kernel'] for group in PINS.values() for _, want in group if 'kernel' in want}
    assert kernels == DMA_KERNELS | {'STAGED_SCALAR', 'STAGED_VEC', 'STAGED_VEC_2BUF'}
    assert {want['refusal'] for _, want in PINS['refusals']} == {'NONE', 'GRID', 'WIDE_SPANS', 'ROWDOT'}
    ksum = {(want['ksum_op'], want['math']) for _, want in PINS['every_instance'] if want.get('kernel') == 'DMA_KSUM' and 'ksum_op' in want}
    assert ksum == {(op, mode) for op in (1, 2) for mode in (0, 1, 2)}


@pytest.mark.parametrize('group', sorted(CONV_PINS))
def test_conv_plan(plans, group):
    got = {request: plans[request] for request, _ in CONV_PINS[group]}
    assert got == dict(CONV_PINS[group])


def test_pick_splits_and_split_ranges(plans):
    assert {request: plans[request] for request, _ in FUNCTION_PINS} == dict(FUNCTION_PINS)
    # the compiled pick_splits against the restatement, on the hand-evaluated values of test_conv_host.test_pick_splits_restatement
    for args in ((2, 16, 256), (25, 512, 256), (25, 512, 256, 4), (25, 512, 256, 6), (25, 512, 256, 12), (25, 512, 256, 0, 2), (3, 1024, 256, 0, 3),
                 (600, 512, 256)):
        full = args + (0, 4)[len(args) - 3:]
        assert int(plans['pick %d %d %d %d %d 0' % full]) == CC.pick_splits(*args), args


def test_conv_plans_agree_with_the_restated_dispatch(plans):
    listed = conv_agreement()
    assert len(listed) > 3000
    for request, want, plan in listed:
        got = plans[request]
        assert got.split(' | ')[0] == want, request
        if plan is not None:
            fields = dict(word.split('=') for word in got.split(' | ')[1].split())
            assert {key: int(fields[key]) for key in plan} == {key: int(value) for key, value in plan.items()}, request


def test_gemm_plans_agree_with_the_restated_dispatch(plans):
    listed = gemm_agreement()
    lists = gemm_lists()
    assert len(lists['grid']) > 800 and len(lists['wide']) == 64 and len(lists['staged']) == 30 and len(lists['tile_map']) == 36
    assert len(listed) >= 22 * sum(len(v) for v in lists.values())
    for request, want in listed:
        got = gemm_fields(plans[request])
        assert got['refusal'] == 'NONE', request
        assert {key: got[key] for key in want} == want, request
