// The launch plan of the row kernels that keep a row in registers (npm_rowops.hip): which register width a row length takes,
// where the nontemporal hint goes and how large the grid is, as a pure function of explicit inputs.  Plain C++17, no HIP and no
// globals: a host program can include it (tests/test_row_plan_host.py pins the table below).
//
// Common to all kinds:
//   width class   d <= 256 -> VPL 1, <= 512 -> 2, <= 1024 -> 4, <= 2048 -> 8, else 16 (VPL float4 per lane; 0 = the generic kernel)
//   fast path     d % 4 == 0, d <= 4096 and the entry point's alignment condition; otherwise the generic re-reading kernel
//   nt            NPM_TUNE_STREAM_NT on and 4 * rows * d >= 32 MB: the tensor streams through, far more than the caches hold
//   row_blocks    ceil(rows / ROWS_PER_BLOCK)
//   f, b          NPM_TUNE_LN_NT_SPLIT >> 2 (forward mode) and & 3 (backward mode)
//
//   kind                        | hint when nt                                                       | grid
//   ----------------------------+--------------------------------------------------------------------+---------------------------
//   softmax fwd, bwd            | BOTH                                                               | row_blocks
//   layernorm fwd, rmsnorm fwd  | d in (512, 1024]: f == 0 BOTH, f == 1 LOADS, any other f STORES;   | row_blocks
//                               | other widths BOTH                                                  |
//   layernorm bwd, rmsnorm bwd  | d in (512, 1024]: b == 1 LOADS, b == 2 STORES, else BOTH;          | fast: min(row_blocks,
//                               | other widths BOTH                                                  | blocks_per_cu * CUs);
//                               |                                                                    | generic: row_blocks
//   layernorm dropout fwd       | d in (512, 1024] and f == 1: LOADS; otherwise BOTH (f == 2 too:    | row_blocks
//                               | the dropout forms have no stores-only instance)                    |
//   layernorm dropout bwd       | d in (512, 1024] and b == 1: LOADS; otherwise BOTH                 | min(row_blocks,
//                               |                                                                    | blocks_per_cu * CUs)
//
// Without nt the hint is PLAIN everywhere, and the generic kernels never take one.  A grid of row_blocks >= 2^31 does not fit
// (the entry points refuse it); the capped grids always fit.
#pragma once

#include <algorithm>
#include <cstdint>

namespace npm {

constexpr int ROWS_PER_BLOCK = 4;                           // 256 threads = 4 waves, one row per wave
constexpr uint64_t STREAM_NT_BYTES = (uint64_t)32 << 20;    // the L2's size: tensors from here on take the nontemporal instances

enum class RowKind { SOFTMAX, NORM_FWD, NORM_BWD, DROPOUT_FWD, DROPOUT_BWD };
enum class RowHint { PLAIN, BOTH, LOADS, STORES };

struct RowPlan {
    int vpl;         // float4 per lane: 1 / 2 / 4 / 8 / 16, or 0 for the generic kernel
    RowHint hint;
    int grid;        // meaningful when fits
    bool fits;       // the row-block count fits a grid
};

inline RowPlan row_plan(RowKind kind, int64_t rows, int64_t d, bool aligned, int nt_split, bool stream_nt, int blocks_per_cu,
                        int num_cus) {
    RowPlan p{0, RowHint::PLAIN, 0, true};
    const bool fast = d % 4 == 0 && d <= 4096 && aligned;
    if (fast) p.vpl = d <= 256 ? 1 : d <= 512 ? 2 : d <= 1024 ? 4 : d <= 2048 ? 8 : 16;
    if (fast && stream_nt && sizeof(float) * (uint64_t)rows * (uint64_t)d >= STREAM_NT_BYTES) {
        const int f = nt_split >> 2, b = nt_split & 3;
        const bool split = d > 512 && d <= 1024;
        p.hint = RowHint::BOTH;
        if (split && kind == RowKind::NORM_FWD && f != 0) p.hint = f == 1 ? RowHint::LOADS : RowHint::STORES;
        if (split && kind == RowKind::NORM_BWD && (b == 1 || b == 2)) p.hint = b == 1 ? RowHint::LOADS : RowHint::STORES;
        if (split && kind == RowKind::DROPOUT_FWD && f == 1) p.hint = RowHint::LOADS;
        if (split && kind == RowKind::DROPOUT_BWD && b == 1) p.hint = RowHint::LOADS;
    }
    const int64_t row_blocks = (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    if (kind == RowKind::DROPOUT_BWD || (kind == RowKind::NORM_BWD && fast)) {
        p.grid = (int)std::min<int64_t>(row_blocks, (int64_t)blocks_per_cu * num_cus);
    } else {
        p.fits = row_blocks < ((int64_t)1 << 31);
        if (p.fits) p.grid = (int)row_blocks;
    }
    return p;
}

}  // namespace npm
