// Prefill attention: T new query tokens per sequence straight over a key / value cache, with no limit on T (include/npm_hip.h:
// npm_mha_prefill_fwd).  The contract is that of npm_mha_decode_fwd / _varlen / _paged (csrc/npm_decode.hip) on the same
// npm_mha_decode descriptor; what differs is the shape of the work.  A decode step is one pass over a long stream of keys for a
// handful of rows, so that kernel splits the KEYS over waves and blocks.  A prompt, a chunk of one, or a sequence admitted into a
// running batch brings many rows, so this kernel splits the ROWS:
//   * a block covers a tile of ROWS = 64 query rows of ONE K / V head c of one sequence: the (query head of the group, token)
//     pairs of GB = min(Hq / Hkv, ROWS) heads c + g Hkv and TB = ROWS / GB consecutive tokens, so K / V of head c is read once for
//     the whole group, as in the decode kernel.  grid = (token tiles x head chunks, Hkv, B).
//   * each of the four waves owns 16 of those rows for the WHOLE key walk (online softmax in registers, nothing to merge), and
//     the waves SHARE every 16-key tile: the block stages it once in LDS (K padded against bank conflicts, V plain: the reads
//     below are then conflict free or two-way on one slot), double buffered, one barrier per tile; the global loads of tile
//     i + 1 are in flight while tile i is multiplied.
//   * the key walk stops at the tile's own limit: a block walks key tiles 0 .. ceil(max limit of its rows / 16) - 1, which skips
//     the causal upper triangle and everything at or past L_b, and a wave skips the products of a tile none of its rows sees.
//   * a block whose token tile starts at or past n_b stores its rows (ctx = 0, lse = -inf) and returns before it loads anything.
//   * keys are not split over blocks: every valid row of sequence b is a function of that sequence's q, rows, L_b, n_b and
//     new_tokens alone -- bitwise the same at batch 1, under a larger d->kv_len, through a block table or with the length arrays.
//
// There is no [T, L] object anywhere: causality and lengths are arithmetic on (t, j, L_b, n_b), the lengths are read on the device
// (block-uniform scalar loads), keys are addressed in place -- paged: ONE wave-uniform table lookup per key tile; page_rows is a
// power of two >= 16, so a tile never straddles a page.
//
// MFMA orientation, score masking, the raw running maximum and the exponent arithmetic are those of mha_decode_kernel, operation
// for operation (see the head of npm_decode.hip): S^T = K Q^T with the QUERY ROW on the lane, O^T += V^T P^T with P^T register
// for register the B operand; -inf by SELECTION; loads of keys at or past L_b redirected to key L_b - 1 (in bounds, and inside the
// tile's own page: a walked tile holds a key < L_b), V of such keys zeroed on its way into LDS; table entries past a sequence's
// last page are not read (no walked tile lies there).  Exact fp32 MFMA, contraction off, every fma written out, no atomics.
//
// Half-precision cache (npm_mha_prefill_fwd_f16): the storage type of the cache rows is a parameter KV of the block's body
// (npm_prefill_block.h), float (mha_prefill_kernel, unchanged) or _Float16 (mha_prefill_f16_kernel).  Only the base pointers, load_tile and
// store_tile know it: a 16-byte piece is 8 halves instead of 4 floats (TILE D / 8 pieces a tile: one per thread at D 128, a
// partly used pass below that), kept as halves while in flight and converted exactly (v_cvt_f32_f16: subnormals, +-0 and inf are
// kept) on the way into LDS, as two 16-byte stores.  LDS then holds the same fp32 tiles in the same layout, and everything after
// the barrier is the same code: the fp16 call is BITWISE the fp32 call on a cache holding the rounded values.  Pitches, strides
// and the page stride count halves.  The fp16 instances carry a kernel name of their own so that the twelve fp32 instances keep
// theirs, symbol for symbol.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "npm_kvattn.h"

namespace {

constexpr int WAVES = 4;          // per block
constexpr int ROWS = WAVES * 16;  // query rows per block

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

char g_last[128] = "";

struct PrefillArgs {
    const float *q, *k, *v;       // k, v: the cache in its storage type KV (halves behind a float pointer for KV = _Float16)
    long q_pitch, k_pitch, k_sb, v_pitch, v_sb;   // k_ / v_: in elements of KV
    float *ctx;
    long ctx_pitch;
    float *lse;                   // optional [B, Hq, T]
    int heads, kv_heads, tokens, len, causal;
    int group, gb, tb, head_chunks;   // Hq / Hkv; heads of the group and tokens per block (gb tb <= ROWS); ceil(group / gb)
    float c, scale;               // scale * log2(e), scale
    int window;                   // npm_mha_prefill_fwd_window: keys a row sees, itself included (read by the WN instances only)
};

// D: head size.  VL: the sequence has L = kv_lens[b] valid keys and nb = new_lens[b] (NULL: a.tokens) new tokens; VL = false reads
// neither array (L = a.len, nb = a.tokens) and is otherwise the same code.  PG (implies VL): a.k / a.v are page pools, a.k_sb /
// a.v_sb the page strides, pg the block table.  KV: the storage type of the cache, float or _Float16 (npm_mha_prefill_fwd_f16);
// the body is npm_prefill_block.h, the same text for both.
template <int D, bool VL, bool PG>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefill_kernel(const PrefillArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    using KV = float;
    constexpr bool WN = false;
#include "npm_prefill_block.h"
}

template <int D, bool VL, bool PG>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefill_f16_kernel(const PrefillArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    using KV = _Float16;
    constexpr bool WN = false;
#include "npm_prefill_block.h"
}

// Sliding-window attention (npm_mha_prefill_fwd_window), per-sequence layouts only: row t sees keys max(0, limit - a.window) <= j
// < limit.  The block's walk starts at the tile of the smallest floor of its live rows, a wave skips the tiles wholly below its
// own rows' smallest floor as it skips those at and above wlimit; a key below a row's floor gets -inf by selection and V rows
// below the block's smallest floor are zeroed on their way into LDS.  Kernel names of their own: the instances above keep theirs.
template <int D, bool PG>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefill_window_kernel(const PrefillArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    using KV = float;
    constexpr bool VL = true, WN = true;
#include "npm_prefill_block.h"
}

template <int D, bool PG>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefill_window_f16_kernel(const PrefillArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    using KV = _Float16;
    constexpr bool VL = true, WN = true;
#include "npm_prefill_block.h"
}

template <int D, typename KV>
void launch_prefill(const PrefillArgs &a, const int *kv_lens, const int *new_lens, const PageArgs &pg, dim3 grid, hipStream_t s) {
    const dim3 block(WAVES * 64);
    if (a.window > 0) {
        if constexpr (sizeof(KV) == 2) {
            if (pg.table) hipLaunchKernelGGL((mha_prefill_window_f16_kernel<D, true>), grid, block, 0, s, a, kv_lens, new_lens, pg);
            else hipLaunchKernelGGL((mha_prefill_window_f16_kernel<D, false>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        } else {
            if (pg.table) hipLaunchKernelGGL((mha_prefill_window_kernel<D, true>), grid, block, 0, s, a, kv_lens, new_lens, pg);
            else hipLaunchKernelGGL((mha_prefill_window_kernel<D, false>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        }
        return;
    }
    if constexpr (sizeof(KV) == 2) {
        if (pg.table) hipLaunchKernelGGL((mha_prefill_f16_kernel<D, true, true>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        else if (kv_lens) hipLaunchKernelGGL((mha_prefill_f16_kernel<D, true, false>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        else hipLaunchKernelGGL((mha_prefill_f16_kernel<D, false, false>), grid, block, 0, s, a, nullptr, nullptr, pg);
    } else {
        if (pg.table) hipLaunchKernelGGL((mha_prefill_kernel<D, true, true>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        else if (kv_lens) hipLaunchKernelGGL((mha_prefill_kernel<D, true, false>), grid, block, 0, s, a, kv_lens, new_lens, pg);
        else hipLaunchKernelGGL((mha_prefill_kernel<D, false, false>), grid, block, 0, s, a, nullptr, nullptr, pg);
    }
}

int prefill_head_ok(const char *name, const npm_mha_decode *d) {
    if (!npm_mha_prefill_supported(d->head_dim))
        return npm::fail(NPM_E_UNSUPPORTED, "%s: head_dim %d is not supported (head_dim in {16, 32, 64, 128})", name, d->head_dim);
    return NPM_OK;
}

}  // namespace

extern "C" int npm_mha_prefill_supported(int head_dim) {
    return head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128;
}

extern "C" const char *npm_last_prefill_kernel(void) { return g_last; }

// npm_mha_prefill_fwd and npm_mha_prefill_fwd_f16: one host path.  KV = _Float16: d->k / d->v hold halves and their pitches and
// strides count halves (multiples of 8: 16 bytes); the same checks, grid and launch.  ``name``: the entry point, for the error texts.
// window > 0 (npm_mha_prefill_fwd_window; the entry point has checked it, d->causal and kv_lens): the windowed instances, same grid.
template <typename KV>
static int prefill_fwd(const char *name, const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                       const int32_t *block_table, int32_t table_pitch, int32_t page_rows, int32_t window = 0) {
    const bool varlen = kv_lens != nullptr, paged = block_table != nullptr;
    PageArgs pg{};
    if (int rc = check_kv_attn(name, d, varlen, block_table, table_pitch, page_rows, 16 / sizeof(KV), prefill_head_ok, &pg)) return rc;
    if (d->batch > 65535 || d->kv_heads > 65535)
        return npm::fail(NPM_E_BAD_ARGUMENT, "%s: bad argument: d->batch <= 65535 && d->kv_heads <= 65535", name);
    const int D = d->head_dim;

    PrefillArgs a{};
    a.q = d->q; a.k = d->k; a.v = d->v;
    a.q_pitch = d->q_pitch; a.k_pitch = d->k_pitch; a.k_sb = d->k_stride_b; a.v_pitch = d->v_pitch; a.v_sb = d->v_stride_b;
    a.ctx = d->ctx; a.ctx_pitch = d->ctx_pitch; a.lse = d->lse;
    a.heads = d->heads; a.kv_heads = d->kv_heads; a.tokens = d->new_tokens; a.len = d->kv_len; a.causal = d->causal != 0;
    a.group = d->heads / d->kv_heads;
    a.gb = std::min(a.group, ROWS);
    a.tb = ROWS / a.gb;
    a.head_chunks = (a.group + a.gb - 1) / a.gb;
    a.c = d->scale * LOG2E;
    a.scale = d->scale;
    a.window = window;
    const int64_t token_tiles = ((int64_t)d->new_tokens + a.tb - 1) / a.tb;
    if (token_tiles * a.head_chunks > 0x7fffffff)
        return npm::fail(NPM_E_BAD_ARGUMENT, "%s: bad argument: token_tiles * a.head_chunks <= 0x7fffffff", name);

    const dim3 grid((unsigned)(token_tiles * a.head_chunks), d->kv_heads, d->batch);
    hipStream_t s = npm::ctx().stream;
    switch (D) {
        case 16: launch_prefill<16, KV>(a, kv_lens, new_lens, pg, grid, s); break;
        case 32: launch_prefill<32, KV>(a, kv_lens, new_lens, pg, grid, s); break;
        case 64: launch_prefill<64, KV>(a, kv_lens, new_lens, pg, grid, s); break;
        default: launch_prefill<128, KV>(a, kv_lens, new_lens, pg, grid, s); break;
    }
    NPM_CHECK_LAUNCH();
    // the longest string, "mha_prefill_kernel D=128 T=2147483647 rows=64 causal=1 varlen=1 paged=1073741824 kv=f16", is 87 characters
    int at = snprintf(g_last, sizeof g_last, "mha_prefill_kernel D=%d T=%d rows=%d causal=%d%s", D, d->new_tokens, ROWS, a.causal,
                      varlen ? " varlen=1" : "");
    if (paged) at += snprintf(g_last + at, sizeof g_last - at, " paged=%d", page_rows);
    if (sizeof(KV) == 2) at += snprintf(g_last + at, sizeof g_last - at, " kv=f16");
    if (window > 0) snprintf(g_last + at, sizeof g_last - at, " window=%d", window);
    return NPM_OK;
}

extern "C" int npm_mha_prefill_fwd(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                   const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    return prefill_fwd<float>("npm_mha_prefill_fwd", d, kv_lens, new_lens, block_table, table_pitch, page_rows);
}

extern "C" int npm_mha_prefill_fwd_f16(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                       const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    return prefill_fwd<_Float16>("npm_mha_prefill_fwd_f16", d, kv_lens, new_lens, block_table, table_pitch, page_rows);
}

// Sliding-window attention over the per-sequence layouts (NULL block_table: the contiguous cache; kv_f16: halves).  The refusals of
// npm_mha_prefill_fwd[_f16], and: window < 1, a call that is not causal, NULL kv_lens.  A refused call launches nothing.
extern "C" int npm_mha_prefill_fwd_window(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                          const int32_t *block_table, int32_t table_pitch, int32_t page_rows, int32_t window,
                                          int32_t kv_f16) {
    const char *name = "npm_mha_prefill_fwd_window";
    if (!npm::ctx().ready) return npm::fail(NPM_E_NOT_INITIALIZED, "%s: npm_init() has not been called", name);
    if (window < 1) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: window %d is not >= 1", name, window);
    if (d == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: the descriptor is NULL", name);
    if (d->causal == 0) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: a window needs causal attention", name);
    if (kv_lens == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: kv_lens is NULL", name);
    if (kv_f16) return prefill_fwd<_Float16>(name, d, kv_lens, new_lens, block_table, table_pitch, page_rows, window);
    return prefill_fwd<float>(name, d, kv_lens, new_lens, block_table, table_pitch, page_rows, window);
}
