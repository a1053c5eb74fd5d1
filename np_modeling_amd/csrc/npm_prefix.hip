// Attention over a key / value prefix that every sequence of a batch shares (include/npm_hip.h: npm_mha_prefix_fwd,
// npm_attn_combine).  After PagedKVCache.fork the leading pages of several block-table rows are the SAME pages; the decode and
// prefill kernels would stream them once per sequence.  Here the prefix is read once for all of them:
//   * the R = B T query rows of ALL sequences are one list (the batch is folded into the token index: row tt = b T + t), and a
//     block covers 64 (head of the group, row) pairs of ONE K / V head c, as the prefill block does (npm_prefill_block.h): GB =
//     min(Hq / Hkv, 64) heads c + g Hkv and TB = 64 / GB consecutive rows.  Each wave owns 16 of the pairs for its whole key walk
//     and the four waves share every 16-key tile through LDS, double buffered, one barrier per tile.
//   * unlike the prefill kernel the KEYS are split over gridDim.z blocks, in contiguous ranges of whole tiles, because a decode
//     step brings few rows and a long prefix: grid = (row tiles, Hkv, splits).  Every (split, row, head) leaves a partial result,
//     ctx normalised within the split and the split's lse, and npm_attn_combine merges them in split order.  No atomics.
//   * every sequence sees the whole prefix: P is a multiple of page_rows (so of the tile), hence there are no lengths, no causal
//     arithmetic, no score is masked and no load is redirected.  The pages are those of ONE table row, one wave-uniform lookup per
//     tile.  A row with t >= new_lens[b] loads no q and stores nothing; a block without a live row returns before it loads a key.
//
// MFMA orientation, the raw running maximum and the exponent arithmetic are those of mha_prefill_kernel, operation for operation
// (see the head of npm_decode.hip): S^T = K Q^T with the query row on the lane, O^T += V^T P^T.  Exact fp32 MFMA, contraction
// off, every fma written out.  A row's partial depends on its own q, the keys of its split and the tile partition only, so a
// sequence in a batch is bitwise that sequence alone under the same split count.
//
// kv_f16: the pools hold halves; a 16-byte piece is 8 of them, converted exactly on the way into LDS, which then holds the fp32
// tiles of the fp32 instance: the call is bitwise the fp32 one on the rounded values.
//
// npm_attn_combine is the second half: per live row, the splits' partials in split order and then the result of the ordinary paged
// call over each sequence's own suffix, weighted by exp(lse_i - max lse).  One pass, 16 bytes per thread and access.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "npm_kvattn.h"

namespace {

constexpr int WAVES = 4;          // per block
constexpr int ROWS = WAVES * 16;  // (head, row) pairs per block
constexpr int MIN_TILES = 8;      // the automatic rule keeps at least this many tiles (128 keys) in a split

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

int g_splits = 0;                 // NPM_TUNE_PREFIX_SPLITS: 0 automatic, n > 0 forced
char g_last[128] = "";

struct PrefixArgs {
    const float *q, *k, *v;       // k, v: the page pools in their storage type KV (halves behind a float pointer for KV = _Float16)
    long q_pitch, k_pitch, k_sb, v_pitch, v_sb;   // k_ / v_: in elements of KV; _sb: the page stride
    float *part_ctx;              // [splits, B T, Hq, D]
    float *part_lse;              // [splits, B T, Hq]
    const int *table;             // the pages of the prefix, P / page_rows of them
    int shift;                    // log2 page_rows
    int heads, kv_heads, tokens, total;           // total = B T
    int group, gb, tb, head_chunks;               // Hq / Hkv; heads of the group and rows per block (gb tb <= ROWS); ceil(group / gb)
    int tiles, tiles_per_split;
    float c, scale;               // scale * log2(e), scale
};

template <int D, typename KV>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefix_kernel(const PrefixArgs a, const int *__restrict__ new_lens) {
#pragma clang fp contract(off)
    constexpr int KU = D / 16;                    // 16-byte K reads per lane and tile
    constexpr int VW = D >= 64 ? 4 : D / 16;      // floats per V read
    constexpr int DQ = D / (16 * VW);             // V reads per lane and key
    constexpr int NS = KU >= 4 ? 4 : KU;          // score accumulation chains
    constexpr int KP = D + 4;                     // LDS row pitch of K: lanes of one ds_read_b128 group land on distinct 16-byte slots
    constexpr int VP = D;                         //                of V: 16 lanes read one contiguous row
    constexpr int PW = 16 / sizeof(KV);           // elements of the pool in a 16-byte piece
    constexpr int F4 = TILE * D / PW;             // 16-byte pieces of one K (or V) tile in the pool
    constexpr int NLD = (F4 + WAVES * 64 - 1) / (WAVES * 64);   // ... per thread
    using VVec = typename VecOf<VW>::type;
    using Piece = typename PieceOf<KV>::type;
    __shared__ __attribute__((aligned(16))) float s_k[2][TILE][KP];
    __shared__ __attribute__((aligned(16))) float s_v[2][TILE][VP];

    const int c = blockIdx.y, split = blockIdx.z;
    const int tok0 = (int)(blockIdx.x / a.head_chunks) * a.tb, g0 = (int)(blockIdx.x % a.head_chunks) * a.gb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;

    // this lane's pair: row tok0 + r % tb of the folded list, head c + (g0 + r / tb) Hkv
    const int r = wave * 16 + n;
    const int tt = tok0 + r % a.tb, gi = g0 + r / a.tb;
    const int h = c + gi * a.kv_heads;
    const bool exists = r < a.gb * a.tb && gi < a.group && tt < a.total;
    const int b = exists ? tt / a.tokens : 0;
    const int t = tt - b * a.tokens;
    const bool live = exists && (new_lens == nullptr || t < new_lens[b]);
    if (!__syncthreads_or(live)) return;          // a tile of padding: nothing loaded, nothing stored
    const bool wave_live = __builtin_amdgcn_ballot_w64(live) != 0;

    f32x4v q[KU];
    {
        const float *src = a.q + (long)(live ? tt : 0) * a.q_pitch + (long)(live ? h : 0) * D + 4 * g;
#pragma unroll
        for (int u = 0; u < KU; ++u) q[u] = live ? *reinterpret_cast<const f32x4v *>(src + 16 * u) : f32x4v{0.f, 0.f, 0.f, 0.f};
    }

    f32x4v acc[DQ][VW];
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[dq][e] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const KV *kbase = reinterpret_cast<const KV *>(a.k) + (long)c * D;
    const KV *vbase = reinterpret_cast<const KV *>(a.v) + (long)c * D;
    const int first = split * a.tiles_per_split, last = min(first + a.tiles_per_split, a.tiles);

    // staging: piece i of a tile is columns PW (i % (D / PW)) .. + PW - 1 of key i / (D / PW), in flight in the storage type
    Piece kst[NLD], vst[NLD];
    auto load_tile = [&](int tile) {
        const int key0 = tile * TILE;
        // the page of the tile, a function of the tile index and kernel arguments only: wave-uniform, a scalar load
        const int page = a.table[__builtin_amdgcn_readfirstlane(key0) >> a.shift];
        const long koff = (long)page * a.k_sb, voff = (long)page * a.v_sb;
        const int in_page = (1 << a.shift) - 1;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int key = key0 + piece / (D / PW), col = (piece % (D / PW)) * PW;
                const long row = key & in_page;
                kst[i] = *reinterpret_cast<const Piece *>(kbase + koff + row * a.k_pitch + col);
                vst[i] = *reinterpret_cast<const Piece *>(vbase + voff + row * a.v_pitch + col);
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int row = piece / (D / PW), col = (piece % (D / PW)) * PW;
                if constexpr (PW == 4) {
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col]) = kst[i];
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col]) = vst[i];
                } else {
                    // halves -> fp32, exactly, as two 16-byte stores each
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col]) = __builtin_convertvector(__builtin_shufflevector(kst[i], kst[i], 0, 1, 2, 3), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col + 4]) = __builtin_convertvector(__builtin_shufflevector(kst[i], kst[i], 4, 5, 6, 7), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col]) = __builtin_convertvector(__builtin_shufflevector(vst[i], vst[i], 0, 1, 2, 3), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col + 4]) = __builtin_convertvector(__builtin_shufflevector(vst[i], vst[i], 4, 5, 6, 7), f32x4v);
                }
            }
        }
    };

    if (first < last) {
        load_tile(first);
        store_tile(first & 1);
    }
    __syncthreads();
    for (int tile = first; tile < last; ++tile) {
        const int buf = tile & 1;
        if (tile + 1 < last) load_tile(tile + 1);                     // in flight during the products below
        if (wave_live) {
            // S^T = K Q^T: NS independent accumulation chains, summed pairwise (as in mha_prefill_kernel)
            f32x4v sp[NS], s;
#pragma unroll
            for (int i = 0; i < NS; ++i) sp[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const f32x4v kr = *reinterpret_cast<const f32x4v *>(&s_k[buf][n][16 * u + 4 * g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sp[u % NS] = MFMA16(kr[e], q[u][e], sp[u % NS]);
            }
            s = NS == 4 ? (sp[0] + sp[1]) + (sp[2] + sp[3]) : NS == 2 ? sp[0] + sp[1] : sp[0];
            float tmax = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m, tmax);                       // raw
            const float ref = m_new * a.c;
            const float alpha = __builtin_amdgcn_exp2f(m * a.c - ref);    // the first tile: -inf * c = -inf: 0
            m = m_new;
            float psum = 0.f;
            f32x4v p;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                p[w] = __builtin_amdgcn_exp2f(fmaf(s[w], a.c, -ref));
                psum += p[w];
            }
            l = l * alpha + psum;
            // O^T += V^T P^T
#pragma unroll
            for (int dq = 0; dq < DQ; ++dq) {
                VVec va[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) va[w] = *reinterpret_cast<const VVec *>(&s_v[buf][4 * g + w][16 * VW * dq + VW * n]);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    f32x4v o = acc[dq][e] * alpha;
#pragma unroll
                    for (int w = 0; w < 4; ++w) o = MFMA16(comp<VW>(va[w], e), p[w], o);
                    acc[dq][e] = o;
                }
            }
        }
        // the other buffer was last read for tile - 1, before the barrier that ended that step
        if (tile + 1 < last) store_tile(buf ^ 1);
        __syncthreads();
    }

    // every wave stores its own live pairs: register w of acc[dq][e] is column d = 16 VW dq + VW (4 g + w) + e of pair n
    float lt = l;
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    if (!live) return;
    const bool none = m == -INFINITY;             // an empty split: 0 and -inf by selection, not 0 / 0
    const float rf = none ? 0.f : m * a.c;
    const long prow = ((long)split * a.total + tt) * a.heads + h;
    float *dst = a.part_ctx + prow * D;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            VVec o;
#pragma unroll
            for (int e = 0; e < VW; ++e) put<VW>(o, e, none ? 0.f : acc[dq][e][w] / lt);
            *reinterpret_cast<VVec *>(dst + 16 * VW * dq + VW * (4 * g + w)) = o;
        }
    if (g == 0) a.part_lse[prow] = none ? -INFINITY : fmaf(a.scale, m, (__builtin_amdgcn_logf(lt) + fmaf(-m, a.c, rf)) * LN2);
}

// One thread per (row of the folded list, head, four columns): the splits' partials in split order, then the suffix result that
// ctx / lse hold, merged in place.  A weight of a -inf lse is 0 by selection and its ctx is not read; a row with t >= new_lens[b]
// (and one nothing saw) is ctx = 0, lse = -inf by selection.  The D / 4 threads of a (row, head) are lanes of ONE wave (D / 4 divides
// 64), which has loaded the suffix lse in all of them before the d = 0 lane stores the merged one.
template <int D>
__global__ void __launch_bounds__(256)
attn_combine_kernel(const float *__restrict__ part_ctx, const float *__restrict__ part_lse, int splits, float *__restrict__ ctx,
                    long ctx_pitch, float *__restrict__ lse, int tokens, int heads, const int *__restrict__ new_lens, int store_lse,
                    long total) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % (D / 4)) * 4;
    const int h = (int)((i / (D / 4)) % heads);
    const long tt = i / ((long)(D / 4) * heads);
    const long rows = total / ((long)(D / 4) * heads);
    const long b = tt / tokens;
    const int t = (int)(tt - b * tokens);
    float *out = ctx + tt * ctx_pitch + (long)h * D + d;
    float *out_lse = lse + (b * heads + h) * tokens + t;
    const f32x4v zero{0.f, 0.f, 0.f, 0.f};
    if (new_lens && t >= new_lens[b]) {
        *reinterpret_cast<f32x4v *>(out) = zero;
        if (d == 0 && store_lse) *out_lse = -INFINITY;
        return;
    }
    const float ls = *out_lse;
    float mt = ls;
    for (int s = 0; s < splits; ++s) mt = fmaxf(mt, part_lse[((long)s * rows + tt) * heads + h]);
    if (mt == -INFINITY) {
        *reinterpret_cast<f32x4v *>(out) = zero;
        return;                                   // lse holds -inf already
    }
    float sum = 0.f;
    f32x4v o = zero;
    for (int s = 0; s < splits; ++s) {
        const long prow = ((long)s * rows + tt) * heads + h;
        const float lp = part_lse[prow];
        if (lp == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f((lp - mt) * LOG2E);
        sum += w;
        o += *reinterpret_cast<const f32x4v *>(part_ctx + prow * D + d) * w;
    }
    if (ls != -INFINITY) {
        const float w = __builtin_amdgcn_exp2f((ls - mt) * LOG2E);
        sum += w;
        o += *reinterpret_cast<const f32x4v *>(out) * w;
    }
    *reinterpret_cast<f32x4v *>(out) = o / sum;
    if (d == 0 && store_lse) *out_lse = mt + __builtin_amdgcn_logf(sum) * LN2;
}

int prefix_head_ok(const char *name, const npm_mha_decode *d) {
    if (!npm_mha_prefix_supported(d->head_dim))
        return npm::fail(NPM_E_UNSUPPORTED, "%s: head_dim %d is not supported (head_dim in {16, 32, 64, 128})", name, d->head_dim);
    return NPM_OK;
}

// the row tiles of `rows` folded rows: heads of the group and rows per block, head chunks, tiles
struct RowTiles {
    int group, gb, tb, head_chunks;
    long tiles;
};

RowTiles row_tiles(long rows, int heads, int kv_heads) {
    RowTiles r{};
    r.group = heads / kv_heads;
    r.gb = std::min(r.group, ROWS);
    r.tb = ROWS / r.gb;
    r.head_chunks = (r.group + r.gb - 1) / r.gb;
    r.tiles = (rows + r.tb - 1) / r.tb * r.head_chunks;
    return r;
}

template <typename KV>
void launch_prefix(int D, const PrefixArgs &a, const int *new_lens, dim3 grid, hipStream_t s) {
    const dim3 block(WAVES * 64);
    switch (D) {
        case 16: hipLaunchKernelGGL((mha_prefix_kernel<16, KV>), grid, block, 0, s, a, new_lens); break;
        case 32: hipLaunchKernelGGL((mha_prefix_kernel<32, KV>), grid, block, 0, s, a, new_lens); break;
        case 64: hipLaunchKernelGGL((mha_prefix_kernel<64, KV>), grid, block, 0, s, a, new_lens); break;
        default: hipLaunchKernelGGL((mha_prefix_kernel<128, KV>), grid, block, 0, s, a, new_lens); break;
    }
}

}  // namespace

extern "C" int npm_prefix_set_splits(int value) {
    if (value < 0 || value > NPM_PREFIX_MAX_SPLITS)
        return npm::fail(NPM_E_BAD_ARGUMENT, "npm_set_tuning: NPM_TUNE_PREFIX_SPLITS takes 0 .. %d", NPM_PREFIX_MAX_SPLITS);
    g_splits = value;
    return NPM_OK;
}

extern "C" int npm_mha_prefix_supported(int head_dim) { return head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128; }

extern "C" int npm_mha_prefix_splits(int rows, int heads, int kv_heads, int prefix_rows) {
    if (rows < 1 || heads < 1 || kv_heads < 1 || heads % kv_heads || prefix_rows < 1) return 1;
    if (g_splits > 0) return g_splits;
    // Fill the chip: about two blocks per compute unit of the 256, but never fewer than MIN_TILES tiles (128 keys: two rounds of
    // the double buffer per wave and barrier amortised) per split -- below that the partials cost more than the idle units.
    const long planes = row_tiles(rows, heads, kv_heads).tiles * kv_heads;
    const long want = (512 + planes - 1) / planes;
    const long by_len = std::max<long>(1, prefix_rows / (TILE * MIN_TILES));
    return (int)std::max<long>(1, std::min<long>(std::min(want, by_len), NPM_PREFIX_MAX_SPLITS));
}

extern "C" const char *npm_last_prefix_kernel(void) { return g_last; }

extern "C" int npm_mha_prefix_fwd(const npm_mha_decode *d, const int32_t *new_lens, const int32_t *prefix_table, int32_t page_rows,
                                  int32_t prefix_rows, int32_t splits, float *part_ctx, float *part_lse, int32_t kv_f16) {
    NPM_REQUIRE_INIT();
    NPM_ARG(d != nullptr);
    NPM_ARG(prefix_table != nullptr && page_shift(page_rows) >= 0);
    NPM_ARG(prefix_rows >= page_rows && prefix_rows % page_rows == 0);
    NPM_ARG(splits >= 1 && splits <= NPM_PREFIX_MAX_SPLITS && part_ctx != nullptr && part_lse != nullptr);
    NPM_ARG((int64_t)d->batch * d->new_tokens <= 0x7fffffff);
    // To the shared check this is the per-sequence call over prefix_rows keys that writes part_ctx: d->kv_len, d->causal, d->ctx and
    // d->lse are not read.  The table is one row and has been checked above, so the check sees none.
    npm_mha_decode p = *d;
    p.kv_len = prefix_rows; p.ctx = part_ctx; p.ctx_pitch = (int64_t)d->heads * d->head_dim;
    PageArgs none{};
    if (int rc = check_kv_attn("npm_mha_prefix_fwd", &p, true, nullptr, 0, 0, kv_f16 ? 8 : 4, prefix_head_ok, &none)) return rc;
    const int D = d->head_dim;
    NPM_ARG(d->k_stride_b >= (int64_t)page_rows * d->k_pitch && d->v_stride_b >= (int64_t)page_rows * d->v_pitch);
    NPM_ARG(d->kv_heads <= 65535);

    const RowTiles rt = row_tiles((long)d->batch * d->new_tokens, d->heads, d->kv_heads);
    NPM_ARG(rt.tiles <= 0x7fffffff);
    PrefixArgs a{};
    a.q = d->q; a.k = d->k; a.v = d->v;
    a.q_pitch = d->q_pitch; a.k_pitch = d->k_pitch; a.k_sb = d->k_stride_b; a.v_pitch = d->v_pitch; a.v_sb = d->v_stride_b;
    a.part_ctx = part_ctx; a.part_lse = part_lse;
    a.table = prefix_table; a.shift = page_shift(page_rows);
    a.heads = d->heads; a.kv_heads = d->kv_heads; a.tokens = d->new_tokens; a.total = d->batch * d->new_tokens;
    a.group = rt.group; a.gb = rt.gb; a.tb = rt.tb; a.head_chunks = rt.head_chunks;
    a.tiles = prefix_rows / TILE;
    a.tiles_per_split = (a.tiles + splits - 1) / splits;
    a.c = d->scale * LOG2E;
    a.scale = d->scale;

    const dim3 grid((unsigned)rt.tiles, d->kv_heads, splits);
    hipStream_t s = npm::ctx().stream;
    if (kv_f16) launch_prefix<_Float16>(D, a, new_lens, grid, s);
    else launch_prefix<float>(D, a, new_lens, grid, s);
    NPM_CHECK_LAUNCH();
    snprintf(g_last, sizeof g_last, "mha_prefix_kernel D=%d R=%d rows=%d prefix=%d splits=%d paged=%d%s", D, a.total, ROWS, prefix_rows,
             splits, page_rows, kv_f16 ? " kv=f16" : "");
    return NPM_OK;
}

extern "C" int npm_attn_combine(const float *part_ctx, const float *part_lse, int32_t splits, float *ctx, int64_t ctx_pitch, float *lse,
                                int32_t batch, int32_t new_tokens, int32_t heads, int32_t head_dim, const int32_t *new_lens,
                                int32_t store_lse) {
    NPM_REQUIRE_INIT();
    NPM_ARG(splits >= 1 && splits <= NPM_PREFIX_MAX_SPLITS && batch >= 1 && new_tokens >= 1 && heads >= 1);
    NPM_ARG(part_ctx != nullptr && part_lse != nullptr && ctx != nullptr && lse != nullptr);
    if (!npm_mha_prefix_supported(head_dim))
        return npm::fail(NPM_E_UNSUPPORTED, "npm_attn_combine: head_dim %d is not supported (head_dim in {16, 32, 64, 128})", head_dim);
    NPM_ARG(aligned16(part_ctx) && aligned16(ctx) && ctx_pitch % 4 == 0 && ctx_pitch >= (int64_t)heads * head_dim);
    const long total = (long)batch * new_tokens * heads * (head_dim / 4);
    NPM_ARG((total + 255) / 256 <= 0x7fffffff);
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    hipStream_t s = npm::ctx().stream;
#define NPM_COMBINE(DD) hipLaunchKernelGGL((attn_combine_kernel<DD>), grid, block, 0, s, part_ctx, part_lse, splits, ctx, (long)ctx_pitch, \
                                           lse, new_tokens, heads, new_lens, store_lse, total)
    switch (head_dim) {
        case 16: NPM_COMBINE(16); break;
        case 32: NPM_COMBINE(32); break;
        case 64: NPM_COMBINE(64); break;
        default: NPM_COMBINE(128); break;
    }
#undef NPM_COMBINE
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}
