// Incremental decoding: attention of T new query tokens over a key / value cache, and the append into that cache
// (include/npm_hip.h: npm_mha_decode_fwd, npm_kv_append), and their forms with one length per sequence for ragged batches
// (npm_mha_decode_fwd_varlen, npm_kv_append_varlen, npm_kv_gather_varlen), and the forms of those over a PAGED cache
// (npm_mha_decode_fwd_paged, npm_kv_append_paged, npm_kv_gather_paged): K / V rows live in a pool of pages of page_rows rows each
// and a per-sequence block table names the page of every page_rows logical rows.  Inference only: nothing is saved for a backward.
//
//   ctx[b, t, h, :] = sum_j softmax_j(scale q[b, t, h, :] . K[b, j, h % Hkv, :]) V[b, j, h % Hkv, :]
//   j < L (causal = 0)    j <= L - T + t (causal = 1: the T new tokens are the last T keys of the cache)
//
// The work is one pass over K and V, so the kernel is shaped around that stream:
//   * ONE block serves a whole grouped-query group: the rows of its score tile are the R = (Hq / Hkv) T pairs (query head of the
//     group, new token) that share K / V head c -- heads c, c + Hkv, c + 2 Hkv, ... (the project's h % Hkv mapping) -- so K and
//     V of that head are read once per (batch, K / V head, key range), not once per query head.
//   * the keys are SPLIT over gridDim.x blocks so that small B Hkv still fills the chip; each split leaves (m, l, acc[D]) per row
//     (largest raw score, sum, unnormalised accumulator) in pooled scratch and mha_decode_combine_kernel merges the
//     splits of a row in split order: no atomics, bitwise reproducible.  One split: the kernel writes ctx itself.
//   * inside a block the four waves take the 16-key tiles of the split's range round robin and merge through LDS, wave 0 first.
//
// MFMA orientation (v_mfma_f32_16x16x4_f32: lane l supplies A[m = l & 15][k = l >> 4] and B[k = l >> 4][n = l & 15]; register w of
// the result is row m = 4 (l >> 4) + w, column n = l & 15).  As in the training forward the QUERY ROW is on the lane:
//   S^T[key, row] = K Q^T       A = K (key j = l & 15), B = Q (row i = l & 15).  The contraction index is permuted so that a
//                               lane's K operand is one 16-byte load: step (u, e) contracts d = 16 u + 4 (l >> 4) + e.
//   O^T[d, row] += V^T P^T      P^T is, register for register, the B operand: register w of S^T holds key 4 (l >> 4) + w, so step w
//                               contracts keys {4 g + w}, and A = V[key 4 (l >> 4) + w][d]: lane c = l & 15 loads VW = min(4, D / 16)
//                               consecutive floats at d = 16 VW dq + VW c; component e of that load feeds output block (dq, e),
//                               whose row m is d = 16 VW dq + VW m + e.  (D = 16 / 32 have fewer than 64 floats per key, so there
//                               V moves 4 / 8 bytes per lane; K always moves 16.)
// Row statistics are lane-local but for one exchange across the four 16-lane groups; the running sum stays a per-lane partial
// (every lane of a row applies the same rescale) and is reduced once at the end.
//
// Nothing past the valid length enters a result: a key at or past L, or one a causal row may not see, gets score -inf by
// SELECTION (never by arithmetic on what was loaded); loads of such keys are redirected to key L - 1 (in bounds whatever the
// capacity) and V of keys >= L is zeroed, which only the last tile of a call pays for; a row (or a whole split) without a
// visible key has m = -inf, l = 0 and is given weight 0 by comparing, not by exp(-inf - -inf).
//
// The running maximum is kept as the RAW score s_max (before the scale): the reference point of the exponents is m = s_max c
// (c = scale log2(e); rounding is monotone, so that is the largest scaled score), and lse = scale s_max + ln(2) log2(l) takes one
// rounding of a large number instead of the three of ln(2) (s_max c + log2(l)).  Every exponent is fma(s, c, -m) with the ROUNDED
// m = fl(s_max c) (so the sums l are relative to m exactly, and merging waves and splits, exp2(m_a - m_b), is consistent); the
// rounding of m itself, delta = m - s_max c, is recovered exactly by one fma and added to log2(l).  Floating-point contraction
// is off in these kernels: each fma is written out.
//
// Paged (PG): page_rows is a power of two >= TILE, so a 16-key tile never straddles a page and the redirect to key L - 1 stays in
// the tile's own page (a loaded tile holds a key < L: key0 <= L - 1 < key0 + 16).  Paging is then ONE wave-uniform table lookup per
// tile (a scalar load) in front of the same address arithmetic; the source asks for a tile's page one loop step before the loads
// that need it (the compiler schedules the scalar load next to those loads all the same: DESIGN.md 4.5b has the measured cost).
// The table index is clamped to the page of key L - 1: entries past a sequence's
// last page are not even read.  Split partition, online softmax, wave merge and the combine kernel do not know about pages, so a
// paged call is bitwise the varlen call on a contiguous cache of the same rows.
//
// Row copies (the appends into a cache, the gathers out of one): two kernel templates, kv_append_kernel<VL, PG> and
// kv_gather_kernel<PG>, over ONE description of where the rows of a cache live (RowLayout, by value) and one device helper,
// row_of<PG>(layout, b, j), that turns (sequence, logical row) into an address -- base + b * stride + j * pitch, or through the
// block table pool + table[b * table_pitch + (j >> shift)] * page_stride + (j & mask) * pitch.  The flags keep the five entry
// points' code apart: the uniform append reads the scalar `at` and loads no length, the ragged and paged ones read at_lens[b] and
// skip t >= new_lens[b], a gather writes zeros for j >= lens[b] and reads neither that row nor its table entry.  One host
// function, row_copy, holds what the entry points share (checks, grid, launch); each entry point is its own preconditions -- the
// paged ones refuse a NULL length array or table even when there is nothing to copy -- and one call.
//
// Half-precision cache (npm_kv_append_f16, npm_kv_gather_f16, npm_mha_decode_fwd_f16): the storage type of the cache rows is a
// template parameter KV of the three kernel templates, float (the instances above, unchanged) or _Float16.  K / V rows are rounded
// once, by the append (round to nearest even, the hardware's v_cvt_f16_f32: bit for bit NumPy's astype(float16), subnormal results
// included; |x| >= 65520 becomes +-inf, there is no clamp), and converted back exactly by the loads of load_tile and of the gather.
// Pitches and strides of an fp16 cache count halves.  The assignment of head-dimension indices to lanes is the fp32 one -- a
// lane's K load is the 4 consecutive halves (8 bytes) of the 4 floats it loaded before, its V load VW halves -- so every
// floating-point operation after the load is that of the fp32 instance on the converted values: the result is BITWISE that of
// the fp32 call on a cache holding the rounded values.  Everything else (q, scores, softmax, accumulators, ctx, lse) stays fp32.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "npm_kvattn.h"

namespace {

constexpr int WAVES = 4;          // per block; TILE (npm_kvattn.h): keys per wave tile

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

int g_splits = 0;                 // NPM_TUNE_DECODE_SPLITS: 0 automatic, n > 0 forced
int g_nt = 0;                     // NPM_TUNE_DECODE_NT: 0 by size (npm::stream_nt_enabled of the valid K bytes), 1 always, 2 never
char g_last[128] = "";

struct DecodeArgs {
    const float *q, *k, *v;       // k, v: the cache in its storage type KV (halves behind a float pointer for KV = _Float16)
    long q_pitch, k_pitch, k_sb, v_pitch, v_sb;   // k_ / v_: in elements of KV
    float *ctx;
    long ctx_pitch;
    float *lse;                   // optional [B, Hq, T]
    float *part_ml;               // splits > 1: [B, Hkv, splits, RP, 2]: largest raw score, sum
    float *part_acc;              //             [B, Hkv, splits, RP, D]
    int heads, kv_heads, tokens, len, causal, rows, tiles_per_split;
    float c, scale;               // scale * log2(e), scale
    int window;                   // npm_mha_decode_fwd_window: keys a row sees, itself included (read by the WN instances only)
};

template <bool NT, typename V>
__device__ __forceinline__ V ld_kv(const float *p) {
    if (NT) return __builtin_nontemporal_load(reinterpret_cast<const V *>(p));
    return *reinterpret_cast<const V *>(p);
}

// The same elements out of an fp16 cache: one load of as many halves, converted exactly (v_cvt_f32_f16; subnormals are kept)
template <bool NT, typename V>
__device__ __forceinline__ V ld_kv(const _Float16 *p) {
    constexpr int VW = sizeof(V) / sizeof(float);
    using H = typename HalfVecOf<VW>::type;
    H h;
    if (NT) h = __builtin_nontemporal_load(reinterpret_cast<const H *>(p));
    else h = *reinterpret_cast<const H *>(p);
    if constexpr (VW == 1) return (float)h;
    else return __builtin_convertvector(h, V);
}

// D: head size; RB: 16-row blocks of the score tile (rows = (Hq / Hkv) T <= 16 RB); NT: nontemporal K / V loads.
// VL (npm_mha_decode_fwd_varlen): the sequence has L = kv_lens[b] <= a.len valid keys and nb = new_lens[b] <= a.tokens new tokens.
// The tile partition stays that of a.len, so a sequence with L == a.len and nb == a.tokens computes, operation for operation, what
// the VL = false instance computes; a block whose key range starts at or past L leaves an empty partial and returns before it
// loads anything; a row without a visible key (a padded token, L = 0) is stored as ctx = 0, lse = -inf by selection.
// PG (npm_mha_decode_fwd_paged, implies VL): a.k / a.v are page pools, a.k_sb / a.v_sb the page strides, pg the block table.
// KV: the storage type of the cache, float or _Float16 (npm_mha_decode_fwd_f16); only the loads of load_tile know it.
template <int D, int RB, bool NT, bool VL, bool PG, typename KV = float>
__global__ void __launch_bounds__(WAVES * 64)
mha_decode_kernel(const DecodeArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    constexpr bool WN = false;
#include "npm_decode_block.h"
}

// Sliding-window attention (npm_mha_decode_fwd_window): the same body with WN on, for the per-sequence layouts only (VL).  Row t of
// sequence b sees keys max(0, limit - a.window) <= j < limit; the walk starts at the sequence's first live tile
// lo = max(0, L - nb + 1 - a.window) / 16 and a.tiles_per_split partitions the tiles FROM THERE (the host sizes it for the most
// tiles min(a.len, window + T - 1) keys can touch).  A key below a row's floor gets -inf by selection, V rows below the smallest
// floor of the sequence are zeroed by selection, tiles below lo are not loaded and their table entries not read.  A kernel name
// of its own: the instances above keep theirs, symbol for symbol.
template <int D, int RB, bool NT, bool PG, typename KV>
__global__ void __launch_bounds__(WAVES * 64)
mha_decode_window_kernel(const DecodeArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    constexpr bool VL = true, WN = true;
#include "npm_decode_block.h"
}

// One thread per (batch, K / V head, row, four columns): the splits of the row merged in split order.
// VL: a row none of whose splits saw a key (a padded token, a sequence without keys) is ctx = 0, lse = -inf by selection.
template <int D, bool VL = false>
__global__ void __launch_bounds__(256)
mha_decode_combine_kernel(const float *__restrict__ part_ml, const float *__restrict__ part_acc, float *__restrict__ ctx,
                          long ctx_pitch, float *__restrict__ lse, int batch, int heads, int kv_heads, int tokens, int rows,
                          int rows_pad, int splits, float c2, float scale) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)batch * kv_heads * rows * (D / 4);
    if (i >= total) return;
    const int d = (int)(i % (D / 4)) * 4;
    const int r = (int)((i / (D / 4)) % rows);
    const long plane = i / ((long)(D / 4) * rows);                    // b * kv_heads + c
    const int c = (int)(plane % kv_heads);
    const long b = plane / kv_heads;
    const long first = plane * splits * rows_pad + r;
    float mt = -INFINITY;
    for (int s = 0; s < splits; ++s) mt = fmaxf(mt, part_ml[2 * (first + (long)s * rows_pad)]);
    float lt = 0.f;
    f32x4v o{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < splits; ++s) {
        const long prow = first + (long)s * rows_pad;
        const float ms = part_ml[2 * prow];
        if (ms == -INFINITY) continue;                                // a split without a visible key: weight 0, its acc is not read
        const float w = __builtin_amdgcn_exp2f(ms * c2 - mt * c2);
        lt += part_ml[2 * prow + 1] * w;
        o += *reinterpret_cast<const f32x4v *>(part_acc + prow * D + d) * w;
    }
    const int t = r % tokens, h = c + (r / tokens) * kv_heads;
    const bool none = VL && mt == -INFINITY;
    *reinterpret_cast<f32x4v *>(ctx + (b * tokens + t) * ctx_pitch + (long)h * D + d) = none ? f32x4v{0.f, 0.f, 0.f, 0.f} : o / lt;
    if (d == 0 && lse)
        lse[(b * heads + h) * tokens + t] = none ? -INFINITY : fmaf(scale, mt, (__builtin_amdgcn_logf(lt) + fmaf(-mt, c2, mt * c2)) * LN2);
}

// ---- row copies: the appends into a cache and the gathers out of one ------------------------------------------------------------
// Where the rows of a cache live.  Contiguous (table == nullptr): row j of sequence b is base + b * stride + j * pitch.  Paged:
// base is the page pool, stride the page stride and the row is row j & (page_rows - 1) of page table[b * table_pitch + (j >> shift)].
struct RowLayout {
    float *base;                  // an fp16 cache: halves behind the float pointer; pitch and stride count elements of the cache
    long pitch, stride;
    const int *table;
    int table_pitch, shift;
};

template <bool PG, typename KV = float>
__device__ __forceinline__ KV *row_of(const RowLayout &c, long b, int j) {
    KV *base = reinterpret_cast<KV *>(c.base);
    if (PG) return base + (long)c.table[b * c.table_pitch + (j >> c.shift)] * c.stride + (long)(j & ((1 << c.shift) - 1)) * c.pitch;
    return base + b * c.stride + (long)j * c.pitch;
}

// 16 bytes of the cache per thread and step: 4 floats, or 8 halves (then two 16-byte accesses on the fp32 side)
template <typename KV> struct RowVec { static constexpr int W = 4; };
template <> struct RowVec<_Float16> { static constexpr int W = 8; };

// row (at + t) of sequence b = src[b * T + t, :row_len], 16 bytes per thread and step.  VL = false (npm_kv_append): at is the scalar
// and no length is loaded.  VL: at = at_lens[b], and only t < new_lens[b] (NULL: every t) is written; other rows are not touched.
// KV = _Float16 (npm_kv_append_f16): the destination holds halves, rounded to nearest even here (row4: 8-column steps per row).
template <bool VL, bool PG, typename KV = float>
__global__ void __launch_bounds__(256)
kv_append_kernel(const float *__restrict__ src, long src_pitch, const RowLayout dst, int tokens, int row4, int at,
                 const int *__restrict__ at_lens, const int *__restrict__ new_lens, long total) {
    static_assert(VL || !PG, "a paged cache has per-sequence lengths");
    constexpr int W = RowVec<KV>::W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % row4) * W;
        const long row = i / row4;
        const long b = row / tokens;
        const int t = (int)(row - b * tokens);
        if (VL && new_lens && t >= new_lens[b]) continue;
        KV *to = row_of<PG, KV>(dst, b, (VL ? at_lens[b] : at) + t) + col;
        const float *from = src + row * src_pitch + col;
        if constexpr (W == 4) {
            *reinterpret_cast<f32x4v *>(to) = *reinterpret_cast<const f32x4v *>(from);
        } else {
            const f16x4v lo = __builtin_convertvector(*reinterpret_cast<const f32x4v *>(from), f16x4v);
            const f16x4v hi = __builtin_convertvector(*reinterpret_cast<const f32x4v *>(from + 4), f16x4v);
            *reinterpret_cast<f16x8v *>(to) = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    }
}

// out[b, j, :row_len] = j < lens[b] ? row j of sequence b : 0 for j < rows; out is [B, rows, row_len], contiguous.  Neither a row at
// or past lens[b] nor its table entry is read.
// KV = _Float16 (npm_kv_gather_f16): the source holds halves, converted exactly (row4: 8-column steps per row).
template <bool PG, typename KV = float>
__global__ void __launch_bounds__(256)
kv_gather_kernel(const RowLayout src, float *__restrict__ out, int rows, int row4, const int *__restrict__ lens, long total) {
    constexpr int W = RowVec<KV>::W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int col = (int)(i % row4) * W;
        const long row = i / row4;
        const long b = row / rows;
        const int j = (int)(row - b * rows);
        if constexpr (W == 4) {
            f32x4v x{0.f, 0.f, 0.f, 0.f};
            if (j < lens[b]) x = *reinterpret_cast<const f32x4v *>(row_of<PG, KV>(src, b, j) + col);
            *reinterpret_cast<f32x4v *>(out + row * (4L * row4) + col) = x;
        } else {
            f16x8v h = f16x8v((_Float16)0.f);
            if (j < lens[b]) h = *reinterpret_cast<const f16x8v *>(row_of<PG, KV>(src, b, j) + col);
            float *to = out + row * ((long)W * row4) + col;
            *reinterpret_cast<f32x4v *>(to) = __builtin_convertvector(__builtin_shufflevector(h, h, 0, 1, 2, 3), f32x4v);
            *reinterpret_cast<f32x4v *>(to + 4) = __builtin_convertvector(__builtin_shufflevector(h, h, 4, 5, 6, 7), f32x4v);
        }
    }
}

// Copy-on-write of a paged cache (npm_kv_copy_pages): the first rows[i] rows of page src_pages[i] become those of page
// dst_pages[i], for all n pairs in one launch.  Bytes, 16 at a time, so one kernel serves f32 and f16 pools: the rows of a page
// are contiguous, row16 such pieces each, and a page lies page16 pieces from the next.  blockIdx.y walks the pairs, blockIdx.x the
// rows[i] * row16 pieces of one; pieces at and past that (the rows at and past rows[i] of the destination) are not written.
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256)
kv_copy_pages_kernel(u32x4v *__restrict__ pool, long page16, long row16, const int *__restrict__ src_pages,
                     const int *__restrict__ dst_pages, const int *__restrict__ rows, int n) {
    for (int pair = blockIdx.y; pair < n; pair += gridDim.y) {
        const long pieces = (long)rows[pair] * row16;
        const u32x4v *from = pool + src_pages[pair] * page16;
        u32x4v *to = pool + dst_pages[pair] * page16;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += (long)gridDim.x * blockDim.x) to[i] = from[i];
    }
}

// npm_kv_copy_pages_planes: the copy above with a plane index on the grid.  A layered cache keeps the K and V pools of all its
// layers in one allocation, plane16 pieces apart, with ONE block table: the same (src, dst, rows) pairs are copied in every plane.
// blockIdx.z walks the planes, the rest is kv_copy_pages_kernel.
__global__ void __launch_bounds__(256)
kv_copy_pages_planes_kernel(u32x4v *__restrict__ pool, long page16, long row16, const int *__restrict__ src_pages,
                            const int *__restrict__ dst_pages, const int *__restrict__ rows, int n, int planes, long plane16) {
    for (int plane = blockIdx.z; plane < planes; plane += gridDim.z) {
        u32x4v *base = pool + plane * plane16;
        for (int pair = blockIdx.y; pair < n; pair += gridDim.y) {
            const long pieces = (long)rows[pair] * row16;
            const u32x4v *from = base + src_pages[pair] * page16;
            u32x4v *to = base + dst_pages[pair] * page16;
            for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += (long)gridDim.x * blockDim.x) to[i] = from[i];
        }
    }
}

// VL = false (npm_mha_decode_fwd): the instances that never look at the length arrays; PG: the ones that read through a block table
template <int D, int RB, bool VL, bool PG, typename KV>
void launch_decode(const DecodeArgs &a, const int *kv_lens, const int *new_lens, const PageArgs &pg, dim3 grid, bool nt, hipStream_t s) {
    if (nt) hipLaunchKernelGGL((mha_decode_kernel<D, RB, true, VL, PG, KV>), grid, dim3(WAVES * 64), 0, s, a, kv_lens, new_lens, pg);
    else hipLaunchKernelGGL((mha_decode_kernel<D, RB, false, VL, PG, KV>), grid, dim3(WAVES * 64), 0, s, a, kv_lens, new_lens, pg);
}

template <int D, typename KV>
void launch_decode_rb(const DecodeArgs &a, const int *kv_lens, const int *new_lens, const PageArgs &pg, dim3 grid, int rb, bool nt,
                      hipStream_t s) {
    if (pg.table) {
        if (rb == 1) launch_decode<D, 1, true, true, KV>(a, kv_lens, new_lens, pg, grid, nt, s);
        else launch_decode<D, 2, true, true, KV>(a, kv_lens, new_lens, pg, grid, nt, s);
    } else if (kv_lens) {
        if (rb == 1) launch_decode<D, 1, true, false, KV>(a, kv_lens, new_lens, pg, grid, nt, s);
        else launch_decode<D, 2, true, false, KV>(a, kv_lens, new_lens, pg, grid, nt, s);
    } else if (rb == 1) launch_decode<D, 1, false, false, KV>(a, nullptr, nullptr, pg, grid, nt, s);
    else launch_decode<D, 2, false, false, KV>(a, nullptr, nullptr, pg, grid, nt, s);
}

template <int D, typename KV>
void launch_decode_window(const DecodeArgs &a, const int *kv_lens, const int *new_lens, const PageArgs &pg, dim3 grid, int rb, bool nt,
                          hipStream_t s) {
    const dim3 block(WAVES * 64);
#define NPM_WINDOW(RB, NT, PG) hipLaunchKernelGGL((mha_decode_window_kernel<D, RB, NT, PG, KV>), grid, block, 0, s, a, kv_lens, new_lens, pg)
#define NPM_WINDOW_NT(RB, PG) do { if (nt) NPM_WINDOW(RB, true, PG); else NPM_WINDOW(RB, false, PG); } while (0)
    if (pg.table) {
        if (rb == 1) NPM_WINDOW_NT(1, true); else NPM_WINDOW_NT(2, true);
    } else {
        if (rb == 1) NPM_WINDOW_NT(1, false); else NPM_WINDOW_NT(2, false);
    }
#undef NPM_WINDOW_NT
#undef NPM_WINDOW
}

// The keys one sequence of a windowed call can hold live: its T rows see at most window + T - 1 of them, and never more than kv_len
long window_keys(long kv_len, long tokens, long window) { return std::min(kv_len, window + tokens - 1); }

// The decode kernel's own rule: the head size and the rows of a score tile
int decode_head_ok(const char *name, const npm_mha_decode *d) {
    const int rows = d->heads / d->kv_heads * d->new_tokens;
    if (!npm_mha_decode_supported(d->head_dim, rows))
        return npm::fail(NPM_E_UNSUPPORTED, "%s: head_dim %d with %d rows per K / V head is not supported "
                         "(head_dim in {16, 32, 64, 128}, rows <= %d)", name, d->head_dim, rows, NPM_DECODE_MAX_ROWS);
    return NPM_OK;
}

}  // namespace

extern "C" int npm_decode_set_splits(int value) {
    if (value < 0 || value > NPM_DECODE_MAX_SPLITS)
        return npm::fail(NPM_E_BAD_ARGUMENT, "npm_set_tuning: NPM_TUNE_DECODE_SPLITS takes 0 .. %d", NPM_DECODE_MAX_SPLITS);
    g_splits = value;
    return NPM_OK;
}

extern "C" int npm_decode_set_nt(int value) {
    if (value < 0 || value > 2) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_set_tuning: NPM_TUNE_DECODE_NT takes 0, 1 or 2");
    g_nt = value;
    return NPM_OK;
}

extern "C" int npm_mha_decode_supported(int head_dim, int group_rows) {
    const bool dim_ok = head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128;
    return dim_ok && group_rows >= 1 && group_rows <= NPM_DECODE_MAX_ROWS;
}

extern "C" int npm_mha_decode_splits(int batch, int kv_heads, int kv_len) {
    if (batch < 1 || kv_heads < 1 || kv_len < 1) return 1;
    if (g_splits > 0) return g_splits;
    // Fill the chip: about two blocks per compute unit of the 256, but never fewer than 256 keys (16 tiles, four per wave) per
    // split -- below that the partials and the second launch cost more than the idle units.  Shape arguments only.
    const long planes = (long)batch * kv_heads;
    const long want = (512 + planes - 1) / planes;
    const long by_len = std::max<long>(1, kv_len / 256);
    return (int)std::max<long>(1, std::min<long>(std::min(want, by_len), NPM_DECODE_MAX_SPLITS));
}

extern "C" int npm_mha_decode_window_splits(int batch, int kv_heads, int kv_len, int new_tokens, int window) {
    if (kv_len < 1 || new_tokens < 1 || window < 1) return 1;
    return npm_mha_decode_splits(batch, kv_heads, (int)window_keys(kv_len, new_tokens, window));
}

extern "C" const char *npm_last_decode_kernel(void) { return g_last; }

// npm_mha_decode_fwd (kv_lens == nullptr), npm_mha_decode_fwd_varlen and npm_mha_decode_fwd_paged (block_table != nullptr): one
// host path, so that the split count, the tile partition and the load policy of a varlen or paged call are those of the uniform
// call at d->kv_len.  KV = _Float16 (npm_mha_decode_fwd_f16): d->k / d->v hold halves and their pitches and strides count halves
// (multiples of 8: 16 bytes); the same checks, split count and partition, and the load policy on the BYTES of the valid part of K.
// window > 0 (npm_mha_decode_fwd_window; the entry point has checked it, d->causal and kv_lens): split count, partition, scratch,
// grid and load policy follow keys_bound = min(kv_len, window + T - 1) -- kv_len itself under a covering window, so that call is
// the unwindowed one operation for operation.
template <typename KV = float>
static int decode_fwd(const char *name, const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                      const int32_t *block_table = nullptr, int32_t table_pitch = 0, int32_t page_rows = 0, int32_t window = 0) {
    const bool varlen = kv_lens != nullptr, paged = block_table != nullptr;
    PageArgs pg{};
    if (int rc = check_kv_attn(name, d, varlen, block_table, table_pitch, page_rows, 16 / sizeof(KV), decode_head_ok, &pg)) return rc;
    if (d->batch > 65535 || d->kv_heads > 65535)
        return npm::fail(NPM_E_BAD_ARGUMENT, "%s: bad argument: d->batch <= 65535 && d->kv_heads <= 65535", name);
    const int D = d->head_dim, rows = d->heads / d->kv_heads * d->new_tokens;

    // window: an interval of keys_bound keys touches at most (keys_bound + 14) / 16 + 1 tiles wherever it starts, and no more than
    // the cache has
    const int keys_bound = window > 0 ? (int)window_keys(d->kv_len, d->new_tokens, window) : d->kv_len;
    const int tiles = window > 0 ? std::min((d->kv_len + TILE - 1) / TILE, (keys_bound + TILE - 2) / TILE + 1) : (d->kv_len + TILE - 1) / TILE;
    const int splits = npm_mha_decode_splits(d->batch, d->kv_heads, keys_bound);
    const int rb = rows > 16 ? 2 : 1;
    DecodeArgs a{};
    a.q = d->q; a.k = d->k; a.v = d->v;
    a.q_pitch = d->q_pitch; a.k_pitch = d->k_pitch; a.k_sb = d->k_stride_b; a.v_pitch = d->v_pitch; a.v_sb = d->v_stride_b;
    a.ctx = d->ctx; a.ctx_pitch = d->ctx_pitch; a.lse = d->lse;
    a.heads = d->heads; a.kv_heads = d->kv_heads; a.tokens = d->new_tokens; a.len = d->kv_len; a.causal = d->causal != 0;
    a.rows = rows;
    a.tiles_per_split = (tiles + splits - 1) / splits;
    a.c = d->scale * LOG2E;
    a.scale = d->scale;
    a.window = window;

    hipStream_t s = npm::ctx().stream;
    npm::Scratch ml, acc;
    const long prow = (long)d->batch * d->kv_heads * splits * rb * 16;
    if (splits > 1) {
        if (int rc = ml.alloc(sizeof(float) * 2 * prow)) return rc;
        if (int rc = acc.alloc(sizeof(float) * prow * D)) return rc;
        a.part_ml = static_cast<float *>(ml.ptr);
        a.part_acc = static_cast<float *>(acc.ptr);
    }
    const dim3 grid(splits, d->kv_heads, d->batch);
    // Each K / V byte is read once by one block.  Measured (tools/decode_bench.py, profiles/r08_decode_bench.log): from 64 MB of
    // K + V up the nontemporal hint is 3 - 13 % faster (the stream does not displace itself in the L2s and the Infinity Cache);
    // below that plain loads are 0 - 3 % faster.  The project's rule for streaming tensors (32 MB each) draws the same line.
    const bool nt = g_nt == 1 || (g_nt == 0 && npm::stream_nt_enabled(sizeof(KV) * (size_t)d->batch * keys_bound * d->kv_heads * D));
    if (window > 0) {
        switch (D) {
            case 16: launch_decode_window<16, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            case 32: launch_decode_window<32, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            case 64: launch_decode_window<64, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            default: launch_decode_window<128, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
        }
    } else {
        switch (D) {
            case 16: launch_decode_rb<16, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            case 32: launch_decode_rb<32, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            case 64: launch_decode_rb<64, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
            default: launch_decode_rb<128, KV>(a, kv_lens, new_lens, pg, grid, rb, nt, s); break;
        }
    }
    NPM_CHECK_LAUNCH();
    if (splits > 1) {
        const long total = (long)d->batch * d->kv_heads * rows * (D / 4);
        const dim3 cgrid((unsigned)((total + 255) / 256));
#define NPM_COMBINE_VL(DD, VL) hipLaunchKernelGGL((mha_decode_combine_kernel<DD, VL>), cgrid, dim3(256), 0, s, a.part_ml, a.part_acc, \
                                                  a.ctx, a.ctx_pitch, a.lse, d->batch, d->heads, d->kv_heads, d->new_tokens, rows, rb * 16, \
                                                  splits, a.c, a.scale)
#define NPM_COMBINE(DD) do { if (varlen) NPM_COMBINE_VL(DD, true); else NPM_COMBINE_VL(DD, false); } while (0)
        switch (D) {
            case 16: NPM_COMBINE(16); break;
            case 32: NPM_COMBINE(32); break;
            case 64: NPM_COMBINE(64); break;
            default: NPM_COMBINE(128); break;
        }
#undef NPM_COMBINE
#undef NPM_COMBINE_VL
        NPM_CHECK_LAUNCH();
    }
    int at = snprintf(g_last, sizeof g_last, "mha_decode_kernel D=%d rows=%d splits=%d causal=%d%s", D, rows, splits, a.causal,
                      varlen ? " varlen=1" : "");
    if (paged) at += snprintf(g_last + at, sizeof g_last - at, " paged=%d", page_rows);
    if (sizeof(KV) == 2) at += snprintf(g_last + at, sizeof g_last - at, " kv=f16");
    if (window > 0) snprintf(g_last + at, sizeof g_last - at, " window=%d", window);
    return NPM_OK;
}

extern "C" int npm_mha_decode_fwd(const npm_mha_decode *d) { return decode_fwd("npm_mha_decode_fwd", d, nullptr, nullptr); }

extern "C" int npm_mha_decode_fwd_varlen(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens) {
    if (kv_lens == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_varlen: kv_lens is NULL");
    return decode_fwd("npm_mha_decode_fwd_varlen", d, kv_lens, new_lens);
}

extern "C" int npm_mha_decode_fwd_paged(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                        const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    if (kv_lens == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_paged: kv_lens is NULL");
    if (block_table == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_paged: block_table is NULL");
    if (page_shift(page_rows) < 0)
        return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_paged: page_rows %d is not a power of two >= %d", page_rows, TILE);
    return decode_fwd("npm_mha_decode_fwd_paged", d, kv_lens, new_lens, block_table, table_pitch, page_rows);
}

// The three layouts over an fp16 cache: NULL kv_lens is npm_mha_decode_fwd, NULL block_table npm_mha_decode_fwd_varlen, else
// npm_mha_decode_fwd_paged -- with the refusals of that entry point.
extern "C" int npm_mha_decode_fwd_f16(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                      const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    if (block_table != nullptr) {
        if (kv_lens == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_f16: a block table needs kv_lens");
        if (page_shift(page_rows) < 0)
            return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_decode_fwd_f16: page_rows %d is not a power of two >= %d", page_rows, TILE);
    }
    return decode_fwd<_Float16>("npm_mha_decode_fwd_f16", d, kv_lens, new_lens, block_table, table_pitch, page_rows);
}

// Sliding-window attention over the per-sequence layouts: NULL block_table is the contiguous cache (npm_mha_decode_fwd_varlen),
// else the paged one; kv_f16: d->k / d->v hold halves.  The refusals of that entry point, and: window < 1, a call that is not
// causal (the window is a rule about a growing self-attention cache), NULL kv_lens.  A refused call launches nothing.
extern "C" int npm_mha_decode_fwd_window(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                         const int32_t *block_table, int32_t table_pitch, int32_t page_rows, int32_t window,
                                         int32_t kv_f16) {
    const char *name = "npm_mha_decode_fwd_window";
    NPM_REQUIRE_INIT();
    if (window < 1) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: window %d is not >= 1", name, window);
    if (d == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: the descriptor is NULL", name);
    if (d->causal == 0) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: a window needs causal attention", name);
    if (kv_lens == nullptr) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: kv_lens is NULL", name);
    if (block_table != nullptr && page_shift(page_rows) < 0)
        return npm::fail(NPM_E_BAD_ARGUMENT, "%s: page_rows %d is not a power of two >= %d", name, page_rows, TILE);
    if (kv_f16) return decode_fwd<_Float16>(name, d, kv_lens, new_lens, block_table, table_pitch, page_rows, window);
    return decode_fwd<float>(name, d, kv_lens, new_lens, block_table, table_pitch, page_rows, window);
}

// What the five row-copy entry points share, after NPM_REQUIRE_INIT and the preconditions that hold even for an empty call: the
// checks, the grid and the launch.  ``rows`` [batch * count, row_len] with pitch rows_pitch is the source of an append (gather =
// false) or the contiguous destination of a gather; ``lens``: at_lens of a ragged append (NULL: the uniform one at ``at``) or the
// lengths of a gather; page_rows > 0: ``cache`` is paged.  An empty call is NPM_OK whatever the pointers are.  KV = _Float16: the
// cache holds halves (its pitch and stride count halves), ``rows`` stays fp32; 8 columns per thread, so everything on the fp16 side
// and row_len are multiples of 8.
template <typename KV = float>
static int row_copy(const char *name, bool gather, const float *rows, int64_t rows_pitch, const RowLayout &cache, int32_t page_rows,
                    int32_t batch, int32_t count, int32_t row_len, bool ragged, int32_t at, const int32_t *lens,
                    const int32_t *new_lens) {
#define ROW_ARG(cond)                                                                                           \
    do {                                                                                                        \
        if (!(cond)) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: bad argument: %s", name, #cond);                \
    } while (0)
    ROW_ARG(batch >= 0 && count >= 0 && row_len >= 0 && at >= 0);
    if (batch == 0 || count == 0 || row_len == 0) return NPM_OK;
    ROW_ARG(rows != nullptr && cache.base != nullptr && (lens != nullptr || !ragged));
    ROW_ARG(aligned16(rows) && aligned16(cache.base));
    constexpr int W = RowVec<KV>::W;
    ROW_ARG(row_len % W == 0 && rows_pitch % 4 == 0 && cache.pitch % W == 0 && cache.stride % W == 0);
    ROW_ARG(rows_pitch >= row_len && cache.pitch >= row_len && (!page_rows || cache.stride >= (int64_t)page_rows * cache.pitch));
#undef ROW_ARG
    const long total = (long)batch * count * (row_len / W);
    const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 2048)), block(256);
    hipStream_t s = npm::ctx().stream;
    const int row4 = row_len / W;
    if (gather) {
        float *out = const_cast<float *>(rows);                       // the entry point's own float *out
        if (page_rows) hipLaunchKernelGGL((kv_gather_kernel<true, KV>), grid, block, 0, s, cache, out, count, row4, lens, total);
        else hipLaunchKernelGGL((kv_gather_kernel<false, KV>), grid, block, 0, s, cache, out, count, row4, lens, total);
    } else if (page_rows) {
        hipLaunchKernelGGL((kv_append_kernel<true, true, KV>), grid, block, 0, s, rows, (long)rows_pitch, cache, count, row4, at, lens, new_lens, total);
    } else if (ragged) {
        hipLaunchKernelGGL((kv_append_kernel<true, false, KV>), grid, block, 0, s, rows, (long)rows_pitch, cache, count, row4, at, lens, new_lens, total);
    } else {
        hipLaunchKernelGGL((kv_append_kernel<false, false, KV>), grid, block, 0, s, rows, (long)rows_pitch, cache, count, row4, at, lens, new_lens, total);
    }
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

static RowLayout contiguous(const void *cache, int64_t pitch, int64_t stride_b) {
    return RowLayout{static_cast<float *>(const_cast<void *>(cache)), (long)pitch, (long)stride_b, nullptr, 0, 0};
}

static RowLayout paged(const void *pool, int64_t row_pitch, int64_t page_stride, const int32_t *table, int32_t table_pitch,
                       int32_t page_rows) {
    return RowLayout{static_cast<float *>(const_cast<void *>(pool)), (long)row_pitch, (long)page_stride, table, table_pitch, page_shift(page_rows)};
}

extern "C" int npm_kv_append(const float *src, int64_t src_pitch, float *cache, int64_t cache_pitch, int64_t cache_stride_b,
                             int32_t batch, int32_t new_tokens, int32_t row_len, int32_t at) {
    NPM_REQUIRE_INIT();
    return row_copy("npm_kv_append", false, src, src_pitch, contiguous(cache, cache_pitch, cache_stride_b), 0, batch, new_tokens, row_len,
                    false, at, nullptr, nullptr);
}

extern "C" int npm_kv_append_varlen(const float *src, int64_t src_pitch, float *cache, int64_t cache_pitch, int64_t cache_stride_b,
                                    int32_t batch, int32_t new_tokens, int32_t row_len, const int32_t *at_lens,
                                    const int32_t *new_lens) {
    NPM_REQUIRE_INIT();
    return row_copy("npm_kv_append_varlen", false, src, src_pitch, contiguous(cache, cache_pitch, cache_stride_b), 0, batch, new_tokens,
                    row_len, true, 0, at_lens, new_lens);
}

extern "C" int npm_kv_gather_varlen(const float *cache, int64_t cache_pitch, int64_t cache_stride_b, float *out, int32_t batch,
                                    int32_t rows, int32_t row_len, const int32_t *lens) {
    NPM_REQUIRE_INIT();
    return row_copy("npm_kv_gather_varlen", true, out, row_len, contiguous(cache, cache_pitch, cache_stride_b), 0, batch, rows, row_len,
                    true, 0, lens, nullptr);
}

// The paged forms refuse a NULL length array or table and a bad page size even when there is nothing to copy.
extern "C" int npm_kv_append_paged(const float *src, int64_t src_pitch, float *pool, int64_t row_pitch, int64_t page_stride,
                                   int32_t batch, int32_t new_tokens, int32_t row_len, const int32_t *at_lens,
                                   const int32_t *new_lens, const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    NPM_REQUIRE_INIT();
    NPM_ARG(at_lens != nullptr && block_table != nullptr && table_pitch >= 0 && page_shift(page_rows) >= 0);
    return row_copy("npm_kv_append_paged", false, src, src_pitch, paged(pool, row_pitch, page_stride, block_table, table_pitch, page_rows),
                    page_rows, batch, new_tokens, row_len, true, 0, at_lens, new_lens);
}

extern "C" int npm_kv_gather_paged(const float *pool, int64_t row_pitch, int64_t page_stride, float *out, int32_t batch, int32_t rows,
                                   int32_t row_len, const int32_t *lens, const int32_t *block_table, int32_t table_pitch,
                                   int32_t page_rows) {
    NPM_REQUIRE_INIT();
    NPM_ARG(lens != nullptr && block_table != nullptr && table_pitch >= 0 && page_shift(page_rows) >= 0);
    return row_copy("npm_kv_gather_paged", true, out, row_len, paged(pool, row_pitch, page_stride, block_table, table_pitch, page_rows),
                    page_rows, batch, rows, row_len, true, 0, lens, nullptr);
}

// The row copies of an fp16 cache, each the entry point of its layout above: at_lens == NULL is npm_kv_append at ``at``,
// block_table == NULL the contiguous cache (cache_stride the batch stride), else the page pool (cache_stride the page stride).
extern "C" int npm_kv_append_f16(const float *src, int64_t src_pitch, void *cache, int64_t cache_pitch, int64_t cache_stride,
                                 int32_t batch, int32_t new_tokens, int32_t row_len, int32_t at, const int32_t *at_lens,
                                 const int32_t *new_lens, const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    NPM_REQUIRE_INIT();
    if (block_table != nullptr) {
        NPM_ARG(at_lens != nullptr && table_pitch >= 0 && page_shift(page_rows) >= 0);
        return row_copy<_Float16>("npm_kv_append_f16", false, src, src_pitch,
                                  paged(cache, cache_pitch, cache_stride, block_table, table_pitch, page_rows), page_rows, batch,
                                  new_tokens, row_len, true, 0, at_lens, new_lens);
    }
    return row_copy<_Float16>("npm_kv_append_f16", false, src, src_pitch, contiguous(cache, cache_pitch, cache_stride), 0, batch,
                              new_tokens, row_len, at_lens != nullptr, at_lens ? 0 : at, at_lens, new_lens);
}

extern "C" int npm_kv_gather_f16(const void *cache, int64_t cache_pitch, int64_t cache_stride, float *out, int32_t batch,
                                 int32_t rows, int32_t row_len, const int32_t *lens, const int32_t *block_table,
                                 int32_t table_pitch, int32_t page_rows) {
    NPM_REQUIRE_INIT();
    if (block_table != nullptr) {
        NPM_ARG(lens != nullptr && table_pitch >= 0 && page_shift(page_rows) >= 0);
        return row_copy<_Float16>("npm_kv_gather_f16", true, out, row_len,
                                  paged(cache, cache_pitch, cache_stride, block_table, table_pitch, page_rows), page_rows, batch,
                                  rows, row_len, true, 0, lens, nullptr);
    }
    return row_copy<_Float16>("npm_kv_gather_f16", true, out, row_len, contiguous(cache, cache_pitch, cache_stride), 0, batch, rows,
                              row_len, true, 0, lens, nullptr);
}

// Copy-on-write of a paged cache: rows 0 .. rows[i] - 1 of page dst_pages[i] = those of page src_pages[i], i < n, in one launch.
// The pool is bytes here -- page_stride_bytes between pages, rows of row_bytes back to back inside one -- so f32 and f16 pools
// take the same call.  src_pages, dst_pages and rows are device arrays; the caller guarantees pages of the pool, src != dst and
// rows[i] * row_bytes <= page_stride_bytes.  The grid is sized for a full page; n == 0 or row_bytes == 0 is NPM_OK and no launch.
extern "C" int npm_kv_copy_pages(void *pool, int64_t page_stride_bytes, int64_t row_bytes, const int32_t *src_pages,
                                 const int32_t *dst_pages, const int32_t *rows, int32_t n) {
    NPM_REQUIRE_INIT();
    NPM_ARG(n >= 0 && row_bytes >= 0 && page_stride_bytes >= 0);
    if (n == 0 || row_bytes == 0) return NPM_OK;
    NPM_ARG(pool != nullptr && src_pages != nullptr && dst_pages != nullptr && rows != nullptr);
    NPM_ARG(aligned16(pool) && row_bytes % 16 == 0 && page_stride_bytes % 16 == 0 && page_stride_bytes >= row_bytes);
    const long page16 = page_stride_bytes / 16;
    const dim3 grid((unsigned)std::min<long>((page16 + 255) / 256, 64), (unsigned)std::min(n, 65535)), block(256);
    hipLaunchKernelGGL(kv_copy_pages_kernel, grid, block, 0, npm::ctx().stream, static_cast<u32x4v *>(pool), page16, (long)(row_bytes / 16),
                       src_pages, dst_pages, rows, n);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

// The copy-on-write of a layered cache: npm_kv_copy_pages in `planes` pools that lie plane_stride_bytes apart behind `pool`, the
// same pairs in each, in one launch.  planes == 0 is NPM_OK and no launch, as n == 0 and row_bytes == 0 are.
extern "C" int npm_kv_copy_pages_planes(void *pool, int64_t page_stride_bytes, int64_t row_bytes, const int32_t *src_pages,
                                        const int32_t *dst_pages, const int32_t *rows, int32_t n, int32_t planes,
                                        int64_t plane_stride_bytes) {
    NPM_REQUIRE_INIT();
    NPM_ARG(n >= 0 && row_bytes >= 0 && page_stride_bytes >= 0 && planes >= 0 && plane_stride_bytes >= 0);
    if (n == 0 || row_bytes == 0 || planes == 0) return NPM_OK;
    NPM_ARG(pool != nullptr && src_pages != nullptr && dst_pages != nullptr && rows != nullptr);
    NPM_ARG(aligned16(pool) && row_bytes % 16 == 0 && page_stride_bytes % 16 == 0 && page_stride_bytes >= row_bytes);
    NPM_ARG(plane_stride_bytes % 16 == 0 && (planes == 1 || plane_stride_bytes >= page_stride_bytes));
    const long page16 = page_stride_bytes / 16;
    const dim3 grid((unsigned)std::min<long>((page16 + 255) / 256, 64), (unsigned)std::min(n, 65535), (unsigned)std::min(planes, 65535)),
        block(256);
    hipLaunchKernelGGL(kv_copy_pages_planes_kernel, grid, block, 0, npm::ctx().stream, static_cast<u32x4v *>(pool), page16,
                       (long)(row_bytes / 16), src_pages, dst_pages, rows, n, planes, (long)(plane_stride_bytes / 16));
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}
