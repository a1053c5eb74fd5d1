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
#include <algorithm>
#include <cmath>
#include <cstring>

#include "npm_internal.h"

namespace {

constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;
constexpr int WAVES = 4;          // per block
constexpr int TILE = 16;          // keys per tile
constexpr int ROWS = WAVES * 16;  // query rows per block

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

char g_last[112] = "";

struct PrefillArgs {
    const float *q, *k, *v;
    long q_pitch, k_pitch, k_sb, v_pitch, v_sb;
    float *ctx;
    long ctx_pitch;
    float *lse;                   // optional [B, Hq, T]
    int heads, kv_heads, tokens, len, causal;
    int group, gb, tb, head_chunks;   // Hq / Hkv; heads of the group and tokens per block (gb tb <= ROWS); ceil(group / gb)
    float c, scale;               // scale * log2(e), scale
};

struct PageArgs {
    const int *table;
    int pitch, shift;
};

template <int VW> struct VecOf;
template <> struct VecOf<4> { using type = f32x4v; };
template <> struct VecOf<2> { using type = f32x2v; };
template <> struct VecOf<1> { using type = float; };

template <int VW> __device__ __forceinline__ float comp(const typename VecOf<VW>::type &x, int e) { return x[e]; }
template <> __device__ __forceinline__ float comp<1>(const float &x, int) { return x; }
template <int VW> __device__ __forceinline__ void put(typename VecOf<VW>::type &x, int e, float y) { x[e] = y; }
template <> __device__ __forceinline__ void put<1>(float &x, int, float y) { x = y; }

// D: head size.  VL: the sequence has L = kv_lens[b] valid keys and nb = new_lens[b] (NULL: a.tokens) new tokens; VL = false reads
// neither array (L = a.len, nb = a.tokens) and is otherwise the same code.  PG (implies VL): a.k / a.v are page pools, a.k_sb /
// a.v_sb the page strides, pg the block table.
template <int D, bool VL, bool PG>
__global__ void __launch_bounds__(WAVES * 64)
mha_prefill_kernel(const PrefillArgs a, const int *__restrict__ kv_lens, const int *__restrict__ new_lens, const PageArgs pg) {
#pragma clang fp contract(off)
    static_assert(VL || !PG, "a paged cache has per-sequence lengths");
    constexpr int KU = D / 16;                    // 16-byte K reads per lane and tile
    constexpr int VW = D >= 64 ? 4 : D / 16;      // floats per V read
    constexpr int DQ = D / (16 * VW);             // V reads per lane and key
    constexpr int NS = KU >= 4 ? 4 : KU;          // score accumulation chains
    constexpr int KP = D + 4;                     // LDS row pitch of K: lanes of one ds_read_b128 group land on distinct 16-byte slots
    constexpr int VP = D;                         //                of V: 16 lanes read one contiguous row
    constexpr int F4 = TILE * D / 4;              // 16-byte pieces of one K (or V) tile
    constexpr int NLD = (F4 + WAVES * 64 - 1) / (WAVES * 64);   // ... per thread
    using VVec = typename VecOf<VW>::type;
    __shared__ __attribute__((aligned(16))) float s_k[2][TILE][KP];
    __shared__ __attribute__((aligned(16))) float s_v[2][TILE][VP];

    const int c = blockIdx.y, b = blockIdx.z;
    const int tok0 = (int)(blockIdx.x / a.head_chunks) * a.tb, g0 = (int)(blockIdx.x % a.head_chunks) * a.gb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int T = a.tokens;
    // block-uniform loads of the sequence's own lengths (scalar loads; nothing is stored through the scalar unit)
    const int L = VL ? kv_lens[b] : a.len;
    const int nb = VL ? (new_lens ? new_lens[b] : T) : T;

    // this lane's query row: token tok0 + r % tb of head c + (g0 + r / tb) Hkv.  A row of the tile that is no row of the call
    // (past the group, past T) is never stored; a row of a padded token (t >= nb) is stored as ctx = 0, lse = -inf.
    const int r = wave * 16 + n;
    const int t = tok0 + r % a.tb, gi = g0 + r / a.tb;
    const int h = c + gi * a.kv_heads;
    const bool exists = r < a.gb * a.tb && gi < a.group && t < T;
    const bool live = exists && t < nb;
    const int limit = live ? max(0, min(a.causal ? L - nb + t + 1 : L, L)) : 0;     // keys this row may see: j < limit

    // the block's walk: key tiles below the largest limit of its rows (its last live token's).  tok0 >= nb: no live row, no tile,
    // no load -- the rows are stored below and the block is done.
    const int seen = tok0 < nb ? max(0, min(a.causal ? L - nb + min(tok0 + a.tb, nb) : L, L)) : 0;
    const int tiles = (seen + TILE - 1) / TILE;   // every walked tile holds a key < L, so L >= 1 wherever a load is redirected
    int wlimit = limit;                           // the largest limit of this wave's rows (wave-uniform)
    wlimit = max(wlimit, __shfl_xor(wlimit, 1));
    wlimit = max(wlimit, __shfl_xor(wlimit, 2));
    wlimit = max(wlimit, __shfl_xor(wlimit, 4));
    wlimit = max(wlimit, __shfl_xor(wlimit, 8));
    wlimit = __builtin_amdgcn_readfirstlane(wlimit);

    f32x4v q[KU];
    {
        const float *src = a.q + ((long)b * T + (live ? t : 0)) * a.q_pitch + (long)(live ? h : 0) * D + 4 * g;
#pragma unroll
        for (int u = 0; u < KU; ++u) q[u] = live ? *reinterpret_cast<const f32x4v *>(src + 16 * u) : f32x4v{0.f, 0.f, 0.f, 0.f};
    }

    f32x4v acc[DQ][VW];
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[dq][e] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const float *kbase = a.k + (PG ? 0L : (long)b * a.k_sb) + (long)c * D;
    const float *vbase = a.v + (PG ? 0L : (long)b * a.v_sb) + (long)c * D;

    // staging: piece i of a tile is columns 4 (i % (D / 4)) .. + 3 of key i / (D / 4)
    f32x4v kst[NLD], vst[NLD];
    auto load_tile = [&](int tile) {
        const int key0 = tile * TILE;
        long koff = 0, voff = 0;
        int in_page = ~0;
        if (PG) {
            // the page of the tile, a function of b, the tile index and kernel arguments only: wave-uniform, a scalar load.
            // key0 < L, so the entry is one of the sequence's own pages.
            const int page = pg.table[(long)b * pg.pitch + (__builtin_amdgcn_readfirstlane(key0) >> pg.shift)];
            koff = (long)page * a.k_sb;
            voff = (long)page * a.v_sb;
            in_page = (1 << pg.shift) - 1;
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int key = key0 + piece / (D / 4), col = (piece % (D / 4)) * 4;
                const long row = min(key, L - 1) & in_page;
                kst[i] = *reinterpret_cast<const f32x4v *>(kbase + koff + row * a.k_pitch + col);
                vst[i] = *reinterpret_cast<const f32x4v *>(vbase + voff + row * a.v_pitch + col);
                if (key >= L) vst[i] = f32x4v{0.f, 0.f, 0.f, 0.f};      // the last tile of the sequence only
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int row = piece / (D / 4), col = (piece % (D / 4)) * 4;
                *reinterpret_cast<f32x4v *>(&s_k[buf][row][col]) = kst[i];
                *reinterpret_cast<f32x4v *>(&s_v[buf][row][col]) = vst[i];
            }
        }
    };

    if (tiles > 0) {
        load_tile(0);
        store_tile(0);
    }
    __syncthreads();
    for (int tile = 0; tile < tiles; ++tile) {
        const int key0 = tile * TILE, buf = tile & 1;
        if (tile + 1 < tiles) load_tile(tile + 1);                    // in flight during the products below
        if (key0 < wlimit) {                                          // wave-uniform: some row of this wave sees a key of the tile
            // S^T = K Q^T: NS independent accumulation chains, summed pairwise (as in mha_decode_kernel)
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
            // -inf by selection for keys the row does not see; then log2 units
            float x[4], tmax = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                x[w] = key0 + 4 * g + w < limit ? s[w] : -INFINITY;
                tmax = fmaxf(tmax, x[w]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m, tmax);                       // raw
            const float ref = m_new == -INFINITY ? 0.f : m_new * a.c; // a row with nothing visible yet: exponents stay -inf, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m * a.c - ref);    // -inf * c = -inf: 0
            m = m_new;
            float psum = 0.f;
            f32x4v p;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                p[w] = __builtin_amdgcn_exp2f(fmaf(x[w], a.c, -ref));
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
        if (tile + 1 < tiles) store_tile(buf ^ 1);
        __syncthreads();
    }

    // every wave stores its own rows: register w of acc[dq][e] is column d = 16 VW dq + VW (4 g + w) + e of row n
    float lt = l;
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    if (!exists) return;
    const bool none = m == -INFINITY;             // no visible key: 0 and -inf by selection, not 0 / 0
    const float rf = none ? 0.f : m * a.c;
    float *dst = a.ctx + ((long)b * T + t) * a.ctx_pitch + (long)h * D;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            VVec o;
#pragma unroll
            for (int e = 0; e < VW; ++e) put<VW>(o, e, none ? 0.f : acc[dq][e][w] / lt);
            *reinterpret_cast<VVec *>(dst + 16 * VW * dq + VW * (4 * g + w)) = o;
        }
    if (g == 0 && a.lse)
        a.lse[((long)b * a.heads + h) * T + t] = none ? -INFINITY : fmaf(a.scale, m, (__builtin_amdgcn_logf(lt) + fmaf(-m, a.c, rf)) * LN2);
}

template <int D>
void launch_prefill(const PrefillArgs &a, const int *kv_lens, const int *new_lens, const PageArgs &pg, dim3 grid, hipStream_t s) {
    const dim3 block(WAVES * 64);
    if (pg.table) hipLaunchKernelGGL((mha_prefill_kernel<D, true, true>), grid, block, 0, s, a, kv_lens, new_lens, pg);
    else if (kv_lens) hipLaunchKernelGGL((mha_prefill_kernel<D, true, false>), grid, block, 0, s, a, kv_lens, new_lens, pg);
    else hipLaunchKernelGGL((mha_prefill_kernel<D, false, false>), grid, block, 0, s, a, nullptr, nullptr, pg);
}

// page_rows -> log2, or -1 unless it is a power of two >= TILE
int page_shift(int page_rows) {
    if (page_rows < TILE || (page_rows & (page_rows - 1))) return -1;
    return __builtin_ctz((unsigned)page_rows);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int npm_mha_prefill_supported(int head_dim) {
    return head_dim == 16 || head_dim == 32 || head_dim == 64 || head_dim == 128;
}

extern "C" const char *npm_last_prefill_kernel(void) { return g_last; }

extern "C" int npm_mha_prefill_fwd(const npm_mha_decode *d, const int32_t *kv_lens, const int32_t *new_lens,
                                   const int32_t *block_table, int32_t table_pitch, int32_t page_rows) {
    const bool varlen = kv_lens != nullptr, paged = block_table != nullptr;
    NPM_REQUIRE_INIT();
    NPM_ARG(d != nullptr);
    PageArgs pg{};
    if (paged) {
        if (!varlen) return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_prefill_fwd: a block table needs kv_lens");
        if (page_shift(page_rows) < 0)
            return npm::fail(NPM_E_BAD_ARGUMENT, "npm_mha_prefill_fwd: page_rows %d is not a power of two >= %d", page_rows, TILE);
        NPM_ARG(d->kv_len >= 0 && (int64_t)table_pitch * page_rows >= d->kv_len);       // a table row names every page of kv_len rows
        NPM_ARG(d->k_stride_b >= (int64_t)page_rows * d->k_pitch && d->v_stride_b >= (int64_t)page_rows * d->v_pitch);
        pg.table = block_table; pg.pitch = table_pitch; pg.shift = page_shift(page_rows);
    }
    NPM_ARG(d->batch >= 1 && d->heads >= 1 && d->kv_heads >= 1 && d->new_tokens >= 1 && d->head_dim >= 1);
    NPM_ARG(d->heads % d->kv_heads == 0);
    NPM_ARG(varlen ? d->kv_len >= 0 : d->kv_len >= d->new_tokens);     // varlen: new_lens[b] <= kv_lens[b] <= kv_len is the caller's
    NPM_ARG(d->scale > 0.f);
    NPM_ARG(d->q != nullptr && d->k != nullptr && d->v != nullptr && d->ctx != nullptr);
    const int D = d->head_dim;
    if (!npm_mha_prefill_supported(D))
        return npm::fail(NPM_E_UNSUPPORTED, "npm_mha_prefill_fwd: head_dim %d is not supported (head_dim in {16, 32, 64, 128})", D);
    NPM_ARG(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->ctx));
    NPM_ARG(d->q_pitch % 4 == 0 && d->k_pitch % 4 == 0 && d->v_pitch % 4 == 0 && d->ctx_pitch % 4 == 0);
    NPM_ARG(d->k_stride_b % 4 == 0 && d->v_stride_b % 4 == 0);
    NPM_ARG(d->q_pitch >= (int64_t)d->heads * D && d->ctx_pitch >= (int64_t)d->heads * D);
    NPM_ARG(d->k_pitch >= (int64_t)d->kv_heads * D && d->v_pitch >= (int64_t)d->kv_heads * D);
    NPM_ARG(d->batch <= 65535 && d->kv_heads <= 65535);

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
    const int64_t token_tiles = ((int64_t)d->new_tokens + a.tb - 1) / a.tb;
    NPM_ARG(token_tiles * a.head_chunks <= 0x7fffffff);

    const dim3 grid((unsigned)(token_tiles * a.head_chunks), d->kv_heads, d->batch);
    hipStream_t s = npm::ctx().stream;
    switch (D) {
        case 16: launch_prefill<16>(a, kv_lens, new_lens, pg, grid, s); break;
        case 32: launch_prefill<32>(a, kv_lens, new_lens, pg, grid, s); break;
        case 64: launch_prefill<64>(a, kv_lens, new_lens, pg, grid, s); break;
        default: launch_prefill<128>(a, kv_lens, new_lens, pg, grid, s); break;
    }
    NPM_CHECK_LAUNCH();
    int at = snprintf(g_last, sizeof g_last, "mha_prefill_kernel D=%d T=%d rows=%d causal=%d%s", D, d->new_tokens, ROWS, a.causal,
                      varlen ? " varlen=1" : "");
    if (paged) snprintf(g_last + at, sizeof g_last - at, " paged=%d", page_rows);
    return NPM_OK;
}
