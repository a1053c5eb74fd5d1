// npm_rope_kv_append (include/npm_hip.h): what stands in front of the attention of a decode step over a packed projection -- the
// rotation of its q and k heads (npm_rope) and the two appends of its k and v heads (npm_kv_append and its _varlen / _paged /
// _f16 forms) -- in ONE launch instead of three.  A decode step is launch-bound, and the three kernels walk the same rows.
//
// Work items run over (row, head, piece of the first half of the head) of the packed rows [B * T, (H + 2 Hkv) D]:
//   * a q head (h < H): the pair (lo, hi) = (x[i], x[i + D / 2]) is rotated in place, exactly as npm_rope does;
//   * a k head: the same, and for t < new_lens[b] the rotated pair is also stored at row at_b + t of sequence b of the K cache;
//   * a v head: nothing is computed; for t < new_lens[b] the pair is stored in the V cache.
// Without tables (cos == NULL) the q heads are not part of the grid at all and the k heads are only copied.  A row whose position
// is not inside the table is not rotated (npm_rope leaves it untouched) and its k head is stored as it stands (the append copies
// what is there).  Padded rows t >= new_lens[b] are rotated, as npm_rope rotates every row, and stored nowhere.
//
// Bits.  The arithmetic is npm_rope's rotate_pair under `#pragma clang fp contract(off)`: every product and every sum is rounded
// on its own.  An fp16 cache takes the values through the conversion the fp16 append uses (__builtin_convertvector / a scalar
// cast: v_cvt_f16_f32, round to nearest even).  So the packed buffer and both caches hold, bit for bit, what the three launches
// leave.  Vector instance (head_dim % 8 == 0, pitch % 4 == 0, 16-byte aligned qkv, cos and sin): a lane moves one float4 of the
// first half and its partner -- 16-byte loads and stores on the fp32 side, 16 bytes (fp32 cache) or 8 bytes (the 4 halves of an
// fp16 cache) per store on the cache side.  Scalar instance: one pair per lane, for everything else the two contracts allow.
// Plain C++ and vector stores only.

#include "npm_kvattn.h"

#include <algorithm>
#include <cstdio>

namespace {

char g_last_rope_append[96] = "";

// (lo, hi) -> (lo c - hi s, hi c + lo s), six roundings (npm_rope.hip)
template <typename T>
__device__ __forceinline__ void rotate_pair(T &lo, T &hi, const T c, const T s) {
#pragma clang fp contract(off)
    const T a = lo * c, b = hi * s, d = hi * c, e = lo * s;
    lo = a - b;
    hi = d + e;
}

// Where the rows of the two caches live: contiguous (table == nullptr) row j of sequence b is base + b * stride + j * pitch;
// paged: row j & (page_rows - 1) of page table[b * table_pitch + (j >> shift)].  Elements of the cache's type.
struct CacheRows {
    void *k, *v;
    long pitch, stride;
    const int *table;
    int table_pitch, shift;
};

template <bool PG>
__device__ __forceinline__ long row_offset(const CacheRows &c, long b, int j) {
    if (PG) return (long)c.table[b * c.table_pitch + (j >> c.shift)] * c.stride + (long)(j & ((1 << c.shift) - 1)) * c.pitch;
    return b * c.stride + (long)j * c.pitch;
}

__device__ __forceinline__ void store4(float *to, const f32x4v x) { *reinterpret_cast<f32x4v *>(to) = x; }
__device__ __forceinline__ void store4(_Float16 *to, const f32x4v x) {
    *reinterpret_cast<f16x4v *>(to) = __builtin_convertvector(x, f16x4v);
}
__device__ __forceinline__ void store1(float *to, const float x) { *to = x; }
__device__ __forceinline__ void store1(_Float16 *to, const float x) { *to = (_Float16)x; }

struct Shape {
    unsigned tokens, heads, kv_heads, half;     // half = D / 2
    unsigned first_head, active_heads;          // the heads the grid covers: all H + 2 Hkv, or (no rotation) the 2 Hkv behind q
    int table_rows, at;
};

// VEC: items are float4 pieces (pieces = half / 4 per half head), else single elements (pieces = half).  ROT: there are tables.
// VL: at_lens / new_lens are read (new_lens may still be NULL: every t).  PG: the caches are page pools.
template <bool VEC, bool ROT, bool VL, bool PG, typename KV>
__global__ void __launch_bounds__(256)
rope_kv_append_kernel(float *x, long pitch, const Shape sh, const float *__restrict__ cos_t, const float *__restrict__ sin_t,
                      const int *__restrict__ at_lens, const int *__restrict__ new_lens, const CacheRows cache, unsigned total) {
    static_assert(VL || !PG, "a paged cache has per-sequence lengths");
    constexpr unsigned W = VEC ? 4 : 1;
    const unsigned pieces = sh.half / W;
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned rh = i / pieces, e = (i - rh * pieces) * W;        // (row, active head), first element of the piece
        const unsigned row = rh / sh.active_heads, head = sh.first_head + (rh - row * sh.active_heads);
        const unsigned b = row / sh.tokens, t = row - b * sh.tokens;
        const int first = VL ? at_lens[b] : sh.at;
        float *lo_ptr = x + (long)row * pitch + (long)head * (2 * sh.half) + e;
        const bool is_v = head >= sh.heads + sh.kv_heads;
        const bool stored = head >= sh.heads && !(VL && new_lens && (int)t >= new_lens[b]);
        const long p = (long)first + (long)t;
        const bool rotated = ROT && !is_v && p >= 0 && p < sh.table_rows;
        if (!rotated && !stored) continue;
        KV *to = nullptr;
        if (stored) {
            const unsigned kv_head = head - sh.heads - (is_v ? sh.kv_heads : 0);
            to = static_cast<KV *>(is_v ? cache.v : cache.k) + row_offset<PG>(cache, b, first + (int)t) + (long)kv_head * (2 * sh.half) + e;
        }
        if constexpr (VEC) {
            f32x4v lo = *reinterpret_cast<const f32x4v *>(lo_ptr);
            f32x4v hi = *reinterpret_cast<const f32x4v *>(lo_ptr + sh.half);
            if (rotated) {
                const long tab = p * sh.half + e;
                rotate_pair(lo, hi, *reinterpret_cast<const f32x4v *>(cos_t + tab), *reinterpret_cast<const f32x4v *>(sin_t + tab));
                *reinterpret_cast<f32x4v *>(lo_ptr) = lo;
                *reinterpret_cast<f32x4v *>(lo_ptr + sh.half) = hi;
            }
            if (stored) {
                store4(to, lo);
                store4(to + sh.half, hi);
            }
        } else {
            float lo = lo_ptr[0], hi = lo_ptr[sh.half];
            if (rotated) {
                const long tab = p * sh.half + e;
                rotate_pair(lo, hi, cos_t[tab], sin_t[tab]);
                lo_ptr[0] = lo;
                lo_ptr[sh.half] = hi;
            }
            if (stored) {
                store1(to, lo);
                store1(to + sh.half, hi);
            }
        }
    }
}

template <bool VEC, bool ROT, typename KV, typename... Args>
void launch_layout(bool ragged, bool paged, dim3 grid, hipStream_t s, Args... args) {
    if (paged) hipLaunchKernelGGL((rope_kv_append_kernel<VEC, ROT, true, true, KV>), grid, dim3(256), 0, s, args...);
    else if (ragged) hipLaunchKernelGGL((rope_kv_append_kernel<VEC, ROT, true, false, KV>), grid, dim3(256), 0, s, args...);
    else hipLaunchKernelGGL((rope_kv_append_kernel<VEC, ROT, false, false, KV>), grid, dim3(256), 0, s, args...);
}

template <typename KV, typename... Args>
void launch(bool vec, bool rot, bool ragged, bool paged, dim3 grid, hipStream_t s, Args... args) {
    if (vec && rot) launch_layout<true, true, KV>(ragged, paged, grid, s, args...);
    else if (vec) launch_layout<true, false, KV>(ragged, paged, grid, s, args...);
    else if (rot) launch_layout<false, true, KV>(ragged, paged, grid, s, args...);
    else launch_layout<false, false, KV>(ragged, paged, grid, s, args...);
}

}  // namespace

extern "C" const char *npm_last_rope_append_kernel(void) { return g_last_rope_append; }

extern "C" int npm_rope_kv_append(float *qkv, int64_t pitch, int32_t batch, int32_t tokens, int32_t heads, int32_t kv_heads,
                                  int32_t head_dim, const float *cos, const float *sin, int32_t table_rows, int32_t at,
                                  const int32_t *at_lens, const int32_t *new_lens, void *k_cache, void *v_cache,
                                  int64_t cache_pitch, int64_t cache_stride, const int32_t *block_table, int32_t table_pitch,
                                  int32_t page_rows, int32_t kv_f16) {
    NPM_REQUIRE_INIT();
    const bool rot = cos != nullptr || sin != nullptr, paged = block_table != nullptr, ragged = at_lens != nullptr;
    // the paged append's own preconditions, which hold even for an empty call
    if (paged) NPM_ARG(at_lens != nullptr && table_pitch >= 0 && page_shift(page_rows) >= 0);
    NPM_ARG(heads >= 1 && kv_heads >= 1 && head_dim >= 1);
    const int64_t row_len = (int64_t)kv_heads * head_dim, width = (int64_t)(heads + 2 * kv_heads) * head_dim;
    if (rot) {      // npm_rope on the first heads + kv_heads heads
        NPM_ARG(qkv != nullptr && cos != nullptr && sin != nullptr);
        NPM_ARG(batch >= 1 && tokens >= 1 && head_dim >= 2 && head_dim % 2 == 0 && table_rows >= 1);
        NPM_ARG(at_lens != nullptr || (at >= 0 && (int64_t)at + tokens <= table_rows));
    }
    // the appends of the k and the v heads
    NPM_ARG(batch >= 0 && tokens >= 0 && (ragged || at >= 0));
    if (batch == 0 || tokens == 0) return NPM_OK;
    NPM_ARG(head_dim % 2 == 0 && pitch >= width);
    NPM_ARG(qkv != nullptr && k_cache != nullptr && v_cache != nullptr);
    const int w = kv_f16 ? 8 : 4;
    NPM_ARG(aligned16(qkv + (int64_t)heads * head_dim) && aligned16(qkv + (int64_t)heads * head_dim + row_len));
    NPM_ARG(aligned16(k_cache) && aligned16(v_cache));
    NPM_ARG(row_len % w == 0 && pitch % 4 == 0 && cache_pitch % w == 0 && cache_stride % w == 0);
    NPM_ARG(cache_pitch >= row_len && (!paged || cache_stride >= (int64_t)page_rows * cache_pitch));
    const int half = head_dim / 2;
    const bool vec = head_dim % 8 == 0 && aligned16(qkv) && (!rot || (aligned16(cos) && aligned16(sin)));
    const int active = rot ? heads + 2 * kv_heads : 2 * kv_heads;
    const int64_t total = (int64_t)batch * tokens * active * (vec ? half / 4 : half);
    if (total > 0x7fffffffLL)
        return npm::fail(NPM_E_UNSUPPORTED, "%s: %lld work items do not fit the 32-bit index of the kernel", __func__, (long long)total);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, npm::ew_grid_cap())));
    const Shape sh{(unsigned)tokens, (unsigned)heads, (unsigned)kv_heads, (unsigned)half, (unsigned)(rot ? 0 : heads), (unsigned)active,
                   (int)table_rows, (int)at};
    const CacheRows cache{k_cache, v_cache, (long)cache_pitch, (long)cache_stride, block_table, table_pitch,
                          paged ? page_shift(page_rows) : 0};
    hipStream_t s = npm::ctx().stream;
    if (kv_f16) launch<_Float16>(vec, rot, ragged, paged, grid, s, qkv, (long)pitch, sh, cos, sin, at_lens, new_lens, cache, (unsigned)total);
    else launch<float>(vec, rot, ragged, paged, grid, s, qkv, (long)pitch, sh, cos, sin, at_lens, new_lens, cache, (unsigned)total);
    NPM_CHECK_LAUNCH();
    snprintf(g_last_rope_append, sizeof g_last_rope_append, "rope_kv_append_kernel D=%d vec=%d rope=%d varlen=%d paged=%d kv=%s", (int)head_dim,
             (int)vec, (int)rot, (int)ragged, paged ? (int)page_rows : 0, kv_f16 ? "f16" : "f32");
    return NPM_OK;
}
