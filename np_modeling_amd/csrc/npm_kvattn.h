// What the three attention kernels over a key / value cache share (npm_decode.hip, npm_prefill.hip, npm_prefix.hip; internal):
// the vector types and their accessors, how a page table is handed to a kernel, and the ONE check of an npm_mha_decode
// descriptor with its optional lengths and page table.  Everything lives in the including file's anonymous namespace, so every
// kernel keeps its symbol.
#pragma once

#include <cstdint>

#include "npm_internal.h"

namespace {

constexpr float LOG2E = 1.44269504088896340736f;
constexpr float LN2 = 0.69314718055994530942f;
constexpr int TILE = 16;          // keys per tile: a page holds whole tiles

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8v __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

// VW floats of a V row, and the same elements out of an fp16 cache
template <int VW> struct VecOf;
template <> struct VecOf<4> { using type = f32x4v; };
template <> struct VecOf<2> { using type = f32x2v; };
template <> struct VecOf<1> { using type = float; };

template <int VW> struct HalfVecOf;
template <> struct HalfVecOf<4> { using type = f16x4v; };
template <> struct HalfVecOf<2> { using type = f16x2v; };
template <> struct HalfVecOf<1> { using type = _Float16; };

// A 16-byte piece of a cache row: 4 floats or 8 halves
template <typename KV> struct PieceOf;
template <> struct PieceOf<float> { using type = f32x4v; };
template <> struct PieceOf<_Float16> { using type = f16x8v; };

template <int VW> __device__ __forceinline__ float comp(const typename VecOf<VW>::type &x, int e) { return x[e]; }
template <> __device__ __forceinline__ float comp<1>(const float &x, int) { return x; }
template <int VW> __device__ __forceinline__ void put(typename VecOf<VW>::type &x, int e, float y) { x[e] = y; }
template <> __device__ __forceinline__ void put<1>(float &x, int, float y) { x = y; }

// A paged cache: row j of sequence b is row (j & (rows - 1)) of page table[b * pitch + (j >> shift)]; rows = 1 << shift
struct PageArgs {
    const int *table;
    int pitch, shift;
};

// page_rows -> log2, or -1 unless it is a power of two >= TILE
int page_shift(int page_rows) {
    if (page_rows < TILE || (page_rows & (page_rows - 1))) return -1;
    return __builtin_ctz((unsigned)page_rows);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The check of an attention call over a cache: descriptor ``d``, per-sequence ``lengths`` or not, an optional block table, for a
// cache whose 16 bytes hold ``kv_align`` elements.  ``name`` is the entry point the caller used: every refusal names it.
// ``head_ok`` is the caller's own rule about head size and rows (NPM_E_UNSUPPORTED with its own text); it runs where it always
// ran, behind the shape and pointer checks and in front of the alignment and pitch checks, so a call that breaks two rules is
// refused with the code it was refused with before.  The grid bounds are the caller's.  NPM_OK: ``pg`` is what the kernel takes.
int check_kv_attn(const char *name, const npm_mha_decode *d, bool lengths, const int32_t *block_table, int32_t table_pitch,
                  int32_t page_rows, int kv_align, int (*head_ok)(const char *, const npm_mha_decode *), PageArgs *pg) {
#define KV_ARG(cond)                                                                                   \
    do {                                                                                               \
        if (!(cond)) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: bad argument: %s", name, #cond);        \
    } while (0)
    if (!npm::ctx().ready) return npm::fail(NPM_E_NOT_INITIALIZED, "%s: npm_init() has not been called", name);
    KV_ARG(d != nullptr);
    *pg = PageArgs{};
    if (block_table != nullptr) {
        if (!lengths) return npm::fail(NPM_E_BAD_ARGUMENT, "%s: a block table needs kv_lens", name);
        if (page_shift(page_rows) < 0)
            return npm::fail(NPM_E_BAD_ARGUMENT, "%s: page_rows %d is not a power of two >= %d", name, page_rows, TILE);
        KV_ARG(d->kv_len >= 0 && (int64_t)table_pitch * page_rows >= d->kv_len);        // a table row names every page of kv_len rows
        KV_ARG(d->k_stride_b >= (int64_t)page_rows * d->k_pitch && d->v_stride_b >= (int64_t)page_rows * d->v_pitch);
        pg->table = block_table; pg->pitch = table_pitch; pg->shift = page_shift(page_rows);
    }
    KV_ARG(d->batch >= 1 && d->heads >= 1 && d->kv_heads >= 1 && d->new_tokens >= 1 && d->head_dim >= 1);
    KV_ARG(d->heads % d->kv_heads == 0);
    KV_ARG(lengths ? d->kv_len >= 0 : d->kv_len >= d->new_tokens);      // lengths: new_lens[b] <= kv_lens[b] <= kv_len is the caller's
    KV_ARG(d->scale > 0.f);
    KV_ARG(d->q != nullptr && d->k != nullptr && d->v != nullptr && d->ctx != nullptr);
    if (int rc = head_ok(name, d)) return rc;
    const int64_t D = d->head_dim;
    KV_ARG(aligned16(d->q) && aligned16(d->k) && aligned16(d->v) && aligned16(d->ctx));
    KV_ARG(d->q_pitch % 4 == 0 && d->k_pitch % kv_align == 0 && d->v_pitch % kv_align == 0 && d->ctx_pitch % 4 == 0);
    KV_ARG(d->k_stride_b % kv_align == 0 && d->v_stride_b % kv_align == 0);
    KV_ARG(d->q_pitch >= d->heads * D && d->ctx_pitch >= d->heads * D);
    KV_ARG(d->k_pitch >= d->kv_heads * D && d->v_pitch >= d->kv_heads * D);
#undef KV_ARG
    return NPM_OK;
}

}  // namespace
