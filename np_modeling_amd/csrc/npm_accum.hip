// Gradient accumulation over micro-batches (include/npm_hip.h): the fold dst += src over up to 32 pairs of ranges in one launch,
// optionally with the fp64 sum of squares of the NEW dst values in the same pass, and the clip factor of a gradient that is still
// to be multiplied by a scale (1 / micro-batches, 1 / tokens).  HBM-bound: every dst element is read and written once with
// 16-byte accesses, every src element read once.
//
// The tiling and the element order of a tile RESTATE sumsq_tiles_kernel / sumsq_finish_kernel of npm_clip.hip: the sum this file
// produces has to be, bit for bit, what npm_sumsq_ranges computes on the updated buffers.  Nothing is shared with that file on
// purpose (its kernels stay as they are); the bitwise tests of tests/accum_cases.py hold the two together.
#include <algorithm>
#include <climits>
#include <cmath>

#include "npm_internal.h"

namespace {

constexpr int kTile = NPM_SUMSQ_TILE;
constexpr int kLanes = 256;
static_assert(kTile % (4 * kLanes) == 0, "a tile is a whole number of 16-byte accesses per lane");

// The pairs of one launch: a kernel argument, indexed with a block-uniform r -> scalar loads.
struct accum_table {
    float *dst[NPM_SUMSQ_MAX_RANGES];
    const float *src[NPM_SUMSQ_MAX_RANGES];
    uint64_t n[NPM_SUMSQ_MAX_RANGES];
    int32_t count;
};

__device__ __forceinline__ double square(float x) {
    const double d = (double)x;
    return d * d;                               // exact: 24 + 24 significant bits
}

// red[0 .. 256) -> red[0], the fixed tree of npm_clip.hip
__device__ __forceinline__ void block_tree(double *red) {
    __syncthreads();
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}

typedef float f32x4v __attribute__((ext_vector_type(4)));

// Every element is touched once: the interior's loads and stores are non-temporal.  A measured choice (tools/accum_bench.py,
// profiles/r28_accum_bench.log): plain accesses 32.7 / 451.5 us per fold of 12.6 M / 200 M elements, non-temporal src loads alone
// 32.5 / 441.6, non-temporal on both sides 29.1 / 429.1, with a spread of 1 - 2 % on the yardstick beside them.
__device__ __forceinline__ float4 load_dst(const float4 *p) {
    const f32x4v v = __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store_dst(float4 *p, const float4 &v) {
    __builtin_nontemporal_store(f32x4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f32x4v *>(p));
}
// four src floats at xs: ONE 16-byte load where src has dst's 16-byte phase, four 4-byte loads where not
template <bool kAligned>
__device__ __forceinline__ float4 load_src(const float *xs) {
    if (kAligned) {
        const f32x4v v = __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(xs));
        return make_float4(v.x, v.y, v.z, v.w);
    }
    return make_float4(__builtin_nontemporal_load(xs), __builtin_nontemporal_load(xs + 1), __builtin_nontemporal_load(xs + 2),
                       __builtin_nontemporal_load(xs + 3));
}

// The aligned interior of a tile: lane t takes groups t, t + 256, ... in ascending order, x y z w inside a group.  Four groups
// at a time with every load issued before the first use (128 bytes in flight per lane); the order of the additions, and of the
// squares that join s, is the ascending one whatever the batching.
constexpr int kBatch = 4;
template <bool kSum, bool kAligned>
__device__ __forceinline__ void fold_groups(float4 *__restrict__ d4, const float *__restrict__ xs, size_t groups, int t, double &s) {
    auto finish = [&](float4 v, const float4 a, size_t q) {
        v.x += a.x;
        v.y += a.y;
        v.z += a.z;
        v.w += a.w;
        store_dst(d4 + q, v);
        if (kSum) {
            s += square(v.x);
            s += square(v.y);
            s += square(v.z);
            s += square(v.w);
        }
    };
    size_t q = t;
    for (; q + (kBatch - 1) * kLanes < groups; q += kBatch * kLanes) {
        float4 v[kBatch], a[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            v[u] = load_dst(d4 + q + u * kLanes);
            a[u] = load_src<kAligned>(xs + 4 * (q + u * kLanes));
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) finish(v[u], a[u], q + u * kLanes);
    }
    for (; q < groups; q += kLanes) finish(load_dst(d4 + q), load_src<kAligned>(xs + 4 * q), q);
}

// One block, one tile of dst, cut by dst's alignment exactly as sumsq_tiles_kernel cuts it: `head` elements in front of the first
// 16-byte boundary (lanes 0 .. head - 1, first), `groups` aligned groups of four (group q on lane q % 256, ascending, x y z w),
// `tail` elements behind (lanes 0 .. tail - 1, last).  src is read 16 bytes at a time where it has dst's 16-byte phase and with four
// 4-byte loads where not: one float32 addition per element either way, the same bits.  kSum: the lane also adds the exact fp64
// square of every value it stores, in that order, and the block reduces with the tree into partials[tile].
template <bool kSum>
__global__ void __launch_bounds__(kLanes)
accum_tiles_kernel(const accum_table table, double *__restrict__ partials) {
    unsigned tile = blockIdx.x;
    int r = 0;
    for (; r < table.count; ++r) {              // the same walk in every lane: scalar
        const unsigned tiles = (unsigned)((table.n[r] + (kTile - 1)) / kTile);
        if (tile < tiles) break;
        tile -= tiles;
    }
    double s = 0.0;
    if (r < table.count) {                      // always true for the grid the host launches
        const size_t begin = (size_t)tile * kTile;
        const size_t len = std::min<size_t>(table.n[r] - begin, (size_t)kTile);
        float *__restrict__ d = table.dst[r] + begin;        // the host refuses a dst range that meets anything else
        const float *__restrict__ x = table.src[r] + begin;
        const size_t head = std::min<size_t>((size_t)((16 - ((uintptr_t)d & 15)) & 15) / 4, len);
        const size_t groups = (len - head) / 4;
        const size_t tail = len - head - 4 * groups;
        const int t = threadIdx.x;
        if ((size_t)t < head) {
            const float v = d[t] + x[t];
            d[t] = v;
            if (kSum) s += square(v);
        }
        float4 *__restrict__ d4 = reinterpret_cast<float4 *>(d + head);
        const float *__restrict__ xs = x + head;
        if ((((uintptr_t)xs) & 15) == 0) fold_groups<kSum, true>(d4, xs, groups, t, s);      // block-uniform
        else fold_groups<kSum, false>(d4, xs, groups, t, s);
        if ((size_t)t < tail) {
            const size_t i = head + 4 * groups + t;
            const float v = d[i] + x[i];
            d[i] = v;
            if (kSum) s += square(v);
        }
    }
    if (kSum) {
        __shared__ double red[kLanes];
        red[threadIdx.x] = s;
        block_tree(red);
        if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
    }
}

// ONE block: lane t adds partials t, t + 256, ... in that order, then the tree; the total joins *acc (sumsq_finish_kernel restated).
__global__ void __launch_bounds__(kLanes)
accum_finish_kernel(const double *__restrict__ partials, int count, double *__restrict__ acc) {
    __shared__ double red[kLanes];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += kLanes) s += partials[i];
    red[threadIdx.x] = s;
    block_tree(red);
    if (threadIdx.x == 0) *acc = *acc + red[0];
}

__global__ void clip_finish_scaled_kernel(double *__restrict__ state, double max_norm, double grad_scale) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double root = sqrt(state[0]);
    const double norm = grad_scale * root;
    state[1] = norm;
    if (!isfinite(norm)) {
        state[2] = 0.0;
        state[3] = 0.0;
    } else {
        const double ratio = max_norm / (norm + 1e-6);
        const double c = ratio < 1.0 ? ratio : 1.0;
        const double factor = grad_scale * c;
        state[2] = (double)(float)factor;
        state[3] = 1.0;
    }
}

inline bool overlap(const float *a, uint64_t an, const float *b, uint64_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return an != 0 && bn != 0 && a0 < b0 + 4 * bn && b0 < a0 + 4 * an;
}

}  // namespace

extern "C" {

int npm_accumulate_ranges(const npm_ranges *dst, const npm_ranges *src, double *sumsq_acc) {
    NPM_REQUIRE_INIT();
    NPM_ARG(dst != nullptr && src != nullptr);
    NPM_ARG(dst->count >= 0 && dst->count <= NPM_SUMSQ_MAX_RANGES);
    NPM_ARG(src->count == dst->count);
    accum_table table = {};
    uint64_t tiles = 0;
    for (int r = 0; r < dst->count; ++r) {
        NPM_ARG(dst->n[r] == src->n[r]);
        NPM_ARG(dst->n[r] == 0 || (dst->ptr[r] != nullptr && src->ptr[r] != nullptr));
        NPM_ARG(((uintptr_t)dst->ptr[r] & 3) == 0 && ((uintptr_t)src->ptr[r] & 3) == 0);
        table.dst[r] = const_cast<float *>(dst->ptr[r]);
        table.src[r] = src->ptr[r];
        table.n[r] = dst->n[r];
        tiles += dst->n[r] / kTile + (dst->n[r] % kTile != 0);
    }
    table.count = dst->count;
    for (int r = 0; r < dst->count; ++r) {      // a dst range is written: it may meet no other dst range and no src range
        for (int q = 0; q < dst->count; ++q) {
            NPM_ARG(q == r || !overlap(dst->ptr[r], dst->n[r], dst->ptr[q], dst->n[q]));
            NPM_ARG(!overlap(dst->ptr[r], dst->n[r], src->ptr[q], src->n[q]));
        }
    }
    if (tiles == 0) return NPM_OK;
    NPM_ARG(tiles <= (uint64_t)INT_MAX);
    hipStream_t s = npm::ctx().stream;
    if (sumsq_acc == nullptr) {
        hipLaunchKernelGGL(accum_tiles_kernel<false>, dim3((unsigned)tiles), dim3(kLanes), 0, s, table, (double *)nullptr);
        NPM_CHECK_LAUNCH();
        return NPM_OK;
    }
    npm::Scratch part;
    int rc = part.alloc(sizeof(double) * tiles);
    if (rc) return rc;
    double *p = (double *)part.ptr;
    hipLaunchKernelGGL(accum_tiles_kernel<true>, dim3((unsigned)tiles), dim3(kLanes), 0, s, table, p);
    NPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(accum_finish_kernel, dim3(1), dim3(kLanes), 0, s, (const double *)p, (int)tiles, sumsq_acc);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

int npm_clip_finish_scaled(double *state, double max_norm, double grad_scale) {
    NPM_REQUIRE_INIT();
    NPM_ARG(state != nullptr);
    NPM_ARG(max_norm > 0.0);                    // false for NaN too; +inf: no clipping
    NPM_ARG(grad_scale > 0.0 && std::isfinite(grad_scale));
    hipLaunchKernelGGL(clip_finish_scaled_kernel, dim3(1), dim3(64), 0, npm::ctx().stream, state, max_norm, grad_scale);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

}  // extern "C"
