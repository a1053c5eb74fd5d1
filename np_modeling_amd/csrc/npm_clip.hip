// AdamW with global-norm gradient clipping (include/npm_hip.h): the fp64 sum of squares over the gradient buckets, the one
// thread that turns it into a clip factor in HBM, and an AdamW step that reads the factor from there.  HBM-bound: the sum reads
// every gradient once with 16-byte loads, the step is one grid-stride pass like adam_kernel (npm_optim.hip).
#include <algorithm>
#include <climits>
#include <cmath>

#include "npm_internal.h"

namespace {

constexpr int kTile = NPM_SUMSQ_TILE;
constexpr int kLanes = 256;
static_assert(kTile % (4 * kLanes) == 0, "a tile is a whole number of 16-byte loads per lane");

__device__ __forceinline__ double square(float x) {
    const double d = (double)x;
    return d * d;                               // exact: 24 + 24 significant bits
}

// red[0 .. 256) -> red[0], a fixed tree
__device__ __forceinline__ void block_tree(double *red) {
    __syncthreads();
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
}

// One block, one tile.  The tile's elements are x[0 .. len): `head` of them in front of the first 16-byte boundary (lanes
// 0 .. head - 1 take one each, first), then `groups` aligned groups of four (group q belongs to lane q % 256, which adds its
// groups in ascending order, x y z w inside a group), then `tail` elements behind (lanes 0 .. tail - 1, last).  Then the tree.
// A product of exact squares and fp64 additions: contraction would not change a bit (the product is exact either way).
__global__ void __launch_bounds__(kLanes)
sumsq_tiles_kernel(const npm_ranges ranges, double *__restrict__ partials) {
    __shared__ double red[kLanes];
    unsigned tile = blockIdx.x;
    int r = 0;
    for (; r < ranges.count; ++r) {             // the same walk in every lane: scalar
        const unsigned tiles = (unsigned)((ranges.n[r] + (kTile - 1)) / kTile);
        if (tile < tiles) break;
        tile -= tiles;
    }
    double s = 0.0;
    if (r < ranges.count) {                     // always true for the grid the host launches
        const size_t begin = (size_t)tile * kTile;
        const size_t len = std::min<size_t>(ranges.n[r] - begin, (size_t)kTile);
        const float *x = ranges.ptr[r] + begin;
        const size_t head = std::min<size_t>((size_t)((16 - ((uintptr_t)x & 15)) & 15) / 4, len);
        const size_t groups = (len - head) / 4;
        const size_t tail = len - head - 4 * groups;
        const int t = threadIdx.x;
        if ((size_t)t < head) s += square(x[t]);
        const float4 *x4 = reinterpret_cast<const float4 *>(x + head);
        // (measured: all 16 loads of a lane in flight at once, or four running sums per lane, read no faster than this)
#pragma unroll 4
        for (size_t q = t; q < groups; q += kLanes) {
            const float4 v = x4[q];
            s += square(v.x);
            s += square(v.y);
            s += square(v.z);
            s += square(v.w);
        }
        if ((size_t)t < tail) s += square(x[head + 4 * groups + t]);
    }
    red[threadIdx.x] = s;
    block_tree(red);
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

// ONE block: lane t adds partials t, t + 256, ... in that order, then the tree; the total joins *acc.
__global__ void __launch_bounds__(kLanes)
sumsq_finish_kernel(const double *__restrict__ partials, int count, double *__restrict__ acc) {
    __shared__ double red[kLanes];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += kLanes) s += partials[i];
    red[threadIdx.x] = s;
    block_tree(red);
    if (threadIdx.x == 0) *acc = *acc + red[0];
}

__global__ void clip_finish_kernel(double *__restrict__ state, double max_norm) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double norm = sqrt(state[0]);
    state[1] = norm;
    if (!isfinite(norm)) {
        state[2] = 0.0;
        state[3] = 0.0;
    } else {
        const double ratio = max_norm / (norm + 1e-6);
        state[2] = (double)(float)(ratio < 1.0 ? ratio : 1.0);
        state[3] = 1.0;
    }
}

// The contract of include/npm_hip.h, operation for operation; every operation rounded on its own.
__global__ void __launch_bounds__(256)
adamw_kernel(float *__restrict__ var, const float *__restrict__ grad, double *__restrict__ m, double *__restrict__ v, size_t n,
             double lr, double beta1, double beta2, double eps, double corr1, double corr2, double omb1, double omb2, double lw,
             const double *__restrict__ clip_state) {
#pragma clang fp contract(off)
    float scale = 1.f;
    if (clip_state != nullptr) {
        if (clip_state[3] == 0.0) return;       // a norm that was not finite: the whole step is skipped
        scale = (float)clip_state[2];
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float g0 = grad[i];
        const float g = clip_state != nullptr ? scale * g0 : g0;
        const double G = (double)g;
        const double GG = G * G;
        const double bm = beta1 * m[i], bv = beta2 * v[i];
        const double t1 = omb1 * G, t2 = omb2 * GG;
        const double nm = bm + t1, nv = bv + t2;
        m[i] = nm;
        v[i] = nv;
        const double p = (double)var[i];
        const double decay = lw * p;
        const double d = p - decay;
        const double step = lr * ((nm / corr1) / (sqrt(nv / corr2) + eps));
        var[i] = (float)(d - step);
    }
}

inline int grid_for(size_t n, int cap = 4096) {
    return (int)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, (size_t)cap));
}

}  // namespace

extern "C" {

int npm_sumsq_ranges(const npm_ranges *ranges, double *acc) {
    NPM_REQUIRE_INIT();
    NPM_ARG(ranges != nullptr && acc != nullptr);
    NPM_ARG(ranges->count >= 0 && ranges->count <= NPM_SUMSQ_MAX_RANGES);
    npm_ranges table = {};
    uint64_t tiles = 0;
    for (int r = 0; r < ranges->count; ++r) {
        NPM_ARG(ranges->n[r] == 0 || ranges->ptr[r] != nullptr);
        NPM_ARG(((uintptr_t)ranges->ptr[r] & 3) == 0);
        table.ptr[r] = ranges->ptr[r];
        table.n[r] = ranges->n[r];
        tiles += ranges->n[r] / kTile + (ranges->n[r] % kTile != 0);
    }
    table.count = ranges->count;
    if (tiles == 0) return NPM_OK;
    NPM_ARG(tiles <= (uint64_t)INT_MAX);
    hipStream_t s = npm::ctx().stream;
    npm::Scratch part;
    int rc = part.alloc(sizeof(double) * tiles);
    if (rc) return rc;
    double *p = (double *)part.ptr;
    hipLaunchKernelGGL(sumsq_tiles_kernel, dim3((unsigned)tiles), dim3(kLanes), 0, s, table, p);
    NPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sumsq_finish_kernel, dim3(1), dim3(kLanes), 0, s, (const double *)p, (int)tiles, acc);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

int npm_clip_finish(double *state, double max_norm) {
    NPM_REQUIRE_INIT();
    NPM_ARG(state != nullptr);
    NPM_ARG(max_norm > 0.0);                    // false for NaN too
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(64), 0, npm::ctx().stream, state, max_norm);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

int npm_adamw_step(float *var, const float *grad, double *m, double *v, size_t n, double lr, double beta1, double beta2,
                   double eps, int step, double weight_decay, const double *clip_state) {
    NPM_REQUIRE_INIT();
    NPM_ARG(step >= 1);
    NPM_ARG(weight_decay >= 0.0);               // false for NaN too
    if (n == 0) return NPM_OK;
    NPM_ARG(var && grad && m && v);
    const double corr1 = 1.0 - pow(beta1, (double)step), corr2 = 1.0 - pow(beta2, (double)step);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, npm::ctx().stream, var, grad, m, v, n, lr, beta1, beta2, eps,
                       corr1, corr2, 1.0 - beta1, 1.0 - beta2, lr * weight_decay, clip_state);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

}  // extern "C"
