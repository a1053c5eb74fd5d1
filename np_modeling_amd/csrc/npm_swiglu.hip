// The gate of a gated-SiLU ("SwiGLU") feed-forward: npm_swiglu_fwd / npm_swiglu_bwd (include/npm_hip.h).
//
// pre [rows, 2 units] (pitch ld) is the packed projection's output: gate columns [0, units), up columns [units, 2 units).
//   forward   h = (gate sigma(gate)) up
//   backward  dgate = dh up sigma(gate) (1 + gate (1 - sigma(gate))),  dup = dh (gate sigma(gate)); sigma is recomputed from pre
// HBM-bound (12 B per element forward, 20 B backward): one thread per 4 columns with 16-byte accesses where units, the pitches and
// the bases allow it, one per element otherwise; grid-stride under NPM_TUNE_EW_GRID_CAP with the (row, column) pair carried
// along instead of divided out every trip; nontemporal instances by npm_rowops.hip's stream_nt rule on the bytes of pre.
#include <algorithm>

#include "npm_internal.h"

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int W, bool NT>
struct Vec;
template <bool NT>
struct Vec<4, NT> {
    typedef f32x4v type;
    static __device__ __forceinline__ type load(const float *p) {
        if (NT) return __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(p));
        return *reinterpret_cast<const f32x4v *>(p);
    }
    static __device__ __forceinline__ void store(float *p, type v) {
        if (NT) __builtin_nontemporal_store(v, reinterpret_cast<f32x4v *>(p));
        else *reinterpret_cast<f32x4v *>(p) = v;
    }
    static __device__ __forceinline__ float &at(type &v, int i) { return reinterpret_cast<float *>(&v)[i]; }
};
template <bool NT>
struct Vec<1, NT> {
    typedef float type;
    static __device__ __forceinline__ type load(const float *p) { return NT ? __builtin_nontemporal_load(p) : *p; }
    static __device__ __forceinline__ void store(float *p, type v) {
        if (NT) __builtin_nontemporal_store(v, p);
        else *p = v;
    }
    static __device__ __forceinline__ float &at(type &v, int) { return v; }
};

// sigma(g) and 1 - sigma(g) = sigma(-g), both without overflow and without cancellation: t = exp(-|g|) is in [0, 1],
// p = 1 / (1 + t) is sigma of the non-negative one of g and -g, q = t / (1 + t) of the other.
__device__ __forceinline__ void sigmoid_pair(float g, float &sig, float &one_minus) {
    const float t = expf(-fabsf(g));
    const float p = 1.0f / (1.0f + t), q = t / (1.0f + t);
    sig = g >= 0.f ? p : q;
    one_minus = g >= 0.f ? q : p;
}

__device__ __forceinline__ float swiglu_one(float g, float u) {
    const float t = expf(-fabsf(g));
    const float sig = g >= 0.f ? 1.0f / (1.0f + t) : t / (1.0f + t);
    return (g * sig) * u;
}

// item i = (row, column group); a thread starts at its own pair and advances by the grid's stride as (row_step, col_step)
template <int W, bool NT>
__global__ void __launch_bounds__(256)
swiglu_fwd_kernel(const float *__restrict__ pre, long ld, long rows, long units, long per_row, long row_step, long col_step,
                  float *__restrict__ h, long ldh) {
    typedef Vec<W, NT> V;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long row = first / per_row, col = first - row * per_row;
    for (; row < rows;) {
        const float *gate = pre + row * ld + col * W;
        typename V::type g = V::load(gate), u = V::load(gate + units), o;
#pragma unroll
        for (int i = 0; i < W; ++i) V::at(o, i) = swiglu_one(V::at(g, i), V::at(u, i));
        V::store(h + row * ldh + col * W, o);
        row += row_step;
        col += col_step;
        if (col >= per_row) { col -= per_row; ++row; }
    }
}

template <int W, bool NT>
__global__ void __launch_bounds__(256)
swiglu_bwd_kernel(const float *__restrict__ pre, long ld, const float *__restrict__ dh, long lddh, long rows, long units,
                  long per_row, long row_step, long col_step, float *__restrict__ dpre, long lddpre) {
    typedef Vec<W, NT> V;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long row = first / per_row, col = first - row * per_row;
    for (; row < rows;) {
        const float *gate = pre + row * ld + col * W;
        typename V::type g = V::load(gate), u = V::load(gate + units), d = V::load(dh + row * lddh + col * W), dg, du;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            float sig, one_minus;
            sigmoid_pair(V::at(g, i), sig, one_minus);
            V::at(dg, i) = (V::at(d, i) * V::at(u, i)) * (sig * (1.0f + V::at(g, i) * one_minus));
            V::at(du, i) = V::at(d, i) * (V::at(g, i) * sig);
        }
        float *out = dpre + row * lddpre + col * W;
        V::store(out, dg);
        V::store(out + units, du);
        row += row_step;
        col += col_step;
        if (col >= per_row) { col -= per_row; ++row; }
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

struct Plan {
    long per_row, row_step, col_step;
    int grid;
};

inline Plan plan(long rows, long units, int w) {
    Plan p;
    p.per_row = units / w;
    const long total = rows * p.per_row;
    p.grid = (int)std::max<long>(1, std::min<long>((total + 255) / 256, npm::ew_grid_cap()));
    const long stride = (long)p.grid * 256;
    p.row_step = stride / p.per_row;
    p.col_step = stride - p.row_step * p.per_row;
    return p;
}

}  // namespace

extern "C" {

int npm_swiglu_fwd(const float *pre, int64_t ld, int64_t rows, int64_t units, float *h, int64_t ldh) {
    NPM_REQUIRE_INIT();
    NPM_ARG(rows >= 0 && units >= 1 && units <= (1L << 30) && ld >= 2 * units && ldh >= units);
    if (rows == 0) return NPM_OK;
    NPM_ARG(pre != nullptr && h != nullptr);
    NPM_ARG(rows < (1L << 31));
    hipStream_t s = npm::ctx().stream;
    const bool nt = npm::stream_nt_enabled(sizeof(float) * 2 * (size_t)rows * (size_t)units);
    const bool vec = units % 4 == 0 && ld % 4 == 0 && ldh % 4 == 0 && aligned16(pre) && aligned16(h);
    const Plan p = plan(rows, units, vec ? 4 : 1);
#define NPM_SWIGLU_FWD(W, NT) hipLaunchKernelGGL((swiglu_fwd_kernel<W, NT>), dim3(p.grid), dim3(256), 0, s, pre, (long)ld, (long)rows, (long)units, p.per_row, p.row_step, p.col_step, h, (long)ldh)
    if (vec) { if (nt) NPM_SWIGLU_FWD(4, true); else NPM_SWIGLU_FWD(4, false); }
    else { if (nt) NPM_SWIGLU_FWD(1, true); else NPM_SWIGLU_FWD(1, false); }
#undef NPM_SWIGLU_FWD
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

int npm_swiglu_bwd(const float *pre, int64_t ld, const float *dh, int64_t lddh, int64_t rows, int64_t units, float *dpre,
                   int64_t lddpre) {
    NPM_REQUIRE_INIT();
    NPM_ARG(rows >= 0 && units >= 1 && units <= (1L << 30) && ld >= 2 * units && lddh >= units && lddpre >= 2 * units);
    if (rows == 0) return NPM_OK;
    NPM_ARG(pre != nullptr && dh != nullptr && dpre != nullptr);
    NPM_ARG(rows < (1L << 31));
    hipStream_t s = npm::ctx().stream;
    const bool nt = npm::stream_nt_enabled(sizeof(float) * 2 * (size_t)rows * (size_t)units);
    const bool vec = units % 4 == 0 && ld % 4 == 0 && lddh % 4 == 0 && lddpre % 4 == 0 && aligned16(pre) && aligned16(dh) && aligned16(dpre);
    const Plan p = plan(rows, units, vec ? 4 : 1);
#define NPM_SWIGLU_BWD(W, NT) hipLaunchKernelGGL((swiglu_bwd_kernel<W, NT>), dim3(p.grid), dim3(256), 0, s, pre, (long)ld, dh, (long)lddh, (long)rows, (long)units, p.per_row, p.row_step, p.col_step, dpre, (long)lddpre)
    if (vec) { if (nt) NPM_SWIGLU_BWD(4, true); else NPM_SWIGLU_BWD(4, false); }
    else { if (nt) NPM_SWIGLU_BWD(1, true); else NPM_SWIGLU_BWD(1, false); }
#undef NPM_SWIGLU_BWD
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

}  // extern "C"
