// Rotary position embedding, in place, on the head slices of a [B, T, ..] projection (include/npm_hip.h: npm_rope).
//
//   half = D / 2; element i < half of a head is paired with element i + half ("rotate-half"); for the row's position p
//   c = cos[p, i], s = sin[p, i] (fp32 tables [table_rows, half], made on the host):
//     forward   y[i] = x[i] c - x[i + half] s      y[i + half] = x[i + half] c + x[i] s
//     inverse   y[i] = x[i] c + x[i + half] s      y[i + half] = x[i + half] c - x[i] s      (the transpose: gradients)
//
// Every product and every sum is rounded to fp32 on its own: the result is, bit for bit, what NumPy gives for these expressions
// on float32 arrays.  hipcc contracts a * c - b * s into v_fma_f32 by default (and through __fmul_rn / __fsub_rn too), so the
// arithmetic lives in one function under `#pragma clang fp contract(off)`; the inverse is the forward with -s, which is exact
// (a - (-p) == a + p in IEEE arithmetic, signed zeros included).  The kernels compute no trigonometry.
//
// One stream over x: each pair is read once and written once, the table rows (1 / (2 heads) of the bytes) stay in L2.  The
// attention that follows re-reads the rows, so no nontemporal hint.  Vector kernel: a lane moves one float4 of the first half and
// its partner at + half -- two 16-byte loads of x, one each of cos and sin, two 16-byte stores -- and lanes run over (row, head,
// vector) with the vector fastest, so a wave's accesses are contiguous within a head.  Scalar kernel: the same arithmetic one pair
// per lane, for every other even head size, pitch or alignment.  Both are grid-stride loops under the elementwise kernels' grid
// cap (NPM_TUNE_EW_GRID_CAP).  A row whose position is not inside the table is left untouched: no lane reads past a table,
// whatever lengths a caller uploads.

#include "npm_internal.h"

#include <algorithm>

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// (lo, hi) -> (lo c - hi s, hi c + lo s), six roundings
template <typename T>
__device__ __forceinline__ void rotate_pair(T &lo, T &hi, const T c, const T s) {
#pragma clang fp contract(off)
    const T a = lo * c, b = hi * s, d = hi * c, e = lo * s;
    lo = a - b;
    hi = d + e;
}

// position of row (b, t), or -1 when the tables have no row for it
__device__ __forceinline__ int position_of(unsigned row, unsigned tokens, int at, const int *__restrict__ at_lens, int table_rows) {
    const unsigned b = row / tokens;
    const long p = (long)(at_lens ? at_lens[b] : at) + (long)(row - b * tokens);
    return p >= 0 && p < table_rows ? (int)p : -1;
}

// total = rows * heads * hv items, hv = half / 4 vectors per half head
__global__ void __launch_bounds__(256)
rope_vec_kernel(float *x, long pitch, unsigned tokens, unsigned heads, unsigned hv, const float *__restrict__ cos_t,
                const float *__restrict__ sin_t, int table_rows, int at, const int *__restrict__ at_lens, int inverse, unsigned total) {
    const unsigned stride = gridDim.x * blockDim.x;
    const unsigned half = 4 * hv;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned hi_ = i / hv, v = i - hi_ * hv;                    // (row, head), vector
        const unsigned row = hi_ / heads, head = hi_ - row * heads;
        const int p = position_of(row, tokens, at, at_lens, table_rows);
        if (p >= 0) {
            float *lo_ptr = x + (long)row * pitch + (long)head * (2 * half) + 4 * v;
            const long tab = (long)p * half + 4 * v;
            f32x4v lo = *reinterpret_cast<const f32x4v *>(lo_ptr);
            f32x4v hi = *reinterpret_cast<const f32x4v *>(lo_ptr + half);
            const f32x4v c = *reinterpret_cast<const f32x4v *>(cos_t + tab);
            f32x4v s = *reinterpret_cast<const f32x4v *>(sin_t + tab);
            if (inverse) s = -s;
            rotate_pair(lo, hi, c, s);
            *reinterpret_cast<f32x4v *>(lo_ptr) = lo;
            *reinterpret_cast<f32x4v *>(lo_ptr + half) = hi;
        }
    }
}

// total = rows * heads * half items
__global__ void __launch_bounds__(256)
rope_scalar_kernel(float *x, long pitch, unsigned tokens, unsigned heads, unsigned half, const float *__restrict__ cos_t,
                   const float *__restrict__ sin_t, int table_rows, int at, const int *__restrict__ at_lens, int inverse, unsigned total) {
    const unsigned stride = gridDim.x * blockDim.x;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const unsigned hi_ = i / half, e = i - hi_ * half;
        const unsigned row = hi_ / heads, head = hi_ - row * heads;
        const int p = position_of(row, tokens, at, at_lens, table_rows);
        if (p >= 0) {
            float *lo_ptr = x + (long)row * pitch + (long)head * (2 * half) + e;
            const long tab = (long)p * half + e;
            float lo = lo_ptr[0], hi = lo_ptr[half];
            const float c = cos_t[tab];
            float s = sin_t[tab];
            if (inverse) s = -s;
            rotate_pair(lo, hi, c, s);
            lo_ptr[0] = lo;
            lo_ptr[half] = hi;
        }
    }
}

}  // namespace

extern "C" int npm_rope(float *x, int64_t pitch, int32_t batch, int32_t tokens, int32_t heads, int32_t head_dim, const float *cos,
                        const float *sin, int32_t table_rows, int32_t at, const int32_t *at_lens, int32_t inverse) {
    NPM_REQUIRE_INIT();
    NPM_ARG(x != nullptr && cos != nullptr && sin != nullptr);
    NPM_ARG(batch >= 1 && tokens >= 1 && heads >= 1 && head_dim >= 2 && head_dim % 2 == 0 && table_rows >= 1);
    NPM_ARG(pitch >= (int64_t)heads * head_dim);
    NPM_ARG(at_lens != nullptr || (at >= 0 && (int64_t)at + tokens <= table_rows));
    const int half = head_dim / 2;
    const bool vec = head_dim % 8 == 0 && pitch % 4 == 0 && aligned16(x) && aligned16(cos) && aligned16(sin);
    const int64_t total = (int64_t)batch * tokens * heads * (vec ? half / 4 : half);
    if (total > 0x7fffffffLL)
        return npm::fail(NPM_E_UNSUPPORTED, "%s: %lld work items do not fit the 32-bit index of the kernels", __func__, (long long)total);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, npm::ew_grid_cap()));
    hipStream_t s = npm::ctx().stream;
    if (vec)
        hipLaunchKernelGGL(rope_vec_kernel, dim3(grid), dim3(256), 0, s, x, (long)pitch, (unsigned)tokens, (unsigned)heads,
                           (unsigned)(half / 4), cos, sin, (int)table_rows, (int)at, at_lens, (int)(inverse != 0), (unsigned)total);
    else
        hipLaunchKernelGGL(rope_scalar_kernel, dim3(grid), dim3(256), 0, s, x, (long)pitch, (unsigned)tokens, (unsigned)heads,
                           (unsigned)half, cos, sin, (int)table_rows, (int)at, at_lens, (int)(inverse != 0), (unsigned)total);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}
