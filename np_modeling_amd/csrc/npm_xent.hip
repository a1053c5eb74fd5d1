// Softmax cross-entropy from logits and token ids, loss and gradient in one launch (include/npm_hip.h: npm_softmax_xent_rows
// states the contract and the error bound; tests/xent_reference.py restates it in fp64).  It replaces, for a language model, the
// Softmax layer composed with CrossEntropyLoss over a dense one-hot [rows, V] tensor: five passes over [rows, V] become one read
// and, with a gradient, one write.
//
// A thread owns the 16-byte chunks idx = 4 (tid + k G), k = 0, 1, ... of its row, G the threads that share the row, in EVERY
// instance and on both the vector and the scalar path (the scalar path moves a chunk as four 4-byte accesses): the partial sums
// and the trees over them are the same whatever the alignment, so the pitch and the base never change a bit of the result.
//
//   xent_wave              V <= 1024    one wavefront per row (4 rows per block of 256), 4 chunks = 16 registers per lane
//   xent_block256          V <= 8192    one block of 256 per row, 8 chunks = 32 registers per thread
//   xent_block1024         V <= 32768   one block of 1024 per row, 8 chunks = 32 registers per thread
//   xent_block1024_global  V >  32768   one block of 1024 per row, passes 2 and 3 re-read the row
//
// The first three read the row ONCE, every load of a thread issued before the first use, and keep it in registers: no LDS but the
// few words of the block reductions.  (A first version parked the row in LDS as npm_sample_rows does: 128 KB for V = 32000 leaves one block per compute
// unit, whose three passes cannot overlap anything -- 0.32 of the HBM peak for the loss alone at 16384 x 32000, below even the
// instance that re-reads; DESIGN.md 4.5k keeps its figures.)
//
// Three passes over the owned chunks: the maximum m (exact); the fp64 sums of expf(z - m) over every token BUT the target and,
// with smoothing, of z -- the register instances keep expf(z - m) in place of z, a masked token marked by -1; the gradient.  The
// target's own term joins after the tree, so that 1 - p_t = s_excl / s is a quotient of sums and not a difference of nearly equal
// numbers: the target's gradient keeps its relative accuracy when p_t is within 2^-24 of 1.
// Reductions: xor butterflies inside a wavefront, then the wave partials in LDS summed in wave order by every thread.  No atomics.
// The loss sum is a second launch of one block over row_loss[0 .. rows) in fp64, fixed order, and one 8-byte copy to the host.

#include "npm_internal.h"

#include <cmath>

namespace {

enum { KIND_WAVE = 0, KIND_BLOCK = 1, KIND_GLOBAL = 2 };
// 16-byte chunks a thread keeps in registers: 4 per lane of a wavefront, 8 per thread of a block.  (Sixteen per thread of a block of
// 512 spill: the compiler keeps a 64-bit address per chunk for the loads and another for the stores.)
constexpr int chunks_of(int kind) { return kind == KIND_WAVE ? 4 : kind == KIND_BLOCK ? 8 : 1; }
constexpr int WAVE_MAX_V = 4 * 64 * chunks_of(KIND_WAVE), BLOCK256_MAX_V = 4 * 256 * chunks_of(KIND_BLOCK),
              BLOCK1024_MAX_V = 4 * 1024 * chunks_of(KIND_BLOCK);
static_assert(WAVE_MAX_V == 1024 && BLOCK256_MAX_V == 8192 && BLOCK1024_MAX_V == 32768, "tests/xent_cases.py lists these boundaries");
constexpr int MAX_V = 1 << 30;

char g_last_xent_kernel[128] = "";

typedef float f32x4v __attribute__((ext_vector_type(4)));

// n = min(4, V - idx) floats at p; VEC: p is 16-byte aligned
template <bool VEC, bool NT>
__device__ __forceinline__ float4 ld_chunk(const float *p, int n) {
    if (VEC && n == 4) {
        if (NT) {
            const f32x4v v = __builtin_nontemporal_load(reinterpret_cast<const f32x4v *>(p));
            return make_float4(v.x, v.y, v.z, v.w);
        }
        return *reinterpret_cast<const float4 *>(p);
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < n) v[q] = NT ? __builtin_nontemporal_load(p + q) : p[q];
    return make_float4(v[0], v[1], v[2], v[3]);
}

template <bool VEC, bool NT>
__device__ __forceinline__ void st_chunk(float *p, const float4 &g, int n) {
    if (VEC && n == 4) {
        if (NT) __builtin_nontemporal_store(f32x4v{g.x, g.y, g.z, g.w}, reinterpret_cast<f32x4v *>(p));
        else *reinterpret_cast<float4 *>(p) = g;
        return;
    }
    const float v[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < n) {
            if (NT) __builtin_nontemporal_store(v[q], p + q);
            else p[q] = v[q];
        }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// f(c, idx) for every chunk the thread owns: c counts them, idx is the chunk's first token.  The register instances unroll over
// their CHUNKS, so that c is a constant where it indexes the registers.
template <int KIND, int T, class F>
__device__ __forceinline__ void for_chunks(int tid, int vocab, F f) {
    if constexpr (KIND == KIND_GLOBAL) {
        for (int idx = 4 * tid; idx < vocab; idx += 4 * T) f(0, idx);
    } else {
        constexpr int G = KIND == KIND_WAVE ? 64 : T, CHUNKS = chunks_of(KIND);
#pragma unroll
        for (int c = 0; c < CHUNKS; ++c) {
            const int idx = 4 * (c * G + tid);
            if (idx < vocab) f(c, idx);
        }
    }
}

// expf(z - m), or -1 for a masked token (z = -inf): what pass 3 needs of a logit
__device__ __forceinline__ float term_of(float z, float m) { return z == -INFINITY ? -1.f : expf(z - m); }

struct XentArgs {
    const float *logits; long ld;
    const int *targets;
    long rows; int vocab;
    float smoothing, grad_scale;
    float *dlogits; long ldd;
    float *row_loss, *row_lse;
};

// T threads per block; VEC: 16-byte accesses; NT: nontemporal hint on the loads that are the last use of a logit and on the
// gradient stores; GRAD: write dlogits.  The register instances may take 128 registers (4 waves per SIMD: one block of 1024 or
// four of 256 per compute unit), the one that re-reads 64 (two blocks of 1024).
template <int KIND, int T, bool VEC, bool NT, bool GRAD>
__global__ void __launch_bounds__(T, KIND == KIND_GLOBAL ? 8 : 4)
xent_rows_kernel(const XentArgs a) {
#pragma clang fp contract(off)
    constexpr int WAVES = T / 64;
    constexpr bool NT_FIRST = NT && KIND != KIND_GLOBAL;         // KIND_GLOBAL reads the row again: only its last read is a stream
    __shared__ float red_max[WAVES];
    __shared__ double red_sum[2][WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, vocab = a.vocab;
    const long r = KIND == KIND_WAVE ? (long)blockIdx.x * WAVES + wave : (long)blockIdx.x;
    const int tid = KIND == KIND_WAVE ? lane : (int)threadIdx.x;
    if (KIND == KIND_WAVE && r >= a.rows) return;               // no block barrier in this instance
    const int t = a.targets[r];
    float *drow = GRAD ? a.dlogits + r * a.ldd : nullptr;       // no __restrict__: in place it is the logit row

    if (t < 0) {                                                // ignored: the logits are not read (uniform over the row's threads)
        if (GRAD)
            for_chunks<KIND, T>(tid, vocab, [&](int, int idx) {
                st_chunk<VEC, NT>(drow + idx, make_float4(0.f, 0.f, 0.f, 0.f), min(4, vocab - idx));
            });
        if (tid == 0) {
            a.row_loss[r] = 0.f;
            if (a.row_lse != nullptr) a.row_lse[r] = NAN;
        }
        return;
    }
    const float *zrow = a.logits + r * a.ld;                    // may alias drow: every read of a logit precedes its overwrite
    const bool in_range = t < vocab;
    // every thread needs z_t; it feeds s below, which every gradient store depends on: the load is complete before any store
    const float zt = in_range ? zrow[t] : NAN;

    float4 regs[chunks_of(KIND)];

    // ---- pass 1: the maximum; NaN is skipped here and caught by the sum ----
    float m = -INFINITY;
    for_chunks<KIND, T>(tid, vocab, [&](int c, int idx) {
        const int n = min(4, vocab - idx);
        const float4 v = ld_chunk<VEC, NT_FIRST>(zrow + idx, n);
        if constexpr (KIND != KIND_GLOBAL) regs[c] = v;
        const float z[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < n) m = fmaxf(m, z[q]);
    });
    m = wave_max(m);
    if constexpr (KIND != KIND_WAVE) {
        if (lane == 0) red_max[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < WAVES; ++w) m = fmaxf(m, red_max[w]);
    }

    // ---- pass 2: s_excl = sum over j != t of expf(z_j - m), and sum z_j when smoothing reads it; fp64 accumulators ----
    const bool smooth = a.smoothing != 0.f;
    double s_excl = 0.0, sz = 0.0;
    for_chunks<KIND, T>(tid, vocab, [&](int c, int idx) {
        const int n = min(4, vocab - idx);
        float4 v;
        if constexpr (KIND == KIND_GLOBAL) v = ld_chunk<VEC, false>(zrow + idx, n);
        else v = regs[c];
        const float z[4] = {v.x, v.y, v.z, v.w};
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            p[q] = term_of(z[q], m);
            if (q < n) {
                if (idx + q != t) s_excl += (double)(p[q] < 0.f ? 0.f : p[q]);      // not fmaxf: a NaN must reach the sum
                if (smooth) sz += (double)z[q];
            }
        }
        if constexpr (KIND != KIND_GLOBAL) regs[c] = make_float4(p[0], p[1], p[2], p[3]);
    });
    s_excl = wave_sum(s_excl);
    if (smooth) sz = wave_sum(sz);
    if constexpr (KIND != KIND_WAVE) {
        if (lane == 0) {
            red_sum[0][wave] = s_excl;
            red_sum[1][wave] = sz;
        }
        __syncthreads();
        s_excl = 0.0;
        sz = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            s_excl += red_sum[0][w];
            sz += red_sum[1][w];
        }
    }
    // a NaN or +inf anywhere in the row, a row of -inf (m = -inf) and a target outside the vocabulary all make s NaN
    const double s = s_excl + (double)expf(zt - m);
    const double e = (double)a.smoothing;
    if (tid == 0) {
        const double lse = (double)m + log(s);
        double loss = lse - (1.0 - e) * (double)zt;
        if (smooth) loss -= e / (double)vocab * sz;
        a.row_loss[r] = (float)loss;
        if (a.row_lse != nullptr) a.row_lse[r] = (float)lse;
    }
    if (!GRAD) return;

    // ---- pass 3: the gradient ----
    const bool valid = s == s;
    const float inv_s = (float)(1.0 / s);
    const float e_v = (float)(e / (double)vocab), gs = a.grad_scale;
    // p_t - (1 - e) - e / V = e (1 - 1 / V) - s_excl / s
    const float gt = zt == -INFINITY && valid ? 0.f : gs * (float)(e * (1.0 - 1.0 / (double)vocab) - s_excl / s);
    for_chunks<KIND, T>(tid, vocab, [&](int c, int idx) {
        const int n = min(4, vocab - idx);
        float p[4];
        if constexpr (KIND == KIND_GLOBAL) {
            const float4 v = ld_chunk<VEC, NT>(zrow + idx, n);
            p[0] = term_of(v.x, m), p[1] = term_of(v.y, m), p[2] = term_of(v.z, m), p[3] = term_of(v.w, m);
        } else {
            p[0] = regs[c].x, p[1] = regs[c].y, p[2] = regs[c].z, p[3] = regs[c].w;
        }
        float g[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float x = (p[q] < 0.f ? 0.f : p[q]) * inv_s - e_v;
            g[q] = gs * x;
            if (p[q] < 0.f && valid) g[q] = 0.f;                // a masked token
            if (idx + q == t) g[q] = gt;
        }
        st_chunk<VEC, NT>(drow + idx, make_float4(g[0], g[1], g[2], g[3]), n);
    });
}

// out[0] = sum of x[0 .. n) in fp64: thread i adds x[i], x[i + 1024], ... in that order (eight loads in flight), then a tree over
// the 1024 partials
__global__ void __launch_bounds__(1024)
xent_loss_sum_kernel(const float *__restrict__ x, long n, double *__restrict__ out) {
    __shared__ double red[1024];
    double acc = 0.0;
#pragma unroll 8
    for (long i = threadIdx.x; i < n; i += 1024) acc += (double)x[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 512; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

template <int KIND, int T, bool VEC, bool NT>
void launch_grad(const XentArgs &a, bool grad) {
    const unsigned blocks = KIND == KIND_WAVE ? (unsigned)((a.rows + T / 64 - 1) / (T / 64)) : (unsigned)a.rows;
    if (grad) hipLaunchKernelGGL((xent_rows_kernel<KIND, T, VEC, NT, true>), dim3(blocks), dim3(T), 0, npm::ctx().stream, a);
    else hipLaunchKernelGGL((xent_rows_kernel<KIND, T, VEC, NT, false>), dim3(blocks), dim3(T), 0, npm::ctx().stream, a);
}

template <int KIND, int T>
void launch(const XentArgs &a, bool grad, bool vec, bool nt) {
    if (vec) {
        if (nt) launch_grad<KIND, T, true, true>(a, grad);
        else launch_grad<KIND, T, true, false>(a, grad);
    } else {
        if (nt) launch_grad<KIND, T, false, true>(a, grad);
        else launch_grad<KIND, T, false, false>(a, grad);
    }
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int npm_softmax_xent_rows(const float *logits, int64_t ld, const int32_t *targets, int64_t rows, int64_t vocab,
                                     float smoothing, float grad_scale, float *dlogits, int64_t ldd, float *row_loss,
                                     float *row_lse, double *loss_sum) {
    NPM_REQUIRE_INIT();
    NPM_ARG(loss_sum != nullptr);
    NPM_ARG(rows >= 0 && rows <= 0x7fffffff);
    NPM_ARG(vocab >= 1 && vocab <= MAX_V && ld >= vocab);
    NPM_ARG(smoothing >= 0.f && smoothing < 1.f);               // false for NaN
    NPM_ARG(dlogits == nullptr || ldd >= vocab);
    if (rows == 0) {
        snprintf(g_last_xent_kernel, sizeof(g_last_xent_kernel), "xent_none rows=0");
        *loss_sum = 0.0;
        return NPM_OK;
    }
    NPM_ARG(logits != nullptr && targets != nullptr && row_loss != nullptr);
    const bool grad = dlogits != nullptr, inplace = grad && dlogits == logits;
    if (inplace) {
        NPM_ARG(ldd == ld);
    } else if (grad) {                                          // no other overlap of the two [rows, V] extents
        const uintptr_t z0 = (uintptr_t)logits, z1 = z0 + 4 * (uintptr_t)((rows - 1) * ld + vocab);
        const uintptr_t d0 = (uintptr_t)dlogits, d1 = d0 + 4 * (uintptr_t)((rows - 1) * ldd + vocab);
        NPM_ARG(z1 <= d0 || d1 <= z0);
    }
    const bool vec = aligned16(logits) && ld % 4 == 0 && (!grad || (aligned16(dlogits) && ldd % 4 == 0));
    const bool nt = npm::stream_nt_enabled(sizeof(float) * (size_t)rows * (size_t)vocab);
    const XentArgs a = {logits, (long)ld, targets, (long)rows, (int)vocab, smoothing, grad_scale, dlogits, (long)ldd, row_loss, row_lse};
    const char *name;
    if (vocab <= WAVE_MAX_V) {
        name = "xent_wave";
        launch<KIND_WAVE, 256>(a, grad, vec, nt);
    } else if (vocab <= BLOCK256_MAX_V) {
        name = "xent_block256";
        launch<KIND_BLOCK, 256>(a, grad, vec, nt);
    } else if (vocab <= BLOCK1024_MAX_V) {
        name = "xent_block1024";
        launch<KIND_BLOCK, 1024>(a, grad, vec, nt);
    } else {
        name = "xent_block1024_global";
        launch<KIND_GLOBAL, 1024>(a, grad, vec, nt);
    }
    snprintf(g_last_xent_kernel, sizeof(g_last_xent_kernel), "%s V=%lld grad=%d inplace=%d vec=%d nt=%d", name, (long long)vocab,
             (int)grad, (int)inplace, (int)vec, (int)nt);
    NPM_CHECK_LAUNCH();
    npm::Scratch total;
    int rc = total.alloc(sizeof(double));
    if (rc) return rc;
    hipLaunchKernelGGL(xent_loss_sum_kernel, dim3(1), dim3(1024), 0, npm::ctx().stream, (const float *)row_loss, (long)rows,
                       (double *)total.ptr);
    NPM_CHECK_LAUNCH();
    return npm_d2h(loss_sum, total.ptr, sizeof(double));
}

extern "C" const char *npm_last_xent_kernel(void) { return g_last_xent_kernel; }
