// One row of token sampling as a device function: what sample_rows_kernel and verify_rows_kernel (npm_sample.hip) both run, so that
// a row of a speculative step is sampled by the very instructions that sample it in the one-token-per-step loop.  The passes
// are described at the top of npm_sample.hip; include/npm_hip.h npm_sample_rows states the contract.
#pragma once

#include "npm_internal.h"
#include "npm_philox.h"

#include <cmath>

namespace {

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int NT = 1024, NW = NT / 64;
constexpr int LDS_ROW = NPM_SAMPLE_LDS_ROW;
constexpr unsigned NEG_INF_KEY = 0x007FFFFFu;          // key(-inf): every finite logit has a larger key

// larger z <=> larger key; -0.0 and 0.0 share one key
__device__ __forceinline__ unsigned order_key(float z) {
    unsigned b = __float_as_uint(z);
    if ((b << 1) == 0) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// floor(exp((z - zmax) / t) 2^32): the difference, the product with 1 / t and the exponential each rounded to fp32
__device__ __forceinline__ u64 weight_of(float z, float zmax, float inv_t) {
#pragma clang fp contract(off)
    const float d = z - zmax;
    const float a = d * inv_t;
    const float q = expf(a);
    return (u64)(q * 4294967296.0f);
}

// f(i, z) for every token of the row, each by exactly one thread
template <bool VEC, typename F>
__device__ __forceinline__ void for_row_global(const float *__restrict__ g, int vocab, F f) {
    if (VEC) {
        const int n4 = vocab >> 2;
        for (int i4 = threadIdx.x; i4 < n4; i4 += NT) {
            const f32x4v v = *reinterpret_cast<const f32x4v *>(g + 4 * i4);
            f(4 * i4, v.x);
            f(4 * i4 + 1, v.y);
            f(4 * i4 + 2, v.z);
            f(4 * i4 + 3, v.w);
        }
        for (int i = 4 * n4 + threadIdx.x; i < vocab; i += NT) f(i, g[i]);
    } else {
        for (int i = threadIdx.x; i < vocab; i += NT) f(i, g[i]);
    }
}

template <bool VEC, typename F>
__device__ __forceinline__ void for_row(const float *__restrict__ g, const float *lds, bool in_lds, int vocab, F f) {
    if (in_lds) {
        for (int i = threadIdx.x; i < vocab; i += NT) f(i, lds[i]);
    } else {
        for_row_global<VEC>(g, vocab, f);
    }
}

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// inclusive prefix over the 64 lanes
__device__ __forceinline__ u64 wave_scan_u64(u64 v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_scan_u32(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

struct Shared {
    u64 mass[256];
    unsigned cnt[256];
    u64 red_mass[NW];
    unsigned red_cnt[NW];
    float red_max[NW];
    int red_idx[NW];
    unsigned red_flag[NW];
    // what thread 0 decides and every thread reads after the barrier
    u64 b_need, b_above_mass;
    unsigned b_prefix, b_above_cnt;
};

// the sum of (m, c) over the block, in every thread; integer sums: the order does not matter
__device__ __forceinline__ void block_sum(Shared &sh, u64 &m, unsigned &c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    m = wave_sum_u64(m);
    c = wave_sum_u32(c);
    __syncthreads();                       // the previous readers of red_* are done
    if (lane == 0) {
        sh.red_mass[wave] = m;
        sh.red_cnt[wave] = c;
    }
    __syncthreads();
    m = 0;
    c = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        m += sh.red_mass[w];
        c += sh.red_cnt[w];
    }
}

// Radix select from the top of the order, over the tokens with key > floor_key plus a lump of lump_cnt tokens of key floor_key
// (mass lump_cnt * lump_w).  BY_MASS: the key at which the mass from the top reaches `need` (>= 1, <= the total mass); else the
// key of the need-th token.  Returns the key; above_mass / above_cnt: the tokens with a larger key; rest: what of `need` is left
// for the tokens equal to the key.
template <bool VEC, bool BY_MASS>
__device__ __forceinline__ unsigned radix_select(Shared &sh, const float *__restrict__ g, const float *lds, bool in_lds, int vocab,
                                                 unsigned floor_key, unsigned lump_cnt, u64 lump_w, float zmax, float inv_t, u64 need,
                                                 u64 &above_mass, unsigned &above_cnt, u64 &rest) {
    unsigned prefix = 0, mask = 0;
    above_mass = 0;
    above_cnt = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();                   // the previous pass's readers of the histogram and of b_* are done
        for (int i = threadIdx.x; i < 256; i += NT) {
            sh.mass[i] = 0;
            sh.cnt[i] = 0;
        }
        __syncthreads();
        int cur = -1;
        unsigned c = 0;
        u64 m = 0;
        for_row<VEC>(g, lds, in_lds, vocab, [&](int, float z) {
            const unsigned key = order_key(z);
            if (key > floor_key && (key & mask) == prefix) {
                const int bin = (key >> shift) & 255;
                if (bin != cur) {
                    if (cur >= 0) {
                        atomicAdd(&sh.cnt[cur], c);
                        if (BY_MASS) atomicAdd(&sh.mass[cur], m);
                    }
                    cur = bin;
                    c = 0;
                    m = 0;
                }
                c += 1;
                if (BY_MASS) m += weight_of(z, zmax, inv_t);
            }
        });
        if (cur >= 0) {
            atomicAdd(&sh.cnt[cur], c);
            if (BY_MASS) atomicAdd(&sh.mass[cur], m);
        }
        if (threadIdx.x == 0 && lump_cnt > 0 && (floor_key & mask) == prefix) {
            const int bin = (floor_key >> shift) & 255;
            atomicAdd(&sh.cnt[bin], lump_cnt);
            if (BY_MASS) atomicAdd(&sh.mass[bin], lump_cnt * lump_w);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 acc_m = 0, acc = 0;
            unsigned acc_c = 0;
            int sel = 0;
            for (int bin = 255; bin >= 0; --bin) {
                const u64 here = BY_MASS ? sh.mass[bin] : (u64)sh.cnt[bin];
                if (acc + here >= need) {
                    sel = bin;
                    break;
                }
                acc += here;
                acc_m += sh.mass[bin];
                acc_c += sh.cnt[bin];
            }
            sh.b_need = need - acc;
            sh.b_above_mass = acc_m;
            sh.b_above_cnt = acc_c;
            sh.b_prefix = prefix | ((unsigned)sel << shift);
        }
        __syncthreads();
        need = sh.b_need;
        above_mass += sh.b_above_mass;
        above_cnt += sh.b_above_cnt;
        prefix = sh.b_prefix;
        mask |= 255u << shift;
    }
    rest = need;
    return prefix;
}

struct RowSample {
    int token, kept;
    float prob;
};

// The whole block samples the row g[0 .. vocab) with (t, k, p), seed sd and draw counter `counter`; `row` is the block's LDS_ROW
// floats of LDS.  Returns true in exactly ONE thread, and `out` is the row's result there; every other thread returns false, some
// of them early: no barrier may follow the call.
template <bool VEC>
__device__ __forceinline__ bool sample_row(float *row, Shared &sh, const float *__restrict__ g, int vocab, float t, int k, float p,
                                           u64 sd, u64 counter, RowSample &out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in_lds = vocab <= LDS_ROW;

    // ---- pass 1: maximum with its first index, validity, finite count; the row into LDS ----
    float zmax = -INFINITY;
    int imax = 0x7fffffff;
    unsigned bad = 0, finite = 0;
    for_row_global<VEC>(g, vocab, [&](int i, float z) {
        if (in_lds) row[i] = z;
        bad |= (unsigned)(!(z < INFINITY));             // NaN or +inf
        finite += (unsigned)(z > -INFINITY);
        if (z > zmax || (z == zmax && i < imax)) {
            zmax = z;
            imax = i;
        }
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oz = __shfl_xor(zmax, off, 64);
        const int oi = __shfl_xor(imax, off, 64);
        if (oz > zmax || (oz == zmax && oi < imax)) {
            zmax = oz;
            imax = oi;
        }
        bad |= __shfl_xor(bad, off, 64);
    }
    finite = wave_sum_u32(finite);
    if (lane == 0) {
        sh.red_max[wave] = zmax;
        sh.red_idx[wave] = imax;
        sh.red_flag[wave] = bad;
        sh.red_cnt[wave] = finite;
    }
    __syncthreads();                                    // also: the row is in LDS
    zmax = sh.red_max[0];
    imax = sh.red_idx[0];
    bad = sh.red_flag[0];
    finite = sh.red_cnt[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const float oz = sh.red_max[w];
        const int oi = sh.red_idx[w];
        if (oz > zmax || (oz == zmax && oi < imax)) {
            zmax = oz;
            imax = oi;
        }
        bad |= sh.red_flag[w];
        finite += sh.red_cnt[w];
    }

    const float inv_t = 1.0f / t;
    const bool invalid = bad != 0 || finite == 0 || !(t >= 0.f) || !(p > 0.f);
    const bool greedy = t == 0.f || k == 1 || !(inv_t < INFINITY);
    if (invalid || greedy) {
        out.token = invalid ? -1 : imax;
        out.kept = invalid ? 0 : 1;
        out.prob = invalid ? 0.f : 1.f;
        return threadIdx.x == 0;
    }

    // ---- top-k cut: K1 = {key > t1} and the q1 lowest indices of {key == t1} ----
    const unsigned k_eff = (k <= 0 || (unsigned)k > finite) ? finite : (unsigned)k;
    unsigned t1 = NEG_INF_KEY, q1 = 0;
    u64 unused_m, rest;
    unsigned unused_c;
    if (k_eff < finite) {
        t1 = radix_select<VEC, false>(sh, g, row, in_lds, vocab, NEG_INF_KEY, 0, 0, zmax, inv_t, k_eff, unused_m, unused_c, rest);
        q1 = (unsigned)rest;
    }
    const u64 w1 = weight_of(key_value(t1), zmax, inv_t);
    u64 mass1 = 0;
    unsigned cnt1 = 0;
    for_row<VEC>(g, row, in_lds, vocab, [&](int, float z) {
        if (order_key(z) > t1) mass1 += weight_of(z, zmax, inv_t);
    });
    block_sum(sh, mass1, cnt1);
    mass1 += q1 * w1;                                    // W1

    // ---- top-p cut: K2 = {key > t2} and the q2 lowest indices of {key == t2} ----
    unsigned t2 = t1, q2 = q1, n_kept = k_eff;
    u64 w2 = w1, mass_k = mass1;
    if (p < 1.f) {
        u64 need = (u64)floor((double)p * (double)mass1);
        if (need < 1) need = 1;
        u64 above_mass;
        unsigned above_cnt;
        t2 = radix_select<VEC, true>(sh, g, row, in_lds, vocab, t1, q1, w1, zmax, inv_t, need, above_mass, above_cnt, rest);
        w2 = weight_of(key_value(t2), zmax, inv_t);
        q2 = w2 ? (unsigned)((rest + w2 - 1) / w2) : 0;
        n_kept = above_cnt + q2;
        mass_k = above_mass + q2 * w2;                   // Wk
    }

    // ---- the draw: target = floor(Wk u24 / 2^24), exact ----
    unsigned c4[4] = {(unsigned)counter, (unsigned)(counter >> 32), 0u, 0u};
    philox4x32_10(c4, (unsigned)sd, (unsigned)(sd >> 32));
    const u64 u24 = c4[0] >> 8;
    const u64 target = (mass_k >> 24) * u24 + (((mass_k & 0xFFFFFFull) * u24) >> 24);

    // ---- the token, in index order ----
    const int seg = ((vocab + NW - 1) / NW + 63) / 64 * 64;          // a wave's tokens: contiguous, whole steps of 64
    const int begin = wave * seg, end = begin + seg < vocab ? begin + seg : vocab;
    u64 seg_mass = 0;
    unsigned seg_eq = 0;
    for (int i = begin + lane; i < end; i += 64) {
        const float z = in_lds ? row[i] : g[i];
        const unsigned key = order_key(z);
        if (key > t2) seg_mass += weight_of(z, zmax, inv_t);
        seg_eq += (unsigned)(key == t2);
    }
    seg_mass = wave_sum_u64(seg_mass);
    seg_eq = wave_sum_u32(seg_eq);
    __syncthreads();
    if (lane == 0) {
        sh.red_mass[wave] = seg_mass;
        sh.red_cnt[wave] = seg_eq;
    }
    __syncthreads();
    u64 run_mass = 0;                                    // of key > t2, in the waves before this one
    unsigned run_eq = 0;
    for (int w = 0; w < wave; ++w) {
        run_mass += sh.red_mass[w];
        run_eq += sh.red_cnt[w];
    }
    const u64 before = run_mass + (u64)(run_eq < q2 ? run_eq : q2) * w2;
    const unsigned eq_after = run_eq + seg_eq;
    const u64 after = run_mass + seg_mass + (u64)(eq_after < q2 ? eq_after : q2) * w2;
    if (!(before <= target && target < after)) return false;   // exactly one wave goes on: the running mass ends at Wk > target
    for (int base = begin; base < end; base += 64) {
        const int i = base + lane;
        u64 m = 0, w = 0;
        unsigned e = 0;
        if (i < end) {
            const float z = in_lds ? row[i] : g[i];
            const unsigned key = order_key(z);
            if (key > t2) m = w = weight_of(z, zmax, inv_t);
            if (key == t2) {
                e = 1;
                w = w2;
            }
        }
        const u64 m_incl = wave_scan_u64(m, lane);
        const unsigned e_incl = wave_scan_u32(e, lane);
        const unsigned eq_here = run_eq + e_incl;
        const u64 s_incl = run_mass + m_incl + (u64)(eq_here < q2 ? eq_here : q2) * w2;
        const u64 hit = __ballot(s_incl > target);
        if (hit) {
            const bool mine = lane == __ffsll((long long)hit) - 1;
            if (mine) {
                out.token = i;
                out.kept = (int)n_kept;
                out.prob = (float)((double)w / (double)mass_k);
            }
            return mine;
        }
        run_mass += __shfl(m_incl, 63, 64);
        run_eq += __shfl(e_incl, 63, 64);
    }
    return false;                                        // not reached: the running mass ends at Wk > target
}

}  // namespace
