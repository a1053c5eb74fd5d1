// One step of beam search on the device: the best 2 W of the W x V continuations of every prompt, and the split into finished
// hypotheses and next beams (include/npm_hip.h: npm_beam_step states the contract; tests/beam_reference.py restates it).
//
// Two kernels, integers and fp64 between them:
//
//   beam_rows_kernel    one block of 1024 threads per logit row, with the passes of npm_sample_row.h: the row in LDS when it fits,
//                       16-byte loads when base and pitch allow; pass 1 (maximum, validity, finite count), the four-pass radix
//                       select for the exact min(C, finite)-th key T1 and its quota q1 of equal keys, one pass for the integer
//                       mass W1 at temperature 1.  Then the at most C <= 64 survivors go to LDS: those above T1 through an LDS
//                       counter (any order), those equal to T1 by their rank in INDEX order -- every wave owns a contiguous
//                       segment, counts its equal keys, and walks the segment with a wave prefix while the quota lasts -- and one
//                       wavefront ranks them by (key, index), a total order, so the compaction's order is forgotten.  Lane j
//                       forms candidate j's score in fp64, rounds it once, and the row's list goes to the workspace.  A dead
//                       row leaves before its first load.
//   beam_merge_kernel   one block per group: the W lists (non-increasing scores, row order) in LDS; every entry finds its place
//                       in the group's total order -- its own position plus, per other beam, how many entries come first, a
//                       binary search -- and the first C are the candidates.  One wavefront writes them and splits them with a
//                       ballot and a prefix count.
//
// No floating-point atomics, no floating-point sum whose order could vary: a launch is bitwise reproducible, and a group's
// results depend on its own W rows only.

#include "npm_sample_row.h"

namespace {

char g_last_beam_kernel[128] = "";

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

constexpr int MAXC = 2 * NPM_BEAM_MAX_WIDTH;           // 64: one wavefront holds a row's survivors, and a group's candidates

struct Survivors {
    float z[MAXC];
    int idx[MAXC];
    unsigned fill;                                     // the LDS counter of the survivors above T1
};

// i before j in a row: the sampler's order
__device__ __forceinline__ bool row_before(unsigned key_i, int i, unsigned key_j, int j) {
    return key_i > key_j || (key_i == key_j && i < j);
}

// A row that gives nothing.  The beam: an empty list.  LOGPROB: lse and chosen NaN, the top lists -1 / -inf.
template <bool LOGPROB>
__device__ __forceinline__ void empty_row(int r, int cands, float *__restrict__ lse, int *__restrict__ ws_count,
                                          float *__restrict__ ws_score, int *__restrict__ ws_token, float *__restrict__ chosen) {
    if (threadIdx.x == 0) {
        if (!LOGPROB) ws_count[r] = 0;
        lse[r] = __uint_as_float(0x7FC00000u);
        if (LOGPROB && chosen != nullptr) chosen[r] = __uint_as_float(0x7FC00000u);
    }
    if (LOGPROB && (int)threadIdx.x < cands) {
        ws_score[(long)r * cands + threadIdx.x] = -INFINITY;
        ws_token[(long)r * cands + threadIdx.x] = -1;
    }
}

// LOGPROB (npm_logprob_rows): cum is 0 for every row, a row is skipped when ids[r] < 0, the list goes to the caller's top_logprob /
// top_token [rows, cands] (padded with -inf / -1, cands may be 0) and chosen[r] is the score of token ids[r].
template <bool VEC, bool LOGPROB>
__global__ void __launch_bounds__(NT)
beam_rows_kernel(const float *__restrict__ logits, long pitch, int vocab, int cands, const float *__restrict__ cum,
                 float *__restrict__ lse, int *__restrict__ ws_count, float *__restrict__ ws_score, int *__restrict__ ws_token,
                 const int *__restrict__ ids, float *__restrict__ chosen) {
    __shared__ float row[LDS_ROW];
    __shared__ Shared sh;
    __shared__ Survivors sv;
    const int r = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float c = LOGPROB ? 0.f : cum[r];
    const int id = (LOGPROB && ids != nullptr) ? ids[r] : 0;
    if (LOGPROB ? id < 0 : !(c > -INFINITY)) {         // dead (-inf or NaN), or skipped: before any logit is loaded
        empty_row<LOGPROB>(r, cands, lse, ws_count, ws_score, ws_token, chosen);
        return;
    }
    const float *__restrict__ g = logits + (long)r * pitch;
    const bool in_lds = vocab <= LDS_ROW;

    // ---- pass 1: maximum, validity, finite count; the row into LDS (sample_row's pass 1) ----
    float zmax = -INFINITY;
    unsigned bad = 0, finite = 0;
    for_row_global<VEC>(g, vocab, [&](int i, float z) {
        if (in_lds) row[i] = z;
        bad |= (unsigned)(!(z < INFINITY));
        finite += (unsigned)(z > -INFINITY);
        zmax = z > zmax ? z : zmax;
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float oz = __shfl_xor(zmax, off, 64);
        zmax = oz > zmax ? oz : zmax;
        bad |= __shfl_xor(bad, off, 64);
    }
    finite = wave_sum_u32(finite);
    if (lane == 0) {
        sh.red_max[wave] = zmax;
        sh.red_flag[wave] = bad;
        sh.red_cnt[wave] = finite;
    }
    if (threadIdx.x == 0) sv.fill = 0;
    __syncthreads();                                   // also: the row is in LDS
    zmax = sh.red_max[0];
    bad = sh.red_flag[0];
    finite = sh.red_cnt[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
        const float oz = sh.red_max[w];
        zmax = oz > zmax ? oz : zmax;
        bad |= sh.red_flag[w];
        finite += sh.red_cnt[w];
    }
    if (bad != 0 || finite == 0) {                     // invalid: contributes nothing
        empty_row<LOGPROB>(r, cands, lse, ws_count, ws_score, ws_token, chosen);
        return;
    }
    zmax += 0.f;                                       // a maximum of -0.0 enters the arithmetic as 0.0, whichever zero came first

    // ---- the cut: {key > t1} and the q1 lowest indices of {key == t1} ----
    const unsigned k_eff = (unsigned)cands < finite ? (unsigned)cands : finite;
    unsigned t1 = NEG_INF_KEY, q1 = 0, above = finite;
    if (k_eff > 0 && k_eff < finite) {                 // k_eff == 0: npm_logprob_rows with top_n == 0
        u64 unused_m, rest;
        t1 = radix_select<VEC, false>(sh, g, row, in_lds, vocab, NEG_INF_KEY, 0, 0, zmax, 1.f, k_eff, unused_m, above, rest);
        q1 = (unsigned)rest;
    }

    // ---- W1: the sampler's mass at temperature 1 over every finite token; an integer sum ----
    u64 mass = 0;
    unsigned unused_c = 0;
    for_row<VEC>(g, row, in_lds, vocab, [&](int, float z) {
        if (order_key(z) > NEG_INF_KEY) mass += weight_of(z, zmax, 1.f);
    });
    block_sum(sh, mass, unused_c);
    const double n = log((double)mass * (1.0 / 4294967296.0));

    // ---- the survivors into LDS: a wave's tokens are contiguous, whole steps of 64 ----
    const int seg = ((vocab + NW - 1) / NW + 63) / 64 * 64;
    const int begin = wave * seg, end = begin + seg < vocab ? begin + seg : vocab;
    unsigned seg_eq = 0;
    for (int i = begin + lane; i < end && k_eff > 0; i += 64) {
        const float z = in_lds ? row[i] : g[i];
        const unsigned key = order_key(z);
        if (key > t1) {
            const unsigned at = atomicAdd(&sv.fill, 1u);
            if (at < (unsigned)MAXC) {                 // always: `above` < C of them exist
                sv.z[at] = z;
                sv.idx[at] = i;
            }
        }
        seg_eq += (unsigned)(key == t1);
    }
    if (q1 > 0) {                                      // uniform over the block
        seg_eq = wave_sum_u32(seg_eq);
        __syncthreads();                               // block_sum's readers of red_cnt are done
        if (lane == 0) sh.red_cnt[wave] = seg_eq;
        __syncthreads();
        unsigned run_eq = 0;                           // equal keys in the waves before this one
        for (int w = 0; w < wave; ++w) run_eq += sh.red_cnt[w];
        if (seg_eq > 0) {
            for (int base = begin; base < end && run_eq < q1; base += 64) {
                const int i = base + lane;
                const float z = i < end ? (in_lds ? row[i] : g[i]) : -INFINITY;
                const unsigned e = (unsigned)(i < end && order_key(z) == t1);
                const unsigned e_incl = wave_scan_u32(e, lane);
                const unsigned rank = run_eq + e_incl - 1;
                if (e && rank < q1) {                  // above + rank < k_eff <= MAXC
                    sv.z[above + rank] = z;
                    sv.idx[above + rank] = i;
                }
                run_eq += __shfl(e_incl, 63, 64);
            }
        }
    }
    __syncthreads();

    // ---- one wavefront: rank by (key, index), score in fp64 with one rounding, the list to the workspace ----
    if (wave != 0) return;
    if (lane == 0) {
        if (!LOGPROB) ws_count[r] = (int)k_eff;
        lse[r] = (float)((double)zmax + n);
        if (LOGPROB && chosen != nullptr) {
            float s_id = __uint_as_float(0x7FC00000u);
            if (id < vocab) s_id = (float)((((double)c - (double)zmax) - n) + (double)(in_lds ? row[id] : g[id]));
            chosen[r] = s_id;
        }
    }
    if ((unsigned)lane >= k_eff) {
        if (LOGPROB && lane < cands) {
            ws_score[(long)r * cands + lane] = -INFINITY;
            ws_token[(long)r * cands + lane] = -1;
        }
        return;
    }
    const float z = sv.z[lane];
    const int idx = sv.idx[lane];
    const unsigned key = order_key(z);
    int rank = 0;
    for (unsigned m = 0; m < k_eff; ++m) rank += (int)row_before(order_key(sv.z[m]), sv.idx[m], key, idx);
    const double s = (((double)c - (double)zmax) - n) + (double)z;
    ws_score[(long)r * cands + rank] = (float)s;
    ws_token[(long)r * cands + rank] = idx;
}

// One block per group.  Entry j of beam w comes before entry j' of beam w' when its score is larger, or equal with w < w', or
// w == w' and j < j': the lists are in that order already, so an entry's place is j plus what the other beams put in front of it.
__global__ void __launch_bounds__(NT)
beam_merge_kernel(int width, int eos, const int *__restrict__ ws_count, const float *__restrict__ ws_score,
                  const int *__restrict__ ws_token, float *__restrict__ cum, int *__restrict__ cand_slot, int *__restrict__ cand_token,
                  float *__restrict__ cand_score, int *__restrict__ parent, int *__restrict__ ids) {
    __shared__ float score[NPM_BEAM_MAX_WIDTH * MAXC];
    __shared__ int count[NPM_BEAM_MAX_WIDTH];
    __shared__ int out_slot[MAXC], out_token[MAXC];
    __shared__ float out_score[MAXC];
    const int g = blockIdx.x, cands = 2 * width;
    const long first = (long)g * width;

    for (int w = threadIdx.x; w < width; w += NT) count[w] = ws_count[first + w];
    __syncthreads();
    for (int e = threadIdx.x; e < width * cands; e += NT) {
        const int w = e / cands, j = e - w * cands;
        if (j < count[w]) score[e] = ws_score[first * cands + e];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < width * cands; e += NT) {
        const int w = e / cands, j = e - w * cands;
        if (j >= count[w]) continue;
        const float s = score[e];
        int place = j;
        for (int o = 0; o < width && place < cands; ++o) {
            if (o == w) continue;
            // how many of beam o's entries come first: a prefix of its list, since its scores do not increase
            const float *list = score + o * cands;
            int lo = 0, hi = count[o];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const bool before = o < w ? list[mid] >= s : list[mid] > s;
                if (before) lo = mid + 1; else hi = mid;
            }
            place += lo;
        }
        if (place < cands) {
            out_slot[place] = (int)first + w;
            out_token[place] = ws_token[first * cands + e];
            out_score[place] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;

    // ---- one wavefront: the candidates out, and the split ----
    const int lane = threadIdx.x;
    int total = 0;
    for (int w = 0; w < width; ++w) total += count[w];
    total = total < cands ? total : cands;
    const bool have = lane < total;
    const int slot = have ? out_slot[lane] : -1, token = have ? out_token[lane] : -1;
    const float s = have ? out_score[lane] : -INFINITY;
    if (lane < cands) {
        cand_slot[(long)g * cands + lane] = slot;
        cand_token[(long)g * cands + lane] = token;
        cand_score[(long)g * cands + lane] = s;
    }
    const bool other = have && !(eos >= 0 && token == eos);
    const unsigned long long others = __ballot(other);
    const int beam = __popcll(others & ((1ull << lane) - 1ull));
    if (other && beam < width) {
        parent[first + beam] = slot;
        ids[first + beam] = token;
        cum[first + beam] = s;
    }
    const int placed = __popcll(others);
    if (lane >= placed && lane < width) {              // lane < width <= 32
        parent[first + lane] = -1;
        ids[first + lane] = -1;
        cum[first + lane] = -INFINITY;
    }
}

}  // namespace

extern "C" int npm_beam_step(const npm_beam *s) {
    NPM_REQUIRE_INIT();
    NPM_ARG(s != nullptr);
    NPM_ARG(s->groups >= 1 && s->width >= 1 && s->width <= NPM_BEAM_MAX_WIDTH);
    NPM_ARG(s->vocab >= 1 && s->vocab <= NPM_SAMPLE_MAX_VOCAB && s->pitch >= s->vocab);
    NPM_ARG((int64_t)s->groups * s->width * 2 * s->width <= 0x7fffffff);
    NPM_ARG(s->logits != nullptr && s->cum != nullptr && s->lse != nullptr && s->parent != nullptr && s->ids != nullptr);
    NPM_ARG(s->cand_slot != nullptr && s->cand_token != nullptr && s->cand_score != nullptr);
    NPM_ARG(s->workspace != nullptr && s->workspace_bytes >= NPM_BEAM_WORKSPACE_BYTES(s->groups, s->width));
    NPM_ARG(((uintptr_t)s->workspace & 3) == 0);
    const bool vec = aligned16(s->logits) && s->pitch % 4 == 0;
    const int rows = s->groups * s->width, cands = 2 * s->width;
    snprintf(g_last_beam_kernel, sizeof(g_last_beam_kernel), "beam_rows_kernel %s G=%d W=%d V=%d row=%s", vec ? "vec" : "scalar",
             (int)s->groups, (int)s->width, (int)s->vocab, s->vocab <= NPM_SAMPLE_LDS_ROW ? "lds" : "global");
    int *ws_count = (int *)s->workspace;
    float *ws_score = (float *)(ws_count + rows);
    int *ws_token = (int *)(ws_score + (long)rows * cands);
    hipStream_t stream = npm::ctx().stream;
    if (vec)
        hipLaunchKernelGGL((beam_rows_kernel<true, false>), dim3(rows), dim3(NT), 0, stream, s->logits, (long)s->pitch, (int)s->vocab,
                           cands, (const float *)s->cum, s->lse, ws_count, ws_score, ws_token, (const int *)nullptr, (float *)nullptr);
    else
        hipLaunchKernelGGL((beam_rows_kernel<false, false>), dim3(rows), dim3(NT), 0, stream, s->logits, (long)s->pitch, (int)s->vocab,
                           cands, (const float *)s->cum, s->lse, ws_count, ws_score, ws_token, (const int *)nullptr, (float *)nullptr);
    NPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(beam_merge_kernel, dim3(s->groups), dim3(NT), 0, stream, (int)s->width, (int)s->eos, (const int *)ws_count,
                       (const float *)ws_score, (const int *)ws_token, s->cum, s->cand_slot, s->cand_token, s->cand_score, s->parent,
                       s->ids);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" int npm_logprob_rows(const npm_logprob *p) {
    NPM_REQUIRE_INIT();
    NPM_ARG(p != nullptr);
    NPM_ARG(p->rows >= 1 && p->vocab >= 1 && p->vocab <= NPM_SAMPLE_MAX_VOCAB && p->pitch >= p->vocab);
    NPM_ARG(p->top_n >= 0 && p->top_n <= MAXC);
    NPM_ARG(p->logits != nullptr && p->lse != nullptr);
    NPM_ARG(p->ids == nullptr || p->chosen != nullptr);
    NPM_ARG(p->top_n == 0 || (p->top_token != nullptr && p->top_logprob != nullptr));
    const bool vec = aligned16(p->logits) && p->pitch % 4 == 0;
    snprintf(g_last_beam_kernel, sizeof(g_last_beam_kernel), "logprob_rows_kernel %s R=%d V=%d top=%d row=%s", vec ? "vec" : "scalar",
             (int)p->rows, (int)p->vocab, (int)p->top_n, p->vocab <= NPM_SAMPLE_LDS_ROW ? "lds" : "global");
    hipStream_t stream = npm::ctx().stream;
    float *chosen = p->ids != nullptr ? p->chosen : nullptr;
    if (vec)
        hipLaunchKernelGGL((beam_rows_kernel<true, true>), dim3(p->rows), dim3(NT), 0, stream, p->logits, (long)p->pitch, (int)p->vocab,
                           (int)p->top_n, (const float *)nullptr, p->lse, (int *)nullptr, p->top_logprob, p->top_token, p->ids, chosen);
    else
        hipLaunchKernelGGL((beam_rows_kernel<false, true>), dim3(p->rows), dim3(NT), 0, stream, p->logits, (long)p->pitch, (int)p->vocab,
                           (int)p->top_n, (const float *)nullptr, p->lse, (int *)nullptr, p->top_logprob, p->top_token, p->ids, chosen);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" const char *npm_last_beam_kernel(void) { return g_last_beam_kernel; }
