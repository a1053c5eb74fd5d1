// Drafts for speculative decoding by prompt lookup (include/npm_hip.h: npm_ngram_draft states the rule; tests/spec_reference.py
// restates it as a plain loop).  The continuation of an earlier occurrence of a sequence's last n tokens is proposed as its next
// tokens: integers only, so the draft is the same on every run.
//
// One block of 256 threads per slot.  For n from nmax down to nmin the block walks every start j of an earlier occurrence, thread
// t taking j = t, t + 256, ...: neighbouring threads read neighbouring words, and the history is read once per n.  A thread keeps
// the largest match whose continuation is whole (j + n + m_max <= L) and the smallest match of all; the block reduces both with
// integer max / min, so the choice does not depend on which thread found what.

#include "npm_internal.h"

namespace {

constexpr int NT = 256, NW = NT / 64;

char g_last_kernel[128] = "";

__global__ void __launch_bounds__(NT)
ngram_draft_kernel(const int *__restrict__ history, long history_pitch, int history_cap, const int *__restrict__ history_len,
                   const int *__restrict__ limit, int max_draft, int nmax, int nmin, int *__restrict__ chunk, int *__restrict__ n_new) {
    __shared__ int red_full[NW], red_any[NW];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int *__restrict__ h = history + (long)b * history_pitch;
    int *__restrict__ out = chunk + (long)b * (max_draft + 1);
    int len = history_len[b];
    if (len > history_cap) len = history_cap;           // nothing past the capacity is ever read
    const int lim = limit ? limit[b] : max_draft;
    if (len <= 0 || lim < 0) {
        for (int i = threadIdx.x; i <= max_draft; i += NT) out[i] = -1;
        if (threadIdx.x == 0) n_new[b] = 0;
        return;
    }
    const int m_max = lim < max_draft ? lim : max_draft;
    int start = -1;                                     // j + n of the chosen occurrence: where its continuation begins
    if (m_max > 0) {
        for (int n = nmax; n >= nmin; --n) {
            if (len < n + 1) continue;
            int tail[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) tail[i] = i < n ? h[len - n + i] : 0;
            int full = -1, any = 0x7fffffff;
            for (int j = threadIdx.x; j <= len - n - 1; j += NT) {
                bool same = true;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < n) same = same && h[j + i] == tail[i];
                if (same) {
                    if (j + n + m_max <= len && j > full) full = j;
                    if (j < any) any = j;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int of = __shfl_xor(full, off, 64), oa = __shfl_xor(any, off, 64);
                full = of > full ? of : full;
                any = oa < any ? oa : any;
            }
            __syncthreads();                            // the previous n's readers of red_* are done
            if (lane == 0) {
                red_full[wave] = full;
                red_any[wave] = any;
            }
            __syncthreads();
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                full = red_full[w] > full ? red_full[w] : full;
                any = red_any[w] < any ? red_any[w] : any;
            }
            if (any != 0x7fffffff) {                    // the same in every thread: it comes from LDS
                start = (full >= 0 ? full : any) + n;
                break;
            }
        }
    }
    int m = 0;
    if (start >= 0) m = m_max < len - start ? m_max : len - start;
    for (int i = threadIdx.x; i <= max_draft; i += NT) out[i] = i == 0 ? h[len - 1] : (i <= m ? h[start + i - 1] : -1);
    if (threadIdx.x == 0) n_new[b] = 1 + m;
}

}  // namespace

extern "C" int npm_ngram_draft(const int32_t *history, int64_t history_pitch, int32_t history_cap, const int32_t *history_len,
                               const int32_t *limit, int32_t batch, int32_t max_draft, int32_t nmax, int32_t nmin, int32_t *chunk,
                               int32_t *n_new) {
    NPM_REQUIRE_INIT();
    NPM_ARG(batch >= 1 && max_draft >= 0 && max_draft <= NPM_VERIFY_MAX_ROWS - 1);
    NPM_ARG(nmin >= 1 && nmax >= nmin && nmax <= NPM_DRAFT_MAX_NGRAM);
    NPM_ARG(history_cap >= 1 && history_pitch >= history_cap);
    NPM_ARG(history != nullptr && history_len != nullptr && chunk != nullptr && n_new != nullptr);
    snprintf(g_last_kernel, sizeof(g_last_kernel), "ngram_draft_kernel B=%d T=%d ngram=%d..%d cap=%d", (int)batch, (int)max_draft,
             (int)nmax, (int)nmin, (int)history_cap);
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(batch), dim3(NT), 0, npm::ctx().stream, history, (long)history_pitch, (int)history_cap,
                       history_len, limit, (int)max_draft, (int)nmax, (int)nmin, chunk, n_new);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" const char *npm_last_draft_kernel(void) { return g_last_kernel; }
