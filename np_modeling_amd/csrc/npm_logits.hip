// Logit processors on the device: repetition, frequency and presence penalties, a bias list (a value of -inf bans a token) and the
// minimum-length rule for end-of-sequence, applied in place to the logit rows a sampler is about to read (include/npm_hip.h:
// npm_logits_process states the contract; tests/logits_reference.py restates it).  Only the tokens that a slot's history, draft,
// bias list and eos name are touched: the work per slot is O(history + distinct tokens * rows), never O(vocab).
//
// One block of 1024 threads per slot serves all n + 1 rows of the slot.  The slot's row of the int32 workspace (all zero between
// calls) holds, per token, what the history says about it: bits 0 .. 30 the occurrences at positions >= prompt_len, bit 31
// "occurs in the prompt part".
//
//   phase A    the block walks the history; one integer atomic per in-range token (add 1, or set bit 31).
//   phase B1   the at most 320 "extra" entries -- the bias list, the draft, eos -- sit in LDS in that order.  The first entry that
//              names a token owns it (a scan of the entries in front of it): so a token named twice in the bias list takes the
//              entry with the smallest position, and a draft or eos entry that owns a token knows it has no bias.  The owner
//              fetches and clears the token's workspace word with one atomicExch and walks r = 0 .. n with a running count of the
//              draft entries equal to its token: every (row, token) has one writer.
//   phase B2   the block walks the history again: atomicExch on the token's word.  Whoever gets a non-zero word owns the token --
//              B1 cleared the words of every extra token, so the token is in no draft, bias list or eos rule -- and applies the
//              same penalties to all n + 1 rows.  Every word the call touched is zero again.  A thread has eight exchanges, then
//              the loads of eight tokens in four rows, in flight at once: the phase is latency, not bandwidth.
//
// Integer atomics only, and no result depends on which thread wins a word: each token is handled on its own from the complete
// word.  A slot reads and writes its own rows, history, draft, parameters and workspace row only.  A slot without penalties skips
// phases A and B2 and never touches the workspace; a neutral or inactive slot returns before any of it.

#include "npm_internal.h"

#include <cmath>

namespace {

constexpr int NT = 1024;
constexpr int MAX_EXT = NPM_LOGITS_MAX_BIAS + NPM_VERIFY_MAX_ROWS;      // bias entries, rows - 1 draft entries, eos
constexpr unsigned PROMPT_BIT = 0x80000000u, COUNT_MASK = 0x7FFFFFFFu;
constexpr int TOKENS_IN_FLIGHT = 8, ROWS_IN_FLIGHT = 4;                 // phase B2: 8 exchanges, then 8 x 4 loads, per thread at once
constexpr int EXTRA_ROWS_IN_FLIGHT = 8;                                 // phase B1: one token per thread

char g_last_logits_kernel[128] = "";

// steps 1 - 3 of the contract on one logit; every operation rounded to fp32 on its own
__device__ __forceinline__ float processed(float z, bool rep_hit, float rep, bool pen_hit, float freq, float pres, unsigned count,
                                           bool has_bias, float bias) {
#pragma clang fp contract(off)
    if (rep_hit) z = z > 0.f ? z / rep : z * rep;
    if (pen_hit) {
        const float f = freq * (float)count;
        z = z - f;
        z = z - pres;
    }
    if (has_bias) z = z + bias;
    return z;
}

__global__ void __launch_bounds__(NT)
logits_process_kernel(const npm_logits p) {
    __shared__ __attribute__((aligned(16))) int ext[MAX_EXT];
    __shared__ float ext_bias[NPM_LOGITS_MAX_BIAS];
    const int b = blockIdx.x, vocab = p.vocab;

    if (p.active != nullptr && p.active[b] == 0) return;
    int n = 0;                                          // rows 0 .. n count
    if (p.n_draft != nullptr) {
        n = p.n_draft[b];
        if (n < 0) return;
        if (n > p.rows - 1) n = p.rows - 1;
    }
    const float rep = p.repetition ? p.repetition[b] : 1.f;
    const float freq = p.frequency ? p.frequency[b] : 0.f;
    const float pres = p.presence ? p.presence[b] : 0.f;
    const bool rep_on = rep > 0.f && rep < INFINITY && rep != 1.f;
    const bool pen_on = !(freq == 0.f && pres == 0.f);
    int len = 0;
    if (p.history != nullptr) {
        len = p.history_len[b];
        len = len < 0 ? 0 : (len > p.history_cap ? p.history_cap : len);
    }
    int prompt = p.prompt_len ? p.prompt_len[b] : 0;
    prompt = prompt < 0 ? 0 : (prompt > len ? len : prompt);
    int n_bias = 0;
    if (p.bias_cap > 0) {
        n_bias = p.bias_count[b];
        n_bias = n_bias < 0 ? 0 : (n_bias > p.bias_cap ? p.bias_cap : n_bias);
    }
    const long generated = (long)len - prompt;          // gen_r = generated + r
    int eos = -1;
    long min_new = 0;
    if (p.eos != nullptr && p.min_new != nullptr) {
        const int e = p.eos[b];
        min_new = p.min_new[b];
        if (e >= 0 && e < vocab && generated < min_new) eos = e;
    }
    if (!rep_on && !pen_on && n_bias == 0 && eos < 0) return;           // neutral: before any logit is loaded

    const bool counts = rep_on || pen_on;               // otherwise neither the history nor the draft matters
    const bool hist_on = counts && len > 0;
    const int n_draft = counts ? n : 0;
    const int n_ext = n_bias + n_draft + (eos >= 0 ? 1 : 0);
    const int *__restrict__ h = p.history + (long)b * p.history_pitch;
    unsigned *__restrict__ ws = (unsigned *)p.workspace + (long)b * vocab;
    float *__restrict__ z0 = p.logits + (long)b * p.rows * p.pitch;

    for (int e = threadIdx.x; e < n_ext; e += NT) {
        int tok;
        if (e < n_bias) {
            tok = p.bias_index[(long)b * p.bias_cap + e];
            ext_bias[e] = p.bias_value[(long)b * p.bias_cap + e];
        } else if (e < n_bias + n_draft) {
            tok = p.draft[(long)b * p.draft_pitch + (e - n_bias)];
        } else {
            tok = eos;
        }
        ext[e] = tok;
    }

    // ---- phase A: the history into the slot's workspace row ----
    if (hist_on) {
        for (int j = threadIdx.x; j < len; j += NT) {
            const int tok = h[j];
            if (tok >= 0 && tok < vocab) {
                if (j >= prompt) atomicAdd(&ws[tok], 1u);
                else atomicOr(&ws[tok], PROMPT_BIT);
            }
        }
        __threadfence();
    }
    __syncthreads();                                    // ext is complete; every atomic of phase A has been performed

    // ---- phase B1: the extra tokens, each by the first entry that names it ----
    for (int e = threadIdx.x; e < n_ext; e += NT) {
        const int tok = ext[e];
        if (tok < 0 || tok >= vocab) continue;
        bool first = true;                              // no entry in front of e names the token; four entries per LDS read
        for (int o = 0; o < e; o += 4) {
            const int4 x = *reinterpret_cast<const int4 *>(&ext[o]);
            first = first && x.x != tok && !(o + 1 < e && x.y == tok) && !(o + 2 < e && x.z == tok) && !(o + 3 < e && x.w == tok);
        }
        if (!first) continue;
        const unsigned w = hist_on ? atomicExch(&ws[tok], 0u) : 0u;
        const unsigned in_history = w & COUNT_MASK;
        const bool has_bias = e < n_bias;
        const float bias = has_bias ? ext_bias[e] : 0.f;
        unsigned in_draft = 0;                          // of draft[0 .. r)
        for (int r0 = 0; r0 <= n; r0 += EXTRA_ROWS_IN_FLIGHT) {       // the loads of a few rows first: they do not wait for each other
            float v[EXTRA_ROWS_IN_FLIGHT];
#pragma unroll
            for (int q = 0; q < EXTRA_ROWS_IN_FLIGHT; ++q)
                if (r0 + q <= n) v[q] = z0[(long)(r0 + q) * p.pitch + tok];
#pragma unroll
            for (int q = 0; q < EXTRA_ROWS_IN_FLIGHT; ++q) {
                const int r = r0 + q;
                if (r > n) break;
                float *__restrict__ at = z0 + (long)r * p.pitch + tok;
                const unsigned count = in_history + in_draft;
                const bool rep_hit = rep_on && (w != 0u || in_draft != 0u), pen_hit = pen_on && count != 0u;
                if (tok == eos && generated + r < min_new) *at = -INFINITY;
                else if (rep_hit || pen_hit || has_bias) *at = processed(v[q], rep_hit, rep, pen_hit, freq, pres, count, has_bias, bias);
                if (r < n_draft) in_draft += (unsigned)(ext[n_bias + r] == tok);
            }
        }
    }
    if (!hist_on) return;                               // uniform over the block
    __syncthreads();                                    // the words of every extra token are zero

    // ---- phase B2: the other tokens of the history; a thread's exchanges, then its loads, are in flight together ----
    for (int base = threadIdx.x; base < len; base += TOKENS_IN_FLIGHT * NT) {
        int tok[TOKENS_IN_FLIGHT];
        unsigned w[TOKENS_IN_FLIGHT];
#pragma unroll
        for (int u = 0; u < TOKENS_IN_FLIGHT; ++u) {
            const int j = base + u * NT;
            tok[u] = j < len ? h[j] : -1;
        }
#pragma unroll
        for (int u = 0; u < TOKENS_IN_FLIGHT; ++u) w[u] = (tok[u] >= 0 && tok[u] < vocab) ? atomicExch(&ws[tok[u]], 0u) : 0u;
        bool own[TOKENS_IN_FLIGHT], pen_hit[TOKENS_IN_FLIGHT];
        bool any = false;
#pragma unroll
        for (int u = 0; u < TOKENS_IN_FLIGHT; ++u) {    // w == 0: another thread owns the token, or B1 did
            pen_hit[u] = pen_on && (w[u] & COUNT_MASK) != 0u;
            own[u] = w[u] != 0u && (rep_on || pen_hit[u]);
            any = any || own[u];
        }
        if (!any) continue;
        for (int r0 = 0; r0 <= n; r0 += ROWS_IN_FLIGHT) {
            float v[TOKENS_IN_FLIGHT][ROWS_IN_FLIGHT];
#pragma unroll
            for (int u = 0; u < TOKENS_IN_FLIGHT; ++u)
#pragma unroll
                for (int q = 0; q < ROWS_IN_FLIGHT; ++q)
                    if (own[u] && r0 + q <= n) v[u][q] = z0[(long)(r0 + q) * p.pitch + tok[u]];
#pragma unroll
            for (int u = 0; u < TOKENS_IN_FLIGHT; ++u)
#pragma unroll
                for (int q = 0; q < ROWS_IN_FLIGHT; ++q)
                    if (own[u] && r0 + q <= n)
                        z0[(long)(r0 + q) * p.pitch + tok[u]] = processed(v[u][q], rep_on, rep, pen_hit[u], freq, pres, w[u] & COUNT_MASK, false, 0.f);
        }
    }
}

// One thread per slot: step 4 of npm_verify_rows for one token.
__global__ void __launch_bounds__(64)
history_append_kernel(int *__restrict__ history, long history_pitch, int history_cap, int *__restrict__ history_len,
                      const int *__restrict__ ids, const int *__restrict__ active, int batch) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    if (active != nullptr && active[b] == 0) return;
    const int id = ids[b];
    if (id < 0) return;
    int len = history_len[b];
    if (len < 0) len = 0;
    if (len >= history_cap) return;
    history[(long)b * history_pitch + len] = id;
    history_len[b] = len + 1;
}

}  // namespace

extern "C" int npm_logits_process(const npm_logits *p) {
    NPM_REQUIRE_INIT();
    NPM_ARG(p != nullptr);
    NPM_ARG(p->logits != nullptr && p->workspace != nullptr);
    NPM_ARG(p->batch >= 1 && p->rows >= 1 && p->rows <= NPM_VERIFY_MAX_ROWS);
    NPM_ARG(p->vocab >= 1 && p->vocab <= NPM_SAMPLE_MAX_VOCAB && p->pitch >= p->vocab);
    NPM_ARG((int64_t)p->batch * p->rows <= 0x7fffffff);
    NPM_ARG(p->n_draft != nullptr || p->rows == 1);
    NPM_ARG(p->rows == 1 || (p->draft != nullptr && p->draft_pitch >= p->rows - 1));
    NPM_ARG(p->history == nullptr || (p->history_len != nullptr && p->history_cap >= 1 && p->history_pitch >= p->history_cap));
    NPM_ARG(p->bias_cap >= 0 && p->bias_cap <= NPM_LOGITS_MAX_BIAS);
    NPM_ARG(p->bias_cap == 0 || (p->bias_index != nullptr && p->bias_value != nullptr && p->bias_count != nullptr));
    snprintf(g_last_logits_kernel, sizeof(g_last_logits_kernel), "logits_process_kernel B=%d rows=%d V=%d history=%d bias=%d",
             (int)p->batch, (int)p->rows, (int)p->vocab, p->history != nullptr, (int)p->bias_cap);
    hipLaunchKernelGGL(logits_process_kernel, dim3(p->batch), dim3(NT), 0, npm::ctx().stream, *p);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" int npm_history_append(int32_t *history, int64_t history_pitch, int32_t history_cap, int32_t *history_len,
                                  const int32_t *ids, const int32_t *active, int32_t batch) {
    NPM_REQUIRE_INIT();
    NPM_ARG(batch >= 1 && history_cap >= 1 && history_pitch >= history_cap);
    NPM_ARG(history != nullptr && history_len != nullptr && ids != nullptr);
    snprintf(g_last_logits_kernel, sizeof(g_last_logits_kernel), "history_append_kernel B=%d cap=%d", (int)batch, (int)history_cap);
    hipLaunchKernelGGL(history_append_kernel, dim3((batch + 63) / 64), dim3(64), 0, npm::ctx().stream, history, (long)history_pitch,
                       (int)history_cap, history_len, ids, active, (int)batch);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" const char *npm_last_logits_kernel(void) { return g_last_logits_kernel; }
