// Token sampling on the device: one token per row of a [B, V] fp32 logit matrix, every row with its own temperature, top-k,
// top-p, seed and draw counter (include/npm_hip.h: npm_sample_rows states the contract; tests/sample_reference.py restates it).
//
// One block of 1024 threads per row; a row is never split over blocks, and nothing a block computes depends on another row.
// The row is copied to LDS once when it fits (NPM_SAMPLE_LDS_ROW floats = 128 KiB) and every later pass reads it there; a longer
// row is read again from global memory (L2 after the first pass).  16-byte loads when the row base and the pitch allow them,
// else one float per lane -- the same values either way, so the same result.
//
//   pass 1     the row maximum with its first index (ties by index; -0.0 == 0.0), NaN / +inf flags, the count of finite logits.
//              Greedy rows are finished here.
//   top-k cut  radix select over key(z), the order-preserving unsigned image of the float (larger z <=> larger key), in four
//              8-bit passes with an LDS histogram of counts: the exact k-th key T1 and the quota q1 of tokens equal to it that
//              are admitted -- the lowest indices among them.  Logits only: exact.
//   masses     w = floor(exp((z - zmax) * (1 / t)) * 2^32) as a 64-bit integer; every mass from here on is an integer sum, so no
//              result depends on the order in which lanes, waves or LDS atomics add.  W1 = sum over key > T1, plus q1 w(T1).
//   top-p cut  the same select with 64-bit masses (and counts) in the histogram, down to the key T2 at which the mass from the
//              top reaches the target, then a quota q2 = ceil(rest / w(T2)) of the tokens equal to T2.  Tokens equal to T1
//              enter the histogram as one lump of q1 w(T1): equal keys have equal weights, so their indices do not matter here.
//   token      in index order: each wave owns a contiguous segment and sums its kept mass and its count of tokens equal to T2;
//              the wave whose range of running mass holds the target walks its segment 64 tokens at a time with a wave prefix.
//
// A thread adds to a histogram bin through an LDS atomic, but first sums in registers while consecutive tokens of its own fall
// into one bin: the leading byte of the key is sign and exponent, where almost all tokens of a row share two or three bins.
//
// The row itself is sample_row() of npm_sample_row.h, shared with verify_rows_kernel below: npm_verify_rows samples the T + 1 rows
// of every slot of a speculative step, row r at counter draw + r, and a second, tiny kernel (one thread per slot) finds how many
// drafted tokens the samples confirm, advances the counter by the tokens emitted and appends them to the token history.

#include "npm_sample_row.h"

namespace {

char g_last_kernel[128] = "";

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

template <bool VEC>
__global__ void __launch_bounds__(NT)
sample_rows_kernel(const float *__restrict__ logits, long pitch, int vocab, const float *__restrict__ temperature,
                   const int *__restrict__ top_k, const float *__restrict__ top_p, const u64 *__restrict__ seed, u64 *__restrict__ draw,
                   const int *__restrict__ active, int *__restrict__ token, int *__restrict__ kept, float *__restrict__ prob) {
    __shared__ float row[LDS_ROW];
    __shared__ Shared sh;
    const int b = blockIdx.x;

    if (active != nullptr && active[b] == 0) {          // before any logit is loaded; draw[b] stays
        if (threadIdx.x == 0) {
            token[b] = -1;
            if (kept) kept[b] = 0;
            if (prob) prob[b] = 0.f;
        }
        return;
    }
    const u64 counter = draw[b];
    RowSample s;
    if (sample_row<VEC>(row, sh, logits + (long)b * pitch, vocab, temperature[b], top_k[b], top_p[b], seed[b], counter, s)) {
        token[b] = s.token;
        if (kept) kept[b] = s.kept;
        if (prob) prob[b] = s.prob;
        draw[b] = counter + 1;
    }
}

// Block (b, r) samples row r of slot b at counter draw[b] + r when r <= n_draft[b]; any other row gets token -1 without a load.
// draw is only read here: accept_kernel advances it.
template <bool VEC>
__global__ void __launch_bounds__(NT)
verify_rows_kernel(const float *__restrict__ logits, long pitch, int rows, int vocab, const float *__restrict__ temperature,
                   const int *__restrict__ top_k, const float *__restrict__ top_p, const u64 *__restrict__ seed,
                   const u64 *__restrict__ draw, const int *__restrict__ n_draft, int *__restrict__ token, int *__restrict__ kept,
                   float *__restrict__ prob) {
    __shared__ float row[LDS_ROW];
    __shared__ Shared sh;
    const int b = blockIdx.x / rows, r = blockIdx.x - b * rows;
    const long at = (long)blockIdx.x;

    if (r > n_draft[b]) {                               // an inactive slot (n < 0) or a row behind the draft: nothing is loaded
        if (threadIdx.x == 0) {
            token[at] = -1;
            if (kept) kept[at] = 0;
            if (prob) prob[at] = 0.f;
        }
        return;
    }
    RowSample s;
    if (sample_row<VEC>(row, sh, logits + at * pitch, vocab, temperature[b], top_k[b], top_p[b], seed[b], draw[b] + (u64)r, s)) {
        token[at] = s.token;
        if (kept) kept[at] = s.kept;
        if (prob) prob[at] = s.prob;
    }
}

// One thread per slot: a = the first row whose sample is not the drafted token (or the row behind the draft); rows behind a are
// cleared, the counter advances by the a + 1 rows that count, and the tokens emitted go behind the slot's history.
__global__ void __launch_bounds__(64)
accept_kernel(int batch, int rows, const int *__restrict__ draft, long draft_pitch, const int *__restrict__ n_draft,
              int *__restrict__ token, int *__restrict__ kept, float *__restrict__ prob, int *__restrict__ accepted,
              u64 *__restrict__ draw, int *__restrict__ history, long history_pitch, int *__restrict__ history_len, int history_cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    int n = n_draft[b];
    if (n < 0) {                                        // inactive: verify_rows_kernel wrote its row of -1; draw and history stay
        accepted[b] = 0;
        return;
    }
    if (n > rows - 1) n = rows - 1;
    int *tok = token + (long)b * rows;
    int a = 0;
    while (a < n) {
        const int d = draft[(long)b * draft_pitch + a];
        if (d < 0 || tok[a] != d) break;
        ++a;
    }
    for (int r = a + 1; r < rows; ++r) {
        tok[r] = -1;
        if (kept) kept[(long)b * rows + r] = 0;
        if (prob) prob[(long)b * rows + r] = 0.f;
    }
    accepted[b] = a;
    draw[b] += (u64)(a + 1);
    if (history != nullptr) {
        int len = history_len[b];
        if (len < 0) len = 0;
        for (int r = 0; r <= a; ++r) {
            const int id = tok[r];
            if (id >= 0 && len < history_cap) history[(long)b * history_pitch + len++] = id;
        }
        history_len[b] = len;
    }
}

}  // namespace

extern "C" int npm_sample_rows(const npm_sample *s) {
    NPM_REQUIRE_INIT();
    NPM_ARG(s != nullptr);
    NPM_ARG(s->batch >= 1 && s->vocab >= 1 && s->vocab <= NPM_SAMPLE_MAX_VOCAB && s->pitch >= s->vocab);
    NPM_ARG(s->logits != nullptr && s->temperature != nullptr && s->top_k != nullptr && s->top_p != nullptr);
    NPM_ARG(s->seed != nullptr && s->draw != nullptr && s->token != nullptr);
    const bool vec = aligned16(s->logits) && s->pitch % 4 == 0;
    snprintf(g_last_kernel, sizeof(g_last_kernel), "sample_rows_kernel %s B=%d V=%d row=%s", vec ? "vec" : "scalar", (int)s->batch,
             (int)s->vocab, s->vocab <= NPM_SAMPLE_LDS_ROW ? "lds" : "global");
    hipStream_t stream = npm::ctx().stream;
    if (vec)
        hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(s->batch), dim3(NT), 0, stream, s->logits, (long)s->pitch, (int)s->vocab,
                           s->temperature, s->top_k, s->top_p, (const u64 *)s->seed, (u64 *)s->draw, s->active, s->token, s->kept, s->prob);
    else
        hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(s->batch), dim3(NT), 0, stream, s->logits, (long)s->pitch, (int)s->vocab,
                           s->temperature, s->top_k, s->top_p, (const u64 *)s->seed, (u64 *)s->draw, s->active, s->token, s->kept, s->prob);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" int npm_verify_rows(const npm_verify *v) {
    NPM_REQUIRE_INIT();
    NPM_ARG(v != nullptr);
    NPM_ARG(v->batch >= 1 && v->rows >= 1 && v->rows <= NPM_VERIFY_MAX_ROWS);
    NPM_ARG(v->vocab >= 1 && v->vocab <= NPM_SAMPLE_MAX_VOCAB && v->pitch >= v->vocab);
    NPM_ARG((int64_t)v->batch * v->rows <= 0x7fffffff);
    NPM_ARG(v->logits != nullptr && v->temperature != nullptr && v->top_k != nullptr && v->top_p != nullptr);
    NPM_ARG(v->seed != nullptr && v->draw != nullptr && v->n_draft != nullptr && v->token != nullptr && v->accepted != nullptr);
    NPM_ARG(v->rows == 1 || (v->draft != nullptr && v->draft_pitch >= v->rows - 1));
    NPM_ARG(v->history == nullptr || (v->history_len != nullptr && v->history_cap >= 1 && v->history_pitch >= v->history_cap));
    const bool vec = aligned16(v->logits) && v->pitch % 4 == 0;
    snprintf(g_last_kernel, sizeof(g_last_kernel), "verify_rows_kernel %s B=%d rows=%d V=%d row=%s history=%d", vec ? "vec" : "scalar",
             (int)v->batch, (int)v->rows, (int)v->vocab, v->vocab <= NPM_SAMPLE_LDS_ROW ? "lds" : "global", v->history != nullptr);
    hipStream_t stream = npm::ctx().stream;
    const dim3 grid(v->batch * v->rows);
    if (vec)
        hipLaunchKernelGGL(verify_rows_kernel<true>, grid, dim3(NT), 0, stream, v->logits, (long)v->pitch, (int)v->rows, (int)v->vocab,
                           v->temperature, v->top_k, v->top_p, (const u64 *)v->seed, (const u64 *)v->draw, v->n_draft, v->token, v->kept,
                           v->prob);
    else
        hipLaunchKernelGGL(verify_rows_kernel<false>, grid, dim3(NT), 0, stream, v->logits, (long)v->pitch, (int)v->rows, (int)v->vocab,
                           v->temperature, v->top_k, v->top_p, (const u64 *)v->seed, (const u64 *)v->draw, v->n_draft, v->token, v->kept,
                           v->prob);
    NPM_CHECK_LAUNCH();
    hipLaunchKernelGGL(accept_kernel, dim3((v->batch + 63) / 64), dim3(64), 0, stream, (int)v->batch, (int)v->rows, v->draft,
                       (long)v->draft_pitch, v->n_draft, v->token, v->kept, v->prob, v->accepted, (u64 *)v->draw, v->history,
                       (long)v->history_pitch, v->history_len, (int)v->history_cap);
    NPM_CHECK_LAUNCH();
    return NPM_OK;
}

extern "C" const char *npm_last_sample_kernel(void) { return g_last_kernel; }
