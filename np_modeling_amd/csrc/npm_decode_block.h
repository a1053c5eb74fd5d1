// NOT A HEADER OF ITS OWN: a fragment of two function bodies.  It has no include guard, declares nothing at file scope and compiles
// nowhere but at its two places in npm_decode.hip; include it nowhere else.
//
// The body of mha_decode_kernel (after ``constexpr bool WN = false``) and of mha_decode_window_kernel (after ``constexpr bool
// VL = true, WN = true``).  WN: sliding-window attention -- a row with upper limit ``limit`` sees keys floor <= j < limit with
// floor = max(0, limit - a.window); the key walk of the sequence starts at its first live tile ``lo`` and the split partition is
// laid from there.  It is text and not an inlined function template so that the instances without a window compile to what they
// were before the windowed ones existed (as npm_prefill_block.h does for the fp16 prefill instances).
    static_assert(VL || !PG, "a paged cache has per-sequence lengths");
    constexpr int KU = D / 16;                    // 4-element K loads per lane and tile (16 bytes; KV = _Float16: 8)
    constexpr int VW = D >= 64 ? 4 : D / 16;      // elements per V load
    constexpr int DQ = D / (16 * VW);             // V loads per lane and key
    constexpr int NS = KU >= 4 ? 4 : KU;          // score accumulation chains
    using VVec = typename VecOf<VW>::type;
    __shared__ __attribute__((aligned(16))) float s_acc[WAVES][16][D + 4];
    __shared__ float s_m[WAVES][16], s_l[WAVES][16];

    const int split = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int T = a.tokens, R = a.rows;
    // VL: block-uniform loads of the sequence's own lengths (scalar loads; nothing is stored through the scalar unit)
    const int L = VL ? kv_lens[b] : a.len;
    const int nb = VL ? (new_lens ? new_lens[b] : T) : T;
    // WN: the smallest floor of the sequence's rows (that of its first new token) and the tile that holds it: nothing below that
    // tile is loaded and no table entry below its page is read
    const int fmin = WN ? max(0, L - nb + 1 - a.window) : 0;
    const int lo = WN ? fmin / TILE : 0;
    if (VL && a.part_acc && (lo + split * a.tiles_per_split) * TILE >= L) {
        // nothing of this sequence lies in the split's key range: the empty partial (its acc is never read), before any load
        if (threadIdx.x < RB * 16) {
            const long prow = (((long)b * a.kv_heads + c) * gridDim.x + split) * (RB * 16) + threadIdx.x;
            a.part_ml[2 * prow] = -INFINITY;
            a.part_ml[2 * prow + 1] = 0.f;
        }
        return;
    }

    // this lane's query rows (one per row block): head c + (r / T) Hkv, token r % T; padding rows are zeros and never stored
    // (VL: so are the rows of tokens at and past nb, which are stored as ctx = 0, lse = -inf)
    f32x4v q[RB][KU];
    int limit[RB];                                // keys this row may see: j < limit
    int lowest[RB];                               // WN: ... and j >= lowest
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = rb * 16 + n;
        const int t = r % T, h = c + (r / T) * a.kv_heads;
        const bool live = VL ? r < R && t < nb : r < R;
        limit[rb] = live ? (a.causal ? L - nb + t + 1 : L) : 0;
        lowest[rb] = WN ? max(0, limit[rb] - a.window) : 0;
        const float *src = a.q + ((long)b * T + t) * a.q_pitch + (long)h * D + 4 * g;
#pragma unroll
        for (int u = 0; u < KU; ++u) q[rb][u] = live ? *reinterpret_cast<const f32x4v *>(src + 16 * u) : f32x4v{0.f, 0.f, 0.f, 0.f};
    }

    f32x4v acc[RB][DQ][VW];
    float m[RB], l[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        m[rb] = -INFINITY;
        l[rb] = 0.f;
#pragma unroll
        for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
            for (int e = 0; e < VW; ++e) acc[rb][dq][e] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }

    const int tiles = (L + TILE - 1) / TILE;      // VL: the sequence's own tiles within the split ranges of a.len; every tile below
    const int t_begin = lo + split * a.tiles_per_split;  // holds a key < L, so L >= 1 wherever a load is redirected to key L - 1
    const int t_end = min(tiles, t_begin + a.tiles_per_split);
    const KV *kbase = reinterpret_cast<const KV *>(a.k) + (PG ? 0L : (long)b * a.k_sb) + (long)c * D + 4 * g;
    const KV *vbase = reinterpret_cast<const KV *>(a.v) + (PG ? 0L : (long)b * a.v_sb) + (long)c * D + VW * n;

    f32x4v kr[KU];
    VVec vr[4][DQ];
    // PG: the page of a tile, a function of b, the tile index and kernel arguments only -- wave-uniform, a scalar load.  The index
    // is clamped to the page of key L - 1 (callers have L >= 1), so a look-ahead past the sequence's last tile reads a page in use
    // (WN: and from below to the page of tile lo -- pages under it may have been given back).
    auto page_of = [&](int tile) -> int {
        const int key = WN ? max(tile, lo) * TILE : tile * TILE;
        const int idx = __builtin_amdgcn_readfirstlane(min(key, L - 1) >> pg.shift);
        return pg.table[(long)b * pg.pitch + idx];
    };
    auto load_tile = [&](int tile, int page) {
        const int key0 = tile * TILE;
        const int in_page = PG ? (1 << pg.shift) - 1 : ~0;                // PG: the row within the page
        const KV *kp = kbase + (PG ? (long)page * a.k_sb : 0L) + (long)(min(key0 + n, L - 1) & in_page) * a.k_pitch;
#pragma unroll
        for (int u = 0; u < KU; ++u) kr[u] = ld_kv<NT, f32x4v>(kp + 16 * u);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const KV *vp = vbase + (PG ? (long)page * a.v_sb : 0L) + (long)(min(key0 + 4 * g + w, L - 1) & in_page) * a.v_pitch;
#pragma unroll
            for (int dq = 0; dq < DQ; ++dq) vr[w][dq] = ld_kv<NT, VVec>(vp + 16 * VW * dq);
        }
    };

    int tile = t_begin + wave;
    int page_next = 0;                            // PG: the page of tile + WAVES, looked up one step before its loads
    if (tile < t_end) {
        load_tile(tile, PG ? page_of(tile) : 0);
        if (PG) page_next = page_of(tile + WAVES);
    }
    for (; tile < t_end; tile += WAVES) {
        const int key0 = tile * TILE;
        // S^T = K Q^T
        // NS independent accumulation chains (16-byte load u feeds chain u % NS), summed pairwise: shorter dependent MFMA chains,
        // and a score that is the sum of like-signed terms (a key aligned with the query) loses half the bits a single chain of
        // D / 4 steps loses
        f32x4v sp[RB][NS], s[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int i = 0; i < NS; ++i) sp[rb][i] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) sp[rb][u % NS] = MFMA16(kr[u][e], q[rb][u][e], sp[rb][u % NS]);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) s[rb] = NS == 4 ? (sp[rb][0] + sp[rb][1]) + (sp[rb][2] + sp[rb][3]) : NS == 2 ? sp[rb][0] + sp[rb][1] : sp[rb][0];
        // V of this tile into the A operands (keys >= L zeroed: the last tile of the cache only), then the next tile's loads
        VVec va[4][DQ];
        const bool ragged = key0 + TILE > L || (WN && key0 < fmin);   // wave-uniform (WN: the first tile of the walk too)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int dq = 0; dq < DQ; ++dq) {
                va[w][dq] = vr[w][dq];
                if (ragged && (key0 + 4 * g + w >= L || (WN && key0 + 4 * g + w < fmin))) va[w][dq] = VVec(0.f);
            }
        if (tile + WAVES < t_end) load_tile(tile + WAVES, page_next);
        if (PG) page_next = page_of(tile + 2 * WAVES);

#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            // -inf by selection for keys the row does not see; then log2 units
            float x[4], tmax = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const bool seen = key0 + 4 * g + w < limit[rb] && (!WN || key0 + 4 * g + w >= lowest[rb]);
                x[w] = seen ? s[rb][w] : -INFINITY;
                tmax = fmaxf(tmax, x[w]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m[rb], tmax);                   // raw
            const float ref = m_new == -INFINITY ? 0.f : m_new * a.c; // a row with nothing visible yet: exponents stay -inf, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m[rb] * a.c - ref);   // -inf * c = -inf: 0
            m[rb] = m_new;
            float psum = 0.f;
            f32x4v p;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                p[w] = __builtin_amdgcn_exp2f(fmaf(x[w], a.c, -ref));
                psum += p[w];
            }
            l[rb] = l[rb] * alpha + psum;
#pragma unroll
            for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    f32x4v o = acc[rb][dq][e] * alpha;
#pragma unroll
                    for (int w = 0; w < 4; ++w) o = MFMA16(comp<VW>(va[w][dq], e), p[w], o);
                    acc[rb][dq][e] = o;
                }
        }
    }

    // merge the four waves in wave order, one row block at a time, and store
    const long slot = ((long)b * a.kv_heads + c) * gridDim.x + split;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        float lsum = l[rb];
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        if (rb) __syncthreads();
        if (g == 0) { s_m[wave][n] = m[rb]; s_l[wave][n] = lsum; }
        __syncthreads();
        float m_tot = -INFINITY;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) m_tot = fmaxf(m_tot, s_m[w][n]);
        const float ref = m_tot == -INFINITY ? 0.f : m_tot * a.c;
        const float weight = __builtin_amdgcn_exp2f(m[rb] * a.c - ref);   // 0 for a wave that saw nothing of this row
#pragma unroll
        for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
            for (int e = 0; e < VW; ++e)
#pragma unroll
                for (int w = 0; w < 4; ++w) s_acc[wave][n][16 * VW * dq + VW * (4 * g + w) + e] = acc[rb][dq][e][w] * weight;
        __syncthreads();
        for (int i = threadIdx.x; i < 16 * (D / 4); i += WAVES * 64) {
            const int row = i / (D / 4), d = (i % (D / 4)) * 4;
            const int r = rb * 16 + row;
            float mt = -INFINITY;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) mt = fmaxf(mt, s_m[w][row]);
            const float rf = mt == -INFINITY ? 0.f : mt * a.c;
            float lt = 0.f;
            f32x4v o{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                lt += s_l[w][row] * __builtin_amdgcn_exp2f(s_m[w][row] * a.c - rf);
                o += *reinterpret_cast<const f32x4v *>(&s_acc[w][row][d]);
            }
            if (a.part_acc) {                      // this split's (m, l, acc) of the row, padding rows included (finite: q = 0)
                const long prow = slot * (RB * 16) + r;
                *reinterpret_cast<f32x4v *>(a.part_acc + prow * D + d) = o;
                if (d == 0) { a.part_ml[2 * prow] = mt; a.part_ml[2 * prow + 1] = lt; }
            } else if (r < R) {
                const int t = r % T, h = c + (r / T) * a.kv_heads;
                const bool none = VL && mt == -INFINITY;       // no visible key: 0 and -inf by selection, not 0 / 0
                *reinterpret_cast<f32x4v *>(a.ctx + ((long)b * T + t) * a.ctx_pitch + (long)h * D + d) =
                    none ? f32x4v{0.f, 0.f, 0.f, 0.f} : o / lt;
                if (d == 0 && a.lse)
                    a.lse[((long)b * a.heads + h) * T + t] =
                        none ? -INFINITY : fmaf(a.scale, mt, (__builtin_amdgcn_logf(lt) + fmaf(-mt, a.c, rf)) * LN2);
            }
        }
    }
