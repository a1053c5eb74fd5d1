// NOT A HEADER OF ITS OWN: a fragment of four function bodies.  It has no include guard, declares nothing at file scope and compiles
// nowhere but at its four places in npm_prefill.hip; include it nowhere else.
//
// The body of mha_prefill_kernel, mha_prefill_f16_kernel and their windowed forms mha_prefill_window_kernel /
// mha_prefill_window_f16_kernel (npm_prefill.hip includes this file once inside each, after ``using KV = float`` or ``_Float16``
// and ``constexpr bool WN``; the windowed ones fix VL = true): the storage type of the cache, and whether a row sees only the
// a.window keys below its limit.  Only the base pointers, load_tile and store_tile know it.
// It is text and not an inlined function template because the fp32 kernels then compile to what they were before the fp16
// instances existed, register for register (an inlined body costs some instances two scalar registers).
    static_assert(VL || !PG, "a paged cache has per-sequence lengths");
    constexpr int KU = D / 16;                    // 16-byte K reads per lane and tile
    constexpr int VW = D >= 64 ? 4 : D / 16;      // floats per V read
    constexpr int DQ = D / (16 * VW);             // V reads per lane and key
    constexpr int NS = KU >= 4 ? 4 : KU;          // score accumulation chains
    constexpr int KP = D + 4;                     // LDS row pitch of K: lanes of one ds_read_b128 group land on distinct 16-byte slots
    constexpr int VP = D;                         //                of V: 16 lanes read one contiguous row
    constexpr int PW = 16 / sizeof(KV);           // elements of the cache in a 16-byte piece
    constexpr int F4 = TILE * D / PW;             // 16-byte pieces of one K (or V) tile in the cache
    constexpr int NLD = (F4 + WAVES * 64 - 1) / (WAVES * 64);   // ... per thread
    using VVec = typename VecOf<VW>::type;
    using Piece = typename PieceOf<KV>::type;
    __shared__ __attribute__((aligned(16))) float s_k[2][TILE][KP];
    __shared__ __attribute__((aligned(16))) float s_v[2][TILE][VP];

    const int c = blockIdx.y, b = blockIdx.z;
    const int tok0 = (int)(blockIdx.x / a.head_chunks) * a.tb, g0 = (int)(blockIdx.x % a.head_chunks) * a.gb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, g = lane >> 4;
    const int T = a.tokens;
    // block-uniform loads of the sequence's own lengths (scalar loads; nothing is stored through the scalar unit)
    const int L = VL ? kv_lens[b] : a.len;
    const int nb = VL ? (new_lens ? new_lens[b] : T) : T;

    // this lane's query row: token tok0 + r % tb of head c + (g0 + r / tb) Hkv.  A row of the tile that is no row of the call
    // (past the group, past T) is never stored; a row of a padded token (t >= nb) is stored as ctx = 0, lse = -inf.
    const int r = wave * 16 + n;
    const int t = tok0 + r % a.tb, gi = g0 + r / a.tb;
    const int h = c + gi * a.kv_heads;
    const bool exists = r < a.gb * a.tb && gi < a.group && t < T;
    const bool live = exists && t < nb;
    const int limit = live ? max(0, min(a.causal ? L - nb + t + 1 : L, L)) : 0;     // keys this row may see: j < limit
    const int lowest = WN ? max(0, limit - a.window) : 0;                           // WN: ... and j >= lowest

    // the block's walk: key tiles below the largest limit of its rows (its last live token's).  tok0 >= nb: no live row, no tile,
    // no load -- the rows are stored below and the block is done.
    const int seen = tok0 < nb ? max(0, min(a.causal ? L - nb + min(tok0 + a.tb, nb) : L, L)) : 0;
    const int tiles = (seen + TILE - 1) / TILE;   // every walked tile holds a key < L, so L >= 1 wherever a load is redirected
    int wlimit = limit;                           // the largest limit of this wave's rows (wave-uniform)
    wlimit = max(wlimit, __shfl_xor(wlimit, 1));
    wlimit = max(wlimit, __shfl_xor(wlimit, 2));
    wlimit = max(wlimit, __shfl_xor(wlimit, 4));
    wlimit = max(wlimit, __shfl_xor(wlimit, 8));
    wlimit = __builtin_amdgcn_readfirstlane(wlimit);
    // WN: the smallest floor of the block's live rows (its first token's) -- the walk starts at its tile, V rows below it are
    // zeroed on their way into LDS, no table entry below its page is read -- and of this wave's live rows (wave-uniform): the
    // wave skips the tiles wholly below it
    const int bmin = WN && tok0 < nb ? max(0, L - nb + tok0 + 1 - a.window) : 0;
    const int tile0 = WN ? bmin / TILE : 0;
    int wlow = 0;
    if (WN) {
        wlow = live ? lowest : 0x7fffffff;
        wlow = min(wlow, __shfl_xor(wlow, 1));
        wlow = min(wlow, __shfl_xor(wlow, 2));
        wlow = min(wlow, __shfl_xor(wlow, 4));
        wlow = min(wlow, __shfl_xor(wlow, 8));
        wlow = __builtin_amdgcn_readfirstlane(wlow);
    }

    f32x4v q[KU];
    {
        const float *src = a.q + ((long)b * T + (live ? t : 0)) * a.q_pitch + (long)(live ? h : 0) * D + 4 * g;
#pragma unroll
        for (int u = 0; u < KU; ++u) q[u] = live ? *reinterpret_cast<const f32x4v *>(src + 16 * u) : f32x4v{0.f, 0.f, 0.f, 0.f};
    }

    f32x4v acc[DQ][VW];
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int e = 0; e < VW; ++e) acc[dq][e] = f32x4v{0.f, 0.f, 0.f, 0.f};

    const KV *kbase = reinterpret_cast<const KV *>(a.k) + (PG ? 0L : (long)b * a.k_sb) + (long)c * D;
    const KV *vbase = reinterpret_cast<const KV *>(a.v) + (PG ? 0L : (long)b * a.v_sb) + (long)c * D;

    // staging: piece i of a tile is columns PW (i % (D / PW)) .. + PW - 1 of key i / (D / PW), in flight in the storage type
    Piece kst[NLD], vst[NLD];
    auto load_tile = [&](int tile) {
        const int key0 = tile * TILE;
        long koff = 0, voff = 0;
        int in_page = ~0;
        if (PG) {
            // the page of the tile, a function of b, the tile index and kernel arguments only: wave-uniform, a scalar load.
            // key0 < L, so the entry is one of the sequence's own pages.
            const int page = pg.table[(long)b * pg.pitch + (__builtin_amdgcn_readfirstlane(key0) >> pg.shift)];
            koff = (long)page * a.k_sb;
            voff = (long)page * a.v_sb;
            in_page = (1 << pg.shift) - 1;
        }
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int key = key0 + piece / (D / PW), col = (piece % (D / PW)) * PW;
                const long row = min(key, L - 1) & in_page;
                kst[i] = *reinterpret_cast<const Piece *>(kbase + koff + row * a.k_pitch + col);
                vst[i] = *reinterpret_cast<const Piece *>(vbase + voff + row * a.v_pitch + col);
                if (key >= L || (WN && key < bmin)) vst[i] = Piece(KV(0));   // the last tile of the sequence only (WN: and the first of the walk)
                // (WN: a wave whose rows have a higher floor than bmin multiplies p = 0 by the V rows in bmin .. its floor as they
                // are.  That is sound only because every row in bmin .. L - 1 is a live row of the sequence -- the cache gives back
                // nothing at or above the floor of the sequence's first new token.  A reclaim bound above that needs a zero here.)
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int piece = i * WAVES * 64 + (int)threadIdx.x;
            if (F4 % (WAVES * 64) == 0 || piece < F4) {
                const int row = piece / (D / PW), col = (piece % (D / PW)) * PW;
                if constexpr (PW == 4) {
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col]) = kst[i];
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col]) = vst[i];
                } else {
                    // halves -> fp32, exactly, as two 16-byte stores each
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col]) = __builtin_convertvector(__builtin_shufflevector(kst[i], kst[i], 0, 1, 2, 3), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_k[buf][row][col + 4]) = __builtin_convertvector(__builtin_shufflevector(kst[i], kst[i], 4, 5, 6, 7), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col]) = __builtin_convertvector(__builtin_shufflevector(vst[i], vst[i], 0, 1, 2, 3), f32x4v);
                    *reinterpret_cast<f32x4v *>(&s_v[buf][row][col + 4]) = __builtin_convertvector(__builtin_shufflevector(vst[i], vst[i], 4, 5, 6, 7), f32x4v);
                }
            }
        }
    };

    if (tiles > tile0) {
        load_tile(tile0);
        store_tile(tile0 & 1);
    }
    __syncthreads();
    for (int tile = tile0; tile < tiles; ++tile) {
        const int key0 = tile * TILE, buf = tile & 1;
        if (tile + 1 < tiles) load_tile(tile + 1);                    // in flight during the products below
        if (key0 < wlimit && (!WN || key0 + TILE > wlow)) {           // wave-uniform: some row of this wave sees a key of the tile
            // S^T = K Q^T: NS independent accumulation chains, summed pairwise (as in mha_decode_kernel)
            f32x4v sp[NS], s;
#pragma unroll
            for (int i = 0; i < NS; ++i) sp[i] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int u = 0; u < KU; ++u) {
                const f32x4v kr = *reinterpret_cast<const f32x4v *>(&s_k[buf][n][16 * u + 4 * g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) sp[u % NS] = MFMA16(kr[e], q[u][e], sp[u % NS]);
            }
            s = NS == 4 ? (sp[0] + sp[1]) + (sp[2] + sp[3]) : NS == 2 ? sp[0] + sp[1] : sp[0];
            // -inf by selection for keys the row does not see; then log2 units
            float x[4], tmax = -INFINITY;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                x[w] = key0 + 4 * g + w < limit && (!WN || key0 + 4 * g + w >= lowest) ? s[w] : -INFINITY;
                tmax = fmaxf(tmax, x[w]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m, tmax);                       // raw
            const float ref = m_new == -INFINITY ? 0.f : m_new * a.c; // a row with nothing visible yet: exponents stay -inf, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m * a.c - ref);    // -inf * c = -inf: 0
            m = m_new;
            float psum = 0.f;
            f32x4v p;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                p[w] = __builtin_amdgcn_exp2f(fmaf(x[w], a.c, -ref));
                psum += p[w];
            }
            l = l * alpha + psum;
            // O^T += V^T P^T
#pragma unroll
            for (int dq = 0; dq < DQ; ++dq) {
                VVec va[4];
#pragma unroll
                for (int w = 0; w < 4; ++w) va[w] = *reinterpret_cast<const VVec *>(&s_v[buf][4 * g + w][16 * VW * dq + VW * n]);
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    f32x4v o = acc[dq][e] * alpha;
#pragma unroll
                    for (int w = 0; w < 4; ++w) o = MFMA16(comp<VW>(va[w], e), p[w], o);
                    acc[dq][e] = o;
                }
            }
        }
        // the other buffer was last read for tile - 1, before the barrier that ended that step
        if (tile + 1 < tiles) store_tile(buf ^ 1);
        __syncthreads();
    }

    // every wave stores its own rows: register w of acc[dq][e] is column d = 16 VW dq + VW (4 g + w) + e of row n
    float lt = l;
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    if (!exists) return;
    const bool none = m == -INFINITY;             // no visible key: 0 and -inf by selection, not 0 / 0
    const float rf = none ? 0.f : m * a.c;
    float *dst = a.ctx + ((long)b * T + t) * a.ctx_pitch + (long)h * D;
#pragma unroll
    for (int dq = 0; dq < DQ; ++dq)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            VVec o;
#pragma unroll
            for (int e = 0; e < VW; ++e) put<VW>(o, e, none ? 0.f : acc[dq][e][w] / lt);
            *reinterpret_cast<VVec *>(dst + 16 * VW * dq + VW * (4 * g + w)) = o;
        }
    if (g == 0 && a.lse)
        a.lse[((long)b * a.heads + h) * T + t] = none ? -INFINITY : fmaf(a.scale, m, (__builtin_amdgcn_logf(lt) + fmaf(-m, a.c, rf)) * LN2);
