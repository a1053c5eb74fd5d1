"""Multi-head attention on the fp32 MFMA GEMM (reference layers/attentions.py:11-199).

Every einsum of the reference is a GEMM view, addressed in place -- no transposes are
materialised:

* projections ``'...ab,cdb->...acd'`` (attentions.py:88-100): [B*S, F] x w[H*D, F]^T, bias in
  the epilogue; q/k/v stay in the reference's [B, S, H, D] layout;
* ``QK^T`` / ``PV`` and their four gradients (attentions.py:103-112,146-162): GEMMs batched
  over (B, H) whose operands are head slices of [B, S, H, D] (row pitch H*D, batch strides
  (S*H*D, D));
* the context ("values") is written as [B, Sq, H, Dv] so that the output projection
  ``'...abc,...dac->...bd'`` (attentions.py:116) is a plain [B*Sq, H*Dv] x wo[F, H*Dv]^T GEMM
  (the reference's own cache is head-major [B, H, Sq, Dv]; this one is private state);
* softmax forward/backward with the 1/sqrt(Dk) scaling fused (attentions.py:104,150-155).

Where the head size allows (Dk == Dv in {16, 32, 64, 128}, exact-fp32 math) the score / softmax / context chain and
its gradient run as ONE kernel each (``npm_mha_core_fwd`` / ``npm_mha_core_bwd``, csrc/npm_attn.hip): the
[B, H, Sq, Skv] probabilities are never stored, only a log-sum-exp per query row.  The GEMM composition above stays
as the path for other head sizes and for the split-bf16 math modes.

Masks.  The reference tests ``if mask:`` (attentions.py:84,106), which raises ValueError for any array of more than
one element, and its backward raises NotImplementedError (attentions.py:152-153): masked attention is unreachable
there.  This layer implements the evident intent instead: ``mask`` is a boolean array broadcastable to
[B, H, Sq, Skv]; excluded positions get ``-inf`` before the softmax (``np.where(mask, scaled, -inf)``) and
probability exactly 0, in forward and backward; a query row with no position left yields NaN, as that ``np.where``
followed by the reference's softmax would.  A ``device.AttnMask`` made once (``AttnMask(mask, B, H, Sq, Skv)``) may be
passed instead of the array: its bytes and its tile summary (which lets the kernels skip tiles without an allowed
position) then stay on the device between steps.

Parameter layouts are the reference's: wq/wk [H, Dk, H*Dk], wv [H, Dv, H*Dv], wo [H*Dk, H, Dv],
bq/bk [H, Dk], bv [H, Dv], bo [H*Dk] (attentions.py:46-65), drawn in that order.

Grouped-query attention (``num_kv_heads=Hkv``, the reference's ``gqa_fwd``, layers/attentions_test.py:267-358): the
Hq = ``num_heads`` query heads share Hkv key / value heads, so wk [Hkv, Dk, F], wv [Hkv, Dv, Fv], bk [Hkv, Dk] and
bv [Hkv, Dv] (Dk = F / Hq, Dv = Fv / Hq as in MHA; same draw order).  Query head h = g * Hkv + c reads K / V head
c = h % Hkv (the reference reshapes q to [B, Sq, Hq / Hkv, Hkv, Dk] and pairs its Hkv axis with k's heads).  The fused
kernels take the grouping as an argument (``npm_mha_core_*_grouped``); the GEMM composition runs one batched GEMM over
(B, Hkv) per group g -- query head g * Hkv + c is a column offset g * Hkv * D of the [B, S, Hq, D] tensors -- and sums
the dK / dV of the groups in the residual epilogue, in the order g = 0, 1, ...  ``num_kv_heads=None`` (or ``num_heads``)
is multi-head attention, run exactly as without the keyword.

Incremental decoding (inference; the reference has none: ``# TODO: support cache``, layers/transformer.py:120).
``make_cache(batch, capacity)`` returns a ``device.KVCache`` with Hkv heads; ``forward(x, cache=cache)`` projects the T new
tokens (one packed GEMM where the parameters allow), appends their K / V rows behind the ``cache.length`` valid ones and attends
causally over all of them -- T is the whole prompt or 1.  Cross-attention projects K / V once with ``fill_cache(cache, key,
value)`` and then ``forward(x, cache=cache)`` attends to the whole frozen cache.  Nothing is saved for a backward.

Ragged batches.  ``forward(x, cache=cache, new_lengths=n)``: ``x`` [B, T, F] is padded on the right and sequence b brings n[b] <= T
tokens (0: it rides along); their K / V go behind the sequence's own ``cache.lengths[b]`` rows and row t < n[b] sees keys
j <= lengths[b] + t.  ``fill_cache(cache, key, value, lengths=...)`` does the same for a padded cross-attention memory.  Valid rows
equal what the sequence gives alone at batch 1; padded rows are unspecified but finite; nothing at or past a sequence's length
enters a result.  Lengths that are all equal take exactly the calls they took without the keyword.

Which kernel attends (``cached_route``; ``_cached_path`` names the path of the last cached forward).  A call is in the
*per-sequence form* when ``new_lengths`` is given or the cache is ragged, paged or windowed -- its entry points read the lengths
(and the block table) on the device -- else in the *uniform form*.  R = (Hq / Hkv) T is the number of score rows per K / V head;
the first row of the table that applies decides:

====  ====================================================  ==================  ====================================================
rule  when                                                  path                runs
====  ====================================================  ==================  ====================================================
1     the cache has a ``window`` (never frozen: ValueError;  ``decode`` where    the windowed entry points, f32 and f16 alike,
      exact-fp32 kernels only: NotImplementedError)         rule 2's predicate  whatever the switches say, a prefill from empty
                                                            holds, else         included: nothing else knows the window
                                                            ``prefill``
2     ``mha_decode_supported(Dk, R, Dv)``; the uniform      ``decode``          ``npm_mha_decode_fwd`` (csrc/npm_decode.hip: one
      form also needs T <= length (the kernel's contract)                       block per K / V head serves its group of query
                                                                                heads, keys split over blocks), ``_varlen``,
                                                                                ``_paged`` or ``_f16`` by the cache
3     the switch of the cache's type is on                  ``prefill``         ``npm_mha_prefill_fwd[_f16]`` (csrc/npm_prefill.hip)
      (``device.PREFILL_KERNEL``, NPM_PREFILL_KERNEL=1,                         over the cache in place, through the block table:
      for f32; ``device.PREFILL_KERNEL_F16``,                                   no gathered K / V, no mask, no copy per sequence.
      NPM_PREFILL_KERNEL_F16=1, for f16; both off by                            A half-precision cache is attended to as stored,
      default) and ``mha_prefill_supported(Dk, Dv)`` --                         a prefill from empty included
      except a uniform f32 call whose fresh projection is
      the whole cache (a prefill from empty)
4     per-sequence form, an f16 cache, or                   ``fused_masked``    the fused training forward with a mask.  Uniform
      ``mha_core_supported(Dk, Dv)`` in any math mode                           f32: K / V are the fresh projection (from empty),
                                                                                the cache itself (full, or batch 1) or a copy of
                                                                                the valid rows, and the mask is the causal rule
                                                                                (none at T = 1).  Otherwise: the fresh projection
                                                                                only for an f32 cache empty in every sequence,
                                                                                else ``cache.gather``; the mask is built from the
                                                                                lengths and its tile summary skips what lies past
                                                                                them
5     otherwise (uniform f32, other head sizes)             ``gemm``            the GEMM composition on the valid rows; no masked
                                                                                softmax, so a causal chunk runs row by row
6     rule 2 or 3 in the per-sequence form and              ``decode_shared``   the same call over the rows behind the prefix,
      ``cache.attend_prefix_rows(n, causal)`` is not 0      ``prefill_shared``  ``npm_mha_prefix_fwd`` and ``npm_attn_combine``
      (a forked paged cache, ``device.SHARED_PREFIX``)                          (``KVCache.attend``)
====  ====================================================  ==================  ====================================================

The kernels of rules 1 - 3 run the exact-fp32 MFMA only, so under a split math mode the ``*_supported`` predicates are false and
the call falls to rule 4 or 5, which honour the mode.  Before anything is launched ``forward`` refuses what no rule serves: a
per-sequence or f16 call whose head sizes neither the decode kernel nor the fused forward takes (NotImplementedError: the GEMM
composition has no masked softmax).  With every switch off each call sequence is what it was before the switch existed.

Rotary position embeddings (``rope_base``, default None: the reference has no positional encoding and neither has this layer).
With a positive ``rope_base`` the projected q and k are rotated in place by their positions -- element i < Dk / 2 of a head pairs
with element i + Dk / 2, angle p * rope_base ** (-2 i / Dk); Dk must be even, v is never rotated -- by ``npm_rope``
(csrc/npm_rope.hip) from cos / sin tables made on the host (``device.RopeTable``): ONE launch on the packed projection (the q and
k heads are adjacent in every row), two on separate tensors, each side counted from position 0.  It runs in front of the fused
core or the GEMM composition in every math mode (exact fp32 element-wise work); ``_q`` / ``_k`` are saved rotated, and the backward
applies the transposed rotation to dq / dk between the attention gradient and the in-projection gradient GEMMs.  With a cache the
new tokens are rotated at the positions ``cache.lengths[b] + t`` BEFORE ``cache.append`` -- the scalar ``cache.length`` for a
uniform contiguous cache, else the ``before`` row of the cache's device length mirror, which the append then finds uploaded -- so
the cache, the decode and prefill kernels and the fp16 rounding see rotated rows and need nothing of their own; ``make_cache``
sizes the tables for ``capacity``.  A frozen cross-attention cache has no query position: ``fill_cache`` and a cached forward over
one raise NotImplementedError.  ``rope_base=None`` launches nothing and allocates nothing: every call sequence is what it was.

One launch in front of the cached attention (opt-in: ``device.FUSED_ROPE_APPEND``, NPM_FUSED_ROPE_APPEND=1, or the layer's own
``_fused_rope_append``, which ``models.CausalLM`` sets; off by default).  Where the projection is packed and Dk == Dv, the rotation
and the two appends above are ONE call, ``cache.append_rotated`` (npm_rope_kv_append, csrc/npm_rope_append.hip): the packed buffer
is left rotated and the cache holds the same bits as after the three launches, with or without ``rope_base``.  Separate projections
(rebound parameters, Dk != Dv) keep the three launches.

Half-precision weight copies (opt-in).  ``half_weights()`` returns a ``device.HalfWeights`` snapshot of wq / wk / wv (one half
buffer when they are adjacent, so the packed projection stays one product) and wo; ``forward(x, cache=cache, weights=hw)`` reads
the projections of that cached forward from it: ``npm_sgemm_skinny_w16`` over the halves in place where the skinny-M GEMM
applies, else the halves converted back and ``npm_sgemm`` -- the rounded weights either way, whatever M is.  Biases stay fp32; the
cache, whatever its layout or type, does not look at the weights.  ``weights=`` without ``cache=`` raises ValueError; a snapshot
whose parameter was rebound since raises RuntimeError (``hw.refresh()``).  Without the keyword nothing changes.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np

from np_modeling_amd import device as D
from np_modeling_amd import parallel
from np_modeling_amd.device import Mat
from np_modeling_amd.layers import activations, layer

_PARAMS = ('_wq', '_wk', '_wv', '_wo', '_bq', '_bk', '_bv', '_bo')
_IN_PROJECTIONS = (('_wq', '_bq'), ('_wk', '_bk'), ('_wv', '_bv'))


def _from(x: D.DeviceArray, offset: int) -> D.DeviceArray:
    """``x`` entered ``offset`` elements later (a head-slice operand of the grouped composition), spanning to its end."""
    return x if offset == 0 else x.flat_view(offset, [x.size - offset])


def _gemm_attention(q: Mat, k: Mat, v: Mat, ctx: Mat, dims, scale: float) -> D.DeviceArray:
    """ctx = softmax(scale q k^T) v out of GEMMs: attention[b, h] = q_h k_h^T, scores = softmax(attention / sqrt(dk)) in place,
    context[b, :, h, :] = scores[b, h] v_h; returns the scores [B, H, rows, keys].  One GEMM batched over (B, Hkv) per group g:
    query heads g Hkv .. g Hkv + Hkv - 1 with K / V heads 0 .. Hkv - 1 (one group when not grouped).  ``q`` / ``ctx``
    [B, rows, H, D] and ``k`` / ``v`` [B, keys, Hkv, D] are named by first element, row pitch and batch stride."""
    b, h, hkv, rows, keys, dk, dv = dims
    plane = rows * keys
    scores = D.empty([b, h, rows, keys])
    groups = [Mat(_from(scores, g * hkv * plane), keys, h * plane, plane) for g in range(h // hkv)]
    for g, s_g in enumerate(groups):
        D.gemm(rows, keys, dk, Mat(q.ptr + 4 * g * hkv * dk, q.ld, q.s0, dk), Mat(k.ptr, k.ld, k.s0, dk), s_g, trans_b=True,
               batch=(b, hkv))
    D.softmax_fwd(scores, scale, out=scores)
    for g, s_g in enumerate(groups):
        D.gemm(rows, dv, keys, s_g, Mat(v.ptr, v.ld, v.s0, dv), Mat(ctx.ptr + 4 * g * hkv * dv, ctx.ld, ctx.s0, dv), batch=(b, hkv))
    return scores


def cached_route(cache, heads: int, tokens: int, causal: bool, fresh_whole: bool, per_sequence: bool, n=None) -> str:
    """The path of a cached forward (the table in the module docstring), decided without effects: ``'decode'``, ``'prefill'``,
    ``'fused_masked'`` or ``'gemm'``, the first two with ``'_shared'`` behind them when ``cache`` reads a shared prefix once.
    ``tokens`` query rows per sequence of ``heads`` heads; ``causal`` False: ``cache`` is frozen; ``fresh_whole``: the fresh
    projection is the whole cache (every sequence was empty); ``per_sequence``: the call has per-sequence lengths -- ``n`` [B]
    new tokens each -- because ``new_lengths`` was given or the cache is ragged, paged or windowed.  A windowed cache that
    neither kernel can serve raises here, before anything is launched."""
    dk, dv, rows = cache.key_dim, cache.value_dim, heads // cache.kv_heads * tokens
    if cache.window is not None:
        # no gather, mask or GEMM composition knows the window: the two windowed kernels, whatever the switches say
        if not causal:
            raise ValueError('a windowed cache is a self-attention cache: it cannot be frozen for cross-attention')
        if not D.mha_prefill_supported(dk, dv):
            raise NotImplementedError('a windowed cache needs the exact-fp32 decode and prefill kernels (head sizes Dk == Dv in '
                                      '{16, 32, 64, 128}, math mode f32)')
        return 'decode' if D.mha_decode_supported(dk, rows, dv) else 'prefill'
    f16 = cache.dtype != 'f32'
    shared = '_shared' if per_sequence and cache.attend_prefix_rows(n, causal) else ''
    if D.mha_decode_supported(dk, rows, dv) and (per_sequence or tokens <= cache.length):    # (the uniform kernel's contract: L >= T)
        return 'decode' + shared
    if (D.PREFILL_KERNEL_F16 if f16 else D.PREFILL_KERNEL) and D.mha_prefill_supported(dk, dv) \
            and not (fresh_whole and not per_sequence and not f16):      # there the fused forward reads the projection in place
        return 'prefill' + shared
    if per_sequence or f16 or D.mha_core_supported(dk, dv, any_math=True):
        return 'fused_masked'            # (_forward_cached has refused the head sizes it does not take)
    return 'gemm'


class MultiHeadAttention(layer.StatefulLayer):
    def __init__(self, num_heads: int, *args, num_kv_heads: Optional[int] = None, rope_base: Optional[float] = None,
                 window: Optional[int] = None, **kwargs):
        super().__init__(*args, **kwargs)
        if window is not None and (isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1):
            raise ValueError(f'window must be None or an integer >= 1, got {window!r}')
        self._window = None if window is None else int(window)              # None: every cache this layer makes is unwindowed
        self._num_heads = num_heads
        self._num_kv_heads = num_heads if num_kv_heads is None else num_kv_heads
        if rope_base is not None and not rope_base > 0:
            raise ValueError(f'rope_base must be None or a positive number, got {rope_base!r}')
        self._rope_base = None if rope_base is None else float(rope_base)   # None: no rotation, no table, no launch
        self._rope = None                                                   # device.RopeTable, made at the first use
        self._softmax = activations.Softmax()
        self._cached_forward = False    # the last forward ran with a cache: it saved nothing a backward could use
        self._fused_rope_append = None  # None: device.FUSED_ROPE_APPEND decides; True / False: this layer's own choice (models.CausalLM)
        self._cached_path = None        # 'decode' | 'prefill' | 'fused_masked' | 'gemm' (| 'decode_shared' | 'prefill_shared'): how the last cached forward attended

    def initialize(self, query, key=None, value=None, *args, **kwargs) -> None:
        # query [B, Sq, H*Dk]; key [B, Skv, H*Dk]; value [B, Skv, H*Dv]
        if key is None:
            key = query
        if value is None:
            value = key
        assert query.shape[0] == key.shape[0]
        assert query.shape[2] == key.shape[2]
        assert query.shape[0] == value.shape[0]
        assert key.shape[1] == value.shape[1]
        self._seq_len_q = query.shape[1]
        self._seq_len_kv = key.shape[1]
        h, hkv = self._num_heads, self._num_kv_heads
        assert hkv >= 1 and h % hkv == 0, f'num_heads {h} is not a multiple of num_kv_heads {hkv}'
        assert key.shape[2] % h == 0
        self._key_dim = dk = key.shape[2] // h
        if self._rope_base is not None and dk % 2:
            raise ValueError(f'rope_base: rotary position embedding needs an even head size Dk, got {dk}')
        assert value.shape[2] % h == 0
        self._value_dim = dv = value.shape[2] // h
        # Draw order wq, wk, wv, wo, bq, bk, bv, bo (attentions.py:46-65).  When the three in-projections
        # have one head size they are stored back to back (views of one [H + 2 Hkv, D, F] buffer), so that
        # self-attention can run them as ONE GEMM; rebinding any of them (weight binders do) just
        # falls back to three GEMMs.
        draws = [self._initializer([h, dk, h * dk]), self._initializer([hkv, dk, h * dk]),
                 self._initializer([hkv, dv, h * dv])]
        wo = self._initializer([h * dk, h, dv])
        bias_draws = [self._initializer([h, dk]), self._initializer([hkv, dk]), self._initializer([hkv, dv])]
        bo = self._initializer([h * dk])
        if dk == dv:
            packed_w, packed_b = D.empty([h + 2 * hkv, dk, h * dk]), D.empty([h + 2 * hkv, dk])
            for i, (name, bname) in enumerate((('_wq', '_bq'), ('_wk', '_bk'), ('_wv', '_bv'))):
                first, heads = (0, h) if i == 0 else (h + (i - 1) * hkv, hkv)       # head rows of the packed buffer
                setattr(self, name, packed_w.flat_view(first * dk * h * dk, [heads, dk, h * dk]).set(draws[i]))
                setattr(self, bname, packed_b.flat_view(first * dk, [heads, dk]).set(bias_draws[i]))
        else:
            self._wq, self._wk, self._wv = (D.as_device(a) for a in draws)
            self._bq, self._bk, self._bv = (D.as_device(a) for a in bias_draws)
        self._wo = D.as_device(wo)
        self._bo = D.as_device(bo)
        # one arena in the order backward produces the gradients (dbo, dwo, the in-projection weights, their biases)
        self._pack_parameters(self._segments())

    def _params_adjacent(self) -> bool:
        """wq/wk/wv (and bq/bk/bv) still back to back in memory?  Checked at EVERY use: parameters may be
        rebound between a forward and its backward (weight binders, tests)."""
        w = [self._param(p) for p in ('_wq', '_wk', '_wv')]
        b = [self._param(p) for p in ('_bq', '_bk', '_bv')]
        return (w[0].shape[1:] == w[1].shape[1:] and w[1].shape == w[2].shape and
                w[1].ptr == w[0].ptr + w[0].nbytes and w[2].ptr == w[1].ptr + w[1].nbytes and
                b[1].ptr == b[0].ptr + b[0].nbytes and b[2].ptr == b[1].ptr + b[1].nbytes)

    def _packed_qkv(self, query, key, value) -> bool:
        """Self-attention with the in-projection parameters adjacent in memory: one GEMM makes q, k and v."""
        if not (query is key and key is value) or self._key_dim != self._value_dim or not D.PACK_QKV:
            return False
        return self._params_adjacent()

    def _numel(self) -> int:
        return sum(self._param(p).size for p in _PARAMS) + 4 * len(_PARAMS)

    def _rope_table(self, rows: int) -> D.RopeTable:
        """The layer's cos / sin tables, covering positions 0 .. rows - 1 (``rope_base`` is set)."""
        if self._rope is None:
            self._rope = D.RopeTable(self._key_dim, self._rope_base)
        return self._rope.ensure(rows)

    def _rotate(self, packed, q: D.DeviceArray, k: D.DeviceArray, b: int, sq: int, skv: int, inverse: bool = False) -> None:
        """Rotary position embedding on q [B, Sq, H, Dk] and k [B, Skv, Hkv, Dk] in place, each counted from position 0 (or
        their gradients: ``inverse``).  ``packed``: they are the first H + Hkv heads of the rows of one [B, S, H + 2 Hkv, D]
        buffer ``q``, which one launch rotates; the V heads behind them are not touched."""
        h, hkv, dk = self._num_heads, self._num_kv_heads, self._key_dim
        table = self._rope_table(max(sq, skv))
        if packed:
            D.rope(Mat(q, (h + 2 * hkv) * dk), b, sq, h + hkv, dk, table, inverse=inverse)
        else:
            D.rope(Mat(q, h * dk), b, sq, h, dk, table, inverse=inverse)
            D.rope(Mat(k, hkv * dk), b, skv, hkv, dk, table, inverse=inverse)

    def _segments(self):
        """Parameters in the order ``_backward_impl`` produces their gradients (device.ParamArena segments)."""
        return [[(self, '_bo')], [(self, '_wo')], [(self, '_wq'), (self, '_wk'), (self, '_wv')],
                [(self, '_bq'), (self, '_bk'), (self, '_bv')]]

    # -- forward -------------------------------------------------------------------------
    def half_weights(self) -> D.HalfWeights:
        """A snapshot of wq / wk / wv / wo as IEEE fp16 for ``forward(x, cache=cache, weights=...)``: of the weights as they are
        NOW (``device.HalfWeights``; ``refresh()`` after the parameters changed)."""
        if not self._initialized:
            raise RuntimeError('half_weights: the layer has no parameters yet (run one forward, or bind weights, first)')
        return D.HalfWeights([(self, p) for p in ('_wq', '_wk', '_wv', '_wo')])

    def _project_in(self, query, key, value, rows: Optional[int] = None, weights: Optional[D.HalfWeights] = None,
                    skinny_ok: bool = False):
        """The in-projections [rows, F] x w[H*D, F]^T + b of those of ``query`` / ``key`` / ``value`` [B, S, F] that are not None:
        ``(Mats, arrays, packed)`` with q [B, S, H, Dk], k [B, S, Hkv, Dk], v [B, S, Hkv, Dv] (None where not asked for) as GEMM
        operands and as the arrays behind them.  ``packed``: ONE GEMM made all three as parts of one [B, S, H + 2 Hkv, D] buffer
        (``_packed_qkv``) -- k and v are that buffer entered F and F + Hkv*Dk elements later, spanning to its end, with its row
        pitch; otherwise one GEMM each.  ``rows``: only the first ``rows`` rows of a batch of one.  ``weights``: the fp16 copies
        to read (RuntimeError if a parameter was rebound since the snapshot); ``skinny_ok``: a decode step (``device.gemm``)."""
        h, hkv, dk, dv = self._num_heads, self._num_kv_heads, self._key_dim, self._value_dim
        inputs = (query, key, value)
        halves = [None if weights is None or x is None else weights.view(self, w) for x, (w, _) in zip(inputs, _IN_PROJECTIONS)]
        if query is not None and self._packed_qkv(query, key, value):
            b, s, f = query.shape
            width = f + 2 * hkv * dk
            qkv = D.empty([b, s, h + 2 * hkv, dk])
            # (adjacent parameters at unchanged addresses were adjacent when the snapshot was taken: so are their halves)
            D.gemm(b * s, width, f, Mat(query, f), Mat(self._param('_wq'), f, half=halves[0]), Mat(qkv, width), trans_b=True,
                   bias=self._param('_bq'), skinny_ok=skinny_ok)
            arrays = [qkv, _from(qkv, f), _from(qkv, f + hkv * dk)]
            return [Mat(a, width) for a in arrays], arrays, True
        mats, arrays = [None, None, None], [None, None, None]
        for i, (x, (heads, d), (w, bias)) in enumerate(zip(inputs, ((h, dk), (hkv, dk), (hkv, dv)), _IN_PROJECTIONS)):
            if x is not None:
                b, s, f = x.shape
                s = s if rows is None else rows
                arrays[i] = D.empty([b, s, heads, d])
                mats[i] = Mat(arrays[i], heads * d)
                D.gemm(b * s, heads * d, f, Mat(x, f), Mat(self._param(w), f, half=halves[i]), mats[i], trans_b=True,
                       bias=self._param(bias), skinny_ok=skinny_ok)
        return mats, arrays, False

    def forward(self, query, key=None, value=None, mask=None, cache=None, new_lengths=None, weights=None):
        if weights is not None and cache is None:
            raise ValueError('weights= (half-precision weight copies) serves the cached forward of incremental decoding: it needs cache=')
        query = D.as_device(query)
        if cache is not None:
            if key is not None or value is not None or mask is not None:
                raise ValueError('with a cache, forward takes the new query tokens only: cross-attention keys and values go '
                                 'through fill_cache(cache, key, value), and the causal rule is implied')
            return self._forward_cached(query, cache, new_lengths=new_lengths, weights=weights)
        if new_lengths is not None:
            raise ValueError('new_lengths counts the tokens a ragged batch adds to a cache: it needs cache=')
        key = query if key is None else D.as_device(key)
        value = key if value is None else D.as_device(value)
        return self._forward_impl(query, key, value, mask=mask)

    def _forward_impl(self, query, key, value, residual: Optional[D.DeviceArray] = None, mask=None):
        h, dk, dv = self._num_heads, self._key_dim, self._value_dim
        hkv = self._num_kv_heads
        grouped = hkv != h
        b, sq, f = query.shape
        skv = key.shape[1]
        fv = value.shape[2]
        assert f == h * dk and key.shape == (b, skv, f) and value.shape[:2] == (b, skv) and fv == h * dv
        wo, bo = self._param('_wo'), self._param('_bo')
        self._query, self._key, self._value = query, key, value
        self._cached_forward = False
        if mask is not None and not isinstance(mask, D.AttnMask) and np.ndim(mask) == 0 and not mask:   # `if mask:` false (attentions.py:84,106)
            mask = None
        if isinstance(mask, D.AttnMask):                               # made once by the caller (its bytes and tile summary stay
            assert mask.dims == (b, h, sq, skv), f'AttnMask made for {mask.dims}, used with {(b, h, sq, skv)}'   # on the device)
            self._mask = mask
        else:
            self._mask = None if mask is None else D.AttnMask(mask, b, h, sq, skv)
        core = D.mha_core_supported(dk, dv, any_math=self._mask is not None)
        if self._mask is not None and not core:
            raise NotImplementedError('masked attention needs head sizes Dk == Dv in {16, 32, 64, 128} (fused kernels)')
        self._core = core

        (mq, mk, mv), (q, k, v), packed = self._project_in(query, key, value)
        self._packed = packed
        if self._rope_base is not None:                                 # q and k are saved rotated: what the backward needs
            self._rotate(packed, q, k, b, sq, skv)
        self._q, self._k, self._v = q, k, v
        pq, pk, pv = self._pitches = (mq.ld, mk.ld, mv.ld)              # row pitches of q, k, v

        self._scale = 1.0 / math.sqrt(dk)
        if core:
            # scores, softmax and context in one kernel; what the backward needs is the log-sum-exp per row
            ctx, self._lse, self._raw_scores = D.mha_core_fwd(
                mq, mk, mv, (b, h, sq, skv, dk), self._scale, self._mask,
                save_scores=D.attn_save_scores(dk), kv_heads=hkv if grouped else None)
            self._softmax._y = self._attention_scores = None
        else:
            ctx = D.empty([b, sq, h, dv])                                # [B, Sq, H, Dv]
            scores = _gemm_attention(Mat(q, pq, sq * pq), Mat(k, pk, skv * pk), Mat(v, pv, skv * pv), Mat(ctx, h * dv, sq * h * dv),
                                     (b, h, hkv, sq, skv, dk, dv), self._scale)
            self._softmax._y = self._attention_scores = scores
        self._context = ctx

        # output projection: [B*Sq, H*Dv] x wo[F, H*Dv]^T + bo (+ skip connection)
        out = D.empty([b, sq, f])
        D.gemm(b * sq, f, h * dv, Mat(ctx, h * dv), Mat(wo, h * dv), Mat(out, f), trans_b=True, bias=bo,
               residual=None if residual is None else Mat(residual, f))
        return out

    # -- incremental decoding ------------------------------------------------------------------
    def make_cache(self, batch: int, capacity: int, page_size: Optional[int] = None, pages: Optional[int] = None,
                   dtype: str = 'f32', layers: int = 1) -> D.KVCache:
        """An empty key / value cache for ``batch`` sequences of up to ``capacity`` tokens (Hkv heads: grouped-query attention
        keeps its smaller cache).  The layer must have its parameters (one forward, or a weight binder).

        ``page_size`` (a power of two >= 16): a ``device.PagedKVCache`` -- rows live in a pool of ``pages`` pages (None: enough
        for every sequence to reach ``capacity``) that sequences take as they grow and give back with ``cache.release(b)``.

        ``dtype`` 'f16': K / V rows are stored as IEEE fp16 (half the bytes; see ``device.KVCache``) and every attention over the
        cache sees them as stored.  It needs the head sizes the decode kernel takes.

        A layer made with ``window=W`` gives the cache that window (``device.KVCache(window=)``): cached forwards run the windowed
        decode kernel (up to its row limit, ``device.mha_decode_supported``) or the windowed prefill kernel, never a gather, a mask or a GEMM
        composition, so it needs their head sizes too; a paged cache then gives pages back as its sequences move on.

        ``layers`` N > 1: one cache for a stack of N layers of this geometry (``device.KVCache(layers=)``); this layer's cached
        forward then takes ``cache.layer(i)``, between the ``begin`` and ``commit`` of the model that owns the stack."""
        if not self._initialized:
            raise RuntimeError('make_cache: the layer has no parameters yet (run one forward, or bind weights, first)')
        if dtype not in D.KV_ITEMSIZE:
            raise ValueError(f"make_cache: dtype must be one of {sorted(D.KV_ITEMSIZE)}, got {dtype!r}")
        dk, dv = self._key_dim, self._value_dim
        if dtype != 'f32' and not (dk == dv and dk in (16, 32, 64, 128)):
            raise NotImplementedError(f'an {dtype} cache needs head sizes Dk == Dv in {{16, 32, 64, 128}} (the decode kernel and the '
                                      f'fused masked forward on the gathered rows), got {dk} / {dv}')
        if self._window is not None and not (dk == dv and dk in (16, 32, 64, 128)):
            raise ValueError(f'a windowed cache needs head sizes Dk == Dv in {{16, 32, 64, 128}} (the windowed decode and prefill '
                             f'kernels), got {dk} / {dv}')
        if self._rope_base is not None:
            self._rope_table(capacity)                                   # sized once: decoding up to the capacity never grows it
        if page_size is None:
            if pages is not None:
                raise ValueError('make_cache: pages= sizes the pool of a paged cache: it needs page_size=')
            return D.KVCache(batch, capacity, self._num_kv_heads, dk, dv, dtype=dtype, window=self._window, layers=layers)
        if not (D.mha_decode_supported(dk, self._num_heads // self._num_kv_heads, dv) or D.mha_core_supported(dk, dv, any_math=True)):
            raise NotImplementedError('a paged cache needs head sizes Dk == Dv in {16, 32, 64, 128} (the decode kernel or '
                                      'the fused masked forward); the GEMM composition has no masked softmax')
        return D.PagedKVCache(batch, capacity, self._num_kv_heads, dk, dv, page_size=page_size, pages=pages, dtype=dtype,
                              window=self._window, layers=layers)

    def fill_cache(self, cache: D.KVCache, key, value=None, lengths=None) -> D.KVCache:
        """Cross-attention: project ``key`` / ``value`` [B, Skv, F] once into ``cache`` and freeze it; ``forward(x, cache=cache)``
        then attends to all of it, not causally, and appends nothing.  ``lengths`` [B]: the memory is padded on the right and
        sequence b has only ``lengths[b]`` rows; the rest is neither stored nor attended to."""
        if self._rope_base is not None:
            raise NotImplementedError('fill_cache with rope_base: a cross-attention chunk has no defined query position over a '
                                      'frozen cache; rotary position embedding is for self-attention caches')
        key = D.as_device(key)
        value = key if value is None else D.as_device(value)
        h, dk, dv = self._num_heads, self._key_dim, self._value_dim
        b, skv, f = key.shape
        fv = value.shape[2]
        assert f == h * dk and value.shape[:2] == (b, skv) and fv == h * dv
        cache.reset()
        cache.room(skv, lengths)                                         # ValueError before anything is launched
        (_, k, v), _, _ = self._project_in(None, key, value)
        cache.append(k, v, skv, lengths)
        cache.frozen = True
        return cache

    def fill_slot(self, cache: D.KVCache, b: int, key, rows: int) -> None:
        """Cross-attention: sequence ``b`` of a filled cache is replaced by the first ``rows`` rows of the memory ``key`` [1, Skv, F]
        (``TransformerDecoder.admit``).  K is projected and written, then V: one projection is live at a time."""
        cache.write_slot(b, self._project_in(None, key, None, rows=rows)[0][1], None, rows)
        cache.write_slot(b, None, self._project_in(None, None, key, rows=rows)[0][2], rows)

    def _forward_cached(self, query: D.DeviceArray, cache: D.KVCache, residual: Optional[D.DeviceArray] = None, new_lengths=None,
                        weights: Optional[D.HalfWeights] = None):
        """``forward(query, cache=cache)``: self-attention over a growing cache (causal), or cross-attention over a frozen one.
        ``new_lengths`` [B]: ``query`` is padded on the right and sequence b brings n[b] <= T tokens.  The projections are
        row-wise, so the padded rows (which must be finite) ride along; their K / V are not stored and their outputs are
        unspecified but finite.  ``weights``: the projections read the fp16 copies of this snapshot (every weight this call
        multiplies by must be in it)."""
        h, hkv, dk, dv = self._num_heads, self._num_kv_heads, self._key_dim, self._value_dim
        b, t, f = query.shape
        assert f == h * dk and (cache.batch, cache.kv_heads, cache.key_dim, cache.value_dim) == (b, hkv, dk, dv), \
            f'cache made for {(cache.batch, cache.kv_heads, cache.key_dim, cache.value_dim)}, used with {(b, hkv, dk, dv)}'
        cross = cache.frozen
        rope = self._rope_base is not None
        if rope and cross:
            raise NotImplementedError('a frozen (cross-attention) cache with rope_base: the query chunk has no defined position')
        new_lengths = cache.new_lengths(t, new_lengths)                  # None when it says what T says
        # a paged cache has no [B, capacity, Hkv, D] tensor to hand to the uniform paths: it always takes the per-sequence route,
        # whose kernels read through the block table (uniform lengths are bitwise the uniform entry point there)
        # (so does a windowed cache: its entry points exist in the per-sequence form only)
        ragged = new_lengths is not None or cache.ragged or cache.paged or cache.window is not None
        if (ragged or cache.dtype != 'f32') and not (D.mha_decode_supported(dk, h // hkv * t, dv) or D.mha_core_supported(dk, dv, any_math=True)):
            raise NotImplementedError('per-sequence lengths need head sizes Dk == Dv in {16, 32, 64, 128} (the decode kernel or '
                                      'the fused masked forward); the GEMM composition has no masked softmax')
        if not cross:
            cache.room(t, new_lengths)                                   # ValueError before anything is launched
        elif cache.max_length == 0:
            raise ValueError('the frozen cache is empty: fill_cache(cache, key, value) first')
        before = cache.lengths.copy()
        self._cached_forward = True
        fresh = None                                                     # the new tokens' own (k, v) Mats, self-attention only
        if cross:
            (q, _, _), _, _ = self._project_in(query, None, None, weights=weights, skinny_ok=True)
        else:
            # ONE GEMM over M = B T rows makes q, k and v where the parameters are adjacent; K and V rows then go into the cache
            # straight out of the packed buffer (npm_kv_append reads with its row pitch)
            (q, *fresh), _, packed = self._project_in(query, query, query, weights=weights, skinny_ok=True)
            fuse = D.FUSED_ROPE_APPEND if self._fused_rope_append is None else self._fused_rope_append
            if fuse and packed and dk == dv:
                # the rotation and the two appends in ONE launch on the packed buffer (npm_rope_kv_append): the same bits in the
                # buffer and in the cache as the three launches below; q is left rotated for the attention
                cache.append_rotated(q, h, t, new_lengths, self._rope_table(cache.max_length + t) if rope else None)
            elif rope:
                # q and the fresh k rows at positions lengths[b] + t, BEFORE they are stored: the cache, its kernels and the
                # fp16 rounding see rotated rows and need nothing of their own.  Per-sequence positions are the `before` row of
                # the length mirror; the append below finds the same numbers there and uploads nothing.
                if cache._scalar_call(new_lengths):
                    at, at_lens = cache.length, None
                else:
                    at, at_lens = 0, cache._device_lengths(cache.lengths, cache._counts(t, new_lengths))[0]
                table = self._rope_table(cache.max_length + t)
                if packed:                                               # q and k heads are adjacent in every row: one launch
                    D.rope(q, b, t, h + hkv, dk, table, at, at_lens)
                else:
                    D.rope(q, b, t, h, dk, table, at, at_lens)
                    D.rope(fresh[0], b, t, hkv, dk, table, at, at_lens)
            if not (fuse and packed and dk == dv):
                cache.append(fresh[0], fresh[1], t, new_lengths)
        ctx = self._attend(q, cache, t, not cross, fresh, before, new_lengths, ragged)
        out = D.empty([b, t, f])
        D.gemm(b * t, f, h * dv, Mat(ctx, h * dv), Mat(self._param('_wo'), h * dv, half=None if weights is None else weights.view(self, '_wo')),
               Mat(out, f), trans_b=True, bias=self._param('_bo'), residual=None if residual is None else Mat(residual, f), skinny_ok=True)
        return out

    def _attend(self, q: Mat, cache: D.KVCache, t: int, causal: bool, fresh, before: np.ndarray, new_lengths,
                per_sequence: bool) -> D.DeviceArray:
        """ctx [B, T, Hq, Dv] of the T query rows ``q`` over the valid rows of ``cache``, by the path ``cached_route`` names; sets
        ``_cached_path``.  ``before`` [B] rows were valid before this call; ``fresh``: the new tokens' own (k, v), or None over
        a frozen cache.  ``per_sequence``: sequence b brings ``new_lengths[b]`` (None: T) of the T padded rows, and row
        t < n[b] sees keys j <= before[b] + t (causal) or j < lengths[b] (frozen)."""
        h, scale = self._num_heads, 1.0 / math.sqrt(self._key_dim)
        n = cache._counts(t, new_lengths) if per_sequence else None
        fresh_whole = fresh is not None and not before.any()
        path = cached_route(cache, h, t, causal, fresh_whole, per_sequence, n)
        self._cached_path = path
        if path == 'fused_masked':
            return self._fused_masked(q, cache, t, causal, fresh if fresh_whole else None, before, n)
        if path == 'gemm':
            return self._gemm_rows(q, cache, t, causal)
        return cache.attend(q, h, t, scale, causal, new_lengths=n, kernel=path.partition('_')[0])[0]

    def _fused_masked(self, q: Mat, cache: D.KVCache, t: int, causal: bool, fresh, before: np.ndarray, n) -> D.DeviceArray:
        """The fused training forward with the causal rule (or the lengths) as a mask.  It addresses K / V as [B, L, Hkv, D];
        ``fresh``: the new tokens' own projection when they are the whole cache, ``n``: None in the uniform form."""
        h, hkv, dk = self._num_heads, self._num_kv_heads, self._key_dim
        b, scale = cache.batch, 1.0 / math.sqrt(dk)
        if n is None and cache.dtype == 'f32':
            # uniform fp32: the projection in place (a prefill from empty), the cache itself when it is full or holds one
            # sequence, else a copy of the valid rows; the mask is the causal rule, which one query row does not need
            keys = cache.length
            if fresh is not None:
                k, v = fresh
            elif keys == cache.capacity or b == 1:
                k, v = Mat(cache.k, hkv * dk), Mat(cache.v, hkv * self._value_dim)
            else:
                k, v = (Mat(self._valid_rows(x, keys), hkv * dk) for x in (cache.k, cache.v))
            mask = D.AttnMask(np.arange(keys)[None, :] <= (keys - t + np.arange(t))[:, None], b, h, t, keys) if causal and t > 1 else None
        else:
            # per-sequence lengths, or a half-precision cache (attended to AS STORED: never the fresh projection): the lengths
            # as a mask [B, 1, T, keys], whose tile summary skips what lies past them.  K / V: the fresh projection when every
            # sequence started empty (keys = T; the rows of padded tokens are masked), else the valid rows gathered with zeros
            # behind them (P = 0 times stale memory could be NaN).
            n = cache._counts(t, n)
            if fresh is not None and cache.dtype == 'f32':
                keys, (k, v) = t, fresh
            else:
                keys = cache.max_length
                k, v = (Mat(x, hkv * dk) for x in cache.gather(keys))
            limit = (before[:, None] + np.arange(t)[None, :] + 1) if causal else np.broadcast_to(cache.lengths[:, None], (b, t))
            limit = np.where(np.arange(t)[None, :] < n[:, None], limit, 0)
            visible = np.arange(keys)[None, None, :] < limit[:, :, None]                      # [B, T, keys]
            visible[:, :, 0] |= ~visible.any(axis=2)                     # a row without a key is given key 0: finite, unspecified
            mask = D.AttnMask(visible[:, None], b, h, t, keys)
        return D.mha_core_fwd(q, k, v, (b, h, t, keys, dk), scale, mask, kv_heads=hkv if hkv != h else None)[0]

    def _gemm_rows(self, q: Mat, cache: D.KVCache, t: int, causal: bool) -> D.DeviceArray:
        """Other head sizes, uniform fp32: the GEMM composition on the valid rows, batched over (B, Hkv) per group as in
        ``_forward_impl``.  It has no masked softmax, so a causal chunk runs one query row at a time, each over the keys it sees."""
        h, hkv, dk, dv = self._num_heads, self._num_kv_heads, self._key_dim, self._value_dim
        b, length, scale = cache.batch, cache.length, 1.0 / math.sqrt(dk)
        ctx = D.empty([b, t, h, dv])
        pk, pv, cap = hkv * dk, hkv * dv, cache.capacity
        for first, rows, keys in ([(i, 1, length - t + i + 1) for i in range(t)] if causal and t > 1 else [(0, t, length)]):
            _gemm_attention(Mat(q.ptr + 4 * first * q.ld, q.ld, t * q.ld), Mat(cache.k, pk, cap * pk), Mat(cache.v, pv, cap * pv),
                            Mat(ctx.ptr + 4 * first * h * dv, h * dv, t * h * dv), (b, h, hkv, rows, keys, dk, dv), scale)
        return ctx

    @staticmethod
    def _valid_rows(x: D.DeviceArray, length: int) -> D.DeviceArray:
        """The first ``length`` rows of every batch entry of a cache tensor [B, capacity, Hkv, D], contiguous."""
        b, cap, hkv, d = x.shape
        out = D.empty([b, length, hkv, d])
        D.kv_gather(x, out, length)
        return out

    # -- backward --------------------------------------------------------------------------
    _NO_BACKWARD = ('backward after a forward with a cache: incremental decoding is inference only and saves none of the '
                    'activations a backward needs -- run forward without a cache first')

    def backward(self, dy, optimizer_):
        if self._cached_forward:
            raise RuntimeError(self._NO_BACKWARD)
        with parallel.grad_scope(self._numel(), self._arena) as scope:
            return self._backward_impl(D.as_device(dy), optimizer_, scope)

    def _backward_impl(self, dy, optimizer_, scope, *, sum_inputs: bool = False, sum_kv: bool = False,
                       residual: Optional[D.DeviceArray] = None):
        """Returns (dquery, dkey, dvalue) (attentions.py:199), or -- for a composite that feeds
        one tensor as query, key and value -- their sum (+ residual) accumulated in the GEMM
        epilogues when ``sum_inputs`` is set (reference layers/transformer.py:84-85).  ``sum_kv``
        (cross-attention over one kv tensor): returns (dquery (+ residual), dkey + dvalue), the second
        accumulated in its GEMMs' epilogues (transformer.py:186)."""
        if self._cached_forward:
            raise RuntimeError(self._NO_BACKWARD)
        h, dk, dv = self._num_heads, self._key_dim, self._value_dim
        hkv = self._num_kv_heads
        grouped, fkv, fvkv = hkv != h, hkv * dk, hkv * dv
        query, key, value = self._query, self._key, self._value
        q, k, v, scores, ctx = self._q, self._k, self._v, self._attention_scores, self._context
        b, sq, f = dy.shape
        skv, fv = key.shape[1], value.shape[2]
        wq, wk, wv, wo = (self._param(p) for p in ('_wq', '_wk', '_wv', '_wo'))
        m_q, m_kv = b * sq, b * skv

        # output projection (attentions.py:129-136)
        # dbo = sum over (batch, position) of dy: taken from the dy tiles of the weight-gradient GEMM
        dbo = scope.take([f], owner=(self, '_bo'))
        dwo = scope.take(wo.shape, owner=(self, '_wo'))
        D.gemm(f, h * dv, m_q, Mat(dy, f), Mat(ctx, h * dv), Mat(dwo, h * dv), trans_a=True, asum_out=dbo)   # dy^T ctx
        dctx = D.empty([b, sq, h, dv])
        # dy wo.  At head size 128 a column block of that GEMM's tiles IS a head: its epilogue also takes the row terms
        # -scale * (dctx_i . ctx_i) the fused backward needs (the Jacobian-vector product of Softmax.backward,
        # activations.py:42-45 / attentions.py:150-155), [H, B * Sq], instead of a pass over dctx and ctx behind it.
        neg_delta = None
        if self._core and dv == 128 and D.ATTN_ROWDOT and D.attn_save_scores(dk) and f % 16 == 0 and sq % 4 == 0 \
                and D._C.current_math() == 'f32':
            rows = D.zeros([h, m_q])
            try:
                D.gemm(m_q, h * dv, f, Mat(dy, f), Mat(wo, h * dv), Mat(dctx, h * dv), rowdot=(Mat(ctx, h * dv), rows, -self._scale))
                neg_delta = (rows, sq, m_q)
            except D._C.NpmError as err:                   # operands the row-dot instance does not take (alignment): the plain product
                if err.code != 10003:
                    raise
        if neg_delta is None:
            D.gemm(m_q, h * dv, f, Mat(dy, f), Mat(wo, h * dv), Mat(dctx, h * dv))

        packed = self._packed
        pq, pk, pv = self._pitches
        # dbq/dbk/dbv = sum over (batch, position) of dq/dk/dv (attentions.py:186-188): taken from the dq/dk/dv
        # tiles of the in-projection weight-gradient GEMMs below
        width = f + 2 * fkv                 # packed: row width of [B, S, H + 2 Hkv, D]
        if packed:      # gradients of the packed parameters and of q/k/v live in packed buffers too
            dw_all = scope.take([h + 2 * hkv, dk, f], owner=(self, '_wq'))
            db_all = scope.take([h + 2 * hkv, dk], owner=(self, '_bq'))
            dwq, dwk, dwv = (dw_all.flat_view(first * dk * f, [heads, dk, f]) for first, heads in ((0, h), (h, hkv), (h + hkv, hkv)))
            dbq, dbk, dbv = (db_all.flat_view(first * dk, [heads, dk]) for first, heads in ((0, h), (h, hkv), (h + hkv, hkv)))
            dqkv = D.empty([b, sq, h + 2 * hkv, dk])
            dq, dk_, dv_ = dqkv, dqkv.flat_view(f, [dqkv.size - f]), dqkv.flat_view(f + fkv, [dqkv.size - f - fkv])
            gq = gk = gv = width
        else:
            dwq, dwk, dwv = (scope.take(w_.shape, owner=(self, a_)) for w_, a_ in ((wq, '_wq'), (wk, '_wk'), (wv, '_wv')))
            dbq, dbk, dbv = (scope.take([n_, d_], owner=(self, a_)) for n_, d_, a_ in ((h, dk, '_bq'), (hkv, dk, '_bk'), (hkv, dv, '_bv')))
            dq, dk_, dv_ = D.empty([b, sq, h, dk]), D.empty([b, skv, hkv, dk]), D.empty([b, skv, hkv, dv])
            gq, gk, gv = h * dk, fkv, fvkv
        if self._core:
            # attentions.py:146-162 in one kernel: P is recomputed from the saved log-sum-exp, tile by tile
            D.mha_core_bwd(Mat(q, pq), Mat(k, pk), Mat(v, pv), ctx, self._lse, dctx, Mat(dq, gq), Mat(dk_, gk),
                           Mat(dv_, gv), (b, h, sq, skv, dk), self._scale, self._mask, self._raw_scores, neg_delta=neg_delta,
                           kv_heads=hkv if grouped else None)
        elif grouped:
            self._grouped_composition_bwd(dctx, dq, dk_, dv_, (gq, gk, gv))
        else:
            # softmax @ V (attentions.py:146-148)
            # dP = dctx_h v_h^T followed by the softmax backward and the 1/sqrt(dk) of attentions.py:150-155.
            # The row term sum_j dP_ij P_ij equals dctx_i . ctx_i (ctx = P v), so it is one cheap row-dot and the
            # rest, datt = scale * P * (dP - row term), is elementwise: it rides the epilogue of the dP GEMM
            # and dP itself never goes to memory.
            datt = D.empty([b, h, sq, skv])
            if D.FUSE_SOFTMAX_BWD:
                delta = D.attn_rowdot(dctx, ctx)
                D.gemm(sq, skv, dv, Mat(dctx, h * dv, sq * h * dv, dv), Mat(v, pv, skv * pv, dv),
                       Mat(datt, skv, h * sq * skv, sq * skv), trans_b=True, batch=(b, h), alpha=self._scale,
                       softmax_bwd=(Mat(scores, skv), delta))
            else:
                D.gemm(sq, skv, dv, Mat(dctx, h * dv, sq * h * dv, dv), Mat(v, pv, skv * pv, dv),
                       Mat(datt, skv, h * sq * skv, sq * skv), trans_b=True, batch=(b, h))        # dctx_h v_h^T
                D.softmax_bwd(scores, datt, self._scale, out=datt)
            D.gemm(skv, dv, sq, Mat(scores, skv, h * sq * skv, sq * skv), Mat(dctx, h * dv, sq * h * dv, dv),
                   Mat(dv_, gv, skv * gv, dv), trans_a=True, batch=(b, h))                        # P_h^T dctx_h
            # Q K^T (attentions.py:161-162)
            D.gemm(sq, dk, skv, Mat(datt, skv, h * sq * skv, sq * skv), Mat(k, pk, skv * pk, dk),
                   Mat(dq, gq, sq * gq, dk), batch=(b, h))                                        # datt_h k_h
            D.gemm(skv, dk, sq, Mat(datt, skv, h * sq * skv, sq * skv), Mat(q, pq, sq * pq, dk),
                   Mat(dk_, gk, skv * gk, dk), trans_a=True, batch=(b, h))                        # datt_h^T q_h

        if self._rope_base is not None:     # dq, dk are gradients of the ROTATED q, k: the transposed rotation takes them back
            self._rotate(packed, dq, dk_, b, sq, skv, inverse=True)
        # in-projections (attentions.py:167-188): dw = dproj^T x ; dx = dproj w
        if packed:
            D.gemm(width, f, m_q, Mat(dqkv, width), Mat(query, f), Mat(dw_all, f), trans_a=True, asum_out=db_all)
        else:
            D.gemm(h * dk, f, m_q, Mat(dq, gq), Mat(query, f), Mat(dwq, f), trans_a=True, asum_out=dbq)
            D.gemm(fkv, f, m_kv, Mat(dk_, gk), Mat(key, f), Mat(dwk, f), trans_a=True, asum_out=dbk)
            D.gemm(fvkv, fv, m_kv, Mat(dv_, gv), Mat(value, fv), Mat(dwv, fv), trans_a=True, asum_out=dbv)
        # every parameter gradient of this layer now exists: start exchanging them (data parallel) under
        # the remaining input-gradient GEMMs
        scope.flush()
        if sum_inputs:
            assert query is key and key is value
            total = D.empty([b, sq, f])
            res = None if residual is None else Mat(residual, f)
            if packed and self._params_adjacent():      # dq wq + dk wk + dv wv: one contraction over the packed (H + 2 Hkv) D axis
                D.gemm(m_q, f, width, Mat(dqkv, width), Mat(wq, f), Mat(total, f), residual=res)
            else:
                D.gemm(m_q, f, h * dk, Mat(dq, gq), Mat(wq, f), Mat(total, f), residual=res)
                D.gemm(m_kv, f, fkv, Mat(dk_, gk), Mat(wk, f), Mat(total, f), residual=Mat(total, f))
                D.gemm(m_kv, fv, fvkv, Mat(dv_, gv), Mat(wv, fv), Mat(total, fv), residual=Mat(total, fv))
            result = total
        elif sum_kv:
            assert key is value and fv == f
            dquery, dkv = D.empty([b, sq, f]), D.empty([b, skv, f])
            D.gemm(m_q, f, h * dk, Mat(dq, gq), Mat(wq, f), Mat(dquery, f),
                   residual=None if residual is None else Mat(residual, f))
            D.gemm(m_kv, f, fkv, Mat(dk_, gk), Mat(wk, f), Mat(dkv, f))
            D.gemm(m_kv, f, fvkv, Mat(dv_, gv), Mat(wv, f), Mat(dkv, f), residual=Mat(dkv, f))
            result = (dquery, dkv)
        else:
            assert residual is None
            dquery, dkey, dvalue = D.empty([b, sq, f]), D.empty([b, skv, f]), D.empty([b, skv, fv])
            D.gemm(m_q, f, h * dk, Mat(dq, gq), Mat(wq, f), Mat(dquery, f))
            D.gemm(m_kv, f, fkv, Mat(dk_, gk), Mat(wk, f), Mat(dkey, f))
            assert value.shape == (b, skv, h * dv)
            D.gemm(m_kv, fv, fvkv, Mat(dv_, gv), Mat(wv, fv), Mat(dvalue, fv))
            result = (dquery, dkey, dvalue)

        # update order of attentions.py:190-197
        for attribute, grad in (('_wq', dwq), ('_wk', dwk), ('_wv', dwv), ('_wo', dwo),
                                ('_bq', dbq), ('_bk', dbk), ('_bv', dbv), ('_bo', dbo)):
            scope.defer(optimizer_, self, attribute, grad)
        return result

    def _grouped_composition_bwd(self, dctx, dq, dk_, dv_, pitches) -> None:
        """attentions.py:146-162 for grouped-query attention from GEMMs: per group g one product batched over (B, Hkv) for each of
        dP, dV, dQ, dK (query heads g Hkv + c, K / V heads c); dV and dK sum the groups in the residual epilogue aliased to C, in
        the order g = 0, 1, ..., so the result does not depend on scheduling."""
        h, hkv, dk, dv = self._num_heads, self._num_kv_heads, self._key_dim, self._value_dim
        q, k, v, scores = self._q, self._k, self._v, self._attention_scores
        pq, pk, pv = self._pitches
        gq, gk, gv = pitches
        b, sq = dctx.shape[:2]
        skv = self._key.shape[1]
        plane = sq * skv
        datt = D.empty([b, h, sq, skv])
        for g in range(h // hkv):                 # dP = dctx_h v_c^T
            D.gemm(sq, skv, dv, Mat(_from(dctx, g * hkv * dv), h * dv, sq * h * dv, dv), Mat(v, pv, skv * pv, dv),
                   Mat(_from(datt, g * hkv * plane), skv, h * plane, plane), trans_b=True, batch=(b, hkv))
        D.softmax_bwd(scores, datt, self._scale, out=datt)
        for g in range(h // hkv):
            s_g = Mat(_from(scores, g * hkv * plane), skv, h * plane, plane)
            a_g = Mat(_from(datt, g * hkv * plane), skv, h * plane, plane)
            acc_v = None if g == 0 else Mat(dv_, gv, skv * gv, dv)
            acc_k = None if g == 0 else Mat(dk_, gk, skv * gk, dk)
            D.gemm(skv, dv, sq, s_g, Mat(_from(dctx, g * hkv * dv), h * dv, sq * h * dv, dv),
                   Mat(dv_, gv, skv * gv, dv), trans_a=True, batch=(b, hkv), residual=acc_v)          # (+)= P_h^T dctx_h
            D.gemm(sq, dk, skv, a_g, Mat(k, pk, skv * pk, dk),
                   Mat(_from(dq, g * hkv * dk), gq, sq * gq, dk), batch=(b, hkv))                      # datt_h k_c
            D.gemm(skv, dk, sq, a_g, Mat(_from(q, g * hkv * dk), pq, sq * pq, dk),
                   Mat(dk_, gk, skv * gk, dk), trans_a=True, batch=(b, hkv), residual=acc_k)          # (+)= datt_h^T q_h
