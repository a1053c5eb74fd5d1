"""TransformerEncoder / TransformerDecoder (reference layers/transformer.py:8-203).

Composition only: the sub-layers do the arithmetic.  In the encoder -- with or without dropout: a DropOut always sits
directly in front of a LayerNormalization there and rides inside that norm's kernels (normalizations.py
``LayerNormalization._forward_impl``) -- and in the decoder with ``drop_rate == 0`` the residual additions of
transformer.py:39,53,78,90 (encoder; 130,141,152,170-198 decoder) and the three-way sum of transformer.py:85 are folded into GEMM
epilogues / the LayerNorm backward kernel, and the ReLU backward of ``dense1`` is folded
into the epilogue of ``dense2``'s dx GEMM, so no standalone elementwise pass runs.
All parameter updates are deferred to the end of ``backward`` (every dx is computed from
pre-update weights in the reference too), which lets the data-parallel gradient all-reduce
overlap the rest of the backward pass.

``num_kv_heads`` (default None: multi-head attention) makes every attention layer grouped-query attention with that many
key / value heads (attentions.py); nothing else changes.

``rope_base`` (default None: no positional information, as the reference) turns on rotary position embeddings in the
self-attention (attentions.py): q and k are rotated by their positions, counted from 0, in forward, backward and incremental
decoding -- where a sequence's position is its row count in the cache, so one admitted into a freed slot starts at 0 again.  The
decoder's cross-attention never rotates.

``TransformerDecoder(causal=True)`` gives the self-attention a lower-triangular mask (the decoder everybody means by the word;
the reference's passes none, transformer.py:127), and ``start_decoding`` / ``decode`` run it incrementally over key / value
caches (inference; the reference marks the gap: ``# TODO: support cache``, transformer.py:120).  With ``causal=True`` and no
dropout, feeding a sequence to ``decode`` in chunks of any sizes gives, row for row, what ``forward`` gives for all of it.
"""

from __future__ import annotations

from typing import Optional

import numpy as np

from np_modeling_amd import device as D
from np_modeling_amd import parallel
from np_modeling_amd.layers import attentions, layer, mlp, normalizations


def _identity_dropout(*dropouts) -> bool:
    return all(d._drop_prob == 0.0 for d in dropouts)


def _dropout_folds(features: int, *dropouts) -> bool:
    """Whether the dropouts can ride inside the LayerNorm kernels behind them (device.layernorm_dropout_supported): always
    when they are the identity."""
    return _identity_dropout(*dropouts) or D.layernorm_dropout_supported(features)


def _linear_segments(lin):
    return [[(lin, '_b')], [(lin, '_w')]]              # Linear._backward_impl takes db, then dw


def _norm_segments(norm):
    return [[(norm, '_gamma')], [(norm, '_beta')]]


def _block_segments(norm, body, norm_first: bool):
    """A residual block's parameters in the order its backward produces their gradients: the norm's come after the
    body's with pre-norm, before them with post-norm."""
    return body + _norm_segments(norm) if norm_first else _norm_segments(norm) + body


# A transformer layer is a chain of residual blocks around a body (attention or the feed-forward pair):
#     pre-norm :  y = x + body(norm(drop(x)))          post-norm:  y = norm(drop(x + body(x)))
# The two helpers below are that block and its mirror image, built from standalone device adds -- the literal
# (unfused) composition, used when dropout is active, by the decoder, and as the reference the fused encoder is
# tested against.
def _block_forward(x, norm, dropout, norm_first: bool, body):
    x = D.as_device(x)
    if norm_first:
        return D.add(D.as_device(body(norm(dropout(x)))), x)
    return D.as_device(norm(dropout(D.add(D.as_device(body(x)), x))))


def _block_backward(dy, norm, dropout, norm_first: bool, body_backward, optimizer_, scope):
    """``body_backward(dy)`` returns the gradient w.r.t. the body's (first) input; the skip path adds ``dy``."""
    if not norm_first:
        dy = dropout.backward(norm._backward_impl(D.as_device(dy), optimizer_, scope))
    through_skip = D.as_device(dy)
    through_body = D.as_device(body_backward(through_skip))
    if norm_first:
        through_body = D.as_device(dropout.backward(norm._backward_impl(through_body, optimizer_, scope)))
    return D.add(through_body, through_skip)


class TransformerEncoder(layer.Layer):
    def __init__(self, num_heads: int, hidden_units: int, norm_first: bool, drop_rate: float = 0.0,
                 *args, num_kv_heads: Optional[int] = None, rope_base: Optional[float] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self._self_attention = attentions.MultiHeadAttention(num_heads, num_kv_heads=num_kv_heads, rope_base=rope_base)
        self._dense1 = mlp.Dense(units=hidden_units)
        self._norm1 = normalizations.LayerNormalization()
        self._norm2 = normalizations.LayerNormalization()
        self._norm_first = norm_first
        self._dropout1 = normalizations.DropOut(drop_rate)
        self._dropout2 = normalizations.DropOut(drop_rate)
        self._fused = True      # which composition the last forward ran (the backward mirrors it)

    def initialize(self, qkv):
        features = qkv.shape[-1]
        self._dense2 = mlp.Linear(units=features)  # no activation (transformer.py:25-27)

    def _numel(self) -> int:
        att = self._self_attention._numel()
        lin1, lin2 = self._dense1._linear, self._dense2
        norms = 2 * (self._norm1._param('_gamma').size + self._norm2._param('_gamma').size)
        return att + lin1._w.size + lin1._b.size + lin2._w.size + lin2._b.size + norms + 64

    def _pack(self) -> None:
        """After the first forward (every sub-layer has drawn its parameters, in the reference's order): all 16 parameters
        into ONE arena, ordered as ``backward`` produces their gradients -- feed-forward block, then attention block --
        so that gradient bucket, exchange and the deferred updates walk one range (one optimizer launch per step)."""
        if self._arena is None:
            pre = self._norm_first
            ffn = _linear_segments(self._dense2) + _linear_segments(self._dense1._linear)
            if pre:     # dense2 | dense1, norm2 | attention | norm1 -- the four flushes of _backward_fused
                segments = ffn + _norm_segments(self._norm2) + self._self_attention._segments() + _norm_segments(self._norm1)
            else:       # norm2, dense2 | dense1 | norm1, attention
                segments = (_norm_segments(self._norm2) + ffn + _norm_segments(self._norm1)
                            + self._self_attention._segments())
            self._pack_parameters(segments)

    # Sub-layers initialise lazily at their first call, in call order, exactly as in the
    # reference (layer.py:33-35) -- that fixes the global-RNG draw order of the parameters.
    @staticmethod
    def _ensure(sub, *args):
        if not sub._initialized:
            sub.initialize(*args)
            sub._initialized = True

    def forward(self, qkv):
        qkv = D.as_device(qkv)
        batch, seq_len_q, features = qkv.shape
        self._fused = _dropout_folds(features, self._dropout1, self._dropout2) and self._dense1._fused_relu()
        if not self._fused:
            return self._forward_unfused(qkv)
        att, dense1, dense2 = self._self_attention, self._dense1, self._dense2
        norm1, norm2 = self._norm1, self._norm2
        skip = qkv
        h = qkv
        if self._norm_first:
            h = norm1._forward_impl(h, self._dropout1)                   # dropout1 inside the norm (transformer.py:35-36)
        self._ensure(att, h)
        out = att._forward_impl(h, h, h, residual=skip)                  # ... + skip (transformer.py:39)
        if not self._norm_first:
            out = norm1._forward_impl(out, self._dropout1)               # transformer.py:40-41
        out = out.reshape(-1, features)
        skip = out
        if self._norm_first:
            out = norm2._forward_impl(out, self._dropout2)               # transformer.py:49-50
        out = dense1(out)
        self._ensure(dense2, out)
        out = dense2._forward_impl(out, residual=skip)                   # ... + skip (transformer.py:53)
        if not self._norm_first:
            out = norm2._forward_impl(out, self._dropout2)               # transformer.py:55-56
        self._pack()
        return out.reshape(batch, seq_len_q, features)

    def _feed_forward(self, x):
        return self._dense2(self._dense1(x))

    def _feed_forward_backward(self, dy, optimizer_, scope):
        dy = self._dense2._backward_impl(D.as_device(dy), optimizer_, scope)
        dy = self._dense1._activation.backward(dy)
        return self._dense1._linear._backward_impl(D.as_device(dy), optimizer_, scope)

    def _forward_unfused(self, qkv):
        """The reference's composition (transformer.py:29-59) out of standalone kernels: two residual blocks."""
        batch, seq_len_q, features = qkv.shape
        out = _block_forward(qkv, self._norm1, self._dropout1, self._norm_first, self._self_attention)
        out = _block_forward(out.reshape(-1, features), self._norm2, self._dropout2, self._norm_first,
                             self._feed_forward)
        self._pack()
        return out.reshape(batch, seq_len_q, features)

    def backward(self, dy, optimizer_):
        dy = D.as_device(dy)
        with parallel.grad_scope(self._numel(), self._arena) as scope:
            if self._fused and self._dense1._fused_relu():           # the composition the forward ran
                return self._backward_fused(dy, optimizer_, scope)
            return self._backward_unfused(dy, optimizer_, scope)

    def _backward_fused(self, dy, optimizer_, scope):
        batch, seq_len_q, features = dy.shape
        att, lin1, lin2 = self._self_attention, self._dense1._linear, self._dense2
        pre1 = self._dense1._activation._x
        dy = dy.reshape(-1, features)
        if not self._norm_first:
            dy = self._norm2._backward_impl(dy, optimizer_, scope)
        dskip = dy
        # dense2: dx masked by dense1's ReLU (activations.py:19) in the GEMM epilogue; dense1's bias gradient
        # (the column sums of that masked dx, mlp.py:34) comes out of dense1's weight-gradient GEMM
        dh = lin2._backward_impl(dy, optimizer_, scope, relu_mask_pre=pre1)
        scope.flush()
        if self._norm_first:
            dy = lin1._backward_impl(dh, optimizer_, scope)
            dy = self._norm2._backward_impl(dy, optimizer_, scope, residual=dskip)     # dy += dskip
        else:
            dy = lin1._backward_impl(dh, optimizer_, scope, residual=dskip)            # dy += dskip
        scope.flush()
        dy = dy.reshape(batch, seq_len_q, features)
        if not self._norm_first:
            dy = self._norm1._backward_impl(dy, optimizer_, scope)
        dskip = dy
        if self._norm_first:
            dy = att._backward_impl(dy, optimizer_, scope, sum_inputs=True)            # dq + dk + dv
            dy = self._norm1._backward_impl(dy, optimizer_, scope, residual=dskip)     # dy += dskip
        else:
            dy = att._backward_impl(dy, optimizer_, scope, sum_inputs=True, residual=dskip)
        return dy

    def _backward_unfused(self, dy, optimizer_, scope):
        """Mirror of ``_forward_unfused`` (transformer.py:61-92); the attention block sums dquery + dkey + dvalue."""
        batch, seq_len_q, features = dy.shape
        dy = _block_backward(dy.reshape(-1, features), self._norm2, self._dropout2, self._norm_first,
                             lambda g: self._feed_forward_backward(g, optimizer_, scope), optimizer_, scope)
        return _block_backward(dy.reshape(batch, seq_len_q, features), self._norm1, self._dropout1, self._norm_first,
                               lambda g: D.add3(*self._self_attention._backward_impl(g, optimizer_, scope)),
                               optimizer_, scope)


class TransformerDecoder(layer.Layer):
    """Self-attention, cross-attention over ``kv``, feed-forward; three LayerNorms
    (transformer.py:95-203).  ``backward`` returns ``(dq, dkv)`` with
    ``dkv = dkey + dvalue`` of the cross-attention (transformer.py:186)."""

    def __init__(self, num_heads: int, hidden_units: int, norm_first: bool, drop_rate: float = 0.0,
                 *args, num_kv_heads: Optional[int] = None, causal: bool = False, rope_base: Optional[float] = None,
                 window: Optional[int] = None, **kwargs):
        super().__init__(*args, **kwargs)
        if window is not None and not causal:
            raise ValueError('TransformerDecoder: window= is a rule of causal self-attention: it needs causal=True')
        self._num_heads = num_heads
        self._causal = bool(causal)
        self._causal_masks = {}         # (B, Sq) -> device.AttnMask: bytes and tile summary stay on the device between steps
        self._decoded = False           # decode() ran since the last forward: the saved activations are not that forward's
        # window: token p sees keys max(0, p - W + 1) .. p in the self-attention only -- a band mask in training, windowed caches
        # in decoding; the cross-attention sees the whole memory
        self._self_attention = attentions.MultiHeadAttention(num_heads, num_kv_heads=num_kv_heads, rope_base=rope_base, window=window)
        self._window = self._self_attention._window
        self._cross_attention = attentions.MultiHeadAttention(num_heads, num_kv_heads=num_kv_heads)   # never rotates: no query position
        self._dense1 = mlp.Dense(units=hidden_units)
        self._norm1 = normalizations.LayerNormalization()
        self._norm2 = normalizations.LayerNormalization()
        self._norm3 = normalizations.LayerNormalization()
        self._norm_first = norm_first
        self._dropout1 = normalizations.DropOut(drop_rate)
        self._dropout2 = normalizations.DropOut(drop_rate)
        self._dropout3 = normalizations.DropOut(drop_rate)

    def initialize(self, q, kv):
        features = q.shape[-1]
        self._dense2 = mlp.Linear(units=features)  # no activation

    def _feed_forward(self, x):
        return self._dense2(self._dense1(x))

    @staticmethod
    def _ensure(sub, *args):
        if not sub._initialized:
            sub.initialize(*args)
            sub._initialized = True

    _fused = True          # which composition the last forward ran (the backward mirrors it)

    def _fusable(self, features: int = 0) -> bool:
        """The fused composition: always without dropout; with dropout when the LayerNorm kernels can apply it (row
        length: device.layernorm_dropout_supported)."""
        return _dropout_folds(features, self._dropout1, self._dropout2, self._dropout3) and self._dense1._fused_relu()

    def _numel(self) -> int:
        """Floats the gradients of one backward need (26 parameter tensors): ONE bucket for the exchange, like the
        encoder's (round 4 opened the scope without a size: every gradient was a collective of its own at N > 1)."""
        lin1, lin2 = self._dense1._linear, self._dense2
        norms = sum(2 * n._param('_gamma').size for n in (self._norm1, self._norm2, self._norm3))
        return (self._self_attention._numel() + self._cross_attention._numel() + lin1._w.size + lin1._b.size
                + lin2._w.size + lin2._b.size + norms + 128)

    def _pack(self) -> None:
        """See TransformerEncoder._pack: feed-forward block, cross-attention block, self-attention block."""
        if self._arena is None:
            pre = self._norm_first
            ffn = _linear_segments(self._dense2) + _linear_segments(self._dense1._linear)
            ca, sa = self._cross_attention._segments(), self._self_attention._segments()
            self._pack_parameters(_block_segments(self._norm3, ffn, pre) + _block_segments(self._norm2, ca, pre)
                                  + _block_segments(self._norm1, sa, pre))

    def _self_mask(self, batch: int, seq: int):
        """None, or (``causal=True``) the lower-triangular mask of the self-attention -- with ``window=W`` the band
        ``tril & ~tril(-W)`` -- made once per (B, Sq): its tile summary lets the fused kernels skip the tiles outside it."""
        if not self._causal:
            return None
        key = (int(batch), int(seq))
        if key not in self._causal_masks:
            band = np.tril(np.ones([seq, seq], dtype=bool))
            if self._window is not None:
                band &= ~np.tril(np.ones([seq, seq], dtype=bool), -self._window)
            self._causal_masks[key] = D.AttnMask(band, batch, self._num_heads, seq, seq)
        return self._causal_masks[key]

    def forward(self, q, kv):
        """Three residual blocks: self-attention, cross-attention over ``kv``, feed-forward (transformer.py:120-157).
        The residual additions ride the producing GEMMs' epilogues and the dropouts the LayerNorm kernels, as in the encoder."""
        q, kv = D.as_device(q), D.as_device(kv)
        batch, seq_len_q, features = q.shape
        self._decoded = False
        self._fused = self._fusable(features)
        if not self._fused:
            return self._forward_unfused(q, kv)
        pre = self._norm_first
        sa, ca, dense1, dense2 = self._self_attention, self._cross_attention, self._dense1, self._dense2
        self._kv = kv
        # each DropOut sits directly in front of a LayerNormalization (transformer.py:125-126,131-132,137-138,142-143,
        # 149-150,154-155) and is applied inside that norm's kernels
        h = self._norm1._forward_impl(q, self._dropout1) if pre else q
        self._ensure(sa, h)
        out = sa._forward_impl(h, h, h, residual=q, mask=self._self_mask(batch, seq_len_q))   # ... + skip (transformer.py:130)
        if not pre:
            out = self._norm1._forward_impl(out, self._dropout1)
        skip = out
        h = self._norm2._forward_impl(out, self._dropout2) if pre else out
        self._ensure(ca, h, kv)
        out = ca._forward_impl(h, kv, kv, residual=skip)                  # ... + skip (transformer.py:141)
        if not pre:
            out = self._norm2._forward_impl(out, self._dropout2)
        out = out.reshape(-1, features)
        skip = out
        h = self._norm3._forward_impl(out, self._dropout3) if pre else out
        h = dense1(h)
        self._ensure(dense2, h)
        out = dense2._forward_impl(h, residual=skip)                      # ... + skip (transformer.py:152)
        if not pre:
            out = self._norm3._forward_impl(out, self._dropout3)
        self._pack()
        return out.reshape(batch, seq_len_q, features)

    # -- incremental decoding (inference) ------------------------------------------------------------------------------
    def start_decoding(self, kv, capacity: int, kv_lengths=None, *, page_size: Optional[int] = None, pages: Optional[int] = None,
                       memory_capacity: Optional[int] = None, cache_dtype: str = 'f32', weights: Optional[str] = None) -> 'DecodeState':
        """Caches for ``decode``: an empty self-attention cache of ``capacity`` tokens per sequence and the cross-attention's
        keys / values, projected from ``kv`` [B, Skv, F] once.  ``kv_lengths`` [B]: ``kv`` is padded on the right and sequence b
        has only that many memory rows.  The layer must have its parameters (one forward, or bound weights).

        ``page_size`` (and ``pages``): the self-attention cache is a ``device.PagedKVCache`` -- ``DecodeState.release(b)`` returns
        a finished sequence's pages and ``admit`` puts a new sequence into its slot.  The cross-attention cache stays contiguous
        (the memory fixes its size); ``memory_capacity`` (default Skv) is its row count, so that a sequence admitted later may
        bring a longer memory than the first batch had.

        ``cache_dtype`` 'f16': both caches -- the self-attention one and the frozen cross-attention one -- store their K / V rows as
        IEEE fp16 (``MultiHeadAttention.make_cache(dtype=)``): half the cache bytes, attention over the rows as stored.

        ``weights`` 'f16' (default None): the six matrices a decode step streams -- the self-attention's q / k / v and output
        projections, the cross-attention's query and output projections, ``dense1`` and ``dense2`` -- are copied ONCE as IEEE fp16
        (``device.HalfWeights``, kept in ``DecodeState.weights``) and ``decode`` reads those: half the weight bytes per step, the
        model whose six matrices are the rounded ones at every chunk size.  Biases and LayerNorm parameters stay fp32, and so do
        the memory projections here and in ``admit``.  The snapshot is of the weights as they are now: after they change,
        ``state.weights.refresh()``.  None allocates and launches nothing new."""
        if weights not in (None, 'f16'):
            raise ValueError(f"start_decoding: weights must be None or 'f16', got {weights!r}")
        if cache_dtype not in D.KV_ITEMSIZE:
            raise ValueError(f"start_decoding: cache_dtype must be one of {sorted(D.KV_ITEMSIZE)}, got {cache_dtype!r}")
        if not (self._initialized and self._self_attention._initialized and self._cross_attention._initialized):
            raise RuntimeError('start_decoding: the decoder has no parameters yet (run one forward, or bind weights, first)')
        kv = D.as_device(kv)
        batch, seq_kv, _ = kv.shape
        rows = seq_kv if memory_capacity is None else int(memory_capacity)
        if rows < seq_kv:
            raise ValueError(f'start_decoding: memory_capacity {rows} is less than the {seq_kv} memory rows given')
        cross = self._cross_attention.fill_cache(self._cross_attention.make_cache(batch, rows, dtype=cache_dtype), kv, lengths=kv_lengths)
        if page_size is None and pages is None:
            state = DecodeState(self._self_attention.make_cache(batch, capacity, dtype=cache_dtype), cross)
        else:
            state = DecodeState(self._self_attention.make_cache(batch, capacity, page_size=page_size, pages=pages, dtype=cache_dtype), cross)
        if weights == 'f16':
            state.weights = self._half_weights()
        return state

    def _half_weights(self) -> D.HalfWeights:
        """The six matrices of a decode step as halves, in the order the step reads them."""
        sa, ca, lin1, lin2 = self._self_attention, self._cross_attention, self._dense1._linear, self._dense2
        if not (self._dense1._initialized and lin2._initialized):
            raise RuntimeError("start_decoding(weights='f16'): the feed-forward layers have no parameters yet (run one forward, or "
                               'bind weights, first)')
        return D.HalfWeights([(sa, '_wq'), (sa, '_wk'), (sa, '_wv'), (sa, '_wo'), (ca, '_wq'), (ca, '_wo'), (lin1, '_w'), (lin2, '_w')])

    def admit(self, state: 'DecodeState', b: int, kv_b, kv_length: Optional[int] = None) -> None:
        """A new sequence into slot ``b`` of a running batch (``state.release(b)`` emptied it): its memory ``kv_b`` [1, Skv, F]
        (``kv_length`` valid rows, default all) is projected with the cross-attention's K / V weights into slot b of the cross
        cache.  The next ``decode(q_new, state, new_lengths=n)`` carries the sequence's prompt in row b of the padded chunk."""
        b = int(b)
        cross, ca = state.cross_cache, self._cross_attention
        if not 0 <= b < cross.batch:
            raise IndexError(f'admit: no slot {b} in a batch of {cross.batch}')
        if state.self_cache.lengths[b] != 0:
            raise ValueError(f'admit: slot {b} still holds {int(state.self_cache.lengths[b])} rows; release({b}) it first')
        kv_b = D.as_device(kv_b)
        one, skv, f = kv_b.shape
        rows = skv if kv_length is None else int(kv_length)
        if one != 1 or not 1 <= rows <= skv:
            raise ValueError(f'admit: the memory is [1, Skv, F] with 1 <= kv_length <= Skv, got {kv_b.shape} and {kv_length}')
        if rows > cross.capacity:
            raise ValueError(f'admit: {rows} memory rows do not fit the cross-attention cache of {cross.capacity} rows '
                             '(start_decoding(..., memory_capacity=))')
        hkv = cross.kv_heads

        def project(w, bias, dim):
            proj = D.empty([1, rows, hkv, dim])
            D.gemm(rows, hkv * dim, f, D.Mat(kv_b, f), D.Mat(ca._param(w), f), D.Mat(proj, hkv * dim), trans_b=True, bias=ca._param(bias))
            return D.Mat(proj, hkv * dim)

        cross.write_slot(b, project('_wk', '_bk', cross.key_dim), None, rows)     # K is projected and written, then V
        cross.write_slot(b, None, project('_wv', '_bv', cross.value_dim), rows)

    def fork(self, state: 'DecodeState', src: int, dst: int) -> None:
        """Slot ``dst`` of a running batch continues sequence ``src`` (n completions of one prompt, n-best sampling):
        ``DecodeState.fork``."""
        state.fork(src, dst)

    def reorder(self, state: 'DecodeState', parents, memory: str = 'shared') -> None:
        """Slot b of a running batch continues the sequence slot ``parents[b]`` held before the call, -1 ends it (a beam step):
        ``DecodeState.reorder``."""
        state.reorder(parents, memory=memory)

    def decode(self, q_new, state: 'DecodeState', new_lengths=None):
        """One incremental step: the T new tokens ``q_new`` [B, T, F] through cached causal self-attention, cross-attention over
        the frozen cache, feed-forward and the three norms -> [B, T, F].  Dropout is the identity (inference: the reference's
        ``DropOut.forward(training=False)``).  T may be a whole prompt or 1; the self-attention cache grows by T.

        ``new_lengths`` [B] (a ragged batch): ``q_new`` is padded on the right (with finite values) and sequence b brings
        n[b] <= T tokens, 0 for one that has finished; its cache grows by n[b].  Only the two attentions look across rows, and
        they are told the lengths; LayerNorm, the dense layers and the residual additions work row by row, so a padded row
        passes through them without touching a valid row or being touched by one.  Output rows t >= n[b] are unspecified but
        finite; rows t < n[b] are what sequence b gives when decoded alone."""
        q = D.as_device(q_new)
        batch, tokens, features = q.shape
        state.self_cache.room(tokens, new_lengths)                        # ValueError before anything is launched
        self._decoded = True
        pre = self._norm_first
        sa, ca = self._self_attention, self._cross_attention
        hw = state.weights                                                # None, or the fp16 copies of the six matrices below
        h = self._norm1._forward_impl(q) if pre else q
        out = sa._forward_cached(h, state.self_cache, residual=q, new_lengths=new_lengths, weights=hw)
        if not pre:
            out = self._norm1._forward_impl(out)
        skip = out
        h = self._norm2._forward_impl(out) if pre else out
        out = ca._forward_cached(h, state.cross_cache, residual=skip, new_lengths=new_lengths, weights=hw)
        if not pre:
            out = self._norm2._forward_impl(out)
        out = out.reshape(-1, features)
        skip = out
        h = self._norm3._forward_impl(out) if pre else out
        self._ensure(self._dense1, h)
        half1 = None if hw is None else hw.view(self._dense1._linear, '_w')
        half2 = None if hw is None else hw.view(self._dense2, '_w')
        out = self._dense2._forward_impl(self._dense1.forward(h, decode=True, half=half1), residual=skip, decode=True, half=half2)
        if not pre:
            out = self._norm3._forward_impl(out)
        return out.reshape(batch, tokens, features)

    def _forward_unfused(self, q, kv):
        batch, seq_len_q, features = q.shape
        mask = self._self_mask(batch, seq_len_q)
        out = _block_forward(q, self._norm1, self._dropout1, self._norm_first,
                             self._self_attention if mask is None else lambda x: self._self_attention(x, mask=mask))
        out = _block_forward(out, self._norm2, self._dropout2, self._norm_first,
                             lambda x: self._cross_attention(x, kv))
        out = _block_forward(out.reshape(-1, features), self._norm3, self._dropout3, self._norm_first,
                             self._feed_forward)
        self._pack()
        return out.reshape(batch, seq_len_q, features)

    def backward(self, dy, optimizer_):
        """Returns ``(dq, dkv)``; ``dkv`` is the cross-attention's dkey + dvalue (transformer.py:159-203)."""
        if self._decoded:
            raise RuntimeError('backward after decode(): incremental decoding is inference only and overwrote what the last '
                               'forward saved -- run forward again first')
        dy = D.as_device(dy)
        with parallel.grad_scope(self._numel(), self._arena) as scope:
            if self._fused and self._dense1._fused_relu():           # the composition the forward ran
                return self._backward_fused(dy, optimizer_, scope)
            return self._backward_unfused(dy, optimizer_, scope)

    def _backward_fused(self, dy, optimizer_, scope):
        """Mirror of the fused forward: skip-connection gradients ride the LayerNorm backward (pre-norm) or the
        input-gradient GEMMs (post-norm); dense1's ReLU backward is the mask epilogue of dense2's dx GEMM; the
        cross-attention's dkey + dvalue and the self-attention's dq + dk + dv accumulate in GEMM epilogues."""
        batch, seq_len_q, features = dy.shape
        pre = self._norm_first
        sa, ca, lin1, lin2 = self._self_attention, self._cross_attention, self._dense1._linear, self._dense2
        dy = dy.reshape(-1, features)
        if not pre:
            dy = self._norm3._backward_impl(dy, optimizer_, scope)
        dskip = dy
        dh = lin2._backward_impl(dy, optimizer_, scope, relu_mask_pre=self._dense1._activation._x)
        scope.flush()
        if pre:
            dy = self._norm3._backward_impl(lin1._backward_impl(dh, optimizer_, scope), optimizer_, scope, residual=dskip)
        else:
            dy = lin1._backward_impl(dh, optimizer_, scope, residual=dskip)
        scope.flush()
        dy = dy.reshape(batch, seq_len_q, features)
        if not pre:
            dy = self._norm2._backward_impl(dy, optimizer_, scope)
        dskip = dy
        if pre:
            dquery, dkv = ca._backward_impl(dy, optimizer_, scope, sum_kv=True)
            dy = self._norm2._backward_impl(dquery, optimizer_, scope, residual=dskip)
        else:
            dy, dkv = ca._backward_impl(dy, optimizer_, scope, sum_kv=True, residual=dskip)
        if not pre:
            dy = self._norm1._backward_impl(dy, optimizer_, scope)
        dskip = dy
        if pre:
            dy = sa._backward_impl(dy, optimizer_, scope, sum_inputs=True)
            dy = self._norm1._backward_impl(dy, optimizer_, scope, residual=dskip)
        else:
            dy = sa._backward_impl(dy, optimizer_, scope, sum_inputs=True, residual=dskip)
        return dy, dkv

    def _backward_unfused(self, dy, optimizer_, scope):
        batch, seq_len_q, features = dy.shape
        kv_grad = []

        def feed_forward_backward(g):
            g = self._dense2._backward_impl(D.as_device(g), optimizer_, scope)
            g = self._dense1._activation.backward(g)
            return self._dense1._linear._backward_impl(D.as_device(g), optimizer_, scope)

        def cross_attention_backward(g):
            dquery, dkey, dvalue = self._cross_attention._backward_impl(g, optimizer_, scope)
            kv_grad.append(D.add(dkey, dvalue))
            return dquery

        def self_attention_backward(g):
            return D.add3(*self._self_attention._backward_impl(g, optimizer_, scope))

        dy = _block_backward(dy.reshape(-1, features), self._norm3, self._dropout3, self._norm_first,
                             feed_forward_backward, optimizer_, scope)
        dy = _block_backward(dy.reshape(batch, seq_len_q, features), self._norm2, self._dropout2,
                             self._norm_first, cross_attention_backward, optimizer_, scope)
        dy = _block_backward(dy, self._norm1, self._dropout1, self._norm_first, self_attention_backward,
                             optimizer_, scope)
        return dy, kv_grad[0]


class DecodeState:
    """What ``TransformerDecoder.decode`` carries from step to step: the self-attention's growing key / value cache and the
    cross-attention's frozen one (``device.KVCache``).  ``position``: tokens decoded so far while that is the same number for
    every sequence (it raises once a ragged batch made them differ); ``positions``: the number per sequence.  ``weights``: None,
    or the ``device.HalfWeights`` snapshot ``start_decoding(..., weights='f16')`` took -- ``release`` and ``admit`` leave it alone."""

    __slots__ = ('self_cache', 'cross_cache', 'weights')

    def __init__(self, self_cache: D.KVCache, cross_cache: D.KVCache, weights: Optional[D.HalfWeights] = None):
        self.self_cache, self.cross_cache, self.weights = self_cache, cross_cache, weights

    def release(self, b) -> None:
        """Sequence ``b`` (an index or several) has finished: its self-attention pages go back to the pool and both caches hold
        0 rows of it.  It then rides along with ``new_lengths[b] = 0`` until ``TransformerDecoder.admit`` fills the slot."""
        if not self.self_cache.paged:
            raise ValueError('DecodeState.release: the self-attention cache is not paged (start_decoding(..., page_size=))')
        self.self_cache.release(b)
        self.cross_cache.lengths[np.unique(np.atleast_1d(np.asarray(b, dtype=np.int64)))] = 0

    def fork(self, src: int, dst: int) -> None:
        """Slot ``dst`` becomes sequence ``src``: the self-attention cache is forked (a paged one shares its pages until the
        sequences grow apart, ``device.PagedKVCache.fork``; a contiguous one copies the rows) and so is the frozen
        cross-attention cache (a copy of the memory's projected rows).  ``weights`` is left alone; rotary positions follow the
        lengths.  ValueError, with nothing changed, while slot ``dst`` still holds rows (``release`` it first), as ``admit``."""
        src, dst = self.self_cache._fork_slots(src, dst)
        if self.self_cache.lengths[dst] != 0:
            raise ValueError(f'fork: slot {dst} still holds {int(self.self_cache.lengths[dst])} rows; release({dst}) it first')
        self.self_cache.fork(src, dst)
        self.cross_cache.fork(src, dst)

    def reorder(self, parents, memory: str = 'shared') -> None:
        """Slot b becomes the sequence slot ``parents[b]`` held BEFORE the call (int [B]; -1 empties the slot): the
        self-attention cache is reordered (``device.PagedKVCache.reorder``: table rows, nothing launched; a contiguous cache
        copies rows).  ``memory`` 'shared' (default): slot b and slot ``parents[b]`` attend the same memory, as the beams of
        one prompt do, so the cross-attention cache is left alone -- ValueError, with nothing changed, if their cross
        ``lengths`` differ; a -1 still sets the slot's cross length to 0.  'copy': the cross-attention cache is reordered too
        (``device.KVCache.reorder``, O(L) per moved slot).  ``weights`` is left alone; rotary positions follow the lengths."""
        if memory not in ('shared', 'copy'):
            raise ValueError(f"reorder: memory must be 'shared' or 'copy', got {memory!r}")
        p = self.self_cache._parents(parents)
        cross = self.cross_cache
        if memory == 'shared':
            live = p >= 0
            if (cross.lengths[live] != cross.lengths[p[live]]).any():
                raise ValueError(f"reorder: memory='shared' but the cross-attention lengths {cross.lengths.tolist()} differ between "
                                 f"a slot and its parent in {p.tolist()}; memory='copy' moves the memory along")
        self.self_cache.reorder(p)
        if memory == 'shared':
            cross.lengths = np.where(p >= 0, cross.lengths, 0)
        else:
            cross.reorder(p)

    def truncate(self, rows) -> None:
        """The last ``rows`` (an integer or [B]) tokens leave the self-attention cache (``device.KVCache.truncate``): the drafted
        tokens of a speculative step that were not accepted.  The cross-attention cache is not touched; rotary positions follow
        the lengths."""
        self.self_cache.truncate(rows)

    @property
    def position(self) -> int:
        return self.self_cache.length

    @property
    def positions(self) -> np.ndarray:
        return self.self_cache.lengths.copy()
