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

``norm`` ('layer', the default, or 'rms') and ``ffn`` ('relu', the default, or 'swiglu') choose the other half of the block:
``normalizations.RMSNormalization`` in every norm's place, and ``mlp.GatedDense`` -- the packed gate | up projection [F, 2 U] and the
gate kernel, ``hidden_units`` being the gated width U -- in ``dense1``'s place in front of ``dense2`` [U, F].  ``norm_epsilon``
(None: 1e-3 for 'layer', 1e-6 for 'rms') is the norms' epsilon.  Both have the fused composition; the RMSNorm kernels apply no
dropout mask, so ``norm='rms'`` with ``drop_rate > 0`` runs the literal composition with the standalone DropOut in front of the
norm.  With the defaults not one launch, upload or result differs from the reference's block.  ``decode`` and ``weights='f16'``
use the same two layers: the packed matrix is the one ``dense1`` holds.

``TransformerDecoder(cross_attention=False)`` (default True: not one launch, upload or result differs) is the decoder of a
decoder-only language model: self-attention and feed-forward only -- the middle block, ``_cross_attention``, its norm and its dropout
do not exist, and the layer holds ``TransformerEncoder``'s parameter set in one arena with one gradient bucket.  ``forward(q)`` takes
no memory, ``backward`` returns ``dq`` alone, ``start_decoding(None, capacity, batch=B, ...)`` makes a state whose ``cross_cache`` is
None, ``admit(state, b)`` takes no memory.  ``models.CausalLM`` stacks N of them over one key / value cache; ``_mask_source`` is how
it hands every layer the one causal mask of the stack.

``TransformerDecoder(causal=True)`` gives the self-attention a lower-triangular mask (the decoder everybody means by the word;
the reference's passes none, transformer.py:127), and ``start_decoding`` / ``decode`` run it incrementally over key / value
caches (inference; the reference marks the gap: ``# TODO: support cache``, transformer.py:120).  With ``causal=True`` and no
dropout, feeding a sequence to ``decode`` in chunks of any sizes gives, row for row, what ``forward`` gives for all of it.
"""

from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence

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


def _block_segments(norm, body, norm_first: bool):
    """A residual block's parameters in the order its backward produces their gradients: the norm's come after the
    body's with pre-norm, before them with post-norm."""
    return body + norm._segments() if norm_first else norm._segments() + body


NORMS = {'layer': normalizations.LayerNormalization, 'rms': normalizations.RMSNormalization}
FFNS = ('relu', 'swiglu')


def _check_kinds(who: str, norm: str, ffn: str) -> None:
    if norm not in NORMS:
        raise ValueError(f"{who}: norm must be one of {sorted(NORMS)}, got {norm!r}")
    if ffn not in FFNS:
        raise ValueError(f"{who}: ffn must be one of {sorted(FFNS)}, got {ffn!r}")


def _make_norm(norm: str, epsilon: Optional[float]):
    """A norm layer of that kind; ``epsilon`` None: the kind's own default (1e-3 'layer', 1e-6 'rms')."""
    return NORMS[norm]() if epsilon is None else NORMS[norm](epsilon)


def _make_dense1(ffn: str, hidden_units: int):
    """The first half of the feed-forward: Dense with a ReLU, or the packed gate | up projection of the gated-SiLU form."""
    return mlp.GatedDense(units=hidden_units) if ffn == 'swiglu' else mlp.Dense(units=hidden_units)


# A transformer layer is a chain of residual blocks around a body (attention or the feed-forward pair):
#     pre-norm :  y = x + body(norm(drop(x)))          post-norm:  y = norm(drop(x + body(x)))
# A layer lists its blocks (``_blocks``) and everything it does is a walk over that list.  The norm order is looked at by the
# four functions below and by ``_block_segments``, nowhere else.
class _Block(NamedTuple):
    norm: layer.StatefulLayer                   # LayerNormalization or RMSNormalization
    dropout: Optional[normalizations.DropOut]   # directly in front of the norm; None: inference
    forward: Callable                           # fused body, (h, residual=skip) -> body(h) + skip: the addition rides a GEMM epilogue
    backward: Optional[Callable] = None         # its mirror, (dy, optimizer_, scope, residual=) -> gradient of h (+ residual)
    body: Optional[Callable] = None             # the literal body, x -> body(x)
    body_backward: Optional[Callable] = None    # (dy, optimizer_, scope) -> gradient of the body's (first) input
    segments: Sequence = ()                     # the body's parameters in the order its backward produces their gradients
    numel: Optional[Callable] = None            # floats those gradients need
    flat: bool = False                          # works on the [rows, F] view
    flush: bool = False                         # a scope.flush() closes the block's backward (attention flushes by itself)


def _fused_forward(x, block: _Block, norm_first: bool):
    """The block with its residual addition inside the body's last GEMM and its dropout inside the norm's kernels."""
    if norm_first:
        return block.forward(block.norm._forward_impl(x, block.dropout), residual=x)
    return block.norm._forward_impl(block.forward(x, residual=x), block.dropout)


def _fused_backward(dy, block: _Block, norm_first: bool, optimizer_, scope):
    """Mirror of ``_fused_forward``: the skip path's gradient rides the LayerNorm backward (pre-norm) or the body's
    input-gradient GEMM (post-norm)."""
    if norm_first:
        dx = block.norm._backward_impl(block.backward(dy, optimizer_, scope), optimizer_, scope, residual=dy)
    else:
        dy = block.norm._backward_impl(dy, optimizer_, scope)
        dx = block.backward(dy, optimizer_, scope, residual=dy)
    if block.flush:
        scope.flush()
    return dx


# The same block and its mirror image built from standalone device adds -- the literal (unfused) composition, used when
# the dropout cannot ride the norm's kernels or the activation is not a ReLU, and as the reference the fused one is tested against.
def _block_forward(x, block: _Block, norm_first: bool):
    x = D.as_device(x)
    if norm_first:
        return D.add(D.as_device(block.body(block.norm(block.dropout(x)))), x)
    return D.as_device(block.norm(block.dropout(D.add(D.as_device(block.body(x)), x))))


def _block_backward(dy, block: _Block, norm_first: bool, optimizer_, scope):
    """``body_backward`` returns the gradient w.r.t. the body's (first) input; the skip path adds ``dy``."""
    if not norm_first:
        dy = block.dropout.backward(block.norm._backward_impl(D.as_device(dy), optimizer_, scope))
    through_skip = D.as_device(dy)
    through_body = D.as_device(block.body_backward(through_skip, optimizer_, scope))
    if norm_first:
        through_body = D.as_device(block.dropout.backward(block.norm._backward_impl(through_body, optimizer_, scope)))
    return D.add(through_body, through_skip)


def _shaped(x, flat: bool, shape):
    """``x`` as [rows, F] (``flat``) or as ``shape`` [B, S, F]."""
    if flat == (len(x.shape) == 2):
        return x
    return x.reshape(-1, shape[-1]) if flat else x.reshape(shape)


# Sub-layers initialise lazily at their first call, in call order, exactly as in the
# reference (layer.py:33-35) -- that fixes the global-RNG draw order of the parameters.
def _ensure(sub, *args):
    if not sub._initialized:
        sub.initialize(*args)
        sub._initialized = True


class _ResidualBlocks(layer.Layer):
    """What TransformerEncoder and TransformerDecoder share: a list of residual blocks, walked forward and backward in the
    fused or the literal composition."""

    _SLACK = 0          # floats of the gradient bucket beyond the parameters' own
    _norm = 'layer'     # which norm the blocks hold ('layer' | 'rms') and which feed-forward ('relu' | 'swiglu')
    _ffn = 'relu'

    def initialize(self, x, *memory):
        self._dense2 = mlp.Linear(units=x.shape[-1])  # no activation (transformer.py:25-27)

    def _self_mask(self, batch: int, seq: int):
        return None

    def _blocks(self, kv=None, kv_grad=None) -> List[_Block]:
        raise NotImplementedError

    def _self_attention_block(self, norm, dropout) -> _Block:
        att = self._self_attention

        def forward(h, residual):
            _ensure(att, h)
            return att._forward_impl(h, h, h, residual=residual, mask=self._self_mask(*h.shape[:2]))     # ... + skip (transformer.py:39)

        return _Block(norm, dropout, forward,
                      lambda dy, optimizer_, scope, residual=None:                                     # dq + dk + dv (+ skip)
                      att._backward_impl(dy, optimizer_, scope, sum_inputs=True, residual=residual),
                      lambda x: att(x, mask=self._self_mask(*x.shape[:2])),
                      lambda dy, optimizer_, scope: D.add3(*att._backward_impl(dy, optimizer_, scope)),
                      att._segments(), att._numel)

    def _feed_forward_block(self, norm, dropout) -> _Block:
        if self._ffn == 'swiglu':
            return self._gated_feed_forward_block(norm, dropout)
        dense1, dense2 = self._dense1, self._dense2
        lin1 = dense1._linear

        def forward(h, residual):
            h = dense1(h)
            _ensure(dense2, h)
            return dense2._forward_impl(h, residual=residual)                                           # ... + skip (transformer.py:53)

        def backward(dy, optimizer_, scope, residual=None):
            # dense2: dx masked by dense1's ReLU (activations.py:19) in the GEMM epilogue; dense1's bias gradient
            # (the column sums of that masked dx, mlp.py:34) comes out of dense1's weight-gradient GEMM
            dh = dense2._backward_impl(dy, optimizer_, scope, relu_mask_pre=dense1._activation._x)
            scope.flush()
            return lin1._backward_impl(dh, optimizer_, scope, residual=residual)

        def body_backward(dy, optimizer_, scope):
            dy = dense2._backward_impl(D.as_device(dy), optimizer_, scope)
            dy = dense1._activation.backward(dy)
            return lin1._backward_impl(D.as_device(dy), optimizer_, scope)

        return _Block(norm, dropout, forward, backward, lambda x: dense2(dense1(x)), body_backward,
                      _linear_segments(dense2) + _linear_segments(lin1),
                      lambda: lin1._w.size + lin1._b.size + dense2._w.size + dense2._b.size, flat=True, flush=True)

    def _gated_feed_forward_block(self, norm, dropout) -> _Block:
        """``ffn='swiglu'``: dense1 is a ``mlp.GatedDense`` -- the packed gate | up projection [F, 2 U] and the gate kernel --
        and dense2 [U, F] takes the skip in its epilogue."""
        gated, dense2 = self._dense1, self._dense2
        lin1 = gated._linear

        def forward(h, residual):
            h = gated(h)
            _ensure(dense2, h)
            return dense2._forward_impl(h, residual=residual)

        def backward(dy, optimizer_, scope, residual=None):
            dpre = gated._gate_backward(dense2._backward_impl(dy, optimizer_, scope))      # no ReLU mask: the gate has a kernel
            scope.flush()
            return lin1._backward_impl(dpre, optimizer_, scope, residual=residual)

        return _Block(norm, dropout, forward, backward, lambda x: dense2(gated(x)),
                      lambda dy, optimizer_, scope: gated.backward(dense2.backward(D.as_device(dy), optimizer_), optimizer_),
                      _linear_segments(dense2) + _linear_segments(lin1),
                      lambda: lin1._w.size + lin1._b.size + dense2._w.size + dense2._b.size, flat=True, flush=True)

    def _walk(self, run, x, blocks, *args):
        shape = x.shape
        for block in blocks:
            x = run(_shaped(x, block.flat, shape), block, self._norm_first, *args)
        return _shaped(x, False, shape)

    def _fusable(self, features: int = 0) -> bool:
        """The fused composition: always without dropout; with dropout when the LayerNorm kernels can apply it (row
        length: device.layernorm_dropout_supported) -- the RMSNorm kernels apply none, so ``norm='rms'`` with dropout runs the
        literal composition, the standalone DropOut in front of the norm."""
        dropouts = [block.dropout for block in self._blocks()]
        folds = _identity_dropout(*dropouts) if self._norm == 'rms' else _dropout_folds(features, *dropouts)
        return folds and self._fused_feed_forward()

    def _fused_feed_forward(self) -> bool:
        """Whether the feed-forward has a fused form: the gated one, or a Dense whose activation is the ReLU."""
        return self._ffn == 'swiglu' or self._dense1._fused_relu()

    def _numel(self) -> int:
        """Floats the gradients of one backward need: ONE bucket for the exchange (opened without a size, every gradient
        would be a collective of its own at N > 1)."""
        return sum(block.numel() + block.norm._grad_floats() for block in self._blocks()) + self._SLACK

    def _pack(self) -> None:
        """After the first forward (every sub-layer has drawn its parameters, in the reference's order): all parameters
        into ONE arena, ordered as ``backward`` produces their gradients -- last block first -- so that gradient bucket,
        exchange and the deferred updates walk one range (one optimizer launch per step)."""
        if self._arena is None:
            self._pack_parameters([segment for block in reversed(self._blocks())
                                   for segment in _block_segments(block.norm, list(block.segments), self._norm_first)])

    def _forward(self, x, *memory):
        self._fused = self._fusable(x.shape[-1])
        if not self._fused:
            return self._forward_unfused(x, *memory)
        # each DropOut sits directly in front of a LayerNormalization (transformer.py:35-36,40-41,49-50,55-56; the decoder's
        # 125-126,131-132,137-138,142-143,149-150,154-155) and is applied inside that norm's kernels
        out = self._walk(_fused_forward, x, self._blocks(*memory))
        self._pack()
        return out

    def _forward_unfused(self, x, *memory):
        """The reference's composition (transformer.py:29-59, 120-157) out of standalone kernels."""
        self._self_mask(*x.shape[:2])                   # made in front of the first block
        out = self._walk(_block_forward, x, self._blocks(*memory))
        self._pack()
        return out

    def backward(self, dy, optimizer_):
        dy = D.as_device(dy)
        with parallel.grad_scope(self._numel(), self._arena) as scope:
            if self._fused and self._fused_feed_forward():           # the composition the forward ran
                return self._backward_fused(dy, optimizer_, scope)
            return self._backward_unfused(dy, optimizer_, scope)

    def _walk_back(self, run, dy, optimizer_, scope):
        kv_grad = []
        dx = self._walk(run, dy, self._blocks(None, kv_grad)[::-1], optimizer_, scope)
        return (dx, kv_grad[0]) if kv_grad else dx

    def _backward_fused(self, dy, optimizer_, scope):
        """Mirror of the fused forward: skip-connection gradients ride the LayerNorm backward (pre-norm) or the
        input-gradient GEMMs (post-norm); dense1's ReLU backward is the mask epilogue of dense2's dx GEMM; the
        cross-attention's dkey + dvalue and the self-attention's dq + dk + dv accumulate in GEMM epilogues."""
        return self._walk_back(_fused_backward, dy, optimizer_, scope)

    def _backward_unfused(self, dy, optimizer_, scope):
        """Mirror of ``_forward_unfused`` (transformer.py:61-92, 159-203); the attention blocks sum their input gradients
        with standalone adds."""
        return self._walk_back(_block_backward, dy, optimizer_, scope)


class TransformerEncoder(_ResidualBlocks):
    _SLACK = 64

    def __init__(self, num_heads: int, hidden_units: int, norm_first: bool, drop_rate: float = 0.0,
                 *args, num_kv_heads: Optional[int] = None, rope_base: Optional[float] = None, norm: str = 'layer',
                 ffn: str = 'relu', norm_epsilon: Optional[float] = None, **kwargs):
        super().__init__(*args, **kwargs)
        _check_kinds('TransformerEncoder', norm, ffn)
        self._norm, self._ffn = norm, ffn
        self._self_attention = attentions.MultiHeadAttention(num_heads, num_kv_heads=num_kv_heads, rope_base=rope_base)
        self._dense1 = _make_dense1(ffn, hidden_units)
        self._norm1 = _make_norm(norm, norm_epsilon)
        self._norm2 = _make_norm(norm, norm_epsilon)
        self._norm_first = norm_first
        self._dropout1 = normalizations.DropOut(drop_rate)
        self._dropout2 = normalizations.DropOut(drop_rate)
        self._fused = True      # which composition the last forward ran (the backward mirrors it)

    def _blocks(self, kv=None, kv_grad=None) -> List[_Block]:
        """Self-attention, feed-forward (transformer.py:29-59): 16 parameters."""
        return [self._self_attention_block(self._norm1, self._dropout1), self._feed_forward_block(self._norm2, self._dropout2)]

    def forward(self, qkv):
        return self._forward(D.as_device(qkv))


class TransformerDecoder(_ResidualBlocks):
    """Self-attention, cross-attention over ``kv``, feed-forward; three LayerNorms
    (transformer.py:95-203).  ``backward`` returns ``(dq, dkv)`` with
    ``dkv = dkey + dvalue`` of the cross-attention (transformer.py:186)."""

    _SLACK = 128

    def __init__(self, num_heads: int, hidden_units: int, norm_first: bool, drop_rate: float = 0.0,
                 *args, num_kv_heads: Optional[int] = None, causal: bool = False, rope_base: Optional[float] = None,
                 window: Optional[int] = None, norm: str = 'layer', ffn: str = 'relu', norm_epsilon: Optional[float] = None,
                 cross_attention: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        _check_kinds('TransformerDecoder', norm, ffn)
        self._cross = bool(cross_attention)
        self._mask_source = None        # (B, Sq) -> device.AttnMask: a stack's one causal mask for all its layers (models.CausalLM)
        self._norm, self._ffn = norm, ffn
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
        self._dense1 = _make_dense1(ffn, hidden_units)
        self._norm1 = _make_norm(norm, norm_epsilon)
        self._norm2 = _make_norm(norm, norm_epsilon)
        self._norm_first = norm_first
        self._dropout1 = normalizations.DropOut(drop_rate)
        self._dropout2 = normalizations.DropOut(drop_rate)
        if self._cross:
            self._cross_attention = attentions.MultiHeadAttention(num_heads, num_kv_heads=num_kv_heads)   # never rotates: no query position
            self._norm3 = _make_norm(norm, norm_epsilon)
            self._dropout3 = normalizations.DropOut(drop_rate)
        else:
            self._SLACK = TransformerEncoder._SLACK     # the encoder's two blocks and 16 parameters: its bucket
        self._fused = True      # which composition the last forward ran (the backward mirrors it)

    def _blocks(self, kv=None, kv_grad=None) -> List[_Block]:
        """Self-attention, cross-attention over ``kv``, feed-forward (transformer.py:120-157): 26 parameters.  ``kv_grad``: the
        list a backward leaves the cross-attention's dkey + dvalue in (transformer.py:186).  ``cross_attention=False``: the
        encoder's two blocks, 16 parameters."""
        if not self._cross:
            return [self._self_attention_block(self._norm1, self._dropout1), self._feed_forward_block(self._norm2, self._dropout2)]
        ca = self._cross_attention

        def forward(h, residual):
            _ensure(ca, h, kv)
            return ca._forward_impl(h, kv, kv, residual=residual)                                       # ... + skip (transformer.py:141)

        def backward(dy, optimizer_, scope, residual=None):      # dkey + dvalue accumulate in their GEMMs' epilogues
            dquery, dkv = ca._backward_impl(dy, optimizer_, scope, sum_kv=True, residual=residual)
            kv_grad.append(dkv)
            return dquery

        def body_backward(dy, optimizer_, scope):
            dquery, dkey, dvalue = ca._backward_impl(dy, optimizer_, scope)
            kv_grad.append(D.add(dkey, dvalue))
            return dquery

        return [self._self_attention_block(self._norm1, self._dropout1),
                _Block(self._norm2, self._dropout2, forward, backward, lambda x: ca(x, kv), body_backward, ca._segments(), ca._numel),
                self._feed_forward_block(self._norm3, self._dropout3)]

    def _self_mask(self, batch: int, seq: int):
        """None, or (``causal=True``) the lower-triangular mask of the self-attention -- with ``window=W`` the band
        ``tril & ~tril(-W)`` -- made once per (B, Sq): its tile summary lets the fused kernels skip the tiles outside it."""
        if not self._causal:
            return None
        if self._mask_source is not None:
            return self._mask_source(int(batch), int(seq))
        key = (int(batch), int(seq))
        if key not in self._causal_masks:
            band = np.tril(np.ones([seq, seq], dtype=bool))
            if self._window is not None:
                band &= ~np.tril(np.ones([seq, seq], dtype=bool), -self._window)
            self._causal_masks[key] = D.AttnMask(band, batch, self._num_heads, seq, seq)
        return self._causal_masks[key]

    _NO_MEMORY = object()

    def forward(self, q, kv=_NO_MEMORY):
        """Three residual blocks: self-attention, cross-attention over ``kv``, feed-forward (transformer.py:120-157).
        The residual additions ride the producing GEMMs' epilogues and the dropouts the LayerNorm kernels, as in the encoder.
        ``cross_attention=False``: ``forward(q)``, two blocks, and ``backward`` returns ``dq`` alone."""
        if not self._cross:
            if kv is not self._NO_MEMORY:
                raise TypeError('TransformerDecoder(cross_attention=False).forward takes no memory: forward(q)')
            self._decoded = False
            return self._forward(D.as_device(q))
        if kv is self._NO_MEMORY:
            raise TypeError("TransformerDecoder.forward() missing 1 required positional argument: 'kv'")
        q, kv = D.as_device(q), D.as_device(kv)
        self._decoded = False
        self._kv = kv
        return self._forward(q, kv)

    # -- incremental decoding (inference) ------------------------------------------------------------------------------
    def start_decoding(self, kv, capacity: int, kv_lengths=None, *, page_size: Optional[int] = None, pages: Optional[int] = None,
                       memory_capacity: Optional[int] = None, cache_dtype: str = 'f32', weights: Optional[str] = None,
                       batch: Optional[int] = None) -> 'DecodeState':
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
        ``state.weights.refresh()``.  None allocates and launches nothing new.

        ``cross_attention=False``: there is no memory, so ``start_decoding(None, capacity, batch=B, ...)`` -- ``kv`` must be None,
        ``batch`` names the slots, ``kv_lengths`` and ``memory_capacity`` are refused; ``DecodeState.cross_cache`` is None."""
        if weights not in (None, 'f16'):
            raise ValueError(f"start_decoding: weights must be None or 'f16', got {weights!r}")
        if cache_dtype not in D.KV_ITEMSIZE:
            raise ValueError(f"start_decoding: cache_dtype must be one of {sorted(D.KV_ITEMSIZE)}, got {cache_dtype!r}")
        if not (self._initialized and self._self_attention._initialized and (not self._cross or self._cross_attention._initialized)):
            raise RuntimeError('start_decoding: the decoder has no parameters yet (run one forward, or bind weights, first)')
        if not self._cross:
            if kv is not None or kv_lengths is not None or memory_capacity is not None:
                raise ValueError('start_decoding: a decoder without cross-attention has no memory: kv must be None, and kv_lengths '
                                 'and memory_capacity have nothing to describe')
            if batch is None or int(batch) < 1:
                raise ValueError(f'start_decoding: a decoder without cross-attention needs batch= (the number of slots), got {batch!r}')
            paging = {} if page_size is None and pages is None else {'page_size': page_size, 'pages': pages}
            state = DecodeState(self._self_attention.make_cache(int(batch), capacity, dtype=cache_dtype, **paging), None)
            if weights == 'f16':
                state.weights = self._half_weights()
            return state
        if batch is not None:
            raise ValueError('start_decoding: batch= is for a decoder without cross-attention; here the memory kv [B, Skv, F] names it')
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
        """The matrices of a decode step as halves, in the order the step reads them: eight, or six without cross-attention."""
        sa, ca, lin1, lin2 = self._self_attention, getattr(self, '_cross_attention', None), self._dense1._linear, self._dense2
        if not (self._dense1._initialized and lin2._initialized):
            raise RuntimeError("start_decoding(weights='f16'): the feed-forward layers have no parameters yet (run one forward, or "
                               'bind weights, first)')
        cross = [(ca, '_wq'), (ca, '_wo')] if self._cross else []
        return D.HalfWeights([(sa, '_wq'), (sa, '_wk'), (sa, '_wv'), (sa, '_wo')] + cross + [(lin1, '_w'), (lin2, '_w')])

    def admit(self, state: 'DecodeState', b: int, kv_b=None, kv_length: Optional[int] = None) -> None:
        """A new sequence into slot ``b`` of a running batch (``state.release(b)`` emptied it): its memory ``kv_b`` [1, Skv, F]
        (``kv_length`` valid rows, default all) is projected with the cross-attention's K / V weights into slot b of the cross
        cache.  The next ``decode(q_new, state, new_lengths=n)`` carries the sequence's prompt in row b of the padded chunk.
        ``cross_attention=False``: ``admit(state, b)`` takes no memory and only checks that the slot is empty."""
        b = int(b)
        if not self._cross:
            if kv_b is not None or kv_length is not None:
                raise ValueError('admit: a decoder without cross-attention takes no memory: admit(state, b)')
            if not 0 <= b < state.self_cache.batch:
                raise IndexError(f'admit: no slot {b} in a batch of {state.self_cache.batch}')
            if state.self_cache.lengths[b] != 0:
                raise ValueError(f'admit: slot {b} still holds {int(state.self_cache.lengths[b])} rows; release({b}) it first')
            return
        if kv_b is None:
            raise TypeError("admit: the sequence's memory kv_b [1, Skv, F] is required")
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
        ca.fill_slot(cross, b, kv_b, rows)

    def fork(self, state: 'DecodeState', src: int, dst: int) -> None:
        """Slot ``dst`` of a running batch continues sequence ``src`` (n completions of one prompt, n-best sampling):
        ``DecodeState.fork``."""
        state.fork(src, dst)

    def reorder(self, state: 'DecodeState', parents, memory: str = 'shared') -> None:
        """Slot b of a running batch continues the sequence slot ``parents[b]`` held before the call, -1 ends it (a beam step):
        ``DecodeState.reorder``.  ``cross_attention=False``: there is no memory to move, ``memory`` takes its default only."""
        if not self._cross and memory != 'shared':
            raise ValueError(f"reorder: a decoder without cross-attention has no memory to copy: memory={memory!r}")
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
        state.self_cache.room(q.shape[1], new_lengths)                    # ValueError before anything is launched
        self._decoded = True
        sa, ca, dense1, dense2 = self._self_attention, getattr(self, '_cross_attention', None), self._dense1, self._dense2
        hw = state.weights                                                # None, or the fp16 copies of the six matrices below

        def feed_forward(h, residual):
            _ensure(dense1, h)
            half1 = None if hw is None else hw.view(dense1._linear, '_w')
            half2 = None if hw is None else hw.view(dense2, '_w')
            return dense2._forward_impl(dense1.forward(h, decode=True, half=half1), residual=residual, decode=True, half=half2)

        # the blocks of ``forward`` over the caches; no dropout, whatever drop_rate is
        attend = _Block(self._norm1, None, lambda h, residual: sa._forward_cached(h, state.self_cache, residual=residual,
                                                                                  new_lengths=new_lengths, weights=hw))
        if not self._cross:                                               # two blocks: there is no memory to attend to
            return self._walk(_fused_forward, q, (attend, _Block(self._norm2, None, feed_forward, flat=True)))
        return self._walk(_fused_forward, q, (
            attend,
            _Block(self._norm2, None, lambda h, residual: ca._forward_cached(h, state.cross_cache, residual=residual,
                                                                             new_lengths=new_lengths, weights=hw)),
            _Block(self._norm3, None, feed_forward, flat=True)))

    def backward(self, dy, optimizer_):
        """Returns ``(dq, dkv)``; ``dkv`` is the cross-attention's dkey + dvalue (transformer.py:159-203)."""
        if self._decoded:
            raise RuntimeError('backward after decode(): incremental decoding is inference only and overwrote what the last '
                               'forward saved -- run forward again first')
        return super().backward(dy, optimizer_)


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
        if self.cross_cache is not None:                                  # (None: a decoder without cross-attention)
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
        if self.cross_cache is not None:
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
        if cross is None:                                                 # a decoder without cross-attention: the default only
            if memory != 'shared':
                raise ValueError(f"reorder: there is no cross-attention cache to copy: memory={memory!r}")
            self.self_cache.reorder(p)
            return
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
