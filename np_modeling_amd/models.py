"""Whole models out of the layers.  ``CausalLM``: the decoder-only language model

    Embedding(vocab, features)
      -> num_layers x TransformerDecoder(cross_attention=False, causal=True, ...)
      -> a final norm of the same kind (pre-norm stacks only)
      -> Linear(vocab)

It is a ``Layer``: ``Trainer([lm], SoftmaxCrossEntropyLoss())`` trains it from token ids with no adapter -- ``forward(ids [B, S])``
gives logits [B, S, V] (the head runs on the [B S, F] view), ``backward(dlogits, optimizer_)`` walks head, final norm, the layers in
reverse and the embedding and returns None.  Sub-layers initialise lazily in call order, as everywhere else, so a seed fixes the
parameters.  The stack shares what its layers would each keep: ONE ``device.AttnMask`` per (B, S) (``TransformerDecoder._mask_source``),
ONE rotary table, and in decoding ONE key / value cache with N layer views (``device.KVCache(layers=N)``): one ``lengths``, one
length mirror, one block table and one free list, so a decode step uploads what a single layer uploads, whatever N is.

Decoding.  ``state = lm.start_decoding(batch, capacity, ...)``; ``lm.decode(ids, state, new_lengths=None, rows='last')`` embeds
``ids`` (host ints or an ``IdBuffer`` [B, T]), opens a step on the cache (``begin``), walks the layers over their views, commits,
and returns the logits of every sequence's last new token [B, V] (``device.take_rows`` in front of the final norm and the head; a
sequence that brought nothing gets the logits of a zero row) or with ``rows='all'`` of all rows [B T, V].  ``lm.release`` /
``admit`` / ``fork`` / ``reorder`` and ``state.truncate`` act on all layers at once: they are the single-layer host operations of
the one cache.

The generation loops take the model as it is: ``lm.stack`` has the ``decode(x, state, new_lengths=)`` of a decoder over hidden
states (the layers plus the final norm), so ``speculative.decode_step(lm.stack, state, lm.embedding, lm.head, sampler, drafter)`` and
``beam.decode_step(lm.stack, state, lm.embedding, lm.head, search)`` run a multi-layer model.  ``lm.generate`` is the plain
prefill-then-one-token loop.

Batches larger than one forward holds: ``Trainer.train(..., micro_batches=k)`` with ``AdamWOptimizer(accumulate=True)`` (optimizer.py).

Not built: a bias-free ``Linear``, a tied embedding / head, GELU, an in-kernel causal rule for the training kernels (the mask's tile
summary skips tiles up to S 2048), a HIP graph of the step, activation checkpointing, and the one-pass shared-prefix attention
(``device.SHARED_PREFIX``) over a layered cache."""

from __future__ import annotations

from typing import List, Optional

import numpy as np

from np_modeling_amd import device as D
from np_modeling_amd.layers import embedding, layer, mlp, transformer


class _NoMemory:
    """What ``LMState.cross_cache`` is: a decoder-only model has no cross-attention memory.  ``lengths`` says one row per slot,
    so a loop written for an encoder-decoder state that copies a parent's memory into an empty slot (``beam.decode_step``) finds
    no empty slot and copies nothing."""

    def __init__(self, batch: int):
        self.batch = int(batch)
        self.lengths = np.ones([self.batch], dtype=np.int64)


class LMState:
    """What ``CausalLM.decode`` carries from step to step: ``self_cache``, the ONE layered key / value cache of the stack
    (``batch``, ``capacity``, ``lengths``), ``layers``, one ``transformer.DecodeState`` per layer over its view of that cache (and
    its fp16 weight snapshot, if any).  ``release`` / ``fork`` / ``reorder`` / ``truncate`` are one host operation each."""

    def __init__(self, cache: D.KVCache, weights: Optional[List[D.HalfWeights]] = None):
        self.self_cache = cache
        self.cross_cache = _NoMemory(cache.batch)
        self.weights = weights
        self.layers = [transformer.DecodeState(cache.layer(i), None, None if weights is None else weights[i]) for i in range(cache.layers)]

    def release(self, b) -> None:
        if not self.self_cache.paged:
            raise ValueError('LMState.release: the cache is not paged (start_decoding(..., page_size=))')
        self.self_cache.release(b)

    def fork(self, src: int, dst: int) -> None:
        src, dst = self.self_cache._fork_slots(src, dst)
        if self.self_cache.lengths[dst] != 0:
            raise ValueError(f'fork: slot {dst} still holds {int(self.self_cache.lengths[dst])} rows; release({dst}) it first')
        self.self_cache.fork(src, dst)

    def reorder(self, parents, memory: str = 'shared') -> None:
        if memory != 'shared':
            raise ValueError(f"reorder: a decoder-only model has no memory to copy: memory={memory!r}")
        self.self_cache.reorder(parents)

    def truncate(self, rows) -> None:
        self.self_cache.truncate(rows)

    @property
    def position(self) -> int:
        return self.self_cache.length

    @property
    def positions(self) -> np.ndarray:
        return self.self_cache.lengths.copy()


class _CausalMasks:
    """(B, S) -> the lower-triangular ``device.AttnMask`` (with ``window`` the band) of a stack's self-attentions, made once."""

    def __init__(self, heads: int, window: Optional[int]):
        self._heads, self._window, self.masks = heads, window, {}

    def __call__(self, batch: int, seq: int) -> D.AttnMask:
        key = (batch, seq)
        if key not in self.masks:
            band = np.tril(np.ones([seq, seq], dtype=bool))
            if self._window is not None:
                band &= ~np.tril(np.ones([seq, seq], dtype=bool), -self._window)
            self.masks[key] = D.AttnMask(band, batch, self._heads, seq, seq)
        return self.masks[key]


class _Stack:
    """The layers plus the final norm over hidden states, with the calls the generation loops make on a decoder."""

    def __init__(self, layers, final_norm):
        self._layers, self._final_norm = layers, final_norm

    def decode_layers(self, x: D.DeviceArray, state: LMState, new_lengths):
        """[B, T, F] through every layer: ONE ``begin`` -- room, window reclaim, pages, copy-on-write, the uploads -- N appends and
        attentions over the layer views, ONE ``commit``."""
        cache = state.self_cache
        if len(state.layers) != len(self._layers):
            raise ValueError(f'decode: the state was made for {len(state.layers)} layers, the model has {len(self._layers)}')
        cache.begin(x.shape[1], new_lengths)
        try:
            for block, layer_state in zip(self._layers, state.layers):
                x = block.decode(x, layer_state, new_lengths=new_lengths)
        except BaseException:
            cache.abandon()
            raise
        cache.commit()
        return x

    def decode(self, x, state: LMState, new_lengths=None):
        """[B, T, F] -> [B, T, F]: one step of every layer over the one cache, then the final norm."""
        hidden = self.decode_layers(D.as_device(x), state, new_lengths)
        return hidden if self._final_norm is None else self._final_norm._forward_impl(hidden)

    def fork(self, state: LMState, src: int, dst: int) -> None:
        state.fork(src, dst)

    def reorder(self, state: LMState, parents, memory: str = 'shared') -> None:
        state.reorder(parents, memory=memory)


class CausalLM(layer.Layer):
    def __init__(self, vocab: int, features: int, num_layers: int, num_heads: int, hidden_units: int, *args,
                 num_kv_heads: Optional[int] = None, rope_base: Optional[float] = 10000.0, norm: str = 'rms', ffn: str = 'swiglu',
                 norm_epsilon: Optional[float] = None, norm_first: bool = True, window: Optional[int] = None, drop_rate: float = 0.0,
                 **kwargs):
        super().__init__(*args, **kwargs)
        if int(num_layers) < 1:
            raise ValueError(f'CausalLM: num_layers must be at least 1, got {num_layers!r}')
        if int(features) % int(num_heads):
            raise ValueError(f'CausalLM: features {features} is not a multiple of num_heads {num_heads}')
        transformer._check_kinds('CausalLM', norm, ffn)
        self._vocab, self._features, self._num_heads = int(vocab), int(features), int(num_heads)
        self.embedding = embedding.Embedding(vocab, features)
        self.layers = [transformer.TransformerDecoder(num_heads, hidden_units, norm_first, drop_rate, num_kv_heads=num_kv_heads,
                                                      causal=True, rope_base=rope_base, window=window, norm=norm, ffn=ffn,
                                                      norm_epsilon=norm_epsilon, cross_attention=False) for _ in range(int(num_layers))]
        self.final_norm = transformer._make_norm(norm, norm_epsilon) if norm_first else None
        self.head = mlp.Linear(units=vocab)
        self.stack = _Stack(self.layers, self.final_norm)
        self._causal_mask = _CausalMasks(self._num_heads, self.layers[0]._window)      # one mask per (B, S) for the whole stack
        rope = None if rope_base is None else D.RopeTable(self._features // self._num_heads, rope_base)
        for block in self.layers:
            block._mask_source = self._causal_mask
            block._self_attention._rope = rope          # one table for every layer's rotation (made on the device at first use)
        self.fused_rope_append = True                   # the rotation and both appends of a decode step in one launch per layer

    resident_inputs = staticmethod(D.as_ids)            # Trainer.train: token ids stay integers, uploaded once

    @property
    def fused_rope_append(self) -> bool:
        """Whether the layers' cached self-attention runs npm_rope_kv_append instead of npm_rope and two appends (the same bits
        either way; ``device.FUSED_ROPE_APPEND`` is the module's switch, off by default, and this model turns its layers on)."""
        return bool(self.layers[0]._self_attention._fused_rope_append)

    @fused_rope_append.setter
    def fused_rope_append(self, on: bool) -> None:
        for block in self.layers:
            block._self_attention._fused_rope_append = bool(on)

    # ---- training -----------------------------------------------------------------------------------------------------------
    def forward(self, ids):
        ids = D.as_ids(ids)
        if len(ids.shape) != 2:
            raise ValueError(f'CausalLM.forward: token ids are [B, S], got {tuple(ids.shape)}')
        x = self.embedding(ids)
        for block in self.layers:
            x = block(x)
        if self.final_norm is not None:
            x = self.final_norm(x)
        b, s, f = x.shape
        return self.head(x.reshape(b * s, f)).reshape(b, s, self._vocab)

    def backward(self, dlogits, optimizer_):
        dy = D.as_device(dlogits)
        b, s, v = dy.shape
        dx = self.head(dy.reshape(b * s, v), backprop=True, optimizer_=optimizer_).reshape(b, s, self._features)
        if self.final_norm is not None:
            dx = self.final_norm(dx, backprop=True, optimizer_=optimizer_)
        for block in self.layers[::-1]:
            dx = block(dx, backprop=True, optimizer_=optimizer_)
        self.embedding(dx, backprop=True, optimizer_=optimizer_)
        return None

    # ---- incremental decoding (inference) --------------------------------------------------------------------------------------
    def start_decoding(self, batch: int, capacity: int, *, page_size: Optional[int] = None, pages: Optional[int] = None,
                       cache_dtype: str = 'f32', weights: Optional[str] = None) -> LMState:
        """An empty cache of ``capacity`` tokens for each of ``batch`` sequences, shared by all layers; the keywords are
        ``TransformerDecoder.start_decoding``'s.  The model must have its parameters (one forward, or bound weights)."""
        if weights not in (None, 'f16'):
            raise ValueError(f"start_decoding: weights must be None or 'f16', got {weights!r}")
        if not (self._initialized and all(block._initialized and block._self_attention._initialized for block in self.layers)
                and self.head._initialized):
            raise RuntimeError('start_decoding: the model has no parameters yet (run one forward, or bind weights, first)')
        if page_size is None and pages is not None:
            raise ValueError('start_decoding: pages= sizes the pool of a paged cache: it needs page_size=')
        cache = self.layers[0]._self_attention.make_cache(int(batch), capacity, page_size=page_size, pages=pages, dtype=cache_dtype,
                                                          layers=len(self.layers))
        return LMState(cache, [block._half_weights() for block in self.layers] if weights == 'f16' else None)

    def decode(self, ids, state: LMState, new_lengths=None, rows: str = 'last'):
        if rows not in ('last', 'all'):
            raise ValueError(f"decode: rows must be 'last' or 'all', got {rows!r}")
        ids = D.as_ids(ids)
        if len(ids.shape) != 2 or ids.shape[0] != state.self_cache.batch:
            raise ValueError(f'decode: token ids are [{state.self_cache.batch}, T], got {tuple(ids.shape)}')
        batch, tokens = ids.shape
        n = state.self_cache._counts(tokens, state.self_cache.new_lengths(tokens, new_lengths))
        hidden = self.stack.decode_layers(self.embedding.forward(ids), state, new_lengths).reshape(batch * tokens, self._features)
        if rows == 'last':
            hidden = D.take_rows(hidden, np.where(n > 0, np.arange(batch) * tokens + n - 1, -1))
        if self.final_norm is not None:
            hidden = self.final_norm._forward_impl(hidden)
        return self.head.forward(hidden)

    def release(self, state: LMState, b) -> None:
        state.release(b)

    def admit(self, state: LMState, b: int) -> None:
        """Slot ``b`` takes a new sequence with the next ``decode``: only checks that ``release`` emptied it."""
        b = int(b)
        if not 0 <= b < state.self_cache.batch:
            raise IndexError(f'admit: no slot {b} in a batch of {state.self_cache.batch}')
        if state.self_cache.lengths[b] != 0:
            raise ValueError(f'admit: slot {b} still holds {int(state.self_cache.lengths[b])} rows; release({b}) it first')

    def fork(self, state: LMState, src: int, dst: int) -> None:
        state.fork(src, dst)

    def reorder(self, state: LMState, parents) -> None:
        state.reorder(parents)

    def generate(self, prompt_ids, lengths, max_new_tokens: int, sampler) -> np.ndarray:
        """``max_new_tokens`` tokens behind every prompt, int [B, max_new_tokens]: ``prompt_ids`` [B, T] is padded on the right (-1)
        and sequence b has ``lengths[b]`` tokens; one prefill, then one token per step, each drawn by ``sampler`` (a
        ``sampling.Sampler`` of batch B) from the last row's logits."""
        prompt, lengths = np.asarray(prompt_ids), np.asarray(lengths)
        batch = prompt.shape[0]
        state = self.start_decoding(batch, int(lengths.max()) + int(max_new_tokens))
        logits = self.decode(prompt, state, new_lengths=lengths)
        out = []
        for step in range(int(max_new_tokens)):
            result = sampler(logits)
            out.append(result.numpy())
            if step + 1 < max_new_tokens:
                logits = self.decode(D.IdBuffer([batch, 1], result.ids._buf, result.ids.ptr), state)
        return np.stack(out, axis=1) if out else np.zeros([batch, 0], dtype=np.int64)
