"""Token embedding: a [vocab, features] table looked up by integer ids (the reference has no such layer; the call protocol is
that of layers/layer.py).

``forward(ids)``: host integers or a ``device.IdBuffer`` (``sampling.Sampler``'s ``.ids``) of any shape -> [..., features],
one row gather on the device (``npm_take_rows``); an id outside the table, such as the -1 of a finished sequence, gives a row of
zeros.  ``backward(dy, optimizer_)`` is deterministic: the host sorts the ids stably and ``npm_embedding_bwd`` sums the ``dy`` rows
of each distinct token in ascending row order in fp32, without atomics; tokens that did not occur get zero rows, and the dense
[vocab, features] gradient goes through the usual deferred update, so every optimizer works unchanged.  There is no input
gradient: ``backward`` returns None.
"""

from __future__ import annotations

import numpy as np

from np_modeling_amd import device as D
from np_modeling_amd import parallel
from np_modeling_amd.layers import layer


class Embedding(layer.StatefulLayer):
    def __init__(self, vocab: int, features: int, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if int(vocab) < 1 or int(features) < 1:
            raise ValueError(f'Embedding: vocab and features must be at least 1, got {vocab!r}, {features!r}')
        self._vocab, self._features = int(vocab), int(features)

    def initialize(self, *_inputs, **_kwargs) -> None:
        self._w = self._new_param([self._vocab, self._features])
        self._pack_parameters([[(self, '_w')]])

    resident_inputs = staticmethod(D.as_ids)     # Trainer.train: integer inputs stay integers, uploaded once

    def forward(self, ids):
        self._ids = D.as_ids(ids)
        return D.take_rows(self._param('_w'), self._ids)

    def backward(self, dy, optimizer_):
        dy = D.as_device(dy)
        ids = self._ids.numpy()                      # ids that lived on the device are copied: training ids come from the host
        if dy.shape != tuple(ids.shape) + (self._features,):
            raise ValueError(f'Embedding.backward: dy {dy.shape} does not match the ids {ids.shape} of the last forward')
        with parallel.grad_scope(self._vocab * self._features + 8, self._arena) as scope:
            dw = scope.take([self._vocab, self._features], owner=(self, '_w'))
            D.embedding_bwd(dy, ids, dw)
            scope.defer(optimizer_, self, '_w', dw)
        return None

    @property
    def w(self):
        assert self._initialized
        return self._param('_w')
