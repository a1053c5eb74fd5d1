"""Sequential trainer with the interface and the printed output of reference train.py:13-46 (``Step:`` / ``Loss:``
lines, which the golden loss trajectories are parsed from).  Activations and gradients stay on the device from the
first layer to the loss and back; only the scalar loss comes to the host."""

from __future__ import annotations

import inspect
import logging
from typing import Optional, Sequence

from np_modeling_amd import loss as losses
from np_modeling_amd.layers.layer import Layer

log = logging.getLogger(__name__)


class Trainer:
    def __init__(self, layers: Sequence[Layer], loss_: Optional['losses.Loss'] = None):
        self._loss = losses.MSELoss() if loss_ is None else loss_
        self._layers = layers

    def _predict(self, batch):
        for stage in self._layers:
            log.debug('forward: %s', stage.name)
            batch = stage(batch)
        return batch

    def _backward(self, optimizer_) -> None:
        grad = self._loss(backprop=True)
        for stage in self._layers[::-1]:
            log.debug('backward: %s', stage.name)
            grad = stage(grad, backprop=True, optimizer_=optimizer_)

    def _backpropagate(self, optimizer_) -> None:
        self._backward(optimizer_)
        # an optimizer that steps once per backward, with every gradient in hand (optimizer.AdamWOptimizer: the global norm)
        apply = getattr(optimizer_, 'apply', None)
        if apply is not None:
            apply()

    def train(self, inputs, targets, steps: int, optimizer_, micro_batches: int = 1) -> None:
        """``micro_batches`` = k > 1: gradient accumulation.  Every step runs forward and backward on k equal, contiguous parts of the
        batch (views of the one upload, made once per call), the optimizer (``AdamWOptimizer(accumulate=True)``) sums their
        gradients and steps once.  A loss that counts its targets (``SoftmaxCrossEntropyLoss``) must be ``reduction='sum'``: the
        step then uses 1 / (all counted tokens) and ``Loss:`` is the token mean of the whole batch; any other loss is taken as a
        mean over its part, the step uses 1 / k and ``Loss:`` is the mean of the k losses.  Each micro-backward keeps its
        all-reduce."""
        # one upload for the whole loop; a first layer or a loss that takes something else than floats (token ids) says how
        first = self._layers[0] if len(self._layers) else None
        inputs = first.resident_inputs(inputs) if hasattr(first, 'resident_inputs') else self._resident(inputs)
        targets = self._loss.resident_targets(targets) if hasattr(self._loss, 'resident_targets') else self._resident(targets)
        if micro_batches != 1:
            return self._train_accumulating(inputs, targets, steps, optimizer_, micro_batches)
        for index in range(steps):
            print('Step: ', index)
            print('Loss: ', self._loss(self._predict(inputs), targets))
            self._backpropagate(optimizer_)

    def _train_accumulating(self, inputs, targets, steps: int, optimizer_, k) -> None:
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f'micro_batches must be a positive integer, got {k!r}')
        if not (hasattr(optimizer_, 'fold') and hasattr(optimizer_, 'apply') and getattr(optimizer_, 'accumulate', False)):
            raise ValueError(f'micro_batches={k} needs an optimizer that accumulates gradients (AdamWOptimizer(accumulate=True)), '
                             f'got {type(optimizer_).__name__}')
        counted = hasattr(self._loss, 'count')
        if counted and getattr(self._loss, 'reduction', None) != 'sum':
            raise ValueError(f"micro_batches={k} needs {type(self._loss).__name__}(reduction='sum'): a mean of per-micro-batch means is "
                             'not the batch mean when the counts of padded micro-batches differ')
        parts = list(zip(self._micro_views(inputs, k, 'inputs'), self._micro_views(targets, k, 'targets')))
        for index in range(steps):
            print('Step: ', index)
            total, count = 0.0, 0
            for j, (x, t) in enumerate(parts):
                total += self._loss(self._predict(x), t)
                count += self._loss.count if counted else 1
                self._backward(optimizer_)
                if j < k - 1:
                    optimizer_.fold()
            count = max(count, 1)
            print('Loss: ', total / count)
            optimizer_.apply(grad_scale=1.0 / count)

    @staticmethod
    def _micro_views(array, k: int, what: str):
        """``k`` contiguous views of a resident array along its leading dimension: no copy, nothing through the host."""
        from np_modeling_amd import device as D
        shape = tuple(array.shape)
        if not shape or shape[0] % k:
            raise ValueError(f'micro_batches={k} does not divide the leading dimension of the {what}, shape {shape}')
        part = (shape[0] // k,) + shape[1:]
        n = D._prod(part)
        if isinstance(array, D.IdBuffer):
            return [D.IdBuffer(part, array._buf, array.ptr + 4 * j * n) for j in range(k)]
        return [array.flat_view(j * n, part) for j in range(k)]

    @staticmethod
    def _resident(array):
        """A device copy of a host array, made ONCE per call (the arguments are fixed for the duration of a call)."""
        from np_modeling_amd import device as D
        return D.as_device(array)

    def eval(self, inputs, targets) -> None:
        no_grad = {'need_grad': False} if 'need_grad' in inspect.signature(self._loss.forward).parameters else {}
        print('Loss: ', self._loss(self._predict(inputs), targets, **no_grad))
