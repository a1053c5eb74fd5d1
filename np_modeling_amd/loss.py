"""Losses with the reference's interface (reference loss.py:10-39), and ``SoftmaxCrossEntropyLoss``: logits and token ids in, the
loss and its gradient out of one launch -- what training a language model needs (the reference has no such loss).

When the network output is a ``DeviceArray`` the loss value is reduced on the device (fp64
accumulation, one scalar copied back) and the gradient stays on the device, so a Trainer step
never copies activations to the host; host inputs take the NumPy path.
"""

from __future__ import annotations

import abc
import ctypes as C

import numpy as np

from np_modeling_amd import _C
from np_modeling_amd import device as D
from np_modeling_amd.layers import layer


class Loss(layer.Layer):
    @abc.abstractmethod
    def forward(self, *args, **kwargs) -> float:
        pass

    @abc.abstractmethod
    def backward(self, *args, **kwargs):
        pass

    def _device_targets(self, targets, shape):
        """Host targets are read afresh at every forward, as the reference does (a caller may refill the same
        array in place between steps); ``Trainer.train`` uploads them once before its loop instead."""
        if isinstance(targets, D.DeviceArray):
            if tuple(targets.shape) == tuple(shape):
                return targets
            # ``y - targets`` broadcasts in the reference (loss.py:24,28): resident targets of another, broadcastable
            # shape ([B, 1], a scalar) are expanded once per (targets, shape) -- the kernels read y.size elements
            cached = getattr(self, '_expanded', None)
            if cached is None or cached[0] is not targets or cached[1] != tuple(shape):
                wide = np.broadcast_to(np.asarray(targets, dtype=np.float32), shape)    # ValueError if not broadcastable
                self._expanded = cached = (targets, tuple(shape), D.from_host(wide))
            return cached[2]
        return D.from_host(np.broadcast_to(np.asarray(targets, dtype=np.float32), shape))


class MSELoss(Loss):
    """sum((y - t)^2) / y.size and its gradient 2 (y - t) / y.size (loss.py:21-29)."""

    def forward(self, y, targets) -> float:
        self._y = y
        if isinstance(y, D.DeviceArray):
            self._targets = self._device_targets(targets, y.shape)
            value = C.c_double()
            _C.check(_C.lib().npm_mse_fwd(y.ptr, self._targets.ptr, y.size, C.byref(value)), 'npm_mse_fwd')
            return np.float64(value.value)
        self._y = np.asarray(y)
        self._targets = np.asarray(targets)
        delta = self._y - self._targets
        return np.sum(delta ** 2) / self._y.size

    def backward(self, *args, **kwargs):
        if isinstance(self._y, D.DeviceArray):
            dy = D.empty(self._y.shape)
            _C.check(_C.lib().npm_mse_bwd(self._y.ptr, self._targets.ptr, dy.ptr, dy.size), 'npm_mse_bwd')
            return dy
        return 2 * (self._y - self._targets) / self._y.size


class CrossEntropyLoss(Loss):
    """-sum(t * log(y)) and -t / y (loss.py:33-39)."""

    def forward(self, y, targets) -> float:
        self._y = y
        if isinstance(y, D.DeviceArray):
            self._targets = self._device_targets(targets, y.shape)
            value = C.c_double()
            _C.check(_C.lib().npm_xent_fwd(y.ptr, self._targets.ptr, y.size, C.byref(value)), 'npm_xent_fwd')
            return np.float64(value.value)
        self._y = np.asarray(y)
        self._targets = np.asarray(targets)
        return -np.sum(self._targets * np.log(self._y))

    def backward(self, *args, **kwargs):
        if isinstance(self._y, D.DeviceArray):
            dy = D.empty(self._y.shape)
            _C.check(_C.lib().npm_xent_bwd(self._y.ptr, self._targets.ptr, dy.ptr, dy.size), 'npm_xent_bwd')
            return dy
        return -self._targets / self._y


def _xent_numpy(z, t, e, grad_scale, need_grad):
    """Rows of softmax cross-entropy in fp64 with the rules of include/npm_hip.h npm_softmax_xent_rows: z [R, V] float64, t [R]
    integers.  Returns (row_loss, lse, gradient or None)."""
    rows, vocab = z.shape
    row_loss, lse = np.zeros(rows), np.full(rows, np.nan)
    grad = np.zeros((rows, vocab)) if need_grad else None
    with np.errstate(all='ignore'):
        for r in range(rows):
            if t[r] < 0:
                continue
            zr = z[r]
            m = zr.max() if vocab else -np.inf
            bad = t[r] >= vocab or not (np.isfinite(m) and not np.isnan(zr).any())
            if bad:
                row_loss[r] = np.nan
                if need_grad:
                    grad[r] = np.nan
                continue
            s = np.exp(zr - m).sum()
            lse[r] = m + np.log(s)
            row_loss[r] = lse[r] - (1.0 - e) * zr[t[r]] - (e / vocab * zr.sum() if e else 0.0)
            if need_grad:
                g = np.exp(zr - lse[r]) - e / vocab
                g[t[r]] -= 1.0 - e
                g[np.isneginf(zr)] = 0.0
                grad[r] = grad_scale * g
    return row_loss, lse, grad


class SoftmaxCrossEntropyLoss(Loss):
    """Cross-entropy of ``softmax(logits)`` against token ids, from the logits (include/npm_hip.h npm_softmax_xent_rows):

        loss_r = lse_r - (1 - e) z[r, t_r] - (e / V) sum_j z[r, j],        e = label_smoothing in [0, 1)

    in place of ``Softmax`` + ``CrossEntropyLoss`` over a one-hot float tensor of the logits' shape.  One launch reads the logits
    once and produces the loss, the per-token losses and the gradient w.r.t. the logits.

    ``forward(logits, targets, need_grad=True)``: ``logits`` [..., V], a ``DeviceArray`` (a NumPy array takes a NumPy path with
    the same rules, in fp64); ``targets`` of shape ``logits.shape[:-1]``, host integers or a ``device.IdBuffer``.  Host targets
    are checked at every forward -- an integer dtype, the shape, no id >= V, no negative id but ``ignore_index`` -- and uploaded
    when the array object or its contents differ from the last upload (a caller may refill the same array between steps).  A
    target equal to ``ignore_index`` contributes no loss and a zero gradient row and its logits are not read; a non-negative
    ``ignore_index`` becomes -1 on the host.  In an ``IdBuffer`` every negative id is ignored (only a negative ``ignore_index`` is
    accepted with a caller's own buffer; the one ``resident_targets`` makes from host targets is already mapped), and an id >= V gives a NaN loss and a NaN gradient row instead of an error.

    ``reduction``: 'mean' divides the sum by the number of targets that are not ignored (by 1 when there is none), 'sum' does
    not.  That number is counted on the host: for an ``IdBuffer`` this costs one copy of 4 bytes per row per distinct buffer object
    (cached by identity; ``resident_targets`` already knows it).  The gradient carries the same factor and comes out of the same
    launch: into a fresh ``DeviceArray``, or with ``inplace=True`` OVER THE LOGITS -- the caller's logits are gone after forward.
    ``need_grad=False`` writes no gradient and allocates none: the evaluation path.

    After ``forward``: ``row_loss`` (per-token negative log-likelihood, 0 where ignored) and ``lse`` (per-row log-sum-exp, NaN where
    ignored), shaped like the targets; ``count``; ``perplexity()`` = exp(sum(row_loss) / count), defined for
    ``label_smoothing == 0`` only.  ``backward()`` returns the gradient of the last forward, shaped like ``logits``.

    Data parallelism: 'mean' is the mean over THIS rank's counted tokens.  Ranks whose counts differ should use 'sum' and scale by
    their global count themselves; nothing here exchanges counts."""

    def __init__(self, ignore_index: int = -1, label_smoothing: float = 0.0, reduction: str = 'mean', inplace: bool = False):
        super().__init__()
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)):
            raise ValueError(f'SoftmaxCrossEntropyLoss: ignore_index must be an integer, got {ignore_index!r}')
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f'SoftmaxCrossEntropyLoss: label_smoothing must be in [0, 1), got {label_smoothing!r}')
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"SoftmaxCrossEntropyLoss: reduction must be 'mean' or 'sum', got {reduction!r}")
        self._ignore, self._smoothing = int(ignore_index), float(np.float32(label_smoothing))
        self._reduction, self._inplace = reduction, bool(inplace)
        self._uploaded = None           # (host array object, its int32 contents, IdBuffer): the last upload of host targets
        self._known = None              # (IdBuffer, count, largest id or None): what the host knows about a resident buffer
        self._known_before = []         # the same of the buffers used before it (micro-batch views take turns): the last 16
        self._grad = None
        self.row_loss = self.lse = None
        self.count = 0
        self._sum = 0.0

    @property
    def reduction(self) -> str:
        return self._reduction

    # ---- targets ----------------------------------------------------------------------------------------------------------
    def _checked(self, targets) -> np.ndarray:
        """Host targets as int32 with every ignored position -1; ValueError for what is no token id."""
        host = np.asarray(targets)
        if host.dtype == np.bool_ or not np.issubdtype(host.dtype, np.integer):
            raise ValueError(f'SoftmaxCrossEntropyLoss: targets must be integers, got dtype {host.dtype}')
        stray = (host < 0) & (host != self._ignore)
        if stray.any():
            raise ValueError(f'SoftmaxCrossEntropyLoss: negative target {int(host[stray][0])} is not ignore_index ({self._ignore})')
        ids = np.where(host == self._ignore, -1, host)
        if ids.size and ids.max() >= 2 ** 31:
            raise ValueError('SoftmaxCrossEntropyLoss: targets do not fit int32')
        return np.ascontiguousarray(ids.astype(np.int32))

    def resident_targets(self, targets) -> D.IdBuffer:
        """Targets for many forwards (``Trainer.train``): checked and uploaded ONCE; the id range is checked against V at forward."""
        if isinstance(targets, D.IdBuffer):
            return targets                      # a caller's own buffer: forward applies the IdBuffer rules to it
        ids = self._checked(targets)
        buffer = D.ids_from_host(ids)
        self._known = (buffer, int((ids >= 0).sum()), int(ids.max()) if ids.size else -1)
        return buffer

    def _device_ids(self, targets, shape, vocab):
        """(IdBuffer, count) of one forward."""
        if isinstance(targets, D.IdBuffer):
            if self._known is not None and self._known[0] is not targets:       # one of several resident buffers taking turns
                self._known_before = ([self._known] + [k for k in self._known_before if k[0] is not self._known[0]])[:16]
                self._known = next((k for k in self._known_before if k[0] is targets), None)
            # the buffer resident_targets made from host targets holds -1 where ignore_index was: nothing left to map
            mapped = self._known is not None and self._known[0] is targets and self._known[2] is not None
            if self._ignore >= 0 and not mapped:
                raise ValueError('SoftmaxCrossEntropyLoss: in an IdBuffer only negative ids are ignored; '
                                 f'ignore_index={self._ignore} needs host targets')
            if tuple(targets.shape) != tuple(shape):
                raise ValueError(f'SoftmaxCrossEntropyLoss: targets {tuple(targets.shape)} do not match the logits {tuple(shape)} + (V,)')
            if self._known is None or self._known[0] is not targets:
                self._known = (targets, int((targets.numpy() >= 0).sum()), None)      # 4 bytes per row, once per buffer
            if self._known[2] is not None and self._known[2] >= vocab:
                raise ValueError(f'SoftmaxCrossEntropyLoss: target {self._known[2]} is outside the vocabulary of {vocab}')
            return targets, self._known[1]
        ids = self._checked(targets)
        if ids.shape != tuple(shape):
            raise ValueError(f'SoftmaxCrossEntropyLoss: targets {ids.shape} do not match the logits {tuple(shape)} + (V,)')
        if ids.size and ids.max() >= vocab:
            raise ValueError(f'SoftmaxCrossEntropyLoss: target {int(ids.max())} is outside the vocabulary of {vocab}')
        last = self._uploaded
        if last is None or last[0] is not targets or not np.array_equal(last[1], ids):
            self._uploaded = last = (targets, ids, D.ids_from_host(ids))
        return last[2], int((ids >= 0).sum())

    # ---- the loss ----------------------------------------------------------------------------------------------------------
    def forward(self, logits, targets, need_grad: bool = True) -> float:
        self._grad = None
        if not isinstance(logits, D.DeviceArray):
            return self._forward_host(logits, targets, need_grad)
        if logits.ndim < 1 or logits.shape[-1] < 1:
            raise ValueError(f'SoftmaxCrossEntropyLoss: logits must have shape [..., V] with V >= 1, got {logits.shape}')
        lib = _C.lib()
        if not hasattr(lib, 'npm_softmax_xent_rows'):
            raise _C.NpmError('SoftmaxCrossEntropyLoss needs npm_softmax_xent_rows, which the loaded library does not have')
        shape, vocab = logits.shape[:-1], logits.shape[-1]
        ids, count = self._device_ids(targets, shape, vocab)
        rows = logits.size // vocab
        scale = 1.0 / count if self._reduction == 'mean' and count > 0 else 1.0
        per_row = D.empty([2, rows])
        grad = (logits if self._inplace else D.empty(logits.shape)) if need_grad else None
        total = C.c_double()
        _C.check(lib.npm_softmax_xent_rows(logits.ptr, vocab, ids.ptr, rows, vocab, self._smoothing, scale,
                                           None if grad is None else grad.ptr, vocab, per_row.ptr,
                                           per_row.ptr + 4 * rows, C.byref(total)), 'npm_softmax_xent_rows')
        self.row_loss, self.lse = per_row.flat_view(0, shape), per_row.flat_view(rows, shape)
        self._grad, self.count, self._sum = grad, count, total.value
        return np.float64(total.value * scale)

    def _forward_host(self, logits, targets, need_grad):
        host = np.asarray(logits)
        if host.ndim < 1 or host.shape[-1] < 1:
            raise ValueError(f'SoftmaxCrossEntropyLoss: logits must have shape [..., V] with V >= 1, got {host.shape}')
        shape, vocab = host.shape[:-1], host.shape[-1]
        if isinstance(targets, D.IdBuffer):
            if self._ignore >= 0:
                raise ValueError('SoftmaxCrossEntropyLoss: in an IdBuffer only negative ids are ignored; '
                                 f'ignore_index={self._ignore} needs host targets')
            ids = targets.numpy()
        else:
            ids = self._checked(targets)
            if ids.size and ids.max() >= vocab:
                raise ValueError(f'SoftmaxCrossEntropyLoss: target {int(ids.max())} is outside the vocabulary of {vocab}')
        if ids.shape != tuple(shape):
            raise ValueError(f'SoftmaxCrossEntropyLoss: targets {ids.shape} do not match the logits {tuple(shape)} + (V,)')
        count = int((ids >= 0).sum())
        scale = 1.0 / count if self._reduction == 'mean' and count > 0 else 1.0
        row_loss, lse, grad = _xent_numpy(host.reshape(-1, vocab).astype(np.float64), ids.reshape(-1), self._smoothing, scale, need_grad)
        self.row_loss, self.lse, self.count, self._sum = row_loss.reshape(shape), lse.reshape(shape), count, float(row_loss.sum())
        if grad is not None:
            grad = grad.reshape(host.shape).astype(host.dtype if np.issubdtype(host.dtype, np.floating) else np.float64)
            if self._inplace and isinstance(logits, np.ndarray):
                logits[...] = grad
                grad = logits
        self._grad = grad
        return np.float64(self._sum * scale)

    def backward(self, *args, **kwargs):
        if self._grad is None:
            raise RuntimeError('SoftmaxCrossEntropyLoss.backward: the last forward wrote no gradient (need_grad=False), or none ran')
        return self._grad

    def perplexity(self) -> float:
        """exp of the mean negative log-likelihood over the counted tokens of the last forward."""
        if self._smoothing != 0.0:
            raise RuntimeError('SoftmaxCrossEntropyLoss.perplexity is defined for label_smoothing == 0 only')
        return float(np.exp(self._sum / max(self.count, 1)))
