"""Optimizers under the reference's call contract (reference optimizer.py:12-69).

Contract, as the layers use it: ``optimizer_.update(layer, '_w', grad)`` once per parameter at the end of
``backward``; the optimizer fetches the parameter with ``getattr``, changes it IN PLACE (aliases taken before the
backward must see the new values) and stores it back with ``setattr``.  The reference's own, unchanged
``optimizer.py`` drives the device layers just as well (``DeviceArray`` implements ``lr * grad`` and ``-=``); the
classes here are the same contract for machines where the reference is not importable, with

* SGD as one device ``axpy`` per parameter (``lr * grad`` stays symbolic until ``-=`` consumes it), and
* Adam as one kernel per parameter (``npm_adam_step``) on fp64 moments resident in HBM, with the reference's
  arithmetic operation for operation: the gradient products in the gradient's own float32, bias-corrected fp64 moments,
  epsilon INSIDE the square root, one rounding of the parameter; state keyed by ``f'{id(obj)}.{attribute}'``.
  Host arrays take the same arithmetic in NumPy.

Inside ``device.coalesced_updates()`` (what ``parallel.GradScope`` wraps a backward's deferred updates in) the launches
of parameters that are neighbours in memory -- a layer's ``device.ParamArena`` -- are joined: ONE axpy / ONE Adam kernel
per encoder step.  For that the Adam moments of a parameter live at the parameter's own
offset inside two fp64 buffers that mirror the pool block the parameter is a view of, so neighbours in the arena are
neighbours in the moments too; ``update`` is still called once per parameter and the state is still keyed per
``id(obj).attribute``.
"""

from __future__ import annotations

from typing import Optional

import numpy as np


class Optimizer:
    """``update`` is what layers call; subclasses implement ``update_variable``."""

    def update(self, obj: object, attribute: str, gradient) -> None:
        slot = f'{id(obj)}.{attribute}'
        setattr(obj, attribute, self.update_variable(slot, getattr(obj, attribute), gradient))

    def update_variable(self, identifier: str, variable, gradient):
        """Apply one step to ``variable`` in place and return it."""
        raise NotImplementedError


class SGDOptimizer(Optimizer):
    def __init__(self, learning_rate: float):
        self._learning_rate = learning_rate

    def update_variable(self, identifier, variable, gradient):
        variable -= self._learning_rate * gradient        # device operands: a single axpy kernel
        return variable


class _HostMoments:
    """Adam state of one parameter on the host (fp64, like the reference's np.zeros defaults)."""

    def __init__(self, shape):
        self.first = np.zeros(shape)
        self.second = np.zeros(shape)


class _BlockMoments:
    """fp64 first / second moments for EVERY element of one pool block (zero-initialised): a parameter that is a view
    of the block -- a slice of a ParamArena, one of the packed wq / wk / wv -- has its moments at the same element offset."""

    def __init__(self, block):
        from np_modeling_amd import _C, device as D
        self.count = max(block.nbytes // 4, 1)
        self.first, self.second = D._Buffer(8 * self.count), D._Buffer(8 * self.count)
        for buf in (self.first, self.second):
            _C.check(_C.lib(ordered=False).npm_fill_f64(buf.ptr, 0.0, self.count), 'npm_fill_f64')       # fresh buffers: no queued update touches them


class _DeviceMoments:
    """Adam state of one parameter in HBM: ``count`` doubles at ``first_ptr`` / ``second_ptr`` inside ``owner``."""

    def __init__(self, count: int, owner: _BlockMoments, offset: int):
        self.count, self.owner = count, owner
        self.first_ptr, self.second_ptr = owner.first.ptr + 8 * offset, owner.second.ptr + 8 * offset


class AdamOptimizer(Optimizer):
    """Adam as reference optimizer.py:36-69 computes it.  Positional order of the constructor: learning rate,
    beta1, beta2, epsilon."""

    def __init__(self, learning_rate: float, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-7):
        self.learning_rate, self.beta1, self.beta2, self.epsilon = learning_rate, beta1, beta2, epsilon
        self._state = {}          # identifier -> [next step number (from 1), moments]
        self._blocks = None       # pool block -> _BlockMoments (weak keys: the moments go when the block does)

    def _entry(self, identifier, make):
        entry = self._state.get(identifier)
        if entry is None or not make(entry[1]):
            entry = self._state[identifier] = [1, make(None)]
        return entry

    def update_variable(self, identifier, variable, gradient):
        from np_modeling_amd import device as D
        on_device = isinstance(variable, D.DeviceArray) and isinstance(gradient, (D.DeviceArray, D.Scaled)) \
            and gradient.size == variable.size
        if on_device:
            return self._step_on_device(identifier, variable, gradient)
        return self._step_on_host(identifier, variable, np.asarray(gradient))      # in its own dtype, as the reference uses it

    def _moments_for(self, variable, old):
        """The moments of ``variable`` at its offset inside its block's moment buffers.  A parameter that moved (into an
        arena; rebound to an array of the same size) takes its moments along."""
        import weakref
        from np_modeling_amd import _C
        if self._blocks is None:
            self._blocks = weakref.WeakKeyDictionary()
        block = variable._buf
        owner = self._blocks.get(block)
        if owner is None:
            owner = self._blocks[block] = _BlockMoments(block)
        new = _DeviceMoments(variable.size, owner, (variable.ptr - block.ptr) // 4)
        if isinstance(old, _DeviceMoments) and old.count == new.count:
            if old.first_ptr == new.first_ptr and old.owner is owner:
                return old
            if new.count:
                _C.check(_C.lib().npm_d2d(new.first_ptr, old.first_ptr, 8 * new.count), 'npm_d2d')
                _C.check(_C.lib().npm_d2d(new.second_ptr, old.second_ptr, 8 * new.count), 'npm_d2d')
        return new

    def _step_on_device(self, identifier, variable, gradient):
        from np_modeling_amd import _C, device as D
        if isinstance(gradient, D.Scaled):
            gradient = gradient.materialize()
        entry = self._state.get(identifier)
        if entry is None or not isinstance(entry[1], _DeviceMoments) or entry[1].count != variable.size:
            entry = self._state[identifier] = [1, None]             # fresh state (also after a host step or a resize)
        moments = entry[1] = self._moments_for(variable, entry[1])
        hyper = (float(self.learning_rate), float(self.beta1), float(self.beta2), float(self.epsilon), int(entry[0]))
        queue = D.UpdateQueue.active
        if queue is not None:                    # inside device.coalesced_updates(): joined with its neighbours at the end
            queue.adam(variable, gradient, moments.first_ptr, moments.second_ptr, hyper, moments.owner)
        else:
            _C.check(_C.lib().npm_adam_step(variable.ptr, gradient.ptr, moments.first_ptr, moments.second_ptr, variable.size,
                                            *hyper), 'npm_adam_step')
        entry[0] += 1
        return variable

    def _step_on_host(self, identifier, variable, grad):
        def make(old):
            if old is None:
                return _HostMoments(grad.shape)
            return isinstance(old, _HostMoments) and old.first.shape == grad.shape

        entry = self._entry(identifier, make)
        step, moments = entry
        b1, b2 = self.beta1, self.beta2
        moments.first = b1 * moments.first + (1.0 - b1) * grad
        moments.second = b2 * moments.second + (1.0 - b2) * np.square(grad)
        unbiased_first = moments.first / (1.0 - b1 ** step)
        unbiased_second = moments.second / (1.0 - b2 ** step)
        variable -= self.learning_rate * (unbiased_first / np.sqrt(unbiased_second + self.epsilon))
        entry[0] = step + 1
        return variable


def _decays_by_default(obj, attribute: str) -> bool:
    """The matrices and the embedding table (``_w``, ``_wq``, ``_w1`` ...) decay; biases, ``_gamma`` and ``_beta`` do not."""
    return attribute.startswith('_w')


class AdamWOptimizer(AdamOptimizer):
    """AdamW (decoupled weight decay, epsilon OUTSIDE the root: ``npm_adamw_step``, the update ``torch.optim.AdamW`` computes --
    NOT ``AdamOptimizer``'s arithmetic, which is the reference's) with gradient clipping by the global norm and a learning-rate
    schedule, for device parameters only.

    ``update(obj, attribute, grad)`` does NOT step: it records the gradient.  ``apply()`` -- which ``train.Trainer`` calls at the
    end of every backward, and a user who drives ``backward`` by hand calls themselves -- is the one point of a step where every
    gradient exists and no parameter has moved yet: it takes the norm of all recorded gradients (``npm_sumsq_ranges`` over the
    gradient buckets, 32 ranges a call, then ``npm_clip_finish``), and steps every parameter with a kernel that reads the clip
    factor from HBM.  Nothing in ``apply()`` copies anything to the host; ``last_grad_norm()`` is the one call that does (32
    bytes, and it synchronises).

    * ``learning_rate``: a float, or a callable ``step -> float`` called once per ``apply()`` with the 1-based count of applies.
    * ``decay(obj, attribute) -> bool`` says which parameters decay; by default those whose attribute starts with ``_w``.  The
      decay is part of an update's run key (``device.UpdateQueue.adamw``): neighbours of an arena that decay alike are one
      launch, a neighbour that decays differently starts another.  ``decay=lambda *_: True`` makes an arena one launch.
    * A norm that is not finite (an inf or a NaN in any gradient) makes the DEVICE skip the whole step: parameters and moments
      keep their bits.  The host cannot know that without a copy, so the per-parameter step counters (the bias correction)
      advance all the same; ``last_grad_norm()`` reports ``ok == False`` for such a step.
    * Data parallelism: ``parallel.GradScope._finish`` waits for the all-reduce before it calls ``update``, so every rank takes
      the norm of the same reduced gradients and arrives at the same factor with no further collective.
    * ``last`` = {'launches', 'updates', 'ranges', 'folds', 'fold_launches', 'fused_norm'} of the most recent ``apply()``.
    * ``accumulate=True``: gradient accumulation over several backwards (micro-batches).  The FIRST gradient a slot receives after
      an ``apply()`` is adopted as that slot's accumulator -- the bucket slice itself, kept alive as a pending gradient is;
      nothing is launched and nothing is zeroed.  A later ``update`` of the slot records the gradient as incoming, and ``fold()``
      adds every incoming gradient into its accumulator (``npm_accumulate_ranges``: one float32 addition per element, 32 joined
      pairs a call) and drops the incoming buffers.  ``apply(grad_scale)`` folds what is left, takes the norm of the SCALED sum
      and steps with ``grad_scale`` inside the clip factor, so the gradients themselves are never rescaled.  Where the last fold
      covers exactly the ranges of the norm, it produces the sum of squares in the same pass (``device.ACCUM_FUSED_NORM``): the
      bits of ``npm_sumsq_ranges`` afterwards, without that pass.  Memory: during micro-batches 2 .. k a SECOND set of gradients
      exists beside the accumulators, from its backward until the fold.  With one backward per ``apply()`` the calls and the bits
      are those of ``accumulate=False``, where a second gradient for a pending slot raises as it always did.
    """

    def __init__(self, learning_rate, beta1: float = 0.9, beta2: float = 0.999, epsilon: float = 1e-8,
                 weight_decay: float = 0.01, clip_norm: Optional[float] = None, decay=None, accumulate: bool = False):
        super().__init__(learning_rate, beta1, beta2, epsilon)
        if not weight_decay >= 0.0:
            raise ValueError(f'weight_decay must be >= 0, got {weight_decay!r}')
        if clip_norm is not None and not clip_norm > 0.0:
            raise ValueError(f'clip_norm must be positive (or None: no clipping), got {clip_norm!r}')
        self.weight_decay, self.clip_norm = float(weight_decay), None if clip_norm is None else float(clip_norm)
        self.decay = _decays_by_default if decay is None else decay
        self.last = None
        self.accumulate = bool(accumulate)
        self._pending = {}        # slot -> (obj, attribute, gradient), in update order; the gradient keeps its bucket alive
        self._incoming = {}       # accumulate: slot -> a later gradient, not yet folded into the pending one (its accumulator)
        self._folds = self._fold_launches = 0     # since the last apply()
        self._fused = False       # the most recent apply() took its sum of squares out of the last fold
        self._applies = 0
        self._clip_state = None   # 4 doubles in HBM: sumsq, norm, scale, ok
        self._clipped = False     # the most recent apply() wrote _clip_state

    def update(self, obj: object, attribute: str, gradient) -> None:
        from np_modeling_amd import device as D
        variable = getattr(obj, attribute)
        if isinstance(gradient, D.Scaled):
            gradient = gradient.materialize()
        if not isinstance(variable, D.DeviceArray) or not isinstance(gradient, D.DeviceArray):
            raise TypeError(f'AdamWOptimizer is device-only: {type(obj).__name__}.{attribute} is a {type(variable).__name__} with a '
                            f'{type(gradient).__name__} gradient')
        if gradient.size != variable.size:
            raise ValueError(f'{type(obj).__name__}.{attribute}: {variable.size} elements, gradient of {gradient.size}')
        slot = f'{id(obj)}.{attribute}'
        if slot in self._pending:
            if not self.accumulate:
                raise RuntimeError(f'{type(obj).__name__}.{attribute} already has a gradient waiting: call apply() after every backward '
                                   '(a second update would replace the first gradient, not add to it)')
            if slot in self._incoming:
                self.fold()
            self._incoming[slot] = gradient
            return
        self._pending[slot] = (obj, attribute, gradient)

    def _ranges(self):
        """The pending gradients as (address, elements): buffers in update order (a backward hands a bucket's slices over in
        its own order, not by address), the slices of one buffer by address, joined only where one starts EXACTLY where the one
        before ends -- the padding between slices of a bucket is uninitialised and never enters the norm.  A function of the
        update order and the addresses alone: every rank builds the same table."""
        buffers = {}
        for _, _, grad in self._pending.values():
            if grad.size:
                buffers.setdefault(id(grad._buf), []).append((grad.ptr, grad.size))
        out = []
        for slices in buffers.values():
            end = None
            for ptr, n in sorted(slices):
                if ptr == end:
                    out[-1][1] += n
                else:
                    out.append([ptr, n])
                end = ptr + 4 * n
        return out

    def _fold_pairs(self):
        """The incoming gradients as [accumulator address, gradient address, elements], ordered as ``_ranges()`` orders the
        accumulators and joined only where BOTH sides continue exactly: bucket padding never enters."""
        buffers = {}
        for slot, (_, _, acc) in self._pending.items():
            grad = self._incoming.get(slot)
            if grad is not None and acc.size:
                buffers.setdefault(id(acc._buf), []).append((acc.ptr, grad.ptr, acc.size))
        out = []
        for slices in buffers.values():
            ends = None
            for dst, src, n in sorted(slices):
                if (dst, src) == ends:
                    out[-1][2] += n
                else:
                    out.append([dst, src, n])
                ends = (dst + 4 * n, src + 4 * n)
        return out

    @staticmethod
    def _ranges_route(lib, pairs, with_sum: bool) -> bool:
        """npm_accumulate_ranges (True) or one npm_axpy per pair (False): ``device.ACCUM_RANGES`` where it is set; otherwise the
        ranges, except for a single pair without the sum -- the one shape measured slower than its yardstick (README)."""
        from np_modeling_amd import device as D
        if not hasattr(lib, 'npm_accumulate_ranges') or D.ACCUM_RANGES is False:
            return False
        return D.ACCUM_RANGES is True or with_sum or len(pairs) != 1

    def _fold(self, pairs, sumsq_state: int = 0) -> None:
        import ctypes as C
        from np_modeling_amd import _C, device as D
        lib = _C.lib()                          # a queued update drains first
        if self._ranges_route(lib, pairs, bool(sumsq_state)):
            for begin in range(0, len(pairs), _C.SUMSQ_MAX_RANGES):
                dst, src = _C.npm_ranges(), _C.npm_ranges()
                part = pairs[begin:begin + _C.SUMSQ_MAX_RANGES]
                for i, (d, g, n) in enumerate(part):
                    dst.ptr[i], src.ptr[i], dst.n[i], src.n[i] = d, g, n, n
                dst.count = src.count = len(part)
                _C.check(lib.npm_accumulate_ranges(C.byref(dst), C.byref(src), sumsq_state or None), 'npm_accumulate_ranges')
                self._fold_launches += 1
        else:                                   # the yardstick: 1 * g is exact, the same bits
            assert not sumsq_state
            for d, g, n in pairs:
                _C.check(lib.npm_axpy(d, g, 1.0, n), 'npm_axpy')
                self._fold_launches += 1
        self._folds += 1
        self._incoming = {}

    def fold(self) -> None:
        """Add every incoming gradient into its accumulator and drop the incoming buffers (``accumulate=True``; nothing to
        fold: nothing happens)."""
        if self._incoming:
            self._fold(self._fold_pairs())

    def _norm_on_device(self) -> int:
        import ctypes as C
        from np_modeling_amd import _C, device as D
        if self._clip_state is None:
            self._clip_state = D._Buffer(32)
        state = self._clip_state.ptr
        _C.check(_C.lib().npm_fill_f64(state, 0.0, 4), 'npm_fill_f64')
        ranges = self._ranges()
        pairs = self._fold_pairs() if self._incoming else []
        self._fused = bool(pairs) and D.ACCUM_FUSED_NORM and self._ranges_route(_C.lib(), pairs, True) \
            and [[d, n] for d, _, n in pairs] == ranges
        if self._fused:                         # the last fold touches every element the norm is over: the sum comes out of it
            self._fold(pairs, state)
            return len(ranges)
        if pairs:
            self._fold(pairs)
        for begin in range(0, len(ranges), _C.SUMSQ_MAX_RANGES):
            table = _C.npm_ranges()
            part = ranges[begin:begin + _C.SUMSQ_MAX_RANGES]
            for i, (ptr, n) in enumerate(part):
                table.ptr[i], table.n[i] = ptr, n
            table.count = len(part)
            _C.check(_C.lib().npm_sumsq_ranges(C.byref(table), state), 'npm_sumsq_ranges')
        return len(ranges)

    def _finish_scaled(self, max_norm: float, grad_scale: float) -> None:
        from np_modeling_amd import _C
        lib = _C.lib()
        if not hasattr(lib, 'npm_clip_finish_scaled'):
            raise _C.NpmError('AdamWOptimizer.apply(grad_scale != 1) needs npm_clip_finish_scaled, which the loaded library does not have')
        _C.check(lib.npm_clip_finish_scaled(self._clip_state.ptr, max_norm, grad_scale), 'npm_clip_finish_scaled')

    def apply(self, grad_scale: float = 1.0) -> None:
        """One step of every parameter whose gradient ``update`` recorded since the last ``apply()``.  ``grad_scale``: the factor
        the (accumulated) gradients are still to be multiplied with -- 1 / micro-batches for a mean loss, 1 / counted tokens for a
        summed one.  It travels inside the clip factor (``npm_clip_finish_scaled``); the norm reported and clipped is that of the
        scaled gradients.  1.0: exactly the calls of an optimizer without it."""
        from np_modeling_amd import _C, device as D
        if not self._pending:
            return
        grad_scale = float(grad_scale)
        if not 0.0 < grad_scale < float('inf'):
            raise ValueError(f'grad_scale must be positive and finite, got {grad_scale!r}')
        self._applies += 1
        lr = float(self.learning_rate(self._applies) if callable(self.learning_rate) else self.learning_rate)
        self._fused = False
        self._clipped = self.clip_norm is not None
        if self._clipped:
            ranges = self._norm_on_device()
            if grad_scale == 1.0:
                _C.check(_C.lib().npm_clip_finish(self._clip_state.ptr, self.clip_norm), 'npm_clip_finish')
            else:
                self._finish_scaled(self.clip_norm, grad_scale)
        else:
            ranges = 0
            self.fold()
            if grad_scale != 1.0:               # no norm: a zeroed state whose factor is float(grad_scale)
                if self._clip_state is None:
                    self._clip_state = D._Buffer(32)
                _C.check(_C.lib().npm_fill_f64(self._clip_state.ptr, 0.0, 4), 'npm_fill_f64')
                self._finish_scaled(float('inf'), grad_scale)
        clip = self._clip_state.ptr if self._clipped or grad_scale != 1.0 else 0
        direct = 0
        with D.coalesced_updates() as queue:
            before = queue.launches if queue is not None else 0
            for slot, (obj, attribute, gradient) in self._pending.items():
                variable = getattr(obj, attribute)
                entry = self._state.get(slot)
                if entry is None or not isinstance(entry[1], _DeviceMoments) or entry[1].count != variable.size:
                    entry = self._state[slot] = [1, None]
                moments = entry[1] = self._moments_for(variable, entry[1])
                decay = self.weight_decay if self.decay(obj, attribute) else 0.0
                hyper = (lr, float(self.beta1), float(self.beta2), float(self.epsilon), int(entry[0]), decay, clip)
                if queue is not None:
                    queue.adamw(variable, gradient, moments.first_ptr, moments.second_ptr, hyper, moments.owner)
                else:
                    _C.check(_C.lib().npm_adamw_step(variable.ptr, gradient.ptr, moments.first_ptr, moments.second_ptr, variable.size,
                                                     *hyper[:6], clip or None), 'npm_adamw_step')
                    direct += 1
                entry[0] += 1
        for obj, attribute, _ in self._pending.values():
            setattr(obj, attribute, getattr(obj, attribute))      # the reference's contract: changed in place, stored back
        self.last = {'launches': direct if queue is None else queue.launches - before, 'updates': len(self._pending), 'ranges': ranges,
                     'folds': self._folds, 'fold_launches': self._fold_launches, 'fused_norm': self._fused}
        self._pending = {}
        self._folds = self._fold_launches = 0

    def update_variable(self, identifier, variable, gradient):
        raise TypeError('AdamWOptimizer steps in apply(): update() records the gradient')

    def last_grad_norm(self):
        """(norm, scale, ok) of the most recent clipped ``apply()``: the global gradient norm, the factor the gradients were
        multiplied with, and whether the norm was finite (False: the device skipped that step).  Copies 32 bytes to the host
        and waits for the device; nothing else in this class does."""
        from np_modeling_amd import _C
        if not self._clipped:
            raise RuntimeError('last_grad_norm(): the most recent apply() did not clip (clip_norm is None, or no apply() yet)')
        state = np.zeros(4)
        _C.check(_C.lib().npm_d2h(state.ctypes.data, self._clip_state.ptr, 32), 'npm_d2h')
        return float(state[1]), float(state[2]), bool(state[3] != 0.0)


def warmup_cosine(peak: float, warmup_steps: int, total_steps: int, floor: float = 0.0):
    """A learning rate for ``AdamWOptimizer``: linear from ``peak / warmup_steps`` at step 1 to ``peak`` at ``warmup_steps``, half
    a cosine down to ``floor`` at ``total_steps``, ``floor`` from there on.  Steps count from 1."""
    import math
    peak, floor, warmup_steps, total_steps = float(peak), float(floor), int(warmup_steps), int(total_steps)
    if not 0 <= warmup_steps < total_steps:
        raise ValueError(f'need 0 <= warmup_steps < total_steps, got {warmup_steps} and {total_steps}')

    def rate(step: int) -> float:
        if step <= warmup_steps:
            return peak * step / warmup_steps
        if step >= total_steps:
            return floor
        return floor + 0.5 * (peak - floor) * (1.0 + math.cos(math.pi * (step - warmup_steps) / (total_steps - warmup_steps)))

    return rate
