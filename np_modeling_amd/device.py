"""``DeviceArray``: an fp32 tensor resident in MI355X HBM, plus typed wrappers over the C ABI.

The reference passes ``np.ndarray`` everywhere and relies on three behaviours that a
device tensor has to keep:

* parameters are updated IN PLACE by the optimizer (``variable -= lr * gradient``,
  reference optimizer.py:32) and tests hold aliases to them taken before ``backward``
  (reference layers/mlp_test.py:50-51,93-94) -> ``__isub__`` mutates device memory and
  returns ``self``; ``np.asarray(alias)`` always reads the current device contents;
* array-likes are assigned straight into private attributes (reference
  layers/utils.py:52-88) -> layers convert lazily with :func:`as_device`;
* ``copy.deepcopy(layer)`` (reference layers/attentions_test.py:72) -> ``__deepcopy__``.

Anything that is not on the hot path (losses, Adam's fp64 moment math) works through
``__array__``: the value is copied to the host and NumPy does the arithmetic.
"""

from __future__ import annotations

import ctypes as C
import heapq
import math
import numbers
import os
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from np_modeling_amd import _C

Shape = Tuple[int, ...]


def _prod(shape: Sequence[int]) -> int:
    return int(math.prod(int(s) for s in shape))


class _Buffer:
    """Owns one pool block; returns it to the stream-ordered pool when unreferenced."""

    __slots__ = ('ptr', 'nbytes', '__weakref__')

    def __init__(self, nbytes: int):
        lib = _C.lib(ordered=False)              # an allocation reads and writes no array
        out = C.c_void_p()
        _C.check(lib.npm_malloc(C.byref(out), max(int(nbytes), 4)), 'npm_malloc')
        self.ptr = out.value
        self.nbytes = int(nbytes)

    def __del__(self):
        ptr, self.ptr = getattr(self, 'ptr', None), None
        if ptr and _C._LIB is not None:
            try:
                _C._LIB.npm_free(ptr)
            except Exception:       # interpreter shutdown
                pass

    def __deepcopy__(self, memo):
        """A block of its own with the same bytes, ONCE per deepcopy (``memo``): everything that shared this block
        shares the copy.  (The default protocol would duplicate the owner of ``ptr``: two frees of one block.)"""
        key = ('np_modeling_amd._Buffer', id(self))
        buf = memo.get(key)
        if buf is None:
            buf = _Buffer(self.nbytes)
            if self.nbytes:
                _C.check(_C.lib().npm_d2d(buf.ptr, self.ptr, self.nbytes), 'npm_d2d')
            memo[key] = buf
            memo[id(buf)] = buf                  # keeps `buf` alive for the duration of the deepcopy
        return buf

    def __copy__(self):
        raise TypeError('a device block has one owner: share the _Buffer object or deepcopy it')

    def __reduce__(self):
        raise TypeError('device memory cannot be pickled: copy the array to the host (numpy()) first')


class Scaled:
    """``alpha * array`` kept symbolic so that ``variable -= lr * gradient`` is ONE axpy
    kernel instead of a temporary plus a subtraction.  Materialises on any other use."""

    __slots__ = ('array', 'alpha')

    def __init__(self, array: 'DeviceArray', alpha: float):
        self.array = array
        self.alpha = float(alpha)

    @property
    def shape(self):
        return self.array.shape

    @property
    def size(self):
        return self.array.size

    dtype = np.dtype(np.float32)

    def materialize(self) -> 'DeviceArray':
        out = empty(self.array.shape)
        _C.check(_C.lib().npm_scale(self.array.ptr, out.ptr, self.alpha, self.array.size), 'npm_scale')
        return out

    def __array__(self, dtype=None, copy=None):
        host = self.array.numpy() * np.float32(self.alpha)
        return host if dtype is None else host.astype(dtype)

    def __mul__(self, other):
        if isinstance(other, numbers.Real):
            return Scaled(self.array, self.alpha * float(other))
        return np.asarray(self) * other

    __rmul__ = __mul__

    def __neg__(self):
        return Scaled(self.array, -self.alpha)


class DeviceArray:
    """Contiguous row-major fp32 tensor in device memory (a view into a pool block)."""

    __slots__ = ('_buf', 'ptr', 'shape', '__weakref__')
    dtype = np.dtype(np.float32)
    __array_priority__ = 100.0

    def __init__(self, shape: Sequence[int], _buf: Optional[_Buffer] = None, _ptr: Optional[int] = None):
        self.shape = tuple(int(s) for s in shape)
        if _buf is None:
            _buf = _Buffer(4 * _prod(self.shape))
            _ptr = _buf.ptr
        self._buf = _buf
        self.ptr = _ptr

    # ---- metadata ---------------------------------------------------------------
    @property
    def size(self) -> int:
        return _prod(self.shape)

    @property
    def ndim(self) -> int:
        return len(self.shape)

    @property
    def nbytes(self) -> int:
        return 4 * self.size

    def __len__(self) -> int:
        if not self.shape:
            raise TypeError('len() of unsized object')
        return self.shape[0]

    def __repr__(self) -> str:
        return f'DeviceArray(shape={self.shape}, dtype=float32, ptr=0x{self.ptr:x})'

    # ---- views --------------------------------------------------------------------
    def reshape(self, *shape) -> 'DeviceArray':
        if len(shape) == 1 and not isinstance(shape[0], numbers.Integral):
            shape = tuple(shape[0])
        shape = [int(s) for s in shape]
        if shape.count(-1) > 1:
            raise ValueError('can only specify one unknown dimension')
        if -1 in shape:
            known = _prod([s for s in shape if s != -1])
            shape[shape.index(-1)] = self.size // known if known else 0
        if _prod(shape) != self.size:
            raise ValueError(f'cannot reshape array of size {self.size} into shape {tuple(shape)}')
        return DeviceArray(shape, self._buf, self.ptr)

    def flat_view(self, offset: int, shape: Sequence[int]) -> 'DeviceArray':
        """View of ``prod(shape)`` elements starting ``offset`` elements into this array."""
        n = _prod(shape)
        if offset < 0 or offset + n > self.size:
            raise ValueError('flat_view out of range')
        return DeviceArray(shape, self._buf, self.ptr + 4 * int(offset))

    # ---- host <-> device ----------------------------------------------------------
    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float32)
        if self.size:
            _C.check(_C.lib().npm_d2h(out.ctypes.data, self.ptr, out.nbytes), 'npm_d2h')
        return out

    def __array__(self, dtype=None, copy=None):
        host = self.numpy()
        return host if dtype is None or np.dtype(dtype) == np.float32 else host.astype(dtype)

    def set(self, value) -> 'DeviceArray':
        host = np.ascontiguousarray(np.broadcast_to(np.asarray(value, dtype=np.float32), self.shape))
        if host.size:
            _C.check(_C.lib().npm_h2d(self.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
        return self

    def copy(self) -> 'DeviceArray':
        out = DeviceArray(self.shape)
        if self.size:
            _C.check(_C.lib().npm_d2d(out.ptr, self.ptr, self.nbytes), 'npm_d2d')
        return out

    def __copy__(self):
        return self.copy()

    def __deepcopy__(self, memo):
        """Copies the OWNING pool block once per deepcopy (through ``memo``) and rebases this view into the copy:
        views that shared a block still share one afterwards -- the packed q/k/v projection parameters stay
        adjacent, and pointer views used as strided GEMM operands keep everything they address."""
        buf = self._buf.__deepcopy__(memo)
        return DeviceArray(self.shape, buf, buf.ptr + (self.ptr - self._buf.ptr))

    def astype(self, dtype, copy=True):
        if np.dtype(dtype) == np.float32:
            return self.copy() if copy else self
        return self.numpy().astype(dtype)

    # ---- in-place updates (the optimizer contract) -----------------------------------
    def _axpy(self, other, alpha: float) -> 'DeviceArray':
        if isinstance(other, Scaled):
            alpha, other = alpha * other.alpha, other.array
        if isinstance(other, numbers.Real):
            other = full(self.shape, float(other))
        elif not isinstance(other, DeviceArray) or other.size != self.size:
            host = np.asarray(other, dtype=np.float32)
            other = from_host(np.broadcast_to(host, self.shape))
        queue = UpdateQueue.active
        if queue is not None:                       # inside coalesced_updates(): launched, merged with its neighbours, at the end
            queue.axpy(self, other, float(alpha))
            return self
        _C.check(_C.lib().npm_axpy(self.ptr, other.ptr, float(alpha), self.size), 'npm_axpy')
        return self

    def __isub__(self, other):
        return self._axpy(other, -1.0)

    def __iadd__(self, other):
        return self._axpy(other, 1.0)

    def __imul__(self, other):
        if isinstance(other, numbers.Real):
            _C.check(_C.lib().npm_scale(self.ptr, self.ptr, float(other), self.size), 'npm_scale')
            return self
        return self.set(self.numpy() * np.asarray(other))

    # ---- arithmetic ---------------------------------------------------------------------
    def __mul__(self, other):
        if isinstance(other, numbers.Real):
            return Scaled(self, float(other))
        return self.numpy() * np.asarray(other)

    __rmul__ = __mul__

    def __neg__(self):
        return Scaled(self, -1.0)

    def __add__(self, other):
        if isinstance(other, DeviceArray) and other.shape == self.shape:
            out = empty(self.shape)
            _C.check(_C.lib().npm_add(self.ptr, other.ptr, out.ptr, self.size), 'npm_add')
            return out
        return self.numpy() + np.asarray(other)

    __radd__ = __add__

    def __sub__(self, other):
        return self.numpy() - np.asarray(other)

    def __rsub__(self, other):
        return np.asarray(other) - self.numpy()

    def __truediv__(self, other):
        if isinstance(other, numbers.Real):
            return Scaled(self, 1.0 / float(other))
        return self.numpy() / np.asarray(other)

    def __rtruediv__(self, other):
        return np.asarray(other) / self.numpy()

    def __pow__(self, other):
        return self.numpy() ** other

    def __getitem__(self, idx):
        return self.numpy()[idx]

    def __iter__(self):
        return iter(self.numpy())

    def sum(self, *a, **k):
        return self.numpy().sum(*a, **k)

    def mean(self, *a, **k):
        return self.numpy().mean(*a, **k)

    def max(self, *a, **k):
        return self.numpy().max(*a, **k)

    def min(self, *a, **k):
        return self.numpy().min(*a, **k)

    def __eq__(self, other):
        return self.numpy() == np.asarray(other)

    def __ne__(self, other):
        return self.numpy() != np.asarray(other)

    def __lt__(self, other):
        return self.numpy() < np.asarray(other)

    def __le__(self, other):
        return self.numpy() <= np.asarray(other)

    def __gt__(self, other):
        return self.numpy() > np.asarray(other)

    def __ge__(self, other):
        return self.numpy() >= np.asarray(other)

    __hash__ = None


ArrayLike = Union[DeviceArray, np.ndarray, Sequence]


# ---- constructors ------------------------------------------------------------------------
# ---- parameters back to back, updates in one launch ------------------------------------------------------------------
COALESCE_UPDATES = os.environ.get('NPM_COALESCE_UPDATES', '1') != '0'   # A/B switch: 0 = one optimizer launch per parameter (rounds 1-4)
_ALIGN = 4                                                              # floats: 16-byte aligned slices (GEMM / DMA operands)


# Gradient accumulation (optimizer.AdamWOptimizer(accumulate=True)), A/B switches.  ACCUM_RANGES: True / NPM_ACCUM_RANGES=1 folds with
# npm_accumulate_ranges whatever the shape, False / 0 with one npm_axpy per joined pair (the yardstick); None (unset) takes the ranges
# except for a single pair without the sum, which tools/accum_bench.py measured slower than npm_axpy.  ACCUM_FUSED_NORM: the last fold
# of a step also produces the sum of squares of the norm -- the same bits either way; on, because the fused call measured 0.73 - 0.83
# of fold + npm_sumsq_ranges at 12.6 M and 200 M elements (profiles/r28_accum_bench.log).
ACCUM_RANGES = {'0': False, '1': True}.get(os.environ.get('NPM_ACCUM_RANGES', ''))
ACCUM_FUSED_NORM = os.environ.get('NPM_ACCUM_FUSED_NORM', '1') != '0'


class _LayerRef:
    """Weak reference to a layer that survives ``copy.deepcopy`` of the structure holding it by pointing at the COPY of
    the layer (through the deepcopy memo).  A ParamArena is an attribute of the layer whose parameters it lists: strong
    references would make every layer a reference cycle, and its device memory would wait for the cycle collector."""
    __slots__ = ('_ref',)

    def __init__(self, obj):
        import weakref
        self._ref = weakref.ref(obj)

    def __call__(self):
        return self._ref()

    def __deepcopy__(self, memo):
        import copy
        target = self._ref()
        return _LayerRef(copy.deepcopy(target, memo)) if target is not None else self


class ParamArena:
    """The parameters of one layer (a composite's sub-layers included) back to back in ONE device buffer, in the order
    their gradients are produced by ``backward`` -- so that the flat gradient bucket of parallel.GradScope mirrors it
    slot for slot and ``parameter -= lr * gradient`` (reference optimizer.py:26-33; Adam: :53-67) is ONE launch over the
    whole range instead of one per parameter.

    ``segments`` is a list of lists of ``(layer, attribute)``; the parameters of one segment stay gap-free (the packed
    wq / wk / wv of MultiHeadAttention must remain adjacent), every segment starts 16-byte aligned.  Building the arena
    COPIES the current values and rebinds the attributes to views of it, so it is built where no outside alias of a
    parameter can exist yet (inside ``initialize``) or where one would be re-taken anyway (end of a composite's first
    forward; the reference's tests take their aliases after the first call).  A parameter that is rebound later
    (weight binders assign arrays into the private attributes, reference layers/utils.py:52-88) simply leaves the
    arena: ``offset_of`` returns None for it and it takes the per-parameter path again."""

    def __init__(self, segments):
        self.entries = []                            # [layer, attribute, offset, size]
        offset = 0
        for segment in segments:
            offset = (offset + _ALIGN - 1) // _ALIGN * _ALIGN
            for obj, attribute in segment:
                value = obj._param(attribute)
                self.entries.append([_LayerRef(obj), attribute, offset, value.size])
                offset += value.size
        self.size = (offset + _ALIGN - 1) // _ALIGN * _ALIGN
        self.flat = zeros([max(self.size, 1)])       # zeros: the alignment gaps are updated along with their neighbours
        for ref, attribute, off, n in self.entries:
            obj = ref()
            old = obj._param(attribute)
            view = self.flat.flat_view(off, old.shape)
            if n:
                _C.check(_C.lib().npm_d2d(view.ptr, old.ptr, 4 * n), 'npm_d2d')
            setattr(obj, attribute, view)

    def offset_of(self, obj, attribute: str, size: int) -> Optional[int]:
        """Where (in floats) ``obj.attribute`` starts inside the arena if ``size`` elements from there are still what
        the attribute(s) hold -- None once a binder has rebound it."""
        for ref, a, off, n in self.entries:
            if a == attribute and ref() is obj:
                value = getattr(obj, attribute)
                if isinstance(value, DeviceArray) and value.ptr == self.flat.ptr + 4 * off and value._buf is self.flat._buf \
                        and off + size <= self.size:
                    return off
                return None
        return None

    def live(self) -> int:
        """How many of the parameters are still where the arena put them."""
        return sum(ref() is not None and self.offset_of(ref(), a, n) == off for ref, a, off, n in self.entries)


class _Pending:
    """One queued update: ``n`` elements at ``var`` and ``grad`` (byte addresses inside the blocks ``var_buf`` / ``grad_buf``),
    side arrays ``extra`` = ((byte address, bytes per element), ...) and ``key`` = everything two updates must agree on to
    be one launch (kind, step size, Adam's hyper-parameters and step number)."""
    __slots__ = ('var', 'grad', 'n', 'key', 'var_buf', 'grad_buf', 'extra')

    def __init__(self, var, grad, n, key, var_buf, grad_buf, extra=()):
        self.var, self.grad, self.n, self.key, self.var_buf, self.grad_buf, self.extra = var, grad, n, key, var_buf, grad_buf, extra

    def continued_by(self, other: '_Pending') -> bool:
        """``other`` starts where this ends -- or up to 3 floats later, the alignment padding between two slices of an
        arena, which the blocks own on every side and which may be updated along (nothing reads it) -- on the parameter
        side, the gradient side and every side array alike."""
        gap = other.var - (self.var + 4 * self.n)
        if gap < 0 or gap > 4 * (_ALIGN - 1) or gap % 4 or self.key != other.key:
            return False
        if self.var_buf is not other.var_buf or self.grad_buf is not other.grad_buf or len(self.extra) != len(other.extra):
            return False
        if other.grad - (self.grad + 4 * self.n) != gap:
            return False
        return all(width == w2 and ptr2 - (ptr + width * self.n) == gap // 4 * width
                   for (ptr, width), (ptr2, w2) in zip(self.extra, other.extra))


class UpdateQueue:
    """Parameter updates issued inside ``coalesced_updates()`` are collected instead of launched; on exit, updates whose
    parameters AND gradients (AND Adam moments) are neighbours in memory -- a ParamArena and the gradient bucket that
    mirrors it -- run as one launch over the joined range.  The optimizer is not involved: the reference's unchanged
    ``SGDOptimizer.update_variable`` (``variable -= lr * gradient``, optimizer.py:32) reaches ``DeviceArray._axpy``
    exactly as before, once per ``Optimizer.update(obj, attribute, grad)``, with its ``id(obj).attribute`` keying.
    Elementwise updates do not care where a range is cut: results are bit-identical to the per-parameter launches.

    Program order is kept for everything an observer can tell apart (any ``Optimizer`` subclass may run in here, not only
    the shipped ones): queued updates are launched sorted by address, so only updates that touch DISJOINT memory wait in
    the queue together -- one that writes what a queued one reads or writes, or reads what a queued one writes (weight
    decay after the step, a momentum buffer updated and then applied), first drains the queue; and so does every library
    call that is not part of the queue (``*=``, ``numpy()``, ``set``, any kernel: ``_C.lib()`` calls ``_C._ORDER_HOOK``)."""

    active: Optional['UpdateQueue'] = None

    def __init__(self):
        self._pending = []
        self._keep = []
        self.launches = 0        # kernels launched by run()
        self.updates = 0         # updates they stand for
        self.drains = 0          # times the queue was emptied early to keep program order

    def _enqueue(self, item: '_Pending') -> None:
        def overlap(a_lo, a_n, b_lo, b_n):
            return a_lo < b_lo + 4 * b_n and b_lo < a_lo + 4 * a_n
        for p in self._pending:
            if overlap(item.var, item.n, p.var, p.n) or overlap(item.var, item.n, p.grad, p.n) or overlap(item.grad, item.n, p.var, p.n):
                self.drains += 1
                self.run()
                break
        self._pending.append(item)
        _C._ORDER_HOOK = self._drain

    def _drain(self) -> None:
        if self._pending:
            self.drains += 1
            self.run()

    def axpy(self, var: 'DeviceArray', grad: 'DeviceArray', alpha: float) -> None:
        self._enqueue(_Pending(var.ptr, grad.ptr, var.size, ('axpy', alpha), var._buf, grad._buf))
        self._keep.append(grad)                     # a temporary (``lr * host_array``) must outlive the deferred launch; AFTER
        #                                             _enqueue, whose drain of an overlapping update ends with ``_keep = []``

    def adam(self, var: 'DeviceArray', grad: 'DeviceArray', first_ptr: int, second_ptr: int, hyper: tuple, owner) -> None:
        """``hyper`` = (lr, beta1, beta2, epsilon, step); ``owner`` keeps the moment buffers alive until run()."""
        self._enqueue(_Pending(var.ptr, grad.ptr, var.size, ('adam',) + tuple(hyper), var._buf, grad._buf,
                               ((first_ptr, 8), (second_ptr, 8))))
        self._keep += [owner, grad]                 # after _enqueue: a drain in there empties _keep, and this update is still pending

    def adamw(self, var: 'DeviceArray', grad: 'DeviceArray', first_ptr: int, second_ptr: int, hyper: tuple, owner) -> None:
        """``hyper`` = (lr, beta1, beta2, epsilon, step, weight decay, address of the clip state or 0): all of it is the run key,
        so neighbours that decay differently are separate launches.  Side arrays and adjacency as ``adam``."""
        self._enqueue(_Pending(var.ptr, grad.ptr, var.size, ('adamw',) + tuple(hyper), var._buf, grad._buf,
                               ((first_ptr, 8), (second_ptr, 8))))
        self._keep += [owner, grad]

    def run(self) -> None:
        _C._ORDER_HOOK = None                       # the launches below are the queue itself
        lib = _C.lib(ordered=False)
        pending, self._pending = sorted(self._pending, key=lambda u: (u.key[0], u.var)), []
        self.updates += len(pending)
        run: Optional[_Pending] = None
        for item in pending + [None]:
            if run is not None and item is not None and run.continued_by(item):
                run.n = (item.var - run.var) // 4 + item.n
                continue
            if run is not None and run.n:
                if run.key[0] == 'axpy':
                    _C.check(lib.npm_axpy(run.var, run.grad, run.key[1], run.n), 'npm_axpy')
                elif run.key[0] == 'adamw':
                    lr, b1, b2, eps, step, decay, clip = run.key[1:]
                    _C.check(lib.npm_adamw_step(run.var, run.grad, run.extra[0][0], run.extra[1][0], run.n, lr, b1, b2, eps,
                                                step, decay, clip or None), 'npm_adamw_step')
                else:
                    lr, b1, b2, eps, step = run.key[1:]
                    _C.check(lib.npm_adam_step(run.var, run.grad, run.extra[0][0], run.extra[1][0], run.n, lr, b1, b2, eps,
                                               step), 'npm_adam_step')
                self.launches += 1
            run = item
        self._keep = []


class coalesced_updates:
    """``with coalesced_updates():`` -- see UpdateQueue.  Nests: an inner context joins the outer one."""

    def __enter__(self) -> UpdateQueue:
        self._mine = UpdateQueue.active is None and COALESCE_UPDATES
        if self._mine:
            UpdateQueue.active = UpdateQueue()
        return UpdateQueue.active

    def __exit__(self, exc_type, exc, tb) -> bool:
        if self._mine:
            queue, UpdateQueue.active = UpdateQueue.active, None
            _C._ORDER_HOOK = None
            if exc_type is None:
                queue.run()
        return False


def empty(shape: Sequence[int]) -> DeviceArray:
    return DeviceArray(shape)


def full(shape: Sequence[int], value: float) -> DeviceArray:
    out = DeviceArray(shape)
    if out.size:
        _C.check(_C.lib().npm_fill_f32(out.ptr, float(value), out.size), 'npm_fill_f32')
    return out


def zeros(shape: Sequence[int]) -> DeviceArray:
    return full(shape, 0.0)


def from_host(value) -> DeviceArray:
    host = np.ascontiguousarray(np.asarray(value, dtype=np.float32))
    out = DeviceArray(host.shape)
    if host.size:
        _C.check(_C.lib().npm_h2d(out.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
    return out


class ByteBuffer:
    """Raw device bytes (dropout masks)."""

    __slots__ = ('_buf', 'ptr', 'nbytes')

    def __init__(self, nbytes: int):
        self._buf = _Buffer(nbytes)
        self.ptr, self.nbytes = self._buf.ptr, int(nbytes)

    def numpy(self) -> np.ndarray:
        host = np.empty([self.nbytes], dtype=np.uint8)
        if self.nbytes:
            _C.check(_C.lib().npm_d2h(host.ctypes.data, self.ptr, self.nbytes), 'npm_d2h')
        return host

    def __deepcopy__(self, memo):
        out = ByteBuffer.__new__(ByteBuffer)
        out._buf = self._buf.__deepcopy__(memo)
        out.ptr, out.nbytes = out._buf.ptr, self.nbytes
        return out


class HalfBuffer(ByteBuffer):
    """Raw device storage of ``shape`` IEEE fp16 elements: the K or V tensor of a half-precision ``KVCache``.  It has a shape, an
    address and a size, and no arithmetic: nothing outside the cache classes reads it as floats (``npm_kv_gather_f16`` is how its
    rows come back as fp32).  ``numpy()``: the stored halves, for tests."""

    __slots__ = ('shape',)

    def __init__(self, shape: Sequence[int]):
        self.shape = tuple(int(s) for s in shape)
        ByteBuffer.__init__(self, 2 * _prod(self.shape))

    def numpy(self) -> np.ndarray:
        return ByteBuffer.numpy(self).view(np.float16).reshape(self.shape)

    def __deepcopy__(self, memo):
        out = HalfBuffer.__new__(HalfBuffer)
        out._buf = self._buf.__deepcopy__(memo)
        out.ptr, out.nbytes, out.shape = out._buf.ptr, self.nbytes, self.shape
        return out


class IdBuffer(ByteBuffer):
    """``shape`` int32 values on the device: token ids, row indices.  What ``sampling.Sampler`` returns as ``.ids`` and what
    ``take_rows`` / ``layers.embedding.Embedding`` take as indices without a trip through the host."""

    __slots__ = ('shape',)

    def __init__(self, shape: Sequence[int], _buf: Optional[_Buffer] = None, _ptr: Optional[int] = None):
        self.shape = tuple(int(s) for s in shape)
        if _buf is None:
            ByteBuffer.__init__(self, 4 * _prod(self.shape))
        else:
            self._buf, self.ptr, self.nbytes = _buf, _ptr, 4 * _prod(self.shape)

    @property
    def size(self) -> int:
        return _prod(self.shape)

    def numpy(self) -> np.ndarray:
        host = np.empty(self.shape, dtype=np.int32)
        if host.size:
            _C.check(_C.lib().npm_d2h(host.ctypes.data, self.ptr, host.nbytes), 'npm_d2h')
        return host

    def __deepcopy__(self, memo):
        buf = self._buf.__deepcopy__(memo)
        return IdBuffer(self.shape, buf, buf.ptr + (self.ptr - self._buf.ptr))


def ids_from_host(value) -> IdBuffer:
    """Integers of any shape as int32 on the device (ValueError for anything that is not integral or does not fit)."""
    host = np.asarray(value)
    if host.dtype == np.bool_ or not np.issubdtype(host.dtype, np.integer):
        raise ValueError(f'indices must be integers, got dtype {host.dtype}')
    if host.size and (host.min() < -2 ** 31 or host.max() >= 2 ** 31):
        raise ValueError('indices do not fit int32')
    host = np.ascontiguousarray(host.astype(np.int32))
    out = IdBuffer(host.shape)
    if host.size:
        _C.check(_C.lib().npm_h2d(out.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
    return out


def as_ids(value) -> IdBuffer:
    return value if isinstance(value, IdBuffer) else ids_from_host(value)


def bytes_from_host(value: np.ndarray) -> ByteBuffer:
    host = np.ascontiguousarray(value).view(np.uint8)
    out = ByteBuffer(host.nbytes)
    if host.nbytes:
        _C.check(_C.lib().npm_h2d(out.ptr, host.ctypes.data, host.nbytes), 'npm_h2d')
    return out


def as_device(value) -> DeviceArray:
    """DeviceArray as is; ``Scaled`` materialised; anything else (np.ndarray, jax Array,
    nested lists) copied to the device as contiguous fp32."""
    if isinstance(value, DeviceArray):
        return value
    if isinstance(value, Scaled):
        return value.materialize()
    return from_host(value)


def synchronize() -> None:
    _C.check(_C.lib().npm_sync(), 'npm_sync')


def pool_stats() -> Tuple[int, int]:
    used, reserved = C.c_size_t(), C.c_size_t()
    _C.check(_C.lib().npm_pool_stats(C.byref(used), C.byref(reserved)))
    return used.value, reserved.value


def trim_pool() -> None:
    """Hand the cached (free) blocks of the pool back to the driver (between workloads of different shapes)."""
    import gc
    gc.collect()
    _C.check(_C.lib().npm_pool_trim(), 'npm_pool_trim')


class Event:
    """HIP event on the compute stream (bench.py times kernels with these)."""

    def __init__(self):
        self._h = C.c_void_p()
        _C.check(_C.lib().npm_event_create(C.byref(self._h)), 'npm_event_create')

    def record(self) -> 'Event':
        _C.check(_C.lib().npm_event_record(self._h), 'npm_event_record')
        return self

    def synchronize(self) -> None:
        _C.check(_C.lib().npm_event_sync(self._h), 'npm_event_sync')

    def elapsed_ms(self, end: 'Event') -> float:
        ms = C.c_float()
        _C.check(_C.lib().npm_event_elapsed_ms(self._h, end._h, C.byref(ms)), 'npm_event_elapsed_ms')
        return float(ms.value)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h and _C._LIB is not None:
            try:
                _C._LIB.npm_event_destroy(h)
            except Exception:
                pass


# ---- kernel wrappers -------------------------------------------------------------------------
FUSE_COLSUM = os.environ.get('NPM_FUSE_COLSUM', '1') != '0'      # A/B switches (see gemm, attentions.py)
FUSE_SOFTMAX_BWD = os.environ.get('NPM_FUSE_SOFTMAX_BWD', '1') != '0'
FUSE_BSUM = os.environ.get('NPM_FUSE_BSUM', '1') != '0'          # bias gradient inside the weight-gradient GEMM
PACK_QKV = os.environ.get('NPM_PACK_QKV', '1') != '0'
ATTN_CORE = os.environ.get('NPM_ATTN_CORE', '1') != '0'            # fused attention core (npm_mha_core_*) where it applies
# Whether the forward keeps the raw scores for the backward.  The fp32 matrix rate is the scarce resource at the large
# head sizes (a 32 x 32 score tile costs 64 MFMAs to recompute at D = 128, 16 loads to read back: forward + backward of the C4
# core 6.6 ms with saved scores against 7.5 ms recomputing); the score tensor does not shrink with the head size while the
# matrix work does, so at small head sizes writing and reading it is what the kernels wait for (H D = 1024, B 256, S 512,
# forward + backward: D 64 7.6 saved / 7.9 ms recomputed, D 32 8.8 / 8.7, D 16 13.4 / 10.4: profiles/r04_attn_modes.log).
# Default: keep them from head size 64 up.  NPM_ATTN_SAVE_SCORES=1 / 0 forces either mode everywhere (0 is the memory-lean
# mode: log-sum-exp only, 2.1 GB less at C4 / C5).
_save = os.environ.get('NPM_ATTN_SAVE_SCORES', '')
ATTN_SAVE_SCORES: Optional[bool] = None if _save == '' else _save != '0'
ATTN_SAVE_SCORES_FROM = 64


def attn_save_scores(head_size: int) -> bool:
    return head_size >= ATTN_SAVE_SCORES_FROM if ATTN_SAVE_SCORES is None else bool(ATTN_SAVE_SCORES)


# masked attention: let the fused kernels skip tiles without an allowed position (NPM_ATTN_TILE_SKIP=0: visit them all)
ATTN_TILE_SKIP = os.environ.get('NPM_ATTN_TILE_SKIP', '1') != '0'
# head size 128: the attention backward's row terms (dctx . ctx per query and head) come out of the epilogue of the GEMM that
# produces dctx (NPM_EPI_ROWDOT) instead of a pass over dctx and ctx in front of the attention kernel (NPM_ATTN_ROWDOT=0: that pass)
ATTN_ROWDOT = os.environ.get('NPM_ATTN_ROWDOT', '1') != '0'
# decode steps: the projections and feed-forward products at M = B T <= SKINNY_MAX_M rows run on npm_sgemm_skinny (the weights
# streamed once over the whole chip) instead of the 128-row training tiles (NPM_SKINNY_GEMM=0: npm_sgemm as before).  The
# threshold is the largest M up to which the skinny kernel measured faster on all six decode shapes, warm and cold
# (tools/skinny_gemm_bench.py, profiles/r11_skinny_gemm_bench.log).
SKINNY_GEMM = os.environ.get('NPM_SKINNY_GEMM', '1') != '0'
SKINNY_MAX_M = 64
_SKINNY_LIB = (None, False)         # (library handle, whether it has the entry points)


def _skinny_entry_points(lib) -> bool:
    """Whether the loaded library handle has npm_sgemm_skinny (a host simulator of an earlier ABI does not)."""
    global _SKINNY_LIB
    if _SKINNY_LIB[0] is not lib:
        _SKINNY_LIB = (lib, hasattr(lib, 'npm_sgemm_skinny') and hasattr(lib, 'npm_sgemm_skinny_supported'))
    return _SKINNY_LIB[1]


_W16_LIB = (None, False)


def _w16_entry_points(lib) -> bool:
    """Whether the loaded library handle has npm_sgemm_skinny_w16 (an earlier library, or a host simulator of one, does not)."""
    global _W16_LIB
    if _W16_LIB[0] is not lib:
        _W16_LIB = (lib, hasattr(lib, 'npm_sgemm_skinny_w16') and hasattr(lib, 'npm_sgemm_skinny_w16_supported'))
    return _W16_LIB[1]


class KernelTimer:
    """Brackets every kernel-wrapper call with HIP events on the compute stream and books its
    ALGORITHMIC work (flops for GEMMs, bytes for the HBM-bound kernels; DESIGN.md has the
    per-unit figures).  bench.py uses it over the timed region for the roofline object."""

    def __init__(self):
        self.records = []          # (name, flops, bytes, start, stop)

    def __enter__(self):
        global _TIMER
        self._prev, _TIMER = _TIMER, self
        return self

    def __exit__(self, *exc):
        global _TIMER
        _TIMER = self._prev
        return False

    def summary(self):
        synchronize()
        out = {}
        for name, flops, nbytes, start, stop in self.records:
            rec = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            rec['launches'] += 1
            rec['ms'] += start.elapsed_ms(stop)
            rec['flops'] += flops
            rec['bytes'] += nbytes
        return out


_TIMER: Optional[KernelTimer] = None


class _timed:
    __slots__ = ('name', 'flops', 'bytes', 'start')

    def __init__(self, name: str, flops: float = 0.0, nbytes: float = 0.0):
        self.name, self.flops, self.bytes = name, flops, nbytes

    def __enter__(self):
        self.start = Event().record() if _TIMER is not None else None

    def __exit__(self, *exc):
        if self.start is not None and _TIMER is not None:
            _TIMER.records.append((self.name, self.flops, self.bytes, self.start, Event().record()))
        return False


class Mat:
    """Operand descriptor for :func:`gemm`: base pointer, row pitch, two batch strides.  ``half`` (a B operand only): a
    ``HalfView`` of the same matrix stored as IEEE fp16 with the same pitch, counted in halves (``HalfWeights.view``)."""

    __slots__ = ('ptr', 'ld', 's0', 's1', '_keep', 'half')

    def __init__(self, array_or_ptr, ld: int, s0: int = 0, s1: int = 0, half: Optional['HalfView'] = None):
        self._keep = array_or_ptr          # keeps a temporary alive until the launch is queued
        self.ptr = array_or_ptr.ptr if isinstance(array_or_ptr, DeviceArray) else int(array_or_ptr)
        self.ld, self.s0, self.s1 = int(ld), int(s0), int(s1)
        self.half = half


class HalfView:
    """Where the fp16 copy of one weight matrix starts inside a ``HalfWeights`` buffer (which it keeps alive)."""

    __slots__ = ('ptr', '_keep')

    def __init__(self, ptr: int, keep):
        self.ptr, self._keep = int(ptr), keep


class HalfWeights:
    """A SNAPSHOT of weight matrices as IEEE fp16, for the matrix products of decode steps (``gemm`` with ``Mat(..., half=)``;
    include/npm_hip.h npm_sgemm_skinny_w16): ``sources`` is a list of (layer, attribute); each parameter is converted once with
    ``npm_cvt_f32_f16`` (round to nearest even, no clamp) and read in place from then on.  Sources that are adjacent in device
    memory stay adjacent in ONE half buffer, in the same order and at the same element offsets -- so the packed q / k / v
    projection remains one product over one half matrix.

    The snapshot is of the weights AS THEY WERE.  It records each source's address and shape; ``view`` raises RuntimeError when
    either differs (a rebound parameter: a weight binder, a test, a re-packed arena).  A change of the VALUES in place -- an
    optimizer step -- cannot be seen: the halves then go on describing the earlier weights until ``refresh()`` converts again."""

    def __init__(self, sources):
        self._sources = [(owner, str(attribute)) for owner, attribute in sources]
        self._entries = {}             # (id(owner), attribute) -> (HalfView, source ptr, source shape)
        self.refresh()

    def refresh(self) -> 'HalfWeights':
        """Convert every source again, from where it lives now."""
        lib = _C.lib()
        if not hasattr(lib, 'npm_cvt_f32_f16'):
            raise _C.NpmError('half-precision weights need npm_cvt_f32_f16, which the loaded library does not have')
        params = [(owner, attribute, owner._param(attribute)) for owner, attribute in self._sources]
        self._entries = {}
        i = 0
        while i < len(params):
            j = i + 1                                       # params[i:j]: one run of sources adjacent in memory
            while j < len(params) and params[j][2].ptr == params[j - 1][2].ptr + params[j - 1][2].nbytes:
                j += 1
            total = sum(p.size for _, _, p in params[i:j])
            buf = HalfBuffer([total])
            first = params[i][2]
            cols = first.shape[-1] if all(p.shape[-1] == first.shape[-1] for _, _, p in params[i:j]) else total
            if total:
                with _timed('cvt_f32_f16', nbytes=6.0 * total):
                    _C.check(lib.npm_cvt_f32_f16(first.ptr, cols, buf.ptr, cols, total // cols, cols), 'npm_cvt_f32_f16')
            offset = 0
            for owner, attribute, p in params[i:j]:
                self._entries[id(owner), attribute] = (HalfView(buf.ptr + 2 * offset, buf), p.ptr, tuple(p.shape))
                offset += p.size
            i = j
        return self

    def __contains__(self, key) -> bool:
        owner, attribute = key
        return (id(owner), attribute) in self._entries

    def view(self, owner, attribute: str) -> HalfView:
        """The fp16 copy of ``owner``'s parameter ``attribute``; RuntimeError when the parameter is no longer the array the
        snapshot was taken of."""
        view, ptr, shape = self._entries[id(owner), attribute]
        now = owner._param(attribute)
        if now.ptr != ptr or tuple(now.shape) != shape:
            raise RuntimeError(f'HalfWeights: {type(owner).__name__}.{attribute} was rebound after the snapshot was taken (then '
                               f'{shape} at {ptr:#x}, now {tuple(now.shape)} at {now.ptr:#x}): refresh() it, or take a new one')
        return view

    def numpy(self, owner, attribute: str) -> np.ndarray:
        """The stored halves of one source, for tests."""
        view, _, shape = self._entries[id(owner), attribute]
        host = np.empty(shape, dtype=np.float16)
        if host.size:
            _C.check(_C.lib().npm_d2h(host.ctypes.data, view.ptr, host.nbytes), 'npm_d2h')
        return host


def gemm(m: int, n: int, k: int, a: Mat, b: Mat, c: Mat, *, trans_a: bool = False, trans_b: bool = False,
         batch: Tuple[int, int] = (1, 1), alpha: float = 1.0, bias: Optional[DeviceArray] = None,
         residual: Optional[Mat] = None, relu_save: Optional[Mat] = None, relu_mask: Optional[Mat] = None,
         split_k: int = 0, colsum_out: Optional[DeviceArray] = None,
         softmax_bwd: Optional[Tuple[Mat, DeviceArray]] = None,
         bsum_out: Optional[DeviceArray] = None, asum_out: Optional[DeviceArray] = None,
         rowdot: Optional[Tuple[Mat, DeviceArray, float]] = None,
         skinny_ok: bool = False, save_optional: bool = False) -> None:
    """C = epilogue(alpha * op(A) @ op(B)); see include/npm_hip.h ``npm_sgemm``.
    ``skinny_ok`` (the decode path sets it): the call may run on ``npm_sgemm_skinny`` when SKINNY_GEMM is on, m <= SKINNY_MAX_M,
    the math mode is f32, the loaded library has the entry point and ``npm_sgemm_skinny_supported`` takes the call; otherwise it
    is the ``npm_sgemm`` call it always was.  ``save_optional``: nobody reads ``relu_save``'s pre-activation (inference), so the
    skinny route applies the ReLU without storing it.
    ``b.half`` (un-batched, ``trans_a`` False): B is read from its fp16 copy.  Under the conditions above, with
    ``npm_sgemm_skinny_w16`` in the library and its predicate true, that is one ``npm_sgemm_skinny_w16`` launch over the halves in
    place.  EVERY other call converts the halves into pooled fp32 scratch (``npm_cvt_f16_f32``) and runs ``npm_sgemm`` on that,
    so the product is the one on the rounded weights at every m, math mode and switch setting -- never the fp32 weights.
    ``rowdot=(X, out, scale)``: besides C = A @ B, out[n // 128, m] (zeros on entry) += scale * sum over each block of 128
    columns of C * X -- the attention backward's row term dctx . ctx per head of size 128, taken where dctx is produced.
    ``colsum_out`` ([batch1, n]) receives the column sums of the stored C (a bias gradient
    taken in the producing GEMM's epilogue instead of a separate pass over C).
    ``softmax_bwd=(P, delta)``: C = alpha * P * (A @ B - delta[row]) -- the softmax backward with its
    row term precomputed (:func:`attn_rowdot`), fused into the GEMM that produces dP.
    ``bsum_out`` ([n]) receives the column sums of B ([k, n], not transposed): the bias gradient that goes
    with a weight gradient x^T @ dy, taken from the dy tiles that GEMM stages anyway; ``asum_out`` ([m]) the
    column sums of a transposed A ([k, m]) for products written dproj^T @ x."""
    g = _C.npm_gemm()
    g.trans_a, g.trans_b = int(trans_a), int(trans_b)
    g.m, g.n, g.k = int(m), int(n), int(k)
    g.batch0, g.batch1 = int(batch[0]), int(batch[1])
    g.a, g.lda, g.stride_a0, g.stride_a1 = a.ptr, a.ld, a.s0, a.s1
    g.b, g.ldb, g.stride_b0, g.stride_b1 = b.ptr, b.ld, b.s0, b.s1
    g.c, g.ldc, g.stride_c0, g.stride_c1 = c.ptr, c.ld, c.s0, c.s1
    g.alpha = float(alpha)
    epi = 0
    if bias is not None:
        epi |= _C.EPI_BIAS
        g.bias = bias.ptr
    if residual is not None:
        epi |= _C.EPI_RESIDUAL
        g.residual, g.ldr = residual.ptr, residual.ld
    if relu_save is not None:
        epi |= _C.EPI_RELU_SAVE
        g.aux, g.ldaux = relu_save.ptr, relu_save.ld
    if relu_mask is not None:
        epi |= _C.EPI_RELU_MASK
        g.aux, g.ldaux = relu_mask.ptr, relu_mask.ld
    if softmax_bwd is not None:
        epi |= _C.EPI_SOFTMAX_BWD
        g.aux, g.ldaux = softmax_bwd[0].ptr, softmax_bwd[0].ld
        g.rowvec = softmax_bwd[1].ptr
    if rowdot is not None:
        epi |= _C.EPI_ROWDOT
        g.aux, g.ldaux = rowdot[0].ptr, rowdot[0].ld
        g.rowdot, g.rowdot_scale = rowdot[1].ptr, float(rowdot[2])
    g.epilogue = epi
    g.split_k = int(split_k)
    fuse = colsum_out is not None and FUSE_COLSUM
    g.colsum = colsum_out.ptr if fuse else None
    fuse_b = bsum_out is not None and FUSE_BSUM
    g.bsum = bsum_out.ptr if fuse_b else None
    fuse_a = asum_out is not None and FUSE_BSUM
    g.asum = asum_out.ptr if fuse_a else None
    layout = 'TN' if trans_a else ('NT' if trans_b else 'NN')
    nb = batch[0] * batch[1]
    unique = 4.0 * nb * (m * k + k * n + m * n * (1 + (residual is not None) + (relu_save is not None) +
                                                  (relu_mask is not None) + (softmax_bwd is not None) + (rowdot is not None)))
    if b.half is not None:
        assert nb == 1 and not trans_a, 'a half operand is the B of an un-batched NN / NT product'
        assert colsum_out is None and bsum_out is None and asum_out is None, 'a half operand goes with no column-sum output'
        lib = _C.lib()
        if skinny_ok and SKINNY_GEMM and 0 < m <= SKINNY_MAX_M and _w16_entry_points(lib) and _C.current_math() == 'f32':
            gs = _C.npm_gemm.from_buffer_copy(g)
            gs.b = b.half.ptr
            if save_optional and epi & _C.EPI_RELU_SAVE:
                gs.epilogue, gs.aux, gs.ldaux = (epi & ~_C.EPI_RELU_SAVE) | _C.EPI_RELU, None, 0
            if lib.npm_sgemm_skinny_w16_supported(C.byref(gs)):
                with _timed('sgemm_skinny_w16_' + layout, flops=2.0 * m * n * k, nbytes=unique - 2.0 * k * n):
                    _C.check(lib.npm_sgemm_skinny_w16(C.byref(gs)), 'npm_sgemm_skinny_w16')
                return
        rows, cols = (n, k) if trans_b else (k, n)
        rounded = empty([rows, cols])                  # pooled; stream order keeps it alive until the product has read it
        with _timed('cvt_f16_f32', nbytes=6.0 * rows * cols):
            _C.check(lib.npm_cvt_f16_f32(b.half.ptr, b.ld, rounded.ptr, cols, rows, cols), 'npm_cvt_f16_f32')
        g.b, g.ldb = rounded.ptr, cols
        with _timed('sgemm_' + layout, flops=2.0 * m * n * k, nbytes=unique):
            _C.check(lib.npm_sgemm(C.byref(g)), 'npm_sgemm')
        return
    if skinny_ok and SKINNY_GEMM and 0 < m <= SKINNY_MAX_M:
        lib = _C.lib()
        if _skinny_entry_points(lib) and _C.current_math() == 'f32':
            gs = g
            if save_optional and epi & _C.EPI_RELU_SAVE:
                gs = _C.npm_gemm.from_buffer_copy(g)
                gs.epilogue, gs.aux, gs.ldaux = (epi & ~_C.EPI_RELU_SAVE) | _C.EPI_RELU, None, 0
            if lib.npm_sgemm_skinny_supported(C.byref(gs)):
                with _timed('sgemm_skinny_' + layout, flops=2.0 * m * n * k, nbytes=unique):
                    _C.check(lib.npm_sgemm_skinny(C.byref(gs)), 'npm_sgemm_skinny')
                return
    with _timed('sgemm_' + layout, flops=2.0 * m * n * k * nb, nbytes=unique):
        _C.check(_C.lib().npm_sgemm(C.byref(g)), 'npm_sgemm')
    if bsum_out is not None and not fuse_b:      # A/B switch: separate pass over B
        assert batch == (1, 1) and not trans_b
        with _timed('colsum', nbytes=4.0 * k * n):
            _C.check(_C.lib().npm_colsum(b.ptr, bsum_out.ptr, k, n, b.ld), 'npm_colsum')
    if asum_out is not None and not fuse_a:
        assert batch == (1, 1) and trans_a
        with _timed('colsum', nbytes=4.0 * k * m):
            _C.check(_C.lib().npm_colsum(a.ptr, asum_out.ptr, k, m, a.ld), 'npm_colsum')
    if colsum_out is not None and not fuse:      # A/B switch: separate pass over the stored C
        assert c.ld == n * batch[1] and (batch[1] == 1 or c.s1 == n), 'unfused colsum needs row-contiguous head slices'
        colsum(DeviceArray([1], c._keep._buf, c.ptr), m * batch[0], n * batch[1], out=colsum_out)


def colsum(x: DeviceArray, rows: int, cols: int, out: Optional[DeviceArray] = None) -> DeviceArray:
    out = empty([cols]) if out is None else out
    with _timed('colsum', nbytes=4.0 * rows * cols):
        _C.check(_C.lib().npm_colsum(x.ptr, out.ptr, rows, cols, cols), 'npm_colsum')
    return out


def add(a: DeviceArray, b: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
    out = empty(a.shape) if out is None else out
    with _timed('add', nbytes=12.0 * a.size):
        _C.check(_C.lib().npm_add(a.ptr, b.ptr, out.ptr, a.size), 'npm_add')
    return out


def add3(a: DeviceArray, b: DeviceArray, c: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
    out = empty(a.shape) if out is None else out
    with _timed('add3', nbytes=16.0 * a.size):
        _C.check(_C.lib().npm_add3(a.ptr, b.ptr, c.ptr, out.ptr, a.size), 'npm_add3')
    return out


def relu_fwd(x: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
    out = empty(x.shape) if out is None else out
    with _timed('relu_fwd', nbytes=8.0 * x.size):
        _C.check(_C.lib().npm_relu_fwd(x.ptr, out.ptr, x.size), 'npm_relu_fwd')
    return out


def relu_bwd(x_pre: DeviceArray, dy: DeviceArray, out: Optional[DeviceArray] = None) -> DeviceArray:
    out = empty(dy.shape) if out is None else out
    with _timed('relu_bwd', nbytes=12.0 * dy.size):
        _C.check(_C.lib().npm_relu_bwd(x_pre.ptr, dy.ptr, out.ptr, dy.size), 'npm_relu_bwd')
    return out


def relu_bwd_colsum(x_pre: DeviceArray, dy: DeviceArray, cols: int, colsum_out: DeviceArray) -> DeviceArray:
    """ReLU backward of a [rows, cols] matrix and the column sums of the result (the bias gradient of the
    layer in front of the ReLU) in one pass: conv.py:54-55, mlp.py:74 + mlp.py:34."""
    out = empty(dy.shape)
    rows = dy.size // cols
    assert rows * cols == dy.size and x_pre.size == dy.size and colsum_out.size == cols
    with _timed('relu_bwd_colsum', nbytes=12.0 * dy.size):
        _C.check(_C.lib().npm_relu_bwd_colsum(x_pre.ptr, dy.ptr, out.ptr, colsum_out.ptr, rows, cols),
                 'npm_relu_bwd_colsum')
    return out


def softmax_fwd(x: DeviceArray, scale: float = 1.0, out: Optional[DeviceArray] = None) -> DeviceArray:
    n = x.shape[-1] if x.ndim else 1
    rows = x.size // n if n else 0
    out = empty(x.shape) if out is None else out
    with _timed('softmax_fwd', nbytes=8.0 * x.size):
        _C.check(_C.lib().npm_softmax_fwd(x.ptr, out.ptr, rows, n, float(scale)), 'npm_softmax_fwd')
    return out


def softmax_bwd(y: DeviceArray, dy: DeviceArray, scale: float = 1.0, out: Optional[DeviceArray] = None) -> DeviceArray:
    n = y.shape[-1] if y.ndim else 1
    rows = y.size // n if n else 0
    out = empty(y.shape) if out is None else out
    with _timed('softmax_bwd', nbytes=12.0 * y.size):
        _C.check(_C.lib().npm_softmax_bwd(y.ptr, dy.ptr, out.ptr, rows, n, float(scale)), 'npm_softmax_bwd')
    return out


def attn_rowdot(a: DeviceArray, b: DeviceArray) -> DeviceArray:
    """out[b, h, s] = sum_d a[b, s, h, d] * b[b, s, h, d]  (inputs [B, S, H, D])."""
    bsz, seq, heads, dim = a.shape
    out = empty([bsz, heads, seq])
    with _timed('attn_rowdot', nbytes=8.0 * a.size):
        _C.check(_C.lib().npm_attn_rowdot(a.ptr, b.ptr, out.ptr, bsz, seq, heads, dim), 'npm_attn_rowdot')
    return out


def layernorm_dropout_supported(d: int) -> bool:
    """Row lengths npm_layernorm_dropout_fwd / _bwd take (include/npm_hip.h): the row-in-registers kernels."""
    return d % 4 == 0 and d <= 4096


def layernorm_fwd(x: DeviceArray, gamma: DeviceArray, beta: DeviceArray, eps: float, drop=None):
    """Returns (z, mean, rstd); mean/rstd have x's shape with the last axis reduced to 1.  ``drop = (mask bytes, keep_prob)``:
    the row is DropOut's output, formed on the way in (the dropped tensor is never stored)."""
    d = x.shape[-1]
    rows = x.size // d
    stat_shape = tuple(x.shape[:-1]) + (1,)
    z, mean, rstd = empty(x.shape), empty(stat_shape), empty(stat_shape)
    if drop is not None:
        with _timed('layernorm_fwd', nbytes=9.0 * x.size + 8.0 * rows):
            _C.check(_C.lib().npm_layernorm_dropout_fwd(x.ptr, drop[0].ptr, float(drop[1]), gamma.ptr, beta.ptr, float(eps), rows, d,
                                                        z.ptr, mean.ptr, rstd.ptr), 'npm_layernorm_dropout_fwd')
        return z, mean, rstd
    with _timed('layernorm_fwd', nbytes=8.0 * x.size + 8.0 * rows):
        _C.check(_C.lib().npm_layernorm_fwd(x.ptr, gamma.ptr, beta.ptr, float(eps), rows, d,
                                            z.ptr, mean.ptr, rstd.ptr), 'npm_layernorm_fwd')
    return z, mean, rstd


def layernorm_bwd(dz: DeviceArray, x: DeviceArray, mean: DeviceArray, rstd: DeviceArray, gamma: DeviceArray,
                  dgamma: DeviceArray, dbeta: DeviceArray, residual: Optional[DeviceArray] = None, drop=None) -> DeviceArray:
    """``drop = (mask bytes, keep_prob)``: ``x`` is the input of the DropOut in front of the norm; the result is the gradient
    with respect to THAT (DropOut.backward applied on the way out, before the residual)."""
    d = x.shape[-1]
    rows = x.size // d
    dx = empty(dz.shape)
    res = None if residual is None else residual.ptr
    if drop is not None:
        with _timed('layernorm_bwd', nbytes=(17.0 if residual is not None else 13.0) * x.size + 8.0 * rows):
            _C.check(_C.lib().npm_layernorm_dropout_bwd(dz.ptr, x.ptr, drop[0].ptr, float(drop[1]), mean.ptr, rstd.ptr, gamma.ptr,
                                                        res, rows, d, dx.ptr, dgamma.ptr, dbeta.ptr), 'npm_layernorm_dropout_bwd')
        return dx
    with _timed('layernorm_bwd', nbytes=(16.0 if residual is not None else 12.0) * x.size + 8.0 * rows):
        _C.check(_C.lib().npm_layernorm_bwd(dz.ptr, x.ptr, mean.ptr, rstd.ptr, gamma.ptr, res, rows, d,
                                            dx.ptr, dgamma.ptr, dbeta.ptr), 'npm_layernorm_bwd')
    return dx


def _entry_point(name: str):
    """``name`` of the loaded library; NpmError naming it when the library is older than the entry point."""
    fn = getattr(_C.lib(), name, None)
    if fn is None:
        raise _C.NpmError(f'this operation needs {name}, which the loaded library does not have')
    return fn


def rmsnorm_fwd(x: DeviceArray, gamma: DeviceArray, eps: float):
    """Returns (z, rstd) with z = gamma * x * rstd, rstd = 1 / sqrt(mean(x^2) + eps) of x's shape with the last axis reduced to 1."""
    fn = _entry_point('npm_rmsnorm_fwd')
    d = x.shape[-1]
    rows = x.size // d
    z, rstd = empty(x.shape), empty(tuple(x.shape[:-1]) + (1,))
    with _timed('rmsnorm_fwd', nbytes=8.0 * x.size + 4.0 * rows):
        _C.check(fn(x.ptr, gamma.ptr, float(eps), rows, d, z.ptr, rstd.ptr), 'npm_rmsnorm_fwd')
    return z, rstd


def rmsnorm_bwd(dz: DeviceArray, x: DeviceArray, rstd: DeviceArray, gamma: DeviceArray, dgamma: DeviceArray,
                residual: Optional[DeviceArray] = None) -> DeviceArray:
    """dx (+ residual); dgamma is written."""
    fn = _entry_point('npm_rmsnorm_bwd')
    d = x.shape[-1]
    rows = x.size // d
    dx = empty(dz.shape)
    with _timed('rmsnorm_bwd', nbytes=(16.0 if residual is not None else 12.0) * x.size + 4.0 * rows):
        _C.check(fn(dz.ptr, x.ptr, rstd.ptr, gamma.ptr, None if residual is None else residual.ptr, rows, d, dx.ptr, dgamma.ptr),
                 'npm_rmsnorm_bwd')
    return dx


def swiglu_fwd(pre: DeviceArray) -> DeviceArray:
    """pre [..., 2 U] = gate | up  ->  h [..., U] = silu(gate) * up."""
    fn = _entry_point('npm_swiglu_fwd')
    units = pre.shape[-1] // 2
    assert 2 * units == pre.shape[-1], pre.shape
    rows = pre.size // (2 * units) if units else 0
    h = empty(tuple(pre.shape[:-1]) + (units,))
    with _timed('swiglu_fwd', nbytes=12.0 * rows * units):
        _C.check(fn(pre.ptr, 2 * units, rows, units, h.ptr, units), 'npm_swiglu_fwd')
    return h


def swiglu_bwd(pre: DeviceArray, dh: DeviceArray) -> DeviceArray:
    """dpre [..., 2 U] = dgate | dup from pre and the gradient of ``swiglu_fwd``'s result."""
    fn = _entry_point('npm_swiglu_bwd')
    units = pre.shape[-1] // 2
    rows = pre.size // (2 * units) if units else 0
    assert dh.size == rows * units, f'{dh.shape} vs {pre.shape}'
    dpre = empty(pre.shape)
    with _timed('swiglu_bwd', nbytes=20.0 * rows * units):
        _C.check(fn(pre.ptr, 2 * units, dh.ptr, units, rows, units, dpre.ptr, 2 * units), 'npm_swiglu_bwd')
    return dpre


# ---- fused attention core ----------------------------------------------------------------------------
def mha_core_supported(head_dim: int, value_dim: Optional[int] = None, *, any_math: bool = False) -> bool:
    """Whether the fused attention kernels take this head size.  They run the exact-fp32 MFMA only, so under a
    split-bf16 math mode the layers keep composing attention from ``gemm`` (which honours the mode) unless
    ``any_math`` is set (masked attention exists only in the fused kernels)."""
    if not ATTN_CORE or (value_dim is not None and value_dim != head_dim):
        return False
    if not any_math and _C.current_math() != 'f32':
        return False
    return bool(_C.lib().npm_mha_core_supported(int(head_dim)))


class AttnMask:
    """A boolean attention mask on the device: bytes plus (batch, head, query) strides; broadcast axes have
    stride 0.  ``np.where(mask, scaled, -inf)`` of reference layers/attentions.py:105-107."""

    def __init__(self, mask, b: int, h: int, sq: int, skv: int):
        self.dims = (int(b), int(h), int(sq), int(skv))
        host = np.asarray(mask).astype(bool)
        while host.ndim < 4:
            host = host[None]
        if host.ndim != 4 or any(have not in (1, want) for have, want in zip(host.shape, (b, h, sq, skv))):
            raise AssertionError(f'mask shape {np.shape(mask)} does not broadcast to {(b, h, sq, skv)}')
        if host.shape[3] != skv:
            host = np.broadcast_to(host, host.shape[:3] + (skv,))
        host = np.ascontiguousarray(host).astype(np.uint8)
        self.host = host.astype(bool)
        self.buf = bytes_from_host(host)
        nb, nh, nq, _ = host.shape
        self.strides = (0 if nb == 1 else nh * nq * skv, 0 if nh == 1 else nq * skv, 0 if nq == 1 else skv)
        # Tile summary (include/npm_hip.h npm_mha_mask_summary): one byte per (32 queries, 128 keys) and distinct mask plane,
        # made on the device from the bytes just uploaded; the fused kernels skip the tiles it marks empty.
        self.summary, self.summary_strides = None, (0, 0)
        if ATTN_TILE_SKIP and sq > 0:
            nqt, nkb = (sq + 31) // 32, (skv + 127) // 128
            self.summary_all_offset = nb * nh * nqt * nkb          # "every position allowed" bytes: the second half
            self.summary = ByteBuffer(2 * self.summary_all_offset)
            _C.check(_C.lib().npm_mha_mask_summary(self.buf.ptr, self.strides[0], self.strides[1], self.strides[2], nb, nh, sq, skv,
                                                   self.summary.ptr), 'npm_mha_mask_summary')
            self.summary_strides = (0 if nb == 1 else nh * nqt * nkb, 0 if nh == 1 else nqt * nkb)

    def full(self, b, h, sq, skv) -> np.ndarray:
        return np.broadcast_to(self.host, (b, h, sq, skv))


def _core_desc(q: Mat, k: Mat, v: Mat, ctx: Mat, lse: DeviceArray, dims, scale: float,
               mask: Optional[AttnMask], scores: Optional[DeviceArray]):
    b, h, sq, skv, d = (int(x) for x in dims)
    c = _C.npm_mha_core()
    c.batch, c.heads, c.seq_q, c.seq_kv, c.head_dim = b, h, sq, skv, d
    c.scale = float(scale)
    c.q, c.q_pitch, c.k, c.k_pitch, c.v, c.v_pitch = q.ptr, q.ld, k.ptr, k.ld, v.ptr, v.ld
    c.ctx, c.ctx_pitch, c.lse = ctx.ptr, ctx.ld, lse.ptr
    if mask is not None:
        c.mask = mask.buf.ptr
        c.mask_stride_b, c.mask_stride_h, c.mask_stride_q = mask.strides
        if mask.summary is not None:
            c.tile_summary = mask.summary.ptr
            c.summary_stride_b, c.summary_stride_h = mask.summary_strides
            c.summary_all_offset = mask.summary_all_offset
    if scores is not None:
        c.scores = scores.ptr
    return c


def mha_core_fwd(q: Mat, k: Mat, v: Mat, dims, scale: float, mask: Optional[AttnMask] = None,
                 save_scores: bool = False, kv_heads: Optional[int] = None):
    """ctx[b, i, h, :] = softmax_j(scale q_i . k_j [masked]) v_j in one kernel (include/npm_hip.h npm_mha_core_fwd).
    ``q``/``k``/``v``: (array, row pitch) of [B, S, H, D] operands.  Returns (ctx [B, Sq, H, D], lse [B, H, Sq],
    scores or None).  ``kv_heads`` (grouped-query attention, npm_mha_core_fwd_grouped): k / v are [B, Skv, kv_heads, D] and
    query head h reads K / V head h % kv_heads; None is the ungrouped call."""
    b, h, sq, skv, d = dims
    hkv = h if kv_heads is None else int(kv_heads)
    ctx, lse = empty([b, sq, h, d]), empty([b, h, sq])
    scores = empty([b, h, sq, skv]) if save_scores else None
    c = _core_desc(q, k, v, Mat(ctx, h * d), lse, dims, scale, mask, scores)
    nbytes = 4.0 * b * d * (2 * h * sq + 2 * hkv * skv) + (4.0 * b * h * sq * skv if save_scores else 0.0)
    with _timed('mha_core_fwd', flops=4.0 * b * h * sq * skv * d, nbytes=nbytes):
        if kv_heads is None:
            _C.check(_C.lib().npm_mha_core_fwd(C.byref(c)), 'npm_mha_core_fwd')
        else:
            _C.check(_C.lib().npm_mha_core_fwd_grouped(C.byref(c), hkv), 'npm_mha_core_fwd_grouped')
    return ctx, lse, scores


def mha_core_bwd(q: Mat, k: Mat, v: Mat, ctx: DeviceArray, lse: DeviceArray, dctx: DeviceArray,
                 dq: Mat, dk: Mat, dv: Mat, dims, scale: float, mask: Optional[AttnMask] = None,
                 scores: Optional[DeviceArray] = None, neg_delta: Optional[Tuple[DeviceArray, int, int]] = None,
                 kv_heads: Optional[int] = None) -> None:
    """dq, dk, dv of the attention core from q, k, v, the forward's ctx and lse, and dctx (npm_mha_core_bwd).
    Algorithmic work: the four products dP, dV, dK, dQ (the recomputed q.k is the kernel's own business).
    ``neg_delta=(array, stride_b, stride_h)``: the row terms -scale * (dctx . ctx) already taken by the GEMM that produced dctx.
    ``kv_heads``: grouped-query attention (npm_mha_core_bwd_grouped), k / v / dk / dv with kv_heads heads."""
    b, h, sq, skv, d = dims
    hkv = h if kv_heads is None else int(kv_heads)
    c = _core_desc(q, k, v, Mat(ctx, h * d), lse, dims, scale, mask, scores)
    c.dctx, c.dctx_pitch = dctx.ptr, h * d
    c.dq, c.dq_pitch, c.dk, c.dk_pitch, c.dv, c.dv_pitch = dq.ptr, dq.ld, dk.ptr, dk.ld, dv.ptr, dv.ld
    if neg_delta is not None:
        c.neg_delta, c.neg_delta_stride_b, c.neg_delta_stride_h = neg_delta[0].ptr, int(neg_delta[1]), int(neg_delta[2])
    nbytes = 4.0 * b * d * (4 * h * sq + 4 * hkv * skv) + (4.0 * b * h * sq * skv if scores is not None else 0.0)
    with _timed('mha_core_bwd', flops=8.0 * b * h * sq * skv * d, nbytes=nbytes):
        if kv_heads is None:
            _C.check(_C.lib().npm_mha_core_bwd(C.byref(c)), 'npm_mha_core_bwd')
        else:
            _C.check(_C.lib().npm_mha_core_bwd_grouped(C.byref(c), hkv), 'npm_mha_core_bwd_grouped')


# ---- incremental decoding: key / value cache ----------------------------------------------------------------------------
def mha_decode_supported(head_dim: int, group_rows: int, value_dim: Optional[int] = None) -> bool:
    """Whether ``npm_mha_decode_fwd`` takes this head size with ``group_rows`` = (Hq / Hkv) * T score rows per K / V head.  The
    kernel runs the exact-fp32 MFMA only, so under a split math mode the layers fall back to compositions that honour it."""
    if not ATTN_CORE or (value_dim is not None and value_dim != head_dim) or _C.current_math() != 'f32':
        return False
    return bool(_C.lib().npm_mha_decode_supported(int(head_dim), int(group_rows)))


class KVLayout(NamedTuple):
    """Where the rows of one cache tensor live, as the entry points of include/npm_hip.h take it.  Contiguous: row j of sequence b
    is ``pitch`` floats long at ``b * stride + j * pitch``.  Paged (``table``: the DEVICE address of the block table, int32
    [B, table_pitch]): ``stride`` is that of a page and the row is row ``j % page_rows`` of page ``table[b, j // page_rows]``.
    ``dtype`` 'f16': the tensor holds halves (``pitch`` and ``stride`` count elements either way) and the calls are the ``_f16``
    entry points."""
    pitch: int
    stride: int
    table: Optional[int] = None
    table_pitch: int = 0
    page_rows: int = 0
    dtype: str = 'f32'


KV_ITEMSIZE = {'f32': 4, 'f16': 2}            # the storage types of a KVCache and their bytes per element


def _kv_dtype(dtype, kv_heads: int, key_dim: int, value_dim: int) -> str:
    if dtype not in KV_ITEMSIZE:
        raise ValueError(f"KVCache: dtype must be one of {sorted(KV_ITEMSIZE)}, got {dtype!r}")
    if dtype == 'f16' and (kv_heads * key_dim % 8 or kv_heads * value_dim % 8):
        raise ValueError(f'KVCache: an f16 cache moves 8 halves at a time: rows of {kv_heads * key_dim} / {kv_heads * value_dim} '
                         'elements are not multiples of 8')
    return dtype


def _kv_window(window, key_dim: int, value_dim: int) -> Optional[int]:
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f'KVCache: window must be None or an integer >= 1, got {window!r}')
    if key_dim != value_dim:
        raise ValueError(f'KVCache: a windowed cache is read by the decode and prefill kernels only: head sizes {key_dim} / {value_dim} differ')
    return int(window)


def kv_append(src: Mat, dst: int, layout: KVLayout, batch: int, tokens: int, at: int, lens, rows: int) -> None:
    """Row ``at + t`` of sequence b of the cache tensor at address ``dst`` = src[b * tokens + t]; ``src``: (array, row pitch) of
    [B, T, Hkv * D] rows, e.g. the K part of a packed projection (include/npm_hip.h npm_kv_append).  ``lens`` = (at_lens,
    new_lens), device addresses of [B] int32: sequence b starts at at_lens[b] and takes only t < new_lens[b]
    (npm_kv_append_varlen; through the block table of a paged ``layout`` npm_kv_append_paged, which always has ``lens``).  The
    caller has checked that the rows fit; ``rows``: the rows written, for the timer."""
    row = layout.pitch
    if layout.dtype == 'f16':
        at_lens, new_lens = (None, None) if lens is None else lens
        with _timed('kv_append', nbytes=6.0 * rows * row):
            _C.check(_C.lib().npm_kv_append_f16(src.ptr, src.ld, dst, row, layout.stride, batch, tokens, row, at, at_lens, new_lens,
                                                layout.table, layout.table_pitch, layout.page_rows), 'npm_kv_append_f16')
        return
    with _timed('kv_append', nbytes=8.0 * rows * row):
        if layout.table is not None:
            _C.check(_C.lib().npm_kv_append_paged(src.ptr, src.ld, dst, row, layout.stride, batch, tokens, row, lens[0], lens[1],
                                                  layout.table, layout.table_pitch, layout.page_rows), 'npm_kv_append_paged')
        elif lens is not None:
            _C.check(_C.lib().npm_kv_append_varlen(src.ptr, src.ld, dst, row, layout.stride, batch, tokens, row, lens[0], lens[1]),
                     'npm_kv_append_varlen')
        else:
            _C.check(_C.lib().npm_kv_append(src.ptr, src.ld, dst, row, layout.stride, batch, tokens, row, at), 'npm_kv_append')


def kv_gather_rows(src: int, layout: KVLayout, out: DeviceArray, lens: int) -> None:
    """out[b, j] = row j of sequence b of the cache tensor at ``src`` for j < lens[b], zeros behind, for ``out`` [B, rows, Hkv, D]
    (include/npm_hip.h npm_kv_gather_varlen, or npm_kv_gather_paged for a paged ``layout``; one launch).  ``lens``: device address
    of [B] int32."""
    b, rows, row = out.shape[0], out.shape[1], layout.pitch
    assert out.size == b * rows * row
    if layout.dtype == 'f16':
        with _timed('kv_gather', nbytes=6.0 * b * rows * row):
            _C.check(_C.lib().npm_kv_gather_f16(src, row, layout.stride, out.ptr, b, rows, row, lens, layout.table, layout.table_pitch,
                                                layout.page_rows), 'npm_kv_gather_f16')
        return
    with _timed('kv_gather', nbytes=8.0 * b * rows * row):
        if layout.table is not None:
            _C.check(_C.lib().npm_kv_gather_paged(src, row, layout.stride, out.ptr, b, rows, row, lens, layout.table, layout.table_pitch,
                                                  layout.page_rows), 'npm_kv_gather_paged')
        else:
            _C.check(_C.lib().npm_kv_gather_varlen(src, row, layout.stride, out.ptr, b, rows, row, lens), 'npm_kv_gather_varlen')


def kv_gather(cache: DeviceArray, out: DeviceArray, length: int) -> None:
    """out[b, :length] = cache[b, :length] for a cache [B, capacity, Hkv, D] and ``out`` [B, length, Hkv, D]: the valid rows made
    contiguous for a kernel that addresses K / V without a batch stride (one device copy per sequence; a fallback path)."""
    b, capacity, hkv, d = cache.shape
    assert out.shape == (b, length, hkv, d) and length <= capacity
    for i in range(b):
        _C.check(_C.lib().npm_d2d(out.ptr + 4 * i * length * hkv * d, cache.ptr + 4 * i * capacity * hkv * d, 4 * length * hkv * d),
                 'npm_d2d')


def _decode_desc(q: Mat, cache: 'KVCache', heads: int, tokens: int, kv_len: int, scale: float, causal: bool, want_lse: bool,
                 out: bool = True):
    """The ``npm_mha_decode`` of ``tokens`` query rows per sequence over ``cache`` -- the only place that fills one -- with fresh
    ctx [B, T, Hq, D] and lse [B, Hq, T] (or None), and the layout of ``cache.k`` (its table is that of ``cache.v`` too).
    ``out`` False: ctx and lse are left out (a call that writes elsewhere: ``mha_prefix``)."""
    b, hkv, d = cache.batch, cache.kv_heads, cache.key_dim
    kl, vl = cache.layout(cache.k), cache.layout(cache.v)
    ctx = empty([b, tokens, heads, d]) if out else None
    lse = empty([b, heads, tokens]) if out and want_lse else None
    c = _C.npm_mha_decode()
    c.batch, c.heads, c.kv_heads, c.new_tokens, c.kv_len, c.head_dim = b, int(heads), hkv, int(tokens), int(kv_len), d
    c.causal, c.scale = int(bool(causal)), float(scale)
    c.q, c.q_pitch = q.ptr, q.ld
    c.k, c.k_pitch, c.k_stride_b = cache.k.ptr, kl.pitch, kl.stride
    c.v, c.v_pitch, c.v_stride_b = cache.v.ptr, vl.pitch, vl.stride
    if out:
        c.ctx, c.ctx_pitch = ctx.ptr, heads * d
        c.lse = None if lse is None else lse.ptr
    return c, ctx, lse, kl


def _behind_prefix(layout: KVLayout, prefix: int) -> KVLayout:
    """``layout`` of a paged cache with every table row starting ``prefix`` rows (whole pages) later; the pitch stays."""
    if not prefix:
        return layout
    assert layout.table is not None and prefix % layout.page_rows == 0, (prefix, layout.page_rows)
    return layout._replace(table=layout.table + 4 * (prefix // layout.page_rows))


def _attend_entry(kernel: str, cache: 'KVCache', layout: KVLayout, lens, window: Optional[int]):
    """The entry point that runs ``kernel`` ('decode' | 'prefill') over ``cache`` and its arguments behind the descriptor, by

    ==========  ======  =================  =============================  ================================================
    window      dtype   layout             entry point                    arguments
    ==========  ======  =================  =============================  ================================================
    W           any     per-sequence       npm_mha_<kernel>_fwd_window    kv_lens, new_lens, table, W, dtype == 'f16'
    None        f16     any                npm_mha_<kernel>_fwd_f16       kv_lens, new_lens, table
    None        f32     any (prefill)      npm_mha_prefill_fwd            kv_lens, new_lens, table
    None        f32     paged (decode)     npm_mha_decode_fwd_paged       kv_lens, new_lens, table
    None        f32     ragged (decode)    npm_mha_decode_fwd_varlen      kv_lens, new_lens
    None        f32     uniform (decode)   npm_mha_decode_fwd             --
    ==========  ======  =================  =============================  ================================================

    ``table``: (block table, its pitch, rows per page), NULL and zeros for a contiguous cache; the lengths are NULL in the
    uniform call."""
    kv_lens, new_lens = (None, None) if lens is None else lens
    table = (layout.table, layout.table_pitch, layout.page_rows)
    if window is not None:
        if lens is None:
            raise ValueError(f'npm_mha_{kernel}_fwd_window: a window needs the per-sequence lengths')
        return f'npm_mha_{kernel}_fwd_window', (kv_lens, new_lens, *table, int(window), int(cache.dtype == 'f16'))
    if cache.dtype == 'f16':
        return f'npm_mha_{kernel}_fwd_f16', (kv_lens, new_lens, *table)
    if kernel == 'prefill':
        return 'npm_mha_prefill_fwd', (kv_lens, new_lens, *table)
    if layout.table is not None:
        return 'npm_mha_decode_fwd_paged', (kv_lens, new_lens, *table)
    return ('npm_mha_decode_fwd_varlen', (kv_lens, new_lens)) if lens is not None else ('npm_mha_decode_fwd', ())


def _mha_cached(kernel: str, q: Mat, cache: 'KVCache', heads: int, tokens: int, kv_len: int, scale: float, causal: bool, want_lse: bool,
                lens, keys: Optional[int], window: Optional[int], prefix: int):
    """``mha_decode`` / ``mha_prefill`` (``kernel``): one descriptor, one entry point out of ``_attend_entry``, one timer."""
    assert cache.key_dim == cache.value_dim and 0 <= kv_len <= cache.capacity and (lens is not None or tokens <= kv_len)
    c, ctx, lse, layout = _decode_desc(q, cache, heads, tokens, kv_len, scale, causal, want_lse)
    entry, args = _attend_entry(kernel, cache, _behind_prefix(layout, prefix), lens, window)
    b, hkv, d = cache.batch, cache.kv_heads, cache.key_dim
    keys = b * kv_len if keys is None else int(keys)
    if window is not None:
        keys = min(keys, b * (int(window) + tokens - 1))                 # the keys a windowed call reads at most
    # q and ctx in fp32, K and V once in the cache's type
    with _timed('mha_' + kernel, flops=4.0 * heads * tokens * keys * d, nbytes=4.0 * d * (2 * b * heads * tokens) + 2.0 * cache.itemsize * d * hkv * keys):
        _C.check(getattr(_C.lib(), entry)(C.byref(c), *args), entry)
    return ctx, lse


def mha_decode(q: Mat, cache: 'KVCache', heads: int, tokens: int, kv_len: int, scale: float, causal: bool, want_lse: bool = False,
               lens=None, keys: Optional[int] = None, window: Optional[int] = None, prefix: int = 0):
    """ctx [B, T, Hq, D] (and lse [B, Hq, T] or None) of ``tokens`` query rows per sequence over the first ``kv_len`` rows of
    ``cache`` (include/npm_hip.h npm_mha_decode_fwd).  ``q``: (array, row pitch).

    ``lens`` = (kv_lens, new_lens), DEVICE addresses of [B] int32 -- valid rows with the new tokens included; new tokens of the
    padded ``tokens``, or None for all -- makes it the call of a ragged batch (npm_mha_decode_fwd_varlen; through the block table
    of a paged cache npm_mha_decode_fwd_paged, bitwise the same on the same rows): ``kv_len`` is then the host's upper bound of
    ``kv_lens`` and rows without a visible key come back as ctx 0, lse -inf.  ``keys``: the sum of the lengths, for the timer.
    ``window`` W: row t sees only the W keys up to its own (npm_mha_decode_fwd_window; per-sequence form, causal).
    ``prefix`` P (a paged cache, whole pages): the call runs over the rows BEHIND the first P of every sequence -- the table moved
    on by P / page_size slots, ``kv_len`` and ``lens`` already in those coordinates (``PagedKVCache`` 's shared-prefix path)."""
    return _mha_cached('decode', q, cache, heads, tokens, kv_len, scale, causal, want_lse, lens, keys, window, prefix)


# prefill: cached forwards with more rows than the decode kernel takes (a prompt chunk on top of cached rows, a ragged or paged
# prefill, a sequence admitted into a running batch, a long query over a frozen cross cache) run npm_mha_prefill_fwd straight
# over the cache instead of the fused training forward on gathered K / V with a host-built mask.  Off by default: the gather /
# mask path stays what every call sequence is until the switch is flipped (measured: tools/prefill_bench.py).
PREFILL_KERNEL = os.environ.get('NPM_PREFILL_KERNEL', '0') != '0'
# The same switch for half-precision caches, independent of the one above: whatever the decode kernel does not take runs
# npm_mha_prefill_fwd_f16 over the stored halves in place instead of the fused training forward on gathered fp32 copies.  Off by
# default: every call sequence is then what it was before the entry point existed (measured: tools/prefill_kv16_bench.py).
PREFILL_KERNEL_F16 = os.environ.get('NPM_PREFILL_KERNEL_F16', '0') != '0'


def mha_prefill_supported(head_dim: int, value_dim: Optional[int] = None) -> bool:
    """Whether ``npm_mha_prefill_fwd`` / ``npm_mha_prefill_fwd_f16`` take this head size (any number of rows).  Exact-fp32 MFMA only, like
    ``mha_decode_supported``: false under a split math mode."""
    if not ATTN_CORE or (value_dim is not None and value_dim != head_dim) or _C.current_math() != 'f32':
        return False
    return bool(_C.lib().npm_mha_prefill_supported(int(head_dim)))


def mha_prefill(q: Mat, cache: 'KVCache', heads: int, tokens: int, kv_len: int, scale: float, causal: bool, want_lse: bool = False,
                lens=None, keys: Optional[int] = None, window: Optional[int] = None, prefix: int = 0):
    """``mha_decode`` without its limit on the rows (include/npm_hip.h npm_mha_prefill_fwd): ctx [B, T, Hq, D] (and lse
    [B, Hq, T] or None) of ``tokens`` query rows per sequence over ``cache``, read in place -- through the block table of a paged
    cache -- with ``lens`` = (kv_lens, new_lens) as there.  No mask and no gathered copy exist.  An fp16 cache takes
    ``npm_mha_prefill_fwd_f16`` (bitwise the fp32 call on the rounded values); this is the low-level call, whatever
    ``PREFILL_KERNEL_F16`` says.  ``window`` W: npm_mha_prefill_fwd_window, as in ``mha_decode``; ``prefix``: as there."""
    return _mha_cached('prefill', q, cache, heads, tokens, kv_len, scale, causal, want_lse, lens, keys, window, prefix)


# shared prefixes: with the switch on, a causal ``attend`` on a paged cache whose active sequences name the same leading pages
# (``PagedKVCache.fork``) reads those pages once for all of them -- npm_mha_prefix_fwd, the ordinary paged call over what lies
# behind them, npm_attn_combine -- from ``SHARED_PREFIX_MIN_ROWS`` shared rows up.  Off by default: every call sequence is then
# what it was before the entry points existed (tools/shared_prefix_bench.py measures both sides).
SHARED_PREFIX = os.environ.get('NPM_SHARED_PREFIX', '0') != '0'
# Measured (tools/shared_prefix_bench.py, profiles/r19_shared_prefix_bench.log; D 128, Hq 8, page 64): at B 8 and Hkv 8 the three
# launches are not slower than the paged call from P 8192 up (0.96 - 1.12 of it; 1.26 - 1.56 at P 2048), which is the default;
# at B 64 they win from P 512 (0.85 - 1.05) to P 8192 (0.19 - 0.31).  At Hkv 1 they LOSE at every measured shape but B 64, P 8192,
# T 4 and f16: leave the switch off for multi-query attention.
SHARED_PREFIX_MIN_ROWS = int(os.environ.get('NPM_SHARED_PREFIX_MIN_ROWS', '8192'))


def mha_prefix_supported(head_dim: int, value_dim: Optional[int] = None) -> bool:
    """Whether ``npm_mha_prefix_fwd`` takes this head size.  Exact-fp32 MFMA only, like ``mha_decode_supported``."""
    if not ATTN_CORE or (value_dim is not None and value_dim != head_dim) or _C.current_math() != 'f32':
        return False
    return bool(_C.lib().npm_mha_prefix_supported(int(head_dim)))


def mha_prefix(q: Mat, cache: 'PagedKVCache', heads: int, tokens: int, scale: float, new_lens: Optional[int], prefix_table: int,
               prefix: int):
    """The partial results of all ``cache.batch * tokens`` query rows over the ``prefix`` rows whose pages the device table row at
    ``prefix_table`` names (include/npm_hip.h npm_mha_prefix_fwd): (splits, part_ctx address, part_lse address, the pooled
    scratch that holds both -- keep it until the combine is launched)."""
    c, _, _, _ = _decode_desc(q, cache, heads, tokens, prefix, scale, False, False, out=False)
    b, hkv, d = cache.batch, cache.kv_heads, cache.key_dim
    rows = b * int(tokens)
    splits = int(_C.lib().npm_mha_prefix_splits(rows, int(heads), hkv, int(prefix)))
    part = empty([splits * rows * heads * (d + 1)])
    part_lse = part.ptr + 4 * splits * rows * heads * d
    row_tiles = -(-rows * heads // (hkv * 64))
    with _timed('mha_prefix', flops=4.0 * heads * rows * prefix * d,
                nbytes=4.0 * d * heads * rows * (1 + splits) + 2.0 * cache.itemsize * d * hkv * prefix * row_tiles):
        _C.check(_C.lib().npm_mha_prefix_fwd(C.byref(c), new_lens, prefix_table, cache.page_size, int(prefix), splits, part.ptr, part_lse,
                                             int(cache.dtype == 'f16')), 'npm_mha_prefix_fwd')
    return splits, part.ptr, part_lse, part


def attn_combine(part_ctx: int, part_lse: int, splits: int, ctx: DeviceArray, lse: DeviceArray, new_lens: Optional[int],
                 store_lse: bool) -> None:
    """``ctx`` [B, T, Hq, D] and ``lse`` [B, Hq, T] of a suffix call become the attention over prefix and suffix together: the
    ``splits`` partials of ``mha_prefix`` merged in split order, the suffix last (include/npm_hip.h npm_attn_combine)."""
    b, t, h, d = ctx.shape
    with _timed('attn_combine', nbytes=4.0 * d * b * t * h * (splits + 2)):
        _C.check(_C.lib().npm_attn_combine(part_ctx, part_lse, int(splits), ctx.ptr, h * d, lse.ptr, b, t, h, d, new_lens,
                                           int(bool(store_lse))), 'npm_attn_combine')


def rope_tables(rows: int, head_dim: int, base: float):
    """(cos, sin) float32 [rows, head_dim / 2] of rotary position embeddings: the angle of position p and pair i is
    p * base ** (-i / half), computed in float64 on the host and rounded once.  Row p does not depend on ``rows``."""
    half = head_dim // 2
    inv_freq = float(base) ** (-np.arange(half, dtype=np.float64) / half)
    angle = np.arange(rows, dtype=np.float64)[:, None] * inv_freq[None, :]
    return np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)


class RopeTable:
    """The cos / sin tables of one attention layer's rotary position embedding on the device (``rope_tables``).  ``ensure(rows)``
    makes them cover positions 0 .. rows - 1: the row count is rounded up to a power of two, so a decode loop does not upload
    them again every step; a layer sizes them once in ``make_cache``."""

    def __init__(self, head_dim: int, base: float):
        if head_dim < 2 or head_dim % 2:
            raise ValueError(f'rotary position embedding pairs element i with element i + D / 2: the head size {head_dim} is odd')
        if not base > 0:
            raise ValueError(f'rope_base must be a positive number, got {base!r}')
        self.head_dim, self.base = int(head_dim), float(base)
        self.rows = 0
        self.cos = self.sin = None

    def ensure(self, rows: int) -> 'RopeTable':
        if rows > self.rows:
            self.rows = 1 << max(int(rows) - 1, 0).bit_length()
            self.cos, self.sin = (from_host(t) for t in rope_tables(self.rows, self.head_dim, self.base))
        return self


def rope(x: Mat, batch: int, tokens: int, heads: int, head_dim: int, table: RopeTable, at: int = 0, at_lens: Optional[int] = None,
         inverse: bool = False) -> None:
    """Rotates, in place, the first ``heads`` heads of the rows b * tokens + t of ``x`` (array, row pitch) by the angles of
    position (``at_lens[b]`` or ``at``) + t (include/npm_hip.h npm_rope); ``inverse``: the transposed rotation, for gradients.
    ``at_lens``: the DEVICE address of [B] int32.  Whatever lies behind the ``heads`` heads in a row -- the V part of a packed
    projection -- is not touched.  ``table`` covers the positions (``RopeTable.ensure``)."""
    assert table.head_dim == head_dim and (at_lens is not None or at + tokens <= table.rows), (head_dim, at, tokens, table.rows)
    rows = batch * tokens
    with _timed('rope', nbytes=8.0 * rows * heads * head_dim + 4.0 * head_dim * min(rows, table.rows)):
        _C.check(_C.lib().npm_rope(x.ptr, x.ld, batch, tokens, heads, head_dim, table.cos.ptr, table.sin.ptr, table.rows, int(at),
                                   at_lens, int(bool(inverse))), 'npm_rope')


# One launch in front of the attention of a cached self-attention step instead of three (npm_rope, the K append, the V append):
# npm_rope_kv_append on the packed projection.  Off by default: every call sequence is what it was until a layer or a model turns
# it on (``MultiHeadAttention._fused_rope_append``; ``models.CausalLM`` does); the same bits either way (tools/lm_decode_bench.py).
FUSED_ROPE_APPEND = os.environ.get('NPM_FUSED_ROPE_APPEND', '0') != '0'


def rope_kv_append(qkv: Mat, k_ptr: int, v_ptr: int, layout: KVLayout, batch: int, tokens: int, heads: int, kv_heads: int,
                   head_dim: int, table: Optional[RopeTable], at: int, lens, rows: int) -> None:
    """``rope(qkv, batch, tokens, heads + kv_heads, head_dim, table, at, at_lens)`` and the two ``kv_append`` s of the k and the v
    heads of the packed projection ``qkv`` (array, row pitch; rows of (heads + 2 kv_heads) * head_dim floats) into the cache tensors
    at ``k_ptr`` / ``v_ptr`` of one ``layout``, in one launch (include/npm_hip.h npm_rope_kv_append).  ``table`` None: no rotation.
    ``lens`` = (at_lens, new_lens) as ``kv_append`` takes them; ``rows``: the rows stored, for the timer."""
    at_lens, new_lens = (None, None) if lens is None else lens
    assert table is None or (table.head_dim == head_dim and (at_lens is not None or at + tokens <= table.rows)), (head_dim, at, tokens)
    cos, sin, table_rows = (None, None, 0) if table is None else (table.cos.ptr, table.sin.ptr, table.rows)
    row = kv_heads * head_dim
    moved = 8.0 * batch * tokens * (heads + kv_heads) * head_dim * (table is not None) + (8.0 + 2.0 * KV_ITEMSIZE[layout.dtype]) * rows * row
    with _timed('rope_kv_append', nbytes=moved):
        _C.check(_entry_point('npm_rope_kv_append')(qkv.ptr, qkv.ld, batch, tokens, heads, kv_heads, head_dim, cos, sin, table_rows, int(at),
                                                    at_lens, new_lens, k_ptr, v_ptr, layout.pitch, layout.stride, layout.table,
                                                    layout.table_pitch, layout.page_rows, int(layout.dtype == 'f16')), 'npm_rope_kv_append')


def take_rows(x2d: DeviceArray, idx, out: Optional[Mat] = None) -> DeviceArray:
    """``x2d[idx]`` for a 2-D ``x2d`` [R, F] and integer ``idx`` of any shape (host integers, or an ``IdBuffer`` that never
    leaves the device): [..., F].  An index outside 0 .. R - 1 gives a row of zeros and reads nothing (include/npm_hip.h
    npm_take_rows).  ``out``: (array, row pitch) to write the rows into instead of a fresh array."""
    x2d = as_device(x2d)
    if x2d.ndim != 2:
        raise ValueError(f'take_rows: the source must be 2-D, got {x2d.shape}')
    idx = as_ids(idx)
    rows, cols = x2d.shape
    result = empty(tuple(idx.shape) + (cols,)) if out is None else None
    dst_ptr, dst_ld = (result.ptr, cols) if out is None else (out.ptr, out.ld)
    with _timed('take_rows', nbytes=8.0 * idx.size * cols):
        _C.check(_C.lib().npm_take_rows(x2d.ptr, cols, rows, idx.ptr, dst_ptr, dst_ld, idx.size, cols), 'npm_take_rows')
    return result


def embedding_bwd(dy: DeviceArray, ids: np.ndarray, dw: DeviceArray) -> None:
    """dw[v] = the sum of the rows r of ``dy`` [n, F] with ids[r] == v, added in ascending r in fp32; rows of tokens that do not
    occur are zero, ids outside the table are skipped (their forward rows were zeros).  The host sorts the ids stably; the
    kernel sums each token's rows in that order (include/npm_hip.h npm_embedding_bwd): deterministic, no atomics."""
    vocab, cols = dw.shape
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    assert dy.size == ids.size * cols, (dy.shape, ids.shape, dw.shape)
    if dw.size:
        _C.check(_C.lib().npm_fill_f32(dw.ptr, 0.0, dw.size), 'npm_fill_f32')
    order = np.argsort(ids, kind='stable')
    order = order[(ids[order] >= 0) & (ids[order] < vocab)]
    if order.size == 0 or cols == 0:
        return
    sorted_ids = ids[order]
    firsts = np.flatnonzero(np.concatenate([[True], sorted_ids[1:] != sorted_ids[:-1]]))
    tokens, starts = sorted_ids[firsts], np.concatenate([firsts, [order.size]])
    packed = bytes_from_host(np.concatenate([order, starts, tokens]).astype(np.int32))
    p_order, p_starts = packed.ptr, packed.ptr + 4 * order.size
    with _timed('embedding_bwd', nbytes=4.0 * cols * (order.size + tokens.size)):
        _C.check(_C.lib().npm_embedding_bwd(dy.ptr, cols, p_order, p_starts, p_starts + 4 * starts.size, int(tokens.size), dw.ptr,
                                            cols, cols), 'npm_embedding_bwd')


class KVCache:
    """Keys and values of the tokens seen so far: ``k`` [B, capacity, Hkv, Dk] and ``v`` [B, capacity, Hkv, Dv] on the device,
    of which the first ``lengths[b]`` rows of sequence b are valid.  Rows at and past that hold whatever was there; nothing reads
    them.  ``frozen`` marks a cross-attention cache (filled once, attended to as a whole, never appended to by ``forward``).

    ``lengths`` (host int64 [B]) is authoritative: ``room`` and every check read it, nothing is read back from the device.  While
    every sequence has the same number of rows the cache is *uniform*: ``length`` is that number and every call is the scalar
    one (npm_kv_append / npm_mha_decode_fwd).  ``new_lengths`` (per-sequence counts n[b] <= tokens of a right-padded chunk) makes
    it *ragged*: ``length`` then raises, ``max_length`` is the largest, and the kernels read the lengths from a device int32
    mirror, uploaded once per ragged call ([3, B] int32 -- rows before, new rows, rows after -- shared by the append and the
    attention that follows it).

    ``append``, ``attend`` and ``gather`` are written once, here: where the rows live is ``layout(x)``, which the wrappers above
    turn into the entry point.  ``paged``: whether that is a page pool (``PagedKVCache``).

    ``dtype`` 'f16': ``k`` and ``v`` are ``HalfBuffer`` s of the same geometry and half the bytes.  Rows are rounded to IEEE fp16
    once, by the append (round to nearest even; |x| >= 65520 becomes inf), and every reader -- the decode kernel, ``gather`` -- sees
    them as stored, converted back exactly (npm_kv_append_f16 / npm_mha_decode_fwd_f16 / npm_kv_gather_f16, and
    npm_mha_prefill_fwd_f16 behind ``PREFILL_KERNEL_F16``).  ``itemsize`` is the bytes per stored element and ``nbytes`` those of
    K + V.

    ``window`` W >= 1 (default None): sliding-window attention -- a token at position p sees keys max(0, p - W + 1) .. p.
    ``attend(..., causal=True)`` then calls the windowed entry points (npm_mha_decode_fwd_window / npm_mha_prefill_fwd_window),
    always in their per-sequence form; ``causal=False`` raises.  A contiguous windowed cache gains the speed only: its memory
    stays B x capacity (``PagedKVCache`` gives pages back)."""

    paged = False

    def __init__(self, batch: int, capacity: int, kv_heads: int, key_dim: int, value_dim: Optional[int] = None, dtype: str = 'f32',
                 window: Optional[int] = None, layers: int = 1):
        value_dim = key_dim if value_dim is None else value_dim
        if min(batch, capacity, kv_heads, key_dim, value_dim) < 1:
            raise ValueError('KVCache: batch, capacity, kv_heads and the head sizes must be positive')
        self.window = _kv_window(window, int(key_dim), int(value_dim))
        self.dtype = _kv_dtype(dtype, int(kv_heads), int(key_dim), int(value_dim))
        self.batch, self.capacity, self.kv_heads = int(batch), int(capacity), int(kv_heads)
        self.key_dim, self.value_dim = int(key_dim), int(value_dim)
        self._allocate_storage([batch, capacity, kv_heads], layers)
        self.lengths = np.zeros([self.batch], dtype=np.int64)
        self._mirror = None               # (host int32 [3, B]: before, new, after; ByteBuffer) of the last ragged call
        self.frozen = False

    def _storage(self, shape):
        return empty(shape) if self.dtype == 'f32' else HalfBuffer(shape)

    # ---- one cache for a stack of layers ---------------------------------------------------------------------------------------
    # ``layers=N`` > 1: the K and V tensors of N attention layers in ONE allocation [2, N, ...] (plane 2 * 0 + i is layer i's K,
    # N + i its V; Dk == Dv) behind ONE set of host state -- ``lengths``, the length mirror, and for a paged cache the block table,
    # the free list, ``refcount`` and ``dropped``.  ``fork`` / ``reorder`` / ``release`` / ``truncate`` are the single-layer host
    # operations.  A decode step is bracketed by the model: ``begin(tokens, new_lengths)`` does, once, what ``append`` does
    # between its checks and its launches (``room``, the window's reclaim, page allocation, copy-on-write in one launch for all
    # planes, the mirror and table upload); every layer then appends to and attends over its own ``layer(i)``, which reads that
    # step's numbers; ``commit()`` advances ``lengths``.  ``layers=1`` (default) is the cache as it always was.
    def _allocate_storage(self, geometry, layers: int) -> None:
        layers = int(layers)
        if layers < 1:
            raise ValueError(f'{type(self).__name__}: layers must be at least 1, got {layers}')
        self.layers, self._step, self._serial, self._planes = layers, None, 0, None
        if layers == 1:
            self.k = self._storage(list(geometry) + [self.key_dim])
            self.v = self._storage(list(geometry) + [self.value_dim])
            return
        if self.key_dim != self.value_dim:
            raise ValueError(f'{type(self).__name__}: a layered cache keeps K and V of every layer as planes of one allocation: the '
                             f'head sizes {self.key_dim} / {self.value_dim} differ')
        shape = list(geometry) + [self.key_dim]
        self._planes = self._storage([2, layers] + shape)
        self._plane_elements = _prod(shape)
        self.k, self.v = self._plane(0, shape), self._plane(layers, shape)      # layer 0's: the geometry every tensor has

    def _plane(self, index: int, shape):
        store, first = self._planes, index * self._plane_elements
        if self.dtype == 'f32':
            return store.flat_view(first, shape)
        out = HalfBuffer.__new__(HalfBuffer)
        out._buf, out.ptr, out.nbytes, out.shape = store._buf, store.ptr + 2 * first, 2 * self._plane_elements, tuple(shape)
        return out

    def _tensors(self):
        """Every K and V tensor of the cache: two, or the 2 N planes of a layered one."""
        if self.layers == 1:
            return [self.k, self.v]
        return [self._plane(i, self.k.shape) for i in range(2 * self.layers)]

    def layer(self, index: int) -> 'KVLayerView':
        """What layer ``index``'s attention sees of a layered cache: its own K and V, everything else this cache's."""
        index = int(index)
        if not 0 <= index < self.layers:
            raise IndexError(f'{type(self).__name__}.layer: no layer {index} among {self.layers}')
        if self.layers == 1:
            return KVLayerView(self, 0, self.k, self.v)
        return KVLayerView(self, index, self._plane(index, self.k.shape), self._plane(self.layers + index, self.k.shape))

    def _single(self, what: str) -> None:
        if self.layers != 1:
            raise ValueError(f'{type(self).__name__}.{what}: a layered cache is appended to and attended over through layer(i), '
                             'between begin() and commit()')

    def begin(self, tokens: int, new_lengths=None) -> None:
        """Opens a step that brings ``tokens`` (``new_lengths[b]``) rows to every layer: every check and all host work of the N
        appends, once.  ValueError, with nothing changed, when the rows do not fit."""
        if self._step is not None:
            raise RuntimeError(f'{type(self).__name__}.begin: the last step was not committed')
        self.room(tokens, new_lengths)
        if self.frozen:
            raise ValueError('KVCache: this cache was filled for cross-attention and is frozen; reset() it first')
        n = self.new_lengths(tokens, new_lengths)
        if self._scalar_call(n):
            step = (int(tokens), np.full([self.batch], int(tokens), dtype=np.int64), int(self.lengths[0]), None)
        else:
            n = self._counts(tokens, n)
            self._allocate(n)
            step = (int(tokens), n, 0, self._device_lengths(self.lengths, n)[:2])
            if self.paged:
                self._device_table()
        self._step, self._serial = step, self._serial + 1

    def commit(self) -> None:
        """Closes the step: ``lengths`` advance by what ``begin`` was told, once for all layers."""
        if self._step is None:
            raise RuntimeError(f'{type(self).__name__}.commit: no step is open')
        self.lengths = self.lengths + self._step[1]
        self._step = None

    def abandon(self) -> None:
        """Closes a step that failed half way: ``lengths`` stay (pages it took are those of rows nobody will read)."""
        self._step = None

    @property
    def itemsize(self) -> int:
        return KV_ITEMSIZE[self.dtype]

    @property
    def nbytes(self) -> int:
        """Bytes of K + V storage, of all layers."""
        return (self.k.nbytes + self.v.nbytes) * self.layers

    def layout(self, x) -> KVLayout:
        """Where the rows of ``x`` (``k`` or ``v``) live; pitches in elements."""
        row = self.kv_heads * x.shape[3]
        return KVLayout(row, self.capacity * row, dtype=self.dtype)

    @property
    def ragged(self) -> bool:
        return bool((self.lengths != self.lengths[0]).any())

    @property
    def length(self) -> int:
        """The number of valid rows while it is the same for every sequence."""
        if self.ragged:
            raise ValueError(f'KVCache.length: the sequences hold different numbers of rows {self.lengths.tolist()}; '
                             'use lengths / max_length')
        return int(self.lengths[0])

    @length.setter
    def length(self, value: int) -> None:
        self.lengths = np.full([self.batch], int(value), dtype=np.int64)

    @property
    def max_length(self) -> int:
        return int(self.lengths.max())

    def reset(self) -> None:
        self.lengths = np.zeros([self.batch], dtype=np.int64)
        self._mirror = None
        self.frozen = False
        self._step = None

    def new_lengths(self, tokens: int, new_lengths) -> Optional[np.ndarray]:
        """``new_lengths`` as int64 [B] with 0 <= n[b] <= tokens (ValueError otherwise); None when it is None or says what the
        scalar call says (every n[b] == tokens)."""
        if new_lengths is None:
            return None
        n = np.asarray(new_lengths)
        if n.shape != (self.batch,) or not np.issubdtype(n.dtype, np.integer) or (n < 0).any() or (n > tokens).any():
            raise ValueError(f'new_lengths must be {self.batch} integers in 0 .. {tokens}, got {np.asarray(new_lengths).tolist()}')
        return None if (n == tokens).all() else n.astype(np.int64)

    def _counts(self, tokens: int, n: Optional[np.ndarray]) -> np.ndarray:
        """The rows every sequence brings, int64 [B]: ``n`` as ``new_lengths()`` returned it, with its None spelled out."""
        return np.full([self.batch], tokens, dtype=np.int64) if n is None else n

    def _scalar_call(self, n: Optional[np.ndarray]) -> bool:
        """Whether a call bringing ``n`` (of ``new_lengths()``) is the scalar one: a contiguous cache, uniform before and after."""
        return n is None and not (self.paged or self.ragged)

    def room(self, tokens: int, new_lengths=None) -> None:
        """ValueError when ``tokens`` (or ``new_lengths[b]``) more rows do not fit ANY sequence -- checked before anything is
        launched."""
        n = self.new_lengths(tokens, new_lengths)
        if tokens < 0 or (self.lengths + (tokens if n is None else n) > self.capacity).any():
            raise ValueError(f'KVCache: {self._counts(tokens, n).tolist() if new_lengths is not None else tokens} new rows after '
                             f'{self.lengths.tolist() if self.ragged else int(self.lengths[0])} do not fit the capacity {self.capacity}')

    def _allocate(self, n: np.ndarray) -> None:
        """What a ragged ``append`` does between its checks and its launches so that n[b] more rows have a place: nothing here."""

    def _device_lengths(self, before: np.ndarray, n: np.ndarray):
        """Device addresses of (before, n, before + n) as int32 [B] each; one upload unless the last one holds the same numbers."""
        host = np.stack([before, n, before + n]).astype(np.int32)
        if self._mirror is None or not np.array_equal(self._mirror[0], host):
            self._mirror = (host, bytes_from_host(host))
        ptr = self._mirror[1].ptr
        return ptr, ptr + 4 * self.batch, ptr + 8 * self.batch

    def _current_lengths(self) -> int:
        """Device address of ``lengths`` as int32 [B]: the last row of the mirror when the last ragged call left them there (an
        append of this forward did), else one upload."""
        if self._mirror is None or not np.array_equal(self._mirror[0][2], self.lengths):
            self._device_lengths(self.lengths, np.zeros([self.batch], dtype=np.int64))
        return self._mirror[1].ptr + 8 * self.batch

    def append(self, k: Mat, v: Mat, tokens: int, new_lengths=None) -> None:
        """``tokens`` freshly projected rows per sequence ([B, T, Hkv * D] with a row pitch each) behind the valid ones; with
        ``new_lengths`` only the first n[b] of them, behind sequence b's own ``lengths[b]`` rows."""
        n, at, lens, rows = self._append_plan(tokens, new_lengths)
        for src, dst in ((k, self.k), (v, self.v)):
            kv_append(src, dst.ptr, self.layout(dst), self.batch, tokens, at, lens, rows)
        self.lengths = self.lengths + n

    def _append_plan(self, tokens: int, new_lengths):
        """What an append does in front of its launches: the checks, the pages of a ragged call, the length upload.  Returns
        (rows every sequence brings, the scalar ``at``, (at_lens, new_lens) or None, rows stored)."""
        self._single('append')
        self.room(tokens, new_lengths)
        if self.frozen:
            raise ValueError('KVCache: this cache was filled for cross-attention and is frozen; reset() it first')
        n = self.new_lengths(tokens, new_lengths)
        if self._scalar_call(n):
            return tokens, int(self.lengths[0]), None, self.batch * tokens
        n = self._counts(tokens, n)
        self._allocate(n)
        return n, 0, self._device_lengths(self.lengths, n)[:2], int(n.sum())

    def append_rotated(self, qkv: Mat, heads: int, tokens: int, new_lengths=None, table: Optional['RopeTable'] = None) -> None:
        """``append`` of the k and the v heads of the packed projection ``qkv`` ([B, T, heads + 2 Hkv, D] with a row pitch) with
        the rotation of its q and k heads (``rope`` at the positions ``lengths[b] + t``; ``table`` None: none) in the same launch
        (``rope_kv_append``).  Dk == Dv.  ``qkv`` is left rotated, as ``rope`` leaves it."""
        assert self.key_dim == self.value_dim
        n, at, lens, rows = self._append_plan(tokens, new_lengths)
        rope_kv_append(qkv, self.k.ptr, self.v.ptr, self.layout(self.k), self.batch, tokens, heads, self.kv_heads, self.key_dim, table,
                       at, lens, rows)
        self.lengths = self.lengths + n

    def _truncated(self, rows) -> np.ndarray:
        """The lengths after ``truncate(rows)``, int64 [B]; every refusal of ``truncate`` is raised here, with nothing changed."""
        if self.frozen:
            raise ValueError('KVCache.truncate: this cache was filled for cross-attention and is frozen')
        r = np.asarray(rows)
        if r.dtype == np.bool_ or not np.issubdtype(r.dtype, np.integer) or r.shape not in ((), (self.batch,)):
            raise ValueError(f'KVCache.truncate: rows must be an integer or {self.batch} integers, got {rows!r}')
        r = np.broadcast_to(r, [self.batch]).astype(np.int64)
        if (r < 0).any() or (r > self.lengths).any():
            raise ValueError(f'KVCache.truncate: {r.tolist()} rows cannot leave sequences of {self.lengths.tolist()} rows')
        return self.lengths - r

    def truncate(self, rows) -> None:
        """The last ``rows`` (an integer, or [B] integers with 0 <= rows[b] <= lengths[b]) rows of every sequence leave the
        cache: ``lengths[b] -= rows[b]``, which is all -- nothing is launched, and nothing reads a row at or past a length.
        What a speculative step does with the rows of the drafted tokens that were not accepted.  ValueError, with nothing
        changed, for anything else and for a frozen cache."""
        self.lengths = self._truncated(rows)

    def write_slot(self, b: int, k: Optional[Mat], v: Optional[Mat], rows: int) -> None:
        """Sequence ``b`` is replaced: its rows 0 .. rows - 1 are the ``rows`` rows of ``k`` / ``v`` ([rows, Hkv * D] with a row
        pitch each) and ``lengths[b] = rows``; the other sequences are not touched (npm_kv_append on slot b alone).  ``k`` or ``v``
        None: that tensor is written by another call (``TransformerDecoder.admit`` projects and writes one after the other)."""
        self._single('write_slot')
        b, rows = int(b), int(rows)
        if not 0 <= b < self.batch:
            raise IndexError(f'KVCache.write_slot: no sequence {b} in a batch of {self.batch}')
        if not 0 <= rows <= self.capacity:
            raise ValueError(f'KVCache.write_slot: {rows} rows do not fit the capacity {self.capacity}')
        for src, dst in ((k, self.k), (v, self.v)):
            if src is not None:
                layout = self.layout(dst)
                kv_append(src, dst.ptr + self.itemsize * b * layout.stride, layout, 1, rows, 0, None, rows)
        self.lengths[b] = rows

    def _fork_slots(self, src, dst):
        src, dst = int(src), int(dst)
        for i in (src, dst):
            if not 0 <= i < self.batch:
                raise IndexError(f'{type(self).__name__}.fork: no sequence {i} in a batch of {self.batch}')
        if src == dst:
            raise ValueError(f'{type(self).__name__}.fork: sequence {src} cannot be forked onto itself')
        return src, dst

    def fork(self, src: int, dst: int) -> None:
        """Slot ``dst`` becomes a copy of sequence ``src``: its ``lengths[src]`` rows of K and V are copied on the device (one
        copy per tensor) and ``lengths[dst] = lengths[src]``; what ``dst`` held is replaced, as by ``write_slot``.  The API of
        ``PagedKVCache.fork`` without the sharing; a frozen (cross-attention) cache may be forked.  IndexError / ValueError with
        nothing changed for a slot outside the batch or ``src == dst``."""
        src, dst = self._fork_slots(src, dst)
        rows = int(self.lengths[src])
        for x in self._tensors():
            slot = self.itemsize * self.layout(x).stride
            if rows:
                _C.check(_C.lib().npm_d2d(x.ptr + dst * slot, x.ptr + src * slot, self.itemsize * rows * self.layout(x).pitch), 'npm_d2d')
        self.lengths[dst] = rows

    def _parents(self, parents) -> np.ndarray:
        """``parents`` of ``reorder`` as int64 [B] with every entry in -1 .. B - 1; ValueError / IndexError otherwise."""
        p = np.asarray(parents)
        if p.shape != (self.batch,) or p.dtype == np.bool_ or not np.issubdtype(p.dtype, np.integer):
            raise ValueError(f'{type(self).__name__}.reorder: parents must be {self.batch} integers, got {parents!r}')
        p = p.astype(np.int64)
        if (p < -1).any() or (p >= self.batch).any():
            raise IndexError(f'{type(self).__name__}.reorder: parents name slots -1 (empty) .. {self.batch - 1}, got {p.tolist()}')
        return p

    def reorder(self, parents) -> None:
        """Slot b becomes the sequence slot ``parents[b]`` held BEFORE the call (int [B]; -1 empties the slot): what a beam
        step does to its W sequences.  A slot whose parent is another slot gets that slot's ``lengths[parent]`` rows of K and of
        V copied on the device -- O(L) per moved slot, where ``PagedKVCache.reorder`` moves a table row.  Swaps and chains are
        safe: a slot that is both read and overwritten is read from a snapshot taken first (one more copy of its rows), and
        slots that only move are copied in place.  A frozen (cross-attention) cache may be reordered.  IndexError / ValueError
        with nothing changed for a vector that is not [B] integers in -1 .. B - 1."""
        p = self._parents(parents)
        moved = [b for b in range(self.batch) if p[b] >= 0 and p[b] != b and self.lengths[p[b]] > 0]
        overwritten = set(moved)
        sources = sorted({int(p[b]) for b in moved})
        for x in self._tensors():
            layout = self.layout(x)
            slot, row = self.itemsize * layout.stride, self.itemsize * layout.pitch
            snapshot = {}
            for s in sources:
                if s in overwritten:                   # its rows are about to change: keep them as they were
                    keep = ByteBuffer(int(self.lengths[s]) * row)
                    _C.check(_C.lib().npm_d2d(keep.ptr, x.ptr + s * slot, keep.nbytes), 'npm_d2d')
                    snapshot[s] = keep
            for b in moved:
                s = int(p[b])
                src = snapshot[s].ptr if s in snapshot else x.ptr + s * slot
                _C.check(_C.lib().npm_d2d(x.ptr + b * slot, src, int(self.lengths[s]) * row), 'npm_d2d')
        self.lengths = np.where(p >= 0, self.lengths[np.maximum(p, 0)], 0)

    def attend(self, q: Mat, heads: int, tokens: int, scale: float, causal: bool, want_lse: bool = False, new_lengths=None,
               kernel: str = 'decode'):
        """``mha_decode`` of ``tokens`` query rows per sequence over the valid rows; with ``new_lengths`` (or a ragged or paged
        cache) its ragged call: rows t >= n[b] are padding and come back as zeros.  ``causal``: the n[b] new tokens are the last
        n[b] valid rows of sequence b (they were appended first).  ``kernel='prefill'``: ``mha_prefill``, the same contract for any
        number of rows (a uniform cache shorter than the query -- a frozen one -- takes its per-sequence call); on an fp16 cache
        only with ``PREFILL_KERNEL_F16`` on."""
        self._single('attend')
        if kernel not in ('decode', 'prefill'):
            raise ValueError(f"KVCache.attend: kernel must be 'decode' or 'prefill', got {kernel!r}")
        windowed = self.window is not None                               # always the per-sequence call, whatever the switch says
        if windowed and not causal:
            raise ValueError('KVCache.attend: a windowed cache is a self-attention cache: causal=False has no window to apply')
        if kernel == 'prefill' and self.dtype != 'f32' and not (PREFILL_KERNEL_F16 or windowed):
            raise ValueError(f"KVCache.attend: the prefill kernel reads an {self.dtype} cache only with PREFILL_KERNEL_F16 on "
                             "(NPM_PREFILL_KERNEL_F16=1); without it the cache takes kernel='decode' or gather()")
        attend = mha_prefill if kernel == 'prefill' else mha_decode
        n = self.new_lengths(tokens, new_lengths)
        if not windowed and self._scalar_call(n) and (kernel == 'decode' or tokens <= int(self.lengths[0])):
            return attend(q, self, heads, tokens, int(self.lengths[0]), scale, causal, want_lse)
        n = self._counts(tokens, n)
        if causal and (n > self.lengths).any():
            raise ValueError(f'KVCache.attend: {n.tolist()} new tokens are not among the {self.lengths.tolist()} valid rows')
        prefix = self.attend_prefix_rows(n, causal)
        if prefix:
            # one upload: the lengths in the coordinates of the rows behind the prefix (a sequence that brings nothing may be shorter)
            behind = np.maximum(self.lengths - prefix, 0)
            _, new_ptr, kv_ptr = self._device_lengths(behind - n, n)
            ctx, lse = attend(q, self, heads, tokens, self.max_length - prefix, scale, True, True, lens=(kv_ptr, new_ptr),
                              keys=int(behind.sum()), prefix=prefix)
            first = int(np.nonzero(n)[0][0])
            table = self.layout(self.k)
            splits, part_ctx, part_lse, keep = mha_prefix(q, self, heads, tokens, scale, new_ptr, table.table + 4 * first * table.table_pitch,
                                                          prefix)
            attn_combine(part_ctx, part_lse, splits, ctx, lse, new_ptr, want_lse)
            return ctx, (lse if want_lse else None)
        _, new_ptr, kv_ptr = self._device_lengths(self.lengths - n, n)
        return attend(q, self, heads, tokens, self.max_length, scale, causal, want_lse, lens=(kv_ptr, new_ptr),
                      keys=int(self.lengths.sum()), window=self.window)

    def attend_prefix_rows(self, n: np.ndarray, causal: bool) -> int:
        """The rows of a shared prefix that ``attend`` reads in one pass for all sequences; 0: the ordinary call.  A contiguous
        cache shares nothing."""
        return 0

    def gather(self, rows: int):
        """(k, v) [B, rows, Hkv, D]: the valid rows of every sequence made contiguous, zeros behind them (``kv_gather_rows``)."""
        self._single('gather')
        assert rows <= self.capacity
        if self.paged and self.dropped.any():
            raise ValueError(f'PagedKVCache.gather: the leading {self.dropped.tolist()} rows were given back (window={self.window}); '
                             'there is nothing to gather them from')
        lens = self._current_lengths()
        out = []
        for x in (self.k, self.v):
            y = empty([self.batch, rows, self.kv_heads, x.shape[3]])
            kv_gather_rows(x.ptr, self.layout(x), y, lens)
            out.append(y)
        return out


# ---- paged key / value cache ---------------------------------------------------------------------------------------------------
class PagedKVCache(KVCache):
    """``KVCache`` whose rows live in a pool of pages: ``k`` [pages, page_size, Hkv, Dk] and ``v`` [pages, page_size, Hkv, Dv] on
    the device, and ``block_table`` (host int32 [B, ceil(capacity / page_size)], -1 = none) naming the page of every
    ``page_size`` logical rows of a sequence.  Pages are handed out as sequences grow (lowest-numbered free page first, so two
    runs build the same table) and come back with ``release(b)``; the released slot then takes a new sequence through the
    ordinary ragged call while the others keep decoding.  The pool, not ``batch * capacity``, is what the cache costs.

    ``capacity`` is the most rows ONE sequence may reach; ``pages`` the pool size (None: ``batch * ceil(capacity / page_size)``,
    which cannot run out).  ``page_size``: a power of two >= 16 (the decode kernel's key tile: a tile never straddles a page).
    Host state is authoritative, as ``lengths`` is; the device mirror of the table is uploaded only when the table changed
    (``table_uploads`` counts them).  Every call is the paged one (npm_kv_append_paged / npm_mha_decode_fwd_paged /
    npm_kv_gather_paged), uniform lengths included: it is bitwise the uniform entry point.

    ``window`` W: pages come back while a sequence is still alive.  After an append left ``lengths[b]`` rows, keys below
    ``lengths[b] - W + 1`` can never be seen again; at the start of the next ``append`` every page whose rows all lie below that
    bound returns to the free list, its table slot becomes -1 and ``dropped[b]`` (host int64 [B], a multiple of ``page_size``)
    counts the leading rows given up.  ``lengths`` stays the absolute length (rotary positions and ``capacity`` do not change); a
    sequence holds at most ceil((W - 1 + T) / page_size) + 1 pages between calls of T tokens; ``room`` counts the pages about to
    come back as free; ``gather`` raises once rows were dropped.

    Sharing: ``fork(src, dst)`` makes two sequences name the same pages.  ``refcount`` (host int32 [pages]) counts the sequences
    naming each page; a page is on the free list exactly when its count is 0, so ``release``, ``truncate`` and the window's
    reclaim only decrement, and ``pages_in_use`` counts distinct pages.  Copy-on-write sits in ``_allocate``: before an append
    writes into a partly filled page that another sequence names, the sequence takes a page of its own and the valid rows are
    copied on the device (npm_kv_copy_pages, one launch per tensor and call; ``page_copies`` counts the pages); ``room`` counts
    those pages.  With ``SHARED_PREFIX`` on, a causal ``attend`` reads the pages all active sequences share once
    (``shared_prefix_rows``; npm_mha_prefix_fwd, the paged call over the rest, npm_attn_combine).

    Its own: the pool and the table (``layout``), the page accounting ``append`` calls on (``room``, ``_reclaim``, ``_allocate``),
    ``release`` and ``fork``; ``append``, ``attend`` and ``gather`` are ``KVCache``'s."""

    paged = True

    def __init__(self, batch: int, capacity: int, kv_heads: int, key_dim: int, value_dim: Optional[int] = None, *, page_size: int,
                 pages: Optional[int] = None, dtype: str = 'f32', window: Optional[int] = None, layers: int = 1):
        value_dim = key_dim if value_dim is None else value_dim
        if min(batch, capacity, kv_heads, key_dim, value_dim) < 1:
            raise ValueError('PagedKVCache: batch, capacity, kv_heads and the head sizes must be positive')
        self.window = _kv_window(window, int(key_dim), int(value_dim))
        self.dtype = _kv_dtype(dtype, int(kv_heads), int(key_dim), int(value_dim))
        page_size = int(page_size)
        if page_size < 16 or page_size & (page_size - 1):
            raise ValueError(f'PagedKVCache: page_size must be a power of two >= 16, got {page_size}')
        self.batch, self.capacity, self.kv_heads = int(batch), int(capacity), int(kv_heads)
        self.key_dim, self.value_dim = int(key_dim), int(value_dim)
        self.page_size = page_size
        self.pages_per_sequence = -(-self.capacity // page_size)
        self.pages = self.batch * self.pages_per_sequence if pages is None else int(pages)
        if self.pages < 1:
            raise ValueError(f'PagedKVCache: pages must be positive, got {pages}')
        self._allocate_storage([self.pages, page_size, kv_heads], layers)
        self.table_uploads = 0
        self.reset()

    def layout(self, x) -> KVLayout:
        row = self.kv_heads * x.shape[3]
        return KVLayout(row, self.page_size * row, self._device_table(), self.pages_per_sequence, self.page_size, self.dtype)

    def reset(self) -> None:
        KVCache.reset(self)
        self.block_table = np.full([self.batch, self.pages_per_sequence], -1, dtype=np.int32)
        self.dropped = np.zeros([self.batch], dtype=np.int64)   # leading rows whose pages were given back (window)
        self._free = list(range(self.pages))          # a heap: the lowest-numbered free page first
        self.refcount = np.zeros([self.pages], dtype=np.int32)   # sequences naming each page; on the free list exactly when 0
        self.page_copies = 0                          # pages copied by copy-on-write so far
        self._table_dev = None                        # ByteBuffer of the table as the device last saw it
        self._table_dirty = True

    @property
    def pages_free(self) -> int:
        return len(self._free)

    @property
    def pages_in_use(self) -> int:
        return self.pages - len(self._free)

    @property
    def length(self) -> int:
        return KVCache.length.fget(self)

    @length.setter
    def length(self, value: int) -> None:
        raise ValueError('PagedKVCache.length cannot be assigned: rows need pages (append), and release(b) returns them')

    def _pages_needed(self, n: np.ndarray) -> np.ndarray:
        """Pages every sequence lacks for n[b] more rows."""
        size = self.page_size
        return -(-(self.lengths + n) // size) - -(-self.lengths // size)

    def room(self, tokens: int, new_lengths=None) -> None:
        """``KVCache.room``, and ValueError when the new rows need more pages than are free -- before anything is launched, with
        lengths, table and free list as they were."""
        KVCache.room(self, tokens, new_lengths)
        n = self._counts(tokens, self.new_lengths(tokens, new_lengths))
        need = int(self._pages_needed(n).sum()) + len(self._copy_on_write(n))
        free = self.pages_free + self._reclaim_frees()
        if need > free:
            raise ValueError(f'PagedKVCache: {n.tolist()} new rows after {self.lengths.tolist()} need {need} more pages of '
                             f'{self.page_size} rows, {free} of {self.pages} are free; release() a sequence first')

    def _reclaimable(self) -> np.ndarray:
        """Rows per sequence, a multiple of ``page_size``, that the next ``append`` gives back: whole pages below
        ``lengths[b] - window + 1`` that are still held."""
        if self.window is None:
            return np.zeros([self.batch], dtype=np.int64)
        bound = np.maximum(self.lengths - self.window + 1, 0) // self.page_size * self.page_size
        return np.maximum(bound - self.dropped, 0)

    def _reclaim_frees(self) -> int:
        """Pages that ``_reclaim`` puts on the free list: those of ``_reclaimable`` that no other sequence goes on naming."""
        rows = self._reclaimable()
        if not rows.any():
            return 0
        left = self.refcount.copy()
        for b in np.nonzero(rows)[0]:
            first = int(self.dropped[b]) // self.page_size
            left[self.block_table[b, first:first + int(rows[b]) // self.page_size]] -= 1
        return int(((left == 0) & (self.refcount > 0)).sum())

    def _unref(self, page: int) -> None:
        """One sequence fewer names ``page``; the last one gives it back to the free list."""
        self.refcount[page] -= 1
        if self.refcount[page] == 0:
            heapq.heappush(self._free, int(page))

    def _copy_on_write(self, n: np.ndarray):
        """[(b, table slot, page, valid rows)] of the appends that must first take a page of their own: sequence b brings rows
        (n[b] > 0), its next row falls into a partly filled page, and that page is still named by another sequence once the
        earlier sequences of this call have taken their copies.  The last owner writes in place; a full page is never copied."""
        out, left = [], {}
        for b in np.nonzero(n)[0]:
            rows = int(self.lengths[b]) % self.page_size
            if not rows:
                continue
            slot = int(self.lengths[b]) // self.page_size
            page = int(self.block_table[b, slot])
            if left.setdefault(page, int(self.refcount[page])) > 1:
                left[page] -= 1
                out.append((int(b), slot, page, rows))
        return out

    def _reclaim(self) -> None:
        """The pages of ``_reclaimable`` given up -- back to the free list unless another sequence names them --, their table
        slots -1, ``dropped`` advanced."""
        rows = self._reclaimable()
        for b in np.nonzero(rows)[0]:
            first = int(self.dropped[b]) // self.page_size
            for slot in range(first, first + int(rows[b]) // self.page_size):
                self._unref(int(self.block_table[b, slot]))
                self.block_table[b, slot] = -1
            self.dropped[b] += rows[b]
            self._table_dirty = True

    def _take(self) -> int:
        page = heapq.heappop(self._free)
        self.refcount[page] = 1
        return page

    def _allocate(self, n: np.ndarray) -> None:
        """Pages for n[b] more rows.  Copy-on-write lives here and nowhere else: a sequence about to write into a partly filled
        page that another sequence names takes a fresh page first, and the valid rows of K and of V are copied into it on the
        device -- one launch per tensor for all sequences of the call (npm_kv_copy_pages)."""
        self._reclaim()
        copies = self._copy_on_write(n)
        for b, slot, page, _ in copies:
            self.block_table[b, slot] = self._take()
            self.refcount[page] -= 1                  # another sequence still names it: it does not come back
            self._table_dirty = True
        need = self._pages_needed(n)
        have = -(-self.lengths // self.page_size)
        for b in np.nonzero(need)[0]:
            for slot in range(int(have[b]), int(have[b] + need[b])):
                self.block_table[b, slot] = self._take()
            self._table_dirty = True
        if copies:
            pairs = bytes_from_host(np.array([[page for _, _, page, _ in copies], [self.block_table[b, slot] for b, slot, _, _ in copies],
                                              [rows for _, _, _, rows in copies]], dtype=np.int32))
            count = len(copies)
            if self.layers > 1:                       # K and V of every layer: the planes of one allocation, one launch
                row, planes = self.itemsize * self.kv_heads * self.key_dim, 2 * self.layers
                with _timed('kv_copy_pages', nbytes=2.0 * planes * row * sum(rows for _, _, _, rows in copies)):
                    _C.check(_entry_point('npm_kv_copy_pages_planes')(
                        self._planes.ptr, self.page_size * row, row, pairs.ptr, pairs.ptr + 4 * count, pairs.ptr + 8 * count, count,
                        planes, self.itemsize * self._plane_elements), 'npm_kv_copy_pages_planes')
            for x in (self.k, self.v) if self.layers == 1 else ():
                row = self.itemsize * self.kv_heads * x.shape[3]
                with _timed('kv_copy_pages', nbytes=2.0 * row * sum(rows for _, _, _, rows in copies)):
                    _C.check(_C.lib().npm_kv_copy_pages(x.ptr, self.page_size * row, row, pairs.ptr, pairs.ptr + 4 * count,
                                                        pairs.ptr + 8 * count, count), 'npm_kv_copy_pages')
            self.page_copies += count

    def fork(self, src: int, dst: int) -> None:
        """Slot ``dst`` becomes the sequence of slot ``src`` with nothing launched and no page taken: the same table row,
        ``lengths`` and ``dropped``, and every named page's ``refcount`` one higher.  The sequences then grow apart through
        copy-on-write (``_allocate``).  ``dst`` must be empty (``lengths[dst] == 0``: ``release`` it first) and not ``src``:
        ValueError / IndexError otherwise, with nothing changed.  A windowed cache may be forked."""
        src, dst = self._fork_slots(src, dst)
        if self.lengths[dst] != 0:
            raise ValueError(f'PagedKVCache.fork: slot {dst} still holds {int(self.lengths[dst])} rows; release() it first')
        self.block_table[dst] = self.block_table[src]
        self.refcount[self.block_table[dst][self.block_table[dst] >= 0]] += 1
        self.lengths[dst] = self.lengths[src]
        self.dropped[dst] = self.dropped[src]
        self._table_dirty = True

    def reorder(self, parents) -> None:
        """Slot b becomes the sequence slot ``parents[b]`` held BEFORE the call (int [B]; -1 empties the slot), all slots at
        once: what a beam step does, where ``release`` / ``fork`` would need a spare slot for a permutation.  Host state only --
        nothing is launched and no page is taken: the new table, ``lengths`` and ``dropped`` are the old rows indexed by
        ``parents``, ``refcount`` becomes the number of table entries naming each page, and pages that reach 0 return to the free
        list.  Children of one parent share its pages and grow apart through copy-on-write (one copied tail page per beam and
        step at most).  The table is marked for upload only if a row changed: an identity reorder, or a parent that keeps its
        only child in its own slot, costs nothing.  Windowed and fp16 caches work unchanged.  IndexError / ValueError with nothing
        changed for a vector that is not [B] integers in -1 .. B - 1."""
        p = self._parents(parents)
        live, source = p >= 0, np.maximum(p, 0)
        table = np.where(live[:, None], self.block_table[source], -1).astype(np.int32)
        lengths, dropped = np.where(live, self.lengths[source], 0), np.where(live, self.dropped[source], 0)
        if not np.array_equal(table, self.block_table):
            refcount = np.bincount(table[table >= 0], minlength=self.pages).astype(np.int32)
            for page in np.nonzero((self.refcount > 0) & (refcount == 0))[0]:
                heapq.heappush(self._free, int(page))
            self.block_table, self.refcount = table, refcount
            self._table_dirty = True
        self.lengths, self.dropped = lengths, dropped

    def shared_prefix_rows(self, n) -> int:
        """P = ``page_size`` x the number of leading table slots that every sequence with n[b] > 0 fills with the SAME page and
        that lie wholly below every such sequence's ``lengths[b] - n[b]``: shared pages hold old rows only (copy-on-write keeps
        the new ones private).  0 with fewer than two such sequences, with a ``window`` and once rows were dropped."""
        n = np.asarray(n)
        active = np.nonzero(n > 0)[0]
        if active.size < 2 or self.window is not None or self.dropped.any():
            return 0
        slots = int((self.lengths[active] - n[active]).min()) // self.page_size
        if slots <= 0:
            return 0
        rows = self.block_table[active, :slots]
        same = ((rows == rows[0]).all(axis=0)) & (rows[0] >= 0)
        return self.page_size * (slots if same.all() else int(np.argmin(same)))

    def attend_prefix_rows(self, n: np.ndarray, causal: bool) -> int:
        if not (SHARED_PREFIX and causal and self.window is None and mha_prefix_supported(self.key_dim, self.value_dim)):
            return 0
        prefix = self.shared_prefix_rows(n)
        return prefix if prefix >= max(SHARED_PREFIX_MIN_ROWS, 1) else 0

    def _device_table(self) -> int:
        """Device address of the block table, int32 [B, pages_per_sequence]; uploaded only when it changed.  Slots without a page
        go up as page 0: no kernel forms an address from them, and the entry stays inside the pool whatever happens."""
        if self._table_dirty or self._table_dev is None:
            self._table_dev = bytes_from_host(np.maximum(self.block_table, 0))
            self._table_dirty = False
            self.table_uploads += 1
        return self._table_dev.ptr

    def release(self, b) -> None:
        """Sequence ``b`` (an index or several) ends: its pages go back to the free list and ``lengths[b] = 0``.  Nothing is
        launched and nothing is cleared -- no kernel reads past a length."""
        for i in np.unique(np.atleast_1d(np.asarray(b, dtype=np.int64))):
            if not 0 <= i < self.batch:
                raise IndexError(f'PagedKVCache.release: no sequence {i} in a batch of {self.batch}')
            for page in self.block_table[i][self.block_table[i] >= 0]:
                self._unref(int(page))
            self.block_table[i] = -1
            self.lengths[i] = 0
            self.dropped[i] = 0
            self._table_dirty = True

    def truncate(self, rows) -> None:
        """``KVCache.truncate``, and every page above ceil(new length / page_size) goes back to the free list, its table slot
        becomes -1 and the table is uploaded again before its next use.  With a ``window`` the new length L' must still have
        its window -- max(L' - window + 1, 0) >= dropped[b] wherever L' > 0 -- else ValueError with lengths, table and free list
        as they were; a rollback inside the chunk just appended always has it, since pages are reclaimed at the start of
        ``append`` from the length before it."""
        after = self._truncated(rows)
        if self.window is not None:
            short = (after > 0) & (np.maximum(after - self.window + 1, 0) < self.dropped)
            if short.any():
                raise ValueError(f'PagedKVCache.truncate: lengths {after.tolist()} would reach below the {self.dropped.tolist()} '
                                 f'leading rows already given back (window={self.window})')
        keep, have = -(-after // self.page_size), -(-self.lengths // self.page_size)
        for b in np.nonzero(have > keep)[0]:
            for slot in range(int(keep[b]), int(have[b])):
                if self.block_table[b, slot] >= 0:                # below ``dropped`` the window gave the page back already
                    self._unref(int(self.block_table[b, slot]))
                self.block_table[b, slot] = -1
            self._table_dirty = True
        self.dropped[after == 0] = 0                              # an emptied sequence starts over, as after release()
        self.lengths = after

    def write_slot(self, b: int, k: Optional[Mat], v: Optional[Mat], rows: int) -> None:
        raise NotImplementedError('PagedKVCache.write_slot: a released slot is filled by the ragged append, which hands out its pages')


class KVLayerView:
    """Layer i of a layered cache (``KVCache(..., layers=N).layer(i)``) as ``MultiHeadAttention._forward_cached`` sees a cache: its
    own ``k`` / ``v`` -- two planes of the parent's one allocation -- and its own ``lengths``: the parent's, plus the open step's
    rows once this layer's ``append`` has stored them, so that the attention behind it finds its rows counted.  Everything else is
    the parent's: geometry, type, window, the length mirror, the block table.  ``room`` is the parent's ``begin``, which ran;
    ``append`` launches the row copies with that step's numbers and touches no host state of the parent.  It shares nothing across
    sequences on its own: ``attend_prefix_rows`` is 0 (the one-pass prefix attention is not built for layered caches)."""

    def __init__(self, parent: KVCache, index: int, k, v):
        self._parent, self.index, self.k, self.v = parent, int(index), k, v
        self._appended = 0                              # the serial of the step this layer has appended its rows of

    def __getattr__(self, name):                        # only what this class does not define
        if name == '_parent':
            raise AttributeError(name)
        return getattr(self._parent, name)

    @property
    def lengths(self) -> np.ndarray:
        parent = self._parent
        if parent._step is not None and self._appended == parent._serial:
            return parent.lengths + parent._step[1]
        return parent.lengths

    ragged = KVCache.ragged
    max_length = KVCache.max_length
    _scalar_call = KVCache._scalar_call
    attend = KVCache.attend
    gather = KVCache.gather

    @property
    def length(self) -> int:
        return KVCache.length.fget(self)

    def layout(self, x) -> KVLayout:
        return type(self._parent).layout(self, x)

    def _single(self, what: str) -> None:
        """(``attend`` and ``gather`` are the single-layer ones, run over this layer's tensors)"""

    def attend_prefix_rows(self, n, causal: bool) -> int:
        return 0

    def _current_lengths(self) -> int:
        parent = self._parent
        if parent._mirror is None or not np.array_equal(parent._mirror[0][2], self.lengths):
            parent._device_lengths(self.lengths, np.zeros([self.batch], dtype=np.int64))
        return parent._mirror[1].ptr + 8 * self.batch

    def _open_step(self, what: str, tokens: int, new_lengths):
        step = self._parent._step
        if step is None:
            raise RuntimeError(f'KVLayerView.{what}: no step is open: the model calls begin(tokens, new_lengths) on the layered cache first')
        n = self._counts(tokens, self.new_lengths(tokens, new_lengths))
        if int(tokens) != step[0] or not np.array_equal(n, step[1]):
            raise ValueError(f'KVLayerView.{what}: {n.tolist()} of {tokens} rows are not what begin() was told ({step[1].tolist()} of {step[0]})')
        return step

    def room(self, tokens: int, new_lengths=None) -> None:
        self._open_step('room', tokens, new_lengths)

    def append(self, k: Mat, v: Mat, tokens: int, new_lengths=None) -> None:
        """This layer's rows of the open step behind its valid ones: the two row copies of ``KVCache.append`` and nothing else."""
        _, n, at, lens = self._open_step('append', tokens, new_lengths)
        if self._appended == self._parent._serial:
            raise RuntimeError(f'KVLayerView.append: layer {self.index} was appended to in this step already')
        if lens is not None:
            lens = self._parent._device_lengths(self.lengths, n)[:2]           # the step's upload, found again
        for src, dst in ((k, self.k), (v, self.v)):
            kv_append(src, dst.ptr, self.layout(dst), self.batch, tokens, at, lens, int(n.sum()))
        self._appended = self._parent._serial

    def append_rotated(self, qkv: Mat, heads: int, tokens: int, new_lengths=None, table: Optional[RopeTable] = None) -> None:
        """``KVCache.append_rotated`` for this layer's rows of the open step: one launch."""
        _, n, at, lens = self._open_step('append', tokens, new_lengths)
        if self._appended == self._parent._serial:
            raise RuntimeError(f'KVLayerView.append: layer {self.index} was appended to in this step already')
        if lens is not None:
            lens = self._parent._device_lengths(self.lengths, n)[:2]
        rope_kv_append(qkv, self.k.ptr, self.v.ptr, self.layout(self.k), self.batch, tokens, heads, self.kv_heads, self.key_dim, table,
                       at, lens, int(n.sum()))
        self._appended = self._parent._serial
