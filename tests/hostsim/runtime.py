"""TEST INFRASTRUCTURE ONLY -- the runtime of the simulated library: memory, copies, events, knobs, and what they record.

* ``calls`` lists the compute entry points in call order; npm_h2d, npm_d2d and npm_d2h are not part of it (tests compare those
  lists between libraries), their byte counts go to ``uploads``, ``copies`` and ``d2h``.  npm_fill_f64 is not part of it either:
  ``fills64`` lists (len(calls) at the time, n) of every one, so that a test can put them back in their place.
* ``live`` / ``peak`` count the bytes of device memory in use now / at most since a test last set ``peak = live``.
* ``decode_splits`` / ``prefix_splits`` are NPM_TUNE_DECODE_SPLITS (knob 20) and NPM_TUNE_PREFIX_SPLITS (knob 24)."""

import ctypes as C

import numpy as np

from .memory import BAD, _addr, _deref, _vec

PREFIX_MAX_SPLITS = 1024


class Runtime:
    def __init__(self):
        super().__init__()
        self._blocks, self._sizes = {}, {}
        self._err = b''
        self.calls, self.uploads, self.copies, self.d2h, self.fills64 = [], [], [], [], []
        self.live = self.peak = 0
        self.decode_splits = self.prefix_splits = 0
        self.math = 0

    def npm_abi_version(self):
        return 2

    def npm_last_error(self):
        return self._err

    def npm_init(self, device):
        return 0

    def npm_shutdown(self):
        return 0

    def npm_sync(self):
        return 0

    def npm_stream(self):
        return 0

    def npm_malloc(self, out, nbytes):
        buf = np.empty(max(int(nbytes), 4) // 4 + 4, dtype=np.float32)
        buf.fill(np.nan)                                   # poison: catches reads of unwritten memory
        addr = (buf.ctypes.data + 15) // 16 * 16
        self._blocks[addr] = buf
        self._sizes[addr] = int(nbytes)
        self.live += int(nbytes)
        self.peak = max(self.peak, self.live)
        _deref(out).value = addr
        return 0

    def npm_free(self, ptr):
        self._blocks.pop(_addr(ptr), None)
        self.live -= self._sizes.pop(_addr(ptr), 0)
        return 0

    def npm_pool_stats(self, a, b):
        _deref(a).value = sum(v.nbytes for v in self._blocks.values())
        _deref(b).value = _deref(a).value
        return 0

    def npm_pool_trim(self):
        return 0

    def _copy(self, record, dst, src, nbytes):
        record.append(int(nbytes))
        C.memmove(_addr(dst), _addr(src), int(nbytes))
        return 0

    def npm_h2d(self, dst, src, nbytes):
        return self._copy(self.uploads, dst, src, nbytes)

    def npm_d2h(self, dst, src, nbytes):
        return self._copy(self.d2h, dst, src, nbytes)

    def npm_d2d(self, dst, src, nbytes):
        return self._copy(self.copies, dst, src, nbytes)

    def npm_fill_f32(self, dst, value, n):
        _vec(dst, n)[:] = value
        return 0

    def npm_fill_f64(self, dst, value, n):
        self.fills64.append((len(self.calls), int(n)))
        if int(n) == 0:
            return 0
        if not _addr(dst):
            return BAD
        if value != 0.0:
            return 10003                                    # only 0.0 is supported
        np.ctypeslib.as_array((C.c_double * int(n)).from_address(_addr(dst)))[:] = value
        return 0

    def npm_event_create(self, out):
        _deref(out).value = 1
        return 0

    def npm_event_destroy(self, ev):
        return 0

    npm_event_record = npm_event_sync = npm_event_destroy

    def npm_event_elapsed_ms(self, a, b, out):
        _deref(out).value = 0.0
        return 0

    def npm_set_math(self, mode):
        self.math = int(mode)
        return 0

    def npm_get_math(self):
        return self.math

    def npm_last_math(self):
        return 0

    def npm_set_tuning(self, knob, value):
        if knob == 20:
            self.decode_splits = int(value)
        if knob == 24:
            if not 0 <= value <= PREFIX_MAX_SPLITS:
                return BAD
            self.prefix_splits = int(value)
        return 0
