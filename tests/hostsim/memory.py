"""TEST INFRASTRUCTURE ONLY -- views of the simulator's "device" memory.  A device pointer is the address of host memory; every
view below is writable and shares that memory."""

import ctypes as C

import numpy as np

BAD, UNSUPPORTED = 10002, 10003          # NPM_E_BAD_ARGUMENT, NPM_E_UNSUPPORTED


def _deref(arg):
    return arg._obj if hasattr(arg, '_obj') else arg


def _addr(p):
    if p is None:
        return 0
    if isinstance(p, int):
        return p
    v = getattr(p, 'value', None)
    return int(v) if v else 0


def _words(ptr, n, ctype):
    return np.ctypeslib.as_array((ctype * int(n)).from_address(_addr(ptr)))


def _ints(ptr, n):
    """n int32 at ``ptr``, as an int64 copy."""
    return _words(ptr, n, C.c_int32).astype(np.int64)


def _vec(ptr, n):
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    return _words(ptr, n, C.c_float)


def _pitched(ptr, rows, cols, ld, ctype, dtype):
    rows, cols, ld = int(rows), int(cols), int(ld)
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols), dtype=dtype)
    flat = _words(ptr, (rows - 1) * ld + cols, ctype).view(dtype)
    return np.lib.stride_tricks.as_strided(flat, shape=(rows, cols), strides=(flat.itemsize * ld, flat.itemsize))


def _mat(ptr, rows, cols, ld):
    """[rows, cols] float32 view with a row pitch of ``ld`` floats."""
    return _pitched(ptr, rows, cols, ld, C.c_float, np.float32)


def _half_rows(ptr, rows, cols, ld):
    """[rows, cols] float16 view with a row pitch of ``ld`` halves."""
    return _pitched(ptr, rows, cols, ld, C.c_uint16, np.float16)


def _heads(ptr, pitch, b, s, h, d):
    """[B, S, H, D] view of a pitched operand."""
    flat = _vec(ptr, ((b * s - 1) * pitch + h * d) if b * s else 0)
    return np.lib.stride_tricks.as_strided(flat, shape=(b, s, h, d), strides=(4 * s * pitch, 4 * pitch, 4 * d, 4))


def _page_ok(page_rows):
    return page_rows >= 16 and page_rows & (page_rows - 1) == 0
