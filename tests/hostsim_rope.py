"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_prefill16.py's simulator plus the rotary position embedding entry point (npm_rope),
restated through tests/rope_reference.py ``rotate`` (the bitwise model of the kernel) with the argument checks of the entry
point.  ``ropes`` records the arguments of every call."""

import numpy as np

import hostsim_prefill16
import rope_reference as RR
from hostsim import _addr, _vec
from hostsim_varlen import _ints


class RopeHostSim(hostsim_prefill16.Prefill16HostSim):
    def __init__(self):
        super().__init__()
        self.ropes = []

    def npm_rope(self, x, pitch, batch, tokens, heads, head_dim, cos, sin, table_rows, at, at_lens, inverse):
        self.calls.append('npm_rope')
        self.ropes.append(dict(x=_addr(x), pitch=int(pitch), batch=batch, tokens=tokens, heads=heads, head_dim=head_dim,
                               table_rows=table_rows, at=at, at_lens=_addr(at_lens), inverse=int(inverse)))
        if not (_addr(x) and _addr(cos) and _addr(sin)):
            return 10002
        if min(batch, tokens, heads, table_rows) < 1 or head_dim < 2 or head_dim % 2 or pitch < heads * head_dim:
            return 10002
        if not _addr(at_lens) and (at < 0 or at + tokens > table_rows):
            return 10002
        half = head_dim // 2
        c, s = (_vec(t, table_rows * half).reshape(table_rows, half) for t in (cos, sin))
        rows = self._heads(x, pitch, batch, tokens, heads, head_dim)       # a writable [B, T, heads, D] view of the pitched rows
        start = _ints(at_lens, batch) if _addr(at_lens) else np.full(batch, at, dtype=np.int64)
        positions = start[:, None] + np.arange(tokens)[None, :]
        inside = (positions >= 0) & (positions < table_rows)               # rows outside the table are left untouched
        rotated = RR.rotate(np.ascontiguousarray(rows), np.where(inside, positions, 0), c, s, inverse=bool(inverse))
        rows[inside] = rotated[inside]
        return 0


def install():
    from np_modeling_amd import _C
    sim = RopeHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_prefill16.uninstall
