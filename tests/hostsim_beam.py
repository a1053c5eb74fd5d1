"""TEST INFRASTRUCTURE ONLY -- tests/hostsim_spec.py's simulator (through tests/hostsim_prefix.py, whose npm_kv_copy_pages the
copy-on-write behind a ``reorder`` calls, and beside tests/hostsim_rope.py's npm_rope) plus npm_beam_step, restated through
tests/beam_reference.py with the argument checks of the entry point.  General rows take NumPy's float32 exponential (``sample_reference.weights32``), as the
simulated sampler does: the contract's steps, not the device's last bit.  Dead rows are not read, and the workspace is filled
with a pattern, as memory whose contents are unspecified.  ``beams`` records the arguments of every call."""

import ctypes as C

import numpy as np

import beam_reference as BR
import hostsim_prefix
import hostsim_rope
from hostsim import _addr, _deref, _vec
from hostsim_sample import _words

BAD = 10002


class BeamHostSim(hostsim_prefix.PrefixHostSim, hostsim_rope.RopeHostSim):
    def __init__(self):
        super().__init__()
        self.beams = []

    def npm_beam_step(self, sref):
        self.calls.append('npm_beam_step')
        if sref is None:
            return BAD
        s = _deref(sref)
        self.beams.append(dict(groups=s.groups, width=s.width, vocab=s.vocab, pitch=s.pitch, eos=s.eos))
        if s.groups < 1 or not 1 <= s.width <= 32 or not 1 <= s.vocab <= (1 << 20) or s.pitch < s.vocab:
            return BAD
        if s.groups * s.width * 2 * s.width >= 2 ** 31:
            return BAD
        if not all(_addr(p) for p in (s.logits, s.cum, s.lse, s.parent, s.ids, s.cand_slot, s.cand_token, s.cand_score, s.workspace)):
            return BAD
        need = 4 * s.groups * s.width * (1 + 4 * s.width)
        if s.workspace_bytes < need or _addr(s.workspace) % 4:
            return BAD
        n, cands = s.groups * s.width, 2 * s.width
        cum = _words(s.cum, n, C.c_float)
        # rows one at a time: a dead row's memory is never touched
        rows = {r: _vec(_addr(s.logits) + 4 * r * s.pitch, s.vocab) for r in range(n) if BR.live(cum[r])}
        out = BR.step(rows, cum, s.groups, s.width, s.eos)
        _words(s.workspace, need // 4, C.c_int32)[:] = 0x5A5A5A5A
        _words(s.cand_slot, s.groups * cands, C.c_int32)[:] = out['cand_slot'].ravel()
        _words(s.cand_token, s.groups * cands, C.c_int32)[:] = out['cand_token'].ravel()
        _words(s.cand_score, s.groups * cands, C.c_float)[:] = out['cand_score'].ravel()
        _words(s.parent, n, C.c_int32)[:] = out['parent']
        _words(s.ids, n, C.c_int32)[:] = out['ids']
        _words(s.lse, n, C.c_float)[:] = out['lse']
        cum[:] = out['cum']
        return 0

    def npm_last_beam_kernel(self):
        return b'hostsim npm_beam_step' if self.beams else b''


def install():
    from np_modeling_amd import _C
    sim = BeamHostSim()
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


uninstall = hostsim_prefix.uninstall
