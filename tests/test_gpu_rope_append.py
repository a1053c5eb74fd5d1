"""GPU: npm_rope_kv_append (csrc/npm_rope_append.hip) through the C ABI against the three launches it fuses, with no tolerance.

Two identical packed projections and two identical pairs of sentinel-filled K / V pools (the pattern of tests/decode_gpu.py): one goes
through npm_rope and the existing appends (npm_kv_append / _varlen / _paged / _f16), one through the fused call.  The whole packed
buffer -- row padding and a guard region behind it included -- and the whole K and V pools must be equal as raw bits, and the
kernel-name string names the instance.  Where the yardstick refuses a call (an fp16 cache row that is no multiple of 8 halves, a
scalar ``at`` outside the table) the fused call refuses it with the same code and writes nothing.

B 3; T 1 and 5; D 16, 64, 128 (vector instance) and 12 (scalar); (H, Hkv) (4, 4), (4, 1), (6, 2); new_lens NULL and (5, 0, 2);
starts 0 and (14, 3, 31), so that a chunk crosses a 16-row page; a table that ends two rows behind the last start, so that a tail
runs off it; scalar-at / varlen / paged x f32 / f16 x rope / cos == NULL; a pitch wider than the row; a table base that is 4-byte
but not 16-byte aligned, which forces the scalar instance at D 16.  The entry point does not exist on the parent commit."""

import itertools

import numpy as np
import pytest

import rope_reference as RP

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 777.0, 256
B, CAP, PAGE = 3, 48, 16
STARTS = (14, 3, 31)
BAD = 10002


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


class Case:
    """One call: the packed buffer, the tables, the lengths and the geometry of the caches, all on the device once."""

    def __init__(self, D, d, heads, kv_heads, tokens, mode, f16, rope, starts, new_lens, pad, tight, table_offset=0):
        self.D, self.d, self.heads, self.kv_heads, self.tokens, self.mode, self.f16, self.rope = D, d, heads, kv_heads, tokens, mode, f16, rope
        rng = np.random.default_rng(d * 1000 + heads * 100 + tokens * 10 + pad)
        self.width = (heads + 2 * kv_heads) * d
        self.pitch = self.width + pad
        self.row = kv_heads * d
        host = np.full([B * tokens * self.pitch + GUARD], SENTINEL, dtype=np.float32)
        host[:B * tokens * self.pitch].reshape(B * tokens, self.pitch)[:, :self.width] = rng.standard_normal([B * tokens, self.width])
        self.x0 = host
        first = np.array(STARTS if starts else (0, 0, 0))
        self.at = int(first[0]) if mode == 'scalar' else 0
        # the table: wide enough, or (tight) ending two rows behind the last start so that the tail of that chunk runs off it
        self.table_rows = (self.at if mode == 'scalar' else int(first.max())) + 2 if tight else CAP
        cos, sin = RP.tables(self.table_rows, d, 10000.0)
        # ``table_offset`` floats in front of the table: a base that is 4-byte but not 16-byte aligned
        self.tables = [D.from_host(np.concatenate([np.zeros(table_offset, dtype=np.float32), t.ravel()])) for t in (cos, sin)]
        self.cos, self.sin = ((t.ptr + 4 * table_offset) if rope else None for t in self.tables)
        self.ints = D.bytes_from_host(np.concatenate([first, np.minimum(new_lens, tokens) if new_lens is not None else np.zeros(B, dtype=np.int64)]).astype(np.int32))
        self.at_lens = None if mode == 'scalar' else self.ints.ptr
        self.new_lens = self.ints.ptr + 4 * B if new_lens is not None and mode != 'scalar' else None
        self.table_host = rng.permutation(9).reshape(B, 3).astype(np.int32)
        self.table = D.bytes_from_host(self.table_host)
        dtype = np.float16 if f16 else np.float32
        self.pool0 = np.full([10 * PAGE * self.row + GUARD], SENTINEL, dtype=dtype)
        self.size = np.dtype(dtype).itemsize
        self.stride = PAGE * self.row if mode == 'paged' else CAP * self.row
        self.vec = int(d % 8 == 0 and not (rope and table_offset % 4))

    def fresh(self):
        D = self.D
        return D.from_host(self.x0), D.bytes_from_host(self.pool0), D.bytes_from_host(self.pool0)

    def paging(self):
        return (self.table.ptr, 3, PAGE) if self.mode == 'paged' else (None, 0, 0)

    def three_launches(self, lib, x, k, v):
        """npm_rope on the first H + Hkv heads, then the append of this layout for the k and for the v heads; the first refusal."""
        if self.rope:
            rc = lib.npm_rope(x.ptr, self.pitch, B, self.tokens, self.heads + self.kv_heads, self.d, self.cos, self.sin, self.table_rows,
                              self.at, self.at_lens, 0)
            if rc:
                return rc
        for part, cache in ((self.heads * self.d, k), (self.heads * self.d + self.row, v)):
            src = x.ptr + 4 * part
            if self.f16:
                rc = lib.npm_kv_append_f16(src, self.pitch, cache.ptr, self.row, self.stride, B, self.tokens, self.row, self.at, self.at_lens,
                                           self.new_lens, *self.paging())
            elif self.mode == 'paged':
                rc = lib.npm_kv_append_paged(src, self.pitch, cache.ptr, self.row, self.stride, B, self.tokens, self.row, self.at_lens,
                                             self.new_lens, *self.paging())
            elif self.mode == 'varlen':
                rc = lib.npm_kv_append_varlen(src, self.pitch, cache.ptr, self.row, self.stride, B, self.tokens, self.row, self.at_lens,
                                              self.new_lens)
            else:
                rc = lib.npm_kv_append(src, self.pitch, cache.ptr, self.row, self.stride, B, self.tokens, self.row, self.at)
            if rc:
                return rc
        return 0

    def fused(self, lib, x, k, v):
        return lib.npm_rope_kv_append(x.ptr, self.pitch, B, self.tokens, self.heads, self.kv_heads, self.d, self.cos, self.sin,
                                      self.table_rows if self.rope else 0, self.at, self.at_lens, self.new_lens, k.ptr, v.ptr, self.row,
                                      self.stride, *self.paging(), int(self.f16))

    def name(self):
        return 'rope_kv_append_kernel D=%d vec=%d rope=%d varlen=%d paged=%d kv=%s' % (
            self.d, self.vec, self.rope, self.mode != 'scalar', PAGE if self.mode == 'paged' else 0, 'f16' if self.f16 else 'f32')


def _compare(npm, case, what):
    """Runs both paths on fresh copies; returns 'equal' or 'refused'."""
    from np_modeling_amd import _C
    lib = _C.lib()
    x_ref, k_ref, v_ref = case.fresh()
    x_got, k_got, v_got = case.fresh()
    rc_ref = case.three_launches(lib, x_ref, k_ref, v_ref)
    rc_got = case.fused(lib, x_got, k_got, v_got)
    assert rc_got == rc_ref, (what, rc_got, rc_ref, _C.lib().npm_last_error())
    if rc_ref:
        assert rc_ref == BAD, (what, rc_ref)
        x_ref, k_ref, v_ref = case.fresh()                       # a refused call writes nothing
    else:
        assert lib.npm_last_rope_append_kernel().decode() == case.name(), what
    assert x_got.numpy().tobytes() == x_ref.numpy().tobytes(), f'{what}: the packed buffer differs'
    assert k_got.numpy().tobytes() == k_ref.numpy().tobytes(), f'{what}: the K pool differs'
    assert v_got.numpy().tobytes() == v_ref.numpy().tobytes(), f'{what}: the V pool differs'
    return 'refused' if rc_ref else 'equal'


def _grid(tokens):
    """(mode, f16, rope, starts, new_lens, pad, tight) of every call at ``tokens`` rows per sequence."""
    for mode, f16, rope, starts, lens, pad in itertools.product(('scalar', 'varlen', 'paged'), (False, True), (True, False), (False, True),
                                                                (None, (5, 0, 2)), (0, 8)):
        if mode == 'scalar' and lens is not None:
            continue                                             # the uniform append has no new_lens
        yield mode, f16, rope, starts, None if lens is None else np.array(lens), pad, False
    for mode, f16 in itertools.product(('varlen', 'paged'), (False, True)):
        yield mode, f16, True, True, np.array((5, 0, 2)), 0, True   # the tail of the last chunk runs off the table
    yield 'scalar', False, True, True, None, 0, True              # a scalar ``at`` whose chunk leaves the table: both refuse at T 5


@pytest.mark.parametrize('tokens', [1, 5])
@pytest.mark.parametrize('heads,kv_heads', [(4, 4), (4, 1), (6, 2)])
@pytest.mark.parametrize('d', [16, 64, 128, 12])
def test_the_fused_call_leaves_the_bits_of_the_three_launches(npm, d, heads, kv_heads, tokens):
    from np_modeling_amd import device as D
    outcomes = {'equal': 0, 'refused': 0}
    for mode, f16, rope, starts, lens, pad, tight in _grid(tokens):
        case = Case(D, d, heads, kv_heads, tokens, mode, f16, rope, starts, lens, pad, tight)
        what = f'D{d} H{heads}/{kv_heads} T{tokens} {mode} f16={f16} rope={rope} starts={starts} new_lens={None if lens is None else lens.tolist()} pad={pad} tight={tight}'
        outcome = _compare(npm, case, what)
        refusable = (f16 and (kv_heads * d) % 8 != 0) or (tight and mode == 'scalar' and tokens > 2)
        assert (outcome == 'refused') == refusable, what
        outcomes[outcome] += 1
    print(f'D{d} H{heads}/{kv_heads} T{tokens}: {outcomes}')
    assert outcomes['equal'] >= 40


def test_a_table_base_that_is_not_16_byte_aligned_takes_the_scalar_instance_with_the_same_bits(npm):
    from np_modeling_amd import device as D
    for mode, f16 in itertools.product(('scalar', 'varlen', 'paged'), (False, True)):
        case = Case(D, 16, 4, 1 if not f16 else 2, 5, mode, f16, True, True, None if mode == 'scalar' else np.array((5, 0, 2)), 8, False,
                    table_offset=1)
        assert case.vec == 0 and case.cos % 16 == 4
        assert _compare(npm, case, f'misaligned tables {mode} f16={f16}') == 'equal'


def test_argument_errors_are_those_of_the_calls_it_fuses(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    case = Case(D, 16, 4, 2, 5, 'paged', False, True, True, np.array((5, 0, 2)), 0, False)
    x, k, v = case.fresh()
    ok = dict(qkv=x.ptr, pitch=case.pitch, batch=B, tokens=5, heads=4, kv_heads=2, head_dim=16, cos=case.cos, sin=case.sin,
              table_rows=case.table_rows, at=0, at_lens=case.at_lens, new_lens=case.new_lens, k=k.ptr, v=v.ptr, cache_pitch=case.row,
              cache_stride=case.stride, table=case.table.ptr, table_pitch=3, page_rows=PAGE, f16=0)
    assert lib.npm_rope_kv_append(*ok.values()) == 0
    for change in (dict(qkv=None), dict(sin=None), dict(k=None), dict(v=None), dict(at_lens=None), dict(page_rows=24), dict(page_rows=8),
                   dict(table_pitch=-1), dict(pitch=case.width - 4), dict(pitch=case.width + 2), dict(head_dim=15), dict(heads=0),
                   dict(kv_heads=0), dict(batch=0), dict(tokens=0), dict(batch=-1), dict(table_rows=0), dict(cache_pitch=case.row - 4),
                   dict(cache_pitch=case.row + 2), dict(cache_stride=case.stride - 4), dict(qkv='+4'), dict(k='+4'),
                   dict(f16=1, cache_pitch=case.row + 4)):
        x, k, v = case.fresh()
        args = {**ok, 'qkv': x.ptr, 'k': k.ptr, 'v': v.ptr}
        args.update({key: args[key] + 4 if value == '+4' else value for key, value in change.items()})      # '+4': 4 bytes off
        assert lib.npm_rope_kv_append(*args.values()) == BAD, change
        assert x.numpy().tobytes() == case.x0.tobytes() and k.numpy().tobytes() == case.pool0.tobytes() and \
            v.numpy().tobytes() == case.pool0.tobytes(), change
    # no tables: an empty call is NPM_OK and launches nothing, as the appends have it; the paged preconditions still hold
    x, k, v = case.fresh()
    quiet = {**ok, 'qkv': x.ptr, 'k': k.ptr, 'v': v.ptr, 'cos': None, 'sin': None}
    assert lib.npm_rope_kv_append(*{**quiet, 'batch': 0}.values()) == 0 and lib.npm_rope_kv_append(*{**quiet, 'tokens': 0}.values()) == 0
    assert lib.npm_rope_kv_append(*{**quiet, 'batch': 0, 'at_lens': None}.values()) == BAD
    assert x.numpy().tobytes() == case.x0.tobytes() and k.numpy().tobytes() == case.pool0.tobytes()
