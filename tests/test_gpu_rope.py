"""GPU: rotary position embeddings -- npm_rope (csrc/npm_rope.hip) through the C ABI, bit for bit against the NumPy model of
tests/rope_reference.py, then ``MultiHeadAttention(rope_base=)``, ``TransformerDecoder`` / ``TransformerEncoder(rope_base=)`` and
incremental decoding against the float64 reference.  The checks are those of tests/rope_cases.py, which tests/test_rope_host.py
runs on the host simulator.

Bounds.  The kernel: none -- every product and every sum of the rotation is one fp32 rounding, so the result is compared as
uint32 with what NumPy computes from the same float32 tables.  Layers: BASELINE's 1e-4 in the metric of tests/conftest.py
``assert_close``.  Decoding: the bounds of the cached-layer tests (tests/test_gpu_decode.py, tests/test_gpu_kv16.py): 1e-5
(|ref| + max |ref|) against float64 -- for an fp16 cache float64 over the rows as stored -- and twice that between two float32
evaluations; the decoder's chunks at 1e-4 against float64.

Every test here needs ``npm_rope`` or ``rope_base``: none passes on the parent commit.
"""

import numpy as np
import pytest

import rope_cases as RC
import rope_reference as RR
from rope_cases import BASE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(scope='module')
def tables(npm):
    """cos / sin of 64 positions for every head size of the grid, on the host and on the device (made once)."""
    host = {d: RR.tables(64, d, BASE) for d in RC.VEC_DIMS + RC.SCALAR_DIMS}
    return host, {d: RC.device_tables(npm, t) for d, t in host.items()}


class _knob:
    def __init__(self, knob, value):
        self.knob, self.value = knob, value

    def _set(self, value):
        from np_modeling_amd import _C
        _C.check(_C.lib().npm_set_tuning(self.knob, int(value)), 'npm_set_tuning')

    def __enter__(self):
        self._set(self.value)

    def __exit__(self, *exc):
        self._set(0)                                                      # 0: the default
        return False


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
def test_kernel_bitwise_over_the_whole_grid(npm, tables):
    """D in {16, 32, 64, 128} (16-byte accesses) and {2, 6, 12, 20} (the scalar kernel) x heads {1, 3, 10} x (B, T) in {(1, 1),
    (3, 5), (2, 17)} x a pitch of heads * D or with four more heads behind (which keep their sentinel) x at in {0, 35} or ragged
    (33, 0, 7) x forward and inverse: 864 calls, each compared as uint32, each with a guard region that keeps its sentinel."""
    host, dev = tables
    rng = np.random.default_rng(0)
    grid = RC.kernel_grid()
    assert len(grid) == 8 * 3 * 3 * 2 * 3 * 2
    for case in grid:
        RC.check_kernel_case(npm, rng, host, dev, *case)


@pytest.mark.parametrize('d,heads', [(64, 10), (16, 3)])
def test_a_misaligned_entry_takes_the_scalar_kernel_with_the_same_bits(npm, tables, d, heads):
    host, dev = tables
    x = RC.kernel_rows(np.random.default_rng(1), 2, 17, heads, d, 4)
    for inverse in (0, 1):
        aligned = RC.run_rope(npm, x, heads, d, host[d], 35, None, inverse, dev=dev[d])
        shifted = RC.run_rope(npm, x, heads, d, host[d], 35, None, inverse, offset=1, dev=dev[d])      # 4 bytes off 16
        want = RC.expected_rows(x, heads, d, host[d], 35, None, inverse)
        assert np.array_equal(RC.bits(aligned), RC.bits(want)) and np.array_equal(RC.bits(shifted), RC.bits(want))
    odd_pitch = np.concatenate([x, np.full([2, 17, 2], np.float32(5.5))], axis=2)                       # pitch % 4 == 2
    got = RC.run_rope(npm, odd_pitch, heads, d, host[d], 0, [33, 7], 0, dev=dev[d])
    assert np.array_equal(RC.bits(got), RC.bits(RC.expected_rows(odd_pitch, heads, d, host[d], 0, [33, 7], 0)))


@pytest.mark.parametrize('d', [64, 12])
def test_grid_stride_loop_above_the_grid_cap(npm, tables, d):
    """NPM_TUNE_EW_GRID_CAP 2: 512 lanes walk 2720 vector items (D 64) or 2040 pairs (D 12) in a grid-stride loop; 1: one block."""
    host, dev = tables
    x = RC.kernel_rows(np.random.default_rng(2), 2, 17, 10, d, 4)
    want = RC.expected_rows(x, 10, d, host[d], 0, [33, 7], 0)
    default = RC.run_rope(npm, x, 10, d, host[d], 0, [33, 7], 0, dev=dev[d])
    assert np.array_equal(RC.bits(default), RC.bits(want))
    for cap in (2, 1, 3):
        with _knob(RC.EW_GRID_CAP_KNOB, cap):
            capped = RC.run_rope(npm, x, 10, d, host[d], 0, [33, 7], 0, dev=dev[d])
        assert np.array_equal(RC.bits(capped), RC.bits(want)), cap


@pytest.mark.parametrize('d', [16, 6])
def test_positions_past_the_table_are_left_untouched(npm, tables, d):
    """Sequence 1 starts at 30 of a 32-row table and brings 5 rows: rows 2, 3 and 4 come back as they were, the others rotated;
    nothing past the table is read (the tables of this test end with their 32nd row)."""
    x = RC.kernel_rows(np.random.default_rng(3), 3, 5, 3, d, 4)
    short = tuple(np.ascontiguousarray(t[:32]) for t in RR.tables(32, d, BASE))
    for inverse in (0, 1):
        got = RC.run_rope(npm, x, 3, d, short, 0, [0, 30, 5], inverse)
        want = RC.expected_rows(x, 3, d, short, 0, [0, 30, 5], inverse)
        assert np.array_equal(RC.bits(got), RC.bits(want))
        assert np.array_equal(RC.bits(got[1, 2:]), RC.bits(x[1, 2:])) and not np.array_equal(RC.bits(got[1, :2]), RC.bits(x[1, :2]))
    # the rule is per row: a start of -1 leaves row 0 alone and rotates rows 1 .. 4 at positions 0 .. 3; a start of 40 leaves the
    # whole sequence alone; a start of 31 rotates row 0 only.  No fault.
    got = RC.run_rope(npm, x, 3, d, short, 0, [-1, 40, 31], 0)
    assert np.array_equal(RC.bits(got), RC.bits(RC.expected_rows(x, 3, d, short, 0, [-1, 40, 31], 0)))
    assert np.array_equal(RC.bits(got[0, 0]), RC.bits(x[0, 0])) and not np.array_equal(RC.bits(got[0, 1:]), RC.bits(x[0, 1:]))
    assert np.array_equal(RC.bits(got[1]), RC.bits(x[1])) and np.array_equal(RC.bits(got[2, 1:]), RC.bits(x[2, 1:]))
    assert not np.array_equal(RC.bits(got[2, 0]), RC.bits(x[2, 0]))


def test_the_same_call_twice_gives_the_same_bits(npm, tables):
    host, dev = tables
    x = RC.kernel_rows(np.random.default_rng(4), 3, 5, 10, 128, 4)
    runs = [RC.run_rope(npm, x, 10, 128, host[128], 0, [33, 0, 7], 0, dev=dev[128]) for _ in range(2)]
    assert np.array_equal(RC.bits(runs[0]), RC.bits(runs[1]))
    # forward twice is the rotation by twice the angle only approximately, but forward then inverse on the device is what NumPy gives
    from np_modeling_amd import _C, device as D
    buf = D.from_host(x)
    for inverse in (0, 1):
        _C.check(_C.lib().npm_rope(buf.ptr, x.shape[2], 3, 5, 10, 128, dev[128][0].ptr, dev[128][1].ptr, 64, 35, None, inverse), 'npm_rope')
    want = RC.expected_rows(RC.expected_rows(x, 10, 128, host[128], 35), 10, 128, host[128], 35, inverse=1)
    assert np.array_equal(RC.bits(buf.numpy()), RC.bits(want))


def test_bad_arguments_are_refused(npm, tables):
    from np_modeling_amd import _C, device as D
    host, dev = tables
    x = D.full([2 * 3 * 64 + RC.GUARD], RC.SENTINEL)
    cos, sin = dev[16]
    lib = _C.lib()

    def call(**kw):
        args = dict(x=x.ptr, pitch=64, batch=2, tokens=3, heads=4, head_dim=16, cos=cos.ptr, sin=sin.ptr, rows=8, at=0, lens=None, inverse=0)
        args.update(kw)
        return lib.npm_rope(*args.values())

    for bad in (dict(head_dim=15, pitch=60), dict(head_dim=0), dict(batch=0), dict(tokens=0), dict(heads=0), dict(rows=0), dict(batch=-1),
                dict(pitch=63), dict(x=None), dict(cos=None), dict(sin=None), dict(at=6), dict(at=-1)):
        assert call(**bad) == 10002, bad
        assert b'npm_rope' in lib.npm_last_error()
    np.testing.assert_array_equal(x.numpy(), RC.SENTINEL)                 # a refused call launches nothing
    assert call(at=5) == 0 and call(at=0, rows=3) == 0


# ---- layers -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f,heads,kv_heads', [(64, 4, 4), (64, 4, 2), (48, 4, 4), (48, 4, 2)])
def test_layer_forward_and_backward_against_float64(npm, f, heads, kv_heads):
    """B 2, S 9; head size 16 takes the fused core (and the 16-byte kernel), head size 12 the GEMM composition (and the scalar
    kernel), each with Hkv 4 and 2."""
    RC.check_layer(npm, f, heads, kv_heads, core=(f == 64))


def test_cross_call_with_different_lengths(npm):
    RC.check_cross(npm)


def test_layer_under_every_math_mode(npm, math_mode):
    """The rotation is exact fp32 element-wise work in every arithmetic of the matrix products (head size 12: the GEMM
    composition, which the split modes apply to)."""
    RC.check_layer(npm, 48, 4, 2)
    RC.check_layer(npm, 64, 4, 2)


@pytest.mark.parametrize('norm_first', [True, False])
def test_decoder_and_encoder_with_rope_base(npm, norm_first):
    RC.check_decoder(npm, norm_first)
    RC.check_encoder(npm, norm_first)


# ---- decoding -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16', 'ragged'])
def test_chunked_attention_equals_the_whole_causal_forward(npm, kind):
    RC.check_chunked_attention(npm, kind)


@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16', 'ragged'])
def test_chunked_decode_equals_the_whole_causal_forward(npm, kind):
    RC.check_chunked_decoder(npm, kind)


def test_release_then_admit_starts_at_position_zero(npm):
    RC.check_release_and_admit(npm)


@pytest.mark.parametrize('f16', [False, True])
def test_prefill_kernel_switches_see_rotated_rows(npm, monkeypatch, f16):
    monkeypatch.setattr(npm.device, 'PREFILL_KERNEL_F16' if f16 else 'PREFILL_KERNEL', True)
    RC.check_prefill_switch(npm, f16)
    from np_modeling_amd import _C
    assert _C.last_prefill_kernel().startswith('mha_prefill_kernel D=16 T=40') and _C.last_prefill_kernel().endswith(' kv=f16') == f16


# ---- the stored rows, the off switch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('kind', ['contiguous', 'paged', 'f16'])
def test_stored_rows_are_the_rotation_of_the_plain_rows_bit_for_bit(npm, kind, ragged):
    RC.check_stored_rows(npm, kind, ragged)


def test_rope_base_none_is_bitwise_the_layer_without_the_keyword(npm):
    RC.check_off_switch(npm)
