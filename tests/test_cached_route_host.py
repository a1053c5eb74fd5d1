"""CPU: ``layers.attentions.cached_route`` alone -- the precedence of the paths of a cached forward, one case per rule boundary,
on stand-in cache objects.  No simulator and no library: the three ``*_supported`` predicates of ``device`` are replaced by their
rules (head sizes Dk == Dv in {16, 32, 64, 128}; the decode kernel takes 1 .. 32 score rows per K / V head)."""

import types

import numpy as np
import pytest

HEADS, KV_HEADS = 4, 2                                                    # two score rows per token and K / V head


@pytest.fixture
def route(monkeypatch):
    from np_modeling_amd import device as D
    from np_modeling_amd.layers import attentions
    fused = lambda dk, dv=None: dk in (16, 32, 64, 128) and dv in (None, dk)
    monkeypatch.setattr(D, 'mha_decode_supported', lambda dk, rows, dv=None: fused(dk, dv) and 1 <= rows <= 32)
    monkeypatch.setattr(D, 'mha_prefill_supported', fused)
    monkeypatch.setattr(D, 'mha_core_supported', lambda dk, dv=None, any_math=False: fused(dk, dv))
    monkeypatch.setattr(D, 'PREFILL_KERNEL', False)
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', False)
    return attentions.cached_route


def _cache(length=40, dim=64, dtype='f32', window=None, prefix=0):
    """What ``cached_route`` reads of a cache; ``attend_prefix_rows`` must not be asked in the uniform form."""
    def attend_prefix_rows(n, causal):
        assert n is not None
        return prefix
    return types.SimpleNamespace(key_dim=dim, value_dim=dim, kv_heads=KV_HEADS, dtype=dtype, window=window, length=length,
                                 attend_prefix_rows=attend_prefix_rows)


def _n(tokens):
    return np.full([3], tokens, dtype=np.int64)


def _both(route, cache, tokens, causal=True, fresh_whole=False):
    """(uniform, per-sequence) paths of the same call."""
    return (route(cache, HEADS, tokens, causal, fresh_whole, False),
            route(cache, HEADS, tokens, causal, fresh_whole, True, _n(tokens)))


def test_rule_1_a_windowed_cache_takes_its_two_kernels_only(route, monkeypatch):
    from np_modeling_amd import device as D
    for dtype in ('f32', 'f16'):
        cache = _cache(window=8, dtype=dtype)
        assert route(cache, HEADS, 16, True, False, True, _n(16)) == 'decode'          # 32 rows
        assert route(cache, HEADS, 17, True, False, True, _n(17)) == 'prefill'         # 34: whatever the switches say (off)
        assert route(cache, HEADS, 16, True, True, True, _n(16)) == 'decode'           # a prefill from empty included
    with pytest.raises(ValueError, match='cannot be frozen'):
        route(_cache(window=8), HEADS, 1, False, False, True, _n(1))
    with pytest.raises(NotImplementedError, match='windowed cache needs'):
        route(_cache(window=8, dim=12), HEADS, 1, True, False, True, _n(1))
    monkeypatch.setattr(D, 'mha_prefill_supported', lambda *a: False)              # a split math mode
    with pytest.raises(ValueError):                                                  # the frozen refusal comes first
        route(_cache(window=8), HEADS, 1, False, False, True, _n(1))
    with pytest.raises(NotImplementedError):
        route(_cache(window=8), HEADS, 1, True, False, True, _n(1))


@pytest.mark.parametrize('dtype', ['f32', 'f16'])
def test_rule_2_decode_up_to_the_row_limit_and_uniform_only_within_the_length(route, dtype):
    cache = _cache(length=40, dtype=dtype)
    assert _both(route, cache, 16) == ('decode', 'decode')                           # 32 rows
    assert _both(route, cache, 17) == ('fused_masked', 'fused_masked')               # 33
    short = _cache(length=7, dtype=dtype)                                            # a frozen cache shorter than the query
    assert _both(route, short, 7, causal=False) == ('decode', 'decode')             # T == length
    assert _both(route, short, 8, causal=False) == ('fused_masked', 'decode')       # T == length + 1: the uniform kernel needs L >= T


def test_rule_2_a_uniform_f16_call_that_fails_it_never_takes_the_decode_kernel(route, monkeypatch):
    from np_modeling_amd import device as D
    short = _cache(length=7, dtype='f16')
    assert route(short, HEADS, 8, False, False, False) == 'fused_masked'             # 16 rows would suit the kernel
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', True)
    assert route(short, HEADS, 8, False, False, False) == 'prefill'


@pytest.mark.parametrize('dtype, own, other', [('f32', 'PREFILL_KERNEL', 'PREFILL_KERNEL_F16'), ('f16', 'PREFILL_KERNEL_F16', 'PREFILL_KERNEL')])
def test_rule_3_prefill_behind_the_switch_of_the_cache_type(route, monkeypatch, dtype, own, other):
    from np_modeling_amd import device as D
    cache = _cache(dtype=dtype)
    monkeypatch.setattr(D, other, True)
    assert _both(route, cache, 17) == ('fused_masked', 'fused_masked')               # the other type's switch says nothing
    monkeypatch.setattr(D, own, True)
    assert _both(route, cache, 17) == ('prefill', 'prefill')
    assert _both(route, cache, 16) == ('decode', 'decode')                           # the decode kernel still comes first
    monkeypatch.setattr(D, 'mha_prefill_supported', lambda *a: False)
    assert _both(route, cache, 17) == ('fused_masked', 'fused_masked')


def test_rule_3_exception_a_uniform_f32_prefill_from_empty_stays_on_the_fused_forward(route, monkeypatch):
    from np_modeling_amd import device as D
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    monkeypatch.setattr(D, 'PREFILL_KERNEL_F16', True)
    assert _both(route, _cache(length=40), 40, fresh_whole=True) == ('fused_masked', 'prefill')
    assert _both(route, _cache(length=40), 40, fresh_whole=False) == ('prefill', 'prefill')
    assert _both(route, _cache(length=40, dtype='f16'), 40, fresh_whole=True) == ('prefill', 'prefill')   # attended to as stored


def test_rules_4_and_5_the_gemm_composition_is_uniform_f32_only(route):
    assert route(_cache(dim=12), HEADS, 5, True, False, False) == 'gemm'
    assert route(_cache(dim=12), HEADS, 1, True, False, False) == 'gemm'
    assert route(_cache(dim=64), HEADS, 17, True, False, False) == 'fused_masked'
    # (_forward_cached refuses the per-sequence and f16 forms of such head sizes before the route is asked)
    assert route(_cache(dim=12), HEADS, 5, True, False, True, _n(5)) == 'fused_masked'
    assert route(_cache(dim=12, dtype='f16'), HEADS, 5, True, False, False) == 'fused_masked'


def test_rule_6_the_shared_suffix_is_per_sequence_decode_and_prefill(route, monkeypatch):
    from np_modeling_amd import device as D
    for prefix, suffix in ((0, ''), (64, '_shared')):
        cache = _cache(prefix=prefix)
        assert route(cache, HEADS, 1, True, False, True, _n(1)) == 'decode' + suffix
        assert route(cache, HEADS, 1, True, False, False) == 'decode'               # the uniform form never asks
        assert route(cache, HEADS, 17, True, False, True, _n(17)) == 'fused_masked'
    monkeypatch.setattr(D, 'PREFILL_KERNEL', True)
    assert route(_cache(prefix=64), HEADS, 17, True, False, True, _n(17)) == 'prefill_shared'
    assert route(_cache(prefix=0), HEADS, 17, True, False, True, _n(17)) == 'prefill'
    assert route(_cache(prefix=64, window=8), HEADS, 1, True, False, True, _n(1)) == 'decode'    # a window shares nothing


def test_the_decision_has_no_effects(route):
    cache = _cache()
    before = dict(vars(cache))
    for tokens in (1, 16, 17, 40):
        _both(route, cache, tokens, fresh_whole=tokens == 40)
    assert vars(cache) == before
