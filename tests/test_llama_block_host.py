"""CPU: ``norm='rms'`` / ``ffn='swiglu'`` through TransformerEncoder and TransformerDecoder on the host simulator (tests/hostsim/;
the four entry points join it with the profile 'llama'): results against tests/llama_reference.py,
the entry points called, one optimizer launch and one bucket per backward, the decode route -- and the default-keyword layers
calling what they called before the keywords existed (tests/golden/llama_default_calls.json)."""

import json

import hostsim
import llama_cases as LC
import numpy as np
import pytest
import transformer_trace_cases as TC
from hostsim.fixtures import activate, deactivate


@pytest.fixture
def npm():
    """The shared fixture's simulator with a recorder of every call and its arguments in front of it."""
    from np_modeling_amd import _C
    package = activate()
    package.recorder = _C._LIB = TC.Recorder(package.sim)
    yield package
    deactivate()


def _names(npm):
    return [r[0] for r in npm.recorder.records]


KINDS = [(kind, pre, literal) for kind in ('encoder', 'decoder') for pre in (True, False) for literal in (False, True)]


@pytest.mark.parametrize('kind,norm_first,literal', KINDS)
def test_rms_swiglu_block_on_the_simulator(npm, kind, norm_first, literal):
    run = LC.run_block(npm, kind, norm_first, literal=literal)
    layer = run['layer']
    # the simulator computes in float64 and stores float32: a few roundings per tensor
    for label, got, ref in [('out', run['out'], run['ref_out']), ('dx', run['dx'], run['ref_dx'])] + \
            ([('dkv', run['dkv'], run['ref_dkv'])] if kind == 'decoder' else []) + \
            [(k, run['params'][k], run['ref_params'][k]) for k in run['start']]:
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6 * np.abs(ref).max(), err_msg=label)
    names = _names(npm)
    blocks = 2 if kind == 'encoder' else 3
    passes = 2                               # the forward that draws the parameters, then the run itself
    assert names.count('npm_rmsnorm_fwd') == passes * blocks
    assert names.count('npm_rmsnorm_bwd') == blocks
    assert names.count('npm_swiglu_fwd') == passes and names.count('npm_swiglu_bwd') == 1
    assert not [n for n in names if n.startswith(('npm_layernorm_', 'npm_relu_'))]
    assert ('npm_add' in names) == literal                                      # the fused composition has no standalone add
    # one bucket for all gradients, mirrored on one arena: one optimizer launch
    assert run['scope']['arena'] and run['scope']['update_launches'] == 1
    floats = sum(v.size for v in run['start'].values())
    attentions = blocks - 1                  # MultiHeadAttention._numel allows 4 floats of alignment for each of its 8 parameters
    assert layer._numel() == floats + 32 * attentions + layer._SLACK
    assert layer._arena.size == floats
    assert len(run['start']) == (14 if kind == 'encoder' else 23)


@pytest.mark.parametrize('kind', ['encoder', 'decoder'])
def test_one_range_is_exchanged_per_flush(npm, kind):
    """Two ranks: the gradients leave as ranges of ONE bucket that together cover every parameter's float once."""
    from np_modeling_amd import parallel
    comm = TC._TwoRanks()
    layer = LC.make(npm, kind, True, seed=5, norm='rms', ffn='swiglu')
    x, kv, dy = LC.inputs(6, [LC.B, LC.S, LC.F], [LC.B, LC.SKV, LC.F], [LC.B, LC.S, LC.F])
    args = (x,) if kind == 'encoder' else (x, kv)
    layer(*args)
    parallel.set_communicator(comm)
    layer(dy, backprop=True, optimizer_=npm.optimizer.SGDOptimizer(0.05))
    first = min(ptr for ptr, _ in comm.sent)
    spans = sorted(((ptr - first) // 4, size) for ptr, size in comm.sent)
    assert parallel.GradScope.last['collectives'] == len(spans) and parallel.GradScope.last['update_launches'] == 1
    end = 0
    for start, size in spans:                        # back to back (alignment gaps of at most 3 floats), no overlap
        assert end <= start <= end + 3
        end = start + size
    assert layer._arena.size <= end <= layer._numel()


@pytest.mark.parametrize('pair', [('rms', 'relu'), ('layer', 'swiglu')])
def test_mixed_pairs(npm, pair):
    norm, ffn = pair
    run = LC.run_block(npm, 'encoder', norm == 'rms', norm=norm, ffn=ffn)
    for label, got, ref in [('out', run['out'], run['ref_out']), ('dx', run['dx'], run['ref_dx'])] + \
            [(k, run['params'][k], run['ref_params'][k]) for k in run['start']]:
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-6 * np.abs(ref).max(), err_msg=label)
    names = _names(npm)
    assert ('npm_rmsnorm_fwd' in names) == (norm == 'rms') and ('npm_layernorm_fwd' in names) == (norm == 'layer')
    assert ('npm_swiglu_fwd' in names) == (ffn == 'swiglu')
    assert run['scope']['update_launches'] == 1


def test_rms_with_dropout_runs_the_literal_composition(npm):
    run = LC.run_block(npm, 'encoder', True, drop=0.25)
    assert not run['layer']._fused
    names = _names(npm)
    assert 'npm_mask_scale' in names and 'npm_rmsnorm_fwd' in names and 'npm_layernorm_dropout_fwd' not in names
    np.testing.assert_allclose(run['out'], run['ref_out'], rtol=2e-5, atol=2e-6 * np.abs(run['ref_out']).max())
    np.testing.assert_allclose(run['dx'], run['ref_dx'], rtol=2e-5, atol=2e-6 * np.abs(run['ref_dx']).max())
    with pytest.raises(ValueError, match='dropout'):
        npm.layers.RMSNormalization()._forward_impl(np.ones((2, 8), dtype=np.float32), npm.layers.DropOut(0.5))


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('weights', [None, 'f16'])
def test_decode_goes_skinny_gate_skinny_and_equals_forward(npm, norm_first, weights):
    dec = LC.make(npm, 'decoder', norm_first, seed=9, norm='rms', ffn='swiglu')
    x, kv = LC.inputs(10, [LC.B, LC.S, LC.F], [LC.B, LC.SKV, LC.F])
    dec(x, kv)
    LC.tame(dec)
    whole = np.asarray(dec(x, kv))
    state = dec.start_decoding(kv, 16, weights=weights)
    skinny = 'npm_sgemm_skinny_w16' if weights else 'npm_sgemm_skinny'
    at, rows = 0, []
    for t in LC.CHUNKS:
        seen = len(npm.recorder.records)
        rows.append(np.asarray(dec.decode(x[:, at:at + t], state)))
        at += t
        names = [r[0] for r in npm.recorder.records[seen:] if not r[0].endswith('_supported')]      # launches, not probes
        gate = names.index('npm_swiglu_fwd')
        assert names.count('npm_swiglu_fwd') == 1 and names[gate - 1] == skinny and names[gate + 1] == skinny        # M = B t <= 64
        assert names.count('npm_rmsnorm_fwd') == 3 and not [n for n in names if n.startswith(('npm_layernorm_', 'npm_relu_'))]
    got = np.concatenate(rows, axis=1)
    tol = 2e-5 if weights is None else 2e-2          # f16: the model whose six matrices are rounded; only its route is this test's
    np.testing.assert_allclose(got, whole, rtol=tol, atol=tol * np.abs(whole).max())
    if weights:
        lin1 = dec._dense1._linear
        assert state.weights.numpy(lin1, '_w').shape == (LC.F, 2 * LC.U)          # the packed matrix, in dense1's place
        np.testing.assert_array_equal(state.weights.numpy(lin1, '_w'), np.asarray(lin1._w).astype(np.float16))


def test_constructor_rejects_unknown_kinds(npm):
    for cls, extra in ((npm.layers.TransformerEncoder, {}), (npm.layers.TransformerDecoder, {'causal': True})):
        with pytest.raises(ValueError, match='norm'):
            cls(2, 48, True, norm='foo', **extra)
        with pytest.raises(ValueError, match='ffn'):
            cls(2, 48, True, ffn='foo', **extra)


def test_a_library_without_the_entry_points_is_an_error_that_names_them():
    from np_modeling_amd import _C, parallel
    import np_modeling_amd as package
    parallel.set_communicator(None)
    hostsim.install('xent')                          # the library from just before the feature: no npm_rmsnorm_*, no npm_swiglu_*
    try:
        x = np.ones((2, 8), dtype=np.float32)
        with pytest.raises(_C.NpmError, match='npm_rmsnorm_fwd'):
            package.layers.RMSNormalization()(x)
        with pytest.raises(_C.NpmError, match='npm_swiglu_fwd'):
            package.layers.GatedDense(4)(x)
    finally:
        hostsim.uninstall()


def test_default_keywords_call_what_they_called_before():
    with open(LC.GOLDEN) as f:
        want = json.load(f)
    assert LC.default_calls() == want
    assert set(want) == {'encoder pre', 'encoder post', 'decoder pre', 'decoder post'}
    called = {n for trace in want.values() for phase in trace.values() for n in phase}
    assert {'npm_layernorm_fwd', 'npm_layernorm_bwd', 'npm_sgemm_skinny'} <= called and not [n for n in called if 'rmsnorm' in n or 'swiglu' in n]
