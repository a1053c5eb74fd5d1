"""GPU: ``norm='rms'`` / ``ffn='swiglu'`` through TransformerEncoder and TransformerDecoder at B 2, S 8, F 32, 2 heads, U 48
(tests/llama_cases.py): the fused and the literal composition against each other and against the float64 restatement of
tests/llama_reference.py -- output, input gradients, every parameter after one SGD step -- under the header's NPM_PARITY_REL_F32 /
NPM_PARITY_SCALED_F32 as tests/test_gpu_parity.py reads them (scaled error over all elements, relative error where |ref| >= 0.1 max
|ref|); then decoding: chunks against ``forward``, half weights beside a paged fp16 cache, one speculative loop."""

import numpy as np
import pytest

import decode_cases as DC
import llama_cases as LC
import spec_cases as XC
from test_gpu_decode import LAYER_TOL, _layer_close
from test_gpu_w16 import SIX, _rounded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.fixture(scope='module')
def bounds():
    from np_modeling_amd import _C
    return _C.parity_bounds()['f32']


def _within(label, got, ref, bounds, worst):
    rel, scaled = bounds
    fs, fr = LC.parity(got, ref, rel, scaled)
    worst[label] = max(fs, fr)
    assert fs <= 1.0 and fr <= 1.0, f'{label}: {fs:.3g} of the scaled bound, {fr:.3g} of the relative bound'


def _check_run(run, other, bounds, what):
    """``run`` against the restatement and against ``other`` (the other composition of the same layer, inputs and step)."""
    worst = {}
    tensors = [('out', 'out', 'ref_out'), ('dx', 'dx', 'ref_dx')] + ([('dkv', 'dkv', 'ref_dkv')] if run['dkv'] is not None else [])
    for label, got, ref in tensors:
        _within(label, run[got], run[ref], bounds, worst)
        if other is not None:
            _within(label + ' fused/literal', run[got], other[got], bounds, worst)
    for name in run['start']:
        _within(name, run['params'][name], run['ref_params'][name], bounds, worst)
        if other is not None:
            _within(name + ' fused/literal', run['params'][name], other['params'][name], bounds, worst)
        if not name.endswith('.bk'):            # dbk is zero in real arithmetic (every row of datt sums to 0): nothing to be relative to
            # the step as a gradient: SCALED on the gradient's scale plus the rounding of the update itself, 2 u max |p| / lr
            g = (run['start'][name] - run['params'][name]) / LC.LR_STEP
            ref_g = run['ref_grads'][name]
            bound = bounds[1] * np.abs(ref_g).max() + 2 * 2.0 ** -24 * np.abs(run['start'][name]).max() / LC.LR_STEP
            worst['d' + name] = float(np.abs(g - ref_g).max() / bound)
            assert worst['d' + name] <= 1.0, f'gradient of {name}: {worst["d" + name]:.3g} of its bound'
    top = max(worst, key=worst.get)
    print(f'{what}: worst {worst[top]:.3f} of its bound ({top})')


@pytest.mark.parametrize('norm_first', [True, False], ids=['pre', 'post'])
@pytest.mark.parametrize('kind', ['encoder', 'decoder'])
def test_fused_and_literal_compositions_against_float64(npm, bounds, kind, norm_first):
    fused = LC.run_block(npm, kind, norm_first)
    literal = LC.run_block(npm, kind, norm_first, literal=True)
    assert fused['layer']._fused and fused['scope']['update_launches'] == 1 and literal['scope']['update_launches'] == 1
    assert len(fused['start']) == (14 if kind == 'encoder' else 23)
    _check_run(fused, literal, bounds, f'{kind} {"pre" if norm_first else "post"} rms swiglu fused')
    _check_run(literal, None, bounds, f'{kind} {"pre" if norm_first else "post"} rms swiglu literal')


@pytest.mark.parametrize('norm,ffn,norm_first', [('rms', 'relu', True), ('layer', 'swiglu', False)])
@pytest.mark.parametrize('kind', ['encoder', 'decoder'])
def test_mixed_pairs(npm, bounds, kind, norm, ffn, norm_first):
    fused = LC.run_block(npm, kind, norm_first, norm=norm, ffn=ffn)
    literal = LC.run_block(npm, kind, norm_first, norm=norm, ffn=ffn, literal=True)
    assert fused['layer']._fused and fused['scope']['update_launches'] == 1
    _check_run(fused, literal, bounds, f'{kind} {norm} {ffn} fused')


@pytest.mark.parametrize('kind', ['encoder', 'decoder'])
def test_rms_with_dropout_runs_and_equals_the_restatement_given_its_masks(npm, bounds, kind):
    run = LC.run_block(npm, kind, True, drop=0.25)
    assert not run['layer']._fused                                        # the literal composition: a DropOut of its own
    worst = {}
    _within('out', run['out'], run['ref_out'], bounds, worst)
    _within('dx', run['dx'], run['ref_dx'], bounds, worst)
    print(f'{kind} rms swiglu drop 0.25: {worst}')


# ---- decoding -----------------------------------------------------------------------------------------------------------------
def _decoder(npm, norm_first, seed=9, hidden=LC.U):
    np.random.seed(seed)
    dec = npm.layers.TransformerDecoder(num_heads=LC.HEADS, hidden_units=hidden, norm_first=norm_first, causal=True, norm='rms',
                                        ffn='swiglu')
    dec(np.zeros([LC.B, 2, LC.F], dtype=np.float32), np.zeros([LC.B, LC.SKV, LC.F], dtype=np.float32))
    LC.tame(dec)
    return dec


def _decode_chunks(dec, q, kv, sizes, capacity, **kwargs):
    state = dec.start_decoding(kv, capacity, **kwargs)
    outs = [np.asarray(dec.decode(np.ascontiguousarray(piece), state)) for piece in DC.split(q, sizes)]
    assert state.position == sum(sizes)
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize('norm_first', [True, False], ids=['pre', 'post'])
def test_decode_in_chunks_equals_forward(npm, norm_first):
    dec = _decoder(npm, norm_first)
    q, kv = LC.inputs(10, [LC.B, LC.S, LC.F], [LC.B, LC.SKV, LC.F])
    whole = np.asarray(dec(q, kv))
    with npm.device.KernelTimer() as timer:
        got = _decode_chunks(dec, q, kv, LC.CHUNKS, capacity=LC.S + 3)
    names = set(timer.summary())
    assert {'rmsnorm_fwd', 'swiglu_fwd', 'sgemm_skinny_NN'} <= names and not names & {'layernorm_fwd', 'relu_fwd', 'sgemm_NN'}, names
    _layer_close(got, whole, 2 * LAYER_TOL, f'rms swiglu decode chunks {LC.CHUNKS} vs forward')


@pytest.mark.parametrize('norm_first', [True, False], ids=['pre', 'post'])
def test_half_weights_beside_a_paged_fp16_cache(npm, norm_first):
    """``weights='f16'`` is the decoder whose six matrices -- the packed gate | up matrix in dense1's place -- are the rounded ones."""
    dec, twin = _decoder(npm, norm_first), _decoder(npm, norm_first)
    for path, attr in SIX:
        arr = getattr(DC.sub(twin, path), attr)
        arr.set(_rounded(np.asarray(arr)))
    q, kv = LC.inputs(12, [LC.B, LC.S, LC.F], [LC.B, LC.SKV, LC.F])
    kwargs = dict(cache_dtype='f16', page_size=16)
    with npm.device.KernelTimer() as timer:
        got = _decode_chunks(dec, q, kv, LC.CHUNKS, capacity=16, weights='f16', **kwargs)
    names = set(timer.summary())
    assert {'sgemm_skinny_w16_NN', 'swiglu_fwd', 'rmsnorm_fwd'} <= names and 'cvt_f16_f32' not in names, names
    want = _decode_chunks(twin, q, kv, LC.CHUNKS, capacity=16, **kwargs)
    print('half weights vs twin: bits equal' if np.array_equal(got.view(np.uint32), want.view(np.uint32)) else 'half weights vs twin: bits differ')
    _layer_close(got, want, 2 * LAYER_TOL, 'rms swiglu decode with half weights vs the decoder holding the rounded matrices')
    lin1 = dec._dense1._linear
    halves = dec.start_decoding(kv, 16, weights='f16').weights.numpy(lin1, '_w')
    assert halves.shape == (LC.F, 2 * LC.U) and np.array_equal(halves, np.asarray(lin1._w).astype(np.float16))


def test_a_speculative_loop_emits_the_tokens_of_the_one_token_loop(npm):
    """tests/test_gpu_spec.py's end-to-end fixture with the rms / swiglu decoder in the default one's place: admit, truncate and
    ``speculative.decode_step`` need no change."""
    _, emb, head, kv, prompts = XC.make_model(npm)
    np.random.seed(XC.SEED)
    dec = npm.layers.TransformerDecoder(num_heads=XC.HEADS, hidden_units=XC.HIDDEN, norm_first=True, num_kv_heads=XC.HEADS, causal=True,
                                        norm='rms', ffn='swiglu')
    dec(np.zeros([3, 2, XC.F], dtype=np.float32), np.zeros([3, 7, XC.F], dtype=np.float32))
    for path, attrs in (('_self_attention', ('_wq', '_wk', '_wv', '_wo')), ('_cross_attention', ('_wq', '_wk', '_wv', '_wo')),
                        ('_dense1._linear', ('_w',)), ('_dense2', ('_w',))):
        for attr in attrs:
            arr = getattr(DC.sub(dec, path), attr)
            arr.set(np.asarray(arr) * np.float32(2.0 / np.sqrt(XC.F)))
    model = (dec, emb, head, kv, prompts)
    want, logits, pages, lengths = XC.plain(npm, model, npm.sampling.Sampler(3))
    gap = XC.least_gap(logits)
    print(f'speculative rms swiglu: least top-2 gap of the plain run {gap:.3e} of max |logit|')
    assert gap >= XC.GAP, 'the fixture has a near-tie: chunked and single-step logits may pick different tokens'
    sampler = npm.sampling.Sampler(3)
    got, log, state, _ = XC.speculative(npm, model, sampler)
    assert [g[:XC.EMIT] for g in got] == want and np.array(want).shape == (3, XC.EMIT)
    accepted, rejected = XC.accepts_and_rejects(log)
    print(f'speculative rms swiglu: {len(log)} steps, slot-steps accepting {accepted}, rejecting {rejected}')
    assert accepted >= 1 and rejected >= 1 and len(log) < XC.EMIT - 1               # as on the host simulator: 8 steps, 9 and 1
    emitted = np.array([len(g) for g in got])
    state.truncate(emitted - XC.EMIT)
    assert state.positions.tolist() == lengths.tolist() and state.self_cache.pages_in_use == pages


def test_constructor_errors(npm):
    for cls, extra in ((npm.layers.TransformerEncoder, {}), (npm.layers.TransformerDecoder, {'causal': True})):
        with pytest.raises(ValueError, match='norm'):
            cls(2, 48, True, norm='foo', **extra)
        with pytest.raises(ValueError, match='ffn'):
            cls(2, 48, True, ffn='foo', **extra)
