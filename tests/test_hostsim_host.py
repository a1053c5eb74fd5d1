"""CPU: the host simulator itself (tests/hostsim/): what its profiles expose, how much of the C ABI it covers, how it is put
together, and one generation loop that needs the whole of it at once."""

import inspect
import json
import math
import os

import numpy as np

import decode_cases as DC
import hostsim
from hostsim.fixtures import npm_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS = (hostsim.Runtime, hostsim.Training, hostsim.KVCache, hostsim.Generation, hostsim.SkinnyGemm)

npm = npm_fixture()


def _exposed(sim):
    return sorted(name for name in dir(type(sim)) if name.startswith('npm_') and hasattr(sim, name))


def test_profiles_are_what_the_tower_of_simulators_was():
    """tests/golden/hostsim_profiles.json holds, per profile, ``sorted(n for n in dir(cls) if n.startswith('npm_'))`` of the
    simulator class of that name on the last commit that had one class per feature (HostSim as 'training', DecodeHostSim as
    'decode', ... LogitsHostSim as 'logits', SkinnyHostSim, W16HostSim), one profile a line.  The last four lines ('xent', 'llama',
    'lm', 'adamw') hold the same of the chain of wrappers that stood around the one class on the last commit that had them: the
    class's names and those of every wrapper up to the one that feature added.  A profile exposes exactly those names,
    ``hasattr`` is False for every other one, and the whole simulator exposes their union."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'hostsim_profiles.json')) as fh:
        recorded = json.load(fh)
    assert len(recorded) == 20 and set(recorded) == set(hostsim.PROFILES)
    try:
        for profile, names in recorded.items():
            sim = hostsim.install(profile)
            assert _exposed(sim) == names == sorted(hostsim.PROFILES[profile]), profile
            assert not any(hasattr(sim, name) for name in set().union(*recorded.values()) - set(names)), profile
        assert _exposed(hostsim.install()) == sorted(set().union(*recorded.values()))
    finally:
        hostsim.uninstall()
    assert len(recorded['logits']) == 99 and not (set(recorded['w16']) - set(recorded['paged'])) & set(recorded['logits'])
    assert len(recorded['adamw']) == 119


def test_coverage_of_the_abi_is_stated():
    from np_modeling_amd import _C
    simulated = set(_exposed(hostsim.HostSim()))
    assert set(hostsim.NOT_SIMULATED) == {'npm_debug_attn_trace', 'npm_debug_gemm_trace', 'npm_device_count', 'npm_device_name'}
    assert set(_C.SIGNATURES) - simulated == set(hostsim.NOT_SIMULATED) and len(hostsim.NOT_SIMULATED) == 4
    assert simulated - set(_C.SIGNATURES) == {
        'npm_abi_version', 'npm_last_error', 'npm_stream', 'npm_last_attn_kernel', 'npm_last_beam_kernel', 'npm_last_decode_kernel',
        'npm_last_draft_kernel', 'npm_last_logits_kernel', 'npm_last_prefill_kernel', 'npm_last_prefix_kernel',
        'npm_last_sample_kernel', 'npm_last_skinny_kernel', 'npm_last_xent_kernel', 'npm_last_rope_append_kernel'}


def test_one_class_of_parts_that_do_not_override_each_other():
    assert hostsim.HostSim.__bases__ == PARTS and not hostsim.HostSim.__subclasses__()
    assert {name for name in vars(hostsim.HostSim) if not name.startswith('__')} == set()
    owners = {}
    for part in PARTS:
        assert part.__bases__ == (object,)
        for name in vars(part):
            if name == '__init__' or not callable(getattr(part, name)):
                continue
            assert name not in owners, f'{name}: defined by {owners[name].__name__} and {part.__name__}'
            owners[name] = part
            if 'super()' in inspect.getsource(getattr(part, name)):
                raise AssertionError(f'{part.__name__}.{name} calls super()')
    for name in ('npm_h2d', 'npm_d2h', 'npm_d2d', 'npm_malloc', 'npm_free', 'npm_set_tuning'):
        assert owners[name] is hostsim.Runtime
    source = ''.join(inspect.getsource(part) for part in PARTS)
    assert source.count('decode_attention(') == 1 and source.count('WC.attention(') == 1


def test_the_runtime_records_in_every_profile():
    import ctypes
    for profile in ('training', 'paged', None):
        sim = hostsim.HostSim(profile)
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert sim.npm_malloc(ctypes.byref(a), 64) == 0 and sim.npm_malloc(ctypes.byref(b), 32) == 0
        host = np.arange(8, dtype=np.float32)
        sim.npm_h2d(a, host.ctypes.data, 32)
        sim.npm_d2d(b, a, 32)
        back = np.zeros(8, dtype=np.float32)
        sim.npm_d2h(back.ctypes.data, b, 16)
        assert (sim.uploads, sim.copies, sim.d2h, sim.calls) == ([32], [32], [16], []) and back.tolist() == [0, 1, 2, 3, 0, 0, 0, 0]
        assert (sim.live, sim.peak) == (96, 96) and sim.npm_free(a) == 0 and (sim.live, sim.peak) == (32, 96)
        assert sim.npm_set_tuning(20, 3) == 0 and sim.decode_splits == 3
        assert sim.npm_set_tuning(24, 1025) == 10002 and sim.npm_set_tuning(24, 5) == 0 and sim.prefix_splits == 5


# ---- the whole ABI at once -----------------------------------------------------------------------------------------------------------
F, VOCAB = 32, 50


def _generate(npm, **kwargs):
    """Three one-token steps of a batch of 2 through decode -> head -> processor -> sampler; (calls of the steps, tokens)."""
    dec, _ = DC.make_decoder(npm, F, 2, 2, 64, True, True, seed=11, batch=2)
    emb = npm.layers.Embedding(VOCAB, F)
    emb(np.zeros([1], dtype=np.int64))
    head = npm.layers.Linear(units=VOCAB)
    head(np.zeros([1, F], dtype=np.float32))
    sampler = npm.sampling.Sampler(2)
    sampler.set(1, temperature=0.8, top_k=10, top_p=0.9, seed=5)
    proc = npm.sampling.LogitProcessor(2, VOCAB, max_bias=1)
    proc.set(0, repetition_penalty=1.2)
    proc.set(1, logit_bias={3: -math.inf})
    history = npm.sampling.TokenHistory(2, 8)
    ids = np.array([1, 2], dtype=np.int64)
    for b in range(2):
        history.admit(b, [int(ids[b])])
    memory = np.random.default_rng(12).standard_normal([2, 7, F]).astype(np.float32)
    state = dec.start_decoding(memory, 16, page_size=16, **kwargs)
    first, tokens = len(npm.sim.calls), []
    for _ in range(3):
        z = head(dec.decode(emb.forward(ids).reshape(2, 1, F), state).reshape(2, F))
        result = sampler(proc(z, history))
        history.append(result)
        ids = result.ids
        tokens.append(result.numpy().tolist())
    return npm.sim.calls[first:], tokens


def test_a_generation_loop_runs_on_the_skinny_gemms_with_either_weights(npm):
    """Sampling and logit processors used to be simulated on one branch of the simulators and the skinny / fp16-weight GEMMs on
    another: no host test could run the first on the second."""
    assert hasattr(npm.sim, 'npm_sgemm_skinny') and hasattr(npm.sim, 'npm_logits_process')
    calls, tokens = _generate(npm)
    assert 'npm_sgemm_skinny' in calls and 'npm_logits_process' in calls and 'npm_sample_rows' in calls
    assert 'npm_sgemm_skinny_w16' not in calls and calls.count('npm_logits_process') == calls.count('npm_sample_rows') == 3
    assert all(0 <= t < VOCAB for step in tokens for t in step) and 3 not in [step[1] for step in tokens]
    half_calls, half_tokens = _generate(npm, weights='f16')
    assert 'npm_sgemm_skinny_w16' in half_calls and 'npm_sgemm_skinny' not in half_calls
    assert 'npm_logits_process' in half_calls and 'npm_sample_rows' in half_calls
    assert all(0 <= t < VOCAB for step in half_tokens for t in step) and 3 not in [step[1] for step in half_tokens]
