"""TEST INFRASTRUCTURE ONLY -- a host-memory simulator of the libnpm_hip.so C ABI.

It lets the CPU test-suite exercise the *host-side* logic of the product (Layer protocol, DeviceArray/optimizer contract,
gradient bucketing, the data-parallel exchange over gloo, the key / value caches, generation loops) in a container without a
GPU.  "Device pointers" are addresses of NumPy buffers; every entry point is restated with NumPy / the oracle / the reference
modules of tests/.  The product never loads this: tests install it explicitly with ``hostsim.install()`` (which sets
``np_modeling_amd._C._LIB``).  Numerical parity of the real kernels is established on the GPU (tests marked ``gpu``).

One class, ``HostSim``, assembled from parts that know nothing of each other's methods:

* memory.py      views of "device" memory
* runtime.py     memory, copies, fills, events, knobs and everything they record
* training.py    GEMM, elementwise and row kernels (layer / RMS norm, gated SiLU), the fused attention core, rotary embeddings,
                 conv, Adam, AdamW with its clipping, losses (the fused softmax cross-entropy among them), dropout
* kvcache.py     the key / value cache (append, gather, page copies, each alone and fused: all planes in one call, rotation
                 with the append) and attention over it (decode, prefill, window, prefix)
* generation.py  take_rows, embedding_bwd, sample, verify, draft, beam, logit processors, log-probabilities
* gemm.py        the skinny-M GEMM and the half-precision weight copies

``install()`` gives the whole ABI.  ``install(profile)`` gives the library as it was when the feature of that name had just been
added: the same simulator with every later entry point hidden (``hasattr`` is False), because the product probes for entry
points with ``hasattr`` and tests compare its call traces between an earlier library and a later one.  A profile hides names and
does nothing else: a new entry point joins the part it belongs to and a new profile, and no earlier profile changes.  The features
up to 'logits' grew on two branches ('w16' is the other one); 'xent' joins them, and from there on a profile is the whole library of
its day, so that 'adamw', the last, is ``install()``.  fixtures.py holds the pytest fixtures the host test modules share.
"""

from . import gemm, kvcache  # noqa: F401  (tests read their pure rules: gemm.auto_splits, kvcache.split_ranges, ...)
from .gemm import SkinnyGemm
from .generation import Generation
from .kvcache import KVCache
from .memory import _addr, _deref, _half_rows, _ints, _mat, _page_ok, _vec, _words  # noqa: F401
from .runtime import Runtime
from .training import Training

# Entry points of the C ABI (np_modeling_amd._C.SIGNATURES) that no host test needs simulated.
NOT_SIMULATED = ('npm_debug_attn_trace', 'npm_debug_gemm_trace', 'npm_device_count', 'npm_device_name')

# What every library since the first has; then, feature by feature, the profile it extends and the entry points it added.
_TRAINING = '''
    npm_abi_version npm_last_error npm_init npm_shutdown npm_sync npm_stream npm_malloc npm_free npm_pool_stats npm_pool_trim
    npm_h2d npm_d2h npm_d2d npm_fill_f32 npm_fill_f64 npm_event_create npm_event_destroy npm_event_record npm_event_sync
    npm_event_elapsed_ms npm_set_math npm_get_math npm_last_math npm_set_tuning npm_last_attn_kernel
    npm_sgemm npm_relu_fwd npm_relu_bwd npm_add npm_add3 npm_axpy npm_scale npm_colsum npm_relu_bwd_colsum npm_attn_rowdot
    npm_softmax_fwd npm_softmax_bwd npm_layernorm_fwd npm_layernorm_bwd npm_layernorm_dropout_fwd npm_layernorm_dropout_bwd
    npm_mha_mask_summary npm_mha_core_supported npm_mha_core_fwd npm_mha_core_bwd npm_conv2d_fwd npm_conv2d_bwd_x npm_conv2d_bwd_w
    npm_conv2d_bwd_w_relu npm_adam_step npm_mse_fwd npm_mse_bwd npm_xent_fwd npm_xent_bwd npm_mask_scale npm_dropout_philox'''
_ADDED = {
    'training': ((), _TRAINING),
    'decode': (('training',), '''npm_mha_core_fwd_grouped npm_mha_core_bwd_grouped npm_mha_decode_supported npm_mha_decode_splits
                               npm_mha_decode_fwd npm_kv_append npm_last_decode_kernel'''),
    'varlen': (('decode',), 'npm_mha_decode_fwd_varlen npm_kv_append_varlen npm_kv_gather_varlen'),
    'paged': (('varlen',), 'npm_mha_decode_fwd_paged npm_kv_append_paged npm_kv_gather_paged'),
    'skinny': (('paged',), 'npm_sgemm_skinny npm_sgemm_skinny_supported npm_sgemm_skinny_splits npm_last_skinny_kernel'),
    'w16': (('skinny',), 'npm_sgemm_skinny_w16 npm_sgemm_skinny_w16_supported npm_cvt_f32_f16 npm_cvt_f16_f32'),
    'prefill': (('paged',), 'npm_mha_prefill_supported npm_mha_prefill_fwd npm_last_prefill_kernel'),
    'kv16': (('prefill',), 'npm_kv_append_f16 npm_kv_gather_f16 npm_mha_decode_fwd_f16'),
    'prefill16': (('kv16',), 'npm_mha_prefill_fwd_f16'),
    'rope': (('prefill16',), 'npm_rope'),
    'window': (('prefill16',), 'npm_mha_decode_fwd_window npm_mha_prefill_fwd_window npm_mha_decode_window_splits'),
    'sample': (('window',), 'npm_take_rows npm_embedding_bwd npm_sample_rows npm_last_sample_kernel'),
    'spec': (('sample',), 'npm_verify_rows npm_ngram_draft npm_last_draft_kernel'),
    'prefix': (('spec',), '''npm_kv_copy_pages npm_mha_prefix_supported npm_mha_prefix_splits npm_mha_prefix_fwd npm_attn_combine
                            npm_last_prefix_kernel'''),
    'beam': (('prefix', 'rope'), 'npm_beam_step npm_last_beam_kernel'),
    'logits': (('beam',), 'npm_logits_process npm_history_append npm_logprob_rows npm_last_logits_kernel'),
    'xent': (('logits', 'w16'), 'npm_softmax_xent_rows npm_last_xent_kernel'),
    'llama': (('xent',), 'npm_rmsnorm_fwd npm_rmsnorm_bwd npm_swiglu_fwd npm_swiglu_bwd'),
    'lm': (('llama',), 'npm_kv_copy_pages_planes npm_rope_kv_append npm_last_rope_append_kernel'),
    'adamw': (('lm',), 'npm_sumsq_ranges npm_clip_finish npm_adamw_step'),
}


def _names(profile):
    bases, added = _ADDED[profile]
    return frozenset(added.split()).union(*(_names(b) for b in bases))


PROFILES = {profile: _names(profile) for profile in _ADDED}


class HostSim(Runtime, Training, KVCache, Generation, SkinnyGemm):
    def __init__(self, profile=None):
        super().__init__()
        self._visible = None if profile is None else PROFILES[profile]

    def __getattribute__(self, name):
        if name.startswith('npm_'):
            visible = object.__getattribute__(self, '_visible')
            if visible is not None and name not in visible:
                raise AttributeError('%s: not an entry point of this library' % name)
        return object.__getattribute__(self, name)


def install(profile=None):
    """Install a fresh simulator as the product's library handle; returns it."""
    from np_modeling_amd import _C
    sim = HostSim(profile)
    _C._LIB = sim
    _C._DEVICE = 0
    return sim


def uninstall():
    from np_modeling_amd import _C
    _C._LIB = None
    _C._DEVICE = None
