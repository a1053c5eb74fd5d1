"""GPU: every instance of the buffer-instruction epilogue of the LDS-DMA GEMM (``write_tile_buf`` / ``rmw_epilogue<F, CS>``,
csrc/npm_mfma_tile.h) at tile edges, the kernels behind tuning knobs, and the tile map -- on the case lists of
tests/gemm_epilogue_cases.py, whose properties tests/test_gemm_epilogue_host.py proves without a GPU (every case takes the DMA
kernel, every family the instance it is named after, the harness and the references are right).

Per case: a plain run (flags 0, alpha 1, same math mode, split and column-sum request) gives the accumulators ``acc``, held to
float64 at 2e-6 (conftest.assert_close's metric, the bound of tests/test_gpu_gemm.py).  The epilogue does not touch the K loop, so
the epilogue run works on the same bits and is held to float32 arithmetic on ``acc``:
  * alpha == 1, or no addend: the stored values EQUAL the float32 expression (acc + bias, (acc + bias) + res, max(v, 0),
    aux >= 0 ? v : 0, float32(alpha) * acc); the saved pre-activation equals v;
  * alpha != 1 with an addend (the multiply-add may be contracted): |got - w| <= 3 * 2^-24 (|alpha acc| + |bias| + |res|), w in
    float64 from acc -- three roundings of intermediates no larger than that sum;
  * softmax_bwd: |got - w| <= 2^-22 |w|, w = alpha aux (acc - rowvec) -- three roundings, on two products and one difference.
These bounds are derived, not measured.  Column sums: against the float64 column sums of the stored C at 3e-6, and the same bits
from a second run.  ``npm.last_math()`` after each launch proves the path: the requested mode under a split mode (so the same
descriptor does not take the fallback under 'f32' either), 'f32' with column sums or the wide tile, the bf16 split for a batch
under 'f16x2'.  C starts as NaN everywhere; guard words, padding columns and inputs must keep their bits.
"""

import numpy as np
import pytest

import gemm_epilogue_cases as GC
from conftest import assert_close

pytestmark = pytest.mark.gpu

DEFAULTS = {GC.TUNE_PIPELINE: 2, GC.TUNE_GROUP_M: 8, GC.TUNE_BUF_EPILOGUE: 1, GC.TUNE_WIDE_TILE: 0}      # csrc/npm_gemm.hip: the knobs' initial values


@pytest.fixture(scope='module')
def D():
    from np_modeling_amd import device
    return device


@pytest.fixture(autouse=True)
def _every_math_mode(math_mode):
    return math_mode


def _tune(knob, value):
    from np_modeling_amd import _C
    _C.check(_C.lib().npm_set_tuning(knob, int(value)), 'npm_set_tuning')


@pytest.fixture(autouse=True)
def _knobs_back_to_default():
    """However a test ends, the next one starts from the default pipeline, tile, tile order and epilogue."""
    yield
    for knob, value in DEFAULTS.items():
        _tune(knob, value)


def _last_math():
    import np_modeling_amd as npm
    return npm.last_math()


def _same_bits(a, b, what):
    assert np.array_equal(GC.bits(a), GC.bits(b)), f'{what}: {GC._first(GC.bits(a), GC.bits(b))}'


def _run_exact(D, case, want_math):
    """Sections 'plain run' and 'epilogue run' of the module docstring on one case; returns (operands, plain, epilogue run)."""
    ops = GC.Operands(D, case)
    plain = GC.launch(ops, False)
    assert _last_math() == want_math, (case.what, 'plain run', _last_math())
    got = GC.launch(ops, True)
    assert _last_math() == want_math, (case.what, 'epilogue run', _last_math())
    GC.check(ops, plain, got, exact=True)
    return ops, plain, got


@pytest.mark.parametrize('family,layout', GC.GRID)
def test_epilogue_instance_at_tile_edges(D, math_mode, family, layout):
    fam = GC.FAMILY[family]
    for case in GC.cases(family, layout):
        want_math = GC.expected_math(case, math_mode)
        ops, plain, got = _run_exact(D, case, want_math)
        if fam.colsum:                                         # fixed summation order: the same bits every run
            again = GC.launch(ops, True)
            _same_bits(again.colsum, got.colsum, case.what + ' column sums of a second run')
            _same_bits(again.c, got.c, case.what + ' C of a second run')
        if fam.alpha == 1.0:
            # The other epilogue on the same accumulators: write_tile inside the DMA kernel.  Without the buffer epilogue there are
            # no fused column sums (a pass over C instead) and no f16x2 kernel, so the kernel honours the split mode / runs the bf16
            # split there; where that is another arithmetic than the buffer run's, the float64 bound takes the place of the bits.
            _tune(GC.TUNE_BUF_EPILOGUE, 0)
            other = GC.launch(ops, True)
            other_math = _last_math()
            _tune(GC.TUNE_BUF_EPILOGUE, 1)
            assert other_math == ('bf16x3' if math_mode == 'f16x2' else math_mode), (case.what, other_math)
            if other_math == want_math:
                _same_bits(other.c, got.c, case.what + ' write_tile against write_tile_buf')
                if got.aux is not None:
                    _same_bits(other.aux, got.aux, case.what + ' write_tile against write_tile_buf, saved pre-activation')
                if fam.colsum:
                    assert_close(other.colsum, other.c.astype(np.float64).sum(axis=(0, 1)), tol=3e-6, what=case.what + ' (column sums, pass over C)')
            else:
                GC.check(ops, plain, other, exact=False)


# ---- kernels behind knobs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', GC.WIDE_LAYOUTS)
@pytest.mark.parametrize('family', GC.WIDE_FAMILIES)
def test_wide_tile(D, math_mode, family, layout):
    """NPM_TUNE_GEMM_WIDE_TILE = 1: the 2 x 4-wave 128 x 256 tile, exact fp32 whatever the mode."""
    _tune(GC.TUNE_WIDE_TILE, 1)
    for case in GC.wide_cases(family, layout):
        _run_exact(D, case, GC.expected_math(case, math_mode, wide=True))


@pytest.mark.parametrize('layout', GC.LAYOUTS)
@pytest.mark.parametrize('family', GC.PIPELINE_FAMILIES)
@pytest.mark.parametrize('pipeline', [0, 1])
def test_register_staged_kernels(D, math_mode, pipeline, family, layout):
    """NPM_TUNE_GEMM_PIPELINE = 0 / 1: sgemm_mfma_kernel<..., 0> and <..., true, 1> (the double-buffered one runs nowhere else) on
    shapes that take the DMA kernel by default, held to float64."""
    _tune(GC.TUNE_PIPELINE, pipeline)
    for case in GC.pipeline_cases(family, layout):
        ops = GC.Operands(D, case)
        plain, got = GC.launch(ops, False), GC.launch(ops, True)
        assert _last_math() == 'f32', case.what
        GC.check(ops, plain, got, exact=False, tol_plain=2e-6, tol=3e-6)


@pytest.mark.parametrize('group_m', GC.GROUP_M)
@pytest.mark.parametrize('kind', list(GC.TILE_MAP_KINDS))
def test_tile_map(D, math_mode, kind, group_m):
    """xcd_remap and tile_coords on grids of 1 .. 19 x 1 .. 5 tiles, ragged last row and column, every remainder of the block count
    mod 8, with split-K and with a batch, NPM_TUNE_GEMM_GROUP_M = 8 (default), 1 and 3: a tile visited twice or never shows as a
    wrong value or as the NaN C started with."""
    _tune(GC.TUNE_GROUP_M, group_m)
    for case in GC.tile_map_cases(kind):
        ops = GC.Operands(D, case)
        plain = GC.launch(ops, False)
        assert _last_math() == GC.expected_math(case, math_mode), case.what
        assert_close(plain.c, ops.prod64, tol=2e-6, what=f'{case.what} group_m={group_m}')
