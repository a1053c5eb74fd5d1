"""CPU: the case lists, the harness and the references of the GEMM epilogue tests (tests/gemm_epilogue_cases.py), without a GPU.

* No case can silently miss its target: the dispatch of ``npm_sgemm`` (csrc/npm_gemm_plan.h gemm_plan) and the instance choice of
  ``write_tile_buf`` (csrc/npm_mfma_tile.h:354-411) are restated in Python in the cases module (each line cited there); every case
  of every list must meet the LDS-DMA predicate -- the share left out is zero, as a condition --, every family must reach the
  instance it is named after, and every (family, layout) list must cover all M, N and K classes.
* The harness: the whole grid runs through tests/hostsim/'s ``npm_sgemm`` with the GPU test's own harness -- guards, padding
  sentinels and untouched inputs checked, results held to float64 at 3e-6 (the simulator computes in float64, so the equality arm
  is off here).
* The float32 reference expressions against a per-element Python loop.
"""

import numpy as np
import pytest

import gemm_epilogue_cases as GC
import hostsim


@pytest.fixture
def D():
    from np_modeling_amd import device, parallel
    hostsim.install('training')
    parallel.set_communicator(None)
    yield device
    parallel.set_communicator(None)
    hostsim.uninstall()


def _all_dma_lists():
    for family, layout in GC.GRID:
        yield from GC.cases(family, layout)
    for kind in GC.TILE_MAP_KINDS:
        yield from GC.tile_map_cases(kind)


# ---- no case misses its target ---------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_dma_kernel_with_the_buffer_epilogue():
    listed = list(_all_dma_lists())
    assert len(listed) > 800
    missed = [c.what for c in listed if not GC.takes_dma_kernel(c)]
    assert not missed, missed
    # ... and with NPM_TUNE_GEMM_BUF_EPILOGUE = 0 the same kernel runs write_tile: dma without dma_path
    assert not any(GC.takes_dma_kernel(c, buf_epilogue=0) for c in listed)
    wide = [c for family in GC.WIDE_FAMILIES for layout in GC.WIDE_LAYOUTS for c in GC.wide_cases(family, layout)]
    assert len(wide) == 4 * 2 * 8 and all(GC.takes_wide_tile(c) for c in wide)
    assert {c.m for c in wide} == {1, 65, 129, 257} and {c.n for c in wide} == {256, 512} and {c.k for c in wide} == {32}
    # the register-staged kernels run where the pipeline knob says so, whatever the shape
    staged = [c for family in GC.PIPELINE_FAMILIES for layout in GC.LAYOUTS for c in GC.pipeline_cases(family, layout)]
    assert not any(GC.takes_dma_kernel(c, pipeline=p) for c in staged for p in (0, 1))
    assert sum(GC.takes_dma_kernel(c) for c in staged) >= 20          # most of them would take the DMA kernel by default


def test_the_predicate_knows_the_fallbacks():
    """The restated predicate is not vacuous: it rejects what ``test_epilogues`` and the unaligned sweeps run."""
    C = GC.Case
    assert not GC.takes_dma_kernel(C('plain', 'NN', 200, 136, 72))            # K % 16 != 0
    assert not GC.takes_dma_kernel(C('plain', 'NN', 128, 130, 32))            # B [K, N] with N % 4 != 0
    assert not GC.takes_dma_kernel(C('plain', 'TN', 130, 128, 32))            # A [K, M] with M % 4 != 0
    assert GC.takes_dma_kernel(C('plain', 'NT', 129, 129, 32))
    assert not GC.takes_wide_tile(C('plain', 'NN', 128, 384, 32)) and not GC.takes_wide_tile(C('plain_colsum', 'NN', 128, 256, 32))


@pytest.mark.parametrize('family', [f.name for f in GC.FAMILIES])
def test_every_family_reaches_the_instance_it_is_named_after(family):
    fam = GC.FAMILY[family]
    assert GC.instance_of(fam.flags, fam.alpha, fam.colsum) == fam.instance


def test_the_families_name_every_branch():
    reached = {f.instance for f in GC.FAMILIES}
    B, R, S, K, X, ONE = GC.BIAS, GC.RESIDUAL, GC.RELU_SAVE, GC.RELU_MASK, GC.SOFTMAX_BWD, GC.ONE
    store_only = {('store', 'a'), ('store', 'alpha*a'), ('store', 'a+bias'), ('store', 'generic', False)}
    compile_time = {('rmw', key, False) for key in (B | R | ONE, R | ONE, B | S | ONE, S | ONE, K | ONE, K | R | ONE, X)}
    assert reached == store_only | compile_time | {('rmw', -1, False), ('rmw', K | ONE, True), ('store', 'generic', True), ('rmw', -1, True)}
    # the run-time instance is reached four ways, softmax_bwd at alpha 1 and not 1, the residual once aliasing C
    assert sum(f.instance == ('rmw', -1, False) for f in GC.FAMILIES) == 4
    assert {f.alpha for f in GC.FAMILIES if f.flags & X} == {1.0, 0.125} and sum(f.alias for f in GC.FAMILIES) == 1
    # with column sums requested no compile-time instance without them may be chosen (it would leave the sums at zero)
    for flags in range(64):
        for alpha in (1.0, 0.5):
            assert GC.instance_of(flags, alpha, True)[-1] is True


@pytest.mark.parametrize('family,layout', GC.GRID)
def test_every_list_covers_the_classes(family, layout):
    listed = GC.cases(family, layout)
    single = [c for c in listed if c.batch == (1, 1)]
    assert {c.m for c in single} == set(GC.m_classes(layout)) and {c.n for c in single} == set(GC.n_classes(layout))
    assert {c.k for c in single} == {16, 32, 48}
    assert [c.batch for c in listed if c.batch != (1, 1)] == [(2, 3)]
    if layout == 'TN':
        assert all(c.m % 4 == 0 for c in listed)
    if layout != 'NT':
        assert all(c.n % 4 == 0 for c in listed)
    assert all(c.split_k == 1 for c in listed)
    fam = GC.FAMILY[family]
    for c in listed:
        d = GC.describe(c)
        assert d.lda % 4 == 0 and d.ldb % 4 == 0 and all(s % 4 == 0 for s in d.sa + d.sb)
        pitches = [d.ldc] + ([d.ldr] if fam.flags & GC.RESIDUAL and not fam.alias else []) + \
                  ([d.ldaux] if fam.flags & (GC.RELU_SAVE | GC.RELU_MASK | GC.SOFTMAX_BWD) else [])
        assert len(set(pitches)) == len(pitches), (c.what, pitches)


def test_grid_size():
    """20 families x 3 layouts; 15 descriptors per list in NN and NT (14 M classes + the batched one), 11 in TN."""
    per_family = {f.name: sum(len(GC.cases(f.name, layout)) for fam, layout in GC.GRID if fam == f.name) for f in GC.FAMILIES}
    assert set(per_family.values()) == {41} and len(GC.GRID) == 60


def test_tile_map_lists():
    plain = GC.tile_map_cases('plain')
    tiles = lambda c: (-(-c.m // 128), -(-c.n // 128))
    assert {tiles(c)[0] for c in plain} == set(GC.TILES_M) and {tiles(c)[1] for c in plain} == set(GC.TILES_N) and len(plain) == 24
    everything = [c for kind in GC.TILE_MAP_KINDS for c in GC.tile_map_cases(kind)]
    assert all(c.m % 128 == 1 and c.n % 128 == 4 for c in everything)                      # ragged last tile row and column
    assert {GC.grid_blocks(c) % 8 for c in everything} == set(range(8))                    # xcd_remap: every remainder of the grid
    assert {GC.grid_blocks(c) % 8 for c in plain} == set(range(8)) - {4}                   # (no product of the listed tile counts is 4 mod 8)
    split, batch = GC.tile_map_cases('split'), GC.tile_map_cases('batch')
    assert all(c.k == 96 and c.split_k == 3 and GC.grid_blocks(c) == 3 * tiles(c)[0] * tiles(c)[1] for c in split)
    assert all(c.batch == (2, 3) and GC.grid_blocks(c) == 6 * tiles(c)[0] * tiles(c)[1] for c in batch)
    for cases in (split, batch):
        assert {tiles(c)[0] for c in cases} == set(GC.TILES_M)


def test_expected_math():
    C = GC.Case
    assert GC.expected_math(C('bias_res', 'NN', 128, 128, 32), 'bf16x3') == 'bf16x3'
    assert GC.expected_math(C('bias_res', 'NN', 128, 128, 32), 'f16x2') == 'f16x2'
    assert GC.expected_math(C('bias_res', 'NN', 128, 128, 32, (2, 3)), 'f16x2') == 'bf16x3'
    assert GC.expected_math(C('plain_colsum', 'NN', 128, 128, 32), 'bf16x3_fast') == 'f32'
    assert GC.expected_math(C('plain', 'NN', 128, 256, 32), 'bf16x3', wide=True) == 'f32'


# ---- the harness, on the simulator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,layout', GC.GRID)
def test_harness_and_references_on_the_simulator(D, family, layout):
    for case in GC.cases(family, layout):
        ops = GC.Operands(D, case)
        plain, got = GC.launch(ops, False), GC.launch(ops, True)
        GC.check(ops, plain, got, exact=False, tol_plain=3e-6, tol=3e-6)
        fam = ops.fam
        if fam.flags & (GC.RELU_MASK | GC.SOFTMAX_BWD):          # the special values are where the lists say: all four, last row and column
            for v in GC.SPECIALS if case.n >= 4 else []:
                assert (GC.bits(ops.aux) == GC.bits(v)).any(), case.what
            assert (GC.bits(ops.aux[:, -1, :, -1]) == 0x80000000).all(), case.what
        if fam.flags & GC.RELU_MASK:                             # x >= 0 passes, zeros of either sign included
            zeros = ops.aux == 0
            want, _ = GC.epilogue(fam._replace(flags=fam.flags & ~GC.RELU_MASK), ops.prod64, ops.bias, ops.res, ops.aux, None, np.float64)
            np.testing.assert_allclose(got.c[zeros], want[zeros], rtol=1e-5)
            assert (got.c[ops.aux < 0] == 0).all()


@pytest.mark.parametrize('kind', ['split', 'batch'])
def test_tile_map_cases_on_the_simulator(D, kind):
    for case in GC.tile_map_cases(kind)[:3]:
        ops = GC.Operands(D, case)
        GC.check(ops, GC.launch(ops, False), GC.launch(ops, True), exact=False)


@pytest.mark.parametrize('layout', GC.LAYOUTS)
def test_knob_lists_on_the_simulator(D, layout):
    listed = [c for family in GC.PIPELINE_FAMILIES for c in GC.pipeline_cases(family, layout)]
    if layout in GC.WIDE_LAYOUTS:
        listed += [c for family in GC.WIDE_FAMILIES for c in GC.wide_cases(family, layout)]
    for case in listed:
        ops = GC.Operands(D, case)
        GC.check(ops, GC.launch(ops, False), GC.launch(ops, True), exact=False)


def test_the_harness_sees_a_written_padding_word_and_a_changed_input(D):
    case = GC.Case('bias_res_relu_save', 'NN', 5, 8, 16)
    ops = GC.Operands(D, case)
    g = GC.Guarded(5, 8, (1, 1), 12, 0, 0).upload(D)
    g.download('clean')
    flat = g.dev.numpy()
    flat[GC.GUARD + 9] = 1.0                                    # a padding column of row 0
    g.dev.set(flat)
    with pytest.raises(AssertionError, match='guard or padding'):
        g.download('dirty')
    flat = ops.g_res.dev.numpy()
    flat[GC.GUARD] = -flat[GC.GUARD]
    ops.g_res.dev.set(flat)
    with pytest.raises(AssertionError, match='an input was written'):
        GC.launch(ops, True)
    with pytest.raises(AssertionError, match='overlaps'):
        GC.Guarded(4, 8, (1, 1), 6, 0, 0)


def test_the_exact_arm_catches_one_wrong_bit(D):
    """On the simulator the equality arm must FAIL somewhere (float64 arithmetic rounded once is not the float32 expression);
    with outputs made from the float32 expression it passes, and one flipped mantissa bit in one element fails it again."""
    case = GC.Case('bias_res', 'NT', 33, 31, 32)
    ops = GC.Operands(D, case)
    plain = GC.launch(ops, False)
    want, _ = GC.epilogue(ops.fam, plain.c, ops.bias, ops.res, None, None, np.float32)
    GC.check(ops, plain, GC.Output(want, None, None), exact=True)
    wrong = want.copy()
    wrong.view(np.uint32)[0, 32, 0, 30] ^= 1
    with pytest.raises(AssertionError, match='differs from the float32 expression'):
        GC.check(ops, plain, GC.Output(wrong, None, None), exact=True)
    # the derived bounds admit the float32 expression evaluated without contraction
    for family in ('bias_neg2', 'bias_res_half', 'relu_mask_res_neg2', 'softmax_bwd', 'softmax_bwd_eighth'):
        ops = GC.Operands(D, GC.Case(family, 'NT', 65, 33, 48))
        plain = GC.launch(ops, False)
        rowvec = ops.rowvec_planes() if ops.rowvec is not None else None
        want, _ = GC.epilogue(ops.fam, plain.c, ops.bias, ops.res, ops.aux, rowvec, np.float32)
        GC.check(ops, plain, GC.Output(want, None, None), exact=True)
        wrong = want.copy()
        at = np.unravel_index(np.abs(want).argmax(), want.shape)
        wrong[at] *= np.float32(1 + 2.0 ** -20)
        with pytest.raises(AssertionError, match='bound exceeded'):
            GC.check(ops, plain, GC.Output(wrong, None, None), exact=True)


# ---- the references against a loop --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', [f.name for f in GC.FAMILIES])
def test_float32_expressions_against_a_python_loop(family):
    fam = GC.FAMILY[family]
    rng = np.random.default_rng(GC.FAMILIES.index(fam))
    shape = (1, 5, 2, 6)
    acc, res, aux = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    bias = rng.standard_normal(6).astype(np.float32)
    rowvec = rng.standard_normal((1, 5, 2, 1)).astype(np.float32)
    GC.plant_specials(aux)
    acc[0, 1, 0, :4] = -bias[:4] if fam.flags & GC.BIAS else GC.SPECIALS        # pre-activations of exactly zero and of either tiny sign
    want_c, want_pre = GC.epilogue_loop(fam, acc, bias, res, aux, rowvec)
    got_c, got_pre = GC.epilogue(fam, acc, bias, res, aux, rowvec, np.float32)
    assert got_c.dtype == np.float32 and np.array_equal(got_c, want_c)
    assert (got_pre is None) == (want_pre is None)
    if got_pre is not None:
        assert np.array_equal(GC.bits(got_pre), GC.bits(want_pre))
