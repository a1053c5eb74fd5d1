"""CPU: the case lists of tests/conv_cases.py reach every cell they name (``route`` is the dispatch of csrc/npm_conv.hip
restated; tests/test_gpu_conv_paths.py asserts on the device that the library reports the same string), every geometry class has
the property it is named for, the float64 oracle the GPU is judged by agrees with an independent formulation on every geometry of
the lists, and ``fast_div`` is exact."""

import itertools

import numpy as np
import pytest

import conv_cases as CC
from oracle import np_oracle as O

CUS = (256, 304, 64)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cus', CUS)
def test_forward_and_grad_x_cases_reach_every_instance_at_every_geometry(cus):
    """Forward / grad_x do not split K: their route does not depend on the CU count.  Cells: instance x geometry class."""
    reached = set()
    for case in CC.FWD_PLAIN + CC.FWD_DMA:
        want = CC.CHANNELS[(case.c0, case.c1)]
        got = tuple(CC.instance(r) for r in case.routes(cus))
        assert got == want, case.id
        reached.update((inst, case.geometry) for inst in got)
        for mode, (math, _) in CC.CONV_MATH.items():              # the math mode reaches the report on the DMA instances only
            for r, inst in zip(case.routes(cus, mode), got):
                f = CC.fields(r)
                assert f['math'] == (math if inst in ('dma', 'tall') else 0) and CC.instance(r) == inst
                assert f['buf'] == (inst in ('dma', 'tall')) and f['korder'] == (inst in ('dma', 'tall'))
    classes = [g for g, _ in CC.FWD_GEOMETRIES]
    assert len(classes) == 9
    assert reached == set(itertools.product(('scalar', 'vec', 'dma', 'tall'), classes))
    # every DMA channel pair is a DMA pair, and none of the plain ones is
    assert all(set(CC.CHANNELS[c]) & {'dma', 'tall'} for c in CC.DMA_CHANNELS) and len(CC.DMA_CHANNELS) == 6
    assert {CC.CHANNELS[c][0] for c in CC.DMA_CHANNELS} == {'dma', 'tall', 'vec'} and {CC.CHANNELS[c][1] for c in CC.DMA_CHANNELS} == {'dma', 'tall', 'vec'}


@pytest.mark.parametrize('cus', CUS)
def test_knob_cases_change_what_they_say(cus):
    classes = {g for g, _ in CC.FWD_GEOMETRIES}
    by_cell = {}
    for case in CC.FWD_KNOBS + CC.FWD_PRIO + CC.FWD_MISALIGNED:
        by_cell.setdefault(case.cell, []).append(case)
        base = case._replace(knobs=CC.DEFAULT, offset=0).routes(cus)
        if case.cell != 'misaligned':                                              # knob variants sit on DMA-eligible cases
            assert {CC.instance(r) for r in base} & {'dma', 'tall'}, case.id
        fwd, bwd = (CC.fields(r) for r in case.routes(cus))
        if case.cell == 'korder0':
            assert fwd['korder'] == 0 and CC.instance(case.routes(cus)[0]) in ('dma', 'tall') and case.c0 >= 32
        elif case.cell == 'dma0':                                                  # the fallback of the 2^30 / 2^31 guards
            assert [CC.instance(r) for r in case.routes(cus)] == ['vec', 'vec'] and fwd['buf'] == 0 and bwd['buf'] == 0
        elif case.cell == 'dma2':                                                  # the square tile at N <= 64
            assert [CC.instance(r) for r in base] == ['tall', 'tall'] and [CC.instance(r) for r in case.routes(cus)] == ['dma', 'dma']
        elif case.cell.startswith('prio'):
            assert case.routes(cus) == base                                        # priorities change no route: bit-equal results
        else:
            assert case.cell == 'misaligned' and [CC.instance(r) for r in case.routes(cus)] == ['scalar', 'scalar']
            assert 'scalar' not in [CC.instance(r) for r in base]                  # at vec-friendly and at DMA-eligible channels
    assert set(by_cell) == {'korder0', 'dma0', 'dma2', 'prio1', 'prio2', 'prio3', 'misaligned'}
    for cell in ('korder0', 'dma0', 'dma2'):
        assert {c.geometry for c in by_cell[cell]} == classes
    assert {c.knobs.prio for c in CC.FWD_PRIO} == {1, 2, 3}
    for cell in ('korder0', 'dma0'):                                               # on the square and on the tall tile
        assert {CC.instance(c._replace(knobs=CC.DEFAULT).routes(cus)[0]) for c in by_cell[cell]} == {'dma', 'tall'}
    assert [name for name, *_ in CC.EPILOGUES] == ['bias_relu_pre', 'relu', 'bias', 'none']
    assert {(b, r, p) for _, b, r, p in CC.EPILOGUES} == {(True, 1, True), (False, 1, False), (True, 0, False), (False, 0, False)}


@pytest.mark.parametrize('cus', CUS)
def test_filter_gradient_cases_reach_every_instance(cus):
    for case in CC.WGRAD_DMA + CC.WGRAD_PLAIN:
        for mode in CC.CONV_MATH:
            r = case.route(cus, mode)
            assert CC.instance(r) == case.expect, (case.id, mode, r)
            assert (case.n * case.h * case.w) % 16 == 0 or case.expect != 'dma'
    assert {c.expect for c in CC.WGRAD_PLAIN} == {'vec', 'scalar'}
    cells = {c.cell for c in CC.WGRAD_DMA + CC.WGRAD_PLAIN}
    assert cells >= {'one_ktile', 'w2_h1', 'w2', 'w3', 'k7_w8', 'm240', 'split_seam', 'one_split', 'split_seam_blocks',
                     'many_tiles_blocks', 'pixels_not_16', 'scalar_channels', 'dma0', 'misaligned'}
    one = next(c for c in CC.WGRAD_DMA if c.cell == 'one_ktile')
    assert one.w == 1 and one.n * one.h * one.w == 16 and CC.fields(one.route(cus))['splits'] == 1
    # splits engage at 16 K tiles of 32 pixels, not at 15: whatever the CU count
    seam, single = (next(c for c in CC.WGRAD_DMA if c.cell == name) for name in ('split_seam', 'one_split'))
    f = CC.fields(seam.route(cus))
    pixels = seam.n * seam.h * seam.w
    assert -(-pixels // 32) == 16 and (f['splits'], f['kper']) == (2, 256)
    assert CC.seams(pixels, f['splits'], f['kper']) == [256] and 256 % seam.w != 0, 'seam inside a row'
    assert 0 < pixels - (f['splits'] - 1) * f['kper'] < f['kper'], 'last split shorter'
    assert -(-(single.n * single.h * single.w) // 32) == 15 and CC.fields(single.route(cus))['splits'] == 1
    assert single._replace(h=seam.h, w=seam.w).shape == seam.shape                  # a neighbour: only the width differs
    assert {c.knobs.blocks for c in CC.WGRAD_DMA if c.cell == 'split_seam_blocks'} == {-1, 3, 4, 6, 12}
    assert all(CC.fields(c.route(cus))['splits'] == 2 for c in CC.WGRAD_DMA if c.cell == 'split_seam_blocks')      # 16 K tiles: 2 at most


def test_wgrad_blocks_values_are_different_split_counts():
    """At (1,16,31) every NPM_TUNE_CONV_WGRAD_BLOCKS value is capped by nkt / 8 = 2; the many-tiles case is where the values
    differ, and where the renormalisation of ``splits`` by ``kt_per`` changes the count (30 -> 29, 61 -> 57).  It depends on the
    CU count: stated here for 256, asserted on the device through its own."""
    many = [c for c in CC.WGRAD_DMA if c.cell == 'many_tiles_blocks']
    assert all(c.cus_dependent for c in many) and not any(c.cus_dependent for c in CC.WGRAD_DMA if c.cell != 'many_tiles_blocks')
    got = {c.knobs.blocks: CC.fields(c.route(256))['splits'] for c in many}
    assert got == {0: 29, 3: 29, -1: 31, 4: 40, 6: 57, 12: 64}
    for c in many:
        f = CC.fields(c.route(256))
        pixels = c.n * c.h * c.w
        assert (f['splits'] - 1) * f['kper'] < pixels <= f['splits'] * f['kper']      # no empty split
    assert CC._renormalise(512, 30) == (29, 18) and CC._renormalise(512, 61) == (57, 9)
    assert len({CC.fields(c.route(cus))['splits'] for c in many for cus in (304,)}) >= 4


@pytest.mark.parametrize('cus', CUS)
def test_fused_cases_reach_every_tiling_and_every_fallback(cus):
    tilings, modes = {}, set()
    for case in CC.FUSED:
        r = case.route(cus)
        modes.add(case.knobs.fused)
        if case.knobs.fused == 0:
            assert r.startswith('two_pass conv_wgrad_glds'), case.id
            continue
        assert CC.instance(r) == 'fused', (case.id, r)
        tilings.setdefault(CC.tiling_class(*case.shape, case.knobs, cus), []).append(case)
    assert modes == {0, 1, 2, 3}
    plain = {t.split('+')[0] for t in tilings}
    assert plain >= {'128x1', '192x1', '128x3', 'trio', '192x5', '192x2', '128x5', '192x3'}, plain
    assert '192x2+ragged96' in tilings                          # WGRAD_FUSED = 3 on k*k*C0 = 288
    assert {c.cell for c in tilings['trio']} == {'h1', 'seam_in_row', 'odd_ktiles'}
    assert {c.cell for c in CC.FUSED} == {g for g, _ in CC.FUSED_GEOMETRIES}
    assert {c.c1 for c in CC.FUSED} == {4, 20, 132}
    for t, cases in tilings.items():                            # the trio needs splits, the four-wave 192 x 3 is what is left without
        for c in cases:
            f = CC.fields(c.route(cus))
            assert (f['trio'] == 1) == (t == 'trio') and f['ksync'] == 0 and f['wr'] == (3 if t == 'trio' or t.startswith('192') else 2)
    # every route of a (geometry, channels) is there once
    assert len({(c.shape, c.route(cus)) for c in CC.FUSED}) == len(CC.FUSED) or cus != 256
    want = {'w15': 'dma', 'pixels_not_16': 'vec', 'channels_not_4': 'scalar', 'cout_not_4': 'scalar', 'math': 'dma', 'dma0': 'vec',
            'misaligned': 'scalar'}
    assert [c.cell for c in CC.FUSED_FALLBACK] == list(want)
    for case in CC.FUSED_FALLBACK:
        r = case.route(cus)
        assert r.startswith('two_pass ') and CC.instance(r) == want[case.cell], (case.id, r)
        # exactly one reason each: the shape takes the fused kernel once the reason is gone
        fixed = dict(w15=dict(w=16), pixels_not_16=dict(h=16), channels_not_4=dict(c0=8), cout_not_4=dict(c1=8), math=dict(knobs=CC.DEFAULT),
                     dma0=dict(knobs=CC.DEFAULT), misaligned=dict(offset=0))[case.cell]
        assert CC.instance(case._replace(**fixed).route(cus)) == 'fused', case.id
    assert CC.fields(CC.FUSED_FALLBACK[4].route(cus))['math'] == 2


@pytest.mark.parametrize('cus', CUS)
def test_rendezvous_case_engages(cus):
    """(4,64,64,64,128,3) under WGRAD_FUSED = 3: 1024 K tiles; the rendezvous needs every split to be two intervals long and the
    whole grid resident.  It holds at each CU count here; the GPU test asserts it for the device at hand."""
    for every in CC.RENDEZVOUS_KSYNC:
        kn = CC.Knobs(fused=3, ksync=every)
        plan = CC.fused_plan(*CC.RENDEZVOUS_SHAPE, kn, cus)
        assert plan['rows'] == 192 and plan['tiles_m'] == 3 and not plan['trio'] and plan['splits'] > 1
        assert plan['ksync'] == every and plan['kt_per'] >= 8
        assert CC.fields(CC.route('bwd_w_relu', *CC.RENDEZVOUS_SHAPE, kn, cus))['ksync'] == every
    assert CC.ksync_every(3) == 0 and CC.ksync_every(128) == 128
    assert CC.fused_plan(*CC.RENDEZVOUS_SHAPE, CC.Knobs(fused=1, ksync=2), cus)['trio']          # the default is the twelve-wave block


def test_pick_splits_restatement():
    """Hand-evaluated values of csrc/npm_gemm_plan.h pick_splits."""
    assert CC.pick_splits(2, 16, 256) == 2                       # capped by nkt / 8
    assert CC.pick_splits(25, 512, 256) == 30                    # 3 per CU: cost 3 / 30; 4 per CU: 40 splits, cost 4 / 40: no better
    assert CC.pick_splits(25, 512, 256, 4) == 40
    assert CC.pick_splits(25, 512, 256, 6) == 61 and CC.pick_splits(25, 512, 256, 12) == 64
    assert CC.pick_splits(25, 512, 256, 0, 2) == 20              # two resident blocks: 2 then 2 again
    assert CC.pick_splits(3, 1024, 256, 0, 3) == 128
    assert CC.pick_splits(600, 512, 256) == 1                    # 3 * 256 / 600 = 1


# ---- geometry claims -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,shape', CC.FWD_GEOMETRIES)
def test_forward_geometry_has_its_property(name, shape):
    assert CC.GEOMETRY_CLAIMS[name](*shape), (name, shape)


def test_forward_geometry_details():
    g = dict(CC.FWD_GEOMETRIES)
    assert 5 * 17 == 85 and 85 % 16 == 5 and CC.piece_images(5, 1, 17) == [1, 2, 2, 2, 2, 1]       # M ends mid-piece, pieces straddle
    assert CC.piece_images(16, 1, 1) == [16] and CC.piece_images(3, 2, 2) == [3]                   # sixteen / three images in a piece
    assert max(CC.piece_rows(*g['narrow_five_rows'][:3])) == 6
    n, h, w, k = g['wrap_mixed']
    fast = [CC.piece_is_fast(n, h, w, k, p) for p in range(0, n * h * w, 16)]
    assert any(fast) and not all(fast)
    n, h, w, k = g['m240']
    assert -(-n * h * w // 256) == 1 and -(-n * h * w // 128) == 2 and n * h * w - 128 == 112       # one tall tile; two square, 112 rows
    n, h, w, k = g['w16']
    assert all(CC.piece_is_fast(n, h, w, k, p) for p in range(0, n * h * w, 16))                    # every piece is one whole row


@pytest.mark.parametrize('name,shape', CC.FUSED_GEOMETRIES)
def test_fused_geometry_has_its_property(name, shape):
    n, h, w, k = shape
    assert CC.FUSED_CLAIMS[name](*shape), (name, shape)
    assert w >= 16 and (n * h * w) % 16 == 0


def test_fused_geometry_details():
    g = dict(CC.FUSED_GEOMETRIES)
    plan = CC.fused_plan(1, 33, 16, 64, 4, 3, CC.DEFAULT, 256)
    assert plan['nkt'] == 33 and (plan['splits'], plan['kt_per']) == (4, 9) and 33 - 3 * 9 == 6          # odd count, uneven splits
    plan = CC.fused_plan(1, 16, 31, 32, 20, 3, CC.DEFAULT, 256)
    assert plan['splits'] == 3 and (plan['kper'] % 31) != 0                                               # seams inside image rows
    # five tile rows: the `turn` rotation with a K-tile count that is no multiple of five
    plan = CC.fused_plan(*g['odd_ktiles'][:3], 36, 20, 5, CC.DEFAULT, 256)
    assert plan['tiles_m'] == 5 and plan['rows'] == 192 and plan['kt_per'] % 5 != 0


# ---- the oracle against a second formulation ---------------------------------------------------------------------------------------------------
def direct_fwd(x, filt):
    """y[n, h, w, :] = sum over the k x k window of the explicitly padded image, one output pixel at a time."""
    n, h, w, c0 = x.shape
    k, c1 = filt.shape[0], filt.shape[3]
    pad = k // 2
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c0))
    xp[:, pad:pad + h, pad:pad + w] = x
    y = np.zeros((n, h, w, c1))
    for b, i, j in np.ndindex(n, h, w):
        y[b, i, j] = np.tensordot(xp[b, i:i + k, j:j + k], filt, axes=3)
    return y


def direct_grads(x, filt, dy):
    """The adjoint of ``direct_fwd``, pixel by pixel: each output pixel scatters into its window of dx and adds an outer product to dw."""
    n, h, w, c0 = x.shape
    k = filt.shape[0]
    pad = k // 2
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, c0))
    xp[:, pad:pad + h, pad:pad + w] = x
    dxp, dw = np.zeros_like(xp), np.zeros_like(filt)
    for b, i, j in np.ndindex(n, h, w):
        dxp[b, i:i + k, j:j + k] += np.tensordot(filt, dy[b, i, j], axes=([3], [0]))
        dw += xp[b, i:i + k, j:j + k][..., None] * dy[b, i, j]
    return dxp[:, pad:pad + h, pad:pad + w], dw


def _operands(shape, c0, c1, seed):
    n, h, w, k = shape
    rng = np.random.default_rng([seed, n, h, w, k, c0, c1])
    return rng.standard_normal((n, h, w, c0)), rng.standard_normal((k, k, c0, c1)), rng.standard_normal((n, h, w, c1))


ORACLE_SHAPES = sorted({s for _, s in CC.FWD_GEOMETRIES + CC.FUSED_GEOMETRIES} | {(c.n, c.h, c.w, c.k) for c in CC.WGRAD_DMA + CC.WGRAD_PLAIN
                                                                                   if c.n * c.h * c.w <= 512})


@pytest.mark.parametrize('shape', ORACLE_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_oracle_equals_direct_sums(shape):
    for c0, c1 in ((3, 5), (4, 2)):
        x, filt, dy = _operands(shape, c0, c1, 1)
        np.testing.assert_allclose(O.conv2d_fwd(x, filt), direct_fwd(x, filt), rtol=1e-12, atol=1e-12)
        dx, dw = direct_grads(x, filt, dy)
        np.testing.assert_allclose(O.conv2d_grad_x(dy, filt), dx, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(O.conv2d_grad_w(dy, x, shape[3]), dw, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('shape', sorted((s for _, s in CC.FWD_GEOMETRIES), key=lambda s: s[0] * s[1] * s[2])[:3], ids=lambda s: 'x'.join(map(str, s)))
def test_oracle_gradients_equal_differences_of_the_forward(shape):
    """L = sum(y * dy) is linear in x and in the filter: L(x + e_i) - L(x) IS the gradient's element i, to rounding.  On the three
    smallest geometries (H, W <= pad among them) every element of both gradients."""
    x, filt, dy = _operands(shape, 3, 2, 2)
    loss = lambda xx, ff: float((direct_fwd(xx, ff) * dy).sum())
    base = loss(x, filt)
    gx, gw = O.conv2d_grad_x(dy, filt), O.conv2d_grad_w(dy, x, shape[3])
    for idx in np.ndindex(*x.shape):
        bumped = x.copy()
        bumped[idx] += 1.0
        assert abs(loss(bumped, filt) - base - gx[idx]) <= 1e-9 * (1 + abs(base)), idx
    for idx in np.ndindex(*filt.shape):
        bumped = filt.copy()
        bumped[idx] += 1.0
        assert abs(loss(x, bumped) - base - gw[idx]) <= 1e-9 * (1 + abs(base)), idx


# ---- fast_div ------------------------------------------------------------------------------------------------------------------------------------
def test_fast_div_is_exact_below_2_31():
    """csrc/npm_conv.hip fast_div: floor(n / d) == mulhi(n, mul) >> shift for 0 <= n < 2^31, every d in 1 .. 4096, at the n where a
    too-small or too-large multiplier shows first: just below and at multiples of d, small and close to 2^31."""
    top = 2 ** 31 - 1
    rng = np.random.default_rng(0)
    for d in range(1, 4097):
        mul, shift = CC.fast_div_setup(d)
        assert 0 <= mul < 2 ** 32 and 0 <= shift < 32
        qs = {1, 2, 3, top // d, top // d - 1, (top // d) // 2} | {int(q) for q in rng.integers(1, top // d + 1, size=6)}
        ns = {0, d - 1, d, top} | {q * d - 1 for q in qs if q >= 1} | {q * d for q in qs if q * d <= top}
        for n in ns:
            assert 0 <= n <= top
            assert CC.fast_div(n, d, mul, shift) == n // d, (n, d)
    assert CC.fast_div_setup(1) == (0, 0) and CC.fast_div(12345, 1, 0, 0) == 12345
