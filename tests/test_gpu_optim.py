"""GPU: csrc/npm_optim.hip through the C ABI -- Adam, the MSE / cross-entropy sums and their gradients, npm_mask_scale,
npm_dropout_philox and npm_fill_f64 -- at the sizes where their launches change shape, on unaligned operands, with guards behind
every output.  The cases and checks are those of tests/optim_cases.py, which tests/test_optim_host.py runs on the host simulator;
the models are tests/optim_reference.py.  Nothing here reads the reference: its numbers arrive as tests/golden/adam_steps.npz.

Bounds.
* Adam: both moments bit-equal to the model (fp32 / fp64 multiplies and adds, contraction off).  The parameter bit-equal except
  where the model's fp64 difference lies within 2^-40 |step| + 2^-52 |d| of a float32 rounding boundary -- there an fp64 divide or
  root one ulp off may round it to the other neighbour, so one float32 ulp is allowed; at most 16 such elements per case (the host
  test asserts the count for every case).  Each test prints how many it found and how many of them differ.
* Loss sums: |got - fsum| <= 1e-13 * sum |term|.  From the code: at these sizes a thread adds at most 4 terms serially
  ((seam + 257) / (1024 * 256) rounded up is 2; 4 leaves room), then two 8-level shared-memory trees (the block's, the second pass's)
  and at most 4 serial adds in the second pass: at most 24 additions, 24 * 2^-53 = 2.7e-15 of sum |term|; forming a term rounds at
  most 4 times (the difference is exact in fp64; the square, or the logarithm, its product and the conversion), 4 * 2^-53.  1e-13
  leaves a 30-fold margin and is 10^5 - 10^6 times below what a float32 accumulator reaches (tests/test_optim_host.py shows one
  failing).
* Elementwise outputs (npm_mse_bwd, npm_xent_bwd, npm_mask_scale, the y of npm_dropout_philox): bit-equal to NumPy's float32
  expression; masks byte-equal to Philox4x32-10 as oracle/np_oracle.py evaluates it.
"""

import numpy as np
import pytest

import optim_cases as OC
import optim_reference as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', OC.ADAM_CASES, ids=OC.adam_case_id)
def test_adam_against_the_model(npm, case):
    used = OC.check_adam_case(npm, case)
    print(f'{OC.adam_case_id(case)}: (step, near ties, of those differing) = {used}')


def test_adam_against_the_recorded_reference_steps(npm):
    """The reference's own AdamOptimizer, n = 1031, three steps (tests/golden/adam_steps.npz): the kernel is held to the recorded
    arrays, not only to the restatement."""
    used = OC.check_adam_golden(npm, load_golden('adam_steps'))
    print(f'golden: (step, near ties, of those differing) = {used}')


def test_adam_optimizer_class_on_a_device_parameter(npm):
    """``AdamOptimizer.update`` at 2^20 + 257 elements, two steps: past the grid cap, through the class's own moment buffers."""
    used = OC.check_adam_optimizer_class(npm)
    print(f'AdamOptimizer: (step, near ties, of those differing) = {used}')


def test_encoder_adam_one_launch_equals_sixteen(npm):
    """Encoder d 8, 2 heads, hidden 20, three Adam steps: the one coalesced launch per backward and the 16 per-parameter launches
    (device.COALESCE_UPDATES off) give the same bits in all 16 parameters."""
    OC.check_encoder_adam_coalesced(npm)


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', OC.LOSS_CASES, ids=lambda c: f'n{c[0]}-off{c[1][0]}{c[1][1]}')
def test_loss_sums_against_fsum(npm, case):
    print(f'n={case[0]}: error / bound = {OC.check_loss_sums(npm, case)}')


@pytest.mark.parametrize('case', OC.BWD_CASES, ids=lambda c: f'n{c[0]}-off{"".join(map(str, c[1]))}')
def test_loss_gradients_bitwise(npm, case):
    OC.check_loss_gradients(npm, case)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------
def test_mask_scale_bitwise(npm):
    """Mask bytes from {0, 1, 2, 255}, keep 1.0 / 0.75 / 0.1, the mask at byte offsets 0 .. 3, x / y at float offsets 1 and 3, and
    the sizes around the grid cap."""
    for case in OC.MASK_SCALE_CASES:
        OC.check_mask_scale(npm, case)


def test_dropout_philox_every_branch(npm):
    """n % 4 in all residues x mask byte offsets 0 .. 3 x operand offsets (16-byte branch, scalar branch) and the mask-only call x
    keep 1.0 (threshold 2^32: y == x), 2^-33 (threshold 0: y == 0), 0.75, 0.1, seeds with high words, offsets up to 2^63 + 5."""
    for case in OC.philox_grid():
        OC.check_philox_case(npm, case)
    OC.check_philox_offsets_differ(npm)


def test_dropout_philox_grid_stride_loop(npm):
    """The launch is capped at 2^20 blocks of 256 lanes, so the grid-stride loop starts past 2^28 groups of four: the mask-only call
    at n = 2^30 + 1027 (a 1 GiB byte mask, allocated once and freed before returning; 257 groups take the second pass, the last one
    is odd).  Three 64 KiB windows come back -- the start, across element 2^30 (up to 1024 elements past it), the tail with the
    guard -- and are compared with Philox evaluated for exactly their groups.  The x / y branches past 2^30 elements would need over 9 GB on the device and a host
    reference of that size: left out."""
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    n, window = 2 ** 30 + 1027, 65536
    keep, seed, offset = 0.75, OC.SEEDS[0], 2 ** 32 + 7
    total = n + OC.GUARD
    buf = D.ByteBuffer(total + 3)
    try:
        fill = np.array([0xA5A5A5A5], dtype=np.uint32).view(np.float32)[0]             # every byte the sentinel
        _C.check(lib.npm_fill_f32(buf.ptr, float(fill), (total + 3) // 4), 'npm_fill_f32')
        _C.check(lib.npm_dropout_philox(None, None, buf.ptr, n, keep, seed, offset), 'npm_dropout_philox')
        starts = (0, 2 ** 30 + 1024 - window, (total - window) // 4 * 4)       # n ends 1027 elements past 2^30: the second window ends 1024 past it
        assert all(first % 4 == 0 and 0 <= first and first + window <= total for first in starts)
        got = np.empty([3, window], dtype=np.uint8)
        for row, first in zip(got, starts):
            _C.check(lib.npm_d2h(row.ctypes.data, buf.ptr + first, window), 'npm_d2h')
    finally:
        del buf
        D.trim_pool()
    for row, first in zip(got, starts):
        inside = min(window, n - first)
        want = R.dropout_philox_mask_range(first, inside, keep, seed, offset).astype(np.uint8)
        assert np.array_equal(row[:inside], want), first
        assert (row[inside:] == OC.SENTINEL_BYTE).all(), 'the guard behind the mask was written'
    assert n - starts[2] < window and got[2][:n - starts[2]].max() == 1                # the tail window holds mask bytes and the guard


# ---- npm_fill_f64, argument checks ----------------------------------------------------------------------------------------------------
def test_fill_f64(npm):
    OC.check_fill_f64(npm)


def test_bad_arguments_are_refused(npm):
    OC.check_arguments(npm)
