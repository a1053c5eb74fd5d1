"""GPU: npm_kv_copy_pages_planes (csrc/npm_decode.hip) through the C ABI -- the copy-on-write of a layered key / value cache: the same
(source page, destination page, rows) pairs in every plane of one allocation, in one launch.  Raw bits against NumPy on a
sentinel-filled pool with a guard region behind it (the pattern of tests/test_gpu_fork.py): the valid rows of every destination
page of every plane, and not one other byte.  The entry point does not exist on the parent commit."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 777.0, 1024


@pytest.fixture(scope='module')
def npm():
    import np_modeling_amd
    return np_modeling_amd


@pytest.mark.parametrize('dtype', [np.float32, np.float16])
@pytest.mark.parametrize('n,planes', [(1, 1), (1, 6), (70, 4)])
@pytest.mark.parametrize('page_rows,row_len', [(16, 32), (64, 256), (16, 8)])
def test_the_pairs_are_copied_in_every_plane_and_nothing_else_is_written(npm, dtype, n, planes, page_rows, row_len):
    """rows 0, 1, page_rows - 1 and a whole page, round robin over the pairs; a plane stride with a gap of one page between the pools."""
    from np_modeling_amd import _C, device as D
    rng = np.random.default_rng(n + page_rows + planes)
    pages = 2 * n + 3
    size = np.dtype(dtype).itemsize
    order = rng.permutation(pages)
    src, dst = order[:n], order[n:2 * n]
    rows = np.array([(0, 1, page_rows - 1, page_rows)[(i + n) % 4] for i in range(n)])
    stride = (pages + 1) * page_rows * row_len                       # elements between two planes: the pool and one page of gap
    host = np.full([planes * stride + GUARD * 4 // size], SENTINEL, dtype=dtype)
    pools = host[:planes * stride].reshape(planes, pages + 1, page_rows, row_len)
    pools[:, src] = rng.standard_normal([planes, n, page_rows, row_len]).astype(dtype)
    want = host.copy()
    wpools = want[:planes * stride].reshape(planes, pages + 1, page_rows, row_len)
    for s, d, r in zip(src, dst, rows):
        wpools[:, d, :r] = pools[:, s, :r]
    dev = D.bytes_from_host(host)
    pairs = D.bytes_from_host(np.stack([src, dst, rows]).astype(np.int32))
    _C.check(_C.lib().npm_kv_copy_pages_planes(dev.ptr, page_rows * row_len * size, row_len * size, pairs.ptr, pairs.ptr + 4 * n,
                                               pairs.ptr + 8 * n, n, planes, stride * size), 'npm_kv_copy_pages_planes')
    bits = {2: np.uint16, 4: np.uint32}[size]
    assert np.array_equal(dev.numpy().view(bits), want.view(bits))
    if planes == 1:                                                  # one plane is npm_kv_copy_pages
        again = D.bytes_from_host(host)
        _C.check(_C.lib().npm_kv_copy_pages(again.ptr, page_rows * row_len * size, row_len * size, pairs.ptr, pairs.ptr + 4 * n,
                                            pairs.ptr + 8 * n, n), 'npm_kv_copy_pages')
        assert np.array_equal(again.numpy(), dev.numpy())


def test_empty_calls_launch_nothing_and_bad_arguments_are_refused(npm):
    from np_modeling_amd import _C, device as D
    lib = _C.lib()
    buf = D.full([256 + GUARD], SENTINEL)
    ints = D.bytes_from_host(np.array([0, 1, 1], dtype=np.int32))
    p, i = buf.ptr, ints.ptr
    assert lib.npm_kv_copy_pages_planes(None, 1024, 64, None, None, None, 0, 4, 4096) == 0          # nothing to copy: NPM_OK
    assert lib.npm_kv_copy_pages_planes(p, 512, 0, i, i + 4, i + 8, 1, 1, 512) == 0
    assert lib.npm_kv_copy_pages_planes(p, 512, 64, i, i + 4, i + 8, 1, 0, 512) == 0
    for args in ((None, 512, 64, i, i + 4, i + 8, 1, 1, 1024), (p, 512, 64, None, i + 4, i + 8, 1, 1, 1024),
                 (p, 512, 64, i, i + 4, None, 1, 1, 1024), (p + 4, 512, 64, i, i + 4, i + 8, 1, 1, 1024),
                 (p, 512, 60, i, i + 4, i + 8, 1, 1, 1024), (p, 500, 64, i, i + 4, i + 8, 1, 1, 1024),
                 (p, 32, 64, i, i + 4, i + 8, 1, 1, 1024), (p, 512, 64, i, i + 4, i + 8, -1, 1, 1024),
                 (p, 512, 64, i, i + 4, i + 8, 1, -1, 1024), (p, 512, 64, i, i + 4, i + 8, 1, 2, 1000),
                 (p, 512, 64, i, i + 4, i + 8, 1, 2, 256)):
        assert lib.npm_kv_copy_pages_planes(*args) == 10002, args
    np.testing.assert_array_equal(buf.numpy(), SENTINEL)                                            # nothing was launched
