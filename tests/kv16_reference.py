"""References shared by the tests of the half-precision key / value cache (tests/test_kv16_host.py on the simulator of
tests/hostsim/ (profile 'kv16'), tests/test_gpu_kv16.py on the MI355X): NumPy's own float16 rounding as the definition of what an append
stores, the derived worst-case distance between attention over an fp16 cache and over the fp32 one, the row of edge values, fp16
buffers with guard regions, and the thinned case grid of the bitwise comparison."""

import itertools

import numpy as np

U = 2.0 ** -11                    # unit roundoff of IEEE fp16 (11 significant bits, round to nearest)
SENTINEL16 = 0x5a5a               # the bit pattern rows that nothing addresses, and the guard region, must keep (fp16 210.25)
NAN16, INF16 = 0x7e00, 0x7c00
GUARD16 = 128                     # halves behind every fp16 buffer

# One row of values whose rounding decides something; NumPy's answers (checked on the CPU by tests/test_kv16_host.py):
# the largest finite half, the last float below the overflow threshold, the threshold itself (-> inf), two ties (to even: down,
# up), two subnormal results, the last value that rounds to zero and the first that does not, minus zero, a float32 subnormal.
EDGE_VALUES = np.array([65504.0, 65519.996, 65520.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1e-6, 6e-8, 2.9e-8, 3.1e-8, -0.0, 1e-40,
                        -65520.0, -65519.996, 0.1, -1.0 / 3.0, 2.0 ** -24], dtype=np.float32)
EDGE_BITS = np.array([0x7bff, 0x7bff, 0x7c00, 0x3c00, 0x3c02, 0x0011, 0x0001, 0x0000, 0x0001, 0x8000, 0x0000,
                      0xfc00, 0xfbff, 0x2e66, 0xb555, 0x0001], dtype=np.uint16)


def to_f16(x):
    """What an append stores: IEEE round to nearest even, overflow to inf, subnormal results kept."""
    with np.errstate(over='ignore'):
        return np.asarray(x, dtype=np.float32).astype(np.float16)


def rounded(x):
    """The stored values as float32 (exact)."""
    return to_f16(x).astype(np.float32)


def derived_bound(q, k, v, scale, kernel_bound):
    """Worst-case |ctx16 - ctx32| of one attention whose K / V were rounded to fp16, element-wise relative error at most u each:

        |s16 - s| <= u scale sum_i |q_i| |k_i| =: eps per score, so every softmax weight moves by a factor within exp(+-2 eps)
        (numerator and normaliser by exp(+-eps) each): sum_j |p16_j - p_j| <= expm1(2 eps); and |v16 - v| <= u |v|.  Hence
        |ctx16 - ctx32| <= (expm1(2 eps) + u (1 + expm1(2 eps))) max |v| + the kernel's own error on either side;

    the issue's form drops the second-order term u expm1(2 eps), which this returns as stated: (expm1(2 eps) + u) max|v| +
    ``kernel_bound``.  q [B, T, Hq, D], k / v [B, L, Hkv, D] (the valid rows), float64 inside.  Returns (bound, eps)."""
    q, k, v = (np.asarray(x, dtype=np.float64) for x in (q, k, v))
    hq, hkv = q.shape[2], k.shape[2]
    kk = np.abs(k)[:, :, np.arange(hq) % hkv]                             # query head h reads K / V head h % Hkv
    eps = U * scale * float(np.einsum('bthd,bjhd->bthj', np.abs(q), kk).max())
    return (np.expm1(2 * eps) + U) * float(np.abs(v).max()) + kernel_bound, eps


def half_buffer(shape, fill_bits=SENTINEL16):
    """A device buffer of prod(shape) + GUARD16 halves holding ``fill_bits`` everywhere, the guard region included; (buffer, halves)."""
    from np_modeling_amd import device as D
    n = int(np.prod(shape))
    return D.bytes_from_host(np.full([n + GUARD16], fill_bits, dtype=np.uint16)), n


def upload_halves(values16, pad_bits=SENTINEL16):
    """float16 (or uint16 bit patterns) -> device buffer with a guard region."""
    from np_modeling_amd import device as D
    bits = np.ascontiguousarray(values16).view(np.uint16).ravel()
    return D.bytes_from_host(np.concatenate([bits, np.full([GUARD16], pad_bits, dtype=np.uint16)]))


def paged_table(rng, batch, lmax, page_rows, spare=2):
    """A shuffled block table [B, ceil(lmax / page_rows)] over a pool with ``spare`` unused pages; returns (table, pages)."""
    per = -(-lmax // page_rows)
    pages = batch * per + spare
    return rng.permutation(pages)[:batch * per].reshape(batch, per).astype(np.int32), pages


def to_pages(x, table, page_rows, pages, fill=0.0):
    """x [B, rows, ...] -> pool [pages, page_rows, ...] placed through ``table``; rows past ``rows`` and unused pages: ``fill``."""
    b, rows = x.shape[:2]
    pool = np.full((pages, page_rows) + x.shape[2:], fill, dtype=x.dtype)
    for i in range(b):
        for first in range(0, rows, page_rows):
            take = min(page_rows, rows - first)
            pool[table[i, first // page_rows], :take] = x[i, first:first + take]
    return pool


# ---- the grid of the bitwise comparison (fp16 kernel == fp32 kernel on the rounded values) ------------------------------------------
HEAD_DIMS = (16, 32, 64, 128)
GROUPS = ((8, 8, 1), (6, 2, 1), (8, 1, 2), (4, 4, 17), (8, 2, 8), (2, 1, 16), (3, 3, 3))      # (Hq, Hkv, T): rows 1, 3, 16, 17, 32, 32, 3
GROUP_ROWS = (1, 3, 16, 17, 32)
LENGTHS = (1, 15, 16, 17, 100, 529)
SPLITS = ('one', 'auto', 'many')
LAYOUTS = ('uniform', 'varlen', 'paged16', 'paged64')
NT_MODES = (1, 2)
BATCHES = (1, 3)


def bitwise_cases():
    """(D, Hq, Hkv, T, L, causal, splits, nt, B, layout): every (D, group, L, causal), each with a split mode, a load policy, a
    batch and a layout drawn round robin (not the full product of those four) so that every value of every axis meets the others
    many times; L < T becomes T."""
    out, i = [], 0
    for d, (hq, hkv, t), length, causal in itertools.product(HEAD_DIMS, GROUPS, LENGTHS, (0, 1)):
        out.append((d, hq, hkv, t, max(length, t), causal, SPLITS[(i // 2) % 3], NT_MODES[(i // 6) % 2], BATCHES[(i // 2 + i // 12) % 2],
                    LAYOUTS[(i // 2 + i // 24) % 4]))
        i += 1
    return out


def case_id(c):
    return 'D%d-H%d/%d-T%d-L%d-c%d-%s-nt%d-B%d-%s' % c
