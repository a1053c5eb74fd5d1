"""CPU: the launch plan of the row kernels (np_modeling_amd/csrc/npm_row_plan.h) as a host program sees it.

The header is plain C++17, so a stand-alone program includes it, computes the plan of every case below and prints it; the
expectations are literals taken from the routing table in the header's comment, never computed by the code under test.  Which
instance a call ran changes speed and nothing else, so this is where the routing is pinned.

A plan prints as ``vpl HINT grid`` (vpl 0 = the generic kernel), or ``vpl HINT refused`` when the row blocks do not fit a grid.
All cases: 256 CUs; 4 blocks per CU, NPM_TUNE_LN_NT_SPLIT = 5 and NPM_TUNE_STREAM_NT on unless the case says otherwise."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'np_modeling_amd', 'csrc')

SOFTMAX, NORM_FWD, NORM_BWD, DROPOUT_FWD, DROPOUT_BWD = 'SOFTMAX', 'NORM_FWD', 'NORM_BWD', 'DROPOUT_FWD', 'DROPOUT_BWD'
KINDS = (SOFTMAX, NORM_FWD, NORM_BWD, DROPOUT_FWD, DROPOUT_BWD)
CAPPED = (NORM_BWD, DROPOUT_BWD)


def case(kind, rows, d, want, aligned=True, knob=5, stream=True, blocks_per_cu=4):
    return (kind, rows, d, aligned, knob, stream, blocks_per_cu), want


def per_kind(rows, d, wants, **kw):
    return [case(kind, rows, d, want, **kw) for kind, want in zip(KINDS, wants)]


# register width by row length, below the 32 MB threshold: 8 rows = 2 row blocks
WIDTHS = [case(NORM_FWD, 8, d, '%d PLAIN 2' % vpl) for d, vpl in
          [(4, 1), (256, 1), (260, 2), (512, 2), (516, 4), (640, 4), (1024, 4), (1028, 8), (2048, 8), (2052, 16), (4096, 16)]]

# the generic kernels: d % 4 != 0, d > 4096, or operands that miss the alignment; never a hint, however large the tensor
GENERIC = ([case(NORM_FWD, 8, d, '0 PLAIN 2') for d in (33, 1001, 4100)] +
           [case(NORM_FWD, 8, 640, '0 PLAIN 2', aligned=False),
            case(NORM_FWD, 8192, 1024, '0 PLAIN 2048', aligned=False),
            case(SOFTMAX, 16384, 1001, '0 PLAIN 4096'),
            case(NORM_BWD, 8192, 1024, '0 PLAIN 2048', aligned=False)])

# 4 * rows * d against 2^25 bytes, one row below and at it (13107 * 640 * 4 = 33553920, 13108 * 640 * 4 = 33556480)
THRESHOLD = [case(SOFTMAX, 32767, 256, '1 PLAIN 8192'), case(SOFTMAX, 32768, 256, '1 BOTH 8192'),
             case(SOFTMAX, 8191, 1024, '4 PLAIN 2048'), case(SOFTMAX, 8192, 1024, '4 BOTH 2048'),
             case(SOFTMAX, 2047, 4096, '16 PLAIN 512'), case(SOFTMAX, 2048, 4096, '16 BOTH 512'),
             case(SOFTMAX, 13107, 640, '4 PLAIN 3277'), case(SOFTMAX, 13108, 640, '4 BOTH 3277'),
             case(NORM_FWD, 8191, 1024, '4 PLAIN 2048'), case(NORM_FWD, 8192, 1024, '4 LOADS 2048'),
             case(NORM_BWD, 13107, 640, '4 PLAIN 1024'), case(NORM_BWD, 13108, 640, '4 LOADS 1024')]

# NPM_TUNE_LN_NT_SPLIT = backward mode + 4 * forward mode at d = 640, 13108 rows (3277 row blocks, capped to 4 * 256 = 1024);
# per value the hint of NORM_FWD, NORM_BWD, DROPOUT_FWD, DROPOUT_BWD.  3 (backward mode 3) and 12 (forward mode 3) are undocumented.
KNOB_HINTS = {0: ('BOTH', 'BOTH', 'BOTH', 'BOTH'),
              1: ('BOTH', 'LOADS', 'BOTH', 'LOADS'),
              2: ('BOTH', 'STORES', 'BOTH', 'BOTH'),
              4: ('LOADS', 'BOTH', 'LOADS', 'BOTH'),
              5: ('LOADS', 'LOADS', 'LOADS', 'LOADS'),
              6: ('LOADS', 'STORES', 'LOADS', 'BOTH'),
              8: ('STORES', 'BOTH', 'BOTH', 'BOTH'),
              9: ('STORES', 'LOADS', 'BOTH', 'LOADS'),
              10: ('STORES', 'STORES', 'BOTH', 'BOTH'),
              3: ('BOTH', 'BOTH', 'BOTH', 'BOTH'),
              12: ('STORES', 'BOTH', 'BOTH', 'BOTH')}
KNOBS = []
for _knob, (_fwd, _bwd, _dfwd, _dbwd) in KNOB_HINTS.items():
    KNOBS += per_kind(13108, 640, ['4 BOTH 3277', '4 %s 3277' % _fwd, '4 %s 1024' % _bwd, '4 %s 3277' % _dfwd, '4 %s 1024' % _dbwd],
                      knob=_knob)
# NPM_TUNE_STREAM_NT off: no hint anywhere
KNOBS += per_kind(13108, 640, ['4 PLAIN 3277', '4 PLAIN 3277', '4 PLAIN 1024', '4 PLAIN 3277', '4 PLAIN 1024'], stream=False)
KNOBS += per_kind(8192, 1028, ['8 PLAIN 2048', '8 PLAIN 2048', '8 PLAIN 1024', '8 PLAIN 2048', '8 PLAIN 1024'], stream=False)

# every kind above the threshold: the split at d = 640 and 1024 only, under the default (5) and with the stores modes (10)
KINDS_NT = (per_kind(13108, 640, ['4 BOTH 3277', '4 LOADS 3277', '4 LOADS 1024', '4 LOADS 3277', '4 LOADS 1024']) +
            per_kind(8192, 1024, ['4 BOTH 2048', '4 LOADS 2048', '4 LOADS 1024', '4 LOADS 2048', '4 LOADS 1024']) +
            per_kind(8192, 1024, ['4 BOTH 2048', '4 STORES 2048', '4 STORES 1024', '4 BOTH 2048', '4 BOTH 1024'], knob=10) +
            per_kind(16384, 512, ['2 BOTH 4096', '2 BOTH 4096', '2 BOTH 1024', '2 BOTH 4096', '2 BOTH 1024']) +
            per_kind(16384, 512, ['2 BOTH 4096', '2 BOTH 4096', '2 BOTH 1024', '2 BOTH 4096', '2 BOTH 1024'], knob=10) +
            per_kind(8192, 1028, ['8 BOTH 2048', '8 BOTH 2048', '8 BOTH 1024', '8 BOTH 2048', '8 BOTH 1024']) +
            per_kind(8192, 1028, ['8 BOTH 2048', '8 BOTH 2048', '8 BOTH 1024', '8 BOTH 2048', '8 BOTH 1024'], knob=10))

# grids at d = 64: ceil(rows / 4), on the fast backwards capped to blocks per CU x 256; the generic backward is not capped
GRIDS = []
for _rows, _free, _cap in [(1, 1, 1), (4, 1, 1), (5, 2, 2), (4096, 1024, 1024), (4097, 1025, 1024)]:
    GRIDS += [case(kind, _rows, 64, '1 PLAIN %d' % (_cap if kind in CAPPED else _free)) for kind in KINDS]
GRIDS += [case(kind, 4097, 64, '1 PLAIN %d' % (256 if kind in CAPPED else 1025), blocks_per_cu=1) for kind in KINDS]
GRIDS += [case(NORM_BWD, 4097, 33, '0 PLAIN 1025'), case(NORM_BWD, 4097, 33, '0 PLAIN 1025', blocks_per_cu=1)]

# 2^31 row blocks do not fit a grid: 2^33 - 4 rows are 2^31 - 1 blocks, one row more is 2^31; the capped grids take both
LIMIT = []
for _rows, _free in [(2 ** 33 - 4, '2147483647'), (2 ** 33 - 3, 'refused')]:
    LIMIT += [case(kind, _rows, 64, '1 BOTH ' + _free) for kind in (SOFTMAX, NORM_FWD, DROPOUT_FWD)]
    LIMIT += [case(kind, _rows, 64, '1 BOTH 1024') for kind in CAPPED]
    LIMIT += [case(kind, _rows, 33, '0 PLAIN ' + _free) for kind in (SOFTMAX, NORM_FWD, NORM_BWD)]

GROUPS = dict(widths=WIDTHS, generic=GENERIC, threshold=THRESHOLD, knobs=KNOBS, kinds=KINDS_NT, grids=GRIDS, limit=LIMIT)

PROGRAM = r'''#include <cstdio>
#include "npm_row_plan.h"
static void show(npm::RowKind kind, long long rows, long long d, bool aligned, int knob, bool stream, int blocks_per_cu) {
    const npm::RowPlan p = npm::row_plan(kind, rows, d, aligned, knob, stream, blocks_per_cu, 256);
    static const char *const hints[] = {"PLAIN", "BOTH", "LOADS", "STORES"};
    if (p.fits) std::printf("%d %s %d\n", p.vpl, hints[(int)p.hint], p.grid);
    else std::printf("%d %s refused\n", p.vpl, hints[(int)p.hint]);
}
int main() {
@CALLS@    return 0;
}
'''


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    """Every case's printed plan, keyed by its inputs: one compile and one run for the module."""
    cxx = shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    inputs = [inp for group in GROUPS.values() for inp, _ in group]
    calls = ''.join('    show(npm::RowKind::%s, %dLL, %dLL, %s, %d, %s, %d);\n' %
                    (kind, rows, d, str(aligned).lower(), knob, str(stream).lower(), bpc)
                    for kind, rows, d, aligned, knob, stream, bpc in inputs)
    tmp = tmp_path_factory.mktemp('row_plan')
    src, exe = str(tmp / 'row_plan.cpp'), str(tmp / 'row_plan')
    with open(src, 'w') as f:
        f.write(PROGRAM.replace('@CALLS@', calls))
    subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, src, '-o', exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(inputs)
    return dict(zip(inputs, lines))


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_row_plan(plans, group):
    got = {inp: plans[inp] for inp, _ in GROUPS[group]}
    assert got == dict(GROUPS[group])

