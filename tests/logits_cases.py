"""TEST INFRASTRUCTURE ONLY -- the cases of npm_logits_process shared by tests/test_logits_host.py (host simulator) and
tests/test_gpu_logits.py (device), and the runner that calls the entry point through np_modeling_amd._C on whatever library is
installed and compares the WHOLE padded logit buffer, guard words and pitch padding included, with tests/logits_reference.py.

A case is a dict: batch, rows, vocab, logits [batch * rows, vocab] float32, and the entry point's arguments as host arrays (None:
a NULL pointer) -- history (a list of int arrays, one per slot), history_len, history_cap, history_pitch, prompt_len, draft
[batch, rows - 1], n_draft, active, repetition, presence, frequency, eos, min_new, bias_index / bias_value [batch, bias_cap],
bias_count, bias_cap.  The default parameters make every step inexact: repetition 1.3, frequency 0.1, presence 0.7.
"""

import ctypes as C

import numpy as np

import logits_reference as LR

SENTINEL = 0x5A5A5A5A                  # a finite float: a guard or padding word that changes is seen as bits
NAN_BITS = 0x7FC00000                  # what the rows of an inactive slot are filled with
FRONT, BACK = 5, 8                     # guard words: FRONT = 5 puts the logits 4 bytes off 16-byte alignment (0: aligned)
LENGTHS = (0, 1, 63, 64, 65, 1023, 1025, 5000)


def make(batch, rows, vocab, seed, lengths, cap=None, alphabet=50, scale=3.0):
    """A random case: histories over a small alphabet (so that tokens repeat), drafts from the same alphabet with -1 behind
    n_draft, inexact penalties, an eos from the alphabet with min_new 0 (no rule), no bias list."""
    rng = np.random.default_rng(seed)
    letters = rng.choice(vocab, size=min(alphabet, vocab), replace=False)
    history = [letters[rng.integers(0, letters.size, size=n)].astype(np.int32) for n in lengths]
    n_draft = rng.integers(0, rows, size=batch).astype(np.int32)
    draft = letters[rng.integers(0, letters.size, size=[batch, rows - 1])].astype(np.int32)
    draft[np.arange(rows - 1)[None, :] >= n_draft[:, None]] = -1
    cap = max(max(lengths), 1) if cap is None else cap
    return dict(batch=batch, rows=rows, vocab=vocab, logits=(scale * rng.standard_normal([batch * rows, vocab])).astype(np.float32),
                history=history, history_len=np.array(lengths, dtype=np.int32), history_cap=cap, history_pitch=cap + 2,
                prompt_len=np.array([n // 3 for n in lengths], dtype=np.int32), draft=draft, n_draft=n_draft, active=None,
                repetition=np.full([batch], 1.3, dtype=np.float32), presence=np.full([batch], 0.7, dtype=np.float32),
                frequency=np.full([batch], 0.1, dtype=np.float32), eos=letters[rng.integers(0, letters.size, size=batch)].astype(np.int32),
                min_new=np.zeros([batch], dtype=np.int32), bias_index=None, bias_value=None, bias_count=None, bias_cap=0,
                pitch=vocab + 3, front=FRONT)


def with_bias(case, lists):
    """``lists``: per slot [(index, value), ...]; bias_cap is the longest (at least 1)."""
    cap = max(1, max(len(entries) for entries in lists))
    case['bias_cap'] = cap
    case['bias_index'] = np.full([case['batch'], cap], -7, dtype=np.int32)
    case['bias_value'] = np.full([case['batch'], cap], 9.5, dtype=np.float32)
    case['bias_count'] = np.array([len(entries) for entries in lists], dtype=np.int32)
    for b, entries in enumerate(lists):
        for j, (index, value) in enumerate(entries):
            case['bias_index'][b, j], case['bias_value'][b, j] = index, value
    return case


def shapes(vocab):
    """Three slots of four rows at a small vocabulary: penalties, drafts, a bias list per slot, an eos rule that ends inside the
    chunk, and a fourth, neutral slot."""
    case = make(4, 4, vocab, 100 + vocab, [40, 7, 0, 12])
    rng = np.random.default_rng(vocab)
    case['min_new'][:] = (case['history_len'] - case['prompt_len']) + np.array([2, 0, 5, 9])
    with_bias(case, [[(int(i), float(v)) for i, v in zip(rng.choice(vocab, size=min(5, vocab), replace=False), rng.standard_normal(5))],
                     [(int(case['history'][1][0]), -np.inf)], [], []])
    case['repetition'][3], case['presence'][3], case['frequency'][3], case['eos'][3] = 1.0, 0.0, 0.0, -1
    return case


def large_vocab():
    """V 128256, two slots: the workspace indices pass 2^16 and 2^17."""
    case = make(2, 1, 128256, 7, [300, 200], alphabet=150)
    ids = np.array([65535, 65536, 65537, 131071, 131072, 131073, 128255, 0])
    case['history'][0][:8], case['history'][1][:8] = ids, ids[::-1]
    return with_bias(case, [[(128255, -np.inf), (70000, 0.3)], [(131072, 1.7)]])


def one_length(length):
    """Two slots whose history is exactly as long as the capacity."""
    return make(2, 1, 1000, 200 + length, [length, length], cap=max(length, 1))


def all_lengths():
    """Every length of LENGTHS in one call, the capacity above all of them."""
    return make(len(LENGTHS), 1, 1000, 300, list(LENGTHS), cap=5003)


def clipped_lengths():
    """history_len below 0 and above the capacity: read as 0 and as the capacity."""
    case = make(3, 2, 257, 400, [30, 30, 30])
    case['history_len'] = np.array([-5, 37, 30], dtype=np.int32)
    case['prompt_len'] = np.array([3, 10, -4], dtype=np.int32)
    return case


def contents():
    """One token 5000 times; every token once; random int32 with negatives and ids >= vocab (ignored)."""
    case = make(3, 1, 1000, 500, [5000, 1000, 5000])
    rng = np.random.default_rng(501)
    case['history'][0][:] = 123
    case['history'][1] = rng.permutation(1000).astype(np.int32)
    noise = rng.integers(-2 ** 31, 2 ** 31, size=5000, dtype=np.int64)
    noise[::3] = rng.integers(-3, 1003, size=noise[::3].size)
    case['history'][2] = noise.astype(np.int32)
    case['prompt_len'][:] = [100, 0, 2500]
    return case


def prompts():
    """prompt_len 0, inside the sequence, equal to L and above L over the same history."""
    case = make(4, 2, 257, 600, [64] * 4)
    case['history'] = [case['history'][0]] * 4
    case['prompt_len'] = np.array([0, 31, 64, 90], dtype=np.int32)
    return case


def drafts(rows):
    """Drafts that repeat history tokens and each other, with -1 tails; n_draft -1, 0, rows - 1 and above."""
    case = make(4, rows, 257, 700 + rows, [20, 20, 20, 20], alphabet=6)
    case['n_draft'] = np.array([-1, 0, rows - 1, rows + 5], dtype=np.int32)
    if rows > 1:
        case['draft'][2, :] = case['history'][2][np.arange(rows - 1) % 3]        # repeats the history and itself
        case['draft'][3, 1:] = -1
        case['draft'][3, -1] = 2 ** 31 - 1
    case['min_new'][:] = (case['history_len'] - case['prompt_len']) + 2
    return case


def inactive():
    case = make(4, 3, 63, 800, [10, 10, 10, 10])
    case['active'] = np.array([1, 0, 5, 0], dtype=np.int32)
    case['n_draft'] = np.array([2, 2, -1, -3], dtype=np.int32)
    return case


def bias_lists():
    """Empty; one entry; 256 entries; -inf entries; indices outside the vocabulary; a duplicate index (the first entry counts);
    an entry on a token that is in the history and is eos."""
    case = make(6, 2, 1000, 900, [30] * 6)
    rng = np.random.default_rng(901)
    shared = int(case['history'][5][-1])
    case['eos'][5], case['min_new'][5] = shared, 30 - case['prompt_len'][5] + 1          # row 0 banned, row 1 not
    lists = [[], [(int(case['history'][1][3]), 0.37)],
             [(int(i), float(v)) for i, v in zip(rng.permutation(1000)[:256], rng.standard_normal(256))],
             [(5, -np.inf), (int(case['history'][3][0]), -np.inf), (999, 1.25)],
             [(-1, 3.0), (1000, 3.0), (2 ** 31 - 1, 3.0), (-2 ** 31, 3.0), (17, 0.1), (17, 5.0), (18, 0.2)],
             [(shared, 0.9)]]
    case['n_draft'][:] = 1
    return with_bias(case, lists)


def minimum_length():
    """gen_r crosses min_new between two rows of a chunk; min_new exactly gen_0; eos outside the vocabulary."""
    case = make(4, 4, 63, 1000, [9, 9, 9, 9])
    case['prompt_len'][:] = 7                                                            # gen_0 = 2
    case['n_draft'][:] = 3
    case['draft'] = np.abs(case['draft']) % 63
    case['min_new'] = np.array([4, 2, 100, 100], dtype=np.int32)
    case['eos'] = np.array([11, 11, 63, -1], dtype=np.int32)
    case['repetition'][:], case['presence'][:], case['frequency'][:] = 1.0, 0.0, 0.0    # the rule alone
    return case


def special_values():
    """Rows holding -inf, +-0.0, NaN and +inf at tokens the steps touch: IEEE passes them through."""
    case = make(2, 2, 63, 1100, [16, 16], alphabet=8)
    values = np.array([-np.inf, 0.0, -0.0, np.nan, np.inf, 1e38, -1e38, 1e-45], dtype=np.float32)
    for b in range(2):
        tokens = np.unique(case['history'][b])
        for r in range(2):
            case['logits'][b * 2 + r, tokens] = values[(np.arange(tokens.size) + r) % values.size]
    case['repetition'][1] = 0.75
    return with_bias(case, [[(int(case['history'][0][0]), 2.5)], [(int(case['history'][1][1]), -np.inf), (3, 0.5)]])


CASES = {f'shapes-V{v}': (lambda v=v: shapes(v)) for v in (1, 63, 257, 1000)}
CASES.update({f'length-{n}': (lambda n=n: one_length(n)) for n in LENGTHS})
CASES.update({'large-vocab': large_vocab, 'all-lengths': all_lengths, 'clipped-lengths': clipped_lengths, 'contents': contents,
              'prompts': prompts, 'drafts-rows1': lambda: drafts(1), 'drafts-rows4': lambda: drafts(4), 'drafts-rows8': lambda: drafts(8),
              'inactive': inactive, 'bias-lists': bias_lists, 'minimum-length': minimum_length, 'special-values': special_values})


PER_SLOT = ('history_len', 'prompt_len', 'n_draft', 'active', 'repetition', 'presence', 'frequency', 'eos', 'min_new', 'bias_index',
            'bias_value', 'bias_count', 'draft')


def slot_of(case, b):
    """Slot b of the case as a batch-1 case."""
    rows = case['rows']
    out = dict(case, batch=1, logits=case['logits'][b * rows:(b + 1) * rows].copy(), history=[case['history'][b]])
    for key in PER_SLOT:
        if case[key] is not None:
            out[key] = case[key][b:b + 1].copy()
    return out


def row_of(case, b, r):
    """Row r of slot b as a rows = 1 case of its own: draft[b, :r] appended to the history."""
    one = slot_of(case, b)
    length = LR.clip(one['history_len'][0], 0, case['history_cap'])
    prompt = LR.clip(one['prompt_len'][0], 0, length)
    line = np.concatenate([history_array(one)[0, :length], case['draft'][b, :r]]).astype(np.int32)
    cap = max(line.size, 1)
    return dict(one, rows=1, logits=one['logits'][r:r + 1].copy(), history=[line], history_len=np.array([line.size], dtype=np.int32),
                history_cap=cap, history_pitch=cap, prompt_len=np.array([prompt], dtype=np.int32), draft=np.zeros([1, 0], dtype=np.int32),
                n_draft=None)


def body(case, image):
    """The [batch * rows, vocab] logits inside an image, as uint32."""
    n = case['batch'] * case['rows']
    return image[case['front']:case['front'] + n * case['pitch']].reshape(n, case['pitch'])[:, :case['vocab']]


def live_slots(case):
    return [b for b in range(case['batch']) if (case['active'] is None or case['active'][b] != 0)
            and (case['n_draft'] is None or case['n_draft'][b] >= 0)]


def history_array(case):
    """[batch, history_pitch] int32 with the slots' tokens in front and a filler behind them."""
    lines = np.full([case['batch'], case['history_pitch']], -77, dtype=np.int32)
    for b, line in enumerate(case['history']):
        lines[b, :min(len(line), case['history_pitch'])] = line[:case['history_pitch']]
    return lines


def host_image(case):
    """The padded logit buffer as uint32 words: guards, the rows with their pitch padding, guards; inactive slots NaN."""
    rows, vocab, pitch = case['rows'], case['vocab'], case['pitch']
    n = case['batch'] * rows
    image = np.full([case['front'] + n * pitch + BACK], SENTINEL, dtype=np.uint32)
    body = image[case['front']:case['front'] + n * pitch].reshape(n, pitch)
    body[:, :vocab] = case['logits'].view(np.uint32)
    live = live_slots(case)
    for b in range(case['batch']):
        if b not in live:
            body[b * rows:(b + 1) * rows, :vocab] = NAN_BITS
    return image


def expected(case):
    """(the image after the call, which of its words a step applied to) from the reference."""
    image = host_image(case)
    n, pitch = case['batch'] * case['rows'], case['pitch']
    z = image[case['front']:case['front'] + n * pitch].view(np.float32).reshape(n, pitch)
    keys = ('history_len', 'history_cap', 'prompt_len', 'draft', 'n_draft', 'active', 'repetition', 'presence', 'frequency', 'eos',
            'min_new', 'bias_index', 'bias_value', 'bias_count', 'bias_cap')
    done = LR.process(z, case['batch'], case['rows'], case['vocab'], history=None if case['history'] is None else history_array(case),
                      **{k: case[k] for k in keys})
    written = np.zeros(image.shape, dtype=bool)
    written[case['front']:case['front'] + n * pitch] = done.reshape(-1)
    return image, written


def _upload(D, value, dtype):
    """(buffer, address) of a host array between two guard words, or (None, None)."""
    if value is None:
        return None, None
    host = np.concatenate([[SENTINEL], np.ascontiguousarray(value, dtype=dtype).reshape(-1).view(np.uint32), [SENTINEL]]).astype(np.uint32)
    buf = D.bytes_from_host(host)
    return buf, buf.ptr + 4


def run(case, expect=0):
    """One npm_logits_process on the case; returns the logit image after the call (uint32).  Asserts the return code, that every
    input array and its guard words kept their bits, and that the workspace (between guard words) is all zero afterwards."""
    from np_modeling_amd import _C
    from np_modeling_amd import device as D
    batch, rows, vocab = case['batch'], case['rows'], case['vocab']
    logits = D.bytes_from_host(host_image(case))
    workspace = D.bytes_from_host(np.concatenate([[SENTINEL], np.zeros([batch * vocab], dtype=np.uint32), [SENTINEL]]).astype(np.uint32))
    inputs = dict(history=(None if case['history'] is None else history_array(case), np.int32), history_len=(case['history_len'], np.int32),
                  prompt_len=(case['prompt_len'], np.int32), draft=(case['draft'] if rows > 1 else None, np.int32),
                  n_draft=(case['n_draft'], np.int32), active=(case['active'], np.int32), repetition=(case['repetition'], np.float32),
                  presence=(case['presence'], np.float32), frequency=(case['frequency'], np.float32), eos=(case['eos'], np.int32),
                  min_new=(case['min_new'], np.int32), bias_index=(case['bias_index'], np.int32), bias_value=(case['bias_value'], np.float32),
                  bias_count=(case['bias_count'], np.int32))
    held = {name: _upload(D, value, dtype) for name, (value, dtype) in inputs.items()}
    before = {name: buf.numpy().copy() for name, (buf, _) in held.items() if buf is not None}
    desc = _C.npm_logits(logits=logits.ptr + 4 * case['front'], pitch=case['pitch'], batch=batch, rows=rows, vocab=vocab,
                         history_cap=case['history_cap'], history_pitch=case['history_pitch'], draft_pitch=max(rows - 1, 0),
                         bias_cap=case['bias_cap'], workspace=workspace.ptr + 4, **{name: ptr for name, (_, ptr) in held.items()})
    assert _C.lib().npm_logits_process(C.byref(desc)) == expect
    after = workspace.numpy().view(np.uint32)
    assert after[0] == SENTINEL and after[-1] == SENTINEL, 'a guard word next to the workspace was written'
    assert not after[1:-1].any(), 'the workspace is not all zero after the call'
    for name, image in before.items():
        assert np.array_equal(held[name][0].numpy(), image), f'{name} (or a guard word next to it) was written'
    return logits.numpy().view(np.uint32)


def check(case):
    """Run the case and compare the whole image with the reference; returns the image."""
    want, written = expected(case)
    got = run(case)
    assert LR.same(got.view(np.float32), want.view(np.float32), written), \
        f'{int((got != want).sum())} words differ, first at {np.nonzero(got != want)[0][:8].tolist()} (front {case["front"]}, pitch {case["pitch"]})'
    return got
