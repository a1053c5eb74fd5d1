"""CPU: every scenario of tests/transformer_trace_cases.py asks of the library, call for call and argument for argument, what
tests/golden/transformer_traces.json recorded before layers/transformer.py became one walk over residual blocks and
layers/attentions.py one in-projection -- and returns the same bits: outputs, input gradients, updated parameters, arena
offsets, collectives and flushed ranges.  The file is not regenerated when the layers change: a difference here is a change of
the order of effects, of an argument, or of the arithmetic."""

import json

import pytest

import transformer_trace_cases as TC

with open(TC.GOLDEN) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize('name', list(TC.SCENARIOS))
def test_scenario_equals_the_recorded_trace(name):
    got, want = json.loads(json.dumps(TC.run(name))), GOLDEN[name]
    assert [p['label'] for p in got['phases']] == [p['label'] for p in want['phases']]
    for g, w in zip(got['phases'], want['phases']):
        assert g['calls'] == w['calls'], g['label']
        assert g.get('records') == w.get('records'), g['label']
        assert g['sha256'] == w['sha256'], f'{g["label"]}: same entry points, other arguments'
    for key in want:
        assert got[key] == want[key], key
    assert got.keys() == want.keys()


def test_scenarios_cover_what_they_claim():
    """Read from the RECORDED runs (what the layers reported of themselves), so that an edit of the scenario list cannot hollow
    the fixture out silently."""
    assert set(GOLDEN) == set(TC.SCENARIOS)
    took = {tag for trace in GOLDEN.values() for tag in trace['took']}
    for kind in ('encoder', 'decoder'):
        for order in ('pre', 'post'):
            for composition in ('fused', 'unfused'):
                assert f'{kind} {order} {composition}' in took
    assert {'path decode', 'path fused_masked', 'path gemm', 'self decode', 'cross decode'} <= took
    assert {'packed', 'unpacked', 'core', 'gemm composition'} <= took
    backwards = [name for name, trace in GOLDEN.items() if trace['collectives']]
    assert set(backwards) >= {name for name in GOLDEN if name.startswith(('encoder ', 'decoder '))}
    assert all(len(f) == c for name in backwards for f, c in zip(GOLDEN[name]['flushed'], GOLDEN[name]['collectives']))
    assert all(GOLDEN[name]['phases'][-1].get('records') for name in TC.KEEP_RECORDS)
