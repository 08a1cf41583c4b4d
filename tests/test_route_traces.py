'''Every route of FlexPipeline, pinned without a GPU: each case of tests/route_trace.py (guide x scheduler x eta x step noise x
request x debug x loop mode x fuse switches) is run on the current code with the library replaced by a recorder and compared,
event for event over the whole request, with tests/golden/route_traces.json (recorded by tests/golden/make_route_goldens.py on
the commit the file names).  Names, integers, the null / address pattern, shapes, types and order are compared exactly; floats
to 1e-6 relative: they are float32 coefficients made by libm calls in float64, which allows about 16 ulp of float32 between
machines, and a coefficient of the wrong step differs in the third digit.'''
import json
import os

import pytest

import route_trace as R

NAMES = ['fd_cfg_ddim_step_f32', 'fd_cfg_ddim_masked_step_f32', 'fd_cfg_ddim_noise_step_f32', 'fd_cfg_multistep_step_f32',
         'fd_cfg_multistep_noise_step_f32', 'fd_cfg_linear_multistep_step_f32', 'fd_cfg_rescale_ddim_step_f32',
         'fd_cfg_rescale_multistep_step_f32', 'fd_composite_step_f32', 'fd_composite_ddim_step_f32',
         'fd_composite_multistep_step_f32', 'fd_composite_linear_multistep_step_f32', 'fd_window_gather_f32',
         'fd_window_step_f32', 'fd_window_ddim_step_f32', 'fd_window_multistep_step_f32', 'scheduler.step', 'noise_pred']


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'route_traces.json')) as f:
        return json.load(f)


def differs(got, want):
    '''None, or a word on the first difference.'''
    if type(got) is not type(want):
        return f'{got!r} is not {want!r}'
    if isinstance(want, list):
        if len(got) != len(want):
            return f'{len(got)} entries for {len(want)}: {got!r} / {want!r}'
        for g, w in zip(got, want):
            d = differs(g, w)
            if d:
                return d if not (want and isinstance(want[0], str)) else f'{d} in {got!r} / {want!r}'
        return None
    if isinstance(want, float):
        return None if abs(got - want) <= 1e-6 * abs(want) else f'{got!r} != {want!r}'
    return None if got == want else f'{got!r} != {want!r}'


def test_every_route_makes_the_recorded_calls(golden):
    events, blocks, traces = golden['events'], golden['blocks'], golden['traces']
    assert golden['steps'] == R.TRACE_STEPS and golden['inner'] == [R.inner_key(i) for i in R.INNER]
    mp, ran, bad = pytest.MonkeyPatch(), 0, []
    cases = R.cases()
    assert sorted(R.outer_key(o) for o, _ in cases) == sorted(golden['cases'])
    for outer, inner in cases:
        row = golden['cases'][R.outer_key(outer)]
        assert len(row) == len(inner)
        for i, index in zip(inner, row):
            want = [[events[e] for e in blocks[b]] for b in traces[index]]
            d = differs(json.loads(json.dumps(R.run_case(mp, outer, i))), want)
            ran += 1
            if d:
                bad.append(f'{R.outer_key(outer)}/{R.inner_key(i)}: {d}')
    assert not bad, f'{len(bad)} of {ran} cases differ:\n' + '\n'.join(bad[:20])
    # no case is left out
    assert ran == golden['case_count'] == sum(len(i) for _, i in cases)


def test_the_fixture_reaches_every_launch(golden):
    seen = {e[0] for e in golden['events']}
    assert not [n for n in NAMES if n not in seen]
    assert not [e for e in golden['events'] if e[0] == 'raises']


def test_every_loop_is_reached(monkeypatch):
    '''Every value of `Route.loop` is the route of some case (one request per outer key and loop mode is enough to see it).'''
    from flexdiffuse_amd.pipeline import flex, route
    seen, select = set(), route.select_route

    def recording_select(*a, **k):
        r = select(*a, **k)
        seen.add(r.loop)
        return r
    monkeypatch.setattr(flex, 'select_route', recording_select)
    for outer, inner in R.cases():
        for i in inner:
            if i[:3] == (True, 'txt2img', False):
                R.run_case(monkeypatch, outer, i)
    assert seen == {'ddim', 'multistep', 'linear', 'window', 'planned', 'window_planned', 'generic'}
