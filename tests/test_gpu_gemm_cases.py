'''fd_gemm_f16 through the C ABI on every launch target of the 2-barrier family (csrc/gemm.hip): the case table of tests/gemm_cases.py --
every tile id with each epilogue launch_epi can give it, linear and implicit-GEMM convolution, plain and transposed stores, the one-shot
and the persistent kernel, split-K through both finish kernels -- against a float64 reference of the same rounded operands, with a
per-element bound and a bit-for-bit check of everything around the output; what the ABI refuses; and the FD_GEMM_* / FD_CONV_TAPFAST
arms, each in a fresh process (FD_GEMM_PP only moves the rule, and the cases force their tiles: it has no arm here).  Needs an MI355X; the
whole file takes about two minutes there (109 s measured: 1391 scored launches, 493 in this process and the rest in the eight children), the largest case 0.5 s.'''
import json
import os
import subprocess
import sys

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_device_error = []          # a launch that ended in anything but FD_OK / ValueError: nothing more is started on the device


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _guarded(fn):
    if _device_error:
        pytest.fail(f'not started: {_device_error[0]} ended in a device error')
    try:
        return fn()
    except ValueError:
        raise
    except Exception as e:      # a HIP error is sticky: the cases behind it would only repeat it
        _device_error.append(repr(e)[:200])
        raise


GOOD = G.BY_ID['t10-lin-plain']


@pytest.mark.parametrize('case', G.CASES, ids=[c.id for c in G.CASES])
def test_gemm_case(dev, case):
    '''One launch per case.  Bounds (gemm_cases.check / stats_check): |err| <= 3e-3 + 3e-3 |want| on every element of an fp16 output, 1e-3 + 1e-3 |want|
    of an fp32 one; ln_stats_out / gn_part_out against float64 sums of the stored fp16 rows within what fp32 summation allows.  Every output
    buffer is filled with a sentinel first: an unwritten element fails the bound, a write into padding columns, guard rows or batch gaps
    fails the bit-for-bit comparison.  A refused case must answer ValueError, and a good call must follow it.
    The kernel name printed is PREDICTED by gemm_cases.expected_launch (fd_gemm_plan's tile and split, the restated launch_epi /
    launch_mode), not observed on the device: tests/test_gemm_cases.py holds the restatement against the source of csrc/gemm.hip.'''
    if G.refused(case):
        with pytest.raises(ValueError):
            _guarded(lambda: G.run_on_device(case, dev))
        row = _guarded(lambda: G.run_and_score(GOOD, dev))
        assert row['ok'], row
        return
    row = _guarded(lambda: G.run_and_score(case, dev))
    L = G.expected_launch(case)
    print(f"{L.kernel}{L.tpl}{' + ' + L.finish if L.finish else ''}  {case.id}  err / bound = {row['ratio']:.4f}" +
          (f"  statistics err / bound = {row['stats_ratio']:.4f}" if case.stats_out or case.gn_parts else ''))
    assert row['ratio'] <= 1.0, f"{L.kernel}{L.tpl}: worst error is {row['ratio']:.3g} x the bound"
    assert row['stats_ratio'] <= 1.0, f"{L.kernel}{L.tpl}: the statistics' worst error is {row['stats_ratio']:.3g} x the bound"
    assert row['untouched'], f'{L.kernel}{L.tpl} wrote outside its output, or into an input ({case.layout})'


_child_failed = []


@pytest.mark.parametrize('env', G.ENV_SETTINGS, ids=['-'.join(f'{k}={v}' for k, v in e.items()) for e in G.ENV_SETTINGS])
def test_gemm_ab_switches(env):
    '''The library reads each switch once per process, so each setting gets one fresh interpreter that runs every table case whose expected
    launch the setting changes, and every case that the setting makes the library refuse (of the large persistent walks two), each refusal
    followed by a good call, and prints one JSON line.  One child at a time, each
    under its own timeout; after a child that did not exit cleanly no further child is started.'''
    if _child_failed or _device_error:
        pytest.fail(f'not started: {(_child_failed or _device_error)[0]} did not end cleanly')
    expect, skipped = G.child_cases(env)
    assert expect, f'{env} changes no case of the table'
    walks = [c for c in skipped if G.expected_launch(c).form == 'dmap']
    refuse = [c for c in skipped if c not in walks] + walks[:2]     # (a refusal comes before any look at the data: two of the large walks do)
    good = min(expect, key=lambda c: c.batch * c.M * c.N * (c.K + c.K2))
    child_env = dict(os.environ, **env)
    child_env['PYTHONPATH'] = os.pathsep.join([ROOT] + [p for p in child_env.get('PYTHONPATH', '').split(os.pathsep) if p])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'gemm_cases.py'), '--child',
                            json.dumps({'env': env, 'run': [c.id for c in expect], 'refuse': [c.id for c in refuse], 'good': good.id})],
                           env=child_env, capture_output=True, timeout=900)
    except subprocess.TimeoutExpired:
        _child_failed.append(env)
        raise
    if r.returncode != 0:
        _child_failed.append(env)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    res = json.loads(lines[0])
    for row in res['cases']:
        print(f"{row['kernel']}{tuple(row['tpl'])}  {row['id']}  err / bound = {row['ratio']:.4f}")
    assert [row['id'] for row in res['cases']] == [c.id for c in expect]
    assert [(row['kernel'], tuple(row['tpl']), row['finish']) for row in res['cases']] == [G.expected_launch(c, env)[:2] + (G.expected_launch(c, env).finish,) for c in expect]
    failed = [row for row in res['cases'] if not row['ok']]
    assert not failed, failed
    assert [x['id'] for x in res['refusals']] == [c.id for c in refuse]
    assert all(x['refused'] and x['good_after'] for x in res['refusals']), [x for x in res['refusals'] if not (x['refused'] and x['good_after'])]
