'''fd_attention_f16 through the C ABI on every dispatch branch: the case table of tests/attention_cases.py (head dims
8..160, both sides of each dispatch threshold, the UNet's merged q|k buffer and sliced output, padded leading
dimensions, a custom scale, causal with n_q != n_k) against a float64 reference of the same fp16-rounded inputs; what
the ABI refuses; and the FD_ATTN_* A/B arms, each in a fresh process.  Needs an MI355X.'''
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import attention_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', A.CASES, ids=[c.id for c in A.CASES])
def test_attention_case(dev, case):
    '''One launch per case.  The bound is attention_cases.check: |err| <= 4e-3 + 4e-3 |want| on every element; the O
    buffer is filled with a sentinel first, so an unwritten output fails the bound and a write outside the output rows
    and columns (out_slice: the rows around the slice; padded_ld: the padding columns and sample gaps) fails the
    bit-for-bit comparison.'''
    inp = A.inputs(case)
    if A.refused(case):
        with pytest.raises(ValueError):
            A.run_on_device(case, dev, inp)
        return
    got, untouched = A.run_on_device(case, dev, inp)
    want = A.reference(case, inp)
    ratio = A.worst(got, want)
    print(f'{A.expected_kernel(case)}  {case.id}  err / bound = {ratio:.4f}')
    assert A.check(got, want), f'{A.expected_kernel(case)}: worst error is {ratio:.3g} x the bound'
    assert untouched, f'{A.expected_kernel(case)} wrote outside its output ({case.layout})'


def _desc(dev, n_q=64, n_k=64, heads=2, d=40, pre=False):
    from flexdiffuse_amd import ops
    C = heads * d
    t = {'q': torch.zeros((n_q, C), dtype=torch.float16, device=dev), 'k': torch.zeros((n_k, C), dtype=torch.float16, device=dev),
         'vt': torch.zeros((C, (n_k + 7) // 8 * 8), dtype=torch.float16, device=dev),
         'o': torch.zeros((n_q, C), dtype=torch.float16, device=dev)}
    desc = ops.fd_attention_desc()
    desc.Q, desc.K, desc.Vt, desc.O = (t[n].data_ptr() for n in ('q', 'k', 'vt', 'o'))
    desc.ldq, desc.ldk, desc.ldvt, desc.ldo = C, C, t['vt'].shape[1], C
    desc.q_sample_stride, desc.k_sample_stride, desc.vt_sample_stride, desc.o_sample_stride = n_q * C, n_k * C, t['vt'].numel(), n_q * C
    desc.batch, desc.heads, desc.n_q, desc.n_k, desc.head_dim = 1, heads, n_q, n_k, d
    desc.causal, desc.scale, desc.q_prescaled = 0, 0.0, int(pre)
    return desc, t


def test_attention_refusals(dev):
    '''Each malformed descriptor is answered with ValueError (FD_ESHAPE / FD_EINVAL) and launches nothing; the call after
    each refusal still succeeds (zero q and k: uniform softmax of a zero V^T = zeros over the 1.0 prefill).'''
    from flexdiffuse_amd import hip

    def call(desc):
        hip.call('fd_attention_f16', ctypes.byref(desc), hip.stream())
        torch.cuda.synchronize()

    def bad_ldq(desc):
        desc.ldq += 4

    def bad_ldvt(desc):
        desc.ldvt -= 8

    broken = [(dict(d=4, heads=1), None), (dict(d=12, heads=1), None), (dict(d=168, heads=1), None), (dict(), bad_ldq),
              (dict(n_k=61), bad_ldvt), (dict(d=88, pre=True), None), (dict(d=128, pre=True), None)]
    broken += [(dict(), lambda desc, f=f: setattr(desc, f, None)) for f in ('Q', 'K', 'Vt', 'O')]
    for kw, edit in broken:
        desc, keep = _desc(dev, **kw)
        if edit is not None:
            edit(desc)
        with pytest.raises(ValueError):
            call(desc)
        good, t = _desc(dev)
        t['o'].fill_(1.0)
        call(good)
        assert float(t['o'].float().abs().max()) == 0.0
        del keep


_child_failed = []


@pytest.mark.parametrize('env', A.ENV_SETTINGS, ids=['-'.join(f'{k}={v}' for k, v in e.items()) for e in A.ENV_SETTINGS])
def test_attention_ab_switches(env):
    '''The library reads each FD_ATTN_* variable once per process, so each setting gets one fresh interpreter that runs
    every table case whose kernel the setting changes and prints one JSON line.  One child at a time; after a child
    that did not exit cleanly no further child is started.'''
    if _child_failed:
        pytest.fail(f'not started: the child for {_child_failed[0]} did not exit cleanly')
    expect = [c for c in A.CASES if not A.refused(c) and not A.refused(c, env) and A.expected_kernel(c, env) != A.expected_kernel(c)]
    assert expect, f'{env} changes no case of the table'
    child_env = dict(os.environ, **env)
    child_env['PYTHONPATH'] = os.pathsep.join([ROOT] + [p for p in child_env.get('PYTHONPATH', '').split(os.pathsep) if p])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'attention_cases.py'), '--child', json.dumps(env)],
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
        print(f"{row['kernel']}  {row['id']}  err / bound = {row['ratio']:.4f}")
    assert [row['id'] for row in res['cases']] == [c.id for c in expect]
    assert [row['kernel'] for row in res['cases']] == [A.expected_kernel(c, env) for c in expect]
    failed = [row for row in res['cases'] if not row['ok']]
    assert not failed, failed
    # prescaled q exists only on the default kernels: those cases are the only ones a setting may leave out
    assert all(c.pre for c in A.CASES if c.id in res['skipped'])
