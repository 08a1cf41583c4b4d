'''The implicit-GEMM convolution on every geometry and loader: the table of tests/conv_cases.py -- stride 2 with and without padding, odd
and non-square inputs, the fused nearest upsample, the phase-decomposed upsample, two input slices, split-K, on the one-shot, persistent,
register-staged and ping-pong loaders in both tap orders -- through the C ABI against a float64 reference (torch.nn.functional.conv2d on
the same rounded operands), with gemm_cases' per-element bound and the bit-for-bit check of everything around the output; what the ABI
refuses; the FD_GEMM_PERSIST / FD_GEMM_NO_DMA / FD_CONV_TAPFAST arms (and the persistent kernel under FD_CONV_TAPFAST=2), each in a fresh
process; and a handful of geometries through ops.conv2d / ops.conv2d_up_phases, whose own out_h / out_w derivation the C ABI cases do not
see.  Needs an MI355X; the whole file takes about a quarter of a minute there (15.9 s measured: 169 tests, 432 scored launches, 286 of
them in the five children at 2.3 - 3.1 s per child; tests/test_gpu_gemm_cases.py: 109 s for 1391), the largest case 0.2 s (the first
one, which loads the library).'''
import json
import os
import subprocess
import sys

import pytest
import torch

import conv_cases as C
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


GOOD = C.BY_ID['s2-t10']


@pytest.mark.parametrize('case', C.CASES, ids=[c.id for c in C.CASES])
def test_conv_case(dev, case):
    '''One launch per case.  Bound (gemm_cases.check): |err| <= 3e-3 + 3e-3 |want| on every element of the fp16 output.  Every output buffer
    is filled with a sentinel first, guard rows and padding columns included: a pixel that the interleaved phase store leaves unwritten
    fails the bound, a write outside the output fails the bit-for-bit comparison.  A refused case must answer ValueError, and a good call
    must follow it.  The kernel name printed is PREDICTED by gemm_cases.expected_launch, not observed on the device.'''
    if G.refused(case):
        with pytest.raises(ValueError):
            _guarded(lambda: G.run_on_device(case, dev))
        row = _guarded(lambda: G.run_and_score(GOOD, dev, ref=C.reference))
        assert row['ok'], row
        return
    row = _guarded(lambda: G.run_and_score(case, dev, ref=C.reference))
    L = G.expected_launch(case)
    print(f"{L.kernel}{L.tpl}{' + ' + L.finish if L.finish else ''}{' tap-fastest' if L.tap_fast else ''}  {case.id}  err / bound = {row['ratio']:.4f}")
    assert row['ratio'] <= 1.0, f"{L.kernel}{L.tpl}: worst error is {row['ratio']:.3g} x the bound"
    assert row['untouched'], f'{L.kernel}{L.tpl} wrote outside its output, or into an input ({case.layout})'


_child_failed = []


@pytest.mark.parametrize('env', C.ENV_SETTINGS, ids=['-'.join(f'{k}={v}' for k, v in e.items()) for e in C.ENV_SETTINGS])
def test_conv_ab_switches(env):
    '''The library reads each switch once per process, so each setting gets one fresh interpreter that runs every table case whose expected
    launch the setting changes, and of the cases that the setting makes the library refuse those of one lean tile (13) and every
    phase case (a refusal comes before any look at the data), each refusal followed by a good call, and prints one JSON line.  One child
    at a time, each under its own timeout; after a child that did not exit cleanly no further child is started.'''
    if _child_failed or _device_error:
        pytest.fail(f'not started: {(_child_failed or _device_error)[0]} did not end cleanly')
    expect, skipped = C.child_cases(env)
    assert expect, f'{env} changes no case of the table'
    refuse = [c for c in skipped if c.tile == 13 or c.phase]
    assert bool(refuse) == bool(skipped)
    good = min(expect, key=lambda c: c.M * c.N * c.K)
    child_env = dict(os.environ, **env)
    child_env['PYTHONPATH'] = os.pathsep.join([ROOT] + [p for p in child_env.get('PYTHONPATH', '').split(os.pathsep) if p])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'conv_cases.py'), '--child',
                            json.dumps({'env': env, 'run': [c.id for c in expect], 'refuse': [c.id for c in refuse], 'good': good.id})],
                           env=child_env, capture_output=True, timeout=300)
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


# ------------------------------------------------------------------------------------------------ through the Python wrappers
def _operands(B, H, W, cin, cout, kh, kw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, cin), generator=g).half()
    w = (torch.randn((cout, cin, kh, kw), generator=g) * (kh * kw * cin) ** -0.5)
    b = torch.arange(cout, dtype=torch.float32) * 0.25 - 3.0
    return x, w, b


def _score(case, got, inp):
    '''err / bound of the wrapper's output (the rows of a wider sentinel buffer `got` [rows][ld]) against conv_cases.reference, and whether
    the columns behind the output kept the sentinel.'''
    want = C.reference(case, inp)
    back = got.cpu()
    n = case.N
    ratio = G.worst(case, {'C': back[:, :n].reshape(want['C'].shape)}, want)
    kept = torch.equal(back[:, n:].contiguous().view(torch.int16), torch.full_like(back[:, n:], G.SENTINEL).contiguous().view(torch.int16))
    return ratio, kept


# (stride, pad, up, out_hw, (B, H, W), expected (Ho, Wo)): the geometries of the table whose output size the wrapper derives itself
WRAPPED = {'s2-odd': (2, (1, 1), False, None, (3, 15, 17), (8, 9)),
           's2-vae-odd': (2, (0, 0), False, 'half', (3, 15, 33), (7, 16)),
           's2-vae': (2, (0, 0), False, 'half', (2, 16, 32), (8, 16)),
           'up-odd': (1, (1, 1), True, None, (3, 5, 6), (10, 12)),
           'k1x3-s2': (2, (0, 1), False, None, (2, 16, 32), (8, 16))}


@pytest.mark.parametrize('name', sorted(WRAPPED))
def test_conv2d_wrapper_derives_the_geometry(dev, name):
    '''ops.conv2d on the rule's own tile: odd sizes, out_hw = in // 2 with pad (0, 0), up=True, a 1x3 filter -- out_h / out_w as the
    wrapper derives them, into a strided destination, against the table's reference and bound.'''
    from flexdiffuse_amd import ops
    stride, pad, up, out_hw, (B, H, W), (ho, wo) = WRAPPED[name]
    kh, kw = C.GEOMETRIES[name][:2]
    cin, cout = 64, 160
    x, w, b = _operands(B, H, W, cin, cout, kh, kw, 11 + len(name))
    cw = ops.prep_conv(w, b, dev)
    buf = torch.full((B * ho * wo, cout + 8), G.SENTINEL, dtype=torch.float16, device=dev)
    act = ops.Act(x.reshape(B * H * W, cin).to(dev), B, H, W)
    y = _guarded(lambda: ops.conv2d(act, cw, stride=stride, pad=pad, up=up, out_hw=(H // 2, W // 2) if out_hw == 'half' else None, out=buf[:, :cout]))
    torch.cuda.synchronize()
    assert (y.B, y.H, y.W) == (B, ho, wo)
    case = G.Case(name, 0, B * ho * wo, cout, kh * kw * cin, conv=C._conv(name, cin), rps=ho * wo)
    inp = {'A': x[None], 'W': cw.w.cpu()[None, :, :kh * kw * cin], 'bias': b[None]}
    ratio, kept = _score(case, buf, inp)
    print(f'{name}: err / bound = {ratio:.4f}')
    assert ratio <= 1.0 and kept, (ratio, kept)


def test_conv2d_up_phases_wrapper_into_a_strided_destination(dev):
    '''ops.conv2d_up_phases at the smallest non-square shape ops.up_phases_supported accepts whose samples do not align with the rule's
    256-row tile (8 x 24x40 low-resolution pixels: 960 rows per sample), into a column slice of a wider buffer, against the parity formula
    on the stored fp16 filters.'''
    from flexdiffuse_amd import ops
    B, H, W, cin, cout = 8, 24, 40, 64, 160
    assert ops.up_phases_supported(B * H * W, cout, cin) and (H * W) % 256 != 0
    x, w, b = _operands(B, H, W, cin, cout, 3, 3, 5)
    cw = ops.prep_conv_up_phases(w, b, dev)
    buf = torch.full((B * 4 * H * W, cout + 64), G.SENTINEL, dtype=torch.float16, device=dev)
    act = ops.Act(x.reshape(B * H * W, cin).to(dev), B, H, W)
    y = _guarded(lambda: ops.conv2d_up_phases(act, cw, out=buf[:, :cout]))
    torch.cuda.synchronize()
    assert (y.B, y.H, y.W) == (B, 2 * H, 2 * W)
    case = G.Case('ph-wrapped', 0, B * H * W, cout, 4 * cin, conv=(H, W, cin, 2, 2, 1, 1, 1, 2, H, W), batch=4, rps=H * W)
    ratio, kept = _score(case, buf, {'A': x[None], 'W': cw.w.cpu(), 'bias': b[None]})
    print(f'conv2d_up_phases: err / bound = {ratio:.4f}')
    assert ratio <= 1.0 and kept, (ratio, kept)
