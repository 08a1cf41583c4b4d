'''The four GroupNorm consumers of csrc/norm.hip through the C ABI on every dispatch branch and statistics form: the
case table of tests/groupnorm_cases.py against float64 references of the same fp16-rounded inputs under its derived
per-element bound, with buffers this test owns (sentinel guards around every output, the workspace at exactly
fd_groupnorm_workspace_floats), a second launch for the same bits, and what the ABI refuses.  Needs an MI355X.

Worst |err| / bound on an MI355X per form (test_groupnorm_case prints each case's with -s):
    slab256 0.990   slab1024 0.996   stream 0.997   apply_parts 0.998   fold 0.994   fold_parts 0.996
All of it is the one rounding to half (the fp32 CPU emulation reaches the same 0.99 .. 1.00).  The direct view of the
statistics, bias_out of the indicator cases at mean = 10 sigma, whose bound holds no fp16 term at all: 0.22 behind the
longest streaming lanes (fold 129x2295x24 g8), 0.59 at fold 2x100x320 g32, 0.87 from supplied parts.'''
import pytest
import torch

import groupnorm_cases as GN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _run(case, dev, inp):
    '''A HIP runtime failure (a failed launch, a fault met at the synchronize) ends the session: nothing more is
    started on a device that has faulted.'''
    try:
        return GN.run_on_device(case, dev, inp)
    except RuntimeError as e:
        pytest.exit(f'HIP runtime failure at {case.id}: {e}', returncode=3)


@pytest.mark.parametrize('case', GN.CASES, ids=[c.id for c in GN.CASES])
def test_groupnorm_case(dev, case):
    '''One call per case, then the same call into fresh buffers.  Every output element passes groupnorm_cases.check;
    every guard element before and after y / w_out / bias_out and every workspace float beyond B * nchunk * G * 2 keeps
    its bits; the inputs (padding columns and the wide matrix around a slice included) are unchanged; both launches
    give the same bits.'''
    form = GN.expected_form(case)['form']
    inp = GN.inputs(case)
    got = _run(case, dev, inp)
    want = GN.reference(case, inp, got)
    ratio = GN.worst(case, got, want)
    print(f'{form}  {case.id}  err / bound = {ratio:.4f}')
    assert GN.check(case, got, want), f'{form}: worst error is {ratio:.3g} x the bound'
    assert got['untouched'], f'{form} wrote outside its outputs or beyond its share of the workspace'
    assert got['inputs_kept'], f'{form} changed an input buffer'
    again = _run(case, dev, inp)
    for name in ('y', 'w_out', 'bias_out'):
        if name in got:
            bits = torch.int16 if got[name].dtype == torch.float16 else torch.int32
            assert torch.equal(got[name].view(bits), again[name].view(bits)), f'{form}: {name} differs between two launches'


@pytest.mark.parametrize('name,route,args', GN.REFUSALS, ids=[f'{r}-{n}' for n, r, _ in GN.REFUSALS])
def test_groupnorm_refusals(dev, name, route, args):
    '''Host-side argument checks: the expected error code, nothing launched, no output byte changed.'''
    rc, untouched = GN.call_refused(route, args, dev)
    assert rc == GN.refusal_code(route, args) != GN.FD_OK, f'{GN.ENTRY[route]} answers {rc} to {name}'
    assert untouched, f'{GN.ENTRY[route]} wrote to an output although it refused {name}'
