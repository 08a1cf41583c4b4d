'''fd_xattn_q_f16 and fd_xattn_pack_kv_f16 through the C ABI on every form: the case table of tests/xattn_cases.py (all 16 key
counts of the per-lane tail mask, 1 / 3 / 8 / 9 / 20 row tiles, samples of one and of three tiles, 1..3 context replicas, padded
leading dimensions and strided samples, a sliced output, finished statistics and 2 / 4 / 8 partial slabs with two values of eps)
against a float64 reference of the operands the device receives; the packed images bit for bit against a restatement of their
layout, short contexts included; and what the three entry points refuse.  Needs an MI355X.'''
import ctypes

import pytest
import torch

import xattn_cases as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.mark.parametrize('case', X.CASES, ids=[c.id for c in X.CASES])
def test_xattn_case(dev, case):
    '''One launch pair (pack, attend) per case.  The bound is attention_cases.check: |err| <= 4e-3 + 4e-3 |want| on every element.
    The image buffers start as 0xFF bytes and must equal the restated layout bit for bit (an unwritten byte is a NaN half); the O
    buffer starts as a sentinel, so an unwritten output fails the bound and a write outside the output rows and columns (padding
    columns C .. ldo - 1, the guard rows around a slice, whatever lies behind the last replica) fails the bit-for-bit comparison.
    A second identical launch must give the same bits, and a parts form the bits of the finished-statistics launch.'''
    inp = X.inputs(case)
    r = X.run_on_device(case, dev, inp)
    want = X.reference(case, inp)
    ratio = X.worst(r.out, want)
    stats = 'fin' if case.stats == 'fin' else f'parts{case.stats}'
    print(f'k_xattn<{case.d}>  {stats}  {case.id}  err / bound = {ratio:.4f}')
    kimg, vimg = X.image_reference(case, inp)
    assert torch.equal(r.kimg, kimg), f'k_xattn_pack<{case.d}>: K image differs in {int((r.kimg != kimg).sum())} halfs'
    assert torch.equal(r.vimg, vimg), f'k_xattn_pack<{case.d}>: V^T image differs in {int((r.vimg != vimg).sum())} halfs'
    assert X.check(r.out, want), f'k_xattn<{case.d}>: worst error is {ratio:.3g} x the bound'
    assert r.untouched, f'k_xattn<{case.d}> wrote outside its output ({case.layout})'
    assert torch.equal(r.out.view(torch.int16), r.again.view(torch.int16)), 'two identical launches differ'
    if case.stats != 'fin':
        assert torch.equal(r.out.view(torch.int16), r.fin.view(torch.int16)), 'partial sums and finished statistics give different bits'


@pytest.mark.parametrize('d', (40, 80))
@pytest.mark.parametrize('L', (1, 16, 64))
def test_xattn_pack_short_contexts(dev, L, d):
    '''The packer takes 1..80 keys (the kernel itself needs more than 64): three contexts with strided samples, against the
    restated layouts.'''
    case = X.Case(3, X.row_tile(d), 1, L, d, 'padded_ld', seed=900 + L + d)
    inp = X.inputs(case)
    kimg, vimg, keep = X.pack_on_device(case, dev, X.host_buffers(case, inp))
    torch.cuda.synchronize()
    want_k, want_v = X.image_reference(case, inp)
    assert torch.equal(kimg.cpu().view(torch.int16), want_k) and torch.equal(vimg.cpu().view(torch.int16), want_v)
    del keep


def _staged(dev, d):
    '''A three-tile case on the device: (case, inputs, device tensors, descriptor, reference).'''
    case = X.Case(3, X.row_tile(d), 1, 77, d, seed=950 + d)
    inp = X.inputs(case)
    host = X.host_buffers(case, inp)
    kimg, vimg, kv = X.pack_on_device(case, dev, host)
    t = {'x': host['x'].to(dev), 'w': host['w'].to(dev), 'bias': inp['bias'].to(dev), 'colsum': inp['colsum'].to(dev),
         'kimg': kimg, 'vimg': vimg, 'o': host['o'].to(dev), 'stats': inp['stats'].to(dev), 'k': kv[0], 'vt': kv[1], 'o_host': host['o']}
    return case, inp, t, X.build_desc(case, t, t['stats'], 0), X.reference(case, inp)


@pytest.mark.parametrize('d', (40, 80))
def test_xattn_refusals(dev, d):
    '''Each malformed call is answered with ValueError (FD_EINVAL / FD_ESHAPE) by a check that precedes the launch in
    csrc/xattn.hip, and launches nothing: the sentinel-filled output (the 0xFF-filled images) is unchanged after a sync.  The good
    call straight after each refusal passes `check` (equals the restated images).'''
    from flexdiffuse_amd import hip
    case, inp, t, good, want = _staged(dev, d)
    C, bm = case.C, X.row_tile(d)
    sentinel = t['o_host'].view(torch.int16)

    def attend(desc):
        t['o'].copy_(t['o_host'])
        try:
            hip.call('fd_xattn_q_f16', ctypes.byref(desc), hip.stream())
        finally:
            torch.cuda.synchronize()
        return t['o'].cpu()

    def edit(**kw):
        def apply(desc):
            for name, value in kw.items():
                setattr(desc, name, value(getattr(desc, name)) if callable(value) else value)
        return apply

    broken = [edit(**{f: None}) for f in ('x', 'wq', 'bias', 'ln_colsum', 'ln_stats', 'k_image', 'v_image', 'out')]
    broken += [edit(heads=5), edit(head_dim=64), edit(M=case.M - 8), edit(rows_per_sample=bm // 2), edit(rows_per_sample=2 * bm),
               edit(n_keys=64), edit(n_keys=81), edit(n_rep=0), edit(ldx=C + 4), edit(ldw=C + 4), edit(ldo=C + 2),
               edit(ldx=C - 8), edit(ldw=C - 8), edit(ldo=C - 4), edit(x=lambda p: p + 8), edit(out=lambda p: p + 4), edit(ln_stats_parts=3)]
    assert case.M % (2 * bm) != 0 and case.M % (bm // 2) == 0 and (case.M - 8) % bm != 0
    for apply in broken:
        desc = type(good).from_buffer_copy(good)
        apply(desc)
        with pytest.raises(ValueError):
            attend(desc)
        assert torch.equal(t['o'].cpu().view(torch.int16), sentinel), 'a refused call wrote to its output'
        out, untouched = X.read_output(case, attend(good))
        assert untouched and X.check(out, want)

    p = X.layout_plan(case)
    want_k, want_v = X.image_reference(case, inp)
    args = dict(K=t['k'].data_ptr(), Vt=t['vt'].data_ptr(), kimg=t['kimg'].data_ptr(), vimg=t['vimg'].data_ptr(), samples=case.n_ctx,
                n_keys=case.L, heads=X.HEADS, head_dim=d, ldk=p['ldk'], ldvt=p['ldvt'], sK=p['sK'], sVt=p['sVt'])

    def pack(**kw):
        t['kimg'].fill_(0xFF)
        t['vimg'].fill_(0xFF)
        try:
            hip.call('fd_xattn_pack_kv_f16', *dict(args, **kw).values(), hip.stream())
        finally:
            torch.cuda.synchronize()

    for kw in [dict(K=None), dict(Vt=None), dict(kimg=None), dict(vimg=None), dict(samples=0), dict(n_keys=0), dict(n_keys=81),
               dict(head_dim=64), dict(heads=5), dict(ldvt=case.L - 1), dict(ldk=C - 8)]:
        with pytest.raises(ValueError):
            pack(**kw)
        assert bool((t['kimg'] == 0xFF).all()) and bool((t['vimg'] == 0xFF).all()), 'a refused call wrote to an image'
        pack()
        assert torch.equal(t['kimg'].cpu().view(torch.int16), want_k) and torch.equal(t['vimg'].cpu().view(torch.int16), want_v)

    lib = hip.lib()
    assert lib.fd_xattn_image_bytes(5, 64) == 0 and lib.fd_xattn_image_bytes(8, 64) == 0
    assert lib.fd_xattn_image_bytes(8, 40) == 61440 == X.IMAGE_BYTES[40] and lib.fd_xattn_image_bytes(8, 80) == 102400 == X.IMAGE_BYTES[80]
