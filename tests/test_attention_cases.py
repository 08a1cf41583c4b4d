'''CPU checks of tests/attention_cases.py: its restatement of the fd_attention_f16 dispatcher names exactly the launch
targets in csrc/attention.hip, its table reaches all of them and everything the table promises to cover, and its
acceptance criterion accepts fp16-rounded fp32 attention while rejecting seven kinds of wrong attention.'''
import os
import re

import pytest
import torch

import attention_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCREEN_CAP = 1 << 22     # B * heads * n_q * n_k of a screened case (2048 x 2048 of one head: the smallest k_attention_w8<64, 4, *, false, 2> causal case)
LIVE = [c for c in A.CASES if not A.refused(c)]
SCREENED = [c for c in LIVE if c.B * c.heads * c.n_q * c.n_k <= SCREEN_CAP]


def _dispatcher_text():
    with open(os.path.join(ROOT, 'flexdiffuse_amd', 'csrc', 'attention.hip'), encoding='utf-8') as f:
        src = f.read()
    return src, src[src.index('// Host side: check the descriptor, choose the kernel, launch it.'):]


def _launch_targets():
    '''Every kernel fd_attention_f16 can launch.  Its one hipLaunchKernelGGL launches what attn_choose returns, and
    attn_choose returns an entry of the ATTN_BANDS or ATTN_LAZY table or the one kernel it names itself: so the targets
    are the kernel names between the first table and the end of attn_choose, each spelled in full there.'''
    _, body = _dispatcher_text()
    assert body.count('hipLaunchKernelGGL(') == 1 and 'hipLaunchKernelGGL(c.kernel, ' in body
    assert body.count('attn_choose(') == 2 and 'const AttnChoice c = attn_choose(' in body      # the definition and its one use
    tables = body[body.index('static const AttnBand ATTN_BANDS[]'):body.index('static int attn_check(')]
    assert 'static const AttnLazyRow ATTN_LAZY[]' in tables and 'static AttnChoice attn_choose(' in tables
    code = '\n'.join(ln.split('//')[0] for ln in tables.split('\n'))
    return set(re.findall(r'\bk_attention\w*(?:<[^<>]*>)?', code))


def _reachable():
    '''kernel name -> [(case, env)] over the default and every listed A/B setting.'''
    out = {}
    for env in ({},) + A.ENV_SETTINGS:
        for c in A.CASES:
            if not A.refused(c, env):
                out.setdefault(A.expected_kernel(c, env), []).append((c, env))
    return out


def test_restated_dispatcher_names_the_launch_targets_of_the_source():
    src, _ = _dispatcher_text()
    targets = _launch_targets()
    assert len(targets) == 27, sorted(targets)
    reach = _reachable()
    assert set(reach) <= targets, f'names not launched by fd_attention_f16: {sorted(set(reach) - targets)}'
    assert targets <= set(reach), f'launch targets without a case: {sorted(targets - set(reach))}'
    for name in reach:     # the spelling exists in the source
        assert name in src, name
    for env in A.ENV_SETTINGS:
        (var, _), = env.items()
        assert f'getenv("{var}")' in src


def test_default_build_reaches_every_default_kernel_prescaled_and_not():
    default = {}
    for c in LIVE:
        default.setdefault(A.expected_kernel(c), []).append(c)
    old = {n for n in _launch_targets() if n.startswith('k_attention<') and n not in ('k_attention<96, 6>', 'k_attention<128, 8>')}
    assert set(default) == _launch_targets() - old
    for name in default:     # `true` and `false` PRE twins both present by the set equality above
        assert A.family_of(name) in (('k_attention', None), ('k_attention_w8', 1), ('k_attention_w8', 2), ('k_attention_w8q2m', None))
    refusals = [c for c in A.CASES if A.refused(c)]
    assert sorted((c.d, c.pre) for c in refusals) == [(88, True), (128, True)]


def test_table_covers_what_it_promises():
    assert {c.d for c in LIVE} >= {8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104, 128, 160}
    assert {c.n_q for c in LIVE} >= {1, 17, 127, 129, 2047, 2048} and {c.n_k for c in LIVE} >= {1, 8, 63, 64, 65, 1023, 1024}
    key = {(c.n_q, c.n_k, c.heads, c.d, c.causal) for c in LIVE}
    assert key >= {(256, 256, 8, 160, False), (576, 576, 8, 160, False), (144, 144, 8, 160, False), (1024, 1024, 8, 80, False),
                   (2304, 2304, 8, 80, False), (77, 77, 12, 64, True), (257, 257, 16, 64, False), (257, 257, 16, 80, False)}
    # both sides of each dispatch threshold, on a head dim where the threshold decides the kernel
    k = A.expected_kernel
    pick = lambda **kw: [c for c in LIVE if all(getattr(c, n) == v for n, v in kw.items())]
    assert {A.family_of(k(c)) for c in pick(n_q=2047, d=40)} == {('k_attention_w8', 1)} and pick(n_q=2047, d=40)
    assert {A.family_of(k(c)) for c in pick(n_q=2048, n_k=1024, d=40)} == {('k_attention_w8', 2), ('k_attention_w8q2m', None)}
    assert [k(c) for c in pick(n_q=2048, n_k=63)] == ['k_attention_w8<64, 3, true, true, 1>']
    assert 'k_attention_w8q2m' in [k(c) for c in pick(n_q=2048, n_k=64)]
    assert [k(c) for c in pick(n_q=2048, n_k=1023, d=64)] == ['k_attention_w8<64, 4, true, false, 1>']
    assert [k(c) for c in pick(n_q=2048, n_k=1024, d=64)] == ['k_attention_w8<64, 4, false, false, 2>']
    assert any(c.causal and c.n_q < c.n_k for c in LIVE) and any(c.causal and c.n_q > c.n_k for c in LIVE)
    by_template = {}      # per (template, query blocks per wave)
    for c in LIVE:
        by_template.setdefault(A.family_of(k(c)), []).append(c)
    assert set(by_template) == {('k_attention', None), ('k_attention_w8', 1), ('k_attention_w8', 2), ('k_attention_w8q2m', None)}
    for t, cases in by_template.items():
        assert {c.layout for c in cases} == set(A.LAYOUTS), t
        assert any(c.scale > 0 for c in cases), t
        # the sample strides (and the gaps padded_ld puts between samples) are read only with a second sample
        assert any(c.layout == 'padded_ld' and c.B >= 2 for c in cases), t
        assert any(c.layout in ('merged_qk', 'out_slice') and c.B >= 2 for c in cases), t
        assert any(A.grid_size(c) % 8 for c in cases), t       # XCD remapping with a remainder
    assert any(A.grid_size(c) < 8 for c in LIVE)
    for env in A.ENV_SETTINGS:
        assert any(not A.refused(c, env) and k(c, env) != k(c) for c in LIVE), env


def test_layouts_are_what_their_tags_say():
    for c in LIVE:
        p, C = A.layout_plan(c), c.heads * c.d
        assert p['ldq'] % 8 == 0 and p['ldk'] % 8 == 0 and p['ldvt'] % 8 == 0 and p['ldo'] % 4 == 0
        assert p['sQ'] % 8 == 0 and p['sK'] % 8 == 0 and p['sVt'] % 8 == 0 and p['sO'] % 4 == 0 and p['k_off'] % 8 == 0
        assert p['ldvt'] > A._round8(c.n_k)          # at least one junk column behind the zero padding
        if c.layout == 'merged_qk':
            assert p['ldq'] == p['ldk'] == 2 * C and p['k_off'] == C
        if c.layout == 'padded_ld':
            assert len({p['ldq'], p['ldk'], p['ldo']}) == 3 and min(p['ldq'], p['ldk'], p['ldo']) > C
            assert p['sQ'] > c.n_q * p['ldq'] and p['sK'] > c.n_k * p['ldk'] and p['sO'] > c.n_q * p['ldo'] and p['sVt'] > C * p['ldvt']
        # the last element each operand's view reaches lies inside its buffer
        assert (c.B - 1) * p['sQ'] + (c.n_q - 1) * p['ldq'] + C <= p['q_size']
        assert p['k_off'] + (c.B - 1) * p['sK'] + (c.n_k - 1) * p['ldk'] + C <= (p['q_size'] if p['merged'] else p['k_size'])
        assert (c.B - 1) * p['sVt'] + (C - 1) * p['ldvt'] + p['ldvt'] <= p['vt_size']
        assert p['o_off'] + (c.B - 1) * p['sO'] + (c.n_q - 1) * p['ldo'] + C <= p['o_size']
    c = next(c for c in LIVE if c.layout == 'padded_ld' and c.B == 2)
    inp = A.inputs(c)
    host = A.host_buffers(c, inp)
    p, C = A.layout_plan(c), c.heads * c.d
    assert torch.equal(torch.as_strided(host['k'], (c.B, c.n_k, C), (p['sK'], p['ldk'], 1), 0), inp['k16'])
    vt = torch.as_strided(host['vt'], (c.B, C, p['ldvt']), (p['sVt'], p['ldvt'], 1), 0)
    assert torch.equal(vt[:, :, :c.n_k], inp['v16'].transpose(1, 2)) and float(vt[:, :, c.n_k:A._round8(c.n_k)].abs().sum()) == 0
    assert bool((vt[:, :, A._round8(c.n_k):] == A.JUNK).all())


def test_every_kernel_name_keeps_a_screened_case():
    names = {A.expected_kernel(c) for c in LIVE}
    screened = {A.expected_kernel(c) for c in SCREENED}
    assert names == screened, f'no case under the cap for {sorted(names - screened)}: add a small one'
    old = _reachable()
    for name, hits in old.items():       # the A/B arms as well
        assert any(c in SCREENED for c, _ in hits), name


@pytest.fixture(scope='module')
def screen():
    '''case id -> (worst ratio of fp16-rounded fp32 attention, {mutant: worst ratio, for the mutants that apply}).'''
    out = {}
    for case in SCREENED:
        inp = A.inputs(case)
        want = A.reference(case, inp)
        assert want.shape == (case.B, case.n_q, case.heads * case.d) and bool(torch.isfinite(want).all())
        # a prescaled case hands the kernel q * scale * log2(e) rounded to fp16: the reference must see that rounding
        if case.pre:
            assert torch.equal((inp['q'] * (case.eff_scale * A.QK_LOG2E)).half(), inp['q16'])
        good = A.attend(case, inp, torch.float32).half()
        assert A.check(good, want) == (A.worst(good, want) <= 1.0)
        bad = {m: A.attend(case, inp, torch.float64, m) for m in A.MUTANTS}
        out[case.id] = (A.worst(good, want), {m: A.worst(b, want) for m, b in bad.items() if b is not None})
    return out


@pytest.mark.parametrize('case', SCREENED, ids=[c.id for c in SCREENED])
def test_check_accepts_fp16_rounded_fp32_and_rejects_every_mutant(screen, case):
    good, mutants = screen[case.id]
    assert good <= 1.0, f'fp16-rounded fp32 attention is refused: {good:.3g} x the bound'
    for mutant, ratio in mutants.items():
        assert ratio > 1.0, f'{mutant} passes the bound ({ratio:.3g} x) at {case.id}'


def test_every_kernel_name_saw_the_mutants(screen):
    '''Each default kernel name had the size-independent mutants applied, and every mutant was applied somewhere on
    each template and number of query blocks per wave.'''
    applied = {}
    for case in SCREENED:
        applied.setdefault(A.expected_kernel(case), set()).update(screen[case.id][1])
    by_template = {}
    for name, seen in applied.items():
        assert seen >= {'drop_last_key', 'scale_3pct'}, (name, seen)
        by_template.setdefault(A.family_of(name), set()).update(seen)
    for t, seen in by_template.items():
        assert seen == set(A.MUTANTS), (t, set(A.MUTANTS) - seen)


def _attention_stand_in(name, dref, stream):
    '''fd_attention_f16 as plain fp32 torch on the HOST memory the descriptor points at -- the honest-kernel stand-in that
    lets the GPU test's own driver (layouts, strides, descriptor, read-back, sentinel check) run without a device.'''
    import ctypes
    assert name == 'fd_attention_f16'
    d = dref._obj
    B, H, nq, nk, hd = d.batch, d.heads, d.n_q, d.n_k, d.head_dim
    C = H * hd

    def view(ptr, sample, ld, rows, cols):
        n = (B - 1) * sample + (rows - 1) * ld + cols
        flat = torch.frombuffer((ctypes.c_uint16 * n).from_address(ptr), dtype=torch.float16)
        return torch.as_strided(flat, (B, rows, cols), (sample, ld, 1))

    q, k = view(d.Q, d.q_sample_stride, d.ldq, nq, C), view(d.K, d.k_sample_stride, d.ldk, nk, C)
    vt, o = view(d.Vt, d.vt_sample_stride, d.ldvt, C, nk), view(d.O, d.o_sample_stride, d.ldo, nq, C)
    scale = 1 / A.QK_LOG2E if d.q_prescaled else d.scale if d.scale > 0 else hd ** -0.5
    for b in range(B):
        for h in range(H):
            sl = slice(h * hd, h * hd + hd)
            s = q[b][:, sl].float() @ k[b][:, sl].float().T * scale
            if d.causal:
                s = s.masked_fill(torch.arange(nk)[None] > torch.arange(nq)[:, None], float('-inf'))
            o[b][:, sl] = (s.softmax(-1) @ vt[b][sl].float().T).half()


def test_device_driver_against_a_host_stand_in(monkeypatch):
    '''run_on_device with the library call replaced by the stand-in above: every layout hands the kernel the operands
    the reference sees, reads O back from where it was written and notices a write outside it.'''
    import ctypes
    from flexdiffuse_amd import hip
    monkeypatch.setattr(hip, 'call', _attention_stand_in)
    monkeypatch.setattr(hip, 'stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    small = [c for c in A.CASES if c.B * c.heads * c.n_q * c.n_k <= 1 << 20]
    small = [c for c in small if not A.refused(c)]
    assert {c.layout for c in small} == set(A.LAYOUTS) and any(c.B >= 2 and c.layout == 'padded_ld' for c in small)
    for case in small:
        inp = A.inputs(case)
        got, untouched = A.run_on_device(case, 'cpu', inp)
        assert untouched and A.check(got, A.reference(case, inp)), case.id

    def spill(name, dref, stream):      # one element beyond the last output row
        _attention_stand_in(name, dref, stream)
        d = dref._obj
        end = d.O + 2 * ((d.batch - 1) * d.o_sample_stride + (d.n_q - 1) * d.ldo + d.heads * d.head_dim)
        ctypes.c_uint16.from_address(end).value = 0

    monkeypatch.setattr(hip, 'call', spill)
    case = next(c for c in small if c.layout == 'out_slice')
    assert A.run_on_device(case, 'cpu')[1] is False
