'''CPU checks of tests/layout_cases.py: the tables cover what they promise (cases on both sides of every grid cap, the caps restated
from the text of csrc/elementwise.hip, the rounding-boundary set complete, no buffer above 128 MB), the acceptance criterion accepts
an fp32 emulation of every kernel (both legal forms of the affine) while rejecting a list of wrong computations on every case they
apply to, the k of the exp form is computed on the host, and the GPU test's own driver runs against a host stand-in of the library.'''
import ctypes
import os
import re

import pytest
import torch

import layout_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [c.id for c in L.CASES]


def _source():
    with open(os.path.join(ROOT, 'flexdiffuse_amd', 'csrc', 'elementwise.hip'), encoding='utf-8') as f:
        return f.read()


def _body(src, entry):
    '''The text of one extern "C" entry point.'''
    start = src.index(f'extern "C" int {entry}(')
    return src[start:src.index('\n}\n', start)]


# --------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize('entry', L.ENTRY_POINTS)
def test_every_entry_point_has_cases_on_both_sides_of_its_cap(entry):
    cases = L.cases_of(entry)
    assert cases, f'no case for {entry}'
    body = _body(_source(), entry)
    assert f'FD_PLAN({entry}(' in body
    found = re.findall(r'fd_grid1d\([^,]+,\s*(\d+)\)', body)
    kernel = L.KERNEL[entry]
    assert f'hipLaunchKernelGGL({kernel}' in body.replace('(k_conv3x3_narrow<8>)', 'k_conv3x3_narrow')
    if not found:
        assert kernel not in L.CAP and L.cap_items(entry) is None
        return
    assert [int(v) for v in found] == [L.CAP[kernel]], f'{entry}: the source says {found}, the table {L.CAP[kernel]}'
    limit = L.cap_items(entry)
    below = [c for c in cases if L.work_items(c) <= limit]
    above = [c for c in cases if L.work_items(c) > limit]
    assert below and above, f'{entry}: {len(below)} cases at or below {limit} work items, {len(above)} above'
    assert min(L.work_items(c) for c in above) % L.BLOCK != 0, 'the far side has no ragged remainder'
    assert min(L.work_items(c) for c in above) < limit + 2 * L.BLOCK * 2, 'the far side is not the smallest size that crosses the cap'


def test_no_case_allocates_more_than_128_mb():
    worst = max(L.CASES, key=L.alloc_bytes)
    print(f'largest buffer: {L.alloc_bytes(worst) / 2 ** 20:.1f} MB ({worst.id})')
    assert L.alloc_bytes(worst) <= L.LIMIT_BYTES


def test_boundary_set_holds_a_tie_and_both_neighbours_for_every_adjacent_pair_of_halves():
    s = L.boundary_set()
    assert s.dtype == torch.float32
    have = set(L._bits(s[~torch.isnan(s)]).tolist())
    halves = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).float()
    inf = torch.tensor(float('inf'))
    for sign in (1.0, -1.0):
        lo, hi = sign * halves[:-1], sign * halves[1:]
        tie = ((lo.double() + hi.double()) / 2).float()
        assert torch.equal(tie.double(), (lo.double() + hi.double()) / 2)            # the midpoint is an fp32 number
        for name, v in (('half', lo), ('half', hi), ('tie', tie), ('below', torch.nextafter(tie, -inf)), ('above', torch.nextafter(tie, inf))):
            missing = [b for b in L._bits(v).tolist() if b not in have]
            assert not missing, (sign, name, len(missing))
    for v in (65504.0, 65519.996, 65520.0, float('inf'), float('-inf'), 2.0 ** -26, -2.0 ** -26, 1e-30):
        assert int(L._bits(torch.tensor(v, dtype=torch.float32))) in have, v
    assert bool(torch.isnan(s).any()) and bool(((s == 0) & torch.signbit(s)).any()) and bool(((s == 0) & ~torch.signbit(s)).any())
    # torch's CPU conversion is round-to-nearest-even on all of them: ties go to the even half, the neighbours to their own side
    for sign in (1.0, -1.0):
        lo, hi = sign * halves[:-1], sign * halves[1:]
        tie = ((lo.double() + hi.double()) / 2).float()
        lo_bits, got = L._bits(lo.half()).int(), L._bits(tie.half()).int()
        even = torch.where(lo_bits % 2 == 0, lo_bits, L._bits(hi.half()).int())
        assert torch.equal(got, even)
        toward_lo = torch.nextafter(tie, -inf * sign)
        toward_hi = torch.nextafter(tie, inf * sign)
        assert torch.equal(toward_lo.half().float(), lo) and torch.equal(toward_hi.half().float(), hi)
    assert float(torch.tensor(65519.996).half()) == 65504.0 and float(torch.tensor(65520.0).half()) == float('inf')
    print(f'boundary set: {s.numel()} values')


def test_tables_hold_the_cases_the_contracts_name():
    def P(entry):
        return [c.p for c in L.cases_of(entry)]
    assert {(p.B, p.C, p.HW, p.rep, p.c_pad) for p in P('fd_nchw_f32_to_nhwc_f16')} >= {(3, 4, 64, 1, 4), (2, 3, 35, 3, 8), (1, 1, 1, 1, 1), (2, 4, 4097, 2, 8)}
    assert [p for p in P('fd_nchw_f32_to_nhwc_f16') if p.data == 'boundary' and p.scale == 1.0 and p.B * p.C * p.HW >= L.boundary_set().numel()]
    assert [p for p in P('fd_nchw_f32_to_nhwc_f16') if p.B * p.HW * p.c_pad > 4096 * 256 and p.HW % 2 and p.C < p.c_pad and p.rep == 2]
    assert {p.scale for p in P('fd_nchw_f32_to_nhwc_f16') if p.data == 'rand'} == {L.VAE_SCALE, 0.5}
    for shape in ((2, 4, 64, 4), (3, 3, 35, 8), (1, 1, 1, 1)):
        for ab in ((1.0, 0.0), (0.5, 0.5), (1 / L.VAE_SCALE, 0.0), (-2.0, 3.0)):
            for clamp in (0, 1):
                assert [p for p in P('fd_nhwc_f32_to_nchw_f32') if (p.B, p.C, p.HW, p.ld, p.a, p.b, p.clamp) == shape + ab + (clamp,)]
    im = P('fd_im2col_f16')
    assert [p for p in im if (p.KH, p.KW, p.stride, p.pad_t, p.pad_l, p.Cin, p.k_pad) == (3, 3, 1, 1, 1, 4, 40)]
    assert [p for p in im if (p.KH, p.KW, p.stride, p.pad_t, p.pad_l) == (3, 3, 2, 0, 0) and (p.Ho - 1) * 2 + 2 >= p.Hi and (p.Wo - 1) * 2 + 2 >= p.Wi]
    assert [p for p in im if (p.KH, p.KW, p.stride, p.Cin, p.Hi, p.Wi, p.k_pad) == (14, 14, 14, 3, 28, 42, 592)]
    assert [p for p in im if (p.KH, p.KW) == (1, 1)] and [p for p in im if (p.KH, p.KW) == (1, 3) and p.Hi != p.Wi and p.pad_t != p.pad_l]
    assert [p for p in im if p.Cin == 1] and [p for p in im if p.B == 3]
    assert {(p.M, p.Ca, p.Cb) for p in P('fd_concat_channels_f16')} >= {(5, 8, 8), (77, 320, 640), (1, 1280, 8), (64, 8, 1280)}
    assert [p for p in P('fd_concat_channels_f16') if p.Ca == 0] and [p for p in P('fd_concat_channels_f16') if p.Cb == 0]
    assert [p for p in P('fd_concat_channels_f16') if p.M * (p.Ca + p.Cb) // 8 > 8192 * 256 and p.Ca != p.Cb]
    for entry in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        ps = P(entry)
        assert [p for p in ps if p.lds == p.cols == p.ldd] and [p for p in ps if p.lds > p.cols == p.ldd] and [p for p in ps if p.ldd > p.cols == p.lds]
        assert [p for p in ps if p.lds > p.cols and p.ldd > p.cols] and [p for p in ps if p.s_off > 0 and p.d_off > 0]
        assert [p for p in ps if p.rows == 1] and [p for p in ps if p.cols == 8]
    assert {p.rep for p in P('fd_repeat_rows_f16')} == {1, 2, 3}
    assert [p for p in P('fd_repeat_rows_f16') if p.rows * p.cols // 8 > 8192 * 256 and p.rep == 3]
    ax = [p for p in P('fd_axpby_f32') if not p.exp]
    assert {p.n for p in ax} >= {1, 255, 256, 257, 2048 * 256 + 3}
    assert {(p.a, p.b) for p in ax} >= {(1.0, L.SIGMA), (1 / L.VAE_SCALE, 0.0), (1.0, -L.SIGMA), (1 / L.SIGMA, -1 / L.SIGMA)}
    assert [p for p in ax if p.alias] and [p for p in ax if not p.y] and [p for p in P('fd_axpby_f32') if p.exp]
    assert {(p.B, p.L, p.D, p.vocab) for p in P('fd_embed_tokens_f16')} == {(3, 77, 768, 1000), (1, 1, 8, 2), (2, 5, 257, 50), (2, 77, 1024, 300)}
    assert {(p.B, p.T, p.D) for p in P('fd_vit_assemble_f16')} == {(3, 257, 1024), (1, 2, 8), (2, 50, 768), (4, 5, 257)}
    rb = P('fd_region_blend_f32')
    assert all((p.C, p.H, p.W) == (4, 13, 17) for p in rb) and {p.blend for p in rb} == {0.0, 1.0, 0.37, 1.5}
    for w in (0.0, 1.0, 0.37, 1.5):
        ps = [p for p in rb if p.blend == w]
        assert [p for p in ps if p.oy + p.sh < p.H and p.ox + p.sw < p.W and p.sh > 1 and p.sw > 1]               # inside
        assert [p for p in ps if p.oy + p.sh == p.H and p.oy > 0] and [p for p in ps if p.ox + p.sw == p.W and p.ox > 0]
        assert [p for p in ps if p.oy + p.sh > p.H and p.ox + p.sw <= p.W and p.oy < p.H]
        assert [p for p in ps if p.ox + p.sw > p.W and p.oy + p.sh <= p.H and p.ox < p.W]
        assert [p for p in ps if p.oy + p.sh > p.H and p.ox + p.sw > p.W and p.oy < p.H and p.ox < p.W]
        assert [p for p in ps if (p.oy, p.ox, p.sh, p.sw) == (0, 0, 13, 17)] and [p for p in ps if (p.sh, p.sw) == (1, 1)]
        assert [p for p in ps if p.oy == p.H] and [p for p in ps if p.ox > p.W] and [p for p in ps if p.sh == 0] and [p for p in ps if p.sw == -3]
    cv = P('fd_conv3x3_narrow_f16')
    assert {(p.B, p.Cin, p.H, p.W, p.Cout, p.rep2) for p in cv if p.bias} == {
        (1, 1, 5, 7, 8, 0), (2, 2, 1, 9, 64, 1), (1, 4, 9, 1, 320, 0), (1, 4, 2, 1024, 8, 0), (1, 3, 3, 5, 2048, 2), (2, 4, 6, 300, 24, 0)}
    assert [p for p in cv if not p.bias]
    p = next(p for p in cv if p.Cout == 24)             # 3 chunks, 85 pixel groups, one dead thread
    assert (p.Cout // 8, 256 // (p.Cout // 8), 256 - 256 // (p.Cout // 8) * (p.Cout // 8)) == (3, 85, 1)


def test_inputs_are_what_the_contracts_say():
    c = next(c for c in L.cases_of('fd_cast_f16_to_f32') if c.p.data == 'all')
    assert sorted((L._bits(L.inputs(c)['x']).int() & 0xFFFF).tolist()) == list(range(65536))
    for c in L.cases_of('fd_nhwc_f32_to_nchw_f32'):
        if c.p.B * c.p.HW * c.p.C < 64:
            continue
        x = L.inputs(c)['x'].double()
        e = x * float(L._f32(c.p.a)) + float(L._f32(c.p.b))
        for edge in (0.0, 1.0):
            exact = c.p.a in (1.0, 0.5, -2.0)              # 1 / 0.18215 has no fp32 x with x a == 1: the nearest x stands in
            assert bool((e == edge).any()) if exact else bool(((e - edge).abs() < 1e-7).any()), (c.id, edge)
            near = (e - edge).abs()
            assert int(((near > 0) & (near < 1e-5)).sum()) >= 4, (c.id, edge)
        assert float(e.max()) > 100 and float(e.min()) < -100
    c = next(c for c in L.cases_of('fd_axpby_f32') if c.p.y and c.p.n == 257 and not c.p.alias)
    inp = L.inputs(c)
    ax, by = L._f32(c.p.a) * inp['x'], L._f32(c.p.b) * inp['y']
    ulp = ax.abs() * 2.0 ** -23
    assert int((((ax + by).abs() <= 8 * ulp) & (ax != 0)).sum()) >= 64          # pairs that cancel to a few ulp
    c = next(c for c in L.cases_of('fd_axpby_f32') if not c.p.y and c.p.a == 1.0)
    x = L.inputs(c)['x']
    assert bool(((x == 0) & torch.signbit(x)).any())
    want = L.reference(c).value
    assert not bool(((want == 0) & torch.signbit(want)).any()), 'a x = -0 with y == NULL gives +0'
    for c in L.cases_of('fd_embed_tokens_f16'):
        inp = L.inputs(c)
        ids, V = inp['ids'].reshape(-1), c.p.vocab
        assert V - 1 in ids.tolist() and (c.p.B * c.p.L == 1 or 0 in ids.tolist())
        if c.p.B * c.p.L >= 16:
            assert bool((ids < 0).any()) and bool((ids >= V).any()) and ids.unique().numel() < ids.numel()
            tiny, big = inp['tok'][1].float(), inp['pos'][c.p.L - 1].float()
            assert int(ids[c.p.L - 1]) == 1 and float(tiny.abs().max()) < 1e-5 and float(big.abs().min()) > 90
            assert bool(((tiny.double() + big.double()) != (tiny + big).double()).any()), 'the fp32 sum does not round'
    for c in L.cases_of('fd_vit_assemble_f16'):
        pt = L.inputs(c)['patches'].view(c.p.B, c.p.T - 1, c.p.D)
        assert all(not torch.equal(pt[i], pt[j]) for i in range(c.p.B) for j in range(i))
    for c in L.cases_of('fd_region_blend_f32'):
        src = L.inputs(c)['src']
        sh, sw = L.blend_box(c.p)
        assert int((~torch.isnan(src)).sum()) == c.p.C * sh * sw


# --------------------------------------------------------------------------------------------------- the criterion
@pytest.fixture(scope='module')
def screen():
    '''case id -> (accepted: every legal emulation passes, worst ratio, {mutant: passes, for the mutants that apply}).'''
    out = {}
    for case in L.CASES:
        inp = L.inputs(case)
        want = L.reference(case, inp)
        forms = [L.emulate(case, inp)] + ([L.emulate(case, inp, 2)] if case.entry == 'fd_nhwc_f32_to_nchw_f32' else [])
        ratios = [L.worst(g, want, case) for g in forms]
        bad = {m: L.mutate(case, inp, m) for m in L.MUTANTS[case.entry]}
        assert all((b is not None) == L.applies(case, m) for m, b in bad.items())
        out[case.id] = (all(L.check(g, want, case) for g in forms), max(ratios), {m: L.check(b, want, case) for m, b in bad.items() if b is not None})
    return out


@pytest.mark.parametrize('case', L.CASES, ids=IDS)
def test_check_accepts_the_emulation_and_rejects_every_mutant(screen, case):
    accepted, ratio, mutants = screen[case.id]
    assert accepted and ratio <= 1.0, f'the fp32 emulation reaches {ratio:.3g} x the bound'
    for mutant, passes in mutants.items():
        assert not passes, f'{mutant} passes `check` at {case.id}'


def test_every_mutant_applies_to_a_case(screen):
    for entry, mutants in L.MUTANTS.items():
        for m in mutants:
            hit = [c.id for c in L.cases_of(entry) if m in screen[c.id][2]]
            assert hit, (entry, m)


def test_unfused_and_fused_affine_differ_and_both_pass():
    '''Why fd_nhwc_f32_to_nchw_f32 has a bound and not bits: with an inexact product and b != 0 the two legal forms give different
    bits on the same inputs (the table's own (a, b) pairs have an exact product or b == 0, where the forms agree), and `check`
    accepts both while rejecting a result one part in 10^6 off.'''
    base = next(c for c in L.cases_of('fd_nhwc_f32_to_nchw_f32') if c.p.HW == 35 and not c.p.clamp)
    case = base._replace(p=type(base.p)(**dict(vars(base.p), a=1 / L.VAE_SCALE, b=0.5)))
    inp = L.inputs(case)
    two, one = L.emulate(case, inp), L.emulate(case, inp, 2)
    assert not torch.equal(two, one)
    want = L.reference(case, inp)
    assert L.check(two, want, case) and L.check(one, want, case)
    assert not L.check(two * (1 + 1e-6), want, case)


def test_exp_form_k_is_computed_on_the_host_and_finite():
    k = L.exp_form_k()
    print(f'fd_axpby_f32 exp form: k = {k:.3f} (twice the fp32 CPU error of {k / 2:.3f} x 2^-24 |want|)')
    assert 2.0 <= k < 16.0 and k == k
    case = next(c for c in L.cases_of('fd_axpby_f32') if c.p.exp)
    inp = L.inputs(case)
    x, y = inp['x'], inp['y']
    assert float(x.min()) >= -30 and float(x.max()) <= 30 and bool((x == 0).any()) and bool((y == 0).any())
    assert L.worst(L.emulate(case, inp), L.reference(case, inp), case) <= 0.5 + 1e-9       # k is twice the emulation's own error


# --------------------------------------------------------------------------------------------------- the driver
def _mem(ptr, n, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_uint8 * (n * size)).from_address(ptr), dtype=dtype)


def _stand_in(case, inp, spill=False):
    '''hip.call replaced by the emulation, written through the output pointers the driver hands over.'''
    st = L.stage(case, inp)
    rows = L.emulate(case, inp)
    names = list(st.args)

    def call(name, *a):
        assert name == case.entry and len(a) == len(names) + 1
        r0 = 0
        for buf, (shape, strides, off) in st.outs.items():
            arg = next(i for i, v in enumerate(st.args.values()) if isinstance(v, L.Ptr) and v.buf == buf and v.off == off)
            n = (shape[0] - 1) * strides[0] + shape[1] if shape[0] else 0
            if n:
                mem = _mem(a[arg], n + (1 if spill else 0), rows.dtype)
                torch.as_strided(mem, shape, strides, 0).copy_(rows[r0:r0 + shape[0]])
                if spill:
                    mem[n] = 0
            r0 += shape[0]
    return call


def test_device_driver_against_a_host_stand_in(monkeypatch):
    '''run_on_device with the library replaced by the emulation: every entry point's staging hands over the pointers and reads the
    output back from where the reference expects it, and notices a write one element behind the output.'''
    from flexdiffuse_amd import hip
    monkeypatch.setattr(hip, 'stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    small = [c for c in L.CASES if L.alloc_bytes(c) < (1 << 20)]
    assert {c.entry for c in small} == set(L.ENTRY_POINTS)
    for case in small:
        inp = L.inputs(case)
        monkeypatch.setattr(hip, 'call', _stand_in(case, inp))
        r = L.run_on_device(case, 'cpu', inp)
        assert r.untouched and r.inputs_unchanged and L.check(r.out, L.reference(case, inp), case), case.id
        assert torch.equal(L._bits(r.out), L._bits(r.again)), case.id
    for entry in L.ENTRY_POINTS:
        case = L.refusal_case(entry)
        inp = L.inputs(case)
        monkeypatch.setattr(hip, 'call', _stand_in(case, inp, spill=True))
        assert L.run_on_device(case, 'cpu', inp).untouched is False, entry


def test_refusal_tables_name_real_arguments():
    for entry in L.ENTRY_POINTS:
        case = L.refusal_case(entry)
        names = list(L.stage(case).args)
        assert L.REFUSALS[entry], entry
        for override in L.REFUSALS[entry]:
            assert set(override) <= set(names), (entry, override)
        body = _body(_source(), entry)
        assert body.index('FD_CHECK_ARG') < body.index('hipLaunchKernelGGL') and body.count('FD_CHECK_ARG') >= 1
