'''The layout, gather and elementwise entry points of csrc/elementwise.hip through the C ABI on every form: the case tables of
tests/layout_cases.py (both sides of every grid cap, padded leading dimensions and column slices, every replica count, the
rounding-boundary set of the fp32 -> fp16 conversion, clipped and empty blend boxes, the narrow convolution's thread mappings)
against plain torch references on the CPU -- bits where the contract is bits, a derived bound where it is not; one recorded and
replayed launch per entry point; what every entry point refuses; and the ops wrappers' own checks.  Needs an MI355X.'''
import pytest
import torch

import layout_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _ids(entry):
    return [c.id for c in L.cases_of(entry)]


def _run_case(dev, case):
    '''Two identical launches of the case.  Output buffers start as the sentinel (guards before and behind, padding columns where
    the entry point takes a leading dimension): an unwritten output element fails the comparison with the reference, a write outside
    the output fails `untouched`.  Input padding is NaN.  Inputs must keep their bits and the second launch must repeat the first.'''
    inp = L.inputs(case)
    r = L.run_on_device(case, dev, inp)
    want = L.reference(case, inp)
    ratio = L.worst(r.out, want, case)
    if want.bound is not None:
        print(f'{L.KERNEL[case.entry]}  {case.id}  err / bound = {ratio:.4f}')
    assert L.check(r.out, want, case), f'{L.KERNEL[case.entry]}: {case.id}: ' + (
        f'worst error is {ratio:.3g} x the bound' if want.bound is not None and ratio != float('inf') else
        f'{_differing(r.out, want)} elements differ from the reference')
    assert r.untouched, f'{L.KERNEL[case.entry]} wrote outside its output at {case.id}'
    assert r.inputs_unchanged, f'{L.KERNEL[case.entry]} changed an input at {case.id}'
    assert torch.equal(L._bits(r.out), L._bits(r.again)), 'two identical launches differ'
    return r


def _differing(got, want):
    ref = want.value if want.value is not None else want.exact
    if got.shape != ref.shape:
        return f'shape {tuple(got.shape)} against {tuple(ref.shape)}: all'
    if want.value is None:
        return int((~((got.double() - want.exact).abs() <= want.bound)).sum())
    nan = torch.isnan(ref) if ref.is_floating_point() else torch.zeros_like(ref, dtype=torch.bool)
    return int(((L._bits(got) != L._bits(ref)) & ~nan).sum() + (torch.isnan(got) != nan).sum())


@pytest.mark.parametrize('case', L.cases_of('fd_cast_f16_to_f32'), ids=_ids('fd_cast_f16_to_f32'))
def test_cast_f16_to_f32(dev, case):
    '''Bits of x.float() on all 65536 half patterns (NaN: NaN-ness) and across the cap.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_cast_f32_to_f16'), ids=_ids('fd_cast_f32_to_f16'))
def test_cast_f32_to_f16(dev, case):
    '''Bits of x.half() (round to nearest even) on the rounding-boundary set and across the cap.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_nchw_f32_to_nhwc_f16'), ids=_ids('fd_nchw_f32_to_nhwc_f16'))
def test_nchw_f32_to_nhwc_f16(dev, case):
    '''Bits of half(x * fp32(scale)) -- one product, one rounding -- permuted; +0 padding columns; identical replicas.'''
    r = _run_case(dev, case)
    p = case.p
    rows = r.out.view(p.rep, p.B * p.HW, p.c_pad)
    assert all(L.bits_equal(rows[k], rows[0]) for k in range(1, p.rep)), 'the replicas differ'
    assert bool((L._bits(rows[:, :, p.C:]) == 0).all()), 'padding columns are not +0'


@pytest.mark.parametrize('case', L.cases_of('fd_nhwc_f32_to_nchw_f32'), ids=_ids('fd_nhwc_f32_to_nchw_f32'))
def test_nhwc_f32_to_nchw_f32(dev, case):
    '''|got - (x a + b)| <= 2^-24 (|x a| + |x a + b|) (1 + 2^-20) against float64: one FMA or two roundings; with clamp01 the clamped
    reference, the same bound and 0 <= got <= 1 exactly.  The padding columns C .. ld - 1 of the input hold NaN.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_im2col_f16'), ids=_ids('fd_im2col_f16'))
def test_im2col_f16(dev, case):
    '''Bits of the index-arithmetic restatement k = (kh KW + kw) Cin + ci; +0 in columns K .. k_pad - 1 and for taps outside.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_concat_channels_f16'), ids=_ids('fd_concat_channels_f16'))
def test_concat_channels_f16(dev, case):
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_copy2d_f16'), ids=_ids('fd_copy2d_f16'))
def test_copy2d_f16(dev, case):
    '''Bits; the columns cols .. lds - 1 of the source (and whatever surrounds a column slice) hold NaN, those of the destination the
    sentinel.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_repeat_rows_f16'), ids=_ids('fd_repeat_rows_f16'))
def test_repeat_rows_f16(dev, case):
    _run_case(dev, case)


def test_repeat_rows_equals_rep_copies(dev):
    '''fd_repeat_rows_f16 with rep = 3 into a column slice gives the destination buffer of three fd_copy2d_f16 calls, bit for bit.'''
    from flexdiffuse_amd import hip
    case = next(c for c in L.cases_of('fd_repeat_rows_f16') if c.tag == 'slices-rep3')
    p = case.p
    r = L.run_on_device(case, dev)
    once = r.dev['dst'].cpu()
    r.dev['dst'].copy_(r.st.bufs['dst'])
    src, dst = r.dev['src'].data_ptr() + 2 * p.s_off, r.dev['dst'].data_ptr() + 2 * (L.GUARD + p.d_off)
    for k in range(p.rep):
        hip.call('fd_copy2d_f16', src, p.lds, dst + 2 * k * p.rows * p.ldd, p.ldd, p.rows, p.cols, hip.stream())
    torch.cuda.synchronize()
    assert torch.equal(L._bits(r.dev['dst'].cpu()), L._bits(once))


@pytest.mark.parametrize('case', L.cases_of('fd_axpby_f32'), ids=_ids('fd_axpby_f32'))
def test_axpby_f32(dev, case):
    '''Plain form: bits of fp32(a) x, fp32(b) y and their sum as three separately rounded fp32 operations (y == NULL: y = 0, so
    a x = -0 gives +0; out may alias x).  exp form: |got - exp(0.5 x) y b| <= k 2^-24 |want| against float64, k from the host.'''
    if case.p.exp:
        print(f'k = {L.exp_form_k():.3f}')
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_embed_tokens_f16'), ids=_ids('fd_embed_tokens_f16'))
def test_embed_tokens_f16(dev, case):
    '''Bits of half(float(tok[id]) + float(pos[l])); ids outside [0, vocab) read row 0 / vocab - 1 (NaN rows surround the table).'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_vit_assemble_f16'), ids=_ids('fd_vit_assemble_f16'))
def test_vit_assemble_f16(dev, case):
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_region_blend_f32'), ids=_ids('fd_region_blend_f32'))
def test_region_blend_f32(dev, case):
    '''Bits of d + w (s - d) as three fp32 operations on the clipped box; every other canvas element and the guards keep their bits;
    `src` is NaN outside the box; an empty box changes nothing and returns FD_OK.'''
    _run_case(dev, case)


@pytest.mark.parametrize('case', L.cases_of('fd_conv3x3_narrow_f16'), ids=_ids('fd_conv3x3_narrow_f16'))
def test_conv3x3_narrow_f16(dev, case):
    '''|err| <= 2^-11 |want| + 36 2^-24 (|bias| + sum |x w|) (1 + 2^-10) + 2^-25 against float64 over half(x scale) and the fp16
    weights; outputs are column slices of sentinel buffers; the y2 replicas carry the bits of y.'''
    _run_case(dev, case)


# --------------------------------------------------------------------------------------------------- plan replay
PLAN_CASES = [L.refusal_case(e) for e in L.ENTRY_POINTS] + [c for c in L.cases_of('fd_region_blend_f32') if c.tag == 'origin-beyond-w0.37'] + \
    [c for c in L.cases_of('fd_axpby_f32') if c.tag in ('exp-n1000-b0.7', 'n257-alias')]


@pytest.mark.parametrize('case', PLAN_CASES, ids=[c.id for c in PLAN_CASES])
def test_plan_replay_gives_the_eager_bits(dev, case):
    '''The FD_PLAN line of each entry point restates its argument list by hand: one recorded call, the output overwritten with what
    it held before, then the replay must give the eager launch's bits (a clipped-away blend records one op that replays as a no-op).'''
    from flexdiffuse_amd import hip
    r = L.run_on_device(case, dev)
    d, st = r.dev, r.st

    def reset():
        for name in st.outs:
            d[name].copy_(st.bufs[name])

    reset()
    plan = hip.Plan()
    with plan.record():
        hip.call(case.entry, *L.resolve(st.args, d), hip.stream())
    assert len(plan) == 1
    reset()
    plan.replay()
    torch.cuda.synchronize()
    out, untouched = L.collect(st, {n: d[n].cpu() for n in st.outs})
    assert untouched and torch.equal(L._bits(out), L._bits(r.out))


def test_plan_replay_timestep_embedding(dev):
    from flexdiffuse_amd import hip
    B, dim = 3, 320
    t = torch.tensor([999.0, 501.0, 0.0], device=dev)
    out = torch.full((B, dim), L.PAD, dtype=torch.float16, device=dev)
    plan = hip.Plan()
    with plan.record():
        hip.call('fd_timestep_embedding_f16', t.data_ptr(), 1, out.data_ptr(), B, dim, hip.stream())
    torch.cuda.synchronize()
    eager = out.clone()
    assert len(plan) == 1 and not bool((eager == L.PAD).any())
    out.fill_(L.PAD)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(L._bits(out), L._bits(eager))


# --------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize('entry', L.ENTRY_POINTS)
def test_refusals(dev, entry):
    '''Each malformed call is answered with ValueError naming the entry point (FD_EINVAL / FD_ESHAPE) by a check that precedes the
    launch in csrc/elementwise.hip, and launches nothing: the output buffers hold their bits after a sync.  The good call straight
    after each refusal passes `check`.'''
    from flexdiffuse_amd import hip
    case = L.refusal_case(entry)
    inp = L.inputs(case)
    want = L.reference(case, inp)
    r = L.run_on_device(case, dev, inp)
    d, st = r.dev, r.st
    names = list(st.args)
    good = L.resolve(st.args, d)

    def launch(arglist):
        for name in st.outs:
            d[name].copy_(st.bufs[name])
        try:
            hip.call(entry, *arglist, hip.stream())
        finally:
            torch.cuda.synchronize()
        return {n: d[n].cpu() for n in st.outs}

    for override in L.REFUSALS[entry]:
        with pytest.raises(ValueError, match=entry):
            launch(L.apply_overrides(good, names, override))
        for name in st.outs:
            assert torch.equal(L._bits(d[name].cpu()), L._bits(st.bufs[name])), f'a refused call wrote to its output ({override})'
        out, untouched = L.collect(st, launch(good))
        assert untouched and L.check(out, want, case), override


def test_concat_accepts_a_zero_width_half_next_to_the_refused_negative_one(dev):
    '''Ca = -8 is refused (it used to pass `Ca % 8 == 0`); Ca = 0, its nearest legal neighbour, copies b.'''
    for tag in ('3x0+16', '3x16+0'):
        case = next(c for c in L.cases_of('fd_concat_channels_f16') if c.tag == tag)
        inp = L.inputs(case)
        r = L.run_on_device(case, dev, inp)
        assert r.untouched and L.check(r.out, L.reference(case, inp), case)
        assert torch.equal(L._bits(r.out), L._bits(inp['b'] if case.p.Ca == 0 else inp['a']))


# --------------------------------------------------------------------------------------------------- the ops wrappers
def test_ops_concat_channels_reads_a_column_slice_as_a_slice(dev):
    from flexdiffuse_amd import ops
    g = torch.Generator().manual_seed(77)
    buf = torch.randn((37, 512), generator=g).half().to(dev)
    b = torch.randn((37, 64), generator=g).half().to(dev)
    a = buf[:, 64:384]
    assert not a.is_contiguous()
    got = ops.concat_channels(a, b)
    dense = ops.concat_channels(a.contiguous(), b)
    want = torch.cat([a.cpu(), b.cpu()], 1)
    assert torch.equal(L._bits(got.cpu()), L._bits(want)) and torch.equal(L._bits(dense.cpu()), L._bits(want))
    got = ops.concat_channels(b, buf[:, 8:16])
    assert torch.equal(L._bits(got.cpu()), L._bits(torch.cat([b.cpu(), buf[:, 8:16].cpu()], 1)))
    for bad_a, bad_b in ((a.float(), b), (a, b.float()), (a, b[:5]), (a.unsqueeze(0), b), (a, b[:, ::2]), (buf[:, ::2], b)):
        with pytest.raises(ValueError, match='concat_channels'):
            ops.concat_channels(bad_a, bad_b)


def test_ops_axpby_insists_on_fp32(dev):
    from flexdiffuse_amd import ops
    x = torch.randn(300, device=dev)
    y = torch.randn(300, device=dev)
    want = (torch.tensor(0.5) * x.cpu() + torch.tensor(-1.25) * y.cpu())
    assert torch.equal(L._bits(ops.axpby(x, y, 0.5, -1.25).cpu()), L._bits(want))
    for bad_x, bad_y in ((x.half(), y), (x, y.half()), (x.double(), None), (x, y[:299])):
        with pytest.raises(AssertionError):
            ops.axpby(bad_x, bad_y, 0.5, -1.25)
