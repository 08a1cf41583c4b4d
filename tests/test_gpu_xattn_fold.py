'''Context-folded cross-attention (fd_gemm_desc.softmax_group; ops.xattn_fold / xattn_fold_probs / xattn_fold_out) on the device.

The references are fp32 torch restatements from the SAME fp16 inputs.  Tolerances:
  * launch 1 against the fp32 softmax of the folded operands it reads: the stored probabilities are fp16 (<= 2^-12 absolute below 1) and
    the fp32 logit (1280 products) carries ~1e-4 absolute error, i.e. ~1e-4 relative on a probability: 2^-11 + 2^-9 P.
  * launch 2 against fp32 P V'^T + bias + residual from the fp16 P it reads: one fp16 rounding of the output, 2^-10 max(1, |ref|).
  * the two launches together against the UNFOLDED fp32 formula (LayerNorm, q projection, per-head softmax, P V, out projection, residual):
    at most 2 x the error of today's three launches (LayerNorm-fold q GEMM, fd_attention_f16, out-projection GEMM) against the same
    reference, max-abs and RMS, both measured in the test on the same inputs -- headroom for one more rounding of operands of like size.
    Measured on an MI355X (max-abs, RMS of the three launches -> of the two folded launches; |ref| <= 9.1):
        2 x 128 rows, 77 keys   4.02e-3, 4.28e-4 -> 3.79e-3, 4.37e-4   (finished pairs and partial slabs alike)
        2 x  64 rows, 77 keys   2.47e-3, 4.23e-4 -> 2.72e-3, 4.35e-4
        2 x 128 rows, 80 keys   2.86e-3, 4.20e-4 -> 3.06e-3, 4.33e-4
        2 x 128 rows,  1 key    3.56e-3, 3.82e-4 -> 3.56e-3, 4.38e-4
    Each run prints its own figures (-s).
Shapes: 2 samples x 128 rows (two 64-row tiles / one 128-row tile per sample, several workgroups), 64 rows per sample (the 8x8 map), C = 1280,
8 heads x 80 columns, 77 / 80 / 1 keys.'''
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C, HEADS, DH, G80 = 1280, 8, 160, 80
N = HEADS * G80


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    return torch.device('cuda:0')


_cache = {}


def layer(dev):
    '''One cross-attention layer's constants (shared, never modified): LayerNorm-folded pre-scaled q weight, out projection.'''
    if 'layer' not in _cache:
        from flexdiffuse_amd import ops
        g = torch.Generator().manual_seed(11)
        wq = torch.randn((C, C), generator=g) * C ** -0.5 * (ops.QK_LOG2E * DH ** -0.5) * 3.0
        gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
        q2 = ops.prep_linear_ln(wq, None, gamma, beta, dev)
        o2 = ops.prep_linear(torch.randn((C, C), generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.2, dev)
        _cache['layer'] = (q2, o2, q2.w.t().contiguous())
    return _cache['layer']


def inputs(dev, B, HW, L, seed=0):
    '''(x, k, v, vt, fold) of one shape, cached: hidden states with a row mean (the fold's colsum term matters), context projections.'''
    key = (B, HW, L, seed)
    if key not in _cache:
        from flexdiffuse_amd import ops
        q2, o2, q2t = layer(dev)
        g = torch.Generator().manual_seed(1000 * B + HW + L + seed)
        x = (torch.randn((B * HW, C), generator=g) * 1.3 + torch.randn((B * HW, 1), generator=g) * 0.8).half().to(dev)
        k = torch.randn((B * L, C), generator=g).half().to(dev)
        v = torch.randn((B * L, C), generator=g).half().to(dev)
        ldv = (L + 7) // 8 * 8
        vt = torch.zeros((B, C, ldv), dtype=torch.float16, device=dev)
        vt[:, :, :L] = v.view(B, L, C).transpose(1, 2)
        kf, vf = ops.xattn_fold(k, v, q2t, o2.w, B, L, HEADS)
        fold = ops.XFold(kf, vf, ops.xattn_fold_rows(kf, k, q2.bias, L, HEADS), L)
        _cache[key] = (x, k, v, vt, fold)
    return _cache[key]


def stats_of(x, form):
    '''LayerNorm statistics of the rows of x as the producers hand them over: finished pairs, or 8 partial slabs (sum, sum of squares per
    160-column tile).  -> (what launch 1 takes, the finished pairs)'''
    from flexdiffuse_amd import ops
    if form == 'pairs':
        st = ops.ln_row_stats(x)
        return st, st
    xs = x.float().view(x.shape[0], 8, 160)
    parts = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).contiguous()
    return parts, ops.ln_finalize_stats(parts, C)


def probs_ref(x, pairs, fold, B, HW, L):
    '''fp32 per-head softmax (base 2) of the LayerNorm-fold logits from the folded fp16 operands launch 1 reads.'''
    xs = x.float().view(B, HW, C)
    acc = torch.einsum('bmc,bnc->bmn', xs, fold.kf.float())
    st = pairs.view(B, HW, 2)
    s = acc * st[..., 0:1] + st[..., 1:2] * fold.rows[:, 0].unsqueeze(1) + fold.rows[:, 1].unsqueeze(1)
    s = s.view(B, HW, HEADS, G80)[..., :L]
    p = torch.softmax(s * math.log(2.0), -1)
    out = torch.zeros((B, HW, HEADS, G80), device=x.device)
    out[..., :L] = p
    return out.view(B * HW, N)


def unfolded_ref(x, k, v, B, HW, L, dev, residual=True):
    '''The unfolded formula in fp32: LN-fold q projection (fp16 weights, fp32 bias), per-head softmax over L keys, P V, out projection, + x.'''
    q2, o2, _ = layer(dev)
    xf = x.float()
    mean, var = xf.mean(1, keepdim=True), xf.var(1, unbiased=False, keepdim=True)
    xn = (xf - mean) * torch.rsqrt(var + 1e-5)
    q = (xn @ q2.w.float().t() + q2.bias[:C]).view(B, HW, HEADS, DH)
    kk, vv = k.float().view(B, L, HEADS, DH), v.float().view(B, L, HEADS, DH)
    p = torch.softmax(torch.einsum('bmhd,blhd->bhml', q, kk) * math.log(2.0), -1)
    o = torch.einsum('bhml,blhd->bmhd', p, vv).reshape(B * HW, C)
    return o @ o2.w.float().t() + o2.bias[:C] + (xf if residual else 0.0)


def three_launches(x, k, vt, B, HW, L, dev):
    from flexdiffuse_amd import ops
    q2, o2, _ = layer(dev)
    q = ops.gemm(x, q2, ln_stats=ops.ln_row_stats(x))
    o = ops.attention(q, k, vt, B, HEADS, HW, L, DH, q_prescaled=True)
    return ops.gemm(o, o2, residual=x)


def folded(x, fold, B, HW, L, residual=True, stats='pairs', tile=0, ln_stats_out=None):
    from flexdiffuse_amd import ops
    _, o2, _ = layer(dev=x.device)
    p = ops.xattn_fold_probs(x, fold, stats_of(x, stats)[0], B, HW, L, tile=tile)
    return ops.xattn_fold_out(p, fold, o2.bias, x if residual else None, B, HW, ln_stats_out=ln_stats_out)


# ------------------------------------------------------------------------------------------------------------------ launch 1
@pytest.mark.parametrize('HW,L,form,tile', [(128, 77, 'pairs', 24), (128, 77, 'parts', 24), (128, 77, 'pairs', 25), (128, 77, 'parts', 25),
                                            (128, 80, 'pairs', 0), (128, 80, 'parts', 25), (128, 1, 'pairs', 0), (128, 1, 'parts', 25),
                                            (64, 77, 'pairs', 0), (64, 77, 'parts', 0)])
def test_probs_launch(dev, HW, L, form, tile):
    from flexdiffuse_amd import ops
    B = 2
    x, k, v, vt, fold = inputs(dev, B, HW, L)
    assert ops.xattn_fold_plan(B, HW, C, HEADS, L, parts=8 if form == 'parts' else 0, tile=tile) == (tile or 24)
    st, pairs = stats_of(x, form)
    p = ops.xattn_fold_probs(x, fold, st, B, HW, L, tile=tile)
    assert p.shape == (B * HW, N) and p.dtype == torch.float16
    ref = probs_ref(x, pairs, fold, B, HW, L)
    pv = p.float().view(B * HW, HEADS, G80)
    assert bool((pv[..., L:] == 0).all()), 'pad columns must be exactly 0'
    err = (p.float() - ref).abs()
    print(f'HW {HW} L {L} {form} tile {tile}: max |P - ref| {float(err.max()):.3e}, max row-sum error {float((pv.sum(-1) - 1).abs().max()):.3e}')
    assert bool((err <= 2.0 ** -11 + 2.0 ** -9 * ref).all()), float(err.max())
    # each head's valid columns sum to 1 within the fp16 rounding of its (at most 80) terms: sum_i P_i 2^-11 = 2^-11, doubled for the fp32 steps
    assert float((pv.sum(-1) - 1).abs().max()) <= 2.0 ** -10


def test_probs_refuses_a_tile_of_two_samples(dev):
    '''96 rows per sample: a 64-row tile would hold rows of two samples.  fd_gemm_plan shows the refusal (the caller keeps its unfolded
    launches), the launch itself is refused before anything runs, and the unfolded launches of the same shape are right.'''
    from flexdiffuse_amd import ops
    B, HW, L = 2, 96, 77
    assert ops.xattn_fold_plan(B, HW, C, HEADS, L) == 0
    x, k, v, vt, fold = inputs(dev, B, HW, L)
    with pytest.raises(ValueError, match='straddle'):
        ops.xattn_fold_probs(x, fold, ops.ln_row_stats(x), B, HW, L)
    ref = unfolded_ref(x, k, v, B, HW, L, dev)
    got = three_launches(x, k, vt, B, HW, L, dev).float()
    assert float((got - ref).abs().max()) <= 2e-2 * float(ref.abs().max())
    # more than 80 keys, a foreign tile id
    assert ops.xattn_fold_plan(B, 128, C, HEADS, 81) == 0 and ops.xattn_fold_plan(B, 64, C, HEADS, 77, tile=25) == 0 and ops.xattn_fold_plan(B, 128, C, HEADS, 77, tile=12) == 0


# ------------------------------------------------------------------------------------------------------------------ launch 2
@pytest.mark.parametrize('B,HW,res', [(2, 128, 'full'), (2, 128, None), (4, 128, 'wrap'), (2, 64, 'full'), (2, 64, None), (8, 64, 'wrap')])
@pytest.mark.parametrize('with_stats', [True, False])
def test_out_launch(dev, B, HW, res, with_stats):
    '''P V'^T + bias (+ residual; 'wrap': a residual of 256 rows read modulo its row count) with per-sample weights, with and without the
    LayerNorm partial sums of the output (8 slabs, compared with fd_ln_row_stats_f16 of the stored rows at the tolerance of the existing statistics tests).'''
    from flexdiffuse_amd import ops
    L = 77
    _, o2, _ = layer(dev)
    x, k, v, vt, fold = inputs(dev, B, HW, L)
    p = ops.xattn_fold_probs(x, fold, ops.ln_row_stats(x), B, HW, L)
    r = None if res is None else (x if res == 'full' else x[:256])
    slabs = ops.xattn_fold_out_slabs(B, HW, C, N)
    assert slabs == 8
    st = torch.full((slabs, B * HW, 2), float('nan'), dtype=torch.float32, device=dev) if with_stats else None
    out = ops.xattn_fold_out(p, fold, o2.bias, r, B, HW, ln_stats_out=st)
    ref = torch.einsum('bmn,bcn->bmc', p.float().view(B, HW, N), fold.vf.float()).reshape(B * HW, C) + o2.bias[:C]
    if r is not None:
        ref = ref + r.float().repeat(B * HW // r.shape[0], 1)
    err = (out.float() - ref).abs()
    print(f'B {B} HW {HW} residual {res} stats {with_stats}: max |out - ref| {float(err.max()):.3e}')
    assert bool((err <= 2.0 ** -10 * ref.abs().clamp(min=1.0)).all()), float(err.max())
    if with_stats:
        assert bool(torch.isfinite(st).all())
        s2, want = ops.ln_finalize_stats(st, C), ops.ln_row_stats(out)
        assert float(((s2[:, 0] - want[:, 0]).abs() / want[:, 0]).max()) < 2e-4
        assert float((s2[:, 1] - want[:, 1]).abs().max()) < 2e-4 * max(1.0, float(want[:, 1].abs().max()))


# ------------------------------------------------------------------------------------------------------- both against the unfolded path
@pytest.mark.parametrize('B,HW,L,form', [(2, 128, 77, 'pairs'), (2, 128, 77, 'parts'), (2, 64, 77, 'pairs'), (2, 128, 80, 'pairs'), (2, 128, 1, 'pairs')])
def test_two_launches_against_the_unfolded_path(dev, B, HW, L, form):
    '''max-abs / RMS error against the unfolded fp32 formula: folded <= 2 x today's three launches (both measured here, printed).'''
    x, k, v, vt, fold = inputs(dev, B, HW, L)
    ref = unfolded_ref(x, k, v, B, HW, L, dev)
    e3 = three_launches(x, k, vt, B, HW, L, dev).float() - ref
    e2 = folded(x, fold, B, HW, L, stats=form).float() - ref
    m3, r3, m2, r2 = float(e3.abs().max()), float(e3.pow(2).mean().sqrt()), float(e2.abs().max()), float(e2.pow(2).mean().sqrt())
    print(f'B {B} HW {HW} L {L} {form}: three launches max {m3:.3e} rms {r3:.3e}; folded max {m2:.3e} rms {r2:.3e} (|ref| max {float(ref.abs().max()):.2f})')
    assert m2 <= 2.0 * m3 and r2 <= 2.0 * r3, (m2, m3, r2, r3)


# ------------------------------------------------------------------------------------------------------------------ the fold
def test_fold_against_fp32_and_in_place(dev):
    from flexdiffuse_amd import ops
    B, L = 2, 77
    q2, o2, q2t = layer(dev)
    x, k, v, vt, fold = inputs(dev, B, 128, L)
    kf_ref = torch.einsum('blhj,chj->bhlc', k.float().view(B, L, HEADS, DH), q2t.float().view(C, HEADS, DH))
    vf_ref = torch.einsum('chj,blhj->bchl', o2.w.float().view(C, HEADS, DH), v.float().view(B, L, HEADS, DH))
    kf, vf = fold.kf.float().view(B, HEADS, G80, C), fold.vf.float().view(B, C, HEADS, G80)
    assert bool((kf[:, :, L:] == 0).all()) and bool((vf[..., L:] == 0).all()), 'pad keys must be zero'
    for got, ref, name in ((kf[:, :, :L], kf_ref, 'kf'), (vf[..., :L], vf_ref, 'vf')):
        err = (got - ref).abs()
        print(f'{name}: max |err| {float(err.max()):.3e} at |ref| max {float(ref.abs().max()):.3f}')
        # fp32 accumulation of 160 products, one rounding to fp16 (2^-11 relative; 2^-24 absolute floor of the subnormals is far below)
        assert bool((err <= 2.0 ** -11 * ref.abs() + 1e-5 * float(ref.abs().max())).all())
    rows_ref0 = fold.kf.float().sum(-1)
    rows_ref1 = torch.zeros((B, HEADS, G80), device=dev)
    rows_ref1[..., :L] = torch.einsum('blhj,hj->bhl', k.float().view(B, L, HEADS, DH), q2.bias[:C].view(HEADS, DH))
    assert torch.allclose(fold.rows[:, 0], rows_ref0, rtol=1e-5, atol=1e-4 * float(rows_ref0.abs().max()))
    assert torch.allclose(fold.rows[:, 1], rows_ref1.view(B, N), rtol=1e-5, atol=1e-5 * float(rows_ref1.abs().max()))
    # in-place rewrite from another context: same addresses, new values, pads untouched
    g = torch.Generator().manual_seed(5)
    k2, v2 = torch.randn((B * L, C), generator=g).half().to(dev), torch.randn((B * L, C), generator=g).half().to(dev)
    kc, vc, rc = fold.kf.clone(), fold.vf.clone(), fold.rows.clone()
    ptrs = (kc.data_ptr(), vc.data_ptr(), rc.data_ptr())
    a, b = ops.xattn_fold(k2, v2, q2t, o2.w, B, L, HEADS, out=(kc, vc))
    r = ops.xattn_fold_rows(a, k2, q2.bias, L, HEADS, out=rc)
    assert (a.data_ptr(), b.data_ptr(), r.data_ptr()) == ptrs
    fresh = ops.xattn_fold(k2, v2, q2t, o2.w, B, L, HEADS)
    assert torch.equal(a, fresh[0]) and torch.equal(b, fresh[1]) and not torch.equal(a, fold.kf)


def test_lerp_of_folds_is_the_fold_of_the_lerp(dev):
    '''K' and V' are linear in K and V: blending two folded keyframes (fd_lerp_f16) equals folding the blended K / V within fp16 rounding --
    three roundings on one side (two folds, the blend), two on the other (the blend, the fold): 3 x 2^-11 of the larger magnitude involved.'''
    from flexdiffuse_amd import ops
    B, L, w = 2, 77, 0.37
    q2, o2, q2t = layer(dev)
    _, ka, va, _, fa = inputs(dev, B, 128, L)
    _, kb, vb, _, fb = inputs(dev, B, 128, L, seed=1)
    lk, lv = ops.lerp_f16(fa.kf, fb.kf, w), ops.lerp_f16(fa.vf, fb.vf, w)
    fk, fv = ops.xattn_fold(ops.lerp_f16(ka, kb, w), ops.lerp_f16(va, vb, w), q2t, o2.w, B, L, HEADS)
    for a, b, ea, eb, name in ((lk, fk, fa.kf, fb.kf, 'kf'), (lv, fv, fa.vf, fb.vf, 'vf')):
        mag = torch.maximum(ea.float().abs(), eb.float().abs())
        err = (a.float() - b.float()).abs()
        # the fold of the blend also carries the blend's rounding of each of its 160 inputs (random signs): sqrt(160) 2^-12 of a typical product
        tol = 3 * 2.0 ** -11 * mag + 160 ** 0.5 * 2.0 ** -12 * float(mag.mean())
        print(f'{name}: max |lerp(fold) - fold(lerp)| {float(err.max()):.3e}, worst err / tol {float((err / tol.clamp(min=1e-9)).max()):.3f}')
        assert bool((err <= tol).all())


# ------------------------------------------------------------------------------------------------------------------ determinism
def test_fifty_launches_are_bit_equal(dev):
    '''A fixed count of 50 launches of each kernel on the same inputs, stopped at the first difference.'''
    from flexdiffuse_amd import ops
    B, HW, L = 2, 128, 77
    q2, o2, q2t = layer(dev)
    x, k, v, vt, fold = inputs(dev, B, HW, L)
    parts, _ = stats_of(x, 'parts')
    st = torch.empty((8, B * HW, 2), dtype=torch.float32, device=dev)

    def once():
        p = ops.xattn_fold_probs(x, fold, parts, B, HW, L)
        out = ops.xattn_fold_out(p, fold, o2.bias, x, B, HW, ln_stats_out=st)
        kf, vf = ops.xattn_fold(k, v, q2t, o2.w, B, L, HEADS)
        return p, out, st.clone(), kf, vf, ops.xattn_fold_rows(kf, k, q2.bias, L, HEADS)
    first = once()
    for i in range(49):
        again = once()
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f'launch {i + 2} differs'


# ------------------------------------------------------------------------------------------------------------------ UNet level
def _psnr(a, b):
    a, b = a.float(), b.float()
    return float(10 * torch.log10((b.max() - b.min()) ** 2 / (a - b).pow(2).mean()))


@pytest.fixture(scope='module')
def mini(dev):
    '''The mini UNet (320 / 640 / 1280 channels, 8 heads): its mid block is a C = 1280 cross-attention with head dim 160; 32 x 32 latents put
    64 rows per sample there (the 8x8 map), the smallest map the folded form takes.'''
    from flexdiffuse_amd import build
    from flexdiffuse_amd.unet import UNet2DConditionModel
    sds = build.synthetic_state_dicts('mini', seed=0, parts=('unet',))
    ucfg = build.configs('mini')[0]
    unet = UNet2DConditionModel(sds['unet'], ucfg, dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 32, 32), generator=g).to(dev)
    ctxs = [torch.randn((4, 77, ucfg.cross_attention_dim), generator=g).half().to(dev) for _ in range(2)]
    return unet, x, ctxs


def _forward(unet, x, ctx, fold_on):
    from flexdiffuse_amd import ops
    saved = ops.XATTN_FOLD
    ops.XATTN_FOLD = fold_on
    try:
        return unet.forward_nhwc(x, 400.0, ctx, rep=2).clone()
    finally:
        ops.XATTN_FOLD = saved


def test_unet_folded_against_unfolded_and_replays(dev, mini):
    from flexdiffuse_amd import hip, ops
    unet, x, ctxs = mini
    assert ops.XATTN_FOLD, 'the folded form is the default'
    on = _forward(unet, x, ctxs[0], True)
    assert unet.mid_attn.ctx_fold is not None and ops.xattn_fold_plan(4, 64, 1280, 8, 77) == 24
    off = _forward(unet, x, ctxs[0], False)
    assert not torch.equal(on, off), 'the knob must change the launches'
    p = _psnr(on, off)
    print(f'mini UNet, 4 x 32 x 32 latents: folded vs unfolded PSNR {p:.1f} dB')
    assert p >= 40.0
    # eager, launch plan and HIP graph: bit-equal
    t_dev = torch.full((1,), 400.0, device=dev)
    eager = unet.forward_nhwc(x, t_dev, ctxs[0], rep=2).clone()
    pool, plan = torch.cuda.MemPool(), hip.Plan()
    with torch.cuda.use_mem_pool(pool, device=dev), plan.record():
        eps = unet.forward_nhwc(x, t_dev, ctxs[0], rep=2)
    eps.zero_()
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(eps, eager)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        unet.forward_nhwc(x, t_dev, ctxs[0], rep=2)
    torch.cuda.current_stream().wait_stream(s)
    with torch.cuda.graph(graph):
        geps = unet.forward_nhwc(x, t_dev, ctxs[0], rep=2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(geps, eager)
    # a new context of the same shape: rewritten in place (same addresses, same generation), and the recorded plan sees it
    f, gen = unet.mid_attn.ctx_fold, unet.ctx_generation
    ptrs = (f.kf.data_ptr(), f.vf.data_ptr(), f.rows.data_ptr())
    want = unet.forward_nhwc(x, t_dev, ctxs[1], rep=2).clone()
    f2 = unet.mid_attn.ctx_fold
    assert (f2.kf.data_ptr(), f2.vf.data_ptr(), f2.rows.data_ptr()) == ptrs and unet.ctx_generation == gen
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(eps, want) and not torch.equal(want, eager)


def test_unet_schedule_mode(dev, mini):
    '''Two keyframes: the folded operands live in the arenas and blend with K / V^T; against the unfolded launches on the same blend.'''
    unet, x, ctxs = mini
    h = unet.set_context_keyframes(ctxs)
    f = unet.mid_attn.ctx_fold
    assert f is not None
    arena = unet._ctx_sched['arenas'][-1]
    lo, hi = arena.data_ptr(), arena.data_ptr() + 2 * arena.numel()
    assert lo <= f.kf.data_ptr() < hi and lo <= f.vf.data_ptr() < hi and f.kf.data_ptr() % 16 == 0 and f.vf.data_ptr() % 16 == 0
    unet.blend_context(0, 0.3)
    assert bool((f.kf.view(4, 8, 80, 1280)[:, :, 77:] == 0).all()) and bool((f.vf.view(4, 1280, 8, 80)[..., 77:] == 0).all())
    assert torch.allclose(f.rows[:, 0], f.kf.float().sum(-1), rtol=1e-5, atol=1e-3)
    on = _forward(unet, x, h, True)
    off = _forward(unet, x, h, False)
    p = _psnr(on, off)
    print(f'schedule mode, w = 0.3: folded vs unfolded PSNR {p:.1f} dB')
    assert not torch.equal(on, off) and p >= 40.0
    unet.set_context(ctxs[0])       # leaves schedule mode: buffers of its own again
    assert unet._ctx_sched is None and unet.mid_attn.ctx_fold is not None and not (lo <= unet.mid_attn.ctx_fold.kf.data_ptr() < hi)
