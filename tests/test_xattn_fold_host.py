'''Context-folded cross-attention without a device: the algebra in fp64 torch on small random tensors (the fold, the per-head softmax, the
pad keys, the LayerNorm fold's two rows), and the launch rule's refusals through fd_gemm_plan (host logic only).'''
import math

import pytest
import torch


def _problem(seed=0, B=2, M=5, C=24, heads=3, L=7, G=10):
    g = torch.Generator().manual_seed(seed)
    d = C // heads
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    return dict(B=B, M=M, C=C, heads=heads, d=d, L=L, G=G, x=r(B, M, C) + 0.7, gamma=1 + 0.2 * r(C), beta=0.3 * r(C), wq=r(C, C) * C ** -0.5,
                k=r(B, L, C), v=r(B, L, C), wo=r(C, C) * C ** -0.5, bo=r(C))


def _unfolded(p):
    '''diffusers' attn2 on LayerNorm(x): q = LN(x) Wq^T, per-head softmax(q_h K_h^T) V_h, to_out, + x  (the softmax scale lives in Wq).'''
    B, M, C, H, d, L = (p[k] for k in ('B', 'M', 'C', 'heads', 'd', 'L'))
    xn = torch.nn.functional.layer_norm(p['x'], (C,), p['gamma'], p['beta'], 1e-5)
    q = (xn @ p['wq'].t()).view(B, M, H, d)
    s = torch.einsum('bmhd,blhd->bhml', q, p['k'].view(B, L, H, d))
    o = torch.einsum('bhml,blhd->bmhd', torch.softmax(s, -1), p['v'].view(B, L, H, d)).reshape(B, M, C)
    return o @ p['wo'].t() + p['bo'] + p['x']


def _fold(p):
    '''(K'^T [B][H*G][C], V'^T [B][C][H*G], colsum [B][H*G], bias row [B][H*G]) with G - L zero pad keys per head, as ops.xattn_fold lays them out.'''
    B, C, H, d, L, G = (p[k] for k in ('B', 'C', 'heads', 'd', 'L', 'G'))
    wqf = p['wq'] * p['gamma'][None, :]            # gain-folded q weight [out][in]
    bq = p['wq'] @ p['beta']                       # folded q bias
    kf = torch.zeros(B, H, G, C, dtype=torch.float64)
    vf = torch.zeros(B, C, H, G, dtype=torch.float64)
    bias = torch.zeros(B, H, G, dtype=torch.float64)
    kh, vh = p['k'].view(B, L, H, d), p['v'].view(B, L, H, d)
    kf[:, :, :L] = torch.einsum('blhj,hjc->bhlc', kh, wqf.view(H, d, C))
    vf[..., :L] = torch.einsum('chj,blhj->bchl', p['wo'].view(C, H, d), vh)
    bias[..., :L] = torch.einsum('blhj,hj->bhl', kh, bq.view(H, d))
    kf = kf.view(B, H * G, C)
    return kf, vf.view(B, C, H * G), kf.sum(-1), bias.view(B, H * G)


def _two_gemms(p, kf, vf, colsum, bias):
    B, M, C, H, L, G = (p[k] for k in ('B', 'M', 'C', 'heads', 'L', 'G'))
    x = p['x']
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    rstd = torch.rsqrt(var + 1e-5)
    # launch 1: the LayerNorm fold on the un-normalised rows, then the softmax over each head's L real keys; pad columns 0
    s = rstd * torch.einsum('bmc,bnc->bmn', x, kf) - rstd * mean * colsum[:, None, :] + bias[:, None, :]
    s = s.view(B, M, H, G)
    P = torch.zeros_like(s)
    P[..., :L] = torch.softmax(s[..., :L], -1)
    P = P.view(B, M, H * G)
    # launch 2
    return P, torch.einsum('bmn,bcn->bmc', P, vf) + p['bo'] + x


@pytest.mark.parametrize('seed,L,G', [(0, 7, 10), (1, 10, 10), (2, 1, 10), (3, 5, 8)])
def test_two_gemms_equal_the_unfolded_attention_in_fp64(seed, L, G):
    p = _problem(seed, L=L, G=G)
    P, out = _two_gemms(p, *_fold(p))
    assert torch.allclose(out, _unfolded(p), rtol=1e-11, atol=1e-11)
    Pv = P.view(p['B'], p['M'], p['heads'], G)
    assert bool((Pv[..., L:] == 0).all()) and torch.allclose(Pv.sum(-1), torch.ones(p['B'], p['M'], p['heads'], dtype=torch.float64), atol=1e-13)


def test_pad_keys_need_zero_value_rows_only_if_their_probability_is_zero():
    '''The pad columns of P are exactly 0, so whatever sits in the pad rows of V' cannot reach the output -- and zero pads make the folded
    operands blend linearly (a keyframe lerp of zeros stays zero).'''
    p = _problem(4)
    kf, vf, colsum, bias = _fold(p)
    vf2 = vf.clone().view(p['B'], p['C'], p['heads'], p['G'])
    vf2[..., p['L']:] = 123.0
    assert torch.equal(_two_gemms(p, kf, vf, colsum, bias)[1], _two_gemms(p, kf, vf2.view_as(vf), colsum, bias)[1])


def test_the_fold_is_linear_in_the_context():
    pa, pb = _problem(5), _problem(5)
    g = torch.Generator().manual_seed(9)
    pb['k'], pb['v'] = torch.randn(pa['k'].shape, generator=g, dtype=torch.float64), torch.randn(pa['v'].shape, generator=g, dtype=torch.float64)
    w = 0.37
    pm = dict(pa, k=pa['k'] + w * (pb['k'] - pa['k']), v=pa['v'] + w * (pb['v'] - pa['v']))
    for a, b, m in zip(_fold(pa), _fold(pb), _fold(pm)):
        assert torch.allclose(a + w * (b - a), m, rtol=1e-12, atol=1e-12)


def test_base_two_logits():
    '''The device path folds log2(e) into Wq and exponentiates base 2: the same softmax.'''
    s = torch.randn(4, 9, dtype=torch.float64)
    assert torch.allclose(torch.softmax(s, -1), torch.exp2(s * math.log2(math.e) - (s * math.log2(math.e)).max(-1, keepdim=True)[0]) /
                          torch.exp2(s * math.log2(math.e) - (s * math.log2(math.e)).max(-1, keepdim=True)[0]).sum(-1, keepdim=True))


def test_rule_and_refusals_through_fd_gemm_plan():
    from flexdiffuse_amd import hip, ops
    lib = hip.lib()
    plan = ops.xattn_fold_plan
    # the bench forward: 16 samples x 256 rows (128 workgroups of the 128-row tile), 16 x 64 rows (the 8x8 map: the 64-row tile)
    assert plan(16, 256, 1280, 8, 77) == 25 and plan(16, 256, 1280, 8, 77, parts=8) == 25 and plan(16, 64, 1280, 8, 77, parts=8) == 24
    assert plan(2, 128, 1280, 8, 77) == 24 and plan(2, 128, 1280, 8, 77, tile=25) == 25 and plan(2, 128, 1280, 8, 1) == 24 and plan(2, 128, 1280, 8, 80) == 24
    # refused: a tile of two samples' rows, more than 80 keys, no keys, a forced tile the form does not run on, operands of 2 GiB
    for args, kw, msg in (((2, 96, 1280, 8, 77), {}, b'straddle'), ((2, 32, 1280, 8, 77), {}, b'straddle'), ((2, 128, 1280, 8, 81), {}, b'softmax_valid'),
                          ((2, 128, 1280, 8, 0), {}, b'softmax_valid'), ((2, 64, 1280, 8, 77), {'tile': 25}, b'tile 24'),
                          ((2, 128, 1280, 8, 77), {'tile': 13}, b'tile 24'), ((2, 64 * 16384, 1280, 8, 77), {}, b'2 GiB')):
        assert plan(*args, **kw) == 0 and msg in lib.fd_last_error(), (args, lib.fd_last_error())
    # launch 2 writes the LayerNorm partial sums of its rows from 64 rows per sample on (8 slabs at C = 1280), not below
    assert ops.xattn_fold_out_slabs(16, 256, 1280, 640) == 8 and ops.xattn_fold_out_slabs(16, 64, 1280, 640) == 8
    assert ops.xattn_fold_out_slabs(2, 96, 1280, 640) == 0
    # which layers fold their context: heads x 80 must be below C
    assert ops.xattn_fold_layer(1280, 8, 77) and not ops.xattn_fold_layer(640, 8, 77) and not ops.xattn_fold_layer(320, 8, 77)
    assert not ops.xattn_fold_layer(1280, 8, 81)


def test_a_softmax_launch_is_refused_with_the_options_it_cannot_honour():
    import ctypes
    from flexdiffuse_amd import hip, ops
    lib = hip.lib()
    t, s = ctypes.c_int32(0), ctypes.c_int32(0)

    def rc(**kw):
        d = ops._xf_probs_desc(4096, 1280, (4096, 4096), 2, 128, 1280, 640, 77, 4096)
        d.ln_stats = 4096
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.fd_gemm_plan(ctypes.byref(d), ctypes.byref(t), ctypes.byref(s))
    assert rc() == 0 and t.value == 24 and s.value == 1
    for kw in (dict(residual=4096, ldr=640), dict(act=ops.ACT_GEGLU), dict(out_f32=1), dict(ln_stats=None), dict(ln_stats_out=4096),
               dict(trans_out=1), dict(split_k=2), dict(softmax_group=64), dict(N=600), dict(ldc=644), dict(bias=None)):
        assert rc(**kw) != 0, kw
