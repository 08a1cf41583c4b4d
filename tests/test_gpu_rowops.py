'''The row kernels beside attention -- fd_layernorm_f16, fd_ln_row_stats_f16, fd_ln_finalize_stats_f32,
fd_softmax_rows_f16, fd_timestep_embedding_f16 -- on every dispatch branch and both sides of each boundary, with
strided rows, against float64 references of the same fp16-rounded inputs.  Needs an MI355X.'''
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS24 = 2.0 ** -24      # fp32 unit roundoff
PAD = 7.5               # what the padding columns hold before a launch


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def close(got, want, rtol, atol, what=''):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    ok = err <= atol + rtol * want.abs()
    assert bool(ok.all()), f'{what}: max err {err.max().item():.4g} (max |want| {want.abs().max().item():.4g}), {int((~ok).sum())} elements out'


def ln_rows(rows, C, seed):
    '''fp16 rows around 0.3 with deviation 2; every third row has mean 30 and deviation 0.1 (E[x^2] - E[x]^2 in fp32
    would lose the variance there; the fp16 values are multiples of 2^-6, so the kernel's fp32 row sum is exact).'''
    x = rnd((rows, C), seed) * 2 + 0.3
    x[1::3] = 30.0 + 0.1 * rnd((len(range(1, rows, 3)), C), seed + 1)
    return x.half()


def vpl(C):
    return 1 if C <= 512 else 2 if C <= 1024 else 4


LN_ROWS = (1, 5, 77, 8191, 8192, 8193)
LN_C = (8, 320, 512, 520, 1024, 1032, 1280, 2048)


@pytest.mark.parametrize('C', LN_C)
@pytest.mark.parametrize('rows', LN_ROWS)
def test_layernorm_and_row_stats_on_every_branch(dev, rows, C):
    '''The four branches of both dispatchers: two rows per wave (rows >= 8192, C <= 512: 8191 | 8192 | 8193, the last
    with a half-filled wave), one row per wave with 1, 2 or 4 vectors per lane (C 512 | 520 and 1024 | 1032).
    Bounds: the project's 1e-4 (fp32 output) and 2e-3 (fp16 output), absolute + relative.  Statistics: relative 1e-5 on
    rstd; on -mean * rstd relative 1e-5 plus what fp32 summation allows the mean: a lane adds 8 * VPL values in turn
    and the wave six butterfly levels, each rounding at most 2^-24 of sum |x|, one more for the division:
    |d mean| <= (8 VPL + 7) 2^-24 mean|x|, times rstd.  (Rows whose mean is near 0 make a purely relative bound on
    -mean * rstd meaningless.)'''
    from flexdiffuse_amd import hip, ops
    eps = 1e-5
    x16 = ln_rows(rows, C, 7 * rows + C)
    g, b = (1 + 0.1 * rnd((C,), 2)).float(), (0.1 * rnd((C,), 3)).float()
    x = x16.double()
    mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
    rstd = (var + eps).rsqrt()
    want = (x - mean) * rstd * g.double() + b.double()
    gd, bd = g.to(dev), b.to(dev)

    ldx, ldy = C + 8, C + 16
    xs = torch.full((rows, ldx), PAD, dtype=torch.float16)
    xs[:, :C] = x16
    xs = xs.to(dev)
    for xin in (x16.to(dev), xs[:, :C]):
        for out_f32 in (True, False):
            y = ops.layernorm(xin, gd, bd, eps, out_f32=out_f32)
            tol = 1e-4 if out_f32 else 2e-3
            close(y, want, tol, tol, f'layernorm out_f32={out_f32} ldx={xin.stride(0)}')
        st = ops.ln_row_stats(xin, eps).double().cpu()
        close(st[:, 0], rstd[:, 0], 1e-5, 0.0, 'rstd')
        want_b = (-mean * rstd)[:, 0]
        slack = (8 * vpl(C) + 7) * EPS24 * x.abs().mean(1) * rstd[:, 0]
        err = (st[:, 1] - want_b).abs()
        assert bool((err <= 1e-5 * want_b.abs() + slack).all()), f'-mean rstd: max err {err.max().item():.4g}'
    # strided output: the padding columns keep their bits
    for out_f32 in (True, False):
        dt = torch.float32 if out_f32 else torch.float16
        ybuf = torch.full((rows, ldy), PAD, dtype=dt, device=dev)
        hip.call('fd_layernorm_f16', xs.data_ptr(), ybuf.data_ptr(), gd.data_ptr(), bd.data_ptr(), rows, C, ldx, ldy, eps,
                 int(out_f32), hip.stream())
        torch.cuda.synchronize()
        tol = 1e-4 if out_f32 else 2e-3
        close(ybuf[:, :C], want, tol, tol, f'layernorm strided out_f32={out_f32}')
        assert bool((ybuf[:, C:] == PAD).all()), 'layernorm wrote into the padding columns of y'
    assert bool((xs[:, C:] == PAD).all())


@pytest.mark.parametrize('C', [12, 2056])
def test_layernorm_refuses_what_it_cannot_run(dev, C):
    from flexdiffuse_amd import ops
    x = torch.zeros((4, C), dtype=torch.float16, device=dev)
    g = torch.ones((C,), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        ops.layernorm(x, g, g)
    with pytest.raises(ValueError):
        ops.ln_row_stats(x)
    ok, g16 = torch.ones((4, 16), dtype=torch.float16, device=dev), torch.ones((16,), dtype=torch.float32, device=dev)
    assert float(ops.layernorm(ok, g16, g16).float().sub(1).abs().max()) == 0.0       # a constant row: 0 * gamma + beta


@pytest.mark.parametrize('n_tiles', [1, 2, 3, 4, 5, 8, 64])
def test_ln_finalize_stats_every_instantiation(dev, n_tiles):
    '''The 2 / 3 / 4 / 8 / any-count kernels against float64 arithmetic on the SAME fp32 partial sums.  Bound from the
    kernel's fp32 arithmetic: s1 and s2 are n_tiles-term sums (n_tiles roundings of at most 2^-24 sum |p| each), the
    variance s2 / N - mean^2 adds three more, so |d var| <= (n_tiles + 3) 2^-24 (sum |p2| / N + mean^2), and
    d rstd / rstd = d var / (2 (var + eps)) plus 6 * 2^-24 (the reciprocal square root to 2 ulp = 4, the addition of
    eps and the stored result one each); the mean adds (n_tiles + 2) 2^-24 sum |p1| / N to -mean * rstd.'''
    from flexdiffuse_amd import ops
    M, T, eps = 1000, 160, 1e-5
    N = n_tiles * T
    x = (rnd((M, n_tiles, T), 50 + n_tiles) * 2 + 0.3).half().double()
    parts = torch.stack([x.sum(2), (x * x).sum(2)], dim=-1).permute(1, 0, 2).contiguous().float()     # [n_tiles][M][2]
    got = ops.ln_finalize_stats(parts.to(dev), N, eps).double().cpu()
    p = parts.double()
    s1, s2 = p[:, :, 0].sum(0), p[:, :, 1].sum(0)
    mean = s1 / N
    var = (s2 / N - mean * mean).clamp(min=0)
    rstd = (var + eps).rsqrt()
    dvar = (n_tiles + 3) * EPS24 * (p[:, :, 1].abs().sum(0) / N + mean * mean)
    rel = dvar / (2 * (var + eps)) + 6 * EPS24
    err = (got[:, 0] - rstd).abs()
    assert bool((err <= rel * rstd).all()), f'rstd: max rel err {(err / rstd).max().item():.3g} (allowed {rel.max().item():.3g})'
    want_b = -mean * rstd
    allow = rel * want_b.abs() + rstd * (n_tiles + 2) * EPS24 * p[:, :, 0].abs().sum(0) / N
    err = (got[:, 1] - want_b).abs()
    assert bool((err <= allow).all()), f'-mean rstd: max err {err.max().item():.3g}'


def test_ln_finalize_clamps_a_cancelled_variance_and_refuses_bad_tile_counts(dev):
    '''A constant row of 100s whose sum-of-squares partials are each 1.0 short: s2 / N - mean^2 = -0.0078 in exact and
    in fp32 arithmetic (every operand is exact), far below -eps, so without the clamp at 0 the row is NaN.'''
    from flexdiffuse_amd import ops
    M, n_tiles, N, eps = 70, 4, 512, 1e-5
    parts = torch.empty((n_tiles, M, 2), dtype=torch.float32)
    parts[:, :, 0] = 128 * 100.0
    parts[:, :, 1] = 128 * 1e4
    parts[:, 33, 1] -= 1.0
    got = ops.ln_finalize_stats(parts.to(dev), N, eps).double().cpu()
    assert bool(torch.isfinite(got).all())
    rstd = eps ** -0.5
    assert abs(float(got[33, 0]) - rstd) <= 1e-5 * rstd and abs(float(got[33, 1]) + 100.0 * rstd) <= 1e-5 * 100.0 * rstd
    assert abs(float(got[0, 0]) - rstd) <= 1e-5 * rstd
    for bad in (0, 65):
        with pytest.raises(ValueError):
            ops.ln_finalize_stats(torch.zeros((max(bad, 1), M, 2), dtype=torch.float32, device=dev)[:bad], N, eps)
    assert bool(torch.isfinite(ops.ln_finalize_stats(parts.to(dev), N, eps)).all())


@pytest.mark.parametrize('scale', [1.0, 512 ** -0.5])
@pytest.mark.parametrize('pad', [0, 8])
@pytest.mark.parametrize('N', [8, 256, 2048, 2056, 4096, 9216])
def test_softmax_rows(dev, N, pad, scale):
    '''In-place row softmax at the VAE mid-block's row lengths (4096, 9216: the three `c += 2048` loops iterate) and
    around one full pass (2048 | 2056).  Rows: logits of deviation 3 and 12, a constant row, and a row holding fp16
    60000 (scale 1: exp(60000 - max) must not overflow).  The project's bound: rtol 5e-3, atol 2e-4; each row sums to 1
    within the fp16 rounding of its N terms: 2^-11 relative on each, 2^-25 absolute on the subnormal ones, plus 1e-5
    for the fp32 normalisation.'''
    from flexdiffuse_amd import hip
    ld = N + pad
    x = torch.cat([rnd((3, N), N + pad, 3.0), rnd((2, N), N + 1, 12.0), torch.full((1, N), 2.5), rnd((1, N), N + 2, 3.0)])
    x[-1, N // 3] = 60000.0
    rows = x.shape[0]
    buf = torch.full((rows, ld), PAD, dtype=torch.float16)
    buf[:, :N] = x.half()
    want = (buf[:, :N].double() * float(torch.tensor(scale, dtype=torch.float32))).softmax(-1)
    d = buf.to(dev)
    hip.call('fd_softmax_rows_f16', d.data_ptr(), rows, N, ld, scale, hip.stream())
    torch.cuda.synchronize()
    got = d.cpu()
    assert bool(torch.isfinite(got.float()).all())
    close(got[:, :N], want, 5e-3, 2e-4, 'softmax')
    assert bool((got[:, N:] == PAD).all()), 'softmax wrote into the padding columns'
    total = got[:, :N].double().sum(1)
    assert bool(((total - 1).abs() <= 2.0 ** -11 + N * 2.0 ** -25 + 1e-5).all()), total
    assert float(got[-1, N // 3]) == 1.0


def test_softmax_rows_refuses_a_row_length_off_the_vector_width(dev):
    from flexdiffuse_amd import ops
    with pytest.raises(ValueError):
        ops.softmax_rows_(torch.zeros((2, 12), dtype=torch.float16, device=dev))
    assert float(ops.softmax_rows_(torch.zeros((2, 8), dtype=torch.float16, device=dev)).float().sub(0.125).abs().max()) == 0.0


def _timestep_ref(t64, dim):
    half = dim // 2
    a = t64[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)[None]
    return torch.cat([a.cos(), a.sin()], dim=1)


def _timestep_f32(t64, dim):
    '''The kernel's formula, operation for operation, in torch fp32 on the CPU.'''
    half = dim // 2
    i = torch.arange(half, dtype=torch.float32)
    freq = torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * i / torch.tensor(float(half), dtype=torch.float32))
    a = t64.float()[:, None] * freq[None]
    return torch.cat([a.cos(), a.sin()], dim=1)


@pytest.mark.parametrize('dim', [320, 1280])
def test_timestep_embedding(dev, dim):
    '''[cos | sin](t * exp(-ln(10000) i / (dim / 2))) for every integer timestep 0..999 and three fractional ones, against
    float64.  The bound is not chosen: the fp32 restatement of the formula on the CPU differs from float64 by at most
    5.8e-5 (dim 320) / 7.1e-5 (dim 1280) -- the rounding of t * freq near t = 999 -- to which the fp16 half-ulp of
    values up to 1 (2^-12 = 2.44e-4) is added, and the device's expf / sinf / cosf get 2 x that sum:
    6.0e-4 / 6.3e-4.  The test recomputes the fp32 figure where it runs.'''
    from flexdiffuse_amd import hip
    t64 = torch.cat([torch.arange(1000, dtype=torch.float64), torch.tensor([0.25, 500.5, 998.75], dtype=torch.float64)])
    want = _timestep_ref(t64, dim)
    f32_err = float((_timestep_f32(t64, dim).double() - want).abs().max())
    documented = {320: 5.8e-5, 1280: 7.1e-5}[dim]
    assert 0.5 * documented < f32_err < 1.5 * documented, f32_err        # give or take the host's libm
    bound = 2 * (f32_err + 2.0 ** -12)
    B = t64.numel()
    t = t64.float().to(dev)
    out = torch.full((B, dim), PAD, dtype=torch.float16, device=dev)
    hip.call('fd_timestep_embedding_f16', t.data_ptr(), 1, out.data_ptr(), B, dim, hip.stream())
    torch.cuda.synchronize()
    err = float((out.double().cpu() - want).abs().max())
    print(f'timestep embedding dim {dim}: max err {err:.3g}, fp32 restatement {f32_err:.3g}, bound {bound:.3g}')
    assert err <= bound, f'max err {err:.3g} > {bound:.3g}'
    # t_stride 0: one device scalar for the whole batch
    for j in (999, 1001):
        one = torch.full((4, dim), PAD, dtype=torch.float16, device=dev)
        hip.call('fd_timestep_embedding_f16', t[j:].data_ptr(), 0, one.data_ptr(), 4, dim, hip.stream())
        torch.cuda.synchronize()
        assert torch.equal(one, out[j:j + 1].expand(4, dim))


def test_timestep_embedding_refusals(dev):
    from flexdiffuse_amd import hip
    t = torch.zeros((4,), dtype=torch.float32, device=dev)
    out = torch.zeros((4, 320), dtype=torch.float16, device=dev)
    for stride, dim in ((1, 321), (2, 320)):
        with pytest.raises(ValueError):
            hip.call('fd_timestep_embedding_f16', t.data_ptr(), stride, out.data_ptr(), 4 if stride == 1 else 2, dim, hip.stream())
    hip.call('fd_timestep_embedding_f16', t.data_ptr(), 1, out.data_ptr(), 4, 320, hip.stream())
    torch.cuda.synchronize()
    assert float(out[:, :160].float().sub(1).abs().max()) == 0.0 and float(out[:, 160:].float().abs().max()) == 0.0
