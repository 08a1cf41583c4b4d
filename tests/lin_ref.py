'''fd_cfg_linear_multistep_step_f32 (PLMS and K-LMS in one launch) restated in fp32 torch on the CPU, in the order of its
contract (include/flexdiffuse_hip.h): every operation separately rounded, every scalar rounded to fp32 first.  Shared by
tests/test_linear_multistep_host.py and tests/test_gpu_linear_multistep.py.'''
import torch


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def axpby(x, y, a, b):
    '''fd_axpby_f32: a x + b y, y = 0 when left out.'''
    yv = torch.zeros_like(x) if y is None else y.reshape(x.shape)
    return f32(a) * x + f32(b) * yv


def cfg_mix(eps, B, C, HW, cfg, g):
    '''The guided eps as NCHW (B, C, HW) from the NHWC rows [(cfg + 1) B HW][ld], unconditional half first.'''
    E = 2 if cfg else 1
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)
    return (ev[0] + f32(g) * (ev[1] - ev[0]) if cfg else ev[0]).contiguous()


def blend(xn, mask):
    '''fd_known_blend with its two exact branches; mask = (z0, n, m [HW], k1, k2).'''
    z0, n, m, k1, k2 = mask
    known = f32(k1) * z0.reshape(xn.shape) + f32(k2) * n.reshape(xn.shape)
    return torch.where(m == 1, xn, torch.where(m == 0, known, known + m * (xn - known)))


def kernel_ref(x, eps, form, hist, B, C, HW, cfg, g, weights, coef, mask=None, x_src=None, scale=None):
    '''x, hist rows, x_src: (B, C, HW) fp32.  Returns dict(x=x', h=the row h_out receives, keep=the row x_keep_out receives,
    scaled=the row x_scaled_out receives or None).'''
    e = cfg_mix(eps, B, C, HW, cfg, g)
    one = f32(1.0)
    w = [f32(v) for v in weights]
    n_prev = len(hist)
    if form == 0:
        cs, ce = (f32(v) for v in coef)
        xs = x if x_src is None else x_src
        h = e
        if n_prev == 0:
            E = e
        else:
            E = w[0] * e + w[1] * hist[0]
            for k in range(2, n_prev + 1):
                E = one * E + w[k] * hist[k - 1]
        xn = cs * xs + ce * E
    else:
        ns, is_, nis = (f32(v) for v in coef)
        x0 = one * x + ns * e
        h = is_ * x + nis * x0
        xn = one * x + w[0] * h
        for k in range(1, n_prev + 1):
            xn = one * xn + w[k] * hist[k - 1]
    if mask is not None:
        xn = blend(xn, mask)
    scaled = None if scale is None else f32(scale) * xn + f32(0.0) * f32(0.0)
    return {'x': xn, 'h': h, 'keep': x.clone(), 'scaled': scaled}


def cpu_ops(monkeypatch):
    '''ops.axpby and ops.cfg_linear_multistep_step replaced by the restatements above, so the schedulers run without a GPU.
    Returns the list every fused call is appended to: dict(form, n_prev, h_out, reads, keep, src, scaled) of data pointers.'''
    from flexdiffuse_amd import ops
    calls = []

    def fake_axpby(x, y, a, b, exp_half_x=False):
        assert not exp_half_x
        return axpby(x.contiguous(), y, a, b)

    def fake_step(x, eps_nhwc, form, hist, h_out, B, C, HW, cfg, guidance, weights, coef, mask=None, x_keep_out=None,
                  x_src=None, x_scaled_out=None, scale=0.0):
        hist = list(hist)
        v = lambda t: t.view(B, C, HW)                                   # noqa: E731
        r = kernel_ref(v(x).clone(), eps_nhwc, form, [v(t) for t in hist], B, C, HW, cfg, guidance, weights, coef, mask,
                       None if x_src is None else v(x_src), scale if x_scaled_out is not None else None)
        calls.append({'form': form, 'n_prev': len(hist), 'h_out': None if h_out is None else h_out.data_ptr(),
                      'reads': [t.data_ptr() for t in hist], 'keep': None if x_keep_out is None else x_keep_out.data_ptr(),
                      'src': None if x_src is None else x_src.data_ptr(), 'scaled': x_scaled_out is not None,
                      'weights': tuple(float(w) for w in weights)})
        if h_out is not None:
            h_out.copy_(r['h'].reshape(h_out.shape))
        if x_keep_out is not None:
            x_keep_out.copy_(r['keep'].reshape(x_keep_out.shape))
        x.copy_(r['x'].view_as(x))
        if x_scaled_out is not None:
            x_scaled_out.copy_(r['scaled'].view_as(x_scaled_out))
    monkeypatch.setattr(ops, 'axpby', fake_axpby)
    monkeypatch.setattr(ops, 'cfg_linear_multistep_step', fake_step)
    return calls


def kernel_mask(HW, rng):
    '''A mask holding 0, 1 and fractions.'''
    m = torch.rand((HW,), generator=rng)
    m[m < 0.3] = 0.0
    m[m > 0.7] = 1.0
    m[0], m[1], m[2] = 0.0, 1.0, 0.5
    return m
