'''The composite step entry points (fd_composite_ddim_step_f32, fd_composite_multistep_step_f32,
fd_composite_linear_multistep_step_f32) restated in fp32 torch on the CPU: the composited guided value `e` in the kernel's
order (include/flexdiffuse_hip.h), handed as single-block rows (CFG off) to the restatements the sibling entry points are pinned
by -- dpm_ref.kernel_ref, lin_ref.kernel_ref -- and to the DDIM + step-noise arithmetic stated here.  Every operation is
separately rounded, every scalar rounded to fp32 first.  Shared by tests/test_composite_loop_host.py and
tests/test_gpu_composite_loop.py.'''
import numpy as np
import torch

import dpm_ref
import lin_ref
import philox_ref

f32 = lin_ref.f32


def weight_maps(n, HW, rng):
    '''fp32 [n][HW] holding what a blend that ignored order, zeros or exact weights would get wrong: cells where every entity is
    0, cells where two or more overlap, zeros inside a map, and a weight of exactly 1.0 (`check_maps` asserts all of it).'''
    if n == 0:
        return None
    wm = torch.rand((n, HW), generator=rng)
    wm[wm < 0.35] = 0.0
    wm[:, :7] = 0.0                     # outside every box
    wm[:, 7] = 0.625                    # every entity overlaps here
    wm[0, 8] = 1.0                      # an exact weight: still the lerp
    wm[n - 1, 9] = 1.0
    check_maps(wm)
    return wm


def check_maps(wm):
    assert bool((wm == 0).all(0).any()), 'no cell outside every entity'
    assert bool((wm == 1.0).any()), 'no weight of exactly 1.0'
    assert bool(((wm != 0) & (wm != 1.0)).any()), 'no fractional weight'
    if wm.shape[0] > 1:
        assert bool(((wm != 0).sum(0) >= 2).any()), 'no cell where two entities overlap'
        assert bool((((wm != 0).sum(0) >= 1) & ((wm == 0).sum(0) >= 1)).any()), 'no cell with a zero beside a weight'


def composite_e(eps, wm, B, C, HW, cfg, g):
    '''The guided value (B, C, HW) of the rep-major rows eps [(cfg + 1 + n) B HW][ld]: v = bg; for k ascending, where
    w_k != 0: v = v + w_k (entity_k - v); with cfg: u + g (v - u).'''
    n = 0 if wm is None else wm.shape[0]
    first = 1 if cfg else 0
    E = first + 1 + n
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)
    v = ev[first].clone()
    for k in range(n):
        w = wm[k].reshape(1, 1, HW)
        v = torch.where(w != 0, v + w * (ev[first + 1 + k] - v), v)
    if cfg:
        v = ev[0] + f32(g) * (v - ev[0])
    return v.contiguous()


def rows(e):
    '''(B, C, HW) -> the single-block NHWC rows [B HW][C] a CFG-off entry point reads.'''
    B, C, HW = e.shape
    return e.permute(0, 2, 1).reshape(B * HW, C).contiguous()


def normals(noise, B, C, HW, per, draw):
    '''The step noise of a (B, C, HW) launch as philox_ref states it, rounded to fp32 (the host tests' z; the GPU tests read
    the device's own stream, fd_philox_normal_f32 at stream 0, whose distance to this one tests/test_gpu_step_noise.py bounds).'''
    assert (B * C * HW) % per == 0
    z = philox_ref.normal(noise.seed, B * C * HW // per, per, noise.sample_offset, draw).astype(np.float32)
    return torch.from_numpy(z).view(B, C, HW)


def ddim_ref(x, eps, wm, B, C, HW, cfg, g, coef, vpred, mask=None, sigma=0.0, z=None):
    '''fd_composite_ddim_step_f32: returns (x', e).  x: (B, C, HW); z: the normals, (B, C, HW), read when sigma != 0.'''
    e = composite_e(eps, wm, B, C, HW, cfg, g)
    c1, c2, c3, c4 = (f32(c) for c in coef)
    if vpred:
        x0, en = c2 * x - c1 * e, c2 * e + c1 * x
    else:
        x0, en = (x - c1 * e) / c2, e
    xn = c3 * x0 + c4 * en
    if sigma:
        xn = xn + f32(sigma) * z
    if mask is not None:
        xn = lin_ref.blend(xn, mask)
    return xn, e


def multistep_ref(x, eps, wm, m1, B, C, HW, cfg, g, coef, mask=None, sn=0.0, z=None):
    '''fd_composite_multistep_step_f32: returns (x', m0).  dpm_ref.kernel_ref on the composited rows, the noise between the
    update and the blend.'''
    e = composite_e(eps, wm, B, C, HW, cfg, g)
    xn, m0 = dpm_ref.kernel_ref(x, rows(e), m1, B, C, HW, False, 1.0, coef)
    if sn:
        xn = xn + f32(sn) * z
    if mask is not None:
        xn = lin_ref.blend(xn, mask)
    return xn, m0


def linear_ref(x, eps, wm, form, hist, B, C, HW, cfg, g, weights, coef, mask=None, x_src=None, scale=None):
    '''fd_composite_linear_multistep_step_f32: lin_ref.kernel_ref's dict on the composited rows.'''
    e = composite_e(eps, wm, B, C, HW, cfg, g)
    return lin_ref.kernel_ref(x, rows(e), form, hist, B, C, HW, False, 1.0, weights, coef, mask, x_src, scale)


def cpu_ops(monkeypatch):
    '''ops.axpby and every wrapper the four schedulers' fused steps may call replaced by restatements that carry the wrappers'
    own parameter lists, so the schedulers run without a GPU.  Returns the list of (wrapper name, entity maps or None) of every
    fused call.'''
    from flexdiffuse_amd import ops
    calls = []

    def guided_rows(name, eps_nhwc, wm, B, C, HW, cfg, guidance, composite):
        calls.append((name, wm))
        if not composite:
            return rows(lin_ref.cfg_mix(eps_nhwc, B, C, HW, cfg, guidance))
        return rows(composite_e(eps_nhwc, None if wm is None or wm.shape[0] == 0 else wm, B, C, HW, cfg, guidance))

    def fake_axpby(x, y, a, b, exp_half_x=False):
        assert not exp_half_x
        return lin_ref.axpby(x.contiguous(), y, a, b)

    def linear(name, e_rows, x, form, hist, h_out, B, C, HW, weights, coef, mask, x_keep_out, x_src, x_scaled_out, scale):
        v = lambda t: t.view(B, C, HW)                                   # noqa: E731
        r = lin_ref.kernel_ref(v(x).clone(), e_rows, form, [v(t) for t in hist], B, C, HW, False, 1.0, weights, coef, mask,
                               None if x_src is None else v(x_src), scale if x_scaled_out is not None else None)
        if h_out is not None:
            h_out.copy_(r['h'].reshape(h_out.shape))
        if x_keep_out is not None:
            x_keep_out.copy_(r['keep'].reshape(x_keep_out.shape))
        x.copy_(r['x'].view_as(x))
        if x_scaled_out is not None:
            x_scaled_out.copy_(r['scaled'].view_as(x_scaled_out))

    def cfg_linear(x, eps_nhwc, form, hist, h_out, B, C, HW, cfg, guidance, weights, coef, mask=None, x_keep_out=None,
                   x_src=None, x_scaled_out=None, scale=0.0):
        e_rows = guided_rows('cfg_linear_multistep_step', eps_nhwc, None, B, C, HW, cfg, guidance, False)
        linear('cfg', e_rows, x, form, list(hist), h_out, B, C, HW, weights, coef, mask, x_keep_out, x_src, x_scaled_out, scale)

    def composite_linear(x, eps_nhwc, weights_map, form, hist, h_out, B, C, HW, cfg, guidance, weights, coef, mask=None,
                         x_keep_out=None, x_src=None, x_scaled_out=None, scale=0.0):
        e_rows = guided_rows('composite_linear_multistep_step', eps_nhwc, weights_map, B, C, HW, cfg, guidance, True)
        linear('composite', e_rows, x, form, list(hist), h_out, B, C, HW, weights, coef, mask, x_keep_out, x_src, x_scaled_out,
               scale)

    def multistep(e_rows, x, m0_out, m1, B, C, HW, coef, mask, sn, noise, per, draw):
        v = lambda t: t.view(B, C, HW)                                   # noqa: E731
        xn, m0 = dpm_ref.kernel_ref(v(x).clone(), e_rows, None if m1 is None else v(m1), B, C, HW, False, 1.0, coef[:5])
        if sn:
            xn = xn + f32(sn) * normals(noise, B, C, HW, per, draw)
        if mask is not None:
            xn = lin_ref.blend(xn, mask)
        m0_out.copy_(m0.reshape(m0_out.shape))
        x.copy_(xn.view_as(x))

    def cfg_multistep(x, eps_nhwc, m0_out, m1, B, C, HW, cfg, guidance, coef, mask=None):
        multistep(guided_rows('cfg_multistep_step', eps_nhwc, None, B, C, HW, cfg, guidance, False), x, m0_out, m1, B, C, HW,
                  coef, mask, 0.0, None, 0, 0)

    def cfg_multistep_noise(x, eps_nhwc, m0_out, m1, B, C, HW, cfg, guidance, coef, sn, noise, per, draw, mask=None):
        multistep(guided_rows('cfg_multistep_noise_step', eps_nhwc, None, B, C, HW, cfg, guidance, False), x, m0_out, m1, B, C,
                  HW, coef, mask, sn, noise, per, draw)

    def composite_multistep(x, eps_nhwc, weights, m0_out, m1, B, C, HW, cfg, guidance, coef, mask=None, sn=0.0, noise=None,
                            per=0, draw=0):
        multistep(guided_rows('composite_multistep_step', eps_nhwc, weights, B, C, HW, cfg, guidance, True), x, m0_out, m1, B,
                  C, HW, coef, mask, sn, noise, per or C * HW, draw)

    monkeypatch.setattr(ops, 'axpby', fake_axpby)
    monkeypatch.setattr(ops, 'cfg_linear_multistep_step', cfg_linear)
    monkeypatch.setattr(ops, 'composite_linear_multistep_step', composite_linear)
    monkeypatch.setattr(ops, 'cfg_multistep_step', cfg_multistep)
    monkeypatch.setattr(ops, 'cfg_multistep_noise_step', cfg_multistep_noise)
    monkeypatch.setattr(ops, 'composite_multistep_step', composite_multistep)
    return calls
