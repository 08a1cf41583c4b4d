'''Masked img2img (inpainting), host side, without a GPU: the latent mask, the per-step noise
levels of the known region, the public signatures, the C-ABI argument checks, and the CPU
restatement of the masked loop that tests/test_gpu_inpaint.py compares the device against.

The restatement (`masked_denoise_ref`) is `oracle.pipeline_ref.denoise` with a callback that
replaces each step's new latents in place:  known = k1 z0 + k2 n;  x = x' where m == 1, known
where m == 0, known + m (x' - known) otherwise; (k1, k2) = (sqrt(a_prev), sqrt(1 - a_prev)) of the
step's output level, (1, 0) after the last step.
'''
import inspect

import numpy as np
import pytest
import torch

from oracle import ddim_ref, pipeline_ref


# ---- the CPU restatement -------------------------------------------------------------------------
def ref_coefficients(steps, t_start):
    '''[(k1, k2)] fp32 tensors per step of ddim_ref.timesteps(steps)[t_start:], from the oracle's tables.'''
    acp = ddim_ref.alphas_cumprod()
    ts = [int(t) for t in ddim_ref.timesteps(steps)[t_start:]]
    pairs = []
    for t in ts:
        prev = t - 1000 // steps
        a_p = acp[prev] if prev >= 0 else acp[0]
        pairs.append((a_p.sqrt(), (1 - a_p).sqrt()))
    pairs[-1] = (torch.tensor(1.0), torch.tensor(0.0))
    return ts, pairs


def blend_ref(x, z0, n, m, k1, k2):
    '''fp32 torch in the kernel's operation order; m broadcasts over batch and channels.'''
    known = k1 * z0 + k2 * n
    return torch.where(m == 1, x, torch.where(m == 0, known, known + m * (x - known)))


def step_ref(x, eps, B, C, HW, cfg, g, coef, vpred):
    '''fd_cfg_ddim_step_f32 in fp32 torch on the CPU, in the kernel's operation order.  x: (B, C, HW).'''
    E = 2 if cfg else 1
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)
    v = ev[0] + torch.tensor(g, dtype=torch.float32) * (ev[1] - ev[0]) if cfg else ev[0]
    c1, c2, c3, c4 = (torch.tensor(c, dtype=torch.float32) for c in coef)
    if vpred:
        x0, en = c2 * x - c1 * v, c2 * v + c1 * x
    else:
        x0, en = (x - c1 * v) / c2, v
    return c3 * x0 + c4 * en


def masked_denoise_ref(sd_unet, ucfg, emb, unc, z0, noise, m, steps, guidance, t_start, t_noise):
    '''z0: clean init latents (B,4,h,w); noise: the call's add_noise tensor; m: fp32 [h][w].'''
    ts, pairs = ref_coefficients(steps, t_start)
    lat0 = ddim_ref.add_noise(z0, noise, t_noise, ddim_ref.alphas_cumprod())
    seen = []

    def callback(t, x):
        i = len(seen)
        assert ts[i] == t
        seen.append(t)
        x.copy_(blend_ref(x, z0, noise, m, *pairs[i]))
    return pipeline_ref.denoise(sd_unet, ucfg, emb, unc, lat0, steps, guidance, t_start=t_start, callback=callback)


# ---- 1. latent_mask ------------------------------------------------------------------------------
def test_latent_mask_block_means():
    from flexdiffuse_amd.pipeline.inpaint import latent_mask
    for factor in (8, 2):
        H, W = 4 * factor, 6 * factor
        m = np.zeros((H, W), dtype=np.float32)
        m[:factor, :factor] = 1.0                              # one whole block
        m[factor:2 * factor, :factor // 2] = 1.0               # the left half of a block
        m[2 * factor, 2 * factor] = 1.0                        # one pixel of a block
        got = latent_mask(m, H, W, factor)
        assert got.dtype == torch.float32 and tuple(got.shape) == (4, 6) and got.is_contiguous()
        want = torch.zeros((4, 6))
        want[0, 0], want[1, 0], want[2, 2] = 1.0, 0.5, 1.0 / factor ** 2
        assert torch.equal(got, want), factor
        assert torch.equal(latent_mask(np.ones((H, W)), H, W, factor), torch.ones((4, 6)))
        assert torch.equal(latent_mask(torch.zeros((H, W)), H, W, factor), torch.zeros((4, 6)))
        assert torch.equal(latent_mask(m.tolist(), H, W, factor), want)        # nested lists too


def test_latent_mask_non_square():
    from flexdiffuse_amd.pipeline.inpaint import latent_mask
    H, W = 320, 512                                            # (height, width): 40 x 64 latents at factor 8
    m = np.zeros((H, W), dtype=np.float32)
    m[:, 256:] = 1.0
    m[:, 252:256] = 1.0                                        # half of block column 31
    got = latent_mask(m, H, W, 8)
    assert tuple(got.shape) == (40, 64)
    assert bool((got[:, :31] == 0).all()) and bool((got[:, 31] == 0.5).all()) and bool((got[:, 32:] == 1).all())
    rows = np.zeros((H, W), dtype=np.float32)
    rows[:8] = 1.0                                             # the top latent row only
    got = latent_mask(rows, H, W, 8)
    assert bool((got[0] == 1).all()) and bool((got[1:] == 0).all())


def test_latent_mask_value_errors():
    from flexdiffuse_amd.pipeline.inpaint import latent_mask
    with pytest.raises(ValueError, match='shape'):
        latent_mask(np.ones((16, 24)), 24, 16, 8)              # transposed
    with pytest.raises(ValueError, match='shape'):
        latent_mask(np.ones((2, 16, 16)), 16, 16, 8)
    bad = np.ones((16, 16), dtype=np.float32)
    bad[3, 3] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        latent_mask(bad, 16, 16, 8)
    for v in (-0.01, 1.5):
        bad[3, 3] = v
        with pytest.raises(ValueError, match=r'\[0, 1\]'):
            latent_mask(bad, 16, 16, 8)
    with pytest.raises(ValueError, match='divide'):
        latent_mask(np.ones((20, 16)), 20, 16, 8)


def test_latent_mask_pil():
    from PIL import Image
    from flexdiffuse_amd.encode.clip import sd_size
    from flexdiffuse_amd.pipeline.inpaint import image_size, latent_mask
    rng = np.random.default_rng(3)
    arr = rng.integers(0, 256, (64, 96), dtype=np.uint8)
    arr[:8] = 255
    arr[8:16] = 0
    # at the target size already: read as convert('L') / 255, the array path's values
    got = latent_mask(Image.fromarray(arr), 64, 96, 8)
    want = latent_mask(arr.astype(np.float32) / np.float32(255), 64, 96, 8)
    assert torch.equal(got, want) and bool((got[0] == 1).all()) and bool((got[1] == 0).all())
    rgb = Image.fromarray(np.stack([arr] * 3, axis=-1))
    assert torch.equal(latent_mask(rgb.convert('L'), 64, 96, 8), want)
    # a PIL init image goes through preprocess -> sd_size; its PIL mask is resized to that size
    init = Image.new('RGB', (1024, 640))
    assert image_size(init) == (320, 512) == sd_size(1024, 640)[::-1]
    assert image_size(torch.zeros((1, 3, 96, 64))) == (96, 64)
    half = np.zeros((640, 1024), dtype=np.uint8)
    half[:, 512:] = 255
    got = latent_mask(Image.fromarray(half), *image_size(init), 8)
    assert tuple(got.shape) == (40, 64)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0                  # Lanczos overshoot is clipped
    assert bool((got[:, :30] == 0).all()) and bool((got[:, 34:] == 1).all())


# ---- 2. known_coefficients -----------------------------------------------------------------------
def test_known_coefficients_ddim_vs_oracle():
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from flexdiffuse_amd.scheduler import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(10)
    t_start = 4                                                # 10 steps at strength 0.6
    assert [int(t) for t in s.timesteps[t_start:]] == [int(t) for t in ddim_ref.timesteps(10)[t_start:]]
    pairs = known_coefficients(s, s.timesteps, t_start)
    # the oracle's table through numpy's fp32 sqrt, which is correctly rounded on every machine (torch's CPU sqrt is not:
    # it may be 1 ulp off, differently from one CPU to the next)
    acp = ddim_ref.alphas_cumprod().numpy()
    assert len(pairs) == 6 and all(isinstance(v, float) for p in pairs for v in p)
    for (k1, k2), prev in zip(pairs[:5], (400, 300, 200, 100, 0)):
        assert k1 == float(np.sqrt(acp[prev])) and k2 == float(np.sqrt(np.float32(1) - acp[prev])), prev
    assert pairs[5] == (1.0, 0.0)
    # the restatement's own (torch) pairs: the same up to that ulp of sqrt -- 2^-22 relative leaves room for two
    ts, ref = ref_coefficients(10, t_start)
    assert ts == [500, 400, 300, 200, 100, 0] and len(ref) == 6
    for (a, b), (k1, k2) in zip(ref, pairs):
        assert abs(float(a) - k1) <= 2.0 ** -22 * k1 and abs(float(b) - k2) <= 2.0 ** -22 * k2
    assert (float(ref[5][0]), float(ref[5][1])) == (1.0, 0.0)
    # the whole schedule: ten pairs, the first nine on prev = 800 ... 0
    full = known_coefficients(s, s.timesteps, 0)
    assert len(full) == 10 and full[0][0] == float(np.sqrt(acp[800])) and full[-1] == (1.0, 0.0)
    assert known_coefficients(s, s.timesteps, 10) == []


def test_known_coefficients_lms_and_pndm():
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    s = LMSDiscreteScheduler()
    s.set_timesteps(10)
    pairs = known_coefficients(s, s.timesteps, 4)
    assert len(pairs) == 6
    for i, (k1, k2) in enumerate(pairs[:5]):
        assert k1 == 1.0 and k2 == float(np.float32(s.sigmas[4 + i + 1]))
    assert pairs[5] == (1.0, 0.0) and float(s.sigmas[10]) == 0.0
    # PNDM: what `step` hands to prev_coefficients -- index + 1 - offset, the second call landing on its own timestep
    p = PNDMScheduler()
    p.set_timesteps(10)
    assert [int(t) for t in p.timesteps] == [900, 800, 800, 700, 600, 500, 400, 300, 200, 100, 0]
    full = known_coefficients(p, p.timesteps, 0)
    a = p.alphas_cumprod
    assert len(full) == 11 and full[0] == full[1] == (float(np.sqrt(a[801])), float(np.sqrt(np.float32(1) - a[801])))
    assert full[2] == (float(np.sqrt(a[701])), float(np.sqrt(np.float32(1) - a[701]))) and full[-1] == (1.0, 0.0)
    sliced = known_coefficients(p, p.timesteps, 5)              # [500, 400, 300, 200, 100, 0]: counter restarts at 0
    assert sliced[0] == (float(np.sqrt(a[401])), float(np.sqrt(np.float32(1) - a[401]))) == sliced[1]
    assert sliced[2] == (float(np.sqrt(a[201])), float(np.sqrt(np.float32(1) - a[201])))
    with pytest.raises(TypeError):
        known_coefficients(object(), [1, 2], 0)


def img2img_request(sched, steps, strength):
    '''(t_noise, t_start) of an img2img request as FlexPipeline.__call__ derives them (pipeline/flex.py: the add_noise
    timestep -- for K-LMS an index -- and the first step of the sliced timestep list); sets the scheduler's timesteps.'''
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler
    sched.set_timesteps(steps)
    offset = sched.config.get('steps_offset', 0)
    init_timestep = min(int(steps * strength) + offset, steps)
    t_noise = steps - init_timestep if isinstance(sched, LMSDiscreteScheduler) else int(sched.timesteps[-init_timestep])
    return t_noise, max(steps - init_timestep + offset, 0)


def _trajectory(monkeypatch, sched, steps, strength):
    '''The pipeline's img2img bookkeeping (pipeline/flex.py) around the REAL scheduler.step, on the CPU (fd_axpby_f32
    restated in torch), with a noise prediction that returns the call's own n: returns (z0, n, init, [x_i], known).'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler
    monkeypatch.setattr(ops, 'axpby', lambda x, y, a, b, exp_half_x=False: (
        torch.tensor(a, dtype=torch.float32) * x + torch.tensor(b, dtype=torch.float32) * (y if y is not None else 0)))
    g = torch.Generator().manual_seed(9)
    z0, n = torch.randn((1, 4, 6, 6), generator=g) * 0.7, torch.randn((1, 4, 6, 6), generator=g)
    lms = isinstance(sched, LMSDiscreteScheduler)
    t_noise, t_start = img2img_request(sched, steps, strength)
    x = init = sched.add_noise(z0, n, t_noise)
    known = known_coefficients(sched, sched.timesteps, t_start, start_level(sched, t_noise))
    xs = []
    for i, t in enumerate(sched.timesteps[t_start:]):
        x = sched.step(n, t_start + i if lms else t, x).prev_sample
        xs.append(x)
    assert len(known) == len(xs)
    return z0, n, init, xs, known


def _levels_check(name, z0, n, init, xs, known):
    '''Step i's latents sit on known_i and not on a neighbouring step's level (the factor 10 is a margin: neighbouring
    levels of a 10-step schedule differ by percent of |z0|, rounding by parts in 10^6).'''
    lvl = lambda k: torch.tensor(k[0]) * z0 + torch.tensor(k[1]) * n           # noqa: E731
    for i in range(len(xs) - 1):
        d = lambda ref: float((xs[i] - ref).abs().max())                       # noqa: E731
        wrong = [d(lvl(known[j])) for j in (i - 1, i + 1) if j >= 0 and known[j] != known[i]]
        if i == 0:
            wrong.append(d(init))
        d_right, d_wrong = d(lvl(known[i])), min(wrong)
        print(f'{name} step {i}: d_right {d_right:.3g} d_wrong {d_wrong:.3g}')
        assert d_right < 0.1 * d_wrong, (name, i, d_right, d_wrong)


@pytest.mark.parametrize('offset', [0, 1])
def test_known_levels_follow_the_real_pndm_steps(monkeypatch, offset):
    '''A sliced PNDM request starts off its own table (see `known_coefficients`); with `start` the levels are the ones
    the real `step` calls put a sample on.'''
    from flexdiffuse_amd.scheduler import PNDMScheduler
    for strength in (0.6, 1.0):
        _levels_check(f'pndm offset {offset} strength {strength}',
                      *_trajectory(monkeypatch, PNDMScheduler(steps_offset=offset), 10, strength))


def test_known_levels_follow_the_real_lms_steps(monkeypatch):
    '''K-LMS at strength 1 (the whole sigma table; a sliced request runs its first steps as order-4 formulas over fewer
    derivatives, as the reference's scheduler does, and leaves the table).'''
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler
    _levels_check('lms', *_trajectory(monkeypatch, LMSDiscreteScheduler(), 10, 1.0))


def test_pndm_start_on_the_table_gives_the_table():
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from flexdiffuse_amd.scheduler import PNDMScheduler
    p = PNDMScheduler()
    p.set_timesteps(10)
    a = np.float32(p.alphas_cumprod[901])                      # the level the first step of the whole list assumes
    table = known_coefficients(p, p.timesteps, 0)
    carried = known_coefficients(p, p.timesteps, 0, (float(np.sqrt(a)), float(np.sqrt(np.float32(1) - a))))
    assert len(table) == len(carried) == 11 and carried[-1] == (1.0, 0.0)
    for (a1, a2), (b1, b2) in zip(table, carried):
        assert abs(a1 - b1) < 1e-5 and abs(a2 - b2) < 1e-5


# ---- 3. signatures -------------------------------------------------------------------------------
def _params(fn):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values()]


def test_mask_image_keyword_is_additive():
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    P = inspect.Parameter
    call = _params(FlexPipeline.__call__)
    assert call[-1] == ('mask_image', P.POSITIONAL_OR_KEYWORD, None)
    assert [(n, d) for n, _, d in call[:-1]] == [
        ('self', P.empty), ('guide', P.empty), ('init_image', None), ('init_size', (512, 512)), ('strength', 0.6),
        ('eta', 0.0), ('generator', None), ('output_type', 'pil'), ('return_dict', True), ('debug', False),
        ('latents', None), ('noise', None)]
    gen = _params(Runner.gen)
    assert gen[-1] == ('mask_image', P.KEYWORD_ONLY, None)
    assert [(n, d) for n, _, d in gen[:-1]] == [
        ('self', P.empty), ('prompt', ''), ('init_image', None), ('guide', None), ('init_size', (512, 512)),
        ('mapping_concepts', ''), ('guide_threshold_mult', 0.5), ('guide_threshold_floor', 0.5), ('guide_clustered', 0.5),
        ('guide_linear', (0.0, 0.5)), ('guide_max_guidance', 0.5), ('guide_header_max', 0.15), ('guide_mode', 0),
        ('guide_reuse', True), ('strength', 0.6), ('steps', 10), ('guidance_scale', 8), ('samples', 1), ('seed', None),
        ('debug', False)]
    assert all(k == P.POSITIONAL_OR_KEYWORD for _, k, _ in gen[:-1])
    comp = _params(Runner.compose)
    assert comp[-1] == ('mask_image', P.KEYWORD_ONLY, None)
    assert [(n, d) for n, _, d in comp[:-1]] == [
        ('self', P.empty), ('bg_prompt', ''), ('entities_df', ()), ('start_style', ''), ('end_style', ''),
        ('style_blend', (0.0, 1.0)), ('init_image', None), ('batches', 4), ('strength', 0.7), ('steps', 30),
        ('guidance_scale', 8.0), ('init_size', (512, 512)), ('seed', None), ('debug', False), ('batch_size', 1),
        ('masks', None)]
    assert [k for _, k, _ in comp[-3:]] == [P.KEYWORD_ONLY] * 3


# ---- 4. the restatement itself -------------------------------------------------------------------
def test_oracle_restatement_limits():
    '''All-ones mask: the plain oracle loop's bits; all-zeros: the clean init latents' bits; a fractional cell moves.'''
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('mini', seed=0)
    ucfg = build.configs('mini')[0]
    g = torch.Generator().manual_seed(3)
    B, steps, t_start, guidance = 2, 10, 4, 8.0
    z0 = torch.randn((B, 4, 8, 8), generator=g) * 0.5
    noise = torch.randn((B, 4, 8, 8), generator=g)
    emb = torch.randn((B, 77, ucfg.cross_attention_dim), generator=g)
    unc = torch.randn((1, 77, ucfg.cross_attention_dim), generator=g)
    t_noise = int(ddim_ref.timesteps(steps)[-6])
    assert t_noise == 500
    lat0 = ddim_ref.add_noise(z0, noise, t_noise, ddim_ref.alphas_cumprod())
    plain, used = pipeline_ref.denoise(sds['unet'], ucfg, emb, unc, lat0, steps, guidance, t_start=t_start)
    assert used == [500, 400, 300, 200, 100, 0]
    ones, used1 = masked_denoise_ref(sds['unet'], ucfg, emb, unc, z0, noise, torch.ones((8, 8)), steps, guidance,
                                     t_start, t_noise)
    assert used1 == used and torch.equal(ones, plain)
    zeros, _ = masked_denoise_ref(sds['unet'], ucfg, emb, unc, z0, noise, torch.zeros((8, 8)), steps, guidance,
                                  t_start, t_noise)
    assert torch.equal(zeros, z0)
    m = torch.zeros((8, 8))
    m[:, 5:] = 1.0
    m[:, 4] = 0.25
    mixed, _ = masked_denoise_ref(sds['unet'], ucfg, emb, unc, z0, noise, m, steps, guidance, t_start, t_noise)
    assert torch.equal(mixed[..., :4], z0[..., :4]) and not torch.equal(mixed[..., 5:], plain[..., 5:])
    assert not torch.equal(mixed[..., 4], z0[..., 4]) and bool(torch.isfinite(mixed).all())


# ---- 5. C ABI ------------------------------------------------------------------------------------
def test_masked_step_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    import ctypes
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    x, z0, n, m, eps = a, a + 64, a + 128, a + 192, a + 16
    tail = (0, 1.0, 0.0, 1.0, 1.0, 0.0, 0, 1.0, 0.0, None)      # cfg, guidance, c1..c4, v_prediction, k1, k2, stream
    for args in ((None, None, z0, n, m, 1, 4, 4, 0), (x, None, None, n, m, 1, 4, 4, 0), (x, None, z0, None, m, 1, 4, 4, 0),
                 (x, None, z0, n, None, 1, 4, 4, 0)):
        with pytest.raises(ValueError):
            hip.call('fd_cfg_ddim_masked_step_f32', *args, *tail)
        assert b'null' in hip.lib().fd_last_error()
    for args in ((x, None, z0, n, m, 0, 4, 4, 0), (x, None, z0, n, m, 1, 0, 4, 0), (x, None, z0, n, m, 1, 4, 0, 0),
                 (x, eps, z0, n, m, 1, 4, 4, 3)):                # fused form: ld < C
        with pytest.raises(ValueError):
            hip.call('fd_cfg_ddim_masked_step_f32', *args, *tail)
        assert b'sizes' in hip.lib().fd_last_error()
    for args in ((x, None, x, n, m, 1, 4, 4, 0), (x, None, z0, x, m, 1, 4, 4, 0)):
        with pytest.raises(ValueError):
            hip.call('fd_cfg_ddim_masked_step_f32', *args, *tail)
        assert b'alias' in hip.lib().fd_last_error()


def test_pipeline_rejects_mask_without_init_image():
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    from flexdiffuse_amd.scheduler import DDIMScheduler
    pipe = FlexPipeline(None, None, None, type('U', (), {'device': torch.device('cpu')})(), DDIMScheduler())
    with pytest.raises(ValueError, match='init_image'):
        pipe(guide=None, mask_image=np.ones((8, 8)))
