'''Batched, soft-masked CompositeGuide on the device loop: the fd_composite_step_f32 kernel (blend + CFG + DDIM update
in one launch) against fp32 torch and against the per-entity chain it replaces, and the whole pipeline (mini and
full-size SD1.5 synthetic weights) against the CPU oracle, a batch-1 run per row, and across its launch modes.'''
import numpy as np
import pytest
import torch

from test_composite_masks import composite_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def mini(dev):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('mini', seed=0)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    pipe, clip, tok = build.build_models(sds, 'mini', dev)
    return sds, pipe, clip, tok, build.configs('mini')


@pytest.fixture(scope='module')
def sd15(dev):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False)
    return sds, pipe, clip, tok, build.configs('sd15')


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def soft_mask(w, h, seed):
    m = np.random.default_rng(seed).random((h, w)).astype(np.float32)
    m[m < 0.3] = 0.0
    return m


# ---- kernel ----------------------------------------------------------------------------------------------------------
def kernel_ref(x, eps, wm, B, C, HW, cfg, g, coef, vpred, do_step):
    '''fp32 torch on the CPU, in the kernel's operation order (separately rounded products and sums).'''
    n = 0 if wm is None else wm.shape[0]
    E = (1 if cfg else 0) + 1 + n
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)        # (E, B, C, HW)
    first = 1 if cfg else 0
    v = ev[first].clone()
    for k in range(n):
        w = wm[k].reshape(1, 1, HW)
        v = torch.where(w != 0, v + w * (ev[first + 1 + k] - v), v)
    if cfg:
        v = ev[0] + torch.tensor(g, dtype=torch.float32) * (v - ev[0])
    if not do_step:
        return None, v
    c1, c2, c3, c4 = (torch.tensor(c, dtype=torch.float32) for c in coef)
    if vpred:
        x0, en = c2 * x - c1 * v, c2 * v + c1 * x
    else:
        x0, en = (x - c1 * v) / c2, v
    return c3 * x0 + c4 * en, v


def test_composite_step_kernel_vs_torch(dev):
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(0)
    C, H, W = 4, 6, 10
    HW = H * W
    coef = (0.6, 0.8, 0.9, 0.43589)
    for B in (1, 3):
        for n in (0, 1, 3):
            wm = None
            if n:
                wm = torch.rand((n, HW), generator=rng)
                wm[wm < 0.35] = 0.0                                  # partly zero, overlapping
                wm[:, :7] = 0.0                                      # cells outside every box
            for ld in (4, 8, 5):                                     # 5: the scalar-load kernel
                for cfg in (False, True):
                    E = (1 if cfg else 0) + 1 + n
                    eps = torch.randn((E * B * HW, ld), generator=rng)
                    x = torch.randn((B, C, H, W), generator=rng)
                    for do_step in (False, True):
                        for vpred in (False, True):
                            if vpred and not do_step:
                                continue
                            xd = x.clone().to(dev)
                            out = torch.full((B, C, H, W), float('nan'), device=dev)
                            ops.composite_step(xd if do_step else None, eps.to(dev), None if wm is None else wm.to(dev),
                                               B, C, HW, cfg, 7.5, coef, vpred, do_step=do_step, eps_out=out)
                            wx, wv = kernel_ref(x.reshape(B, C, HW), eps, wm, B, C, HW, cfg, 7.5, coef, vpred, do_step)
                            case = (B, n, ld, cfg, do_step, vpred)
                            assert torch.equal(out.cpu().reshape(B, C, HW), wv), case
                            if do_step:
                                assert torch.equal(xd.cpu().reshape(B, C, HW), wx), case
                            else:
                                assert torch.equal(xd.cpu(), x), case


class _StubEncoder():
    def __init__(self, dev):
        self.dev = dev

    def prompt(self, p):
        g = torch.Generator().manual_seed(sum(map(ord, p)) + 7 * len(p))
        return torch.randn((1, 5, 16), generator=g).to(self.dev)


class _FixedUNet():
    def __init__(self, eps):
        self.eps = eps

    def forward_nhwc(self, latents, step, ctx, rep=1):
        assert ctx.shape[0] == rep * latents.shape[0]
        return self.eps


@pytest.mark.parametrize('guidance', [8.0, 1.0])
def test_composite_step_bitwise_equals_region_blend_chain(dev, guidance):
    '''Rectangles: one fd_composite_step_f32(do_step=0) == nhwc_to_nchw + fd_region_blend_f32 per entity +
    fd_cfg_ddim_step_f32(do_step=0) (CompositeGuide's batch-1 path), bit for bit; once more through a launch plan.'''
    from flexdiffuse_amd import hip, ops
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    C, H, W = 4, 12, 14
    ents = [EntitySchema('a deer', (8, 16), (64, 48), 0.8), EntitySchema('a bird', (80, 40), (64, 64), 0.5),
            EntitySchema('a cat', (-24, 8), (40, 32), 0.6), EntitySchema('a dog', (16, 16), (48, 40), 0.3)]
    schema = Schema('forest', '', '', (0.0, 1.0), ents)
    E = (2 if guidance > 1 else 1) + len(ents)
    eps = torch.randn((E * H * W, C), generator=torch.Generator().manual_seed(3)).to(dev)
    guide = CompositeGuide(_StubEncoder(dev), _FixedUNet(eps), guidance, schema, 10)
    assert not guide.on_device
    want = guide.noise_pred(torch.zeros((1, C, H, W), device=dev), 500)
    got = torch.empty((1, C, H, W), device=dev)
    guide.step(None, eps, eps_out=got)
    assert torch.equal(got, want)
    plan = hip.Plan()
    again = torch.full_like(got, float('nan'))
    with plan.record():
        ops.composite_step(None, eps, guide.weights(H, W), 1, C, H * W, guidance > 1, guidance, do_step=False,
                           eps_out=again)
    assert len(plan) == 1 and torch.equal(again, want)
    again.fill_(float('nan'))
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(again, want)


# ---- mini pipeline ---------------------------------------------------------------------------------------------------
def _mini_schema(masked=True, mask_seed=1):
    from flexdiffuse_amd.composition import EntitySchema, Schema
    return Schema('a forest at dawn', '', '', (0.0, 1.0),
                  [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft_mask(64, 48, mask_seed) if masked else None),
                   EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])          # clipped by the 128x128 canvas


def test_mini_batched_masked_composite_vs_oracle(mini, dev):
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, ddim_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    schema, steps, B = _mini_schema(), 3, 3
    lat0 = torch.randn((B, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(21))
    pipe(guide=CompositeGuide(enc, pipe.unet, 8.0, schema, steps, batch_size=B), init_size=(128, 128), latents=lat0,
         output_type='np')
    got = pipe.last_latents.clone()
    th = lambda p: clip_ref.text_hidden(sds['clip'], ccfg, tok(p).input_ids)   # noqa: E731
    ents = [(th(e.prompt), tuple(v // 8 for v in e.offset), tuple(v // 8 for v in e.size), e.blend, e.mask)
            for e in schema.entities]
    x = lat0.clone()
    acp = ddim_ref.alphas_cumprod()
    for t in ddim_ref.timesteps(steps):
        fn = lambda lat, emb: unet_ref.unet_forward(sds['unet'], ucfg, lat, int(t), emb)   # noqa: E731
        eps = composite_ref(fn, x, th(''), th(schema.background_prompt), ents, 8.0)
        x = ddim_ref.ddim_step(eps, int(t), x, acp, steps)
    e = relerr(got, x)
    print(f'batched masked composite (B={B}): latent rel err {e:.4f}')
    assert e < 2e-2, e
    for b in range(B):
        pipe(guide=CompositeGuide(enc, pipe.unet, 8.0, schema, steps), init_size=(128, 128), latents=lat0[b:b + 1],
             output_type='np')
        eb = relerr(got[b:b + 1], pipe.last_latents)
        assert eb < 1e-2, (b, eb)
    # an all-ones mask is the rectangle (batch-1 rectangles stay on the per-entity chain)
    ones = Schema('a forest at dawn', '', '', (0.0, 1.0),
                  [EntitySchema('a deer', (8, 16), (64, 48), 0.8, np.ones((48, 64), np.float32))])
    rect = Schema('a forest at dawn', '', '', (0.0, 1.0), [EntitySchema('a deer', (8, 16), (64, 48), 0.8)])
    g1 = CompositeGuide(enc, pipe.unet, 8.0, ones, steps)
    g2 = CompositeGuide(enc, pipe.unet, 8.0, rect, steps)
    assert g1.on_device and not g2.on_device
    pipe(guide=g1, init_size=(128, 128), latents=lat0[:1], output_type='np')
    a = pipe.last_latents.clone()
    pipe(guide=g2, init_size=(128, 128), latents=lat0[:1], output_type='np')
    assert relerr(a, pipe.last_latents) < 1e-2


def test_mini_composite_graph_plan_eager_bit_equal(mini, dev):
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    schema = _mini_schema(mask_seed=2)
    keep = pipe.scheduler

    def run(debug=False):
        g = CompositeGuide(enc, pipe.unet, 7.5, schema, 4, batch_size=2)
        pipe(guide=g, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(13), output_type='np',
             debug=debug)
        return pipe.last_latents.clone()
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run()
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run()
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(debug=True)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
        assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
        # PNDM: the planned branch (graph / plan UNet, kernel with do_step=0, scheduler.step) == the protocol path
        pipe.scheduler = PNDMScheduler()
        pipe.use_graph, pipe._graphs = True, {}
        planned = run()
        pipe.scheduler = PNDMScheduler()
        pipe.use_graph, pipe.use_plan = False, False
        protocol = run()
        assert torch.equal(planned, protocol) and bool(torch.isfinite(planned).all())
    finally:
        pipe.scheduler, pipe.use_plan, pipe.use_graph = keep, True, True


def test_mini_composite_img2img_batched(mini, dev):
    from PIL import Image
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    # a PIL image is resized to a long side of 512 (encode/clip.py:24-33) and the mini VAE scales by 2:
    # a 512x64 image keeps the encoder's attention small (256x32 latents)
    img = Image.fromarray(np.random.default_rng(4).integers(0, 256, (64, 512, 3), dtype=np.uint8))

    def run():
        g = CompositeGuide(enc, pipe.unet, 8.0, _mini_schema(), 5, batch_size=2)
        out = pipe(guide=g, init_image=img, strength=0.6, generator=torch.Generator('cpu').manual_seed(5),
                   output_type='np')
        return out.images, pipe.last_latents.clone()
    a, la = run()
    b, lb = run()
    assert a.shape == (2, 64, 512, 3) and la.shape == (2, 4, 32, 256)
    assert bool(torch.isfinite(la).all()) and np.isfinite(a).all()
    assert torch.equal(la, lb) and np.array_equal(a, b)


def test_runner_compose_batched_masks(dev):
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.composition import CompositeGuide
    r = Runner(preset='mini', device='cuda')
    rows = [['a deer', 8, 16, 64, 48, 0.8], ['', 0, 0, 8, 8, 0.5], ['bad', 'x', 0, 8, 8, 0.5],
            ['a red bird', 64, 0, 64, 64, 0.5]]
    masks = [soft_mask(64, 48, 3), np.ones((8, 8)), None, None]
    kw = dict(init_size=(128, 128), steps=3, batches=2, seed=9, batch_size=2, masks=masks)
    imgs, grid = r.compose('a forest at dawn', rows, **kw)
    assert len(imgs) == 4 and [e.prompt for e in r.last_schema.entities] == ['a deer', 'a red bird']
    assert r.last_schema.entities[0].mask is not None and r.last_schema.entities[1].mask is None
    again, _ = r.compose('a forest at dawn', rows, **kw)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(imgs, again))
    assert not np.array_equal(np.asarray(imgs[0]), np.asarray(imgs[2]))     # the generator advances
    guide = CompositeGuide(r.encoder, r.pipe.unet, 8.0, r.last_schema, 3, batch_size=2)
    out = r.pipe(guide=guide, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(9))
    assert all(np.array_equal(np.asarray(out['sample'][i]), np.asarray(imgs[i])) for i in range(2))


# ---- full size -------------------------------------------------------------------------------------------------------
def test_sd15_batched_masked_composite_full_size(sd15, dev):
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = sd15
    enc = CLIPEncoder(clip, tok)
    schema = Schema('a forest at dawn, oil painting', '', '', (0.0, 1.0),
                    [EntitySchema('a deer', (64, 128), (256, 192), 0.8, soft_mask(256, 192, 7)),
                     EntitySchema('a red bird', (320, 0), (256, 256), 0.5)])
    B, steps = 4, 3
    lat0 = torch.randn((B, 4, 64, 64), generator=torch.Generator('cpu').manual_seed(17))

    def run(lat, bs):
        pipe(guide=CompositeGuide(enc, pipe.unet, 8.0, schema, steps, batch_size=bs), init_size=(512, 512), latents=lat,
             output_type='np')
        return pipe.last_latents.clone()
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(lat0, B)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(lat0, B)
        pipe.use_graph, pipe.use_plan = True, True
        assert pipe.graph_fallback is None
        assert bool(torch.isfinite(graph).all()) and torch.equal(graph, plan)
        for b in range(B):
            e = relerr(graph[b:b + 1], run(lat0[b:b + 1], 1))
            print(f'sd15 batched composite row {b}: rel err vs batch 1 {e:.4f}')
            assert e < 2e-2, (b, e)
    finally:
        pipe.use_plan, pipe.use_graph = True, True
