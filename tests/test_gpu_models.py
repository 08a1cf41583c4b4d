'''Parity of the device model containers and of the whole pipeline (through the C ABI) with
the CPU oracle on identical seeded synthetic weights / inputs.  Needs an MI355X.

Tolerances (fp16 storage + fp16 MFMA inputs vs fp32 oracle), stated per test:
  * CLIP towers: max abs err <= 2e-2 on O(1) LayerNorm-ed outputs
  * UNet / VAE single forward: max abs err <= 3% of the output's max magnitude
  * end-to-end: integer timestep lists equal; final-image PSNR >= 40 dB (north_star)
'''
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

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


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def test_clip_towers_vs_reference_goldens(dev):
    '''Device CLIP on the tiny seeded config against the goldens captured from the
    reference's encode/clip.py driving transformers.CLIPModel.'''
    from flexdiffuse_amd import weights as W
    from flexdiffuse_amd.clip import CLIPModel
    from flexdiffuse_amd.encode.clip import CLIPEncoder, clip_pixels, preprocess
    from flexdiffuse_amd.tokenizer import SyntheticTokenizer
    from test_oracle_clip import synth_image
    cg = np.load(os.path.join(GOLDEN, 'clip_goldens.npz'))
    sd = {k[3:]: torch.from_numpy(cg[k].astype(np.float32)) for k in cg.files if k.startswith('sd/')}
    clip = CLIPModel(sd, W.MINI_CLIP, dev)
    tok = SyntheticTokenizer(vocab_size=W.MINI_CLIP.text.vocab_size)
    enc = CLIPEncoder(clip, tok)
    for i, p in enumerate(cg['prompts']):
        got = enc.prompt(str(p)).cpu().numpy()
        assert got.shape == cg[f'prompt{i}/hidden'].shape
        assert np.max(np.abs(got - cg[f'prompt{i}/hidden'])) < 2e-2, i
    got = enc.prompt([str(p) for p in cg['prompts'][:2]]).cpu().numpy()
    assert np.max(np.abs(got - cg['prompt_batch/hidden'])) < 2e-2
    for i in (0, 1, 3):
        w, h = cg['image_sizes'][i]
        img = synth_image(20 + i, int(w), int(h))
        px = clip_pixels(preprocess(img))
        assert np.max(np.abs(px.numpy() - cg[f'image{i}/pixels'].astype(np.float32))) < 4e-3
        got = enc.image(img).cpu().numpy()
        assert got.shape == cg[f'image{i}/tokens'].shape
        err = np.max(np.abs(got - cg[f'image{i}/tokens']))
        assert err < 2e-2 * max(1.0, np.abs(cg[f'image{i}/tokens']).max()), (i, err)


def test_guide_embeds_vs_reference_goldens(dev):
    '''Guide.embeds control-flow branches on device vs goldens from the reference's Guide.
    The tween decisions depend on similarities computed from fp16-tower embeddings, so the
    comparison is made through the oracle fed with the DEVICE embeddings (bit-level blend
    parity is covered in test_gpu_guidance.py); against the goldens a loose bound holds.'''
    from flexdiffuse_amd import Guide, weights as W
    from flexdiffuse_amd.clip import CLIPModel
    from flexdiffuse_amd.tokenizer import SyntheticTokenizer
    from test_oracle_clip import synth_image
    cg = np.load(os.path.join(GOLDEN, 'clip_goldens.npz'))
    sd = {k[3:]: torch.from_numpy(cg[k].astype(np.float32)) for k in cg.files if k.startswith('sd/')}
    clip = CLIPModel(sd, W.MINI_CLIP, dev)
    tok = SyntheticTokenizer(vocab_size=W.MINI_CLIP.text.vocab_size)
    g = Guide(clip, tok, device='cuda')
    p = [str(x) for x in cg['prompts']]
    img = synth_image(20, 512, 512)
    for name, kw in {'text_only': dict(prompt=p[0]), 'text_batch': dict(prompt=p[:2]),
                     'pure_text_guide': dict(guide=p[1]), 'pure_image': dict(guide=img)}.items():
        got = g.embeds(**kw).float().cpu().numpy()
        want = cg['guide/' + name]
        assert got.shape == want.shape, name
        assert np.max(np.abs(got - want)) < 3e-2 * max(1.0, np.abs(want).max()), name
    # ---- the tween branches (guidance.py:409-449), value-checked: the DEVICE text / image
    # embeddings go through the CPU oracle's tween, which must reproduce g.embeds(...) --
    # bit-exact when the oracle is fed the device's own mapping (similarities differ in the
    # last fp32 bits between the MFMA and the numpy mat-vec), and with equal guide indices and
    # |delta| <= 1e-5 when the oracle maps by itself.  Against the reference's goldens (fp32
    # towers) the loose tower bound holds.
    import numpy as _np
    from oracle import guidance_ref as G
    C3 = dict(guide_threshold_floor=0.75, guide_threshold_mult=0.25, guide_clustered=0.25,
              guide_linear=(0.0, 0.0), guide_max_guidance=0.35, guide_header_max=0.0)
    cases = {
        'image_linear': (p[0], dict(guide_threshold_mult=0.0, guide_clustered=0.0,
                                    guide_linear=(0.0, 0.5), guide_max_guidance=0.5)),
        'image_thr': (p[1], dict(guide_threshold_mult=0.25, guide_threshold_floor=0.05,
                                 guide_clustered=0.0, guide_linear=(0.0, 0.0),
                                 guide_max_guidance=0.35, guide_header_max=0.0)),
        'c3_clustered_threshold': (p[0], C3),
        'concepts': (p[0], dict(mapping_concepts='turtle photo', guide_clustered=0.0)),
    }
    img_dev = g.encoder.image(img).float()
    for name, (prompt, kw) in cases.items():
        text_dev = g.encoder.prompt(prompt).float()
        try:
            out = g.embeds(prompt=prompt, guide=img, **kw).cpu()
        except ZeroDivisionError:
            with pytest.raises(ZeroDivisionError):      # the oracle must raise on the same input
                G.tween(text_dev.cpu(), img_dev.cpu(), (kw.get('guide_threshold_floor', 0.5),
                        kw.get('guide_threshold_mult', 0.5)), kw.get('guide_linear', (0.0, 0.5)),
                        kw.get('guide_clustered', 0.5), kw.get('guide_max_guidance', 0.5),
                        kw.get('guide_header_max', 0.15), 1, True)
            continue
        tw = g.last_tweener
        idx, sdev = tw.last_map
        mapped = _np.zeros((77, 2))
        mapped[:, 0] = idx[0].cpu().numpy()
        mapped[:, 1] = sdev[0].cpu().numpy().astype(_np.float64)
        args = ((kw.get('guide_threshold_floor', 0.5), kw.get('guide_threshold_mult', 0.5)),
                kw.get('guide_linear', (0.0, 0.5)), kw.get('guide_clustered', 0.5),
                kw.get('guide_max_guidance', 0.5), kw.get('guide_header_max', 0.15), 1, True)
        want, w, _ = G.tween(text_dev.cpu(), img_dev.cpu(), *args, mapped=mapped)
        own, _, own_map = G.tween(text_dev.cpu(), img_dev.cpu(), *args)
        if kw.get('mapping_concepts'):
            concept_dev = g.encoder.prompt(kw['mapping_concepts']).float().cpu()
            want = G.concept_override(img_dev.cpu(), concept_dev, text_dev.cpu(), out=want)
            own = G.concept_override(img_dev.cpu(), concept_dev, text_dev.cpu(), out=own)
        assert _np.array_equal(w.numpy(), tw.last_weights[0].cpu().numpy()), name
        assert torch.equal(out, want), f'{name}: Guide.embeds != oracle tween of the device embeddings'
        assert _np.array_equal(own_map[:, 0], mapped[:, 0]), name
        assert float((out - own).abs().max()) <= 1e-5, name
        assert float((out - text_dev.cpu()).abs().max()) > 1e-3, f'{name}: the guide changed nothing'
        if 'guide/' + name in cg.files:
            ref = cg['guide/' + name]
            assert out.shape == ref.shape
            assert _np.max(_np.abs(out.numpy() - ref)) < 3e-2 * max(1.0, _np.abs(ref).max()), name
    # a batch of prompts with a guide (the reference raises IndexError there, E2): row b equals
    # the single-prompt result
    both = g.embeds(prompt=p[:2], guide=img, **cases['image_linear'][1]).cpu()
    for b in range(2):
        one = g.embeds(prompt=p[b], guide=img, **cases['image_linear'][1]).cpu()
        assert torch.equal(both[b], one[0])
    with pytest.raises(ValueError):
        g.embeds(prompt=3)
    with pytest.raises(ValueError):
        g.embeds(prompt='', guide=None)


def test_unet_forward_vs_oracle(mini, dev):
    from oracle import unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    g = torch.Generator().manual_seed(1)
    B, h = 2, 16
    x = torch.randn((B, 4, h, h), generator=g)
    ctx = torch.randn((B, 77, ucfg.cross_attention_dim), generator=g).half().float()
    for t in (981, 500, 1):
        want = unet_ref.unet_forward(sds['unet'], ucfg, x, t, ctx)
        got = pipe.unet(x.to(dev), t, encoder_hidden_states=ctx.to(dev)).sample
        assert got.shape == want.shape
        e = relerr(got, want)
        assert e < 3e-2, (t, e)


def test_unet_cfg_prefix_sharing_matches_replicated_batch(mini, dev):
    '''forward_nhwc(rep=2) computes conv_in, the first ResBlock and the first self-attention once
    for both CFG branches; it must equal the plain forward of the replicated batch (oracle
    semantics of pipeline/guide.py:46-58: latents duplicated, one UNet call).'''
    from oracle import unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    g = torch.Generator().manual_seed(5)
    B, h = 3, 16
    x = torch.randn((B, 4, h, h), generator=g)
    ctx = torch.randn((2 * B, 77, ucfg.cross_attention_dim), generator=g).half().float()
    shared = pipe.unet.forward_nhwc(x.to(dev), 437, ctx.to(dev), rep=2)
    plain = pipe.unet.forward_nhwc(torch.cat([x, x]).to(dev), 437, ctx.to(dev), rep=1)
    assert shared.shape == plain.shape == (2 * B * h * h, 4)
    # not bit-identical: the shared prefix runs its GEMMs at M = B*HW, the replicated batch at 2*B*HW, so
    # tile / split-K choices (fp32 summation order) differ and an fp16 rounding can flip (1 ulp = 1e-3)
    assert float((shared - plain).abs().max()) <= 2e-3 * float(plain.abs().max())
    want = unet_ref.unet_forward(sds['unet'], ucfg, torch.cat([x, x]), 437, ctx)
    got = shared.view(2 * B, h, h, 4).permute(0, 3, 1, 2)
    assert relerr(got, want) < 3e-2


def test_unet_inplace_skip_concat_equals_copying_concat(mini, dev):
    '''Skips are written by their producers straight into the decoder's concatenation buffers
    (strided GroupNorm / GEMM operands, no k_concat).  Same kernels, same arithmetic, only the
    placement differs: the result must be bit-identical to the copying concatenation, for the
    plain and the CFG-shared forward.'''
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    unet = pipe.unet
    plan = unet._cat_plan
    assert sum(c is not None for c in plan) >= len(plan) - sum(b['down'] is not None and b['down'].im2col for b in unet.down)
    g = torch.Generator().manual_seed(9)
    B, h = 2, 16
    x = torch.randn((B, 4, h, h), generator=g).to(dev)
    ctx = torch.randn((2 * B, 77, ucfg.cross_attention_dim), generator=g).half().float().to(dev)
    got = [unet.forward_nhwc(x, 311, ctx, rep=2).clone(), unet.forward_nhwc(torch.cat([x, x]), 311, ctx).clone()]
    try:
        unet._cat_plan = [None] * len(plan)
        want = [unet.forward_nhwc(x, 311, ctx, rep=2).clone(), unet.forward_nhwc(torch.cat([x, x]), 311, ctx).clone()]
    finally:
        unet._cat_plan = plan
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_vae_decode_encode_vs_oracle(mini, dev):
    from oracle import vae_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    g = torch.Generator().manual_seed(2)
    z = torch.randn((2, 4, 16, 16), generator=g)
    want = vae_ref.vae_decode(sds['vae'], vcfg, z)
    got = pipe.vae.decode(z.to(dev)).sample
    assert got.shape == want.shape
    assert relerr(got, want) < 3e-2
    img = torch.rand((1, 3, 64, 64), generator=g) * 2 - 1
    mean, logvar = vae_ref.vae_encode_moments(sds['vae'], vcfg, img)
    dist = pipe.vae.encode(img.to(dev)).latent_dist
    assert relerr(dist.mean, mean) < 3e-2 and relerr(dist.logvar, logvar) < 3e-2
    noise = torch.randn(mean.shape, generator=g)
    assert relerr(dist.sample_with(noise.to(dev)), vae_ref.vae_sample(mean, logvar, noise)) < 3e-2


def _run_both(mini, dev, steps, B, guidance, hw, fused=True, init=None, strength=0.6):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    prompts = ['a photo of a turtle', 'zeus, oil painting'][:B]
    ids = tok(prompts).input_ids
    emb_ref = clip_ref.text_hidden(sds['clip'], ccfg, ids)
    unc_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    emb_dev = enc.prompt(prompts)
    guide = SimpleGuide(enc, pipe.unet, guidance, steps, emb_dev)
    if not fused:   # force the generic GuideBase protocol path
        class Wrapped(SimpleGuide):
            def noise_pred(self, latents, step):
                return SimpleGuide.noise_pred(self, latents, step)
        guide = Wrapped(enc, pipe.unet, guidance, steps, emb_dev)
    gen = torch.Generator('cpu').manual_seed(1337)
    lat0 = torch.randn((B, 4, hw // 8, hw // 8), generator=gen)
    out = pipe(guide=guide, init_size=(hw, hw), generator=torch.Generator('cpu').manual_seed(1337),
               output_type='np')
    lat_ref, used = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, guidance)
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    return out, pipe, lat_ref, img_ref, used


def test_pipeline_end_to_end_psnr(mini, dev):
    '''txt2img, 10 DDIM steps, CFG 8, batch 2: exact timesteps, PSNR >= 40 dB vs CPU oracle.'''
    from oracle import pipeline_ref
    steps = 10
    out, pipe, lat_ref, img_ref, used = _run_both(mini, dev, steps, 2, 8.0, 128)
    assert used == [int(t) for t in pipe.scheduler.timesteps] == list(range(900, -1, -100))
    up = 2 ** (len(mini[4][1].block_out_channels) - 1)      # the mini VAE upsamples x2, not x8
    assert out.images.shape == (2, 16 * up, 16 * up, 3)
    lat_err = relerr(pipe.last_latents, lat_ref)
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'latent rel err {lat_err:.4f}, PSNR {p:.1f} dB')
    assert p >= 40.0, p
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'


def test_generic_guide_protocol_matches_fused(mini, dev):
    '''A guide going through guide.noise_pred + scheduler.step equals the fused loop.'''
    out_f, pipe, *_ = _run_both(mini, dev, 4, 1, 8.0, 64, fused=True)
    lat_f = pipe.last_latents.clone()
    out_g, pipe, *_ = _run_both(mini, dev, 4, 1, 8.0, 64, fused=False)
    assert torch.equal(lat_f, pipe.last_latents)


def test_pipeline_errors_and_outputs(mini, dev):
    from flexdiffuse_amd import PromptGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    guide = PromptGuide(enc, pipe.unet, 1.0, 2, 'a cat')     # guidance <= 1: no CFG
    with pytest.raises(ValueError):
        pipe(guide=guide, strength=1.5)
    out = pipe(guide=guide, init_size=(64, 64), generator=torch.Generator('cpu').manual_seed(3))
    assert len(out.images) == 1 and out.images[0].size == (16, 16)   # mini VAE: x2
    assert out['sample'] is out.images and out.nsfw_content_detected == [False]
    imgs, flag = pipe(guide=guide, init_size=(64, 64), return_dict=False, debug=True,
                      generator=torch.Generator('cpu').manual_seed(3))
    assert flag is False and len(imgs) == 3     # initial + 2 steps


@pytest.fixture(scope='module')
def sd15(dev):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False)
    return sds, pipe, clip, tok, build.configs('sd15')


def test_sd15_c1_pipeline_psnr(sd15, dev):
    '''BASELINE configs[0] shape on the full SD1.5 architecture (859,520,964-parameter UNet,
    83.6 M VAE, CLIP ViT-L/14 text tower): 256x256, 10 DDIM steps, batch 1, CFG 8.
    GPU fp16 path vs CPU fp32 oracle on identical seeded weights, ids and CPU-drawn noise:
    integer timestep lists equal, final-image PSNR >= 40 dB, latent error reported.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    enc = CLIPEncoder(clip, tok)
    prompt = 'a photo of a turtle in a forest, oil painting'
    steps, guidance, hw = 10, 8.0, 256
    emb_dev = enc.prompt(prompt)
    out = pipe(guide=SimpleGuide(enc, pipe.unet, guidance, steps, emb_dev), init_size=(hw, hw),
               generator=torch.Generator('cpu').manual_seed(1337), output_type='np')
    text_sd = {k: v for k, v in sds['clip'].items() if k.startswith('text_model')}
    emb_ref = clip_ref.text_hidden(text_sd, ccfg, tok(prompt).input_ids)
    unc_ref = clip_ref.text_hidden(text_sd, ccfg, tok('').input_ids)
    assert relerr(emb_dev, emb_ref) < 2e-2
    lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref, used = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, guidance)
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    assert used == [int(t) for t in pipe.scheduler.timesteps]
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'SD1.5 c1: latent rel err {relerr(pipe.last_latents, lat_ref):.4f}, PSNR {p:.1f} dB, '
          f'image std {float(img_ref.std()):.3f}')
    assert out.images.shape == (1, hw, hw, 3)
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    assert p >= 40.0, p


def test_sd15_c2_headline_psnr(sd15, dev):
    '''BASELINE configs[1] -- the headline configuration -- at batch 1: SD1.5, 512x512, 50 DDIM
    steps, CFG 8, Linear image guidance.  Device path (Guide.embeds with the ViT-L/14 guide ->
    FlexPipeline, fp16) vs the CPU fp32 oracle of the same sample, whose 100 UNet forwards are
    cached as data in tests/golden/c2_oracle.npz (tests/golden/make_c2_oracle.py; the oracle's
    VAE decode runs here).  Integer timestep lists equal, guided embeddings close, final-image
    PSNR >= 40 dB (north_star), latent error reported.  Reference loop: pipeline/flex.py:262-287.'''
    import hashlib
    import sys
    sys.path.insert(0, GOLDEN)
    from make_c2_oracle import C2, c2_inputs
    from flexdiffuse_amd import Guide, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    o = np.load(os.path.join(GOLDEN, 'c2_oracle.npz'))
    steps, size = int(o['steps'][0]), int(o['size'][0])
    assert (steps, size) == (50, 512)
    prompt, img, lat0 = c2_inputs(size)
    assert hashlib.sha256(lat0.numpy().tobytes()).digest() == o['lat0_sha'].tobytes()
    g = Guide(clip, tok, device='cuda')
    embeds = g.embeds(prompt=prompt, guide=img, **C2['embeds_kw'])
    emb_err = float((embeds.float().cpu() - torch.from_numpy(o['embeds'])).abs().max())
    text_moved = float((torch.from_numpy(o['embeds']) - torch.from_numpy(o['text'])).abs().max())
    assert text_moved > 0.1, 'the oracle guidance changed nothing: parity would be vacuous'
    assert emb_err < 3e-2 * max(1.0, float(np.abs(o['embeds']).max())), emb_err
    enc = CLIPEncoder(clip, tok)
    out = pipe(guide=SimpleGuide(enc, pipe.unet, C2['guidance'], steps, embeds), init_size=(size, size),
               latents=lat0, output_type='np')
    assert [int(t) for t in o['timesteps']] == [int(t) for t in pipe.scheduler.timesteps] \
        == list(range(980, -1, -20))
    lat_ref = torch.from_numpy(o['latents'])
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'SD1.5 c2 (512x512, 50 steps, Linear image guidance): guided-embedding max err {emb_err:.4f}, '
          f'latent rel err {relerr(pipe.last_latents, lat_ref):.4f}, PSNR {p:.1f} dB, '
          f'image std {float(img_ref.std()):.3f}')
    assert out.images.shape == (1, size, size, 3)
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    assert p >= 40.0, p
    # the bench runs batch 8 (CFG batch 16): other tile / split-K choices and the shared CFG prefix than
    # batch 1.  Sample 0 of the batch-8 pass (bench.py's prompts and noise) against the same oracle latents.
    import bench
    from flexdiffuse_amd import dist as fdist
    prompts = bench.synth_prompts(8)
    assert prompts[0] == prompt
    emb8 = g.embeds(prompt=prompts, guide=img, **C2['embeds_kw'])
    noise8 = fdist.global_noise(8, (4, size // 8, size // 8), C2['noise_seed'])
    assert torch.equal(noise8[:1], lat0)
    pipe(guide=SimpleGuide(enc, pipe.unet, C2['guidance'], steps, emb8), init_size=(size, size), latents=noise8,
         output_type='np')
    p8 = pipeline_ref.psnr(pipe.last_images[:1].cpu(), img_ref)
    print(f'SD1.5 c2 at batch 8, sample 0: latent rel err {relerr(pipe.last_latents[:1], lat_ref):.4f}, PSNR {p8:.1f} dB')
    assert p8 >= 40.0, p8
    # that pass ran in the default launch mode = HIP-graph replay, the mode the driver's bench line is measured in; the
    # launch plan must give the same bits at full size
    assert pipe.use_graph and pipe.graph_fallback is None and len(pipe._graphs) == 1
    lat_graph = pipe.last_latents.clone()
    try:
        pipe.use_graph = False
        pipe(guide=SimpleGuide(enc, pipe.unet, C2['guidance'], steps, emb8), init_size=(size, size), latents=noise8,
             output_type='np')
        assert torch.equal(lat_graph, pipe.last_latents), 'graph replay and launch plan differ at batch 8'
    finally:
        pipe.use_graph = True


def test_sd15_c3_clustered_threshold_psnr(sd15, dev):
    '''BASELINE configs[2] guidance (Clustered 0.25 + Threshold (0.75, 0.25), linear off, max 0.35, header cap 0) on
    sample 0 of the headline workload: device path vs the cached CPU oracle of the same sample
    (tests/golden/c3_oracle.npz, `make_c2_oracle.py --guidance clustered_threshold`); PSNR >= 40 dB.'''
    path = os.path.join(GOLDEN, 'c3_oracle.npz')
    if not os.path.exists(path):
        pytest.skip('tests/golden/c3_oracle.npz not generated')
    import sys
    sys.path.insert(0, GOLDEN)
    import bench
    from make_c2_oracle import C2, c2_inputs
    from flexdiffuse_amd import Guide, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    o = np.load(path)
    steps, size = int(o['steps'][0]), int(o['size'][0])
    prompt, img, lat0 = c2_inputs(size)
    embeds = Guide(clip, tok, device='cuda').embeds(prompt=prompt, guide=img, **bench.GUIDANCE['clustered_threshold'])
    emb_ref = torch.from_numpy(o['embeds'])
    emb_err = float((embeds.float().cpu() - emb_ref).abs().max())
    moved = float((emb_ref - torch.from_numpy(o['text'])).abs().max())
    assert moved > 0.05, 'the oracle guidance changed nothing: parity would be vacuous'
    assert emb_err < 3e-2 * max(1.0, float(emb_ref.abs().max())), emb_err
    out = pipe(guide=SimpleGuide(CLIPEncoder(clip, tok), pipe.unet, C2['guidance'], steps, embeds),
               init_size=(size, size), latents=lat0, output_type='np')
    assert [int(t) for t in o['timesteps']] == [int(t) for t in pipe.scheduler.timesteps]
    lat_ref = torch.from_numpy(o['latents'])
    p = pipeline_ref.psnr(pipe.last_images.cpu(), pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'SD1.5 c3 guidance (Clustered + Threshold): guided-embedding max err {emb_err:.4f} (text moved {moved:.3f}), '
          f'latent rel err {relerr(pipe.last_latents, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert out.images.shape == (1, size, size, 3) and p >= 40.0, p


@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_sd15_c2_under_pndm_and_lms_psnr(sd15, dev, kind):
    '''The headline sample at FULL size (SD1.5, 512x512, 50 steps, CFG 8, Linear image guidance) under the scheduler the
    reference's harness really passes -- SD-v1-4 ships PNDM (utils.py:70; PLMS: 51 UNet evaluations) -- and under K-LMS with the
    pipeline's sigma scaling (pipeline/flex.py:236-238, 270-274): device pipeline (UNet forward from the launch plan, scheduler
    arithmetic through the generic protocol) vs the CPU oracle's final latents cached by
    `tests/golden/make_c2_oracle.py --scheduler pndm|lms` (oracle/sched_ref.py, parity unpinned like the rest of diffusers);
    final-image PSNR >= 40 dB.'''
    path = os.path.join(GOLDEN, f'c2_{kind}_oracle.npz')
    if not os.path.exists(path):
        pytest.skip(f'{path} not generated')
    import hashlib
    import sys
    sys.path.insert(0, GOLDEN)
    from make_c2_oracle import C2, c2_inputs
    from flexdiffuse_amd import FlexPipeline, Guide, LMSDiscreteScheduler, PNDMScheduler, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    o = np.load(path)
    steps, size = int(o['steps'][0]), int(o['size'][0])
    prompt, img, lat0 = c2_inputs(size)
    assert hashlib.sha256(lat0.numpy().tobytes()).digest() == o['lat0_sha'].tobytes()
    sched = PNDMScheduler() if kind == 'pndm' else LMSDiscreteScheduler()
    p2 = FlexPipeline(pipe.vae, clip, tok, pipe.unet, sched).to(dev)
    embeds = Guide(clip, tok, device='cuda').embeds(prompt=prompt, guide=img, **C2['embeds_kw'])
    out = p2(guide=SimpleGuide(CLIPEncoder(clip, tok), pipe.unet, C2['guidance'], steps, embeds), init_size=(size, size),
             latents=lat0, output_type='np')
    if kind == 'pndm':
        assert [int(t) for t in o['timesteps']] == [int(t) for t in sched.timesteps] and int(o['evaluations'][0]) == steps + 1
    else:
        assert np.allclose(o['sigmas'], sched.sigmas) and int(o['evaluations'][0]) == steps
    lat_ref = torch.from_numpy(o['latents'])
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(p2.last_images.cpu(), img_ref)
    print(f'SD1.5 c2 sample under {kind.upper()}: latent rel err {relerr(p2.last_latents, lat_ref):.4f}, PSNR {p:.1f} dB, '
          f'image std {float(img_ref.std()):.3f}')
    assert out.images.shape == (1, size, size, 3) and float(img_ref.std()) > 0.02
    assert p >= 40.0, p


def _cached_oracle_psnr(name, dev, pipe, clip, tok, sds, vcfg):
    '''Device path of sample 0 of BASELINE configs[3] / configs[4] against the CPU fp32 oracle's final latents
    cached by tests/golden/make_c45_oracle.py (its 60 / 100 UNet forwards at 96x96 take 20-35 CPU-minutes);
    the oracle's VAE decode runs here.'''
    import hashlib
    import sys
    sys.path.insert(0, GOLDEN)
    from make_c45_oracle import CONFIGS, inputs
    from flexdiffuse_amd import Guide, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import pipeline_ref
    c = CONFIGS[name]
    o = np.load(os.path.join(GOLDEN, f'{name}_oracle.npz'))
    inp = inputs(name)
    enc = CLIPEncoder(clip, tok)
    embeds = Guide(clip, tok, device='cuda').embeds(prompt=inp['prompt'], guide=inp['guide'], **c['embeds_kw'])
    d_emb = (embeds.float().cpu() - torch.from_numpy(o['embeds'])).abs()[0]
    emb_err, emb_mag = float(d_emb.max()), max(1.0, float(np.abs(o['embeds']).max()))
    tok_err = d_emb.max(dim=1).values
    print(f'{name}: guided-embedding max err {emb_err:.4f} of magnitude {emb_mag:.2f}; tokens above 1 %: '
          f'{[int(i) for i in torch.nonzero(tok_err > 1e-2 * emb_mag).flatten()]}')
    # fp16 CLIP towers (32-layer ViT-H for c5) against the fp32 oracle: 5 % of the embedding magnitude; what
    # this stage may cost the IMAGE is bounded by the PSNR assertion below
    assert emb_err < 5e-2 * emb_mag, emb_err
    guide = SimpleGuide(enc, pipe.unet, c['guidance'], c['steps'], embeds)
    if c['strength'] is not None:
        assert hashlib.sha256(inp['noise'].numpy().tobytes()).digest() == o['noise_sha'].tobytes()
        out = pipe(guide=guide, init_image=inp['init'], strength=c['strength'],
                   generator=torch.Generator('cpu').manual_seed(c['gen_seed']), output_type='np')
        want_t = [int(t) for t in pipe.scheduler.timesteps[int(o['t_start'][0]):]]
    else:
        assert hashlib.sha256(inp['lat0'].numpy().tobytes()).digest() == o['noise_sha'].tobytes()
        out = pipe(guide=guide, init_size=(c['size'], c['size']), latents=inp['lat0'], output_type='np')
        want_t = [int(t) for t in pipe.scheduler.timesteps]
    assert [int(t) for t in o['timesteps']] == want_t
    lat_ref = torch.from_numpy(o['latents'])
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'{name}: guided-embedding max err {emb_err:.4f}, latent rel err {relerr(pipe.last_latents, lat_ref):.4f}, '
          f'PSNR {p:.1f} dB, image std {float(img_ref.std()):.3f}, {len(want_t)} UNet evaluations')
    assert out.images.shape == (1, c['size'], c['size'], 3)
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    # the config's REAL per-GPU batch (c4: 4, c5: 8 -- other tile / split-K choices, the 288-row tiles and the
    # shared CFG prefix than batch 1): sample 0 of bench.py's batch against the same cached oracle latents
    import bench
    from flexdiffuse_amd import dist as fdist
    nb, h = c['batch'], c['size'] // 8
    prompts = bench.synth_prompts(nb)
    assert prompts[0] == inp['prompt']
    emb_b = Guide(clip, tok, device='cuda').embeds(prompt=prompts, guide=inp['guide'], **c['embeds_kw'])
    guide_b = SimpleGuide(enc, pipe.unet, c['guidance'], c['steps'], emb_b)
    if c['strength'] is not None:
        post, noise_b = fdist.global_img2img_noise(nb, (4, h, h), c['gen_seed'])
        # batch 1 drew (1,4,h,h) twice from the same generator: the posterior sample is shared, and sample 0's
        # add_noise row is given the batch-1 draw so that the cached oracle applies
        noise_b = torch.cat([inp['noise'], noise_b[1:]])
        assert torch.equal(post, inp['posterior_noise'])
        pipe(guide=guide_b, init_image=inp['init'], strength=c['strength'], noise=noise_b,
             generator=torch.Generator('cpu').manual_seed(c['gen_seed']), output_type='np')
    else:
        noise_b = fdist.global_noise(nb, (4, h, h), c['noise_seed'])
        assert torch.equal(noise_b[:1], inp['lat0'])
        pipe(guide=guide_b, init_size=(c['size'], c['size']), latents=noise_b, output_type='np')
    assert pipe.last_images.shape[0] == nb
    pb = pipeline_ref.psnr(pipe.last_images[:1].cpu(), img_ref)
    spread = float((pipe.last_images[0] - pipe.last_images[1]).abs().mean())
    print(f'{name} at batch {nb}, sample 0: latent rel err {relerr(pipe.last_latents[:1], lat_ref):.4f}, '
          f'PSNR {pb:.1f} dB; sample 0 vs 1 mean abs difference {spread:.3f}')
    assert spread > 1e-3, 'all samples of the batch are the same image'
    return min(p, pb)


def test_sd15_c4_img2img_psnr(dev):
    '''BASELINE configs[3] at batch 1 and at its per-GPU batch 4 (sample 0): SD1.5 img2img + Linear image guidance, 768x768, 50 DDIM steps, strength
    0.6 => the 30 evaluations of timesteps[20:] (reference pipeline/flex.py:181-221 init, :262-287 loop): VAE
    encode -> posterior sample -> add_noise -> loop -> decode on the device vs the cached CPU oracle;
    final-image PSNR >= 40 dB.'''
    if not os.path.exists(os.path.join(GOLDEN, 'c4_oracle.npz')):
        pytest.skip('tests/golden/c4_oracle.npz not generated (tests/golden/make_c45_oracle.py c4)')
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=True)
    p = _cached_oracle_psnr('c4', dev, pipe, clip, tok, sds, build.configs('sd15')[1])
    assert p >= 40.0, p


def test_sd21_c5_psnr(dev):
    '''BASELINE configs[4] at batch 1 and at its per-GPU batch 8 (sample 0): SD2.1-size UNet (v-prediction, head dim 64, linear projections, context
    1024) + OpenCLIP ViT-H/14 guide, 768x768, 50 DDIM steps, CFG 8, Linear image guidance, vs the cached CPU
    oracle (no reference behaviour exists for c5: the oracle is the target); final-image PSNR >= 40 dB.'''
    if not os.path.exists(os.path.join(GOLDEN, 'c5_oracle.npz')):
        pytest.skip('tests/golden/c5_oracle.npz not generated (tests/golden/make_c45_oracle.py c5)')
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('sd21', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd21', dev, vae_encoder=False)
    p = _cached_oracle_psnr('c5', dev, pipe, clip, tok, sds, build.configs('sd21')[1])
    assert p >= 40.0, p


def test_img2img_vs_oracle(mini, dev):
    '''img2img branch (pipeline/flex.py:181-221): VAE encode -> posterior sample -> x0.18215 ->
    add_noise at timesteps[-init_timestep] -> loop from t_start.  strength 0.6 / 10 steps.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    steps, strength, guidance, B = 10, 0.6, 8.0, 2
    prompts = ['a photo of a turtle', 'zeus, oil painting']
    g = torch.Generator().manual_seed(5)
    image = (torch.rand((1, 3, 32, 32), generator=g) * 2 - 1).half().float()
    emb_dev = enc.prompt(prompts)
    out = pipe(guide=SimpleGuide(enc, pipe.unet, guidance, steps, emb_dev), init_image=image,
               strength=strength, generator=torch.Generator('cpu').manual_seed(11),
               output_type='np')
    # the same two draws from the same CPU generator stream: posterior noise, then latent noise
    gen = torch.Generator('cpu').manual_seed(11)
    post = torch.randn((1, 4, 16, 16), generator=gen)
    noise = torch.randn((B, 4, 16, 16), generator=gen)
    lat0, t_start = pipeline_ref.img2img_init(sds['vae'], vcfg, image, post, noise, steps, strength, B)
    assert t_start == 4
    ids = tok(prompts).input_ids
    emb_ref = clip_ref.text_hidden(sds['clip'], ccfg, ids)
    unc_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    lat_ref, used = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, guidance,
                                         t_start=t_start)
    assert used == [500, 400, 300, 200, 100, 0]
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'img2img: latent rel err {relerr(pipe.last_latents, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert p >= 40.0, p


def test_sd2_style_unet_vprediction(dev):
    '''SD2.x-shaped small model (linear proj_in/out, head dim 64, v-prediction; BASELINE
    config 5's differences from SD1.x) vs the CPU oracle, single forward + 4-step loop.'''
    from flexdiffuse_amd import SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, pipeline_ref, unet_ref
    sds = build.synthetic_state_dicts('mini2', seed=1)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    pipe, clip, tok = build.build_models(sds, 'mini2', dev)
    ucfg, vcfg, ccfg = build.configs('mini2')
    assert ucfg.use_linear_projection and ucfg.prediction_type == 'v_prediction'
    g = torch.Generator().manual_seed(1)
    x = torch.randn((2, 4, 16, 16), generator=g)
    ctx = torch.randn((2, 77, ucfg.cross_attention_dim), generator=g).half().float()
    want = unet_ref.unet_forward(sds['unet'], ucfg, x, 500, ctx)
    got = pipe.unet(x.to(dev), 500, encoder_hidden_states=ctx.to(dev)).sample
    assert relerr(got, want) < 3e-2
    enc = CLIPEncoder(clip, tok)
    emb_dev = enc.prompt('a cat')
    pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 4, emb_dev), init_size=(64, 64),
         generator=torch.Generator('cpu').manual_seed(2), output_type='np')
    emb_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok('a cat').input_ids)
    unc_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    lat0 = torch.randn((1, 4, 8, 8), generator=torch.Generator('cpu').manual_seed(2))
    lat_ref, _ = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, 4, 8.0)
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(pipe.last_images.cpu(), img_ref)
    print(f'sd2-style: PSNR {p:.1f} dB')
    assert p >= 40.0, p


def test_runner_gen_recipe(dev):
    '''utils.Runner.gen call recipe: seed -> Guide.embeds -> SimpleGuide -> sequential batches;
    the same seed reproduces the same images, a different seed does not.'''
    from flexdiffuse_amd import Runner
    from test_oracle_clip import synth_image
    r = Runner(preset='mini', device='cuda')
    img = synth_image(20, 512, 512)
    imgs, grid = r.gen(prompt='a photo of a turtle', guide=img, init_size=(64, 64), steps=3,
                       samples=2, seed=1337, guide_clustered=0.0)
    assert len(imgs) == 2 and grid.size == (2 * imgs[0].size[0], imgs[0].size[1])
    again, _ = r.gen(prompt='a photo of a turtle', guide=img, init_size=(64, 64), steps=3,
                     samples=2, seed=1337, guide_clustered=0.0)
    other, _ = r.gen(prompt='a photo of a turtle', guide=img, init_size=(64, 64), steps=3,
                     samples=1, seed=7, guide_clustered=0.0)
    assert np.array_equal(np.asarray(imgs[0]), np.asarray(again[0]))
    assert np.array_equal(np.asarray(imgs[1]), np.asarray(again[1]))
    assert not np.array_equal(np.asarray(imgs[0]), np.asarray(other[0]))
    assert r._set_seed(-5) == 0 and r._set_seed(2 ** 40) == 2147483647


def test_runner_gen_vs_oracle(dev):
    '''utils.Runner.gen against the oracle (reference utils.py:149-166: seed -> generator, Guide.embeds with
    gen's own defaults, `samples` sequential pipeline calls on ONE generator stream): the oracle replays the
    recipe -- CPU generator seeded with the clamped seed, one randn per batch, GuideRef.embeds,
    pipeline_ref.denoise, decode -- and every returned PIL image must match at PSNR >= 40 dB.'''
    from flexdiffuse_amd import Runner, build
    from flexdiffuse_amd.tokenizer import SyntheticTokenizer
    from oracle import guide_ref, pipeline_ref
    from test_oracle_clip import synth_image
    sds = build.synthetic_state_dicts('mini', seed=0)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    ucfg, vcfg, ccfg = build.configs('mini')
    r = Runner(state_dicts=sds, preset='mini', device='cuda')
    img = synth_image(20, 512, 512)
    steps, samples, seed, hw = 4, 2, 2 ** 40, 64          # the seed is clamped to 2^31 - 1 (utils.py:78-83)
    kw = dict(guide_clustered=0.0, guide_threshold_mult=0.25, guide_linear=(0.0, 0.5))
    imgs, grid = r.gen(prompt='a photo of a turtle', guide=img, init_size=(hw, hw), steps=steps, samples=samples,
                       seed=seed, guidance_scale=8, **kw)
    assert len(imgs) == samples
    tok = SyntheticTokenizer(vocab_size=ccfg.text.vocab_size, model_max_length=ccfg.text.max_position_embeddings)
    g = guide_ref.GuideRef(sds['clip'], ccfg, tok)
    embeds = g.embeds(prompt='a photo of a turtle', guide=img, guide_mode=0, **kw)     # gen's default guide_mode is 0
    gen = torch.Generator('cpu').manual_seed(2147483647)
    for k in range(samples):
        lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=gen)
        lat, _ = pipeline_ref.denoise(sds['unet'], ucfg, embeds, g.prompt(''), lat0, steps, 8.0)
        want = (pipeline_ref.decode_image(sds['vae'], vcfg, lat) * 255).round() / 255
        got = torch.from_numpy(np.asarray(imgs[k]).astype(np.float32) / 255).permute(2, 0, 1)[None]
        p = pipeline_ref.psnr(got, want)
        print(f'Runner.gen sample {k}: PSNR {p:.1f} dB vs the oracle recipe')
        assert p >= 40.0, (k, p)
    assert float((torch.from_numpy(np.asarray(imgs[0]).astype(np.float32)) -
                  torch.from_numpy(np.asarray(imgs[1]).astype(np.float32))).abs().mean()) > 0.5   # different noise per batch


def test_runner_from_checkpoint_directories_vs_oracle(dev, tmp_path):
    '''SURVEY 8(f) rank 4, end to end on the device: files on disk -> `Runner(local=True, device=...)` built the
    way the reference builds it (utils.py:54-76: CLIPModel + StableDiffusionPipeline checkpoints -> models AND the
    real tokenizer; the hub ids become local directories) -> `gen` -> images, against the oracle fed from the same
    files through independent readers (safetensors.torch.load_file; transformers.CLIPTokenizer on the same
    vocab.json / merges.txt as the third-party tokenizer oracle).  PSNR >= 40 dB per image.'''
    import json
    from safetensors.torch import load_file, save_file
    from flexdiffuse_amd import FlexPipeline, Runner, build
    from flexdiffuse_amd.tokenizer import CLIPBPETokenizer
    from oracle import guide_ref, pipeline_ref
    from test_oracle_clip import synth_image
    from test_tokenizer import toy_vocab
    preset = 'mini_bpe'
    sds = build.synthetic_state_dicts(preset, seed=5)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    sd_dir, clip_dir = tmp_path / 'stable-diffusion', tmp_path / 'clip'
    for sub in ('unet', 'vae', 'tokenizer'):
        os.makedirs(sd_dir / sub)
    os.makedirs(clip_dir)
    save_file({k: v.contiguous() for k, v in sds['unet'].items()}, str(sd_dir / 'unet' / 'diffusion_pytorch_model.safetensors'))
    save_file({k: v.contiguous() for k, v in sds['vae'].items()}, str(sd_dir / 'vae' / 'diffusion_pytorch_model.safetensors'))
    save_file({k: v.contiguous() for k, v in sds['clip'].items()}, str(clip_dir / 'model.safetensors'))
    vocab, merges = toy_vocab()
    ucfg, vcfg, ccfg = build.configs(preset)
    assert len(vocab) <= ccfg.text.vocab_size
    (sd_dir / 'tokenizer' / 'vocab.json').write_text(json.dumps(vocab), encoding='utf-8')
    (sd_dir / 'tokenizer' / 'merges.txt').write_text('#version: 0.2\n' + '\n'.join(' '.join(m) for m in merges) + '\n',
                                                     encoding='utf-8')
    with pytest.raises(RuntimeError):
        Runner(local=False, device='cuda', sd_dir=str(sd_dir), clip_dir=str(clip_dir), preset=preset)
    with pytest.raises(ValueError):
        Runner(local=True, device='cuda', sd_dir=str(sd_dir), preset=preset)
    # (the installed transformers is the third-party tokenizer oracle below, and its CLIPTokenizer is the FAST pipeline:
    # text_cleanup='fast' for this leg; the default 'basic' -- the reference's pinned slow tokenizer -- splits "painter's"
    # at the apostrophe and is pinned by known answers in tests/test_tokenizer.py)
    r = Runner(True, 'cuda', sd_dir=str(sd_dir), clip_dir=str(clip_dir), preset=preset, text_cleanup='fast')
    assert isinstance(r.pipe.tokenizer, CLIPBPETokenizer) and r.encoder.token is r.pipe.tokenizer
    assert type(r.pipe.scheduler).__name__ == 'DDIMScheduler'      # no scheduler/ folder in the checkpoint yet
    p0 = FlexPipeline.from_pretrained(str(sd_dir), str(clip_dir), preset=preset)
    assert isinstance(p0, FlexPipeline) and p0.tokenizer.text_cleanup == 'basic'
    assert not torch.equal(p0.tokenizer("the painter's dog").input_ids, r.pipe.tokenizer("the painter's dog").input_ids)
    prompt = "a photo of the painter's dog, highly detailed oil painting of mountains at sunset"
    img = synth_image(21, 512, 512)
    steps, samples, seed, hw = 4, 2, 77, 64
    kw = dict(guide_clustered=0.0, guide_threshold_mult=0.25, guide_linear=(0.0, 0.5))
    imgs, _ = r.gen(prompt=prompt, guide=img, init_size=(hw, hw), steps=steps, samples=samples, seed=seed,
                    guidance_scale=8, **kw)
    # ---- the oracle, from the same files through other readers
    ref_sds = {'unet': load_file(str(sd_dir / 'unet' / 'diffusion_pytorch_model.safetensors')),
               'vae': load_file(str(sd_dir / 'vae' / 'diffusion_pytorch_model.safetensors')),
               'clip': load_file(str(clip_dir / 'model.safetensors'))}
    transformers = pytest.importorskip('transformers')
    try:
        ref_tok = transformers.CLIPTokenizer(vocab=vocab, merges=merges, model_max_length=77)
    except Exception:
        ref_tok = transformers.CLIPTokenizer(vocab=vocab, merges=[' '.join(m) for m in merges], model_max_length=77)
    ids_ref = ref_tok(prompt, padding='max_length', max_length=77, truncation=True, return_tensors='pt').input_ids
    assert torch.equal(r.pipe.tokenizer(prompt).input_ids, ids_ref) and int((ids_ref != ref_tok.eos_token_id).sum()) > 10
    g = guide_ref.GuideRef(ref_sds['clip'], ccfg, ref_tok)
    embeds = g.embeds(prompt=prompt, guide=img, guide_mode=0, **kw)
    gen = torch.Generator('cpu').manual_seed(seed)
    for k in range(samples):
        lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=gen)
        lat, _ = pipeline_ref.denoise(ref_sds['unet'], ucfg, embeds, g.prompt(''), lat0, steps, 8.0)
        want = (pipeline_ref.decode_image(ref_sds['vae'], vcfg, lat) * 255).round() / 255
        got = torch.from_numpy(np.asarray(imgs[k]).astype(np.float32) / 255).permute(2, 0, 1)[None]
        p = pipeline_ref.psnr(got, want)
        print(f'Runner from checkpoint directories, sample {k}: PSNR {p:.1f} dB vs the oracle')
        assert p >= 40.0, (k, p)
    # ---- the checkpoint's OWN scheduler: CompVis/stable-diffusion-v1-4 ships scheduler/scheduler_config.json with
    # PNDM / skip_prk_steps, and the reference hands `sd.scheduler` to its pipeline (utils.py:70) -> a Runner built from such a
    # directory must sample with PLMS (steps + 1 UNet evaluations), not with DDIM; `scheduler=` overrides
    from flexdiffuse_amd import DDIMScheduler
    from oracle import sched_ref
    os.makedirs(sd_dir / 'scheduler')
    (sd_dir / 'scheduler' / 'scheduler_config.json').write_text(json.dumps({
        '_class_name': 'PNDMScheduler', '_diffusers_version': '0.2.2', 'beta_end': 0.012, 'beta_schedule': 'scaled_linear',
        'beta_start': 0.00085, 'num_train_timesteps': 1000, 'skip_prk_steps': True}), encoding='utf-8')
    r2 = Runner(True, 'cuda', sd_dir=str(sd_dir), clip_dir=str(clip_dir), preset=preset, text_cleanup='fast')
    assert type(r2.pipe.scheduler).__name__ == 'PNDMScheduler' and r2.pipe.scheduler.config['skip_prk_steps'] is True
    r3 = Runner(True, 'cuda', sd_dir=str(sd_dir), clip_dir=str(clip_dir), preset=preset, scheduler=DDIMScheduler())
    assert type(r3.pipe.scheduler).__name__ == 'DDIMScheduler'
    steps2 = 5
    imgs2, _ = r2.gen(prompt=prompt, guide=img, init_size=(hw, hw), steps=steps2, samples=1, seed=seed, guidance_scale=8, **kw)
    assert len(r2.pipe.scheduler.timesteps) == steps2 + 1
    lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=torch.Generator('cpu').manual_seed(seed))
    unc = g.prompt('')
    eps_fn = lambda x, t: pipeline_ref.noise_pred(ref_sds['unet'], ucfg, x, t, embeds, unc, 8.0)
    lat, used = sched_ref.pndm_loop(eps_fn, lat0, steps2)
    assert used == [int(t) for t in r2.pipe.scheduler.timesteps]
    want = (pipeline_ref.decode_image(ref_sds['vae'], vcfg, lat) * 255).round() / 255
    got = torch.from_numpy(np.asarray(imgs2[0]).astype(np.float32) / 255).permute(2, 0, 1)[None]
    p = pipeline_ref.psnr(got, want)
    print(f'Runner from a checkpoint that ships a PNDM scheduler_config.json: {steps2 + 1} UNet evaluations, PSNR {p:.1f} dB vs the PLMS oracle')
    assert p >= 40.0, p


def test_ddim_eta_step_and_loop_vs_oracle(mini, dev):
    '''DDIM eta > 0 (the reference passes `eta` through to scheduler.step, pipeline/flex.py:247-251,280-285):
    (a) one scheduler.step with eta = 0.5 and an explicit CPU generator vs ddim_ref with the same noise, on
    epsilon- and v-prediction; (b) the whole loop at eta = 0.5 -- the generic guide.noise_pred + scheduler.step
    path, variance noise from torch's global CPU generator as the reference's scheduler draws it -- vs the
    oracle loop fed the same noise stream: PSNR >= 40 dB.'''
    from flexdiffuse_amd import DDIMScheduler, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, ddim_ref, pipeline_ref
    g = torch.Generator().manual_seed(4)
    x, eps = torch.randn((2, 4, 8, 8), generator=g), torch.randn((2, 4, 8, 8), generator=g)
    acp = ddim_ref.alphas_cumprod()
    for pred in ('epsilon', 'v_prediction'):
        sch = DDIMScheduler(prediction_type=pred)
        sch.set_timesteps(10)
        for t in (900, 400, 0):
            got = sch.step(eps.to(dev), t, x.to(dev), eta=0.5, generator=torch.Generator('cpu').manual_seed(9)).prev_sample
            z = torch.randn(x.shape, generator=torch.Generator('cpu').manual_seed(9))
            want = ddim_ref.ddim_step(eps, t, x, acp, 10, prediction_type=pred, eta=0.5, noise=z)
            det = ddim_ref.ddim_step(eps, t, x, acp, 10, prediction_type=pred)
            assert float((got.cpu() - want).abs().max()) < 1e-4, (pred, t)
            if t > 0:       # the last step has a_prev = a_t: zero variance, eta changes nothing there
                assert float((want - det).abs().max()) > 1e-2      # the noise term is really there
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    steps, hw, eta = 5, 64, 0.5
    guide = SimpleGuide(enc, pipe.unet, 8.0, steps, enc.prompt('a photo of a turtle'))
    torch.manual_seed(21)
    pipe(guide=guide, init_size=(hw, hw), eta=eta, generator=torch.Generator('cpu').manual_seed(5), output_type='np')
    emb = clip_ref.text_hidden(sds['clip'], ccfg, tok('a photo of a turtle').input_ids)
    unc = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=torch.Generator('cpu').manual_seed(5))
    torch.manual_seed(21)
    lat, used = pipeline_ref.denoise(sds['unet'], ucfg, emb, unc, lat0, steps, 8.0, eta=eta,
                                     noise_fn=lambda shape: torch.randn(shape))
    lat_det, _ = pipeline_ref.denoise(sds['unet'], ucfg, emb, unc, lat0, steps, 8.0)
    assert used == [int(t) for t in pipe.scheduler.timesteps]
    p = pipeline_ref.psnr(pipe.last_images.cpu(), pipeline_ref.decode_image(sds['vae'], vcfg, lat))
    print(f'DDIM eta {eta}: PSNR {p:.1f} dB; latents moved {float((lat - lat_det).abs().max()):.3f} off the eta = 0 path')
    assert float((lat - lat_det).abs().max()) > 0.05
    assert p >= 40.0, p


def test_hip_graph_replay_matches_eager(mini, dev):
    """HIP-graph replay of the UNet forward -- the DEFAULT mode of a default-constructed FlexPipeline and the one bench.py
    measures -- gives bit-identical latents to the launch plan and to the eager front, also when the context tensor is
    replaced between calls (K/V are re-projected in place); no fallback happened on this box."""
    from flexdiffuse_amd import build
    sds, pipe, clip, tok, _ = mini
    fresh = build.build_models(sds, 'mini', dev)[0]
    assert fresh.use_graph is True and fresh.use_plan is True and fresh.graph_fallback is None
    assert pipe.use_graph is True
    try:
        _run_both(mini, dev, 3, 2, 8.0, 64)      # default construction: captures, then replays
        first = pipe.last_latents.clone()
        _run_both(mini, dev, 3, 2, 8.0, 64)      # replays the captured graph with a new context
        second = pipe.last_latents.clone()
        assert pipe.graph_fallback is None and pipe.use_graph and len(pipe._graphs) == 1
        pipe.use_graph = False                   # launch plan
        _run_both(mini, dev, 3, 2, 8.0, 64)
        plan = pipe.last_latents.clone()
        pipe.use_plan = False                    # eager front
        _run_both(mini, dev, 3, 2, 8.0, 64)
        assert torch.equal(first, second) and torch.equal(first, plan) and torch.equal(first, pipe.last_latents)
    finally:
        pipe.use_graph, pipe.use_plan = True, True


def test_planned_unet_under_generic_schedulers_equals_the_protocol_path(mini, dev):
    '''SimpleGuide with a scheduler other than plain DDIM (PNDM -- what the reference's Runner passes, utils.py:70 --, K-LMS,
    DDIM with eta): the UNet forward comes from the launch plan / HIP graph (`planned` in FlexPipeline.__call__) and only the
    scheduler arithmetic stays generic.  Bit-identical latents to the reference protocol path (`guide.noise_pred` +
    `scheduler.step`, plan and graph off), in both launch modes, float LMS timesteps included.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DDIMScheduler, LMSDiscreteScheduler, PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    keep = pipe.scheduler

    def run(sched, eta, seed):
        pipe.scheduler = sched
        g = SimpleGuide(enc, pipe.unet, 7.5, 5, enc.prompt(['a photo of a turtle', 'zeus, oil painting']))
        torch.manual_seed(3)        # DDIM eta > 0 draws its variance noise from the global CPU generator
        pipe(guide=g, init_size=(64, 64), eta=eta, generator=torch.Generator('cpu').manual_seed(seed), output_type='np')
        return pipe.last_latents.clone()
    try:
        for make, eta in ((PNDMScheduler, 0.0), (LMSDiscreteScheduler, 0.0), (DDIMScheduler, 0.5)):
            pipe.use_plan, pipe.use_graph = False, False
            want = run(make(), eta, 11)
            pipe.use_plan, pipe.use_graph, pipe._plans = True, False, {}
            got_plan = run(make(), eta, 11)
            pipe.use_graph, pipe._graphs = True, {}
            got_graph = run(make(), eta, 11)
            assert torch.equal(want, got_plan), make.__name__
            assert torch.equal(want, got_graph), make.__name__
            assert float(want.abs().max()) > 0.1 and bool(torch.isfinite(want).all())
    finally:
        pipe.scheduler, pipe.use_plan, pipe.use_graph = keep, True, True


def test_launch_plan_replay_matches_eager_front(mini, dev):
    """Default launch mode: the UNet forward of the fused loop is replayed from its recorded launch
    plan (hip.Plan / fd_plan_*).  Bit-identical latents to the eager Python front, also when prompts,
    noise and step count change between calls (every input of the recorded launches lives in a
    buffer that is refreshed: a torch op missed by the recorder would replay stale data)."""
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)

    def run(prompts, seed, steps):
        g = SimpleGuide(enc, pipe.unet, 8.0, steps, enc.prompt(prompts))
        pipe(guide=g, init_size=(64, 64), generator=torch.Generator('cpu').manual_seed(seed), output_type='np')
        return pipe.last_latents.clone()
    cases = [(['a photo of a turtle', 'zeus, oil painting'], 1337, 3),
             (['a deer in a forest', 'neon city at night'], 7, 4),
             (['a photo of a turtle', 'zeus, oil painting'], 1337, 3)]
    try:
        pipe.use_graph, pipe.use_plan = False, False
        eager = [run(*c) for c in cases]
        assert pipe.plan_launches() is None or True
        pipe.use_plan, pipe._plans = True, {}
        plan = [run(*c) for c in cases]
        n = pipe.plan_launches()
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert n is not None and n > 50, n
    for e, p in zip(eager, plan):
        assert torch.equal(e, p)
    assert not torch.equal(plan[0], plan[1]) and torch.equal(plan[0], plan[2])


def test_sd15_denoising_loop_determinism_soak(sd15, dev):
    '''20 passes of the headline request (SD1.5 512x512, 50 DDIM steps, CFG batch 16, HIP-graph replay = the product default and
    the mode bench.py times): 1000 CFG forwards = ~300 k launches of every counted-wait kernel of the forward (ping-pong /
    3-stage / persistent GEMM tiles, k_xattn, the split-K finish) must reproduce the first pass bit for bit, and one pass through
    the launch plan must give the same bits.  Round 5's missing phase-3 wait of the ping-pong loop (one launch in 25,000 read a
    stale LDS piece) fails here within a few passes; it was found by luck in a parity test (tools/soak_determinism.py is the
    265-pass form of this test).'''
    import bench
    from flexdiffuse_amd import Guide, SimpleGuide
    from flexdiffuse_amd import dist as fdist
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = sd15
    B, size, steps, passes = 8, 512, 50, 20
    emb = Guide(clip, tok, device='cuda').embeds(prompt=bench.synth_prompts(B), guide=bench.synth_image(2, 512, 512), **bench.GUIDANCE['linear'])
    enc = CLIPEncoder(clip, tok)
    noise = fdist.global_noise(B, (4, size // 8, size // 8), 1337)

    def one():
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb), init_size=(size, size), latents=noise, output_type='np')
        return pipe.last_latents.clone()
    assert pipe.use_graph
    ref = one()
    assert pipe.graph_fallback is None and bool(torch.isfinite(ref).all())
    differ = [i for i in range(1, passes) if not torch.equal(one(), ref)]
    assert not differ, f'graph-replay passes {differ} of {passes} differ from the first'
    try:
        pipe.use_graph = False
        assert torch.equal(one(), ref), 'the launch plan and the graph replay differ'
    finally:
        pipe.use_graph = True


def test_unet_producer_side_groupnorm_equals_separate_launches(sd15, dev):
    '''Full-size SD1.5 forward (CFG batch 16 at 64x64 latents, the bench's shape): the GroupNorms that read a split-K convolution's
    output -- a ResBlock's norm2 behind conv1, the next block's input norm behind conv2 / the downsample convolution, at the 16x16 and 8x8
    levels -- ride in that convolution's finish pass (fd_gemm_desc.gn_out, unet._res / _attn `xn`).  Same bits as with the GroupNorms
    launched on their own (ops.GN_FINISH_FUSE = False), 21 launches fewer.'''
    from flexdiffuse_amd import ops
    sds, pipe, clip, tok, _ = sd15
    g = torch.Generator().manual_seed(11)
    x = torch.randn((8, 4, 64, 64), generator=g).to(dev)
    ctx = torch.randn((16, 77, 768), generator=g).half().to(dev)
    n0 = ops.gn_fused_launches
    a = pipe.unet.forward_nhwc(x, 321, ctx, rep=2).clone()
    fused = ops.gn_fused_launches - n0
    ops.GN_FINISH_FUSE = False
    try:
        b = pipe.unet.forward_nhwc(x, 321, ctx, rep=2).clone()
        assert ops.gn_fused_launches - n0 == fused
    finally:
        ops.GN_FINISH_FUSE = True
    print(f'GroupNorms inside a split-K finish pass per forward: {fused}')
    assert fused >= 18, fused
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_unet_cfg_fanout_residuals_read_modulo_equal_the_replicas(sd15, dev):
    '''Full-size SD1.5 forward with the CFG fan-out (8 latents, 2 contexts): behind the shared prefix the hidden states and the block input are
    residuals only, read modulo the prefix's rows (fd_gemm_desc.residual_rows) instead of from replicas written by fd_repeat_rows_f16.
    Same bits as with the replicas (ops.RES_WRAP = False), two launches fewer.'''
    from flexdiffuse_amd import hip, ops
    sds, pipe, clip, tok, _ = sd15
    g = torch.Generator().manual_seed(12)
    x = torch.randn((8, 4, 64, 64), generator=g).to(dev)
    ctx = torch.randn((16, 77, 768), generator=g).half().to(dev)

    def run():
        plan = hip.Plan()
        with plan.record():
            out = pipe.unet.forward_nhwc(x, 321, ctx, rep=2).clone()
        return out, len(plan)
    assert ops.RES_WRAP
    pipe.unet.forward_nhwc(x, 321, ctx, rep=2)          # (the context's K / V^T projections happen once, outside the recorded forwards)
    a, na = run()
    ops.RES_WRAP = False
    try:
        b, nb = run()
    finally:
        ops.RES_WRAP = True
    print(f'recorded launches per forward: {na} with the residuals read modulo the prefix rows, {nb} with replicas')
    assert nb - na == 2, (na, nb)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_unet_conv_in_in_one_launch_against_the_gemm_path(sd15, dev):
    '''Full-size SD1.5 forward with the CFG fan-out: conv_in as ONE launch from the fp32 NCHW latents (fd_conv3x3_narrow_f16, replicas of the
    first skip tensor included) against layout change + explicit im2col + GEMM + fan-out copy (ops.CONV_IN_DIRECT = False): three launches
    fewer; the same fp16 products summed in another order, so the noise prediction agrees to the forward's fp16 noise, not bit for bit.'''
    from flexdiffuse_amd import hip, ops
    sds, pipe, clip, tok, _ = sd15
    g = torch.Generator().manual_seed(13)
    x = torch.randn((8, 4, 64, 64), generator=g).to(dev)
    ctx = torch.randn((16, 77, 768), generator=g).half().to(dev)
    pipe.unet.forward_nhwc(x, 321, ctx, rep=2)

    def run():
        plan = hip.Plan()
        with plan.record():
            out = pipe.unet.forward_nhwc(x, 321, ctx, rep=2).clone()
        return out, len(plan)
    assert ops.CONV_IN_DIRECT and pipe.unet.conv_in_nw is not None
    a, na = run()
    a2, _ = run()
    ops.CONV_IN_DIRECT = False
    try:
        b, nb = run()
    finally:
        ops.CONV_IN_DIRECT = True
    rel = float((a - b).abs().max() / b.abs().max())
    print(f'recorded launches per forward: {na} with conv_in in one launch, {nb} through the GEMM path; max |d eps| / max |eps| = {rel:.2e}')
    assert nb - na == 3, (na, nb)
    assert torch.equal(a, a2) and bool(torch.isfinite(a).all()) and rel < 5e-3, rel
    # the single-sample, no-fan-out call takes the same kernel
    c = pipe.unet.forward_nhwc(x[:1], 321, ctx[:1], rep=1)
    ops.CONV_IN_DIRECT = False
    try:
        d = pipe.unet.forward_nhwc(x[:1], 321, ctx[:1], rep=1)
    finally:
        ops.CONV_IN_DIRECT = True
    assert float((c - d).abs().max() / d.abs().max()) < 5e-3


def test_clip_towers_through_their_launch_plans(sd15, dev):
    '''The transformer stacks of the full-size CLIP ViT-L/14 towers run from launch plans (clip._PlannedEncoder: one library call per
    tower instead of ~360 trips through the Python front).  First call (records), replays, and the eager front (FD_CLIP_PLAN=0) give
    the same bits; a replay with other inputs gives other outputs (the plan really re-reads its input buffer).'''
    sds, pipe, clip, tok, _ = sd15
    g = torch.Generator().manual_seed(21)
    ids = [torch.randint(0, 49000, (8, 77), generator=g).to(dev) for _ in range(2)]
    px = [torch.randn((1, 3, 224, 224), generator=g).to(dev) for _ in range(2)]

    def towers(i):
        t = clip.text_model(ids[i])[0].clone()
        vm = clip.vision_model
        h = vm.post_layernorm(vm.encoder(vm.pre_layrnorm(vm.embeddings(px[i])))[0])
        return t, clip.visual_projection(h).clone()
    os.environ['FD_CLIP_PLAN'] = '0'
    try:
        want = [towers(0), towers(1)]
    finally:
        del os.environ['FD_CLIP_PLAN']
    clip.text_model._stack._plans.clear()
    clip.vision_model._stack._plans.clear()
    got = [towers(0), towers(1), towers(0), towers(1)]          # record, replay with other inputs, replays
    assert len(clip.text_model._stack._plans) == 1 and len(clip.vision_model._stack._plans) == 1
    for k, (t, v) in enumerate(got):
        assert torch.equal(t, want[k % 2][0]) and torch.equal(v, want[k % 2][1]), k
    assert not torch.equal(got[0][0], got[1][0]) and not torch.equal(got[0][1], got[1][1])


def test_launch_plan_full_size_unet_step(sd15, dev):
    """The recorded plan of the full-size SD1.5 UNet (CFG batch 2 x 2 at 64x64 latents: shared CFG
    prefix, in-place skip concats, LayerNorm-fold statistics, split-K deep levels) replays
    bit-identically to the eager front for new latents / timestep / context."""
    sds, pipe, clip, tok, _ = sd15
    g = torch.Generator().manual_seed(5)
    ctxs = [torch.randn((4, 77, 768), generator=g).half().to(dev) for _ in range(2)]
    lats = [torch.randn((2, 4, 64, 64), generator=g) for _ in range(2)]
    try:
        got, want, graph = [], [], []
        pipe.use_graph = False
        for use in (False, True):
            pipe.use_plan, pipe._plans = use, {}
            for i, t in enumerate((801, 401, 21)):
                lat = pipe.loop_latents(lats[i % 2])
                eps = pipe._unet_eps(lat, t, ctxs[i % 2], 2)
                (got if use else want).append(eps.clone())
        n = pipe.plan_launches()
        pipe.use_graph, pipe._graphs = True, {}          # the default mode: capture at the first call, replay after
        for i, t in enumerate((801, 401, 21)):
            lat = pipe.loop_latents(lats[i % 2])
            graph.append(pipe._unet_eps(lat, t, ctxs[i % 2], 2).clone())
        assert pipe.graph_fallback is None
    finally:
        pipe.use_plan, pipe.use_graph = True, True
    assert n > 200, n          # (308 entry-point calls in round 5; 245 after round 6's fusions)
    for a, b, c in zip(got, want, graph):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(got[0], got[1])


def _eps_ref(mini):
    from oracle import clip_ref, pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    emb = clip_ref.text_hidden(sds['clip'], ccfg, tok('a photo of a turtle').input_ids)
    unc = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    return lambda x, t: pipeline_ref.noise_pred(sds['unet'], ucfg, x, t, emb, unc, 8.0)


@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_pndm_and_lms_schedulers_vs_oracle(mini, dev, kind):
    '''the PLMS scheduler the reference's Runner actually passes
    (utils.py:70) and K-LMS incl. the pipeline's sigma scaling, vs the CPU oracle loops.'''
    from flexdiffuse_amd import FlexPipeline, LMSDiscreteScheduler, PNDMScheduler, SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import sched_ref
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    steps = 5        # a divisor of 1000: 0.3.0's arange-based tables are only regular then
    sched = PNDMScheduler() if kind == 'pndm' else LMSDiscreteScheduler()
    p2 = FlexPipeline(pipe.vae, clip, tok, pipe.unet, sched).to(dev)
    guide = SimpleGuide(enc, pipe.unet, 8.0, steps, enc.prompt('a photo of a turtle'))
    p2(guide=guide, init_size=(64, 64), generator=torch.Generator('cpu').manual_seed(3),
       output_type='np')
    lat0 = torch.randn((1, 4, 8, 8), generator=torch.Generator('cpu').manual_seed(3))
    if kind == 'pndm':
        want, used = sched_ref.pndm_loop(_eps_ref(mini), lat0, steps)
        assert used == [int(t) for t in sched.timesteps] and len(used) == steps + 1
    else:
        want, sigmas = sched_ref.lms_loop(_eps_ref(mini), lat0, steps)
        assert np.allclose(sigmas, sched.sigmas)
    e = relerr(p2.last_latents, want)
    print(f'{kind}: latent rel err {e:.4f}')
    assert e < 2e-2, e


def test_composite_guide_vs_oracle(mini, dev):
    '''CompositeGuide (one UNet batch over uncond/background/entities,
    rectangular latent blend, CFG) through the generic GuideBase protocol of the pipeline.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, sched_ref, unet_ref, ddim_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    schema = Schema('a forest at dawn', '', '', (0.0, 1.0),
                    [EntitySchema('a deer', (0, 16), (64, 48), 0.8),
                     EntitySchema('a red bird', (64, 0), (64, 64), 0.5)])
    steps = 3
    guide = CompositeGuide(enc, pipe.unet, 8.0, schema, steps)
    pipe(guide=guide, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(9),
         output_type='np')
    th = lambda p: clip_ref.text_hidden(sds['clip'], ccfg, tok(p).input_ids)
    ents = [(th(e.prompt), tuple(v // 8 for v in e.offset), tuple(v // 8 for v in e.size), e.blend)
            for e in schema.entities]
    x = torch.randn((1, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(9))
    acp = ddim_ref.alphas_cumprod()
    for t in ddim_ref.timesteps(steps):
        fn = lambda lat, emb: unet_ref.unet_forward(sds['unet'], ucfg, lat, int(t), emb)
        eps = sched_ref.composite_noise_pred(fn, x, th(''), th(schema.background_prompt), ents, 8.0)
        x = ddim_ref.ddim_step(eps, int(t), x, acp, steps)
    e = relerr(pipe.last_latents, x)
    print(f'composite: latent rel err {e:.4f}')
    assert e < 2e-2, e


def test_sd15_composite_guide_full_size_psnr(sd15, dev):
    '''CompositeGuide at FULL size (reference composition/guide.py:32-139 through utils.py:168-207's recipe): SD1.5,
    512x512, 20 DDIM steps, CFG 8, a background prompt and two entity boxes (one clipped by the canvas) -- every step one UNet batch over
    [uncond | background | entities], the region blend on the device (fd_region_blend_f32) and the CFG combine, through the generic
    GuideBase protocol of FlexPipeline -- against the CPU oracle's final latents cached by tests/golden/make_composite_oracle.py; final-image
    PSNR >= 40 dB, and the entity regions really differ from a background-only run.'''
    path = os.path.join(GOLDEN, 'composite_oracle.npz')
    if not os.path.exists(path):
        pytest.skip('tests/golden/composite_oracle.npz not generated')
    import hashlib
    import sys
    sys.path.insert(0, GOLDEN)
    from make_composite_oracle import COMPOSITE as c
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    o = np.load(path)
    enc = CLIPEncoder(clip, tok)
    schema = Schema(c['background'], '', '', (0.0, 1.0), [EntitySchema(p, off, size, blend) for p, off, size, blend in c['entities']])
    h = c['size'] // 8
    lat0 = torch.randn((1, 4, h, h), generator=torch.Generator('cpu').manual_seed(c['seed']))
    assert hashlib.sha256(lat0.numpy().tobytes()).digest() == o['noise_sha'].tobytes()
    guide = CompositeGuide(enc, pipe.unet, c['guidance'], schema, c['steps'])
    out = pipe(guide=guide, init_size=(c['size'], c['size']), generator=torch.Generator('cpu').manual_seed(c['seed']), output_type='np')
    assert [int(t) for t in o['timesteps']] == [int(t) for t in pipe.scheduler.timesteps]
    lat_ref = torch.from_numpy(o['latents'])
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    img_dev = pipe.last_images.cpu()
    p = pipeline_ref.psnr(img_dev, img_ref)
    # background only (no entities): the boxes must have changed the image
    pipe(guide=CompositeGuide(enc, pipe.unet, c['guidance'], Schema(c['background'], '', '', (0.0, 1.0), []), c['steps']),
         init_size=(c['size'], c['size']), generator=torch.Generator('cpu').manual_seed(c['seed']), output_type='np')
    moved = float((pipe.last_images.cpu() - img_dev).abs().mean())
    print(f'CompositeGuide at 512x512 ({len(c["entities"])} entities, {c["steps"]} steps): PSNR {p:.1f} dB; '
          f'entities moved the image by {moved:.4f}')
    assert out.images.shape == (1, c['size'], c['size'], 3) and float(img_ref.std()) > 0.02
    assert moved > 1e-3, 'the entity boxes changed nothing'
    assert p >= 40.0, p


def test_sd15_full_size_unet_properties(sd15, dev):
    """BASELINE configs[1] sizes (SD1.5 UNet, 64x64 latents, CFG batch 16): one sample checked
    against the CPU oracle, and size-independent properties on the whole batch -- sample
    independence (a sample's prediction does not depend on its batch mates, although the
    kernels pick different tiles / split-K for M = 65536 and M = 4096), CFG with g = 1 equals
    the conditional pass, DDIM with eps = 0 is a pure rescale."""
    from flexdiffuse_amd import ops
    from oracle import unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    g = torch.Generator().manual_seed(4)
    x = torch.randn((8, 4, 64, 64), generator=g)
    ctx = torch.randn((16, 77, 768), generator=g).half().float()
    xd, cd = x.to(dev), ctx.to(dev)
    eps = pipe.unet.forward_nhwc(xd, 500, cd, rep=2)                       # [16*4096][4]
    full = ops.nhwc_to_nchw(eps, 16, 4, 64, 64)
    alone = pipe.unet(xd[3:4], 500, encoder_hidden_states=cd[11:12]).sample  # sample 3, cond half
    assert relerr(alone, full[11:12]) < 1e-2
    want = unet_ref.unet_forward(sds['unet'], ucfg, x[3:4], 500, ctx[11:12])
    e = relerr(full[11:12], want)
    print(f'full-size UNet forward vs CPU oracle: rel err {e:.4f}')
    assert e < 3e-2
    # CFG combine with g = 1 returns the conditional half; eps = 0 DDIM step is a rescale
    out = torch.empty((8, 4, 64, 64), dtype=torch.float32, device=dev)
    ops.cfg_ddim_step(None, eps, 8, 4, 4096, True, 1.0, do_step=False, eps_out=out)
    assert torch.allclose(out, full[8:], rtol=1e-6, atol=1e-6)
    pipe.scheduler.set_timesteps(50)
    lat = xd.clone()
    zero = torch.zeros((8 * 4096, 4), dtype=torch.float32, device=dev)
    c = pipe.scheduler.step_coefficients(500)
    ops.cfg_ddim_step(lat, zero, 8, 4, 4096, False, 1.0, c[:4])
    acp = pipe.scheduler.alphas_cumprod
    assert torch.allclose(lat, xd * float(np.sqrt(acp[480] / acp[500])), rtol=1e-5, atol=1e-6)


def test_sd15_stress_weights_forward_and_loop_vs_oracle(sd15, dev):
    '''the end-to-end parity figures above run on synthetic weights that scale residual
    branches by 0.25 and have near-uniform softmax rows.  Here the full-size SD1.5 UNet gets `build.stress_unet_state_dict`:
    preset A (unit branch gain, q / k x 1.5, GroupNorm inputs with group means of ~10 sigma) and preset B (q / k x 4 ->
    logits x 16, the same group means) -- the strongest corners in which the fp32 oracle itself is still well-conditioned
    (tests/test_oracle_stress.py: beyond them a 2^-11 input perturbation moves the ORACLE's output by 80-100 %, which no fp16
    implementation can follow).  One full-size forward (64x64 latents) per preset vs oracle/unet_ref.py within 3 %, and the
    c1-size loop (256x256, 10 DDIM steps, CFG 8) on preset A vs the oracle loop, final-image PSNR stated and >= 40 dB.'''
    from flexdiffuse_amd import build, ops
    from flexdiffuse_amd.scheduler import DDIMScheduler
    from flexdiffuse_amd.unet import UNet2DConditionModel
    from oracle import pipeline_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    g = torch.Generator().manual_seed(12)
    x = torch.randn((1, 4, 64, 64), generator=g)
    ctx = torch.randn((2, 77, 768), generator=g).half().float()
    unets = {}
    for name, kw in (('A', dict(branch_gain=1.0, qk_gain=1.5, gn_shift=6.0)), ('B', dict(branch_gain=0.25, qk_gain=4.0, gn_shift=6.0))):
        sd = {k: v.half().float() for k, v in build.stress_unet_state_dict('sd15', seed=3, **kw).items()}
        unet = UNet2DConditionModel(sd, ucfg, dev)
        got = unet(x.to(dev), 500, encoder_hidden_states=ctx[1:2].to(dev)).sample
        want = unet_ref.unet_forward(sd, ucfg, x, 500, ctx[1:2])
        e = relerr(got, want)
        print(f'stress preset {name} {kw}: full-size UNet forward (64x64 latents) rel err {e:.4f}, |eps| max {float(want.abs().max()):.2f}')
        assert bool(torch.isfinite(got).all()) and e < 3e-2, (name, e)
        unets[name] = (sd, unet)
    # ---- preset C: preset A with conv_in x 300 -- the residual stream (and every skip connection) of the 64x64 level sits at
    # |max| ~1500, std ~290 in fp16 storage (trained checkpoints have such channels); the oracle stays well-conditioned there
    sdc = build.stress_unet_state_dict('sd15', seed=3, branch_gain=1.0, qk_gain=1.5, gn_shift=6.0)
    sdc['conv_in.weight'] = sdc['conv_in.weight'] * 300.0
    sdc = {k: v.half().float() for k, v in sdc.items()}
    xc = x[:, :, :32, :32].contiguous()
    got = UNet2DConditionModel(sdc, ucfg, dev)(xc.to(dev), 500, encoder_hidden_states=ctx[1:2].to(dev)).sample
    want = unet_ref.unet_forward(sdc, ucfg, xc, 500, ctx[1:2])
    e = relerr(got, want)
    print(f'stress preset C (A + conv_in x 300: residual stream |max| ~1500): UNet forward (32x32 latents) rel err {e:.4f}')
    assert bool(torch.isfinite(got).all()) and e < 3e-2, e
    # ---- c1-size loop on preset A (random context pair instead of CLIP outputs: the text tower is not under test)
    sd, unet = unets['A']
    steps, guidance, hw = 10, 8.0, 256
    emb, unc = ctx[1:2], ctx[0:1]
    lat0 = torch.randn((1, 4, hw // 8, hw // 8), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref, used = pipeline_ref.denoise(sd, ucfg, emb, unc, lat0, steps, guidance)
    sched = DDIMScheduler()
    sched.set_timesteps(steps)
    assert used == [int(t) for t in sched.timesteps]
    lat = lat0.to(dev).clone()
    cd = torch.cat([unc, emb]).to(dev)
    for t in sched.timesteps:
        eps = unet.forward_nhwc(lat, int(t), cd, rep=2)
        ops.cfg_ddim_step(lat, eps, 1, 4, (hw // 8) ** 2, True, guidance, sched.step_coefficients(int(t))[:4])
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    img = pipeline_ref.decode_image(sds['vae'], vcfg, lat.cpu())
    p = pipeline_ref.psnr(img, img_ref)
    print(f'stress preset A, c1-size loop (256x256, 10 DDIM steps, CFG 8): latent rel err {relerr(lat, lat_ref):.4f}, '
          f'PSNR {p:.1f} dB, image std {float(img_ref.std()):.3f}, |latent| max {float(lat_ref.abs().max()):.1f}')
    assert bool(torch.isfinite(lat).all())
    assert p >= 40.0, p


def test_sd21_c5_size_unet_properties(dev):
    """BASELINE configs[4] sizes: SD2.1-style UNet (context 1024, head dim 64, linear
    projections, v-prediction) at 96x96 latents (768x768 images), CFG pair of 2 samples.
    No reference behaviour exists for this config (the reference hard-codes SD-v1-4), so the
    target is the CPU oracle on one sample plus sample independence at 9216 tokens."""
    from flexdiffuse_amd import build, ops
    from flexdiffuse_amd.unet import UNet2DConditionModel
    from oracle import unet_ref
    sds = build.synthetic_state_dicts('sd21', seed=0, parts=('unet',))
    ucfg, _, _ = build.configs('sd21')
    unet = UNet2DConditionModel(sds['unet'], ucfg, dev)
    g = torch.Generator().manual_seed(9)
    x = torch.randn((2, 4, 96, 96), generator=g)
    ctx = torch.randn((4, 77, 1024), generator=g).half().float()
    xd, cd = x.to(dev), ctx.to(dev)
    eps = unet.forward_nhwc(xd, 321, cd, rep=2)
    full = ops.nhwc_to_nchw(eps, 4, 4, 96, 96)
    assert bool(torch.isfinite(full).all())
    alone = unet(xd[1:2], 321, encoder_hidden_states=cd[3:4]).sample      # sample 1, cond half
    assert relerr(alone, full[3:4]) < 1e-2
    want = unet_ref.unet_forward(sds['unet'], ucfg, x[1:2], 321, ctx[3:4])
    e = relerr(full[3:4], want)
    print(f'SD2.1-size UNet forward (96x96) vs CPU oracle: rel err {e:.4f}')
    assert e < 3e-2


def test_sd15_c4_size_img2img_properties(dev):
    """BASELINE configs[3]: SD1.5 img2img + image-guidance combo at 768x768 (96x96 latents), batch 4
    per GPU, 50 DDIM steps, strength 0.6 => 30 UNet evaluations from timesteps[20:]
    (pipeline/flex.py:193-221), embeddings from Guide.embeds with a guide image (Linear).  Too
    large for the CPU oracle; checked through size-independent properties: the executed timestep
    list, output range / shape, bit-identical reruns from the same generator, and that both the
    prompts and the guide image change the result."""
    from flexdiffuse_amd import Guide, SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from test_oracle_clip import synth_image
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=True)
    enc = CLIPEncoder(clip, tok)
    g = torch.Generator().manual_seed(6)
    image = (torch.rand((1, 3, 768, 768), generator=g) * 2 - 1)
    prompts = ['a castle on a hill', 'a bowl of fruit', 'a red fox in snow', 'a city street at night']
    guide = Guide(clip, tok, device='cuda')
    kw = dict(guide_threshold_mult=0.0, guide_clustered=0.0, guide_linear=(0.0, 0.5), guide_max_guidance=0.5)
    emb = guide.embeds(prompt=prompts, guide=synth_image(2, 512, 512), **kw)
    emb_plain = guide.embeds(prompt=prompts)
    assert emb.shape == (4, 77, 768) and float((emb - emb_plain).abs().max()) > 0.1   # the guide acted
    seen = []
    inner = pipe._unet_eps          # the loop's one UNet call (replayed from the launch plan)

    def spy(latents, t, ctx, rep):
        seen.append(int(t))
        return inner(latents, t, ctx, rep)
    pipe._unet_eps = spy
    try:
        outs = []
        for _ in range(2):
            out = pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 50, emb), init_image=image, strength=0.6,
                       generator=torch.Generator('cpu').manual_seed(3), output_type='np')
            outs.append(np.asarray(out.images))
        plain = pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 50, emb_plain), init_image=image, strength=0.6,
                     generator=torch.Generator('cpu').manual_seed(3), output_type='np')
    finally:
        del pipe._unet_eps
    want_t = [int(t) for t in pipe.scheduler.timesteps[20:]]
    assert len(want_t) == 30 and seen == want_t * 3
    assert outs[0].shape == (4, 768, 768, 3)
    assert np.isfinite(outs[0]).all() and outs[0].min() >= 0.0 and outs[0].max() <= 1.0
    assert np.array_equal(outs[0], outs[1])           # deterministic kernels, same generator
    assert float(np.abs(outs[0][0] - outs[0][1]).mean()) > 1e-3   # the prompts differ
    assert float(np.abs(outs[0] - np.asarray(plain.images)).mean()) > 1e-4   # the guide image matters


# ---- the reference's own back-half code, replayed on the device -------------------------------
class _ReplayUNet():
    '''Stub with the surface the product guides use (`forward_nhwc`): checks it is called with the
    latents / embedding stack the REFERENCE passed to its UNet (tests/golden/backhalf_goldens.npz)
    and returns the recorded UNet output as NHWC fp32.'''

    def __init__(self, g, key, dev):
        self.lat = torch.from_numpy(g[key + '/unet_latents'])
        self.ctx = torch.from_numpy(g[key + '/unet_ctx'])
        out = torch.from_numpy(g[key + '/unet_out'])
        self.out = out.permute(0, 2, 3, 1).reshape(-1, out.shape[1]).contiguous().to(dev)
        self.calls = 0

    def forward_nhwc(self, latents, step, ctx, rep=1):
        assert torch.equal(torch.cat([latents.cpu()] * rep), self.lat)
        assert torch.equal(ctx.float().cpu(), self.ctx), 'embedding stack ordered differently'
        self.calls += 1
        return self.out


class _StubEncoder():
    def __init__(self, dev):
        self.dev = dev

    def prompt(self, p):
        from test_oracle_backhalf import stub_embed
        ps = [p] if isinstance(p, str) else list(p)
        return torch.cat([stub_embed(s) for s in ps]).to(self.dev)


@pytest.mark.parametrize('name', ['cfg_b2', 'nocfg_b2', 'cfg_b1'])
def test_simple_guide_noise_pred_vs_reference_goldens(dev, name):
    '''Device SimpleGuide / PromptGuide.noise_pred (stack order + CFG combine kernel) against the
    reference's own pipeline/guide.py:46-64 run with a recording stub UNet.'''
    from flexdiffuse_amd import PromptGuide
    g = np.load(os.path.join(GOLDEN, 'backhalf_goldens.npz'))
    key = f'simple/{name}'
    unet = _ReplayUNet(g, key, dev)
    guide = PromptGuide(_StubEncoder(dev), unet, float(g[key + '/guidance'][0]), 10,
                        [str(p) for p in g[key + '/prompts']])
    assert guide.batch_size == len(g[key + '/prompts'])
    got = guide.noise_pred(torch.from_numpy(g[key + '/latents']).to(dev), int(g[key + '/step'][0]))
    want = torch.from_numpy(g[key + '/noise_pred'])
    assert unet.calls == 1 and got.shape == want.shape
    # u + g (t - u): the kernel may contract to an fma -> last-bit differences only
    assert float((got.cpu() - want).abs().max()) <= 2e-6 * float(want.abs().max()), name


def test_composite_guide_vs_reference_goldens(dev):
    '''Device CompositeGuide.noise_pred (region blend kernel with Python slice semantics --
    clipped and negative-offset boxes --, CFG) against the reference's own
    composition/guide.py:56-139 run with a recording stub UNet.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    g = np.load(os.path.join(GOLDEN, 'backhalf_goldens.npz'))
    for name in (str(n) for n in g['composite/names']):
        key = f'composite/{name}'
        ents = [EntitySchema(str(p), (int(e[0]), int(e[1])), (int(e[2]), int(e[3])), float(b))
                for e, b, p in zip(g[key + '/entities'], g[key + '/blend'], g[key + '/entity_prompts'])]
        schema = Schema(str(g['composite/background_prompt']), 'oil painting', 'photograph', (0.0, 1.0), ents)
        unet = _ReplayUNet(g, key, dev)
        guide = CompositeGuide(_StubEncoder(dev), unet, float(g[key + '/guidance'][0]), schema, 10)
        got = guide.noise_pred(torch.from_numpy(g[key + '/latents']).to(dev), 500)
        want = torch.from_numpy(g[key + '/noise_pred'])
        assert unet.calls == 1 and got.shape == want.shape, name
        assert float((got.cpu() - want).abs().max()) <= 2e-6 * float(want.abs().max()), name


def test_runner_compose(dev):
    '''utils.Runner.compose (reference utils.py:168-207): row parsing -> Schema -> CompositeGuide
    -> sequential batches through the generic guide protocol; reproducible from the seed and equal
    to driving CompositeGuide by hand.'''
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.composition import CompositeGuide
    r = Runner(preset='mini', device='cuda')
    rows = [['a deer', 0, 16, 64, 48, 0.8], ['', 0, 0, 8, 8, 0.5], ['bad', 'x', 0, 8, 8, 0.5],
            ['a red bird', 64, 0, 64, 64, 0.5]]
    imgs, grid = r.compose('a forest at dawn', rows, init_size=(128, 128), steps=3, batches=2, seed=9)
    assert len(imgs) == 2 and [e.prompt for e in r.last_schema.entities] == ['a deer', 'a red bird']
    again, _ = r.compose('a forest at dawn', rows, init_size=(128, 128), steps=3, batches=2, seed=9)
    assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(imgs, again))
    assert not np.array_equal(np.asarray(imgs[0]), np.asarray(imgs[1]))   # the generator advances
    guide = CompositeGuide(r.encoder, r.pipe.unet, 8.0, r.last_schema, 3)
    out = r.pipe(guide=guide, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(9))
    assert np.array_equal(np.asarray(out['sample'][0]), np.asarray(imgs[0]))


# ---- full-size towers / decoder and the c5 (OpenCLIP ViT-H) shapes ------------------------------
def test_vit_h_shaped_mini_towers_vs_oracle(dev):
    '''BASELINE configs[4]'s guide towers in miniature: OpenCLIP-style erf-GELU MLPs, vision
    head dim 80 (the non-prescaled k_attention_w8<96,5,false,false,1> path), text head dim 64, 2 layers each,
    against oracle.clip_ref on fp16-exact seeded weights.  Reference call sites:
    encode/clip.py:47-65 (prompt), :86-100 (image).'''
    from flexdiffuse_amd import weights as W
    from flexdiffuse_amd.clip import CLIPModel
    from flexdiffuse_amd.encode.clip import CLIPEncoder, clip_pixels, preprocess
    from flexdiffuse_amd.tokenizer import SyntheticTokenizer
    from oracle import clip_ref
    from test_oracle_clip import synth_image
    cfg = W.CLIPConfig(
        text=W.CLIPTextConfig(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                              num_attention_heads=2, hidden_act='gelu'),
        vision=W.CLIPVisionConfig(hidden_size=160, intermediate_size=320, num_hidden_layers=2,
                                  num_attention_heads=2, hidden_act='gelu'),
        projection_dim=128)
    sd = W.synth_state_dict(W.clip_param_shapes(cfg), seed=7, branch_gain=1.0)
    sd = {k: v.half().float() for k, v in sd.items()}
    clip = CLIPModel(sd, cfg, dev)
    tok = SyntheticTokenizer(vocab_size=512)
    enc = CLIPEncoder(clip, tok)
    img = synth_image(21, 900, 600)
    want = clip_ref.image_tokens(sd, cfg, clip_ref.clip_pixels(clip_ref.preprocess(img)))
    got = enc.image(img)
    assert got.shape == want.shape == (1, 257, 128)
    assert relerr(got, want) < 2e-2, relerr(got, want)
    for p in ('a photo of a turtle', ['zeus, oil painting', '']):
        want = clip_ref.text_hidden(sd, cfg, tok(p).input_ids)
        assert relerr(enc.prompt(p), want) < 2e-2


def test_sd15_full_size_vit_l14_and_vae_decode_vs_oracle(sd15, dev):
    '''The two full-size stages the bench runs but nothing else compares: the ViT-L/14 guide tower
    (257 x 1024, 24 layers; encode/clip.py:86-100) and the VAE decoder at 64x64 latents -> 512x512
    (pipeline/flex.py:112-124), each against the CPU fp32 oracle, 3 % of the output magnitude.'''
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from oracle import clip_ref, vae_ref
    from test_oracle_clip import synth_image
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    enc = CLIPEncoder(clip, tok)
    img = synth_image(2, 512, 512)
    want = clip_ref.image_tokens(sds['clip'], ccfg, clip_ref.clip_pixels(clip_ref.preprocess(img)))
    got = enc.image(img)
    e = relerr(got, want)
    print(f'full-size ViT-L/14 guide tokens vs CPU oracle: rel err {e:.4f}')
    assert got.shape == (1, 257, 768) and e < 3e-2
    z = torch.randn((1, 4, 64, 64), generator=torch.Generator().manual_seed(3))
    want = vae_ref.vae_decode(sds['vae'], vcfg, z)
    got = pipe.vae.decode(z.to(dev)).sample
    e = relerr(got, want)
    print(f'full-size VAE decode 64x64 -> 512x512 vs CPU oracle: rel err {e:.4f}')
    assert got.shape == (1, 3, 512, 512) and e < 3e-2


def test_sd21_c5_vit_h_guide_vs_oracle(dev):
    '''BASELINE configs[4] guide stage at full size: OpenCLIP ViT-H/14 vision tower (width 1280,
    32 layers, head dim 80, erf-GELU) + the 23-layer text tower (width 1024), Guide.embeds with
    the Linear image guidance vs oracle.guide_ref on the CPU.  The reference hard-codes CLIP-L
    (utils.py:24-25), so the oracle is the target here.'''
    from flexdiffuse_amd import Guide, build
    from flexdiffuse_amd.clip import CLIPModel
    from flexdiffuse_amd.tokenizer import SyntheticTokenizer
    from oracle import guide_ref
    from test_oracle_clip import synth_image
    sds = build.synthetic_state_dicts('sd21', seed=0, parts=('clip',))
    _, _, ccfg = build.configs('sd21')
    assert ccfg.vision.hidden_size == 1280 and ccfg.text.num_hidden_layers == 23
    clip = CLIPModel(sds['clip'], ccfg, dev)
    tok = SyntheticTokenizer(vocab_size=ccfg.text.vocab_size)
    img = synth_image(2, 512, 512)
    kw = dict(guide_threshold_mult=0.0, guide_clustered=0.0, guide_linear=(0.0, 0.5), guide_max_guidance=0.5)
    g = Guide(clip, tok, device='cuda')
    got = g.embeds(prompt='a castle on a hill at sunset', guide=img, **kw)
    ref = guide_ref.GuideRef(sds['clip'], ccfg, tok)
    want = ref.embeds(prompt='a castle on a hill at sunset', guide=img, **kw)
    e_img = relerr(g.encoder.image(img), ref.image(img))
    e = relerr(got, want)
    print(f'c5 ViT-H/14 guide: image tokens rel err {e_img:.4f}, guided embeddings rel err {e:.4f}')
    assert got.shape == (1, 77, 1024) and e_img < 3e-2 and e < 3e-2
    assert float((want - ref.prompt('a castle on a hill at sunset')).abs().max()) > 0.1   # guidance acted


def test_vae_decode_in_sample_chunks_and_large_gemm_fallback(mini, dev):
    '''Tensors past the 2 GiB reach of the LDS-DMA buffer descriptors: the VAE decodes a large
    batch in sample chunks (forced here with a tiny limit) with the same result as one pass, and
    fd_gemm_f16 re-dispatches an operand >= 2 GiB to the register-staged 4-wave kernel instead
    of failing.'''
    from flexdiffuse_amd import ops
    sds, pipe, clip, tok, _ = mini
    z = torch.randn((5, 4, 8, 8), generator=torch.Generator().manual_seed(4)).to(dev)
    whole = pipe.vae.decode(z).sample
    try:
        pipe.vae.decode_chunk_elems = 2 * 16 * 16 * 64        # two samples per chunk
        parts = pipe.vae.decode(z).sample
    finally:
        del pipe.vae.decode_chunk_elems
    assert parts.shape == whole.shape and relerr(parts, whole) < 2e-3
    # A of 2.1 GiB (M x K fp16): 16 waves / LDS-DMA cannot address it, the 4-wave kernel can
    M, K, N = 1 << 20, 1088, 64
    a = torch.empty((M, K), dtype=torch.float16, device=dev)
    a.normal_(generator=None)
    w = ops.prep_linear(torch.randn((N, K), generator=torch.Generator().manual_seed(1)) * 0.05, None, dev)
    out = ops.gemm(a, w)
    rows = torch.tensor([0, 12345, M // 2 + 7, M - 1], device=dev)
    want = a[rows].float() @ w.w[:, :K].float().t()
    assert float((out[rows].float() - want).abs().max()) < 2e-2 * float(want.abs().max())


def test_full_size_checkpoint_from_disk_equals_in_memory_build(sd15, dev, tmp_path):
    '''The from-disk path at FULL size (the oracle-checked from-disk test above runs at mini size): the 859.5 M-parameter
    UNet, the VAE and CLIP ViT-L/14 are written as fp32 safetensors in the diffusers / CLIPModel directory layout (5.5 GB, what
    CompVis/stable-diffusion-v1-4 + openai/clip-vit-large-patch14 look like on disk), read back through `FlexPipeline.from_pretrained` (reference
    utils.py:59-71), and the same request -- 256x256, 10 DDIM steps, CFG 8: BASELINE configs[0], whose in-memory build is oracle-checked by
    test_sd15_c1_pipeline_psnr -- must give the same images bit for bit; CLIP text and image features likewise.'''
    import json
    import shutil
    from safetensors.torch import save_file
    from flexdiffuse_amd import FlexPipeline, SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.tokenizer import CLIPBPETokenizer
    from test_oracle_clip import synth_image
    from test_tokenizer import toy_vocab
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = sd15
    sd_dir, clip_dir = tmp_path / 'stable-diffusion', tmp_path / 'clip'
    try:
        for sub in ('unet', 'vae', 'tokenizer'):
            os.makedirs(sd_dir / sub)
        os.makedirs(clip_dir)
        save_file({k: v.contiguous() for k, v in sds['unet'].items()}, str(sd_dir / 'unet' / 'diffusion_pytorch_model.safetensors'))
        save_file({k: v.contiguous() for k, v in sds['vae'].items()}, str(sd_dir / 'vae' / 'diffusion_pytorch_model.safetensors'))
        save_file({k: v.contiguous() for k, v in sds['clip'].items()}, str(clip_dir / 'model.safetensors'))
        on_disk = sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(tmp_path) for f in fs)
        assert on_disk > 4e9, on_disk
        vocab, merges = toy_vocab()
        (sd_dir / 'tokenizer' / 'vocab.json').write_text(json.dumps(vocab), encoding='utf-8')
        (sd_dir / 'tokenizer' / 'merges.txt').write_text('#version: 0.2\n' + '\n'.join(' '.join(m) for m in merges) + '\n', encoding='utf-8')
        p2, clip2, tok2 = build.from_directories(str(sd_dir), str(clip_dir), preset='sd15', device=dev, vae_encoder=False)
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
    assert isinstance(p2, FlexPipeline) and isinstance(tok2, CLIPBPETokenizer) and p2.tokenizer is tok2 and type(p2.scheduler).__name__ == 'DDIMScheduler'
    enc, enc2 = CLIPEncoder(clip, tok), CLIPEncoder(clip2, tok2)
    # CLIP from disk: same ids through both text towers, same pixels through both vision towers
    ids = tok('a photo of a turtle in a forest, oil painting').input_ids.to(dev)
    assert torch.equal(clip.text_model(ids)[0], clip2.text_model(ids)[0])
    img = synth_image(4, 224, 224)
    assert torch.equal(enc.image(img), enc2.image(img))
    # UNet + VAE from disk: the c1 request with the same embeddings and noise
    emb = enc.prompt('a photo of a turtle in a forest, oil painting')
    outs = []
    for pp_, e_ in ((pipe, enc), (p2, enc)):
        pp_(guide=SimpleGuide(e_, pp_.unet, 8.0, 10, emb), init_size=(256, 256), generator=torch.Generator('cpu').manual_seed(1337), output_type='np')
        outs.append((pp_.last_latents.clone(), pp_.last_images.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1].float().std()) > 0.02
