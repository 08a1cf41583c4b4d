'''Tiled VAE decode and encode on the device (mini preset, f = 2): AutoencoderKL.decode_image / encode_moments against the fp32
restatement of the blend applied on the CPU to their own tile batches (bit for bit) and to the CPU oracle's tiles (PSNR); the
one-tile and disabled forms; the pipeline, the Runner and img2img; and one full-size SD decode past the untiled limit.'''
import numpy as np
import pytest
import torch

import tile_ref as R

pytestmark = pytest.mark.gpu

TILING = dict(tile=8, stride=6)              # latent cells: feather 2
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
WIDE = dict(window=64, stride=32)            # the sampler's windows: 8 cells, stride 4


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
    assert pipe.vae.tiling is None
    return sds, pipe, clip, tok, build.configs('mini')


@pytest.fixture()
def vae(mini):
    '''The mini VAE with the test tiling on; off again afterwards, whatever the test did.'''
    v = mini[1].vae
    v.enable_tiling(**TILING)
    yield v
    v.disable_tiling()


def rows(t):
    '''NCHW tile batch -> NHWC rows [n h w][C].'''
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def grid6(g):
    return g.args[:6]


def psnr(got, want, peak=1.0):
    '''min over the batch of 10 log10(peak^2 / MSE).'''
    mse = ((got.double() - want.double()) ** 2).flatten(1).mean(dim=1).clamp_min(1e-20)
    return float((10.0 * torch.log10(peak ** 2 / mse)).min())


def latents(shape, seed=3):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def image(shape, seed=5):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1).half().float()


# ---- decode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,grid_n', [((2, 4, 8, 22), (1, 4)), ((1, 4, 14, 22), (2, 4))])
def test_tiled_decode_vs_own_tiles_and_oracle(mini, vae, dev, shape, grid_n):
    from flexdiffuse_amd import ops
    from oracle import vae_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    B, L, h, w = shape
    z = latents(shape)
    g = vae.tile_grid(h, w)
    assert (g.ny, g.nx) == grid_n and (g.h, g.w) == (8, 8)
    gp, fp = g.scaled(2), vae.tiling.feather_of(2)
    assert fp == (4, 4)
    tiles = torch.empty((B * g.count, L, 8, 8), dtype=torch.float32, device=dev)
    ops.window_gather(z.to(dev), tiles, B, L, g.args)
    assert torch.equal(tiles.cpu(), torch.cat([torch.stack([z[b, :, oy:oy + 8, ox:ox + 8] for oy, ox in g.offsets()])
                                               for b in range(B)]))
    for scale, a, b, clamp in ((1.0, 1.0, 0.0, False), (1.0 / 0.18215, 0.5, 0.5, True)):
        got = vae.decode_image(z.to(dev), scale, a, b, clamp).cpu()
        assert got.shape == (B, 3, 2 * h, 2 * w) and bool(torch.isfinite(got).all())
        # (a) the same gather, the same batch: the same kernels on the same tiles, blended by the restatement
        own = vae.decode_nhwc(tiles, scale)
        assert (own.B, own.H, own.W) == (B * g.count, 16, 16)
        ld = own.t.stride(0)
        want = R.blend_ref(own.t.cpu(), B, 3, ld, grid6(gp), fp, a, b, clamp)
        assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(vae.decode(z.to(dev)).sample.cpu(), vae.decode_image(z.to(dev)).cpu())
    # (b) the oracle's decode of every gathered tile, blended by the restatement, as images in [0, 1]
    ref_tiles = vae_ref.vae_decode(sds['vae'], vcfg, tiles.cpu() / 0.18215)
    ref = R.blend_ref(rows(ref_tiles), B, 3, 3, grid6(gp), fp, 0.5, 0.5, True)
    p = psnr(got, ref)
    print(f'tiled decode {shape} ({g.ny} x {g.nx} tiles): PSNR {p:.1f} dB vs the blended oracle tiles')
    assert p >= 40.0, p


# ---- encode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,grid_n', [((2, 3, 16, 44), (1, 4)), ((1, 3, 28, 44), (2, 4))])
def test_tiled_encode_vs_own_tiles_and_oracle(mini, vae, dev, shape, grid_n):
    '''The blended mean and the logvar before its clamp.  The moments are no image: their PSNR takes the range of the
    reference's values as the peak.'''
    from flexdiffuse_amd import ops
    from oracle import vae_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    B, _, H, W = shape
    x = image(shape)
    g = vae.tile_grid(H // 2, W // 2)
    assert (g.ny, g.nx) == grid_n
    gp = g.scaled(2)
    tiles = torch.empty((B * g.count, 3, 16, 16), dtype=torch.float32, device=dev)
    ops.window_gather(x.to(dev), tiles, B, 3, gp.args)
    got = vae.encode_moments(x.to(dev)).cpu()
    assert got.shape == (B, 8, H // 2, W // 2) and bool(torch.isfinite(got).all())
    own = vae.encode_moments_nhwc(tiles)
    assert (own.B, own.H, own.W) == (B * g.count, 8, 8) and own.t.shape[1] == own.t.stride(0) == 8
    want = R.blend_ref(own.t.cpu(), B, 8, 8, grid6(g), vae.tiling.feather_of())
    assert torch.equal(got, want), float((got - want).abs().max())
    dist = vae.encode(x.to(dev)).latent_dist
    assert torch.equal(dist.mean.cpu(), got[:, :4]) and torch.equal(dist.logvar.cpu(), got[:, 4:].clamp(-30.0, 20.0))
    mean, logvar = vae_ref.vae_encode_moments(sds['vae'], vcfg, tiles.cpu())
    assert float(logvar.min()) > -30.0 and float(logvar.max()) < 20.0          # the oracle's clamp is idle: pre-clamp values
    ref = R.blend_ref(rows(torch.cat([mean, logvar], dim=1)), B, 8, 8, grid6(g), vae.tiling.feather_of())
    for name, sl in (('mean', slice(0, 4)), ('logvar', slice(4, 8))):
        peak = float(ref[:, sl].max() - ref[:, sl].min())
        p = psnr(got[:, sl], ref[:, sl], peak)
        print(f'tiled encode {shape}: {name} PSNR {p:.1f} dB (peak {peak:.3f}) vs the blended oracle tiles')
        assert p >= 40.0, (name, p)


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_one_tile_and_disable_restore_the_untiled_bits(mini, dev):
    vae = mini[1].vae
    small, wide = latents((2, 4, 8, 8)).to(dev), latents((2, 4, 8, 22)).to(dev)
    img = image((1, 3, 16, 16)).to(dev)
    assert vae.tiling is None
    base_small, base_wide, base_mom = vae.decode_image(small, 2.0, 0.5, 0.5, True), vae.decode_image(wide), vae.encode_moments(img)
    vae.enable_tiling(**TILING)
    try:
        assert vae.tile_grid(8, 8) is None
        assert torch.equal(vae.decode_image(small, 2.0, 0.5, 0.5, True), base_small)
        assert torch.equal(vae.encode_moments(img), base_mom)
        tiled = vae.decode_image(wide)
        assert tiled.shape == base_wide.shape and not torch.equal(tiled, base_wide)      # tiling is an approximation
    finally:
        vae.disable_tiling()
    assert torch.equal(vae.decode_image(wide), base_wide)
    assert torch.equal(vae.decode(wide).sample, base_wide)


# ---- pipeline, Runner, img2img -------------------------------------------------------------------------------------------
def test_pipeline_decodes_through_the_tiles(mini, dev):
    '''A WindowedGuide request on a canvas of 8 x 22 cells (16 x 44 pixels under the mini VAE): the images are decode_image
    of the final latents, and the latents are those of the same request with tiling off -- the loop is untouched.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(PROMPTS)
    lat0 = latents((2, 4, 8, 22), seed=21)

    def run():
        out = pipe(guide=WindowedGuide(enc, pipe.unet, 8.0, 3, emb, **WIDE), init_size=(64, 176), latents=lat0, output_type='np')
        return pipe.last_latents.clone(), pipe.last_images.clone(), out.images
    off_lat, off_img, _ = run()
    pipe.enable_vae_tiling(**TILING)
    try:
        assert pipe.vae.tiling is not None
        lat, img, arr = run()
        want = pipe.vae.decode_image(lat, 1.0 / VAE_SCALE, 0.5, 0.5, True)
    finally:
        pipe.disable_vae_tiling()
    assert pipe.vae.tiling is None
    assert torch.equal(lat, off_lat)
    assert img.shape == (2, 3, 16, 44) and torch.equal(img, want) and not torch.equal(img, off_img)
    assert arr.shape == (2, 16, 44, 3) and np.array_equal(arr, img.cpu().permute(0, 2, 3, 1).numpy())


def test_runner_vae_tiling(dev):
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    r = Runner(preset='mini', device='cuda')
    assert r.vae_tiling is None
    kw = dict(size=(64, 176), window=64, stride=32, steps=3, seed=7)
    plain, _ = r.gen_wide('a photo of a turtle', **kw)
    assert r.pipe.vae.tiling is None
    r.vae_tiling = (8, 6)
    imgs, _ = r.gen_wide('a photo of a turtle', **kw)
    t = r.pipe.vae.tiling
    assert (t.tile, t.stride, t.feather) == ((8, 8), (6, 6), (2, 2))
    assert r.pipe.last_latents.shape == (1, 4, 8, 22) and tuple(r.pipe.last_images.shape) == (1, 3, 16, 44)
    assert len(imgs) == 1 and np.asarray(imgs[0]).shape == (16, 44, 3)
    assert torch.equal(r.pipe.last_images, r.pipe.vae.decode_image(r.pipe.last_latents, 1.0 / VAE_SCALE, 0.5, 0.5, True))
    again, _ = r.gen_wide('a photo of a turtle', **kw)
    assert np.array_equal(np.asarray(imgs[0]), np.asarray(again[0]))
    tiled_float = r.pipe.last_images.clone()
    r.vae_tiling = (8, 6, 1)                                                    # the feather reaches the VAE
    r.gen_wide('a photo of a turtle', **kw)
    assert r.pipe.vae.tiling.feather == (1, 1) and not torch.equal(r.pipe.last_images, tiled_float)
    r.vae_tiling = True
    small, _ = r.gen('a photo of a turtle', init_size=(64, 64), steps=2, seed=7)
    assert r.pipe.vae.tiling.tile == (64, 64) and np.asarray(small[0]).shape == (16, 16, 3)
    r.vae_tiling = None
    back, _ = r.gen_wide('a photo of a turtle', **kw)
    assert r.pipe.vae.tiling is None and np.array_equal(np.asarray(back[0]), np.asarray(plain[0]))


def test_img2img_encodes_through_the_tiles(mini, dev):
    '''init_image + mask_image of canvas size (16 x 44 pixels, 8 x 22 cells): the kept region ends on the clean init latents,
    and those are a direct tiled encode(...).latent_dist.sample with the same generator -- not the untiled one.'''
    from flexdiffuse_amd import WindowedGuide, ops
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(PROMPTS)
    img = image((1, 3, 16, 44))
    mask = np.zeros((16, 44), np.float32)
    mask[:, 22:] = 1.0                                                          # repaint the right part; cells 0..10 are kept

    def sample():
        z = pipe.vae.encode(img.to(dev)).latent_dist.sample(generator=torch.Generator('cpu').manual_seed(11))
        return torch.cat([ops.axpby(z, None, VAE_SCALE, 0.0)] * 2)
    untiled = sample()
    pipe.enable_vae_tiling(**TILING)
    try:
        pipe(guide=WindowedGuide(enc, pipe.unet, 8.0, 5, emb, **WIDE), init_image=img, mask_image=mask, strength=0.8,
             generator=torch.Generator('cpu').manual_seed(11), output_type='np')
        got, dec = pipe.last_latents.clone(), pipe.last_images.clone()
        z0 = sample()
    finally:
        pipe.disable_vae_tiling()
    assert got.shape == (2, 4, 8, 22) and bool(torch.isfinite(got).all()) and dec.shape == (2, 3, 16, 44)
    assert torch.equal(got[:, :, :, :11], z0[:, :, :, :11])
    assert not torch.equal(z0[:, :, :, :11], untiled[:, :, :, :11])
    assert float((got[:, :, :, 11:] - z0[:, :, :, 11:]).abs().max()) > 0.05


# ---- full size -----------------------------------------------------------------------------------------------------------
def test_sd_full_size_tiled_decode(dev):
    '''1024 x 2048, the smallest canvas whose untiled score matrix reaches 2 GiB (never decoded untiled here): 3 x 5 tiles of
    the tuned 64 x 64-latent shape in one decode_nhwc batch, one blend launch, bit-equal to the restatement on its own
    tiles.'''
    from flexdiffuse_amd import build, ops
    from flexdiffuse_amd.vae import AutoencoderKL
    from flexdiffuse_amd.weights import SD_VAE
    sd = build.synthetic_state_dicts('sd15', seed=0, parts=('vae',))['vae']
    vae = AutoencoderKL(sd, SD_VAE, dev, encoder=False)
    assert vae.scale_factor == 8 and vae.tiling is None
    vae.enable_tiling()
    z = latents((1, 4, 128, 256), seed=17).to(dev)
    g = vae.tile_grid(128, 256)
    assert g.args == (128, 256, 64, 64, 48, 48, 3, 5)
    got = vae.decode_image(z, 1.0 / 0.18215, 0.5, 0.5, True)
    assert got.shape == (1, 3, 1024, 2048) and bool(torch.isfinite(got).all())
    tiles = torch.empty((15, 4, 64, 64), dtype=torch.float32, device=dev)
    ops.window_gather(z, tiles, 1, 4, g.args)
    own = vae.decode_nhwc(tiles, 1.0 / 0.18215)
    assert (own.B, own.H, own.W) == (15, 512, 512)
    want = R.blend_ref(own.t.cpu(), 1, 3, own.t.stride(0), grid6(g.scaled(8)), (128, 128), 0.5, 0.5, True)
    got = got.cpu()
    assert torch.equal(got, want), float((got - want).abs().max())
    assert float(got.std()) > 1e-3                                              # an image, not a constant
