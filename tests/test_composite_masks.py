'''Batched, soft-masked region composition -- the host side (no GPU): the optional entity mask of
the schema, the latent weight maps CompositeGuide builds from it, the context order of a batched
guide, and a restatement of batched masked composition that reduces bit-exactly to the pinned
oracle (oracle/sched_ref.composite_noise_pred) for one sample with rectangles.'''
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
from flexdiffuse_amd.composition.guide import EntityEmbeds, weight_maps
from oracle import sched_ref


# ---- restatements (fp32 torch) ---------------------------------------------------------------------------------------
def ref_weights(entities, H, W):
    '''[n][H][W]: blend * avg_pool2d(mask, 8) (or blend) written through plain Python slicing of the latent canvas.'''
    out = torch.zeros((len(entities), H, W), dtype=torch.float32)
    for k, (_, (ow, oh), (sw, sh), blend, mask) in enumerate(entities):
        b = torch.tensor(blend, dtype=torch.float32)
        cells = b.expand(sh, sw) if mask is None else \
            b * F.avg_pool2d(torch.as_tensor(mask, dtype=torch.float32)[None, None], 8)[0, 0]
        region = out[k, oh:oh + sh, ow:ow + sw]
        region.copy_(cells[:region.shape[0], :region.shape[1]])
    return out


def composite_ref(unet_fn, latents, uncond, bg, entities, guidance):
    '''Batched composition: one UNet batch over E blocks of B rows ([uncond]*B [bg]*B [e_1]*B ...), per sample
    v = bg; v += w_k (e_k - v) where w_k != 0; CFG u + g (v - u).  entities: [(embed, (ow,oh), (sw,sh), blend, mask)].'''
    B, C, H, W = latents.shape
    cfg = guidance > 1.0
    blocks = ([uncond] if cfg else []) + [bg] + [e[0] for e in entities]
    E = len(blocks)
    emb = torch.cat([b.expand(B, -1, -1) for b in blocks])
    out = unet_fn(torch.cat([latents] * E), emb).view(E, B, C, H, W)
    stack = out[1:] if cfg else out
    v = stack[0].clone()
    wm = ref_weights(entities, H, W)
    for k in range(len(entities)):
        w = wm[k]
        v = torch.where(w != 0, v + w * (stack[1 + k] - v), v)
    if cfg:
        g = torch.tensor(guidance, dtype=torch.float32)
        return out[0] + g * (v - out[0])
    return v


def stub_unet(lat, emb):
    '''Deterministic stand-in for the UNet: each row depends on its latents and its context row.'''
    s = emb[:, :3, :8].sum(dim=(1, 2)).view(-1, 1, 1, 1)
    return torch.sin(lat * s) + 0.25 * emb[:, 0, :lat.shape[1], None, None]


# ---- schema ----------------------------------------------------------------------------------------------------------
def test_mask_validation():
    ok = np.full((16, 24), 0.5, dtype=np.float32)
    e = EntitySchema('a deer', (8, 0), (24, 16), 0.7, ok)
    assert e.mask.dtype == np.float32 and e.mask.shape == (16, 24)
    with pytest.raises(ValueError):
        EntitySchema('a deer', (8, 0), (24, 16), 0.7, np.zeros((24, 16)))          # (width, height): transposed
    with pytest.raises(ValueError):
        EntitySchema('a deer', (8, 0), (24, 16), 0.7, np.zeros((16,)))
    bad = ok.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        EntitySchema('a deer', (8, 0), (24, 16), 0.7, bad)
    for v in (-0.01, 1.01):
        bad = ok.copy()
        bad[0, 0] = v
        with pytest.raises(ValueError):
            EntitySchema('a deer', (8, 0), (24, 16), 0.7, bad)
    # nested lists and CPU torch tensors are array-likes too
    lst = EntitySchema('x', (0, 0), (2, 3), 0.5, [[0, 1], [0.5, 0.25], [1, 1]]).mask
    ten = EntitySchema('x', (0, 0), (2, 3), 0.5, torch.tensor([[0, 1], [0.5, 0.25], [1, 1]])).mask
    assert np.array_equal(lst, ten) and lst.dtype == np.float32


def test_pil_mask_equals_array_mask():
    from PIL import Image
    a = np.random.default_rng(0).integers(0, 256, (16, 24), dtype=np.uint8)
    from_pil = EntitySchema('x', (0, 0), (24, 16), 0.5, Image.fromarray(a, 'L')).mask
    from_rgb = EntitySchema('x', (0, 0), (24, 16), 0.5, Image.fromarray(a, 'L').convert('RGB')).mask
    from_np = EntitySchema('x', (0, 0), (24, 16), 0.5, a.astype(np.float32) / np.float32(255)).mask
    assert np.array_equal(from_pil, from_np) and np.array_equal(from_rgb, from_np)


def test_positional_entities_and_json_unchanged_without_masks():
    e = EntitySchema('a deer', (0, 16), (64, 48), 0.8)
    assert e.mask is None and (e.prompt, e.offset, e.size, e.blend) == ('a deer', (0, 16), (64, 48), 0.8)
    assert EntitySchema('a', (0, 0), (8, 8)).blend == 0.8
    s = Schema('bg', 'a', 'b', (0.0, 1.0), [e, EntitySchema('a red bird', (64, 0), (64, 64), 0.5)])
    want = ('{"background_prompt": "bg", "style_start_prompt": "a", "style_end_prompt": "b", "style_blend": [0.0, 1.0], '
            '"entities": [{"prompt": "a deer", "offset": [0, 16], "size": [64, 48], "blend": 0.8}, '
            '{"prompt": "a red bird", "offset": [64, 0], "size": [64, 64], "blend": 0.5}]}')
    assert s.json() == want
    # equality never compares arrays
    m = np.ones((48, 64), dtype=np.float32)
    assert EntitySchema('a deer', (0, 16), (64, 48), 0.8, m) == e
    masked = Schema('bg', 'a', 'b', (0.0, 1.0), [EntitySchema('x', (0, 0), (2, 2), 0.5, [[0, 0.5], [1, 0.25]])])
    assert json.loads(masked.json())['entities'][0]['mask'] == [[0.0, 0.5], [1.0, 0.25]]


# ---- weight maps -----------------------------------------------------------------------------------------------------
def _entities(rng, H, W):
    def mask(w, h):
        m = rng.random((h, w)).astype(np.float32)
        m[m < 0.3] = 0.0                                   # partly zero
        return m
    boxes = [((8, 16), (64, 48), 0.8, True),               # interior
             ((80, 40), (64, 64), 0.5, True),              # clipped at the far edges
             ((-24, 8), (40, 32), 0.6, True),              # negative start: counts from the end of the axis
             ((-32, -16), (16, 8), 0.9, True),             # negative start that stays inside
             ((4, 12), (60, 44), 0.7, True),               # not multiples of 8
             ((16, 16), (48, 40), 0.3, False),             # rectangle, overlapping the first
             ((-8, 0), (24, 24), 0.4, False)]              # negative rectangle
    out = []
    for (ox, oy), (w, h), blend, masked in boxes:
        out.append(EntitySchema(f'e{len(out)}', (ox, oy), (w, h), blend, mask(w, h) if masked else None))
    return out


@pytest.mark.parametrize('H,W', [(12, 12), (16, 10), (9, 14)])
def test_weight_maps_vs_restatement(H, W):
    ents = _entities(np.random.default_rng(H * 100 + W), H, W)
    embeds = [EntityEmbeds(None, tuple(v // 8 for v in e.offset), tuple(v // 8 for v in e.size), e.blend, e.mask)
              for e in ents]
    got = weight_maps(embeds, H, W)
    want = ref_weights([(None, emb.offset_blocks, emb.size_blocks, e.blend, e.mask) for emb, e in zip(embeds, ents)], H, W)
    assert got.dtype == torch.float32 and got.shape == (len(ents), H, W)
    assert torch.equal(got, want)
    assert float(got.abs().sum()) > 0 and bool((got == 0).any())
    # a rectangle carries exactly fp32(blend) inside its box
    k = 5
    y0, x0 = embeds[k].offset_blocks[1], embeds[k].offset_blocks[0]
    assert float(got[k, y0, x0]) == float(np.float32(ents[k].blend))


# ---- batched guide context -------------------------------------------------------------------------------------------
class _Encoder():
    def prompt(self, p):
        g = torch.Generator().manual_seed(sum(map(ord, p)) + 7 * len(p))
        return torch.randn((1, 5, 16), generator=g)


@pytest.mark.parametrize('guidance', [8.0, 1.0])
def test_batched_context_is_rep_major(guidance):
    ents = [EntitySchema('a deer', (0, 0), (16, 16), 0.8), EntitySchema('a bird', (8, 8), (16, 16), 0.5)]
    enc = _Encoder()
    g = CompositeGuide(enc, None, guidance, Schema('forest', '', '', (0.0, 1.0), ents), 3, batch_size=3)
    blocks = ([''] if guidance > 1 else []) + ['forest', 'a deer', 'a bird']
    assert g.on_device and g.rep == len(blocks) and g.embed_tensor.shape == (3 * len(blocks), 5, 16)
    for r, p in enumerate(blocks):
        for b in range(3):
            assert torch.equal(g.embed_tensor[r * 3 + b], enc.prompt(p)[0])
    one = CompositeGuide(enc, None, guidance, Schema('forest', '', '', (0.0, 1.0), ents), 3)
    assert not one.on_device and one.rep == len(blocks)
    masked = [EntitySchema('a deer', (0, 0), (16, 16), 0.8, np.ones((16, 16)))]
    assert CompositeGuide(enc, None, guidance, Schema('forest', '', '', (0.0, 1.0), masked), 3).on_device
    with pytest.raises(ValueError):
        CompositeGuide(enc, None, guidance, Schema('forest', '', '', (0.0, 1.0), ents), 3, batch_size=0)


# ---- the restatement against the pinned oracle -----------------------------------------------------------------------
@pytest.mark.parametrize('guidance', [8.0, 1.0])
def test_restatement_reduces_to_pinned_oracle(guidance):
    '''B = 1, rectangles: bit-exact to sched_ref.composite_noise_pred (pinned on the reference's own CompositeGuide).'''
    rng = torch.Generator().manual_seed(5)
    H = W = 12
    lat = torch.randn((1, 4, H, W), generator=rng)
    emb = lambda: torch.randn((1, 5, 16), generator=rng)          # noqa: E731
    uncond, bg = emb(), emb()
    boxes = [((0, 2), (8, 6), 0.8), ((8, 0), (8, 8), 0.5), ((-3, 1), (2, 4), 0.6), ((3, 3), (4, 4), 0.3)]
    ents = [(emb(), off, size, blend) for off, size, blend in boxes]
    want = sched_ref.composite_noise_pred(stub_unet, lat, uncond, bg, ents, guidance)
    got = composite_ref(stub_unet, lat, uncond, bg, [e + (None,) for e in ents], guidance)
    assert torch.equal(got, want)


def test_restatement_rows_are_independent_samples():
    '''Row b of a batched (masked) composition equals the B = 1 composition of latents row b.'''
    rng = torch.Generator().manual_seed(6)
    H = W = 10
    lat = torch.randn((3, 4, H, W), generator=rng)
    emb = lambda: torch.randn((1, 5, 16), generator=rng)          # noqa: E731
    uncond, bg = emb(), emb()
    m = np.random.default_rng(1).random((48, 40)).astype(np.float32)
    ents = [(emb(), (1, 2), (5, 6), 0.8, m), (emb(), (6, 0), (8, 8), 0.5, None)]
    got = composite_ref(stub_unet, lat, uncond, bg, ents, 7.5)
    for b in range(3):
        assert torch.equal(got[b:b + 1], composite_ref(stub_unet, lat[b:b + 1], uncond, bg, ents, 7.5))
