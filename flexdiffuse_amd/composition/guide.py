'''Region-composited guidance -- host-side mirror of the reference's `CompositeGuide`
(composition/guide.py:32-139) and `encode_schema` (composition/embeds.py:28-44): ONE UNet
batch over [uncond, background, entity_1..n] on the same latents, each entity's noise
prediction blended onto the background inside its latent-space rectangle
(bg + blend * (entity - bg)), then classifier-free guidance against the unconditional row.

The reference runs only batch_size == 1 (it concatenates `latents` once per embedding row).
Beyond it: `batch_size = B > 1` (B independent compositions in ONE UNet forward over E*B rows,
context in rep-major order [uncond]*B [bg]*B [e_1]*B ...) and soft entity masks (weight
blend * mean of the mask's 8x8 pixel cell per latent cell).  Those requests blend, combine and (in
FlexPipeline's device loop) take the DDIM step in one launch, fd_composite_step_f32; batch 1 without
masks keeps the per-entity fd_region_blend_f32 chain in `noise_pred`.  FlexPipeline (`fuse_composite`, on by default) runs every
CompositeGuide, batch 1 included, on its device loop under every scheduler: the entity blend is the source of the guided
prediction inside the scheduler's own one-launch step (fd_composite_ddim_step_f32, fd_composite_multistep_step_f32,
fd_composite_linear_multistep_step_f32) -- `entity_rows` hands the schedulers the weight maps.  The style-blend embedding the reference
computes at composition/guide.py:114-121 is dead code there and is not evaluated here -- unless the
caller opts in with `style_linear=(l0, l1)`: every prompt block E then gets the two keyframes
E + omega (S_start - E) and E + omega (S_end - E), omega = linspace(l0, l1, tokens) per token (the reference's
Linear style guidance), and step j runs on their blend at s_j = b0 + progress_j (b1 - b0), (b0, b1) the
schema's `style_blend` -- a context schedule (ctx_schedule.py), on the batch-1 and on the device path.
'''
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from .. import hip, ops
from ..ctx_schedule import ContextSchedule, step_weights
from ..pipeline.guide import GuideBase, WindowedGuide
from .schema import EntitySchema, Schema


MAX_WINDOW_ENTITIES = 16          # FD_WINDOW_MAX_ENTITIES, csrc/window.hip


def px_to_block(px_shape: Sequence[int]) -> Tuple[int, ...]:
    return tuple(px // 8 for px in px_shape)


@dataclass
class EntityEmbeds():
    embed: torch.Tensor
    offset_blocks: Tuple[int, int]
    size_blocks: Tuple[int, int]
    blend: float
    mask: Optional[np.ndarray] = None


def box_slices(offset_blocks: Sequence[int], size_blocks: Sequence[int], H: int, W: int) -> Tuple[int, int, int, int]:
    '''(y0, y1, x0, x1) of an entity's latent box.  composition/guide.py:86-98 slices
    noise[:, :, oh:oh+sh, ow:ow+sw]: Python slice semantics -- a box past the canvas is clipped, a
    NEGATIVE start counts from the end of the axis (usually leaving an empty box, i.e. no blend at all).'''
    (ow, oh), (sw, sh) = offset_blocks, size_blocks
    y0, y1, _ = slice(oh, oh + sh).indices(H)
    x0, x1, _ = slice(ow, ow + sw).indices(W)
    return y0, y1, x0, x1


def weight_maps(entities: Sequence[EntityEmbeds], H: int, W: int) -> torch.Tensor:
    '''Dense fp32 [n][H][W] blend weights (CPU), 0 outside every box: fp32(blend) inside a rectangle;
    fp32(blend) * fp32(cell) with a mask, `cell` the mean of the mask's 8x8 image-pixel block (floor, as
    px_to_block).  The mask's top-left cell sits at the box's resolved origin; cells past the canvas are dropped.'''
    out = torch.zeros((len(entities), H, W), dtype=torch.float32)
    for k, e in enumerate(entities):
        y0, y1, x0, x1 = box_slices(e.offset_blocks, e.size_blocks, H, W)
        if y1 <= y0 or x1 <= x0:
            continue
        blend = torch.tensor(float(e.blend), dtype=torch.float32)
        if e.mask is None:
            out[k, y0:y1, x0:x1] = blend
        else:
            cell = F.avg_pool2d(torch.from_numpy(e.mask)[None, None], 8)[0, 0]
            out[k, y0:y1, x0:x1] = blend * cell[:y1 - y0, :x1 - x0]
    return out


class CompositeGuide(GuideBase):
    def __init__(self, encoder, unet, guidance: float, schema: Schema, steps: int,
                 batch_size: int = 1, style_linear: Optional[Tuple[float, float]] = None, mode: str = 'lerp'):
        GuideBase.__init__(self, encoder, unet, guidance, steps)
        if int(batch_size) < 1:
            raise ValueError(f'batch_size must be >= 1, got {batch_size}')
        self.schema = schema
        self.background_embed = encoder.prompt(schema.background_prompt)
        self.entities: List[EntityEmbeds] = [
            EntityEmbeds(encoder.prompt(e.prompt), px_to_block(e.offset), px_to_block(e.size),
                         e.blend, getattr(e, 'mask', None)) for e in schema.entities]
        self.batch_size = B = int(batch_size)
        self.classifier_free_guidance = self.guidance > 1.0
        # batched or masked requests: one fd_composite_step_f32 per step, on FlexPipeline's device loop
        self.on_device = B > 1 or any(e.mask is not None for e in self.entities)
        rows = [self.background_embed] + [e.embed for e in self.entities]
        if self.classifier_free_guidance:
            rows = [self.uncond_embeds] + rows
        self.rep = len(rows)                     # E: context blocks of B rows each
        # built once, rep-major: [uncond]*B, [bg]*B, [e_1]*B ... -- for B = 1 the reference's [uncond, bg, e_1, ...]
        self.embed_tensor = torch.cat([r.float().expand(B, -1, -1) for r in rows]).contiguous()
        self._wmaps = {}
        # opt-in style blend (None: the reference-pinned behaviour above -- the style prompts are encoded nowhere)
        self.context: Optional[ContextSchedule] = None
        if style_linear is not None:
            l0, l1 = (float(v) for v in style_linear)
            first = 1 if self.classifier_free_guidance else 0
            L = self.embed_tensor.shape[1]
            omega = torch.linspace(l0, l1, L, dtype=torch.float32, device=self.embed_tensor.device).view(1, L, 1)
            keys = []
            for prompt in (schema.style_start_prompt, schema.style_end_prompt):
                style = encoder.prompt(prompt).float().to(self.embed_tensor.device)
                key = self.embed_tensor.clone()
                body = key[first * B:]
                body += omega * (style - body)          # the unconditional block keeps its rows: equal in both keyframes
                keys.append(key)
            self.context = ContextSchedule(unet, keys, step_weights(steps, 2, schema.style_blend), mode)

    def stacked_embeds(self) -> torch.Tensor:
        return self.embed_tensor if self.context is None else self.context.handle()

    def at_step(self, j: int):
        '''FlexPipeline calls this with the global step index before every step; nothing without `style_linear`.'''
        if self.context is not None:
            self.context.at_step(j)

    def weights(self, H: int, W: int) -> Optional[torch.Tensor]:
        '''Device fp32 [n][H][W] blend weights (None without entities), built once per latent size and kept: a
        captured graph / recorded plan of the step reads this buffer.'''
        if not self.entities:
            return None
        w = self._wmaps.get((H, W))
        if w is None:
            w = weight_maps(self.entities, H, W).to(self.embed_tensor.device)
            self._wmaps[(H, W)] = w
        return w

    def entity_rows(self, H: int, W: int) -> torch.Tensor:
        '''`weights(H, W)` as the schedulers' `fused_step(entities=)` takes it: device fp32 [n][H W]; without entities an empty
        [0][H W] marker, which still selects the rep-major row count.'''
        w = self.weights(H, W)
        if w is None:
            return torch.empty((0, H * W), dtype=torch.float32, device=self.embed_tensor.device)
        return w.view(w.shape[0], H * W)

    def step(self, x: Optional[torch.Tensor], eps: torch.Tensor, coef=(0.0, 1.0, 1.0, 0.0), v_prediction: bool = False,
             eps_out: Optional[torch.Tensor] = None, mask=None, sigma: float = 0.0, step_noise=None):
        '''Blend + CFG of the UNet output `eps` (NHWC fp32, rep-major rows) into `eps_out` (NCHW fp32, optional) and,
        given `x` (NCHW fp32), the DDIM update of `x` in place: one launch.  With `x`, optionally in that launch
        (fd_composite_ddim_step_f32): `sigma` and `step_noise` = (PhiloxNoise, draw), the eta > 0 term sigma z at C H W
        elements per sample; `mask` = (z0, noise, mask [H W], k1, k2), the known-region blend of masked img2img.'''
        B, C, H, W = (x if x is not None else eps_out).shape
        assert not sigma or (x is not None and step_noise is not None), 'sigma needs the latents and a step_noise'
        if x is not None and (mask is not None or step_noise is not None):
            noise, draw = step_noise if step_noise is not None else (None, 0)
            ops.composite_ddim_step(x, eps, self.weights(H, W), B, C, H * W, self.classifier_free_guidance, self.guidance, coef,
                                    v_prediction, mask, float(sigma), noise, C * H * W, int(draw), eps_out)
            return
        ops.composite_step(x, eps, self.weights(H, W), B, C, H * W, self.classifier_free_guidance, self.guidance,
                           coef, v_prediction, do_step=x is not None, eps_out=eps_out)

    def noise_pred(self, latents: torch.Tensor, step) -> torch.Tensor:
        E = self.rep
        B, C, H, W = latents.shape
        if self.on_device:
            if B != self.batch_size:
                raise ValueError(f'latents batch {B} != the guide\'s batch_size {self.batch_size}')
            eps = self.unet.forward_nhwc(latents, step, self.stacked_embeds(), rep=E)
            out = torch.empty((B, C, H, W), dtype=torch.float32, device=latents.device)
            self.step(None, eps, eps_out=out)
            return out
        eps = self.unet.forward_nhwc(latents, step, self.stacked_embeds(), rep=E)
        stack = ops.nhwc_to_nchw(eps, E, C, H, W)            # (E,C,H,W) fp32
        first = 1 if self.classifier_free_guidance else 0
        bg = stack[first]
        for k, e in enumerate(self.entities):
            y0, y1, x0, x1 = box_slices(e.offset_blocks, e.size_blocks, H, W)
            if y1 <= y0 or x1 <= x0:
                continue
            hip.call('fd_region_blend_f32', bg.data_ptr(), stack[first + 1 + k].data_ptr(), C, H, W,
                     y0, x0, y1 - y0, x1 - x0, float(e.blend), hip.stream())
        if not self.classifier_free_guidance:
            return bg[None].contiguous()
        out = torch.empty((1, C, H, W), dtype=torch.float32, device=latents.device)
        # rows 0 (uncond) and 1 (composited background) are contiguous: u + g (bg - u)
        ops.cfg_ddim_step(None, stack[:2].reshape(-1, 1), C, 1, H * W, True, self.guidance,
                          do_step=False, eps_out=out)
        return out


class WindowedCompositeGuide(WindowedGuide):
    '''CompositeGuide over a canvas larger than the model's own size (beyond the reference): region composition, the headline
    use of MultiDiffusion (Bar-Tal et al. 2023), on `WindowedGuide`'s window batch.  Entities live on the CANVAS: `offset`,
    `size` and `mask` of the schema's entities are in canvas pixels, `weights(H, W)` is `weight_maps` over the canvas
    latent, and a cell's weight does not depend on the window grid.  The UNet batch is the window batch (B Wn latent rows)
    under `rep` = E = cfg + 1 + n context blocks in rep-major order, [uncond] * (B Wn), [bg] * (B Wn), [e_1] * (B Wn) ...;
    per covering window the entities are blended onto the background and CFG is applied, then the windows are averaged and
    ONE step is taken on the canvas -- one launch after the UNet (fd_window_composite_step_f32,
    fd_window_composite_multistep_step_f32).  Every (entity, window) pair is computed, also where the two do not intersect:
    those rows meet weight 0.  `gather`, `bind`, `grid` and `noise_pred` are WindowedGuide's, so FlexPipeline routes this guide
    as it routes that one; `guidance_rescale` and `style_linear` are refused.  A canvas equal to the window is CompositeGuide,
    a schema without entities WindowedGuide on the background prompt, both bit for bit.'''

    def __init__(self, encoder, unet, guidance: float, schema: Schema, steps: int, *, batch_size: int = 1, window=512,
                 stride=256, blend: str = 'uniform', style_linear=None, guidance_rescale: float = 0.0):
        if style_linear is not None:
            raise ValueError('WindowedCompositeGuide does not support style_linear')
        if guidance_rescale:
            raise ValueError('WindowedCompositeGuide does not support guidance_rescale: the per-sample standard deviations '
                             'would have to span the canvas')
        if int(batch_size) < 1:
            raise ValueError(f'batch_size must be >= 1, got {batch_size}')
        B = int(batch_size)
        self.schema = schema
        self.background_embed = encoder.prompt(schema.background_prompt)
        WindowedGuide.__init__(self, encoder, unet, guidance, steps, self.background_embed.expand(B, -1, -1), window=window,
                               stride=stride, blend=blend)
        self.entities: List[EntityEmbeds] = [
            EntityEmbeds(encoder.prompt(e.prompt), px_to_block(e.offset), px_to_block(e.size),
                         e.blend, getattr(e, 'mask', None)) for e in schema.entities]
        if len(self.entities) > MAX_WINDOW_ENTITIES:
            raise ValueError(f'{len(self.entities)} entities: at most {MAX_WINDOW_ENTITIES} over windows')
        self._rows = [self.background_embed] + [e.embed for e in self.entities]
        if self.classifier_free_guidance:
            self._rows = [self.uncond_embeds] + self._rows
        self._wmaps = {}

    @property
    def rep(self) -> int:
        return len(self._rows)                   # E: context blocks of B Wn rows each

    def stacked_embeds(self, count: Optional[int] = None) -> torch.Tensor:
        '''The rep-major E * B * Wn context, built once per window count (default: the count of the last canvas bound).'''
        count = self._count if count is None else count
        if self._wstack is None or self._wstack[0] != count:
            rows = self.batch_size * count
            self._wstack = (count, None, torch.cat([r.float().expand(rows, -1, -1) for r in self._rows]).contiguous())
        return self._wstack[2]

    def weights(self, H: int, W: int) -> Optional[torch.Tensor]:
        '''Device fp32 [n][H][W] blend weights over the canvas latent (None without entities), built once per canvas size and
        kept: a captured graph / recorded plan of the step reads this buffer.'''
        if not self.entities:
            return None
        w = self._wmaps.get((H, W))
        if w is None:
            w = self._wmaps[(H, W)] = weight_maps(self.entities, H, W).to(self.uncond_embeds.device)
        return w

    def entity_maps(self, H: int, W: int) -> torch.Tensor:
        '''`weights(H, W)` as `fused_window_step(entities=)` takes it; without entities an empty [0][H][W] marker, which still
        selects the composite entry point and its rep-major row count.'''
        w = self.weights(H, W)
        return w if w is not None else torch.empty((0, H, W), dtype=torch.float32, device=self.uncond_embeds.device)

    def _check_batch(self, B: int):
        if B != self.batch_size:
            raise ValueError(f'latents batch {B} != the guide\'s batch_size {self.batch_size}')

    def gather(self, canvas: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check_batch(canvas.shape[0])
        return WindowedGuide.gather(self, canvas, out)

    def step(self, x: Optional[torch.Tensor], wins: Optional[torch.Tensor], eps: torch.Tensor, coef=(0.0, 1.0, 1.0, 0.0),
             v_prediction: bool = False, eps_out: Optional[torch.Tensor] = None, mask=None, sigma: float = 0.0,
             step_noise=None):
        '''`WindowedGuide.step` with the entity blend ahead of the CFG combine of every covering window: one launch
        (fd_window_composite_step_f32), combine-only without the canvas `x`.'''
        B, C, H, W = (x if x is not None else eps_out).shape
        self._check_batch(B)
        noise, draw = step_noise if step_noise is not None and sigma else (None, 0)
        ops.window_composite_step(x, wins, eps, self.weights(H, W), B, C, self.grid(H, W).args, self.blend_code,
                                  self.classifier_free_guidance, self.guidance, coef, v_prediction, mask, float(sigma), noise,
                                  int(draw), do_step=x is not None, eps_out=eps_out)
