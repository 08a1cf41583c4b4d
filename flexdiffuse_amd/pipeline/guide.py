'''Noise-prediction guides -- host-side mirror of the reference's `pipeline/guide.py`
(GuideBase :8-36, SimpleGuide :39-64, PromptGuide :67-72): same attributes
(`batch_size, steps, guidance, uncond_embeds, encoder, unet`) and the same
`noise_pred(latents, step)` protocol, so custom guides written against the reference keep
working.  `SimpleGuide` additionally exposes what FlexPipeline's fused device loop needs.
'''
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from .. import ops, windows
from ..ctx_schedule import ContextSchedule, check_keyframes, step_weights


class GuideBase():
    def __init__(self, encoder, unet, guidance: float, steps: int) -> None:
        '''Args mirror pipeline/guide.py:9-29 (encoder: CLIPEncoder, unet, guidance scale as in
        classifier-free guidance -- enabled when > 1 --, number of denoising steps).'''
        self.encoder = encoder
        self.unet = unet
        self.uncond_embeds = encoder.prompt('')
        self.batch_size = 1
        self.guidance = guidance
        self.steps = steps

    def noise_pred(self, latents: torch.Tensor, step: int) -> torch.Tensor:
        raise NotImplementedError('noise_pred must be implemented.')


def check_guidance_rescale(guidance_rescale: float, guidance: float):
    '''ValueError unless 0 <= guidance_rescale <= 1, and classifier-free guidance is on whenever it is > 0.'''
    if not 0.0 <= guidance_rescale <= 1.0:
        raise ValueError(f'guidance_rescale should be in [0.0, 1.0] but is {guidance_rescale}')
    if guidance_rescale > 0.0 and not guidance > 1.0:
        raise ValueError(f'guidance_rescale {guidance_rescale} needs classifier-free guidance (guidance > 1, got {guidance}): '
                         'it rescales the guided output')


class SimpleGuide(GuideBase):
    def __init__(self, encoder, unet, guidance: float, steps: int, clip_embeds: torch.Tensor, *,
                 guidance_rescale: float = 0.0):
        '''`guidance_rescale` (beyond the reference; Lin et al. 2023 sec. 3.4, diffusers' `rescale_noise_cfg`): in [0, 1]; the
        guided output of each sample is scaled towards the standard deviation of its conditional output.  A plain attribute,
        read by FlexPipeline at every call; 0 is the reference's combine.'''
        GuideBase.__init__(self, encoder, unet, guidance, steps)
        self.guidance_rescale = guidance_rescale
        self.embeds = clip_embeds
        self.batch_size = self.embeds.shape[0]
        self._stack = None

    @property
    def classifier_free_guidance(self) -> bool:
        return self.guidance > 1.0

    def stacked_embeds(self) -> torch.Tensor:
        '''[uncond]*B + embeds (pipeline/guide.py:49-53), built once instead of every step so
        the UNet's cross-attention K/V projections of the context are computed once.'''
        if not self.classifier_free_guidance:
            return self.embeds
        if self._stack is None or self._stack_src is not self.embeds:
            B = self.batch_size
            self._stack = torch.cat([self.uncond_embeds.to(self.embeds.dtype).expand(B, -1, -1),
                                     self.embeds]).contiguous()
            self._stack_src = self.embeds
        return self._stack

    def noise_pred(self, latents: torch.Tensor, step) -> torch.Tensor:
        cfg = self.classifier_free_guidance
        B, C, H, W = latents.shape
        # one UNet pass over [uncond | cond]; latents are duplicated inside the layout kernel
        eps = self.unet.forward_nhwc(latents, step, self.stacked_embeds(), rep=2 if cfg else 1)
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=latents.device)
        # u + g (t - u)  (pipeline/guide.py:59-63), NHWC fp32 -> NCHW fp32
        if self.guidance_rescale:
            check_guidance_rescale(self.guidance_rescale, self.guidance)
            ops.cfg_rescale_ddim_step(None, eps, B, C, H * W, self.guidance, self.guidance_rescale, do_step=False, eps_out=out)
        else:
            ops.cfg_ddim_step(None, eps, B, C, H * W, cfg, self.guidance, do_step=False, eps_out=out)
        return out


class PromptGuide(SimpleGuide):
    def __init__(self, encoder, unet, guidance: float, steps: int, prompt: Union[str, List[str]], *,
                 guidance_rescale: float = 0.0):
        SimpleGuide.__init__(self, encoder, unet, guidance, steps, encoder.prompt(prompt), guidance_rescale=guidance_rescale)
        self.prompt = prompt


class WindowedGuide(SimpleGuide):
    '''SimpleGuide over a canvas larger than the model's own size (beyond the reference; MultiDiffusion, Bar-Tal et al. 2023):
    the canvas latents are covered by overlapping windows (`windows.window_grid`), every step runs the UNet on all windows of
    all samples as one batch, the guided predictions are averaged where windows overlap (`blend`: 'uniform', or 'tent'
    weights that fall off towards a window's edge) and ONE scheduler step is taken on the canvas.  `window` and `stride` are
    in image pixels, (height, width) or one int for both, divided by 8 as FlexPipeline divides `init_size`; the canvas is
    whatever latents the guide is handed.  A canvas equal to the window is SimpleGuide, bit for bit.

    `noise_pred` is the generic protocol (gather, eager UNet, combine-only fd_window_step_f32), so every scheduler and any
    caller written against GuideBase works.  FlexPipeline runs its device loop instead: the window batch is the buffer its
    graph / launch plan reads, and under DDIM (eta = 0, or eta > 0 with `pipe.step_noise`), DPM-Solver++ and its SDE form a
    step is the UNet replay plus ONE launch (fd_window_step_f32, fd_window_ddim_step_f32, fd_window_multistep_step_f32: CFG,
    average, the update of the canvas, the step noise, the known-region blend of a masked request, the next window batch).
    The step noise is addressed by the canvas element, so it does not depend on the window grid.  Every other scheduler
    (PNDM, K-LMS, DDIM eta > 0 on generator noise) takes the planned route: one gather, the UNet replay, the combine-only
    form, `scheduler.step` -- the bits of the `noise_pred` loop.  `guidance_rescale` is not supported (its standard
    deviations would have to span the canvas).  Region composition over windows is the subclass
    `composition.guide.WindowedCompositeGuide`: the same routes, the entity blend inside the same one launch.'''

    def __init__(self, encoder, unet, guidance: float, steps: int, clip_embeds: torch.Tensor, *, window=(512, 512),
                 stride=(256, 256), blend: str = 'uniform', guidance_rescale: float = 0.0):
        if guidance_rescale:
            raise ValueError('WindowedGuide does not support guidance_rescale: the per-sample standard deviations would have '
                             'to span the canvas')
        SimpleGuide.__init__(self, encoder, unet, guidance, steps, clip_embeds)
        self.window = tuple(v // 8 for v in windows.pair(window))        # latent cells, (h, w)
        self.stride = tuple(v // 8 for v in windows.pair(stride))
        self.blend = blend
        self.blend_code = windows.check_blend(blend)
        # what the UNet asks of a latent's extents: one halving per level below the first
        chans = (getattr(unet, 'config', None) or {}).get('block_out_channels')
        self._multiple = 2 ** (len(chans) - 1) if chans else 1
        # the geometry errors that do not depend on the canvas surface here, not at the first step
        windows.window_grid(*self.window, *self.window, *self.stride, multiple=self._multiple)
        self.on_device = True
        self._grids = {}
        self._count = 1                          # windows per sample of the canvas last bound
        self._wstack = None

    @property
    def rep(self) -> int:
        return 2 if self.classifier_free_guidance else 1

    def grid(self, H: int, W: int) -> 'windows.WindowGrid':
        '''The window grid over an (H, W) canvas of latent cells (ValueError: windows.window_grid).'''
        g = self._grids.get((H, W))
        if g is None:
            g = self._grids[(H, W)] = windows.window_grid(H, W, *self.window, *self.stride, multiple=self._multiple)
        return g

    def stacked_embeds(self, count: Optional[int] = None) -> torch.Tensor:
        '''[uncond] * (B Wn), then each sample's embedding repeated Wn times: built once per window count (default: the
        count of the last canvas seen).'''
        count = self._count if count is None else count
        if self._wstack is None or self._wstack[0] != count or self._wstack[1] is not self.embeds:
            ctx = windows.window_context(self.uncond_embeds, self.embeds, count, self.classifier_free_guidance)
            self._wstack = (count, self.embeds, ctx)
        return self._wstack[2]

    def bind(self, H: int, W: int) -> 'windows.WindowGrid':
        '''Fix the canvas of the running request: `stacked_embeds()` is then the context of its window batch.'''
        g = self.grid(H, W)
        self._count = g.count
        return g

    def gather(self, canvas: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        '''The window batch (B Wn, C, h, w) of a canvas (B, C, H, W): one launch.'''
        B, C, H, W = canvas.shape
        g = self.bind(H, W)
        if out is None:
            out = torch.empty((B * g.count, C, g.h, g.w), dtype=torch.float32, device=canvas.device)
        ops.window_gather(canvas, out, B, C, g.args)
        return out

    def step(self, x: Optional[torch.Tensor], wins: Optional[torch.Tensor], eps: torch.Tensor, coef=(0.0, 1.0, 1.0, 0.0),
             v_prediction: bool = False, eps_out: Optional[torch.Tensor] = None, mask=None, sigma: float = 0.0,
             step_noise=None):
        '''CFG + average of the UNet output `eps` over the window batch (NHWC fp32) into `eps_out` (NCHW fp32 canvas,
        optional) and, given the canvas `x`, its DDIM update in place plus -- given `wins` -- the next window batch:
        one launch.  With the canvas, optionally in that launch: `sigma` and `step_noise` = (PhiloxNoise, draw), the
        eta > 0 term sigma z addressed by the canvas element; `mask` = (z0, noise, mask [H W], k1, k2), the known-region
        blend of masked img2img (the window batch then holds the blended canvas).'''
        B, C, H, W = (x if x is not None else eps_out).shape
        if x is not None and (mask is not None or sigma):
            noise, draw = step_noise if step_noise is not None else (None, 0)
            ops.window_ddim_step(x, wins, eps, B, C, self.grid(H, W).args, self.blend_code, self.classifier_free_guidance,
                                 self.guidance, coef, v_prediction, mask, float(sigma), noise, int(draw), eps_out)
            return
        ops.window_step(x, wins, eps, B, C, self.grid(H, W).args, self.blend_code, self.classifier_free_guidance,
                        self.guidance, coef, v_prediction, do_step=x is not None, eps_out=eps_out)

    def noise_pred(self, latents: torch.Tensor, step) -> torch.Tensor:
        if self.guidance_rescale:
            raise ValueError('WindowedGuide does not support guidance_rescale')
        latents = latents.to(torch.float32).contiguous()
        wins = self.gather(latents)
        eps = self.unet.forward_nhwc(wins, step, self.stacked_embeds(), rep=self.rep)
        out = torch.empty_like(latents)
        self.step(None, None, eps, eps_out=out)
        return out


class ScheduledGuide(SimpleGuide):
    '''SimpleGuide whose context moves over the steps (beyond the reference): `keyframes` are K >= 2 embeddings of one shape
    (B, L, D) -- prompts, or a prompt and its image-guided form --, step j runs on key_k + w (key_{k+1} - key_k) with (k, w)
    from ctx_schedule.step_weights(steps, K, schedule, positions).  `noise_pred` is SimpleGuide's own, so every fused and
    planned route of FlexPipeline applies; the pipeline calls `at_step(t_start + i)` before each step.  mode='lerp': the
    keyframes' cross-attention projections are cached and a step costs one fd_lerp_f16; mode='project' (or FD_CTX_LERP=0):
    the blended context is reprojected every step.'''

    def __init__(self, encoder, unet, guidance: float, steps: int, keyframes: Sequence[torch.Tensor],
                 schedule: Sequence[float] = (0.0, 1.0), positions: Optional[Sequence[float]] = None, mode: str = 'lerp',
                 *, guidance_rescale: float = 0.0):
        check_keyframes(keyframes)
        weights = step_weights(steps, len(keyframes), schedule, positions)
        SimpleGuide.__init__(self, encoder, unet, guidance, steps, keyframes[0], guidance_rescale=guidance_rescale)
        self.keyframes = list(keyframes)
        B = self.batch_size
        if self.classifier_free_guidance:       # [uncond]*B + keyframe, as SimpleGuide.stacked_embeds stacks its one context
            un = self.uncond_embeds.float().expand(B, -1, -1)
            stacked = [torch.cat([un, k.float()]).contiguous() for k in keyframes]
        else:
            stacked = [k.float().contiguous() for k in keyframes]
        self.context = ContextSchedule(unet, stacked, weights, mode)

    @property
    def weights(self):
        return self.context.weights

    def at_step(self, j: int):
        self.context.at_step(j)

    def stacked_embeds(self) -> torch.Tensor:
        return self.context.handle()
