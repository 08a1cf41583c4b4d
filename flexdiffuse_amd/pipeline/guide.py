'''Noise-prediction guides -- host-side mirror of the reference's `pipeline/guide.py`
(GuideBase :8-36, SimpleGuide :39-64, PromptGuide :67-72): same attributes
(`batch_size, steps, guidance, uncond_embeds, encoder, unet`) and the same
`noise_pred(latents, step)` protocol, so custom guides written against the reference keep
working.  `SimpleGuide` additionally exposes what FlexPipeline's fused device loop needs.
'''
from __future__ import annotations

from typing import List, Optional, Sequence, Union

import torch

from .. import ops
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
