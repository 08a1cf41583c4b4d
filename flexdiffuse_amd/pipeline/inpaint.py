'''Masked img2img (inpainting) by latent-space known-region replacement -- host side.

A mask over the init image (image pixels, 1 = repaint, 0 = keep) is reduced to latent resolution
(`latent_mask`); after every scheduler step the kept region of the latents is put back on the
clean init latents z0, re-noised with the call's own noise n to the level the step's output sits
at: known = k1 z0 + k2 n, with (k1, k2) from the scheduler's own tables (`known_coefficients`).
The blend itself is fd_cfg_ddim_masked_step_f32 (csrc/step.hip), driven by FlexPipeline.
Beyond the reference, whose README names it as the direction of its composition work.
'''
from __future__ import annotations

from typing import Any, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..encode.clip import sd_size
from ..scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, LMSDiscreteScheduler, PNDMScheduler,
                         UniPCMultistepScheduler)


def _is_pil(obj: Any) -> bool:
    try:
        from PIL import Image
    except ImportError:          # pragma: no cover -- PIL is optional for array masks
        return False
    return isinstance(obj, Image.Image)


def image_size(init_image: Any) -> Tuple[int, int]:
    '''(height, width) in pixels the init image ends up at: `sd_size` of a PIL image (what
    `preprocess` resizes it to), a tensor's own last two dimensions.'''
    if isinstance(init_image, torch.Tensor):
        return int(init_image.shape[-2]), int(init_image.shape[-1])
    w, h = sd_size(*init_image.size)
    return int(h), int(w)


def latent_mask(mask: Any, height: int, width: int, factor: int) -> torch.Tensor:
    '''Mask over a `height` x `width` image -> CPU fp32 [height // factor][width // factor]: the
    mean of each factor x factor pixel block (the block one latent cell covers; `factor` is the
    VAE's own, 8 for the SD VAEs).  `mask`: a 2-D array-like or torch tensor of floats in [0, 1]
    of exactly that shape, or a PIL image, read as convert('L') / 255 after a Lanczos resize
    (the resampling of `preprocess`) to that size and clipped to [0, 1].  ValueError on a wrong
    shape, NaN, values outside [0, 1], or a factor that does not divide the image size.'''
    height, width, factor = int(height), int(width), int(factor)
    if factor < 1 or height % factor or width % factor:
        raise ValueError(f'factor {factor} does not divide the image size (height, width) {(height, width)}')
    if _is_pil(mask):
        from PIL import Image
        lanczos = getattr(Image, 'LANCZOS', None) or Image.Resampling.LANCZOS
        grey = mask.convert('L')
        if grey.size != (width, height):
            grey = grey.resize((width, height), resample=lanczos)
        m = np.clip(np.asarray(grey, dtype=np.float32) / np.float32(255), 0.0, 1.0)
    else:
        if hasattr(mask, 'detach'):
            mask = mask.detach().cpu().numpy()
        m = np.array(mask, dtype=np.float32)
    if m.ndim != 2 or m.shape != (height, width):
        raise ValueError(f'mask shape {m.shape} != the init image (height, width) {(height, width)} in image pixels')
    if np.isnan(m).any():
        raise ValueError('mask holds NaN')
    if m.size and (m.min() < 0.0 or m.max() > 1.0):
        raise ValueError(f'mask values must lie in [0, 1], got [{m.min()}, {m.max()}]')
    cell = F.avg_pool2d(torch.from_numpy(np.ascontiguousarray(m))[None, None], factor)[0, 0]
    # a block of ones averages to exactly 1 and one of zeros to exactly 0 (the kernel's exact branches); the clamp only
    # guards a mean that rounding could push past 1
    return cell.clamp_(0.0, 1.0).contiguous()


def known_coefficients(scheduler, timesteps: Sequence, t_start: int,
                       start: Optional[Tuple[float, float]] = None) -> List[Tuple[float, float]]:
    '''One (k1, k2) per step of the request `timesteps[t_start:]`: the noise level of that step's
    OUTPUT, known = k1 z0 + k2 n, from the scheduler's own tables.  DDIM: (sqrt(a_p), sqrt(1 - a_p))
    with the a_p of `_alphas(t)`; PNDM: the same with the a_p its `step` hands to
    `prev_coefficients` (index + 1 - offset; its second call lands on the level of its first);
    K-LMS (sigma space, x = z0 + sigma n): (1, sigmas[i + 1]); DPM-Solver++ and UniPC: (alpha_t, sigma_t) of the step's target
    t = the next timestep of the list (its steps of either order keep a sample with eps = n on that level, and an img2img
    request starts on the table).  The last pair is (1, 0) exactly.

    `start` (PNDM only): the level (k1, k2) the request's initial latents were noised to.  An
    img2img request under PNDM does not start on the level its first `step` assumes (add_noise
    reads alphas_cumprod[t], the step alphas_cumprod[t + 1 - offset], and the sliced timestep list
    moves the repeated timestep), so the table level is not the one the latents are at.  With
    `start`, the level is carried through the request by each call's own `prev_coefficients`
    (x' = cs x + ce eps, eps = n on the known trajectory; the second call restarts from the first
    one's input, as `step` does) -- the level a sample that started at `start` really sits at, which
    is the table's whenever the request starts on it.'''
    ts = list(timesteps[t_start:])
    one = np.float32(1.0)
    pairs: List[Tuple[float, float]] = []
    if isinstance(scheduler, LMSDiscreteScheduler):
        pairs = [(1.0, float(np.float32(scheduler.sigmas[t_start + i + 1]))) for i in range(len(ts))]
    elif isinstance(scheduler, DDIMScheduler):
        for t in ts:
            a_p = scheduler._alphas(int(t))[1]
            pairs.append((float(np.sqrt(a_p)), float(np.sqrt(one - a_p))))
    elif isinstance(scheduler, (DPMSolverMultistepScheduler, UniPCMultistepScheduler)):
        for i in range(len(ts)):
            t = int(ts[i + 1]) if i + 1 < len(ts) else 0
            pairs.append((float(np.float32(scheduler.alpha_t[t])), float(np.float32(scheduler.sigma_t[t]))))
    elif isinstance(scheduler, PNDMScheduler):
        # PNDMScheduler.step: counter == i for a request (set_timesteps resets it); its second call steps from
        # t + ratio to t, from the sample of before the first call
        ratio = scheduler.config['num_train_timesteps'] // scheduler.num_inference_steps
        level = first = None if start is None else (float(start[0]), float(start[1]))
        for i, t in enumerate(ts):
            t, prev = (int(t) + ratio, int(t)) if i == 1 else (int(t), max(int(t) - ratio, 0))
            if start is None:
                a_p = np.float32(scheduler.alphas_cumprod[prev + 1 - scheduler._offset])
                pairs.append((float(np.sqrt(a_p)), float(np.sqrt(one - a_p))))
            else:
                cs, ce = (float(c) for c in scheduler.prev_coefficients(t, prev))
                src = first if i == 1 else level
                level = (cs * src[0], cs * src[1] + ce)
                pairs.append(level)
    else:
        raise TypeError(f'mask_image: no noise-level table for scheduler {type(scheduler).__name__}')
    if pairs:
        pairs[-1] = (1.0, 0.0)
    return pairs


def start_level(scheduler, t_noise: int) -> Optional[Tuple[float, float]]:
    '''The (k1, k2) `scheduler.add_noise(z0, n, t_noise)` noises to, for `known_coefficients(start=)`;
    None for the schedulers whose requests start on their own table (DDIM, K-LMS).'''
    if not isinstance(scheduler, PNDMScheduler):
        return None
    a = np.float32(scheduler.alphas_cumprod[int(t_noise)])
    return float(np.sqrt(a)), float(np.sqrt(np.float32(1.0) - a))
