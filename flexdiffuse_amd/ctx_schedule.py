'''Context schedules -- which blend of a request's keyframe contexts each denoising step sees.

A schedule has K >= 2 keyframe contexts of one shape (Be, L, D), positions 0 = p_0 < ... < p_{K-1} = 1 and one weight per
step.  Step j is the GLOBAL index into the scheduler's timestep list (t_start + i: an img2img request starts inside the
schedule, as its step noise does):

    progress_j = j / (steps - 1)                         (0 when steps == 1)
    s_j        = s_first + (s_last - s_first) progress_j   for a (s_first, s_last) pair; an explicit list of `steps` floats is used as given
    (k, w)     : p_k <= s_j < p_{k+1} ,  w = (s_j - p_k) / (p_{k+1} - p_k)
                 s_j < 0 extrapolates on the first segment (w < 0), s_j >= 1 sits on / extrapolates the last one (w >= 1)

and the step's context is  key_k + w (key_{k+1} - key_k).  A scheduler whose timestep list is longer than `steps` (PLMS repeats
one timestep; DDIM at a step count that does not divide 1000) holds the last step's weight on the extra entries.  Everything here is Python float arithmetic without a device;
`w` reaches the kernels as a float32.  `ContextSchedule` carries a schedule to the UNet for the guides that use one
(pipeline.guide.ScheduledGuide, composition.guide.CompositeGuide(style_linear=)).
'''
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch


def keyframe_positions(n_keyframes: int, positions: Optional[Sequence[float]] = None) -> List[float]:
    '''The validated positions of `n_keyframes` keyframes; None: evenly spaced.'''
    K = int(n_keyframes)
    if K < 2:
        raise ValueError(f'a context schedule needs at least 2 keyframes, got {K}')
    if positions is None:
        return [i / (K - 1) for i in range(K)]
    p = [float(v) for v in positions]
    if len(p) != K:
        raise ValueError(f'{len(p)} positions for {K} keyframes')
    if p[0] != 0.0 or p[-1] != 1.0 or any(b <= a for a, b in zip(p, p[1:])):
        raise ValueError(f'keyframe positions must rise strictly from 0 to 1, got {p}')
    return p


def locate(s: float, positions: Sequence[float]) -> Tuple[int, float]:
    '''(k, w) of schedule value `s` in the keyframe positions: the segment that holds it and the weight inside it.'''
    k = len(positions) - 2
    for i in range(len(positions) - 1):
        if s < positions[i + 1]:
            k = i
            break
    return k, (s - positions[k]) / (positions[k + 1] - positions[k])


def schedule_values(steps: int, schedule: Sequence[float] = (0.0, 1.0)) -> List[float]:
    '''s_j of every step of a `steps`-step request.'''
    steps = int(steps)
    if steps < 1:
        raise ValueError(f'steps must be >= 1, got {steps}')
    s = [float(v) for v in schedule]
    if len(s) == 2:             # (with steps == 2 the pair and the explicit list are the same thing)
        return [s[0] + (s[1] - s[0]) * (j / (steps - 1) if steps > 1 else 0.0) for j in range(steps)]
    if len(s) != steps:
        raise ValueError(f'a schedule is a (first, last) pair or one weight per step: got {len(s)} values for {steps} steps')
    return s


def step_weights(steps: int, n_keyframes: int = 2, schedule: Sequence[float] = (0.0, 1.0),
                 positions: Optional[Sequence[float]] = None) -> List[Tuple[int, float]]:
    '''[(k, w)] for j = 0 .. steps - 1: step j runs on key_k + w (key_{k+1} - key_k).'''
    p = keyframe_positions(n_keyframes, positions)
    return [locate(s, p) for s in schedule_values(steps, schedule)]


def check_keyframes(keyframes: Sequence[torch.Tensor]) -> Tuple[int, int, int]:
    '''The common (Be, L, D) of the keyframe contexts; ValueError for fewer than two or for differing shapes.'''
    if len(keyframes) < 2:
        raise ValueError(f'a context schedule needs at least 2 keyframes, got {len(keyframes)}')
    shape = tuple(keyframes[0].shape)
    if len(shape) != 3:
        raise ValueError(f'a keyframe context is (batch, tokens, dim), got {shape}')
    for i, t in enumerate(keyframes):
        if tuple(t.shape) != shape:
            raise ValueError(f'keyframe {i} has shape {tuple(t.shape)}, keyframe 0 has {shape}')
    return shape


def blend_f32(a: torch.Tensor, b: torch.Tensor, w: float) -> torch.Tensor:
    '''The fp32 blend of two keyframe contexts, a + w (b - a) with w as float32 -- what the `project` route projects and
    what the tests' CPU loop feeds its UNet.'''
    a, b = a.float(), b.float()
    return a + torch.tensor(float(w), dtype=torch.float32, device=a.device) * (b - a)


def resolve_mode(mode: str) -> str:
    '''`lerp` unless asked otherwise; FD_CTX_LERP=0 turns every `lerp` request into `project` (A/B).'''
    if mode not in ('lerp', 'project'):
        raise ValueError(f"mode must be 'lerp' or 'project', got {mode!r}")
    return 'project' if mode == 'lerp' and os.environ.get('FD_CTX_LERP', '1') == '0' else mode


class ContextSchedule():
    '''A schedule bound to a UNet.  `handle()` is the one context tensor the request passes to the UNet at every step;
    `at_step(j)` makes the UNet's cached cross-attention projections those of step j's blend, on the current stream:

      mode='lerp'     the keyframes are projected once (UNet2DConditionModel.set_context_keyframes) and a step is ONE
                      fd_lerp_f16 over the cached projections (blend_context), written where the captured forward reads
      mode='project'  the fp32 blend of the keyframe contexts is written into the handle and today's set_context
                      reprojects it in place -- ~37 launches per step; the yardstick of the tests and the A/B partner
    '''

    def __init__(self, unet, keyframes: Sequence[torch.Tensor], weights: Sequence[Tuple[int, float]], mode: str = 'lerp'):
        check_keyframes(keyframes)
        self.unet = unet
        self.keyframes = [k.float().contiguous() for k in keyframes]
        self.weights = [(int(k), float(w)) for k, w in weights]
        if any(not 0 <= k < len(self.keyframes) - 1 for k, _ in self.weights):
            raise ValueError('a step weight names a segment the keyframes do not have')
        self.mode = resolve_mode(mode)
        self.trace: List[Tuple[int, int, float]] = []      # (j, k, w) of every at_step call of the running request
        self._live = None                                 # project route: the fp32 context the UNet reprojects
        self._held = None

    def handle(self) -> torch.Tensor:
        if self.mode == 'lerp':
            return self.unet.set_context_keyframes(self.keyframes)
        if self._live is None:
            self._live = self.keyframes[0].clone()
            self._held = (0, 0.0)
        return self._live

    def at_step(self, j: int):
        k, w = self.weights[min(int(j), len(self.weights) - 1)]
        if self.trace and j <= self.trace[-1][0]:
            self.trace.clear()                            # a new request
        self.trace.append((int(j), k, w))
        if self.mode == 'lerp':
            self.unet.set_context_keyframes(self.keyframes)
            self.unet.blend_context(k, w)
        elif (k, w) != self._held or self._live is None:
            live = self.handle()
            live.copy_(blend_f32(self.keyframes[k], self.keyframes[k + 1], w))    # in place: bumps the version set_context keys on
            self._held = (k, w)
