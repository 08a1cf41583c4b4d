'''The counter-based normal stream of the stochastic samplers (csrc/philox.h; include/flexdiffuse_hip.h states it).

A value is a pure function of (seed, global sample index, element inside the sample, draw, stream): Philox4x32-10 keyed
by the 64-bit seed on the counter (element >> 2, sample, draw, stream), then Box-Muller on the four words.  The step
kernels generate it in registers (stream 0, draw = the step's index in the scheduler's timestep list); nothing here is
ever drawn on the host.  `sample_offset` is the global index of a call's first sample, so a batch split over ranks
(`dist.sample_offset`) or over sequential calls (`utils.Runner`) sees the noise of the one large batch.

Streams: 0 (`STREAM_STEP`) the step noise of the step kernels, 1 (`STREAM_FILL`) the stand-alone fill, 2 (`STREAM_INIT`) the
start noise of a request that begins from clean latents (`FlexPipeline.__call__(init_latents=)`, the second pass of hires
sampling): draw 0, generated inside fd_latent_upscale_noise_f32 at the canvas element, so the values are those of
`PhiloxNoise.normal((B, C, H, W), 0, stream=STREAM_INIT)` and never collide with a step's draw.
'''
from __future__ import annotations

from typing import Sequence

import torch

STREAM_STEP, STREAM_FILL, STREAM_INIT = 0, 1, 2


class PhiloxNoise():
    '''The address of one request's noise: `seed` (taken modulo 2^64) and the global index of its first sample.'''

    def __init__(self, seed: int, sample_offset: int = 0):
        if sample_offset < 0:
            raise ValueError(f'sample_offset {sample_offset} is negative')
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.sample_offset = int(sample_offset)

    def normal(self, shape: Sequence[int], draw: int = 0, stream: int = STREAM_FILL, device='cuda') -> torch.Tensor:
        '''fp32 device tensor of `shape`, dim 0 the samples (the first is sample `sample_offset`): fd_philox_normal_f32.'''
        from . import ops
        shape = tuple(int(s) for s in shape)
        out = torch.empty(shape, dtype=torch.float32, device=device)
        per = out.numel() // shape[0] if len(shape) > 1 else out.numel()
        return ops.philox_normal(out, per, self.seed, self.sample_offset, draw, stream)

    def __repr__(self):
        return f'PhiloxNoise(seed={self.seed:#x}, sample_offset={self.sample_offset})'
