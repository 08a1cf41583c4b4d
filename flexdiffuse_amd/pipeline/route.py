'''Which loop a FlexPipeline request runs, decided once per request: `select_route` reads the guide, the scheduler, the UNet and
the request's switches and returns a `Route`; `FlexPipeline.__call__` then runs one step method per iteration.  No launch, no
tensor.  This is the route table (DESIGN.md sec. 7 keeps the history of the features behind it).

The guide kind (by whose `noise_pred` the guide's class has; everything needs a UNet with `forward_nhwc`):
  simple      SimpleGuide's own (ScheduledGuide included)
  composite   CompositeGuide's own, with `fuse_composite` on or a batched / masked guide (`on_device`)
  window      WindowedGuide's own (WindowedCompositeGuide included: it inherits it, and carries its entities in its `step`)
  other       anything else: the reference protocol
`fuse` below: a simple guide, or a composite one with `fuse_composite` on (`fuse_entities`: the entity blend rides in the
step's launch).  `on`: graph or plan in use and `debug` off.  `noise`: `pipe.step_noise` given, or an SDE scheduler (which
gets one from the generator's seed).  The first row that applies is the route:

  kind               scheduler, eta                        loop            a step is the UNet replay (debug: eager) and
  simple, composite  DDIM, eta = 0 | eta > 0, noise, fuse  ddim            one launch: fd_cfg_ddim_step_f32 | _masked_ (mask image) |
                                                                           _noise_ (eta > 0) | fd_cfg_rescale_ddim_step_f32 (rescale) |
                                                                           fd_composite_step_f32 (+ a blend-only launch with a mask
                                                                           image) | fd_composite_ddim_step_f32 (fuse_entities and a
                                                                           mask image or eta > 0)
  fuse               DPM-Solver++ (2M), its SDE form       multistep       one launch: fd_cfg_multistep_step_f32 | _noise_ (SDE) |
                                                                           fd_cfg_rescale_multistep_step_f32 |
                                                                           fd_composite_multistep_step_f32
  fuse               UniPC (eta = 0, no step noise)        unipc           one launch: fd_cfg_unipc_step_f32 |
                                                                           fd_cfg_rescale_unipc_step_f32 |
                                                                           fd_composite_unipc_step_f32 (corrector, kept sample and
                                                                           predictor in it)
  fuse               PNDM, K-LMS; on, no rescale,          linear          one launch: fd_cfg_linear_multistep_step_f32 |
                     `fuse_linear_multistep`                               fd_composite_linear_multistep_step_f32 (K-LMS: the launch
                                                                           also writes the next scaled model input)
  simple, composite  any other; on                         planned         the combine-only launch (fd_cfg_ddim_step_f32 |
                                                                           fd_cfg_rescale_ddim_step_f32 | fd_composite_step_f32),
                                                                           `scheduler.step`, the blend-only launch of a mask image
  window             DPM-Solver++ and SDE; DDIM, eta = 0   window          one launch over the window batch: fd_window_step_f32 |
                     | eta > 0, noise                                      fd_window_ddim_step_f32 (mask image or eta > 0) |
                                                                           fd_window_multistep_step_f32; a
                                                                           WindowedCompositeGuide: fd_window_composite_step_f32 |
                                                                           fd_window_composite_multistep_step_f32
  window             any other; on                         window_planned  fd_window_gather_f32, the replay, the combine-only
                                                                           fd_window_step_f32 (a WindowedCompositeGuide: of
                                                                           fd_window_composite_step_f32), `scheduler.step`, the
                                                                           blend-only launch
  any                any                                   generic         `guide.noise_pred`, `scheduler.step`, the blend-only launch

Ahead of the loop, a request that starts from clean latents (`FlexPipeline.from_latents`, the second pass of `hires`) makes ONE
launch, fd_latent_upscale_noise_f32 (upscale + add_noise; the noise in-kernel with `pipe.step_noise`), in place of add_noise:

  loop               the pre-loop launch writes            then
  window             the canvas AND the window batch       nothing: no fd_window_gather_f32, no fd_axpby_f32
  any other          the canvas (windows_out = NULL)       the route's own setup, unchanged (the copy into the persistent buffer,
                                                           K-LMS's scaled input, `window_planned`'s gather)

`ddim`, `multistep`, `unipc` and `linear` (PLMS) step in the persistent buffer the graph / plan reads when `on` (`persistent`); every
loop but `generic` reads the request's time-embedding table (`temb_table`).  Guidance rescale applies to a simple guide only
(any other applies or ignores its own attribute in its `noise_pred`) and is refused for a window guide.  On `planned`,
`window_planned` and `generic` a scheduler whose `step` takes `step_noise=` draws from the stream (`takes_noise`), one whose
`step` takes `eta=` gets it (`accepts_eta`).  UniPC has no stochastic form: `eta > 0` or `pipe.step_noise` under it is a ValueError
on every route; its window guides run `window_planned` / `generic` through `scheduler.step`, the same kernel on B C planes.'''
from __future__ import annotations

import inspect
from dataclasses import dataclass

from ..scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler, LMSDiscreteScheduler,
                         PNDMScheduler, UniPCMultistepScheduler)
from .guide import SimpleGuide, WindowedGuide


@dataclass(frozen=True)
class Route():
    loop: str               # 'ddim' | 'multistep' | 'unipc' | 'linear' | 'window' | 'planned' | 'window_planned' | 'generic'
    guide: str              # 'simple' | 'composite' | 'window' | 'other'
    fuse_entities: bool     # composite: the entity blend inside the scheduler's own one-launch step
    noisy: bool             # DDIM's eta > 0 term from the counter-based stream, inside the step's launch
    multistep: bool         # DPM-Solver++ or its SDE form (what the `window` loop steps with)
    sde: bool
    is_lms: bool
    rescale: float          # the effective guidance rescale: 0 unless the guide is simple
    takes_noise: bool
    accepts_eta: bool
    persistent: bool        # the loop steps in `loop_latents`
    temb_table: bool


def select_route(guide, scheduler, unet, *, eta, step_noise, rescale, debug, use_graph, use_plan, fuse_composite,
                 fuse_linear_multistep) -> Route:
    from ..composition.guide import CompositeGuide
    device = hasattr(unet, 'forward_nhwc')
    pred = type(guide).noise_pred
    kind = 'other'
    if device and pred is SimpleGuide.noise_pred:
        kind = 'simple'
    elif device and pred is CompositeGuide.noise_pred and (fuse_composite or getattr(guide, 'on_device', False)):
        kind = 'composite'
    elif device and pred is WindowedGuide.noise_pred:
        kind = 'window'
    if kind == 'window' and rescale:
        raise ValueError('WindowedGuide does not support guidance_rescale')
    rescale = rescale if kind == 'simple' else 0.0
    fuse_entities = kind == 'composite' and bool(fuse_composite)
    fuse = kind == 'simple' or fuse_entities
    ddim, multistep = isinstance(scheduler, DDIMScheduler), isinstance(scheduler, DPMSolverMultistepScheduler)
    sde, is_lms = isinstance(scheduler, DPMSolverMultistepSDEScheduler), isinstance(scheduler, LMSDiscreteScheduler)
    unipc = isinstance(scheduler, UniPCMultistepScheduler)
    if unipc and (eta or step_noise is not None):
        raise ValueError('UniPCMultistepScheduler has no stochastic form: it takes neither eta > 0 nor pipe.step_noise')
    has_noise = step_noise is not None or sde
    on = bool(use_graph or use_plan) and not debug
    loop, noisy = 'generic', False
    if kind in ('simple', 'composite'):
        noisy = bool(eta) and has_noise and fuse
        if ddim and (not eta or noisy):
            loop = 'ddim'
        elif multistep and fuse:
            loop = 'multistep'
        elif unipc and fuse:
            loop = 'unipc'
        elif on and fuse and not rescale and fuse_linear_multistep and isinstance(scheduler, (PNDMScheduler, LMSDiscreteScheduler)):
            loop = 'linear'
        else:
            loop = 'planned' if on else 'generic'
    elif kind == 'window':
        noisy = bool(eta) and has_noise and ddim
        loop = 'window' if multistep or (ddim and (not eta or noisy)) else 'window_planned' if on else 'generic'
    step = inspect.signature(scheduler.step).parameters
    return Route(loop, kind, fuse_entities, noisy, multistep, sde, is_lms, rescale,
                 takes_noise=has_noise and 'step_noise' in step, accepts_eta='eta' in step,
                 persistent=on and (loop in ('ddim', 'multistep', 'unipc') or (loop == 'linear' and not is_lms)),
                 temb_table=loop != 'generic' and hasattr(unet, 'time_bias_table'))
