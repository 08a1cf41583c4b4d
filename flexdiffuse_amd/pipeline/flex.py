'''Image-guided denoising pipeline -- host-side mirror of the reference's
`pipeline/flex.py` `FlexPipeline` (ctor :46-83, attention slicing :85-110,
_latents_to_image :112-124, __call__ :126-310) with the same call signature, return types
and ValueError, driving the gfx950 kernels.

Device loop: for `SimpleGuide` (and a batched or masked `CompositeGuide`, whose blend + CFG + DDIM
update is one fd_composite_step_f32) + DDIM the whole step is  UNet(NHWC fp16, CFG batch built
inside the layout kernel) -> fused CFG + DDIM update on the fp32 latents  with no host
round trip; any other guide object goes through the reference protocol
(`guide.noise_pred` + `scheduler.step`) unchanged.  The UNet forward of the fused loop is
replayed from a captured HIP GRAPH (`use_graph`, default: one host call per denoising step;
the mode `bench.py` measures) and, if capture fails on a box, from a LAUNCH PLAN (`use_plan`):
its ~310 C-ABI launches recorded once per (shape, context) and re-issued each step by one
library call -- the same eager launches in the same order, without the Python front's per-op
work.  Same kernels, same order, bit-identical results in all three modes.

DPM-Solver++ (`DPMSolverMultistepScheduler`, beyond the reference's pinned diffusers): SimpleGuide runs the same device
loop with fd_cfg_multistep_step_f32 as its one launch after the UNet (CFG, x0, history write, second-order multistep
update, and the known-region blend of a masked request).

PLMS and K-LMS (`PNDMScheduler` -- what the reference's Runner passes, utils.py:70 -- and `LMSDiscreteScheduler`): SimpleGuide
with the graph or the plan on runs the device loop with fd_cfg_linear_multistep_step_f32 as its one launch after the UNet
(`fused_lin`: CFG, the history write, the linear multistep update, the known-region blend of a masked request; under K-LMS the
launch also writes the next step's sigma-scaled model input into the persistent buffer, the unscaled latents being a tensor of
the call's own).  `fuse_linear_multistep = False`, guidance rescale, `debug=True` or a WindowedGuide keep
the planned route below; with neither graph nor plan the reference protocol runs.  The same bits on all of them.

Composition under every scheduler (`fuse_composite`, default True): every CompositeGuide whose `noise_pred` is the class's own --
batch 1 with plain rectangles included -- runs on these loops with the entity blend as the source of the guided prediction inside
the step's one launch: fd_composite_ddim_step_f32 (DDIM with a mask image, or eta > 0 on `pipe.step_noise`),
fd_composite_multistep_step_f32 (DPM-Solver++ and its SDE form, `scheduler.fused_composite_step`),
fd_composite_linear_multistep_step_f32 (PLMS and K-LMS, `scheduler.fused_step(entities=)`).  False restores the earlier routes:
the device loop for a batched or masked composite under DDIM at eta = 0 only (+ a blend-only launch with a mask image), the
planned route under every other scheduler, `guide.noise_pred` for batch 1.  The route table is DESIGN.md sec. 7.4.

Masked img2img (`mask_image=`, beyond the reference; pipeline/inpaint.py): after every step the kept
region of the latents is put back on the re-noised init latents -- inside the fused step's own launch
(fd_cfg_ddim_masked_step_f32) on the SimpleGuide + DDIM loop, by one blend-only launch after the step
everywhere else.  Without a mask no path changes.

Context schedules (beyond the reference; ctx_schedule.py): a guide with `at_step` (ScheduledGuide, a CompositeGuide with
`style_linear=`) is told the global step index `t_start + i` at the top of every iteration, on every route, and makes the
UNet's cached cross-attention projections those of the step's blend of its keyframe contexts -- one fd_lerp_f16 on the
loop's stream before the graph / plan replay.  Guides without it run unchanged.

Stochastic sampling (`pipe.step_noise`, a `noise.PhiloxNoise`; beyond the reference, which forwards `eta` to its scheduler,
pipeline/flex.py:247-251): with it, SimpleGuide + DDIM + `eta > 0` stays on the device loop -- one fd_cfg_ddim_noise_step_f32 per
step, the noise a counter-based stream generated inside the kernel -- and `DPMSolverMultistepSDEScheduler` runs the multistep
loop with fd_cfg_multistep_noise_step_f32; every other route hands the stream's address to `scheduler.step(step_noise=)`.  The
result depends on (seed, global sample index, step) only: not on the loop mode, the batch split or the rank count.  Without
`step_noise`, `eta > 0` is the generator route as before.

Guidance rescale (`guide.guidance_rescale`, beyond the reference; Lin et al. 2023 sec. 3.4): the guided output of each sample is
scaled by a factor from two of its standard deviations, inside the step's own launch (fd_cfg_rescale_ddim_step_f32,
fd_cfg_rescale_multistep_step_f32) on the fused loops and by the combine-only form of the first on the planned and generic
routes -- the same bits on every route.  With 0 every route makes the calls it made before.

Windowed sampling (`WindowedGuide`, beyond the reference; MultiDiffusion, Bar-Tal et al. 2023; windows.py): a canvas larger than
the model's size is covered by overlapping windows, the UNet runs on all of them as one batch -- the loop's persistent buffer,
through the graph / plan -- and ONE launch per step combines, averages, takes the step on the canvas and writes the next window
batch: fd_window_step_f32 (DDIM, eta = 0), fd_window_ddim_step_f32 (a masked request's known-region blend and, with
`pipe.step_noise`, DDIM's eta > 0 term in that launch), fd_window_multistep_step_f32 (DPM-Solver++ and its SDE form, masked or
not).  The step noise is addressed by the canvas element (draw = t_start + i), never by the window grid.  PNDM, K-LMS and DDIM
with eta > 0 on generator noise take a planned route: one fd_window_gather_f32 into the persistent window batch, the graph /
plan replay, the combine-only form, `scheduler.step`, the blend-only launch of a masked request -- the bits of the loop over
`guide.noise_pred`, which remains the route of `debug=True` and of a pipeline with neither graph nor plan.

fd_cfg_ddim_step_f32, fd_cfg_ddim_masked_step_f32 and fd_cfg_multistep_step_f32 (and their two noise forms) are one kernel (csrc/step.hip) over one
statement of the step arithmetic (csrc/latent_step.h), which fd_composite_step_f32 calls too: the paths above are bit-equal
wherever they compute the same thing.

Deliberate differences: E6 initial noise is drawn on the generator's own
device -- pass a CPU generator for results independent of the GPU count; E8 `init_image`
is tested with `is not None`.
'''
from __future__ import annotations

import contextlib
import gc
import inspect
import warnings
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .. import hip, ops
from ..encode.clip import preprocess
from ..noise import PhiloxNoise
from ..scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler, LMSDiscreteScheduler,
                         PNDMScheduler)
from .guide import GuideBase, SimpleGuide, WindowedGuide, check_guidance_rescale
from .inpaint import image_size, known_coefficients, latent_mask, start_level

VAE_SCALE = 0.18215


@contextlib.contextmanager
def _gc_paused():
    was = gc.isenabled()
    if was:
        gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class StableDiffusionPipelineOutput():
    def __init__(self, images, nsfw_content_detected):
        self.images = images
        self.nsfw_content_detected = nsfw_content_detected

    def __getitem__(self, key):
        if key in ('sample', 'images', 0):
            return self.images
        if key in ('nsfw_content_detected', 1):
            return self.nsfw_content_detected
        raise KeyError(key)


class FlexPipeline():
    # PLMS / K-LMS under a SimpleGuide with graph or plan on: the step is the scheduler's one-launch `fused_step`
    # (fd_cfg_linear_multistep_step_f32).  False (on the class or an instance): the planned route, the combine-only launch +
    # `scheduler.step` -- the same bits
    fuse_linear_multistep = True
    # CompositeGuide on the device loop under every scheduler: any CompositeGuide (batch 1 with plain rectangles included) reads
    # the graph / plan and the request's time-embedding table, and its step -- the entity blend, CFG, the update, the step noise,
    # the history write, the known-region blend -- is ONE launch (fd_composite_step_f32, fd_composite_ddim_step_f32,
    # fd_composite_multistep_step_f32, fd_composite_linear_multistep_step_f32).  False (on the class or an instance): only a
    # batched or masked composite under DDIM (eta = 0) steps on the device, with a second blend-only launch for a masked
    # request; every other scheduler takes the planned route and batch 1 `guide.noise_pred` -- the same bits
    fuse_composite = True

    def __init__(self, vae, clip, tokenizer, unet, scheduler):
        scheduler = scheduler.set_format('pt')
        # pipeline/flex.py:57-70: a scheduler config that HAS a steps_offset other than 1 is rewritten
        # to 1 (with a DeprecationWarning) through the scheduler's `_internal_dict`
        cfg = scheduler.config
        if hasattr(cfg, 'steps_offset') and cfg['steps_offset'] != 1:
            warnings.warn(f'The configuration file of this scheduler: {scheduler} is outdated. '
                          f'`steps_offset` should be set to 1 instead of {cfg["steps_offset"]}.',
                          DeprecationWarning)
            fixed = dict(cfg)
            fixed['steps_offset'] = 1
            setattr(scheduler, '_internal_dict', type(cfg)(fixed))
        self.vae = vae
        self.clip = clip
        self.tokenizer = tokenizer
        self.unet = unet
        self.scheduler = scheduler
        self.device = getattr(unet, 'device', torch.device('cuda'))
        self.last_latents: Optional[torch.Tensor] = None
        self.last_images: Optional[torch.Tensor] = None
        # default: replay the UNet forward of the fused loop from a captured HIP graph -- one host call per step, so a
        # host stall cannot starve the device; 0.3-0.6 % faster per forward than the launch plan on the 311-launch
        # forward (profiles/r04_session_ab.txt sec. 2).  If capture fails, `_unet_eps` switches this pipeline to the
        # launch plan (`graph_fallback` says why).
        self.use_graph = True
        self.graph_fallback: Optional[str] = None
        self._graphs = {}
        self._lat_bufs = {}
        # the launch plan (hip.Plan): identical kernels / order / results to the eager front, ~1/5 of its host time;
        # used when use_graph is off or fell back
        self.use_plan = True
        self._plans = {}
        # (timestep -> row, [steps][sum Cout] table) of the ResBlocks' time-embedding biases for the running request's timesteps
        self._temb_tab = None
        # opt-in (bench.py, Runner(pause_gc=True)): keep the cyclic GC off across the denoising loop.
        # Off by default: a drop-in must not change interpreter-global state of someone else's process.
        self.pause_gc = False
        # opt-in: the address of the request's step noise (noise.PhiloxNoise).  With it `eta > 0` under DDIM runs on the
        # fused loop and every scheduler that takes `step_noise=` draws from the counter-based stream; None: the
        # generator route (an SDE scheduler then derives one from the call's generator seed)
        self.step_noise: Optional[PhiloxNoise] = None

    @classmethod
    def from_pretrained(cls, sd_dir, clip_dir=None, tokenizer_dir=None, preset: str = 'sd15',
                        device='cuda', scheduler=None, text_cleanup: str = 'basic', **_):
        '''Local files only (there is no hub access): `sd_dir` is a diffusers-layout checkpoint
        directory (unet/, vae/, optionally tokenizer/), `clip_dir` a CLIPModel directory -- what the
        reference's `Runner.__init__` obtains from the hub (utils.py:59-71).  See
        `flexdiffuse_amd.build.from_directories`.'''
        from .. import build
        return build.from_directories(sd_dir, clip_dir, tokenizer_dir, preset=preset, device=device,
                                      scheduler=scheduler, text_cleanup=text_cleanup)[0]

    def to(self, device):
        self.device = torch.device(device)
        return self

    def progress_bar(self, iterable):
        return iterable

    @staticmethod
    def numpy_to_pil(images: np.ndarray):
        from PIL import Image
        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype('uint8')
        return [Image.fromarray(image) for image in images]

    def enable_attention_slicing(self, slice_size: Optional[Union[str, int]] = 'auto'):
        if slice_size == 'auto':
            slice_size = self.unet.config['attention_head_dim'] // 2
        self.unet.set_attention_slice(slice_size)

    def disable_attention_slicing(self):
        self.enable_attention_slicing(None)

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        '''latents -> device image tensor (B,3,H,W) fp32 in [0,1] (pipeline/flex.py:117-120).'''
        img = self.vae.decode_nhwc(latents, scale=1.0 / VAE_SCALE)
        return ops.nhwc_to_nchw(img.t, img.B, 3, img.H, img.W, 0.5, 0.5, True)

    def _decode_generic(self, latents: torch.Tensor) -> torch.Tensor:
        '''pipeline/flex.py:116-120 for any object with the diffusers surface `decode(z).sample`
        (NCHW): scale, decode, (x/2 + 0.5).clamp(0, 1) -- the affine + clamp on the library's layout
        kernel with the NCHW tensor read as B*C one-channel maps.'''
        z = ops.axpby(latents.to(self.device, torch.float32), None, 1.0 / VAE_SCALE, 0.0)
        image = self.vae.decode(z).sample.to(torch.float32).contiguous()
        B, C, H, W = image.shape
        return ops.nhwc_to_nchw(image.view(-1, 1), B * C, 1, H, W, 0.5, 0.5, True).view(B, C, H, W)

    def _latents_to_image(self, latents: torch.Tensor, pil: bool = True):
        image = self.decode_latents(latents) if hasattr(self.vae, 'decode_nhwc') \
            else self._decode_generic(latents)
        self.last_images = image
        image = image.cpu().permute(0, 2, 3, 1).numpy()
        if pil:
            return self.numpy_to_pil(image)
        return image

    def _temb_row(self, t) -> torch.Tensor:
        '''[1][sum Cout] fp32 time-embedding biases of timestep t: a row of the table the running request computed for all of its
        timesteps at once (`__call__`), or computed here for a timestep outside it.'''
        tab = self._temb_tab
        if tab is not None:
            i = tab[0].get(float(t))
            if i is not None:
                return tab[1][i:i + 1]
        return self.unet.time_bias(float(t), 1)

    def _unet_eps(self, latents: torch.Tensor, t: int, ctx: torch.Tensor, rep: int) -> torch.Tensor:
        '''UNet noise prediction (NHWC fp32) for the fused loop; graph-replayed when enabled.
        `latents` must be the loop's persistent buffer (updated in place by the DDIM kernel).  The time embedding does not
        depend on the latents: the replayed forward reads the ResBlocks' time biases from a persistent buffer that is refreshed
        per step from the request's table (`_temb_row`) -- the three time-embedding GEMMs are not part of the step.'''
        # (per-launch event timing -- bench.py's roofline leg -- cannot see inside a graph: it replays the launch plan,
        # the same kernels in the same order issued by one host call)
        if (self.use_plan and not self.use_graph) or (self.use_graph and hip.prof_is_on()):
            return self._unet_eps_plan(latents, t, ctx, rep)
        Be = latents.shape[0] * rep
        if not self.use_graph:
            return self.unet.forward_nhwc(latents, t, ctx, rep=rep, temb=self._temb_row(t).expand(Be, -1).contiguous())
        self.unet.set_context(ctx)               # eager, in place: the graph reads these buffers
        # ctx_generation changes when the UNet had to reallocate its cached K / V^T (a call with
        # another context shape in between): a graph captured before that reads freed memory
        key = (latents.data_ptr(), tuple(latents.shape), rep, tuple(ctx.shape),
               getattr(self.unet, 'ctx_generation', 0))
        entry = self._graphs.get(key)
        row = self._temb_row(t)
        if entry is None:
            self._graphs = {}                    # drop the previous graph (its private pool holds GBs) before capturing another
            temb_static = torch.empty((Be, row.shape[1]), dtype=torch.float32, device=latents.device)
            # the first call runs eagerly (lazy one-time setup inside the kernels' launchers),
            # the second is captured
            temb_static.copy_(row.expand_as(temb_static))
            self.unet.forward_nhwc(latents, t, ctx, rep=rep, temb=temb_static)
            torch.cuda.synchronize()
            try:
                graph = torch.cuda.CUDAGraph()
                # thread_local: only THIS thread's calls are checked against the capture -- a process-group watchdog
                # thread (RCCL, N > 1) polling its events must not invalidate it
                with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                    eps = self.unet.forward_nhwc(latents, t, ctx, rep=rep, temb=temb_static)
            except Exception as ex:      # noqa: BLE001 -- capture is an optimisation: never fail the request over it
                self.graph_fallback = f'HIP-graph capture failed ({type(ex).__name__}: {str(ex)[:200]}); running on the launch plan'
                warnings.warn(self.graph_fallback, RuntimeWarning)
                self.use_graph, self.use_plan, self._graphs = False, True, {}
                try:                     # a stream left in (or invalidated by) the failed capture must not fail the request either
                    if not torch.cuda.is_current_stream_capturing():
                        torch.cuda.synchronize()
                except Exception:        # noqa: BLE001
                    pass
                return self._unet_eps_plan(latents, t, ctx, rep)
            entry = (graph, temb_static, eps, ctx)
            self._graphs = {key: entry}          # keep one graph (its pool holds GBs)
        graph, temb_static, eps, ctx_ref = entry
        temb_static.copy_(row.expand_as(temb_static))
        graph.replay()
        return eps

    def _unet_eps_plan(self, latents: torch.Tensor, t: int, ctx: torch.Tensor, rep: int) -> torch.Tensor:
        '''The UNet forward through its launch plan.  `latents` is the loop's persistent buffer; the ResBlocks' time biases
        live in a persistent buffer refreshed before every replay (`_temb_row`); the context's
        K / V^T are (re)projected eagerly, in place, before the replay.  The recording run executes
        inside a private torch memory pool that the plan entry keeps alive, so every intermediate
        address the recorded launches use stays reserved for them.'''
        self.unet.set_context(ctx)
        key = (latents.data_ptr(), tuple(latents.shape), rep, tuple(ctx.shape),
               getattr(self.unet, 'ctx_generation', 0), hip.stream().value)
        entry = self._plans.get(key)
        row = self._temb_row(t)
        if entry is None:
            self._plans = {}                     # one plan at a time (its pool holds the activations)
            temb_dev = torch.empty((latents.shape[0] * rep, row.shape[1]), dtype=torch.float32, device=latents.device)
            temb_dev.copy_(row.expand_as(temb_dev))
            # first call eager: one-time setup inside the launchers, scratch buffers of ops.py
            self.unet.forward_nhwc(latents, t, ctx, rep=rep, temb=temb_dev)
            if self.unet.ctx_generation != key[4]:
                key = key[:4] + (self.unet.ctx_generation,) + key[5:]
            pool = torch.cuda.MemPool()
            plan = hip.Plan()
            with torch.cuda.use_mem_pool(pool, device=latents.device), plan.record():
                eps = self.unet.forward_nhwc(latents, t, ctx, rep=rep, temb=temb_dev)
            self._plans = {key: (plan, temb_dev, eps, pool, len(plan))}
            return eps                           # the recording run also executed
        plan, temb_dev, eps = entry[:3]
        temb_dev.copy_(row.expand_as(temb_dev))
        plan.replay()
        return eps

    def plan_launches(self):
        '''Recorded launches of the current plan (None before the first fused step).'''
        for e in self._plans.values():
            return e[4]
        return None

    def loop_latents(self, latents: torch.Tensor) -> torch.Tensor:
        '''The persistent per-shape latent buffer of the fused loop, filled with `latents` (a captured
        graph / recorded plan reads this address every step).'''
        latents = latents.to(self.device, torch.float32)
        buf = self._lat_bufs.get(tuple(latents.shape))
        if buf is None:
            buf = torch.empty_like(latents)
            self._lat_bufs = {tuple(latents.shape): buf}
        buf.copy_(latents)
        return buf

    def _randn(self, shape, generator):
        gdev = getattr(generator, 'device', torch.device('cpu')) if generator is not None \
            else torch.device('cpu')
        return torch.randn(shape, generator=generator, device=gdev,
                           dtype=torch.float32).to(self.device)

    @torch.no_grad()
    def __call__(self,
                 guide: GuideBase,
                 init_image=None,
                 init_size: Tuple[int, int] = (512, 512),
                 strength: float = 0.6,
                 eta: float = 0.0,
                 generator: Optional[torch.Generator] = None,
                 output_type: str = 'pil',
                 return_dict: bool = True,
                 debug: bool = False,
                 latents: Optional[torch.Tensor] = None,
                 noise: Optional[torch.Tensor] = None,
                 mask_image=None):
        '''Arguments and defaults of pipeline/flex.py:127-137, plus two optional tensors for sharded
        runs (flexdiffuse_amd.dist): `latents` -- txt2img initial latents (B,4,h,w) instead of the
        pipeline's own randn; `noise` -- img2img add_noise rows (B,4,h,w) instead of its own randn
        (the rank's rows of the global batch's draw, `dist.global_img2img_noise`).

        `mask_image` (beyond the reference; needs `init_image`): masked img2img / inpainting.  A 2-D map over the
        init image in image pixels (array-like, tensor, or PIL image resized like the init image), 1 = repaint,
        0 = keep, shared by the samples of the call.  Reduced to latent resolution (`inpaint.latent_mask`); after
        every scheduler step the kept region of the latents is put back on the clean init latents re-noised with
        the call's own noise to the step's level (`inpaint.known_coefficients`), on the last step on the clean init
        latents themselves.  The image is the VAE decode of the blended latents: pasting the original pixels back
        over the kept region is out of scope, as are per-sample masks and feathering helpers.'''
        if strength < 0 or strength > 1:
            raise ValueError(
                f'The value of strength should in [0.0, 1.0] but is {strength}')
        if mask_image is not None and init_image is None:
            raise ValueError('mask_image needs an init_image: the mask says which part of it to keep')
        # guidance rescale: the guide's attribute, checked before any launch; 0 keeps every route on its calls
        rescale = float(getattr(guide, 'guidance_rescale', 0.0) or 0.0)
        if rescale:
            check_guidance_rescale(rescale, guide.guidance)
        batch_size = guide.batch_size
        self.scheduler.set_timesteps(guide.steps)
        assert self.scheduler.timesteps is not None

        if init_image is not None:
            if mask_image is not None:
                mask_hw = image_size(init_image)
            if not isinstance(init_image, torch.Tensor):
                init_image = preprocess(init_image)
            init_image = init_image.to(self.device)
            dist = self.vae.encode(init_image).latent_dist
            init_latents = dist.sample(generator=generator)
            init_latents = ops.axpby(init_latents, None, VAE_SCALE, 0.0)
            init_latents = torch.cat([init_latents] * batch_size)
            offset = self.scheduler.config.get('steps_offset', 0)
            init_timestep = int(guide.steps * strength) + offset
            init_timestep = min(init_timestep, guide.steps)
            if isinstance(self.scheduler, LMSDiscreteScheduler):
                t_noise = guide.steps - init_timestep     # pipeline/flex.py:200-204: an index
            else:
                t_noise = int(self.scheduler.timesteps[-init_timestep])
            # one level per sample, as a long tensor (pipeline/flex.py:201-209); built on the host
            t_noise = torch.tensor([t_noise] * batch_size, dtype=torch.long)
            noise = self._randn(init_latents.shape, generator) if noise is None \
                else noise.to(self.device, torch.float32)
            if tuple(noise.shape) != tuple(init_latents.shape):
                raise ValueError(f'noise {tuple(noise.shape)} does not match the latents {tuple(init_latents.shape)}')
            if mask_image is not None:
                # z0 and n stay alive for the loop; add_noise returns a new tensor, so neither aliases the latents
                mask_z0, mask_n = init_latents.to(torch.float32).contiguous(), noise.contiguous()
                h, w = mask_z0.shape[-2:]
                if mask_hw[0] % h or mask_hw[1] % w or mask_hw[0] // h != mask_hw[1] // w:
                    raise ValueError(f'init image {mask_hw} is not a whole multiple of its latents {(h, w)}')
                # uploaded once per call, as z0 and n are
                mask_dev = latent_mask(mask_image, mask_hw[0], mask_hw[1], mask_hw[0] // h).to(self.device)
                mask_start = start_level(self.scheduler, int(t_noise[0]))
            init_latents = self.scheduler.add_noise(init_latents, noise, t_noise)
            t_start = max(guide.steps - init_timestep + offset, 0)
        else:
            height, width = init_size
            channels = self.unet.in_channels
            shape = (batch_size, channels, height // 8, width // 8)
            init_latents = self._randn(shape, generator) if latents is None \
                else latents.to(self.device, torch.float32).clone()
            self.scheduler.set_timesteps(guide.steps)
            if isinstance(self.scheduler, LMSDiscreteScheduler):   # pipeline/flex.py:236-238
                init_latents = ops.axpby(init_latents, None, float(self.scheduler.sigmas[0]), 0.0)
            t_start = 0

        accepts_eta = 'eta' in set(inspect.signature(self.scheduler.step).parameters.keys())
        extra_step_kwargs = {'eta': eta} if accepts_eta else {}

        latents = init_latents.contiguous()
        all_latents = [init_latents] if debug else None
        from ..composition.guide import CompositeGuide
        # CompositeGuide: blend + CFG + the scheduler's update in one launch per step after the UNet forward over its E context
        # blocks (`fuse_composite` off: batched samples or masks only, the batch-1 rectangle path on the generic protocol)
        comp_fused = bool(self.fuse_composite)
        comp = (type(guide).noise_pred is CompositeGuide.noise_pred and (comp_fused or getattr(guide, 'on_device', False))
                and hasattr(self.unet, 'forward_nhwc'))
        comp_fused = comp_fused and comp
        simple = type(guide).noise_pred is SimpleGuide.noise_pred
        device_guide = simple or comp
        # WindowedGuide: a canvas of any size on the UNet's own window size.  The window batch is the loop's persistent buffer,
        # the canvas an ordinary tensor.  DDIM (eta = 0, or eta > 0 on the counter-based stream) and DPM-Solver++ (ODE and
        # SDE): a step is the UNet replay + ONE launch (win_fused, below); every other scheduler: the planned route (gather,
        # replay, combine-only, scheduler.step), or with debug / without graph and plan the generic branch through
        # guide.noise_pred
        win = type(guide).noise_pred is WindowedGuide.noise_pred and hasattr(self.unet, 'forward_nhwc')
        if win and rescale:
            raise ValueError('WindowedGuide does not support guidance_rescale')
        rescale = rescale if simple else 0.0     # any other guide applies (or ignores) its own attribute in its noise_pred
        # the step noise of the request: the pipeline's attribute; an SDE scheduler without one gets the generator's seed
        step_noise = self.step_noise
        sde = isinstance(self.scheduler, DPMSolverMultistepSDEScheduler)
        if sde and step_noise is None:
            step_noise = PhiloxNoise(generator.initial_seed() if generator is not None else 0)
        # eta > 0 stays fused for SimpleGuide when the noise comes from the counter-based stream (fd_cfg_ddim_noise_step_f32)
        # (and for a CompositeGuide: fd_composite_ddim_step_f32)
        noisy = bool(eta) and step_noise is not None and (simple or comp_fused)
        # the windowed device loop: DDIM (its eta > 0 term from the stream, win_noisy) or the multistep solver (win_ms)
        win_ms = win and isinstance(self.scheduler, DPMSolverMultistepScheduler)
        win_noisy = win and bool(eta) and step_noise is not None and isinstance(self.scheduler, DDIMScheduler)
        win_fused = win_ms or win_noisy or (win and isinstance(self.scheduler, DDIMScheduler) and not eta)
        fused = (device_guide
                 and isinstance(self.scheduler, DDIMScheduler) and (not eta or noisy)
                 and hasattr(self.unet, 'forward_nhwc'))
        # SimpleGuide + DPM-Solver++: the same loop, its step (CFG, x0, history, multistep update, known-region blend) one
        # fd_cfg_multistep_step_f32 launch (the SDE form: fd_cfg_multistep_noise_step_f32); `eta` does not apply to it
        # (a CompositeGuide: fd_composite_multistep_step_f32, the entity blend ahead of the CFG combine)
        fused_ms = ((simple or comp_fused) and isinstance(self.scheduler, DPMSolverMultistepScheduler)
                    and hasattr(self.unet, 'forward_nhwc'))
        # generic and planned routes: a scheduler that takes it draws from the stream at (noise, t_start + i)
        takes_noise = step_noise is not None and 'step_noise' in inspect.signature(self.scheduler.step).parameters
        B, C, H, W = latents.shape
        # SimpleGuide with ANY other scheduler (PNDM -- what the reference's Runner passes, utils.py:70 -- LMS, DDIM with
        # eta): the UNet forward still comes from the launch plan / graph; only the scheduler arithmetic stays generic
        planned = (not fused and not fused_ms and device_guide and hasattr(self.unet, 'forward_nhwc')
                   and (self.use_graph or self.use_plan) and not debug)
        is_lms = isinstance(self.scheduler, LMSDiscreteScheduler)
        # SimpleGuide + PLMS / K-LMS on that route: the step (CFG, history write, linear multistep update, known-region blend,
        # K-LMS's next scaled input) is one fd_cfg_linear_multistep_step_f32 launch through `scheduler.fused_step`
        # (a CompositeGuide: fd_composite_linear_multistep_step_f32)
        fused_lin = (planned and (simple or comp_fused) and not rescale and self.fuse_linear_multistep
                     and isinstance(self.scheduler, (PNDMScheduler, LMSDiscreteScheduler)))
        planned = planned and not fused_lin
        # WindowedGuide with any scheduler the windowed loop does not step itself: the same route over the window batch
        win_planned = win and not win_fused and (self.use_graph or self.use_plan) and not debug
        if (fused or fused_ms) and (self.use_graph or self.use_plan) and not debug:
            # persistent latent buffer: the captured UNet graph / recorded plan reads this address
            latents = self.loop_latents(latents)
        lin_scale = lambda j: 1.0 / ((float(self.scheduler.sigmas[j]) ** 2 + 1) ** 0.5)   # noqa: E731 -- pipeline/flex.py:270-274
        if fused_lin and is_lms:
            # K-LMS: the persistent buffer holds the SCALED model input (what the graph / plan reads), written by every step's
            # launch for the next one and by one axpby for the first; the unscaled latents are a tensor of this call's own
            latents = latents.to(self.device, torch.float32).clone()
            lin_input = self.loop_latents(ops.axpby(latents, None, lin_scale(t_start), 0.0))
        elif fused_lin:
            # PLMS: the latents live in the persistent buffer and are stepped in place
            latents = self.loop_latents(latents)
        known = known_coefficients(self.scheduler, self.scheduler.timesteps, t_start, mask_start) if mask_image is not None else None
        self._temb_tab = None
        if (fused or fused_ms or fused_lin or planned or win_fused or win_planned) and hasattr(self.unet, 'time_bias_table'):
            # the time embedding depends on t only: all of the request's timesteps in one pass (three GEMMs over len(timesteps) rows)
            # instead of three GEMMs per step
            ts = [float(t) for t in self.scheduler.timesteps[t_start:]]
            keys = {}
            for t in ts:
                keys.setdefault(t, len(keys))
            self._temb_tab = (keys, self.unet.time_bias_table(list(keys)))
        # loop-invariant: the CFG switch and the UNet's batch replication of a device guide, DDIM's prediction type
        cfg = guide.classifier_free_guidance if device_guide else None
        rep = guide.rep if comp or win else 2 if cfg else 1
        vpred = (fused or win_fused) and self.scheduler.config['prediction_type'] == 'v_prediction'
        # the composite's weight maps [n][HW] as the schedulers' fused steps take them, built once per latent size (a SimpleGuide:
        # no keyword, today's call argument for argument)
        ent = {'entities': guide.entity_rows(H, W)} if comp_fused else {}
        if win_fused or win_planned:
            # the window batch: the one persistent buffer (what the graph / plan reads); the canvas does not evict it
            grid = guide.bind(H, W)
            wshape = (B * grid.count, C, grid.h, grid.w)
            wins = self._lat_bufs.get(wshape)
            if wins is None:
                wins = torch.empty(wshape, dtype=torch.float32, device=latents.device)
                self._lat_bufs = {wshape: wins}
            guide.gather(latents, wins)

        # a guide with a context schedule (ScheduledGuide, CompositeGuide(style_linear=)): told the GLOBAL step index at the top of
        # every iteration, on every route; guides without `at_step` run as before
        at_step = getattr(guide, 'at_step', None)

        def blend_known(x, i):
            # masked img2img behind any scheduler / guide: the blend-only launch on the step's result
            ops.cfg_ddim_masked_step(x, None, mask_z0, mask_n, mask_dev, B, C, H * W, k1=known[i][0], k2=known[i][1])
        # The host only has to stay ahead of the device queue.  A generation-2 collection of the
        # cyclic GC walks every tracked object of the process (~175 k with the SD1.5 weights:
        # ~40 ms) and drains that queue, so collections wait until the images are decoded.
        with (_gc_paused() if self.pause_gc else contextlib.nullcontext()):
            for i, t in enumerate(self.progress_bar(self.scheduler.timesteps[t_start:])):
                if at_step is not None:
                    # a context schedule: the step's blend, issued eagerly on the loop's stream before the graph / plan replay reads it
                    at_step(t_start + i)
                if fused:
                    if debug:
                        # (a composite reads the request's time-bias table as the graph / plan do: bit-equal to them)
                        temb = self._temb_row(int(t)).expand(B * rep, -1).contiguous() if comp and self._temb_tab else None
                        eps = self.unet.forward_nhwc(latents, int(t), guide.stacked_embeds(),
                                                     rep=rep, temb=temb)
                    else:
                        eps = self._unet_eps(latents, int(t), guide.stacked_embeds(), rep)
                    coef = self.scheduler.step_coefficients(int(t), eta if noisy else 0.0)
                    sigma, coef = coef[4], coef[:4]
                    if debug:
                        latents = latents.clone()
                    if rescale:
                        # CFG + rescale + DDIM update (+ sigma z, + the known-region blend) in one launch
                        blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                        ops.cfg_rescale_ddim_step(latents, eps, B, C, H * W, guide.guidance, rescale, coef, vpred, mask=blend,
                                                  sigma=float(sigma) if noisy else 0.0, noise=step_noise if noisy else None,
                                                  draw=t_start + i)
                    elif comp_fused and (noisy or known is not None):
                        # entity blend + CFG + DDIM update + sigma z + the known-region blend of a masked request in one launch
                        blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                        guide.step(latents, eps, coef, vpred, mask=blend, sigma=float(sigma) if noisy else 0.0,
                                   step_noise=(step_noise, t_start + i) if noisy else None)
                    elif noisy:
                        # CFG + DDIM update + sigma z (+ the known-region blend of a masked request) in one launch
                        blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                        ops.cfg_ddim_noise_step(latents, eps, B, C, H * W, cfg, guide.guidance, coef, vpred, float(sigma),
                                                step_noise, C * H * W, t_start + i, blend)
                    elif comp:
                        guide.step(latents, eps, coef, vpred)
                        if known is not None:
                            blend_known(latents, i)
                    elif known is not None:
                        # CFG + DDIM update + known-region blend in the one launch of the unmasked step
                        ops.cfg_ddim_masked_step(latents, eps, mask_z0, mask_n, mask_dev, B, C, H * W, cfg,
                                                 guide.guidance, coef, vpred, known[i][0], known[i][1])
                    else:
                        ops.cfg_ddim_step(latents, eps, B, C, H * W, cfg, guide.guidance, coef, vpred)
                elif fused_ms:
                    if debug:
                        # (a composite reads the request's time-bias table, as on the DDIM loop; a SimpleGuide: the call as it was)
                        temb = {'temb': self._temb_row(int(t)).expand(B * rep, -1).contiguous()} if comp and self._temb_tab else {}
                        eps = self.unet.forward_nhwc(latents, int(t), guide.stacked_embeds(), rep=rep, **temb)
                        latents = latents.clone()
                    else:
                        eps = self._unet_eps(latents, int(t), guide.stacked_embeds(), rep)
                    # masked img2img: the blend rides in the step's launch
                    blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                    if rescale:
                        self.scheduler.fused_rescale_step(latents, eps, int(t), B, C, H * W, guide.guidance, rescale, blend,
                                                          (step_noise, t_start + i) if sde else None)
                    elif comp:
                        # the entity blend ahead of the CFG combine, in the step's launch
                        self.scheduler.fused_composite_step(latents, eps, int(t), B, C, H * W, cfg, guide.guidance, ent['entities'],
                                                            blend, (step_noise, t_start + i) if sde else None)
                    elif sde:
                        self.scheduler.fused_step(latents, eps, int(t), B, C, H * W, cfg, guide.guidance, blend,
                                                  (step_noise, t_start + i))
                    else:
                        self.scheduler.fused_step(latents, eps, int(t), B, C, H * W, cfg, guide.guidance, blend)
                elif fused_lin:
                    blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                    if is_lms:
                        # the scheduler steps by sigma index; the UNet sees the float timestep and the scaled buffer, which
                        # this step's launch refills for the next one
                        eps = self._unet_eps(lin_input, float(t), guide.stacked_embeds(), rep)
                        last = t_start + i + 1 >= len(self.scheduler.timesteps)
                        self.scheduler.fused_step(latents, eps, t_start + i, B, C, H * W, cfg, guide.guidance, blend,
                                                  scaled_out=None if last else lin_input,
                                                  next_scale=0.0 if last else lin_scale(t_start + i + 1), **ent)
                    else:
                        eps = self._unet_eps(latents, float(t), guide.stacked_embeds(), rep)
                        self.scheduler.fused_step(latents, eps, t, B, C, H * W, cfg, guide.guidance, blend, **ent)
                elif win_fused:
                    if debug:
                        temb = self._temb_row(int(t)).expand(wins.shape[0] * rep, -1).contiguous() if self._temb_tab else None
                        eps = self.unet.forward_nhwc(wins, int(t), guide.stacked_embeds(), rep=rep, temb=temb)
                        latents = latents.clone()
                    else:
                        eps = self._unet_eps(wins, int(t), guide.stacked_embeds(), rep)
                    # CFG per window, the average, the update of the canvas, the step noise, the known-region blend of a masked
                    # request and the next window batch (of the blended canvas) in one launch
                    blend = None if known is None else (mask_z0, mask_n, mask_dev, known[i][0], known[i][1])
                    if win_ms:
                        self.scheduler.fused_window_step(latents, wins, eps, int(t), B, C, grid.args, guide.blend_code,
                                                         guide.classifier_free_guidance, guide.guidance, blend,
                                                         (step_noise, t_start + i) if sde else None)
                    else:
                        coef = self.scheduler.step_coefficients(int(t), eta if win_noisy else 0.0)
                        guide.step(latents, wins, eps, coef[:4], vpred, mask=blend, sigma=float(coef[4]) if win_noisy else 0.0,
                                   step_noise=(step_noise, t_start + i) if win_noisy else None)
                else:
                    t_index, model_input = t, latents
                    if is_lms:        # pipeline/flex.py:270-274: continuous-ODE input scaling
                        t_index = t_start + i
                        sigma = float(self.scheduler.sigmas[t_index])
                        model_input = ops.axpby(latents, None, 1.0 / ((sigma ** 2 + 1) ** 0.5), 0.0)
                    if planned:
                        eps = self._unet_eps(self.loop_latents(model_input), float(t), guide.stacked_embeds(), rep)
                        noise_pred = torch.empty((B, C, H, W), dtype=torch.float32, device=latents.device)
                        if comp:
                            guide.step(None, eps, eps_out=noise_pred)
                        elif rescale:
                            ops.cfg_rescale_ddim_step(None, eps, B, C, H * W, guide.guidance, rescale, do_step=False,
                                                      eps_out=noise_pred)
                        else:
                            ops.cfg_ddim_step(None, eps, B, C, H * W, cfg, guide.guidance, do_step=False, eps_out=noise_pred)
                    elif win_planned:
                        # guide.noise_pred with the UNet forward from the graph / plan: gather into the persistent window batch,
                        # replay, the combine-only form of the windowed step
                        guide.gather(model_input.to(self.device, torch.float32).contiguous(), wins)
                        eps = self._unet_eps(wins, float(t), guide.stacked_embeds(), rep)
                        noise_pred = torch.empty((B, C, H, W), dtype=torch.float32, device=latents.device)
                        guide.step(None, None, eps, eps_out=noise_pred)
                    else:
                        noise_pred = guide.noise_pred(model_input, t)
                    if takes_noise:
                        extra_step_kwargs['step_noise'] = (step_noise, t_start + i)
                    latents = self.scheduler.step(noise_pred, t_index, latents,
                                                  **extra_step_kwargs).prev_sample
                    if known is not None:
                        # blend the step's own result (not the persistent buffer, which holds the model input)
                        latents = latents.to(self.device, torch.float32).contiguous()
                        blend_known(latents, i)
                if all_latents is not None:
                    all_latents.append(latents)
            # the fused loop ran on the persistent per-shape buffer, which the next call overwrites:
            # hand out a copy, so a caller holding `pipe.last_latents` keeps the values it read
            persistent = any(latents is b for b in self._lat_bufs.values())
            self.last_latents = latents.clone() if persistent else latents

            if all_latents:
                batches = [self._latents_to_image(l, output_type == 'pil') for l in all_latents]
                if isinstance(batches[0], list):
                    batch_images = [im for ib in batches for im in ib]
                else:
                    batch_images = np.concatenate(batches, axis=0)
            else:
                batch_images = self._latents_to_image(latents, output_type == 'pil')

        if not return_dict:
            return (batch_images, False)
        return StableDiffusionPipelineOutput(images=batch_images,
                                             nsfw_content_detected=[False for _ in batch_images])
