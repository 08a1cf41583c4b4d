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

Which loop a request runs -- and which launch its step ends in -- is decided once per request by `route.select_route`; the table
of every route is that module's docstring.  `__call__` is: argument checks, the first latents (`_init_latents`), the route, the
request's state (`_begin`), and a loop that calls ONE step method per iteration (`_step_ddim`, `_step_multistep`, `_step_linear`,
`_step_window`, `_step_generic`).  Beyond the reference, each on every route and with the same bits on all of them:
  - DPM-Solver++ and its SDE form, UniPC, PLMS and K-LMS on the device loop (`fuse_linear_multistep`), the step one launch after the UNet;
  - composition under every scheduler (`fuse_composite`): the entity blend inside the step's one launch;
  - masked img2img (`mask_image=`; pipeline/inpaint.py): after every step the kept region of the latents is put back on the
    re-noised init latents, inside the step's own launch on the device loops, by one blend-only launch after the step elsewhere;
  - context schedules (ctx_schedule.py): a guide with `at_step` is told the global step index `t_start + i` at the top of every
    iteration and makes the UNet's cached cross-attention projections those of the step's blend, before the replay reads them;
  - stochastic sampling (`pipe.step_noise`, a `noise.PhiloxNoise`): the noise is a counter-based stream generated inside the
    step's launch, or handed to `scheduler.step(step_noise=)`; the result depends on (seed, global sample index, step) only.
    Without it `eta > 0` is the generator route, as the reference forwards `eta` to its scheduler (pipeline/flex.py:247-251);
  - guidance rescale (`guide.guidance_rescale`; Lin et al. 2023 sec. 3.4) inside the step's launch or the combine-only launch;
  - windowed sampling (`WindowedGuide`; MultiDiffusion, windows.py): the window batch is the loop's persistent buffer and ONE
    launch per step combines, averages, steps the canvas and writes the next window batch;
  - region composition over windows (`WindowedCompositeGuide`): that loop with E context blocks over the window batch and the
    entity blend, per covering window, inside the same one launch;
  - two-pass hires sampling (`hires`, `from_latents`): a request may start from clean latents, which ONE launch
    (fd_latent_upscale_noise_f32) resamples onto the canvas, noises to the start level and -- on the `window` route -- scatters
    into the window batch; `output_type='latent'` hands the first pass's latents over without a VAE pass.
The step launches of the simple guide are one kernel (csrc/step.hip) over one statement of the step arithmetic
(csrc/latent_step.h), which the composite's launches call too: the routes are bit-equal wherever they compute the same thing.

Deliberate differences: E6 initial noise is drawn on the generator's own
device -- pass a CPU generator for results independent of the GPU count; E8 `init_image`
is tested with `is not None`.
'''
from __future__ import annotations

import contextlib
import gc
import warnings
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from .. import hip, ops
from ..encode.clip import preprocess
from ..noise import STREAM_INIT, PhiloxNoise
from ..scheduler import LMSDiscreteScheduler
from .guide import GuideBase, check_guidance_rescale
from .inpaint import image_size, known_coefficients, latent_mask, start_level
from .route import Route, select_route

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


class Known():
    '''The kept region of a masked img2img request: the clean init latents, the call's noise, the latent mask and the per-step
    (k1, k2) of `inpaint.known_coefficients`.'''
    def __init__(self, z0, noise, mask, coef):
        self.z0, self.noise, self.mask, self.coef = z0, noise, mask, coef

    def at(self, i):
        '''(z0, noise, mask, k1, k2) of step i, as the step wrappers take their `mask`.'''
        return (self.z0, self.noise, self.mask, self.coef[i][0], self.coef[i][1])


class _Request():
    '''What the step methods read, fixed before the loop (`FlexPipeline._begin`).'''
    def __init__(self, route: Route, guide, shape, t_start: int, known: Optional[Known], eta: float, step_noise, debug: bool):
        self.route, self.guide, self.t_start, self.known = route, guide, t_start, known
        (self.B, self.C, self.H, self.W), self.eta, self.step_noise, self.debug = shape, eta, step_noise, debug
        self.step_kwargs = {'eta': eta} if route.accepts_eta else {}     # of `scheduler.step` (+ the step's step_noise)
        # the CFG switch of a simple or composite guide, the UNet's batch replication, DDIM's prediction type
        self.cfg, self.rep, self.vpred = None, 1, False
        self.ent = {}                              # {'entities': the composite's weight maps [n][HW]} when they ride in the step
                                                   # (a windowed composite's: [n][H][W] over the canvas)
        self.grid = self.wins = None               # window loops: the grid and the persistent window batch
        self.lin_input = None                      # K-LMS on the linear loop: the persistent, sigma-scaled model input

    def mask(self, i: int):
        return None if self.known is None else self.known.at(i)


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

    def enable_vae_tiling(self, tile=64, stride=48, feather=None):
        '''Decode and encode canvases larger than `tile` latent cells as overlapping VAE tiles at `stride`, blended over
        `feather` cells (default tile - stride): AutoencoderKL.enable_tiling.  An approximation by construction.'''
        self.vae.enable_tiling(tile, stride, feather)

    def disable_vae_tiling(self):
        self.vae.disable_tiling()

    def decode_latents(self, latents: torch.Tensor) -> torch.Tensor:
        '''latents -> device image tensor (B,3,H,W) fp32 in [0,1] (pipeline/flex.py:117-120).'''
        return self.vae.decode_image(latents, 1.0 / VAE_SCALE, 0.5, 0.5, True)

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

    def _init_latents(self, guide, init_image, init_size, strength, generator, latents, noise, mask_image):
        '''The request's first latents: txt2img noise (or `latents`), or the init image's latents noised to the start level
        (pipeline/flex.py:186-238).  -> (latents, t_start, the `Known` of a masked request or None).'''
        batch_size = guide.batch_size
        if init_image is None:
            height, width = init_size
            shape = (batch_size, self.unet.in_channels, height // 8, width // 8)
            init_latents = self._randn(shape, generator) if latents is None else latents.to(self.device, torch.float32).clone()
            self.scheduler.set_timesteps(guide.steps)
            if isinstance(self.scheduler, LMSDiscreteScheduler):   # pipeline/flex.py:236-238
                init_latents = ops.axpby(init_latents, None, float(self.scheduler.sigmas[0]), 0.0)
            return init_latents, 0, None
        if mask_image is not None:
            mask_hw = image_size(init_image)
        if not isinstance(init_image, torch.Tensor):
            init_image = preprocess(init_image)
        init_image = init_image.to(self.device)
        init_latents = self.vae.encode(init_image).latent_dist.sample(generator=generator)
        init_latents = ops.axpby(init_latents, None, VAE_SCALE, 0.0)
        init_latents = torch.cat([init_latents] * batch_size)
        t_noise, t_start = self._start_of(guide.steps, strength)
        # one level per sample, as a long tensor (pipeline/flex.py:201-209); built on the host
        t_noise = torch.tensor([t_noise] * batch_size, dtype=torch.long)
        noise = self._randn(init_latents.shape, generator) if noise is None else noise.to(self.device, torch.float32)
        if tuple(noise.shape) != tuple(init_latents.shape):
            raise ValueError(f'noise {tuple(noise.shape)} does not match the latents {tuple(init_latents.shape)}')
        known = None
        if mask_image is not None:
            # z0 and n stay alive for the loop; add_noise returns a new tensor, so neither aliases the latents
            z0 = init_latents.to(torch.float32).contiguous()
            h, w = z0.shape[-2:]
            if mask_hw[0] % h or mask_hw[1] % w or mask_hw[0] // h != mask_hw[1] // w:
                raise ValueError(f'init image {mask_hw} is not a whole multiple of its latents {(h, w)}')
            # uploaded once per call, as z0 and n are
            mask = latent_mask(mask_image, mask_hw[0], mask_hw[1], mask_hw[0] // h).to(self.device)
            known = Known(z0, noise.contiguous(), mask, known_coefficients(
                self.scheduler, self.scheduler.timesteps, t_start, start_level(self.scheduler, int(t_noise[0]))))
        return self.scheduler.add_noise(init_latents, noise, t_noise), t_start, known

    def _start_of(self, steps: int, strength: float) -> Tuple[int, int]:
        '''(t_noise, t_start) of an img2img request (pipeline/flex.py:195-216): the level its first latents are noised to -- a
        timestep, under K-LMS a sigma index (:200-204) -- and the index of its first timestep.'''
        offset = self.scheduler.config.get('steps_offset', 0)
        init_timestep = min(int(steps * strength) + offset, steps)
        if isinstance(self.scheduler, LMSDiscreteScheduler):
            t_noise = steps - init_timestep
        else:
            t_noise = int(self.scheduler.timesteps[-init_timestep])
        return t_noise, max(steps - init_timestep + offset, 0)

    def _noise_level(self, t_noise: int) -> Tuple[float, float]:
        '''The (k1, k2) of `scheduler.add_noise(z0, n, t_noise)` = k1 z0 + k2 n, the floats it hands its one launch.'''
        if isinstance(self.scheduler, LMSDiscreteScheduler):
            return 1.0, float(self.scheduler.sigmas[t_noise])
        a = self.scheduler.alphas_cumprod[t_noise]
        return float(np.sqrt(a)), float(np.sqrt(np.float32(1.0) - a))

    def _init_from_latents(self, guide, init_latents, init_size, strength, generator, noise, upscale, route: Route):
        '''The first latents of a request that starts from clean latents (`from_latents`; the second pass of hires sampling):
        they are resampled onto the canvas of `init_size` and noised to the start level of an img2img request of `strength` by
        ONE launch (fd_latent_upscale_noise_f32) -- no VAE, no host copy, and with `pipe.step_noise` no noise tensor.  The
        noise: the `noise=` tensor, else the stream of `pipe.step_noise` (stream STREAM_INIT, draw 0, generated in the kernel
        at the canvas element), else one host draw of the generator, as img2img draws it.  -> (canvas, t_start, bridge):
        on the `window` route the launch also writes the first window batch, so it is handed to `_begin`, which owns that
        buffer, as `bridge`; on every other route it has been issued here and `bridge` is None.'''
        B, C = guide.batch_size, self.unet.in_channels
        H, W = init_size[0] // 8, init_size[1] // 8
        if init_latents.dim() != 4 or init_latents.shape[0] not in (1, B) or init_latents.shape[1] != C:
            raise ValueError(f'init_latents {tuple(init_latents.shape)} are not (1 | {B}, {C}, h, w)')
        hs, ws = init_latents.shape[-2:]
        if H < hs or W < ws:
            raise ValueError(f'the canvas {(H, W)} of init_size {tuple(init_size)} is smaller than init_latents {(hs, ws)}: only '
                             'upscaling is supported')
        src = init_latents.to(self.device, torch.float32).contiguous()
        t_noise, t_start = self._start_of(guide.steps, strength)
        k1, k2 = self._noise_level(t_noise)
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            if tuple(noise.shape) != (B, C, H, W):
                raise ValueError(f'noise {tuple(noise.shape)} does not match the latents {(B, C, H, W)}')
        elif self.step_noise is not None:
            noise = self.step_noise
        else:
            noise = self._randn((B, C, H, W), generator)
        canvas = torch.empty((B, C, H, W), dtype=torch.float32, device=self.device)

        def bridge(wins=None, grid=None):
            ops.latent_upscale_noise(src, canvas, upscale, k1, k2, noise, 0, STREAM_INIT, wins, grid)
        if route.loop == 'window':
            return canvas, t_start, bridge
        bridge()
        return canvas, t_start, None

    def _lin_scale(self, j: int) -> float:
        return 1.0 / ((float(self.scheduler.sigmas[j]) ** 2 + 1) ** 0.5)     # pipeline/flex.py:270-274

    def _begin(self, route: Route, guide, latents, t_start, known, eta, step_noise, debug, bridge=None):
        '''The request's state and the tensor its loop steps: the persistent buffers a route reads through the graph / plan, the
        time-embedding table, the composite's weight maps, the window batch.  `bridge` (`_init_from_latents`, the `window`
        route): the one launch that fills `latents` and the window batch, instead of the gather.  -> (_Request, latents).'''
        B, C, H, W = latents.shape
        s = _Request(route, guide, (B, C, H, W), t_start, known, eta, step_noise, debug)
        if route.persistent:
            # persistent latent buffer: the captured UNet graph / recorded plan reads this address (PLMS steps it in place)
            latents = self.loop_latents(latents)
        elif route.loop == 'linear':
            # K-LMS: the persistent buffer holds the SCALED model input (what the graph / plan reads), written by every step's
            # launch for the next one and by one axpby for the first; the unscaled latents are a tensor of this call's own
            latents = latents.to(self.device, torch.float32).clone()
            s.lin_input = self.loop_latents(ops.axpby(latents, None, self._lin_scale(t_start), 0.0))
        self._temb_tab = None
        if route.temb_table:
            # the time embedding depends on t only: all of the request's timesteps in one pass (three GEMMs over len(timesteps) rows)
            # instead of three GEMMs per step
            keys = {}
            for t in self.scheduler.timesteps[t_start:]:
                keys.setdefault(float(t), len(keys))
            self._temb_tab = (keys, self.unet.time_bias_table(list(keys)))
        # loop-invariant: the CFG switch and the UNet's batch replication of a device guide, DDIM's prediction type
        if route.guide in ('simple', 'composite'):
            s.cfg = guide.classifier_free_guidance
        s.rep = guide.rep if route.guide in ('composite', 'window') else 2 if s.cfg else 1
        s.vpred = route.loop in ('ddim', 'window') and self.scheduler.config['prediction_type'] == 'v_prediction'
        if route.fuse_entities:
            # the composite's weight maps [n][HW] as the schedulers' fused steps take them, built once per latent size
            s.ent = {'entities': guide.entity_rows(H, W)}
        if route.loop in ('window', 'window_planned'):
            # the window batch: the one persistent buffer (what the graph / plan reads); the canvas does not evict it
            s.grid = guide.bind(H, W)
            wshape = (B * s.grid.count, C, s.grid.h, s.grid.w)
            s.wins = self._lat_bufs.get(wshape)
            if s.wins is None:
                s.wins = torch.empty(wshape, dtype=torch.float32, device=latents.device)
                self._lat_bufs = {wshape: s.wins}
            if bridge is not None:
                bridge(s.wins, s.grid.args)
            else:
                guide.gather(latents, s.wins)
            if hasattr(guide, 'entity_maps'):
                # a WindowedCompositeGuide: its canvas weight maps [n][H][W] ride in the multistep launch (its own `step` carries them)
                s.ent = {'entities': guide.entity_maps(H, W)}
        return s, latents

    def _eps(self, s: _Request, x: torch.Tensor, t: int, latents: torch.Tensor):
        '''The UNet's output on the model input `x` of a fused loop, and the tensor the step writes: the graph / plan replay and
        `latents` itself, or under `debug` the eager forward and a copy (a composite or windowed guide reads the request's
        time-bias table as the graph / plan do: bit-equal to them; a SimpleGuide: the call as it was).'''
        if not s.debug:
            return self._unet_eps(x, t, s.guide.stacked_embeds(), s.rep), latents
        table = s.route.guide != 'simple' and self._temb_tab
        temb = self._temb_row(t).expand(x.shape[0] * s.rep, -1).contiguous() if table else None
        return self.unet.forward_nhwc(x, t, s.guide.stacked_embeds(), rep=s.rep, temb=temb), latents.clone()

    def _blend_known(self, s: _Request, x: torch.Tensor, i: int):
        '''Masked img2img behind any scheduler / guide: the blend-only launch on the step's result.'''
        z0, n, m, k1, k2 = s.known.at(i)
        ops.cfg_ddim_masked_step(x, None, z0, n, m, s.B, s.C, s.H * s.W, k1=k1, k2=k2)

    def _step_ddim(self, s: _Request, i: int, t, latents):
        '''DDIM on the device loop: the UNet, then CFG (+ rescale | the entity blend) + the update + sigma z + the known-region
        blend of a masked request in one launch.'''
        r, guide, B, C, HW = s.route, s.guide, s.B, s.C, s.H * s.W
        eps, latents = self._eps(s, latents, int(t), latents)
        coef = self.scheduler.step_coefficients(int(t), s.eta if r.noisy else 0.0)
        sigma, coef = float(coef[4]) if r.noisy else 0.0, coef[:4]
        noise, draw, blend = s.step_noise if r.noisy else None, s.t_start + i, s.mask(i)
        if r.rescale:
            ops.cfg_rescale_ddim_step(latents, eps, B, C, HW, guide.guidance, r.rescale, coef, s.vpred, mask=blend, sigma=sigma,
                                      noise=noise, draw=draw)
        elif r.fuse_entities and (r.noisy or blend is not None):
            guide.step(latents, eps, coef, s.vpred, mask=blend, sigma=sigma, step_noise=(noise, draw) if r.noisy else None)
        elif r.noisy:
            ops.cfg_ddim_noise_step(latents, eps, B, C, HW, s.cfg, guide.guidance, coef, s.vpred, sigma, noise, C * HW, draw, blend)
        elif r.guide == 'composite':
            guide.step(latents, eps, coef, s.vpred)
            if blend is not None:
                self._blend_known(s, latents, i)
        elif blend is not None:
            ops.cfg_ddim_masked_step(latents, eps, *blend[:3], B, C, HW, s.cfg, guide.guidance, coef, s.vpred, *blend[3:])
        else:
            ops.cfg_ddim_step(latents, eps, B, C, HW, s.cfg, guide.guidance, coef, s.vpred)
        return latents

    def _step_multistep(self, s: _Request, i: int, t, latents):
        '''DPM-Solver++ and its SDE form on the device loop: the UNet, then the scheduler's one launch (CFG, x0, history,
        multistep update, step noise, known-region blend), with the rescale or the entity blend ahead of it in that launch.
        UniPC (`unipc`): the same calls on its scheduler -- corrector, kept sample and predictor in that one launch, no noise.'''
        r, guide, B, C, HW = s.route, s.guide, s.B, s.C, s.H * s.W
        eps, latents = self._eps(s, latents, int(t), latents)
        blend, noise = s.mask(i), (s.step_noise, s.t_start + i) if r.sde else None
        if r.rescale:
            self.scheduler.fused_rescale_step(latents, eps, int(t), B, C, HW, guide.guidance, r.rescale, blend, noise)
        elif r.guide == 'composite':
            self.scheduler.fused_composite_step(latents, eps, int(t), B, C, HW, s.cfg, guide.guidance, s.ent['entities'], blend, noise)
        elif r.sde:
            self.scheduler.fused_step(latents, eps, int(t), B, C, HW, s.cfg, guide.guidance, blend, noise)
        else:
            self.scheduler.fused_step(latents, eps, int(t), B, C, HW, s.cfg, guide.guidance, blend)
        return latents

    def _step_linear(self, s: _Request, i: int, t, latents):
        '''PLMS and K-LMS on the device loop: the UNet replay, then `scheduler.fused_step` (CFG | the entity blend, the history
        write, the linear multistep update, the known-region blend) in one launch.'''
        guide, B, C, HW, j = s.guide, s.B, s.C, s.H * s.W, s.t_start + i
        if not s.route.is_lms:
            eps = self._unet_eps(latents, float(t), guide.stacked_embeds(), s.rep)
            self.scheduler.fused_step(latents, eps, t, B, C, HW, s.cfg, guide.guidance, s.mask(i), **s.ent)
            return latents
        # the scheduler steps by sigma index; the UNet sees the float timestep and the scaled buffer, which this step's launch
        # refills for the next one
        eps = self._unet_eps(s.lin_input, float(t), guide.stacked_embeds(), s.rep)
        last = j + 1 >= len(self.scheduler.timesteps)
        self.scheduler.fused_step(latents, eps, j, B, C, HW, s.cfg, guide.guidance, s.mask(i),
                                  scaled_out=None if last else s.lin_input, next_scale=0.0 if last else self._lin_scale(j + 1), **s.ent)
        return latents

    def _step_window(self, s: _Request, i: int, t, latents):
        '''A windowed canvas on the device loop: the UNet over the window batch, then CFG per window, the average, the update of
        the canvas, the step noise, the known-region blend and the next window batch (of the blended canvas) in one launch.'''
        r, guide = s.route, s.guide
        eps, latents = self._eps(s, s.wins, int(t), latents)
        if r.multistep:
            self.scheduler.fused_window_step(latents, s.wins, eps, int(t), s.B, s.C, s.grid.args, guide.blend_code,
                                             guide.classifier_free_guidance, guide.guidance, s.mask(i),
                                             (s.step_noise, s.t_start + i) if r.sde else None, **s.ent)
        else:
            coef = self.scheduler.step_coefficients(int(t), s.eta if r.noisy else 0.0)
            guide.step(latents, s.wins, eps, coef[:4], s.vpred, mask=s.mask(i), sigma=float(coef[4]) if r.noisy else 0.0,
                       step_noise=(s.step_noise, s.t_start + i) if r.noisy else None)
        return latents

    def _step_generic(self, s: _Request, i: int, t, latents):
        '''`scheduler.step` on the guided prediction, then the blend-only launch of a masked request.  The prediction: on
        `planned` and `window_planned` the UNet replay on the persistent buffer and the guide's combine-only launch (the bits of
        `guide.noise_pred`), else `guide.noise_pred` itself -- the reference protocol (pipeline/flex.py:262-290).'''
        r, guide, B, C, H, W = s.route, s.guide, s.B, s.C, s.H, s.W
        t_index, model_input = t, latents
        if r.is_lms:        # pipeline/flex.py:270-274: continuous-ODE input scaling
            t_index = s.t_start + i
            model_input = ops.axpby(latents, None, self._lin_scale(t_index), 0.0)
        if r.loop == 'generic':
            noise_pred = guide.noise_pred(model_input, t)
        else:
            noise_pred = torch.empty((B, C, H, W), dtype=torch.float32, device=latents.device)
        if r.loop == 'planned':
            eps = self._unet_eps(self.loop_latents(model_input), float(t), guide.stacked_embeds(), s.rep)
            if r.guide == 'composite':
                guide.step(None, eps, eps_out=noise_pred)
            elif r.rescale:
                ops.cfg_rescale_ddim_step(None, eps, B, C, H * W, guide.guidance, r.rescale, do_step=False, eps_out=noise_pred)
            else:
                ops.cfg_ddim_step(None, eps, B, C, H * W, s.cfg, guide.guidance, do_step=False, eps_out=noise_pred)
        elif r.loop == 'window_planned':
            # gather into the persistent window batch, replay, the combine-only form of the windowed step
            guide.gather(model_input.to(self.device, torch.float32).contiguous(), s.wins)
            eps = self._unet_eps(s.wins, float(t), guide.stacked_embeds(), s.rep)
            guide.step(None, None, eps, eps_out=noise_pred)
        if r.takes_noise:
            s.step_kwargs['step_noise'] = (s.step_noise, s.t_start + i)
        latents = self.scheduler.step(noise_pred, t_index, latents, **s.step_kwargs).prev_sample
        if s.known is not None:
            # blend the step's own result (not the persistent buffer, which holds the model input)
            latents = latents.to(self.device, torch.float32).contiguous()
            self._blend_known(s, latents, i)
        return latents

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
        over the kept region is out of scope, as are per-sample masks and feathering helpers.

        `output_type='latent'` (beyond the reference): the final latents (B, 4, h, w) come back as the images, a tensor of
        the caller's own, and the VAE does not run.'''
        return self._sample(guide, init_image, init_size, strength, eta, generator, output_type, return_dict, debug, latents,
                            noise, mask_image)

    @torch.no_grad()
    def from_latents(self, guide: GuideBase, init_latents: torch.Tensor, *, init_size: Tuple[int, int] = (512, 512),
                     strength: float = 0.6, upscale: str = 'bicubic', eta: float = 0.0,
                     generator: Optional[torch.Generator] = None, output_type: str = 'pil', return_dict: bool = True,
                     debug: bool = False, noise: Optional[torch.Tensor] = None):
        '''An img2img request that starts from clean latents instead of an image (beyond the reference; the second pass of
        hires sampling, `hires`): `init_latents`, already scaled, (1 | B, 4, hs, ws) -- one latent may be shared by the B
        samples, each with its own noise -- are resampled onto the canvas of `init_size` (`upscale`: 'nearest', or the
        antialiased 'bilinear' / 'bicubic' of the reference's composition/guide.py:27-29 `_scale`; the canvas may not be
        smaller) and noised to the level `strength` gives an init image (`steps_offset` and K-LMS's index form included),
        all in ONE launch (`_init_from_latents`): no VAE pass, no host copy.  `noise`: canvas-shaped add_noise rows instead
        of the pipeline's own.  Every other argument is `__call__`'s, by keyword (`__call__` itself keeps the reference's
        signature); there is no init image and so no mask image.'''
        if upscale not in ops.UPSCALE_MODES:
            raise ValueError(f'upscale should be one of {sorted(ops.UPSCALE_MODES)} but is {upscale!r}')
        if not isinstance(init_latents, torch.Tensor):
            raise ValueError(f'init_latents should be a tensor (1 | B, 4, h, w) but are {type(init_latents).__name__}')
        return self._sample(guide, None, init_size, strength, eta, generator, output_type, return_dict, debug, None, noise, None,
                            init_latents, upscale)

    def _sample(self, guide, init_image, init_size, strength, eta, generator, output_type, return_dict, debug, latents, noise,
                mask_image, init_latents=None, upscale='bicubic'):
        '''The request behind `__call__` and `from_latents`.'''
        if strength < 0 or strength > 1:
            raise ValueError(
                f'The value of strength should in [0.0, 1.0] but is {strength}')
        if mask_image is not None and init_image is None:
            raise ValueError('mask_image needs an init_image: the mask says which part of it to keep')
        # guidance rescale: the guide's attribute, checked before any launch; 0 keeps every route on its calls
        rescale = float(getattr(guide, 'guidance_rescale', 0.0) or 0.0)
        if rescale:
            check_guidance_rescale(rescale, guide.guidance)
        self.scheduler.set_timesteps(guide.steps)
        assert self.scheduler.timesteps is not None
        route = select_route(guide, self.scheduler, self.unet, eta=eta, step_noise=self.step_noise, rescale=rescale, debug=debug,
                             use_graph=self.use_graph, use_plan=self.use_plan, fuse_composite=self.fuse_composite,
                             fuse_linear_multistep=self.fuse_linear_multistep)
        bridge = None
        if init_latents is not None:
            latents, t_start, bridge = self._init_from_latents(guide, init_latents, init_size, strength, generator, noise, upscale,
                                                               route)
            known = None
        else:
            latents, t_start, known = self._init_latents(guide, init_image, init_size, strength, generator, latents, noise,
                                                         mask_image)
        all_latents = [latents] if debug else None
        # the step noise of the request: the pipeline's attribute; an SDE scheduler without one gets the generator's seed
        step_noise = self.step_noise
        if route.sde and step_noise is None:
            step_noise = PhiloxNoise(generator.initial_seed() if generator is not None else 0)
        s, latents = self._begin(route, guide, latents.contiguous(), t_start, known, eta, step_noise, debug, bridge)
        step = {'ddim': self._step_ddim, 'multistep': self._step_multistep, 'unipc': self._step_multistep,
                'linear': self._step_linear, 'window': self._step_window}.get(route.loop, self._step_generic)
        # a guide with a context schedule (ScheduledGuide, CompositeGuide(style_linear=)): told the GLOBAL step index at the top of
        # every iteration, on every route; guides without `at_step` run as before
        at_step = getattr(guide, 'at_step', None)
        # The host only has to stay ahead of the device queue.  A generation-2 collection of the
        # cyclic GC walks every tracked object of the process (~175 k with the SD1.5 weights:
        # ~40 ms) and drains that queue, so collections wait until the images are decoded.
        with (_gc_paused() if self.pause_gc else contextlib.nullcontext()):
            for i, t in enumerate(self.progress_bar(self.scheduler.timesteps[t_start:])):
                if at_step is not None:
                    # a context schedule: the step's blend, issued eagerly on the loop's stream before the graph / plan replay reads it
                    at_step(t_start + i)
                latents = step(s, i, t, latents)
                if all_latents is not None:
                    all_latents.append(latents)
            # the fused loop ran on the persistent per-shape buffer, which the next call overwrites:
            # hand out a copy, so a caller holding `pipe.last_latents` keeps the values it read
            persistent = any(latents is b for b in self._lat_bufs.values())
            self.last_latents = latents.clone() if persistent else latents

            if output_type == 'latent':
                batch_images = self.last_latents
            elif all_latents:
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

    def hires(self, guide: GuideBase, hires_guide: GuideBase, *, init_size: Tuple[int, int], hires_size: Tuple[int, int],
              hires_strength: float = 0.5, upscale: str = 'bicubic', eta: float = 0.0,
              generator: Optional[torch.Generator] = None, output_type: str = 'pil', return_dict: bool = True):
        '''Two-pass ("hires fix") sampling, beyond the reference: `guide` samples at `init_size`, the model's own size, which
        fixes the layout; its latents are upscaled to `hires_size`, noised back to the level of `hires_strength` and finished
        by `hires_guide` as an img2img request -- typically a `WindowedGuide` over the same embeddings, so every UNet launch
        stays at the model's size.  The two explicit calls, `self(guide, output_type='latent')` and
        `self.from_latents(hires_guide, ...)`, nothing else: between them is one launch (`_init_from_latents`), no VAE pass
        and no host copy.  The guides may be any pair with one `batch_size` (a CompositeGuide / WindowedCompositeGuide pair
        included, with the second one's entities given on its own canvas).'''
        if guide.batch_size != hires_guide.batch_size:
            raise ValueError(f'the guides of the two passes differ in batch_size: {guide.batch_size} and {hires_guide.batch_size}')
        base = self(guide, init_size=init_size, eta=eta, generator=generator, output_type='latent', return_dict=False)[0]
        return self.from_latents(hires_guide, base, init_size=hires_size, strength=hires_strength, upscale=upscale, eta=eta,
                                 generator=generator, output_type=output_type, return_dict=return_dict)
