'''Harness -- host-side mirror of the reference's `utils.Runner` call recipe
(utils.py:54-166: seed handling :78-83, sequential sample batches :90, argument plumbing of
`gen` :114-166) and `image_grid` (:36-50).

`Runner.compose` (utils.py:168-207) is the caller of CompositeGuide: entity rows are parsed with
the reference's forgiving try/except, empty prompts dropped, a `Schema` built and run.

Out of scope here: model download (`from_pretrained`), PNG / grid files
and the filename scheme -- `Runner` takes state dicts (or builds seeded synthetic ones) and
returns the images.  Differences from the reference, all deliberate:
E5 `eta` stays 0.0 (the reference overwrites it with wall-clock seconds after the first
batch); E6 the generator is a CPU generator, so a seed gives the same images on any number
of GPUs; no CUDA autocast context is needed (the kernels are fp16 MFMA by construction).
'''
from __future__ import annotations

import dataclasses
import gc
import inspect
import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import torch

from . import build
from .encode.clip import CLIPEncoder
from .guidance import Guide
from .composition import CompositeGuide, EntitySchema, Schema, WindowedCompositeGuide
from .noise import PhiloxNoise
from .pipeline.guide import GuideBase, ScheduledGuide, SimpleGuide, WindowedGuide
from .scheduler import DPMSolverMultistepSDEScheduler

MAX_SEED = 2147483647          # the reference clamps seeds to int32 (utils.py:22)

# the keyword arguments `gen` forwards untouched to `Guide.embeds` (utils.py:151-162)
_EMBEDS_KEYS = ('mapping_concepts', 'guide_threshold_mult', 'guide_threshold_floor', 'guide_clustered',
                'guide_linear', 'guide_max_guidance', 'guide_header_max', 'guide_mode', 'guide_reuse')


_SAME = object()              # `gen_scheduled(end_guide=)`: the same guide image as `guide`


def image_grid(imgs: Sequence[Any]):
    '''Paste PIL images into one sheet, row-major: ceil(sqrt(n)) columns and n // columns rows, so
    the last images are dropped when they do not fill a row (the reference's arithmetic,
    utils.py:36-50).'''
    from PIL import Image
    cols = math.ceil(math.sqrt(len(imgs)))
    rows = len(imgs) // cols
    w, h = imgs[0].size
    sheet = Image.new('RGB', size=(cols * w, rows * h))
    for k, img in enumerate(imgs):
        sheet.paste(img, box=(k % cols * w, k // cols * h))
    return sheet


def entity_from_row(row: Sequence[Any]) -> Optional[EntitySchema]:
    '''One table row [prompt, x, y, width, height, blend] -> EntitySchema, or None when it cannot be
    coerced (the reference reports and skips such rows, utils.py:188-196).'''
    try:
        prompt, x, y, w, h, blend = (row[k] for k in range(6))
        return EntitySchema(str(prompt).strip(), (int(x), int(y)), (int(w), int(h)), float(blend))
    except Exception as ex:          # noqa: BLE001 -- the reference catches everything here
        print('Failed to build EntitySchema:', ex)
        return None


class Runner():
    # opt-in (beyond the reference): VAE tiling of every request's decode and of an init image's encode
    # (`FlexPipeline.enable_vae_tiling`): None (off), True (tile 64, stride 48) or a (tile, stride[, feather]) tuple in
    # latent cells.  An attribute like `step_noise`; applied to the pipeline's VAE at the top of every run
    vae_tiling = None

    def __init__(self, local: bool = True, device: str = 'cuda', *, sd_dir: Optional[str] = None,
                 clip_dir: Optional[str] = None, tokenizer_dir: Optional[str] = None,
                 state_dicts: Optional[Dict[str, dict]] = None, preset: str = 'sd15', seed_weights: int = 0,
                 freeze_gc: bool = False, pause_gc: bool = False, scheduler=None, text_cleanup: str = 'basic') -> None:
        '''`Runner(local=True, device='cuda')` as the reference constructs it (utils.py:54-76); the hub
        ids the reference hard-codes (utils.py:24-25) become local directories:
          sd_dir        diffusers-layout checkpoint (unet/, vae/, tokenizer/) -- env FD_SD_DIR
          clip_dir      CLIPModel directory                                    -- env FD_CLIP_DIR
          tokenizer_dir vocab.json + merges.txt; default `sd_dir`/tokenizer     -- env FD_TOKENIZER_DIR
        The scheduler is the checkpoint's own (`sd_dir`/scheduler/scheduler_config.json: PNDM/PLMS for SD-v1-4, as the
        reference's `sd.scheduler`, utils.py:70) unless `scheduler=` overrides it; `text_cleanup='basic'` is the
        tokenization of the reference's pinned slow CLIPTokenizer ('fast': CLIPTokenizerFast).
        `local=False` (the reference's --dl) cannot be served: there is no hub access here.
        Without directories: `state_dicts` (fp32 CPU tensors with HF key names) or seeded synthetic
        weights of `preset` with the synthetic tokenizer.
        `freeze_gc` / `pause_gc` (both off by default: they change interpreter-global state): park the
        long-lived model objects in the GC's permanent generation / keep the cyclic GC off across each
        denoising loop -- what `bench.py` runs with.'''
        if not local:
            raise RuntimeError('Runner(local=False): no network access -- place the checkpoint on disk and pass '
                               'sd_dir / clip_dir (or set FD_SD_DIR / FD_CLIP_DIR)')
        sd_dir = sd_dir or os.environ.get('FD_SD_DIR')
        clip_dir = clip_dir or os.environ.get('FD_CLIP_DIR')
        tokenizer_dir = tokenizer_dir or os.environ.get('FD_TOKENIZER_DIR')
        if sd_dir or clip_dir:
            if not (sd_dir and clip_dir):
                raise ValueError('Runner needs both sd_dir and clip_dir (utils.py:24-25: two checkpoints)')
            self.pipe, clip, tok = build.from_directories(sd_dir, clip_dir, tokenizer_dir, preset=preset,
                                                          device=device, scheduler=scheduler, text_cleanup=text_cleanup)
        else:
            if state_dicts is None:
                state_dicts = build.synthetic_state_dicts(preset, seed=seed_weights)
            tok = build.load_tokenizer(tokenizer_dir, text_cleanup) if tokenizer_dir else None
            self.pipe, clip, tok = build.build_models(state_dicts, preset, device, tokenizer=tok, scheduler=scheduler)
        self.pipe.pause_gc = pause_gc
        self.device = device
        self.encoder = CLIPEncoder(clip, self.pipe.tokenizer)     # utils.py:73-74
        self.guide = Guide(clip, self.pipe.tokenizer, device=device)
        self.generator = torch.Generator(device='cpu')     # E6: host generator
        self.eta = 0.0                                      # E5: never overwritten
        # opt-in (always on under an SDE scheduler): step noise from the counter-based stream (noise.PhiloxNoise) keyed by
        # the generator's seed, batch k of B samples at sample offset k * B -- k sequential batches see the noise of one
        # batch of k * B
        self.step_noise = False
        # opt-in (beyond the reference): guidance rescale of the guides `gen` and `gen_scheduled` build (`SimpleGuide(guidance_rescale=)`,
        # Lin et al. 2023 sec. 3.4; 0.7 is what zero-terminal-SNR v-prediction checkpoints are published with).  An attribute
        # like `step_noise`: the signatures of `gen` and `compose` are the reference's
        self.guidance_rescale = 0.0
        # the models and tokenizer tables are millions of long-lived objects: a full collection over them is a 50-100 ms
        # host stall between denoising loops (measured in bench.py's timed region)
        if freeze_gc:
            gc.collect()
            gc.freeze()

    def _set_seed(self, seed: Optional[int]):
        '''Falsy seed -> a random one; otherwise clamped to [0, 2^31 - 1] (utils.py:78-83).'''
        seed = min(max(seed, 0), MAX_SEED) if seed else int(torch.randint(0, MAX_SEED, (1,))[0])
        self.generator.manual_seed(seed)
        return seed

    def _apply_vae_tiling(self):
        '''`vae_tiling` onto the pipeline's VAE, at the top of every run.'''
        # a pipeline around a foreign VAE (`_decode_generic`) has no tiling to switch off
        if self.vae_tiling:
            self.pipe.enable_vae_tiling(*(() if self.vae_tiling is True else self.vae_tiling))
        elif getattr(getattr(self.pipe, 'vae', None), 'tiling', None) is not None:
            self.pipe.disable_vae_tiling()

    def _stochastic(self) -> bool:
        '''Whether a run keys the pipeline's counter-based noise by the generator's seed: `step_noise`, or an SDE scheduler.'''
        return bool(self.step_noise or isinstance(self.pipe.scheduler, DPMSolverMultistepSDEScheduler))

    def _run(self, batches: int, guide: GuideBase, init_image, init_size: Tuple[int, int],
             strength: float, debug: bool, mask_image=None):
        '''`batches` sequential pipeline calls on one generator stream -- the reference's only
        data-parallel axis (utils.py:90) -- and the grid of everything they produced.'''
        self._apply_vae_tiling()
        images: List[Any] = []
        extra = {'mask_image': mask_image} if mask_image is not None else {}
        stochastic = self._stochastic()
        for k in range(batches):
            if stochastic:
                self.pipe.step_noise = PhiloxNoise(self.generator.initial_seed(), sample_offset=k * guide.batch_size)
            result = self.pipe(guide=guide, init_image=init_image, init_size=init_size, strength=strength,
                               generator=self.generator, eta=self.eta, debug=debug, **extra)
            images += list(result['sample'])
        return images, image_grid(images)

    def gen(self,
            prompt='',
            init_image=None,
            guide=None,
            init_size: Tuple[int, int] = (512, 512),
            mapping_concepts: str = '',
            guide_threshold_mult: float = 0.5,
            guide_threshold_floor: float = 0.5,
            guide_clustered: float = 0.5,
            guide_linear: Tuple = (0.0, 0.5),
            guide_max_guidance: float = 0.5,
            guide_header_max: float = 0.15,
            guide_mode: int = 0,
            guide_reuse: bool = True,
            strength: float = 0.6,
            steps: int = 10,
            guidance_scale: float = 8,
            samples: int = 1,
            seed: Optional[int] = None,
            debug: bool = False,
            *,
            mask_image=None):
        '''Same arguments and defaults as utils.py:114-133; returns (images, grid).  Beyond the
        reference: `mask_image` over `init_image` (1 = repaint, 0 = keep; `FlexPipeline.__call__`).'''
        return self._gen(locals())

    def gen_scheduled(self, prompt='', *, end_prompt=None, end_guide=_SAME, schedule: Sequence[float] = (0.0, 1.0), **gen_args):
        '''`gen` whose context moves over the steps (beyond the reference; `ScheduledGuide`): a second keyframe is embedded
        from `end_prompt` (default: `prompt`) and `end_guide` (default: the same guide image as `guide`) with the same
        guidance parameters, and the request goes from the first keyframe to the second by `schedule` -- a (first, last)
        pair of blend weights or one weight per step: prompt travel, or a guide image faded in or out.  Every other
        argument is `gen`'s, by keyword (`gen` itself keeps the reference's signature).'''
        given = inspect.signature(Runner.gen).bind(self, prompt, **gen_args)
        given.apply_defaults()
        return self._gen(dict(given.arguments), (end_prompt, end_guide, schedule))

    def gen_wide(self, prompt='', *, size: Tuple[int, int] = (512, 1536), window=512, stride=256, blend: str = 'uniform',
                 **gen_args):
        '''`gen` on a canvas larger or wider than the model's size (beyond the reference; `WindowedGuide`, MultiDiffusion):
        `size` is the image's (height, width), covered by overlapping `window`s at `stride` (image pixels; an int means both
        axes) whose predictions are averaged ('uniform') or tent-weighted ('tent') where they overlap.  Every other
        argument is `gen`'s, by keyword (`gen` itself keeps the reference's signature); `init_size` is `size`.'''
        given = inspect.signature(Runner.gen).bind(self, prompt, **gen_args)
        given.apply_defaults()
        given = dict(given.arguments)
        given['init_size'] = tuple(size)
        return self._gen(given, wide=(window, stride, blend))

    def gen_hires(self, prompt='', *, size: Tuple[int, int] = (1024, 1024), base_size: Tuple[int, int] = (512, 512),
                  hires_strength: float = 0.5, hires_steps: Optional[int] = None, upscale: str = 'bicubic', window=512,
                  stride=256, blend: str = 'tent', **gen_args):
        '''Two-pass ("hires fix") sampling (beyond the reference; `FlexPipeline.hires`): `gen` at `base_size`, the model's own
        size, then its latents upscaled (`upscale`) to the canvas of `size`, noised back to the level of `hires_strength`
        and finished by `gen_wide`'s windows (`window`, `stride`, `blend`) over the same embeddings in `hires_steps`
        (default: `steps`) -- one launch between the passes instead of a VAE decode, a host resize and a VAE encode.  Every
        other argument is `gen`'s, by keyword (`init_size`, `strength` and `debug` are not read: the passes have their own
        sizes and level, and return no intermediate images); the prompt is embedded once.  `init_image` / `mask_image` and `Runner.guidance_rescale` are refused; `vae_tiling` and
        `step_noise` are honoured.'''
        given = inspect.signature(Runner.gen).bind(self, prompt, **gen_args)
        given.apply_defaults()
        given = dict(given.arguments)
        if given['init_image'] is not None or given['mask_image'] is not None:
            raise ValueError('gen_hires starts from noise at base_size: it takes neither an init_image nor a mask_image')
        if self.guidance_rescale:
            raise ValueError('gen_hires does not support Runner.guidance_rescale: its second pass is windowed, and the standard '
                             'deviations would have to span the canvas')
        self._set_seed(given['seed'])
        unet, scale, steps = self.pipe.unet, given['guidance_scale'], given['steps']
        embeds = self.guide.embeds(prompt=given['prompt'], guide=given['guide'], **{k: given[k] for k in _EMBEDS_KEYS})
        first = SimpleGuide(self.encoder, unet, scale, steps, embeds)
        second = WindowedGuide(self.encoder, unet, scale, hires_steps or steps, embeds, window=window, stride=stride, blend=blend)
        self._apply_vae_tiling()
        images: List[Any] = []
        for k in range(given['samples']):
            if self._stochastic():
                self.pipe.step_noise = PhiloxNoise(self.generator.initial_seed(), sample_offset=k * first.batch_size)
            result = self.pipe.hires(first, second, init_size=tuple(base_size), hires_size=tuple(size),
                                     hires_strength=hires_strength, upscale=upscale, eta=self.eta, generator=self.generator)
            images += list(result['sample'])
        return images, image_grid(images)

    def _gen(self, given: Dict[str, Any], travel=None, wide=None):
        self._set_seed(given['seed'])
        params = {k: given[k] for k in _EMBEDS_KEYS}
        unet, scale, steps = self.pipe.unet, given['guidance_scale'], given['steps']
        embeds = self.guide.embeds(prompt=given['prompt'], guide=given['guide'], **params)
        if wide is not None:
            window, stride, blend = wide
            if self.guidance_rescale:
                raise ValueError('gen_wide does not support Runner.guidance_rescale: its standard deviations would have to '
                                 'span the canvas')
            g = WindowedGuide(self.encoder, unet, scale, steps, embeds, window=window, stride=stride, blend=blend)
        elif travel is None:
            g = SimpleGuide(self.encoder, unet, scale, steps, embeds, guidance_rescale=self.guidance_rescale)
        else:
            end_prompt, end_guide, schedule = travel
            end = self.guide.embeds(prompt=given['prompt'] if end_prompt is None else end_prompt,
                                    guide=given['guide'] if end_guide is _SAME else end_guide, **params)
            g = ScheduledGuide(self.encoder, unet, scale, steps, [embeds, end], schedule, guidance_rescale=self.guidance_rescale)
        mask_image = given['mask_image']
        return self._run(given['samples'], g, given['init_image'], given['init_size'], given['strength'], given['debug'],
                         **({'mask_image': mask_image} if mask_image is not None else {}))

    def compose(self,
                bg_prompt: str = '',
                entities_df: Sequence[Sequence[Any]] = (),
                start_style: str = '',
                end_style: str = '',
                style_blend: Tuple[float, float] = (0.0, 1.0),
                init_image=None,
                batches: int = 4,
                strength: float = 0.7,
                steps: int = 30,
                guidance_scale: float = 8.0,
                init_size: Tuple[int, int] = (512, 512),
                seed: Optional[int] = None,
                debug: bool = False,
                *,
                batch_size: int = 1,
                masks: Optional[Sequence[Any]] = None,
                mask_image=None):
        '''Same arguments and defaults as utils.py:168-181; returns (images, grid).  `entities_df`
        rows are [prompt, offset_x, offset_y, width, height, blend]; a DataFrame is taken through
        its `_values` (utils.py:198-199); rows that do not parse or have an empty prompt are dropped.
        Beyond the reference: `batch_size` samples per pipeline call (one UNet forward; `batches *
        batch_size` images in all) and `masks`, aligned with the table rows (None: the rectangle),
        each an EntitySchema mask over its box; `mask_image` over `init_image` (1 = repaint, 0 = keep:
        masked img2img, `FlexPipeline.__call__`).  The style arguments are stored in the schema and, as in the
        reference, not applied; `compose_styled` applies them.'''
        return self._compose(locals())

    def compose_styled(self, bg_prompt: str = '', entities_df: Sequence[Sequence[Any]] = (), start_style: str = '',
                       end_style: str = '', style_blend: Tuple[float, float] = (0.0, 1.0), *,
                       style_linear: Tuple[float, float] = (0.0, 0.5), **compose_args):
        '''`compose` with the style blend the reference's composer asks for and drops (beyond the reference;
        `CompositeGuide(style_linear=)`): `start_style` / `end_style` pull every prompt by linspace(*style_linear) per
        token and the request moves from the start style to the end style by `style_blend`.  Every other argument is
        `compose`'s, by keyword (`compose` itself keeps the reference's signature).'''
        given = inspect.signature(Runner.compose).bind(self, bg_prompt, entities_df, start_style, end_style, style_blend,
                                                       **compose_args)
        given.apply_defaults()
        return self._compose(dict(given.arguments), style_linear)

    def compose_wide(self, bg_prompt: str = '', entities_df: Sequence[Sequence[Any]] = (), *, size: Tuple[int, int] = (512, 1536),
                     window=512, stride=256, blend: str = 'uniform', **compose_args):
        '''`compose` on a canvas larger or wider than the model's size (beyond the reference; `WindowedCompositeGuide`): a
        background prompt plus entity prompts in rectangles or soft masks given in CANVAS pixels, over `gen_wide`'s
        windows -- `size` is the image's (height, width), covered by overlapping `window`s at `stride` (image pixels; an
        int means both axes) whose predictions, each with the entities blended in, are averaged ('uniform') or tent-weighted
        ('tent') where they overlap.  Every other argument is `compose`'s, by keyword (`compose` itself keeps the
        reference's signature): `batch_size`, `masks`, `init_image` / `mask_image` of canvas size, `seed`, `steps`;
        `init_size` is `size`.  `Runner.guidance_rescale` is refused, as by `gen_wide`.'''
        given = inspect.signature(Runner.compose).bind(self, bg_prompt, entities_df, **compose_args)
        given.apply_defaults()
        given = dict(given.arguments)
        given['init_size'] = tuple(size)
        return self._compose(given, wide=(window, stride, blend))

    def _compose(self, given: Dict[str, Any], style_linear=None, wide=None):
        (bg_prompt, entities_df, start_style, end_style, style_blend, init_image, batches, strength, steps, guidance_scale,
         init_size, seed, debug, batch_size, masks, mask_image) = (given[k] for k in (
             'bg_prompt', 'entities_df', 'start_style', 'end_style', 'style_blend', 'init_image', 'batches', 'strength',
             'steps', 'guidance_scale', 'init_size', 'seed', 'debug', 'batch_size', 'masks', 'mask_image'))
        self._set_seed(seed)
        table = getattr(entities_df, '_values', entities_df)
        parsed = [entity_from_row(row) for row in table]
        if masks is not None:
            if len(masks) != len(parsed):
                raise ValueError(f'{len(masks)} masks for {len(parsed)} table rows')
            # attached before rows are dropped, so the alignment with the table holds
            parsed = [e if e is None or m is None else dataclasses.replace(e, mask=m) for e, m in zip(parsed, masks)]
        entities = [e for e in parsed if e is not None and e.prompt]
        self.last_schema = Schema(bg_prompt, start_style, end_style, style_blend, entities)
        extra = {'batch_size': batch_size} if batch_size != 1 else {}
        if style_linear is not None:
            extra['style_linear'] = style_linear
        if wide is not None:
            window, stride, blend = wide
            if self.guidance_rescale:
                raise ValueError('compose_wide does not support Runner.guidance_rescale: its standard deviations would have to '
                                 'span the canvas')
            guide = WindowedCompositeGuide(self.encoder, self.pipe.unet, guidance_scale, self.last_schema, steps,
                                           window=window, stride=stride, blend=blend, **extra)
        else:
            guide = CompositeGuide(self.encoder, self.pipe.unet, guidance_scale, self.last_schema, steps, **extra)
        # (only when given: a subclass's `_run` with the reference's six arguments keeps working)
        return self._run(batches, guide, init_image, init_size, strength, debug,
                         **({'mask_image': mask_image} if mask_image is not None else {}))
