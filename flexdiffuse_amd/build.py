'''Assembly of the model containers (the part of the reference's `utils.Runner.__init__`,
utils.py:54-76, that is not model download): state dicts -> device containers -> pipeline.'''
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import weights as W
from .clip import CLIPModel
from .scheduler import (DDIMScheduler, DPMSolverMultistepScheduler, LMSDiscreteScheduler, PNDMScheduler,
                        UniPCMultistepScheduler)
from .tokenizer import SyntheticTokenizer
from .unet import UNet2DConditionModel
from .vae import AutoencoderKL

import dataclasses

# SD2.x-style small model: linear proj_in/out, head dim 64, v-prediction (BASELINE config 5 shape)
MINI2_UNET = dataclasses.replace(W.MINI_UNET, num_heads=(5, 10, 20), use_linear_projection=True,
                                 prediction_type='v_prediction')

# the mini model with a text tower wide enough for a real byte-level BPE vocabulary (512 byte symbols + merges +
# the two specials): what the from-disk tests write as vocab.json / merges.txt
MINI_BPE_CLIP = dataclasses.replace(W.MINI_CLIP, text=dataclasses.replace(W.MINI_CLIP.text, vocab_size=1024))

PRESETS = {
    'mini_bpe': (W.MINI_UNET, W.MINI_VAE, MINI_BPE_CLIP),
    'sd15': (W.SD15_UNET, W.SD_VAE, W.CLIP_VIT_L14),
    'mini2': (MINI2_UNET, W.MINI_VAE, W.MINI_CLIP),
    'sd21': (W.SD21_UNET, W.SD_VAE, W.CLIP_VIT_H14),
    'mini': (W.MINI_UNET, W.MINI_VAE, W.MINI_CLIP),
}


def mini_unet_config(clip_cfg: W.CLIPConfig = W.MINI_CLIP) -> W.UNetConfig:
    import dataclasses
    return dataclasses.replace(W.MINI_UNET, cross_attention_dim=clip_cfg.text.hidden_size)


def synthetic_state_dicts(preset: str = 'sd15', seed: int = 0, branch_gain: float = 0.25,
                          parts=('unet', 'vae', 'clip')) -> Dict[str, dict]:
    '''Seeded fp32 CPU state dicts (HF key names) of the named architecture.'''
    ucfg, vcfg, ccfg = PRESETS[preset]
    if preset.startswith('mini'):
        ucfg = dataclasses.replace(ucfg, cross_attention_dim=ccfg.text.hidden_size)
    out = {}
    if 'unet' in parts:
        out['unet'] = W.synth_state_dict(W.unet_param_shapes(ucfg), seed, branch_gain, 'unet.')
    if 'vae' in parts:
        out['vae'] = W.synth_state_dict(W.vae_param_shapes(vcfg), seed, branch_gain, 'vae.')
    if 'clip' in parts:
        out['clip'] = W.synth_state_dict(W.clip_param_shapes(ccfg), seed, 1.0, 'clip.')
    return out


def stress_unet_state_dict(preset: str = 'sd15', seed: int = 0, branch_gain: float = 1.0, qk_gain: float = 1.5,
                           gn_shift: float = 6.0) -> dict:
    '''A UNet state dict in the numerical regime of TRAINED weights that the default synthetic ones avoid on purpose
    (VERDICT r4 weak 1): residual branches at `branch_gain` (default synthetic weights: 0.25), attention q / k projections
    x `qk_gain` (softmax logits x qk_gain^2: peaked rows instead of near-uniform ones), and every ResBlock conv1 bias
    shifted by +-`gn_shift` per 32-channel-group block (the GroupNorm that follows sees group means of ~10 sigma: the
    E[x^2] - E[x]^2 cancellation regime).  Test infrastructure for the fp16-storage paths, not a model of any checkpoint.

    Which combinations are parity targets at all is decided by the ORACLE: with random q / k weights the network turns
    chaotic once the softmax rows become one-hot -- at (branch_gain 1, qk_gain >= 3) a 2^-11 relative perturbation of the
    INPUT moves the fp32 oracle's own output by 80-100 % (tests/test_oracle_stress.py), so no fp16 implementation, the
    reference's autocast included, can be compared there.  The two presets the GPU test uses are the strongest
    well-conditioned corners: A = (1.0, 1.5, 6.0): unit gain + large group means; B = (0.25, 4.0, 6.0): logits x 16.'''
    ucfg = configs(preset)[0]
    sd = W.synth_state_dict(W.unet_param_shapes(ucfg), seed, branch_gain, 'unet.')
    g = torch.Generator('cpu').manual_seed(seed + 977)
    for k, v in sd.items():
        if qk_gain != 1.0 and k.endswith(('attn1.to_q.weight', 'attn1.to_k.weight', 'attn2.to_q.weight', 'attn2.to_k.weight')):
            sd[k] = v * qk_gain
        elif gn_shift and k.endswith('.conv1.bias'):
            groups = 32
            per = v.shape[0] // groups
            sign = (torch.randint(0, 2, (groups,), generator=g) * 2 - 1).float().repeat_interleave(per)
            sd[k] = v + gn_shift * sign
    return sd


# newer diffusers checkpoints name the VAE mid-block attention like the UNet's; the containers
# use the diffusers 0.3.0 names the reference was written against
_VAE_ATTN_ALIASES = (('.to_q.', '.query.'), ('.to_k.', '.key.'), ('.to_v.', '.value.'),
                     ('.to_out.0.', '.proj_attn.'))
_IGNORED_KEYS = ('position_ids',)   # buffers some transformers versions serialise


def _read_safetensors(path: str) -> Dict[str, torch.Tensor]:
    from safetensors import safe_open
    out = {}
    with safe_open(path, framework='pt', device='cpu') as f:
        for k in f.keys():
            out[k] = f.get_tensor(k)
    return out


def _read_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    '''.safetensors, or the torch-pickle .bin files the 2022 repositories shipped (tensors only:
    `weights_only=True`, nothing else in the pickle is executed).'''
    if path.endswith('.safetensors'):
        return _read_safetensors(path)
    sd = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(sd, dict) or not all(isinstance(v, torch.Tensor) for v in sd.values()):
        raise ValueError(f'{path} is not a flat name -> tensor state dict')
    return sd


def _fit(sd: Dict[str, torch.Tensor], shapes, what: str) -> Dict[str, torch.Tensor]:
    '''Check a loaded state dict against the architecture's parameter table (names AND shapes;
    a checkpoint of another architecture must fail loudly, not produce noise images).'''
    got = {}
    for k, v in sd.items():
        if k.endswith(_IGNORED_KEYS):
            continue
        for a, b in _VAE_ATTN_ALIASES:
            if what == 'vae' and a in k:
                k = k.replace(a, b)
        if what == 'vae' and k.endswith('.weight') and v.dim() == 4 and k in shapes and len(shapes[k]) == 2:
            v = v.reshape(v.shape[0], v.shape[1])       # 1x1-conv form of the attention projections
        got[k] = v
    missing = [k for k in shapes if k not in got]
    unexpected = [k for k in got if k not in shapes]
    bad = [(k, tuple(got[k].shape), tuple(shapes[k])) for k in shapes
           if k in got and tuple(got[k].shape) != tuple(shapes[k])]
    if missing or unexpected or bad:
        raise ValueError(f'{what} checkpoint does not match the architecture: {len(missing)} missing '
                         f'(e.g. {missing[:3]}), {len(unexpected)} unexpected (e.g. {unexpected[:3]}), '
                         f'{len(bad)} wrong shape (e.g. {bad[:3]})')
    return {k: got[k].float() for k in shapes}


def load_state_dicts(sd_dir: str, clip_dir: str, preset: str = 'sd15') -> Dict[str, dict]:
    '''Real weights from a local diffusers-layout directory and a CLIPModel directory -- what
    the reference's `Runner.__init__` downloads (utils.py:24-25, 59-68: "CompVis/stable-
    diffusion-v1-4" and "openai/clip-vit-large-patch14"); there is no network here, so the
    files must already be on disk.  `sd_dir` holds unet/ and vae/ with
    diffusion_pytorch_model.safetensors (or .bin), `clip_dir` holds model.safetensors (or
    pytorch_model.bin) of the full CLIPModel (text + vision tower + projections).  Returns the same {'unet','vae','clip'}
    dict of fp32 CPU tensors as `synthetic_state_dicts`, validated name-by-name and
    shape-by-shape against the preset's architecture.'''
    import os
    ucfg, vcfg, ccfg = configs(preset)

    def find(d, names):
        for n in names:
            if os.path.exists(os.path.join(d, n)):
                return os.path.join(d, n)
        raise FileNotFoundError(f'none of {names} under {d}')

    st = ('diffusion_pytorch_model.safetensors', 'diffusion_pytorch_model.fp16.safetensors',
          'diffusion_pytorch_model.bin')
    return {
        'unet': _fit(_read_checkpoint(find(os.path.join(sd_dir, 'unet'), st)),
                     W.unet_param_shapes(ucfg), 'unet'),
        'vae': _fit(_read_checkpoint(find(os.path.join(sd_dir, 'vae'), st)),
                    W.vae_param_shapes(vcfg), 'vae'),
        'clip': _fit(_read_checkpoint(find(clip_dir, ('model.safetensors', 'pytorch_model.bin'))),
                     W.clip_param_shapes(ccfg), 'clip'),
    }


def load_tokenizer(tokenizer_dir: str, text_cleanup: str = 'fast'):
    '''The real BPE tokenizer from vocab.json + merges.txt on disk (the tokenizer/ folder of the
    checkpoint the reference's Runner downloads, utils.py:61-63).  The containers only need
    `__call__(..., padding, max_length, truncation, return_tensors)` and `model_max_length`
    (encode/clip.py:57-63).  `text_cleanup`: 'basic' = the slow `CLIPTokenizer` without ftfy of the
    reference's pinned transformers 4.21.1 (BasicTokenizer first: accents stripped, every punctuation
    character its own piece); 'fast' = `CLIPTokenizerFast` / the ftfy path.  See CLIPBPETokenizer.'''
    from .tokenizer import CLIPBPETokenizer
    return CLIPBPETokenizer.from_pretrained(tokenizer_dir, text_cleanup=text_cleanup)


def load_scheduler(sd_dir: str, prediction_type: str = 'epsilon'):
    '''The scheduler the checkpoint itself ships (`sd_dir`/scheduler/scheduler_config.json), which is what the
    reference passes into its pipeline (utils.py:70: `sd.scheduler` -- PNDM/PLMS for CompVis/stable-diffusion-v1-4, so a
    50-step request is 51 UNet evaluations).  `_class_name` -> PNDMScheduler / LMSDiscreteScheduler / DDIMScheduler /
    DPMSolverMultistepScheduler / UniPCMultistepScheduler with the betas, `skip_prk_steps`, `steps_offset`, `set_alpha_to_one`, `clip_sample`,
    `solver_order`, `lower_order_final`, `rescale_betas_zero_snr` and (DDIM) `timestep_spacing` of the file.  None when the checkpoint has
    no scheduler folder; NotImplementedError for a class this package does not provide (never a silent substitute).'''
    import json
    import os
    path = os.path.join(sd_dir, 'scheduler', 'scheduler_config.json')
    if not os.path.exists(path):
        return None
    with open(path, encoding='utf-8') as f:
        cfg = json.load(f)
    name = cfg.get('_class_name', 'PNDMScheduler')
    # keys the file does not carry take DIFFUSERS' defaults (the class the reference would instantiate from this file:
    # linear betas 1e-4 .. 0.02, skip_prk_steps False), not this package's SD presets
    common = {'num_train_timesteps': cfg.get('num_train_timesteps', 1000), 'beta_start': cfg.get('beta_start', 0.0001),
              'beta_end': cfg.get('beta_end', 0.02), 'beta_schedule': cfg.get('beta_schedule', 'linear')}
    ptype = cfg.get('prediction_type', prediction_type)
    if name in ('PNDMScheduler', 'LMSDiscreteScheduler') and ptype != 'epsilon':
        # neither class has v-prediction arithmetic here: stepping a v-prediction UNet (SD2.1) as epsilon would be a
        # silently wrong image
        raise NotImplementedError(f'{path}: {name} with prediction_type {ptype!r} is not provided (epsilon only); pass '
                                  'scheduler=DDIMScheduler(prediction_type=...) to choose one explicitly')
    zero_snr = bool(cfg.get('rescale_betas_zero_snr', False))
    if zero_snr and ptype != 'v_prediction':
        # at the last timestep of that table alphas_cumprod is 0: an epsilon model's x0 divides by it (PNDM and K-LMS are
        # epsilon only, so the key is never dropped silently for them either)
        raise NotImplementedError(f'{path}: rescale_betas_zero_snr=True with prediction_type {ptype!r} is not provided '
                                  '(zero terminal SNR needs prediction_type \'v_prediction\')')
    if name == 'PNDMScheduler':
        extra = {'skip_prk_steps': cfg.get('skip_prk_steps', False), 'steps_offset': cfg.get('steps_offset', 0)}
        return PNDMScheduler(**common, **extra)
    if name == 'LMSDiscreteScheduler':
        return LMSDiscreteScheduler(**common)
    if name == 'DDIMScheduler':
        extra = {'clip_sample': cfg.get('clip_sample', True), 'set_alpha_to_one': cfg.get('set_alpha_to_one', True),
                 'steps_offset': cfg.get('steps_offset', 0)}
        spacing = cfg.get('timestep_spacing', 'leading')
        if spacing not in ('leading', 'trailing'):
            raise NotImplementedError(f'{path}: DDIMScheduler with timestep_spacing={spacing!r} is not provided (only '
                                      '\'leading\', \'trailing\'); pass scheduler= to choose one explicitly')
        return DDIMScheduler(**common, **extra, prediction_type=ptype, timestep_spacing=spacing,
                             rescale_betas_zero_snr=zero_snr)
    if name == 'DPMSolverMultistepScheduler':
        # DPM-Solver++ (2M), midpoint form, on the linspace grid is what is provided; every other variant the file can ask
        # for is refused by the key that asks for it
        for key, default, ok in (('algorithm_type', 'dpmsolver++', ('dpmsolver++',)), ('solver_type', 'midpoint', ('midpoint',)),
                                 ('solver_order', 2, (1, 2)), ('thresholding', False, (False,)),
                                 ('use_karras_sigmas', False, (False,)), ('timestep_spacing', 'linspace', ('linspace',))):
            if cfg.get(key, default) not in ok:
                raise NotImplementedError(f'{path}: DPMSolverMultistepScheduler with {key}={cfg[key]!r} is not provided '
                                          f'(only {", ".join(repr(v) for v in ok)}); pass scheduler= to choose one explicitly')
        return DPMSolverMultistepScheduler(**common, solver_order=cfg.get('solver_order', 2), prediction_type=ptype,
                                           lower_order_final=cfg.get('lower_order_final', True),
                                           rescale_betas_zero_snr=zero_snr)
    if name == 'UniPCMultistepScheduler':
        # the data-prediction form with its corrector on every step, on the linspace grid, is what is provided
        for key, default, ok in (('predict_x0', True, (True,)), ('solver_type', 'bh2', ('bh1', 'bh2')), ('solver_order', 2, (1, 2, 3)),
                                 ('thresholding', False, (False,)), ('disable_corrector', [], ([], None)),
                                 ('use_karras_sigmas', False, (False,)), ('timestep_spacing', 'linspace', ('linspace',)),
                                 ('rescale_betas_zero_snr', False, (False,))):
            if cfg.get(key, default) not in ok:
                raise NotImplementedError(f'{path}: UniPCMultistepScheduler with {key}={cfg[key]!r} is not provided '
                                          f'(only {", ".join(repr(v) for v in ok)}); pass scheduler= to choose one explicitly')
        return UniPCMultistepScheduler(**common, solver_order=cfg.get('solver_order', 2), solver_type=cfg.get('solver_type', 'bh2'),
                                       prediction_type=ptype, lower_order_final=cfg.get('lower_order_final', True))
    raise NotImplementedError(f'{path}: scheduler class {name!r} is not provided (PNDMScheduler, LMSDiscreteScheduler, '
                              'DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler are); pass scheduler= to choose '
                              'one explicitly')


def from_directories(sd_dir: str, clip_dir: str, tokenizer_dir: Optional[str] = None, preset: str = 'sd15',
                     device='cuda', scheduler=None, text_cleanup: str = 'basic', **kw):
    '''(pipeline, clip, tokenizer) from files on disk -- the local-files half of the reference's
    `Runner.__init__` (utils.py:59-71: CLIPModel.from_pretrained + StableDiffusionPipeline.from_pretrained
    -> FlexPipeline(sd.vae, clip, sd.tokenizer, sd.unet, sd.scheduler)).  The tokenizer comes from
    `tokenizer_dir`, else from `sd_dir`/tokenizer (where the SD checkpoint keeps it).
    Scheduler: `scheduler=` if given, else the checkpoint's own (`load_scheduler`: scheduler/scheduler_config.json, as the
    reference's `sd.scheduler`), else DDIM (a directory without a scheduler folder).  `text_cleanup` defaults to 'basic' here:
    the reference's pinned stack (transformers 4.21.1, slow CLIPTokenizer, no ftfy) tokenizes through BasicTokenizer, so a
    prompt with apostrophes, accents or punctuation gets the reference's ids; pass 'fast' for CLIPTokenizerFast's.'''
    import os
    sds = load_state_dicts(sd_dir, clip_dir, preset)
    tdir = tokenizer_dir or os.path.join(sd_dir, 'tokenizer')
    if not os.path.exists(os.path.join(tdir, 'vocab.json')):
        raise FileNotFoundError(f'no vocab.json under {tdir}: pass tokenizer_dir')
    if scheduler is None:
        scheduler = load_scheduler(sd_dir, configs(preset)[0].prediction_type)
    return build_models(sds, preset, device, tokenizer=load_tokenizer(tdir, text_cleanup), scheduler=scheduler, **kw)


def configs(preset: str):
    ucfg, vcfg, ccfg = PRESETS[preset]
    if preset.startswith('mini'):
        ucfg = dataclasses.replace(ucfg, cross_attention_dim=ccfg.text.hidden_size)
    return ucfg, vcfg, ccfg


def build_models(state_dicts: Dict[str, dict], preset: str = 'sd15', device='cuda',
                 vae_encoder: bool = True, steps_offset: int = 0, tokenizer=None, scheduler=None):
    '''(pipeline, clip, tokenizer): device containers + FlexPipeline around them.  `tokenizer`:
    e.g. `load_tokenizer(dir)`; default is the synthetic one (no vocabulary ships here).  `scheduler`: any of this
    package's schedulers (default: DDIM, the scheduler BASELINE's metric is quoted on).'''
    from .pipeline.flex import FlexPipeline
    ucfg, vcfg, ccfg = configs(preset)
    unet = UNet2DConditionModel(state_dicts['unet'], ucfg, device)
    vae = AutoencoderKL(state_dicts['vae'], vcfg, device, encoder=vae_encoder)
    clip = CLIPModel(state_dicts['clip'], ccfg, device)
    tok = tokenizer or SyntheticTokenizer(vocab_size=ccfg.text.vocab_size,
                                          model_max_length=ccfg.text.max_position_embeddings)
    sched = scheduler if scheduler is not None else DDIMScheduler(steps_offset=steps_offset, prediction_type=ucfg.prediction_type)
    pipe = FlexPipeline(vae, clip, tok, unet, sched).to(device)
    return pipe, clip, tok
