#!/usr/bin/env python
'''Tiled VAE decode (`AutoencoderKL.enable_tiling`, one fd_tile_blend_f32 launch) against the untiled decode, same build, same
process, interleaved, on the SD synthetic VAE weights (decoder only), one device.

  1. 1024 x 1024, where both run: the arms untiled, tiled, untiled again are interleaved, `--reps` (5) timed decodes each, every
     decode ending in a device synchronise.  The two untiled arms are the same code: their difference is the run-to-run spread
     the tiled arm's difference is judged against.
  2. tiled decode alone at 1024 x 2048 and 2048 x 2048 (the untiled path is not run there: its score matrix is 2 GiB and 8 GiB).
  3. the blend launch alone on the tile batch of each size (device events around `--blend-reps` (20) launches), and its bytes --
     16 B per tile pixel read (ld = 4 fp32), 12 B per canvas pixel written -- over that time against the HBM rate of a float4
     copy on this part (6.29 TB/s measured, 8.0 TB/s specified).
  4. torch.cuda.max_memory_allocated of each arm (reset before the arm; the weights are resident throughout and included).
  5. the PSNR of the tiled against the untiled image at 1024 x 1024 -- for the record only: tiling changes the GroupNorm
     statistics and the attention extent by design, and the weights are synthetic, so no closeness is claimed.

Defaults: tile 64, stride 48, feather 16 latent cells.  The device clock printed is the nominal one the runtime reports; the
sustained clock during the run is not sampled.  One JSON line per size, printed and written to `--out`.'''
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--blend-reps', type=int, default=20)
    ap.add_argument('--sizes', default='1024x1024,1024x2048,2048x2048', help='image sizes H x W; the first also runs untiled')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_tiling.txt'))
    args = ap.parse_args()
    import torch
    from flexdiffuse_amd import build, hip, ops
    from flexdiffuse_amd.vae import AutoencoderKL
    from flexdiffuse_amd.weights import SD_VAE
    dev = torch.device('cuda:0')
    sd = build.synthetic_state_dicts('sd15', seed=0, parts=('vae',))['vae']
    vae = AutoencoderKL(sd, SD_VAE, dev, encoder=False)
    f = vae.scale_factor
    info = hip.device_info(0)
    sizes = [tuple(int(v) for v in s.split('x')) for s in args.sizes.split(',')]
    decode_args = (1.0 / 0.18215, 0.5, 0.5, True)

    def decode(z, tiled):
        vae.enable_tiling() if tiled else vae.disable_tiling()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.perf_counter()
        img = vae.decode_image(z, *decode_args)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated(dev), img

    lines = []
    for k, (H, W) in enumerate(sizes):
        z = torch.randn((1, 4, H // f, W // f), generator=torch.Generator().manual_seed(17)).to(dev)
        arms = {'untiled_1': False, 'tiled': True, 'untiled_2': False} if k == 0 else {'tiled': True}
        images = {}
        for arm, tiled in arms.items():               # warm every shape
            decode(z, tiled)
        seen = {arm: [] for arm in arms}
        for _ in range(args.reps):
            for arm, tiled in arms.items():
                ms, peak, images[arm] = decode(z, tiled)
                seen[arm].append((ms, peak))
        vae.enable_tiling()
        g = vae.tile_grid(H // f, W // f)
        out = {'image': [H, W], 'tiles': [g.ny, g.nx], 'tile_cells': [g.h, g.w], 'stride_cells': [g.stride_y, g.stride_x],
               'feather_cells': list(vae.tiling.feather), 'reps': args.reps, 'arch': info['arch'],
               'nominal_clock_mhz': info['clock_khz'] // 1000, 'sustained_clock': 'not sampled'}
        for arm in arms:
            ms = [r[0] for r in seen[arm]]
            out[arm] = {'decode_ms_median': round(statistics.median(ms), 3), 'decode_ms_min': round(min(ms), 3),
                        'decode_ms_max': round(max(ms), 3), 'max_memory_allocated_mib': round(max(r[1] for r in seen[arm]) / 2 ** 20, 1)}
        if k == 0:
            out['untiled_run_to_run_ms'] = round(abs(out['untiled_1']['decode_ms_median'] - out['untiled_2']['decode_ms_median']), 3)
            off = (out['untiled_1']['decode_ms_median'] + out['untiled_2']['decode_ms_median']) / 2.0
            out['tiled_minus_untiled_ms'] = round(out['tiled']['decode_ms_median'] - off, 3)
            out['untiled_bit_equal'] = bool(torch.equal(images['untiled_1'], images['untiled_2']))
            mse = float(((images['tiled'].double() - images['untiled_1'].double()) ** 2).mean())
            out['psnr_tiled_vs_untiled_db_record_only'] = round(10.0 * torch.log10(torch.tensor(1.0 / max(mse, 1e-20))).item(), 2)
        # the blend launch alone, on a tile batch of this size
        gp = g.scaled(f)
        tiles = torch.randn((g.count * gp.h * gp.w, 4), generator=torch.Generator().manual_seed(1)).to(dev)
        canvas = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        blend = lambda: ops.tile_blend(tiles, 1, 3, gp.args, vae.tiling.feather_of(f), 0.5, 0.5, True, out=canvas)   # noqa: E731
        for _ in range(3):
            blend()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.blend_reps):
            blend()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.blend_reps
        nbytes = 16 * g.count * gp.h * gp.w + 12 * H * W
        out['blend'] = {'us_per_launch': round(us, 2), 'bytes': nbytes, 'tb_per_s': round(nbytes / us / 1e6, 3),
                        'share_of_hbm_copy_rate': round(nbytes / us / 1e6 / HBM_COPY_TBS, 3), 'launches_timed': args.blend_reps,
                        'share_of_tiled_decode': round(us / 1e3 / out['tiled']['decode_ms_median'], 4)}
        vae.disable_tiling()
        del tiles, canvas, images
        torch.cuda.empty_cache()
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w', encoding='utf-8') as fh:
        fh.write(__doc__.strip() + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
