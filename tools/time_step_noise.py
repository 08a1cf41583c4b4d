#!/usr/bin/env python
'''Per-step cost of the device loop with in-kernel step noise against the deterministic step, same build, same session.

SD1.5 synthetic weights, 512 x 512, B = 2, guidance 8, graph mode.  Five kinds of request are interleaved: DDIM eta = 0
(`ddim`), DDIM eta = 0.5 with `pipe.step_noise` (`ddim_noise`: fd_cfg_ddim_noise_step_f32 on the fused loop), DDIM eta = 0.5
without it (`ddim_generator`: the host draw per step on the planned route), DPM-Solver++ (`dpm`) and its SDE form (`sde`).
`--reps` (7) timed requests each at 10 and at 50 steps per kind; per-step cost = (median(50) - median(10)) / 40, which
cancels the text encoder, the VAE decode and every other per-request cost (the method of tools/time_multistep.py).
Spread = half the range of the per-repetition estimates (t50_k - t10_k) / 40.  Prints one JSON line.'''
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--preset', default='sd15')
    args = ap.parse_args()
    import torch
    from flexdiffuse_amd import PhiloxNoise, SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    ptype = build.configs(args.preset)[0].prediction_type
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    ddim = DDIMScheduler(prediction_type=ptype)
    # kind -> (scheduler, eta, step noise)
    scheds = {'ddim': (ddim, 0.0, None), 'ddim_noise': (ddim, 0.5, PhiloxNoise(3)), 'ddim_generator': (ddim, 0.5, None),
              'dpm': (DPMSolverMultistepScheduler(prediction_type=ptype), 0.0, None),
              'sde': (DPMSolverMultistepSDEScheduler(prediction_type=ptype), 0.0, None)}

    def request(kind, steps):
        pipe.scheduler, eta, pipe.step_noise = scheds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb), init_size=(args.size, args.size), eta=eta,
             generator=torch.Generator('cpu').manual_seed(3), output_type='np')
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for kind in scheds:                       # capture the graph, warm every shape
        request(kind, 10)
        request(kind, 10)
    assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
    times = {(k, s): [] for k in scheds for s in (10, 50)}
    for _ in range(args.reps):
        for steps in (10, 50):
            for kind in scheds:
                times[(kind, steps)].append(request(kind, steps))
    out = {'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps, 'mode': 'graph'}
    for kind in scheds:
        t10, t50 = times[(kind, 10)], times[(kind, 50)]
        per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
        out[kind] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                     'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                     'request_ms': {str(s): round(statistics.median(times[(kind, s)]), 2) for s in (10, 50)}}
    for a, b in (('ddim_noise', 'ddim'), ('ddim_generator', 'ddim'), ('sde', 'dpm')):
        out[f'{a}_minus_{b}_ms_per_step'] = round(out[a]['ms_per_step'] - out[b]['ms_per_step'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
