#!/usr/bin/env python
'''Per-step cost of the device loop under DPM-Solver++ (2M) against DDIM, same build, same session.

SD1.5 synthetic weights, 512 x 512, B = 2, guidance 8, graph mode.  DDIM and DPM-Solver++ requests are interleaved:
`--reps` (7) timed requests each at 10 and at 50 steps per scheduler; per-step cost = (median(50) - median(10)) / 40, which
cancels the text encoder, the VAE decode and every other per-request cost (the method of the inpainting record in
DESIGN.md sec. 7).  Spread = half the range of the per-repetition estimates (t50_k - t10_k) / 40.  Prints one JSON line.

The user-level figure (20 DPM-Solver++ steps against 50 DDIM steps) follows from the step counts and is printed as
arithmetic on the measured per-step and per-request costs, not as a kernel speed-up.'''
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
    from flexdiffuse_amd import SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    ptype = build.configs(args.preset)[0].prediction_type
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    scheds = {'ddim': DDIMScheduler(prediction_type=ptype), 'dpm': DPMSolverMultistepScheduler(prediction_type=ptype)}

    def request(kind, steps):
        pipe.scheduler = scheds[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb), init_size=(args.size, args.size),
             generator=torch.Generator('cpu').manual_seed(3), output_type='np')
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for kind in scheds:                       # capture the graph, warm every shape
        request(kind, 10)
        request(kind, 10)
    assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
    times = {(k, s): [] for k in scheds for s in (10, 20, 50)}
    for _ in range(args.reps):
        for steps in (10, 50, 20):
            for kind in scheds:
                times[(kind, steps)].append(request(kind, steps))
    out = {'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps, 'mode': 'graph'}
    for kind in scheds:
        t10, t50 = times[(kind, 10)], times[(kind, 50)]
        per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
        out[kind] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                     'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                     'request_ms': {str(s): round(statistics.median(times[(kind, s)]), 2) for s in (10, 20, 50)}}
    out['dpm_minus_ddim_ms_per_step'] = round(out['dpm']['ms_per_step'] - out['ddim']['ms_per_step'], 4)
    # arithmetic on the step counts: images/s of a 20-step DPM-Solver++ request against a 50-step DDIM request
    out['images_per_s'] = {'dpm_20_steps': round(args.batch * 1e3 / out['dpm']['request_ms']['20'], 3),
                           'ddim_50_steps': round(args.batch * 1e3 / out['ddim']['request_ms']['50'], 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
