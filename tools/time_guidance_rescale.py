#!/usr/bin/env python
'''Per-step cost of guidance rescale on the device loop against the unrescaled request, same build, same session.

SD1.5 synthetic weights, 512 x 512, B = 2, guidance 8, DDIM, graph mode.  Plain and rescaled (`guidance_rescale=0.7`)
requests are interleaved: `--reps` (7) timed requests each at 10 and at 50 steps; per-step cost = (median(50) -
median(10)) / 40, which cancels the text encoder, the VAE decode and every other per-request cost (the method of
tools/time_multistep.py).  Spread = half the range of the per-repetition estimates (t50_k - t10_k) / 40.

The difference of two ~25 ms steps cannot resolve a few microseconds, so the step launch is also timed on its own: `--launches`
(200) back-to-back launches of fd_cfg_ddim_step_f32 and of fd_cfg_rescale_ddim_step_f32 on the request's shapes, replayed
from a launch plan between two events, median of `--reps` repetitions.  Prints one JSON line.'''
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
    ap.add_argument('--rescale', type=float, default=0.7)
    ap.add_argument('--launches', type=int, default=200)
    args = ap.parse_args()
    import torch
    from flexdiffuse_amd import SimpleGuide, build, hip, ops
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    kinds = {'plain': 0.0, 'rescaled': args.rescale}

    def request(kind, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb, guidance_rescale=kinds[kind]),
             init_size=(args.size, args.size), generator=torch.Generator('cpu').manual_seed(3), output_type='np')
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for kind in kinds:                        # capture the graph, warm every shape
        request(kind, 10)
        request(kind, 10)
    assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
    times = {(k, s): [] for k in kinds for s in (10, 50)}
    for _ in range(args.reps):
        for steps in (10, 50):
            for kind in kinds:
                times[(kind, steps)].append(request(kind, steps))
    out = {'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps, 'mode': 'graph',
           'rescale': args.rescale}
    for kind in kinds:
        t10, t50 = times[(kind, 10)], times[(kind, 50)]
        per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
        out[kind] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                     'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                     'request_ms': {str(s): round(statistics.median(times[(kind, s)]), 2) for s in (10, 50)}}
    out['rescaled_minus_plain_ms_per_step'] = round(out['rescaled']['ms_per_step'] - out['plain']['ms_per_step'], 4)

    # the step launch on its own, on the request's shapes
    B, C, HW = args.batch, 4, (args.size // 8) ** 2
    x = torch.randn((B, C, HW), device=dev)
    eps = torch.randn((2 * B * HW, C), device=dev)
    coef = (0.6, 0.8, 0.9, 0.3)
    calls = {'plain': lambda: ops.cfg_ddim_step(x, eps, B, C, HW, True, 8.0, coef),
             'rescaled': lambda: ops.cfg_rescale_ddim_step(x, eps, B, C, HW, 8.0, args.rescale, coef)}
    launch = {}
    for kind, call in calls.items():
        plan = hip.Plan()                     # replayed from C: the host cost of the Python front stays out of the figure
        with plan.record():
            for _ in range(args.launches):
                call()
        per_launch = []
        for _ in range(args.reps + 1):        # the first repetition warms up
            x.normal_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            plan.replay()
            b.record()
            torch.cuda.synchronize()
            per_launch.append(a.elapsed_time(b) * 1e3 / args.launches)
        launch[kind] = round(statistics.median(per_launch[1:]), 3)
    out['step_launch_us'] = launch
    print(json.dumps(out))


if __name__ == '__main__':
    main()
