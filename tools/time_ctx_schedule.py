#!/usr/bin/env python
'''Per-step cost of a context schedule on the device loop: plain SimpleGuide against ScheduledGuide mode='lerp' (one
fd_lerp_f16 over the cached projections per step) and mode='project' (the blended context reprojected every step: one cast,
16 K GEMMs, 16 V^T GEMMs and the fd_xattn_pack_kv_f16 launches), same build, same session.

SD1.5 synthetic weights, 512 x 512, B = 2, guidance 8, DDIM, graph mode.  The three kinds of request are interleaved:
`--reps` (7) timed requests each at 10 and at 50 steps per kind; per-step cost = (median(50) - median(10)) / 40, which
cancels the text encoder, the keyframe projections, the VAE decode and every other per-request cost (the method of
tools/time_multistep.py).  Spread = half the range of the per-repetition estimates (t50_k - t10_k) / 40.  Prints one JSON
line.'''
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
    from flexdiffuse_amd import ScheduledGuide, SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    first = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    last = enc.prompt([('a castle at night', 'a bowl of fruit, watercolor')[i % 2] for i in range(args.batch)])
    kinds = ('plain', 'lerp', 'project')

    def guide(kind, steps):
        if kind == 'plain':
            return SimpleGuide(enc, pipe.unet, 8.0, steps, first)
        return ScheduledGuide(enc, pipe.unet, 8.0, steps, [first, last], mode=kind)

    def request(kind, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pipe(guide=guide(kind, steps), init_size=(args.size, args.size), generator=torch.Generator('cpu').manual_seed(3),
             output_type='np')
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for kind in kinds:                        # capture the graphs, warm every shape
        request(kind, 10)
        request(kind, 10)
    assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
    times = {(k, s): [] for k in kinds for s in (10, 50)}
    for _ in range(args.reps):
        for steps in (10, 50):
            for kind in kinds:
                times[(kind, steps)].append(request(kind, steps))
    out = {'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps, 'mode': 'graph', 'scheduler': 'ddim'}
    for kind in kinds:
        t10, t50 = times[(kind, 10)], times[(kind, 50)]
        per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
        out[kind] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                     'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                     'request_ms': {str(s): round(statistics.median(times[(kind, s)]), 2) for s in (10, 50)}}
    for kind in ('lerp', 'project'):
        out[f'{kind}_minus_plain_ms_per_step'] = round(out[kind]['ms_per_step'] - out['plain']['ms_per_step'], 4)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
