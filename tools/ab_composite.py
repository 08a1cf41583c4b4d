#!/usr/bin/env python
'''CompositeGuide: the one-launch device loop (`pipe.fuse_composite = True`) against the earlier routes (False), same build,
same process, interleaved.

Two requests on the SD1.5 synthetic weights at 512 x 512, guidance 8, graph mode:
  compose-default   what `Runner.compose(...)` issues with its defaults: PNDM (PLMS), batch 1, two rectangle entities.  Off arm:
                    `guide.noise_pred` (an eager forward over the 4 context blocks, nhwc_to_nchw, one fd_region_blend_f32 per
                    entity, the combine) + `scheduler.step`'s chain.  On arm: graph replay + fd_composite_linear_multistep_step_f32.
  batched-masked    `--batch` (4) samples, one soft entity mask and one rectangle, DPM-Solver++.  Off arm: graph replay,
                    the combine-only fd_composite_step_f32, `scheduler.step`.  On arm: replay + fd_composite_multistep_step_f32.

The arms off, on, off again are interleaved, `--reps` (3) timed requests each at `--short` (10) and `--long` (30) steps, every
request ending in a device synchronise; per-step figures are (median(long) - median(short)) / (long - short), which cancels the
text encoder, the VAE decode and every other per-request cost.  The two off arms are the same code: their difference is the
run-to-run spread the on arm's difference is judged against.  The same differencing gives, per step, the library calls the
host issues (hip.call; a graph replay and torch's own copies are not among them) and the caching allocator's allocations.  The
final latents of the arms are compared bit for bit.  The device clock printed is the nominal one the runtime reports; the
sustained clock during the run is not sampled.  One JSON line per request, printed and written to `--out`.'''
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--preset', default='sd15')
    ap.add_argument('--short', type=int, default=10)
    ap.add_argument('--long', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'composite_ab.txt'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from flexdiffuse_amd import build, hip
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler, PNDMScheduler
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    S = args.size
    px = lambda v: v * S // 512 // 8 * 8                                         # noqa: E731 -- the 512 x 512 layout, scaled
    deer, bird = ((px(64), px(128)), (px(256), px(192))), ((px(320), 0), (px(192), px(192)))
    soft = np.random.default_rng(1).random((deer[1][1], deer[1][0])).astype(np.float32)
    soft[soft < 0.3] = 0.0
    requests = {
        'compose-default': (PNDMScheduler, 1, [EntitySchema('a deer', *deer, 0.8), EntitySchema('a red bird', *bird, 0.5)]),
        'batched-masked': (DPMSolverMultistepScheduler, args.batch,
                           [EntitySchema('a deer', *deer, 0.8, soft), EntitySchema('a red bird', *bird, 0.5)]),
    }
    arms = {'off_1': False, 'on': True, 'off_2': False}
    calls = [0]
    call = hip.call

    def counting(name, *a):
        calls[0] += 1
        return call(name, *a)
    hip.call = counting
    allocs = lambda: torch.cuda.memory_stats(dev)['allocation.all.allocated']   # noqa: E731
    lines = []
    info = hip.device_info(0)
    for name, (make, B, entities) in requests.items():
        schema = Schema('a forest at dawn, oil painting', '', '', (0.0, 1.0), entities)
        latents = {}

        def request(arm, steps):
            pipe.scheduler = make()
            pipe.fuse_composite = arms[arm]
            guide = CompositeGuide(enc, pipe.unet, 8.0, schema, steps, batch_size=B)
            torch.cuda.synchronize()
            c0, a0, t0 = calls[0], allocs(), time.perf_counter()
            pipe(guide=guide, init_size=(S, S), generator=torch.Generator('cpu').manual_seed(3), output_type='np')
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            latents[(arm, steps)] = pipe.last_latents
            return ms, calls[0] - c0, allocs() - a0

        for arm in arms:                          # capture the graph, warm every shape
            request(arm, args.short)
            request(arm, args.short)
        assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
        seen = {(a, s): [] for a in arms for s in (args.short, args.long)}
        for _ in range(args.reps):
            for steps in (args.short, args.long):
                for arm in arms:
                    seen[(arm, steps)].append(request(arm, steps))
        span = float(args.long - args.short)
        out = {'request': name, 'preset': args.preset, 'size': S, 'batch': B, 'scheduler': make.__name__, 'entities': len(entities),
               'reps': args.reps, 'steps': [args.short, args.long], 'mode': 'graph', 'arch': info['arch'],
               'nominal_clock_mhz': info['clock_khz'] // 1000, 'sustained_clock': 'not sampled'}
        for arm in arms:
            lo, hi = seen[(arm, args.short)], seen[(arm, args.long)]
            med = lambda rows, k: statistics.median(r[k] for r in rows)          # noqa: E731
            per = [(b[0] - a[0]) / span for a, b in zip(lo, hi)]
            out[arm] = {'ms_per_step': round((med(hi, 0) - med(lo, 0)) / span, 4),
                        'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                        'library_calls_per_step': round((med(hi, 1) - med(lo, 1)) / span, 2),
                        'allocations_per_step': round((med(hi, 2) - med(lo, 2)) / span, 2),
                        'request_ms': {str(s): round(med(seen[(arm, s)], 0), 2) for s in (args.short, args.long)}}
        out['off_run_to_run_ms_per_step'] = round(abs(out['off_1']['ms_per_step'] - out['off_2']['ms_per_step']), 4)
        off = (out['off_1']['ms_per_step'] + out['off_2']['ms_per_step']) / 2.0
        out['on_minus_off_ms_per_step'] = round(out['on']['ms_per_step'] - off, 4)
        out['bit_equal'] = all(torch.equal(latents[('on', s)], latents[(a, s)]) for s in (args.short, args.long) for a in arms)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    hip.call = call
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w', encoding='utf-8') as f:
        f.write(__doc__.strip() + '\n\n' + '\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
