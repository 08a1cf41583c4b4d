#!/usr/bin/env python
'''PLMS / K-LMS: the one-launch step (`pipe.fuse_linear_multistep = True`) against the planned route (False), same build, same
process, interleaved.

(a) Counts per step after the UNet, both arms, at order 4 on the request's shapes: library launches from the plan recorder
(`hip.Plan`), torch copies named, device allocations from the caching allocator's counter.

(b) Timing at bench.py's `--scheduler pndm` / `--scheduler lms` configuration (SD1.5 synthetic weights, 512 x 512, B = 8,
guidance 8, graph mode): the arms False, True, False again are interleaved, `--reps` (5) timed requests each at 10 and at 50
steps; per-step cost = (median(50) - median(10)) / 40, which cancels the text encoder, the VAE decode and every other
per-request cost (the method of tools/time_multistep.py).  The two False arms are the same code: their difference is the noise
the True arm's difference is judged against.  The final latents of the arms are compared bit for bit.  Prints one JSON line
per scheduler.'''
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def counts(kind, B, HW, dev, masked):
    '''(launches, allocations) of one order-4 step after the UNet: the planned arm's calls as FlexPipeline issues them
    (its `copy_` into the persistent buffer is a torch launch the recorder does not see: counted by hand), and `fused_step`.'''
    import torch
    from flexdiffuse_amd import hip, ops
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    C, g = 4, 8.0
    make = PNDMScheduler if kind == 'pndm' else LMSDiscreteScheduler
    x0, z0, n = (torch.randn((B, C, HW), device=dev) for _ in range(3))
    m = torch.rand((HW,), device=dev)
    eps = torch.randn((2 * B * HW, C), device=dev)
    buf, scaled = torch.empty_like(x0), torch.empty_like(x0)
    blend = lambda: (z0, n, m, 0.9, 0.4) if masked else None            # noqa: E731
    allocs = lambda: torch.cuda.memory_stats(dev)['allocation.all.allocated']   # noqa: E731
    out = {}
    for arm in ('planned', 'fused'):
        s = make()
        s.set_timesteps(50)
        args = list(range(50)) if kind == 'lms' else [int(t) for t in s.timesteps]
        x = x0.clone()
        for j, arg in enumerate(args[:7]):                               # order 4 from the fifth call (PLMS: the sixth) on
            plan = hip.Plan()
            a0 = allocs()
            with plan.record():
                if arm == 'fused':
                    extra = {'scaled_out': scaled, 'next_scale': 0.5} if kind == 'lms' else {}
                    s.fused_step(x, eps, arg, B, C, HW, True, g, blend(), **extra)
                    torch_launches = 0
                else:
                    inp = ops.axpby(x, None, 0.5, 0.0) if kind == 'lms' else x
                    buf.copy_(inp)
                    torch_launches = 1
                    pred = torch.empty_like(x)
                    ops.cfg_ddim_step(None, eps, B, C, HW, True, g, do_step=False, eps_out=pred)
                    x = s.step(pred, arg, x).prev_sample
                    if masked:
                        ops.cfg_ddim_masked_step(x, None, z0, n, m, B, C, HW, k1=0.9, k2=0.4)
            step = {'launches': len(plan) + torch_launches, 'allocations': allocs() - a0}
        out[arm] = step                                                  # the last one: order 4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--preset', default='sd15')
    ap.add_argument('--schedulers', default='pndm,lms')
    args = ap.parse_args()
    import torch
    from flexdiffuse_amd import SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    arms = {'planned_1': False, 'fused': True, 'planned_2': False}
    for kind in args.schedulers.split(','):
        make = PNDMScheduler if kind == 'pndm' else LMSDiscreteScheduler
        latents = {}

        def request(arm, steps):
            pipe.scheduler = make()
            pipe.fuse_linear_multistep = arms[arm]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb), init_size=(args.size, args.size),
                 generator=torch.Generator('cpu').manual_seed(3), output_type='np')
            torch.cuda.synchronize()
            latents[(arm, steps)] = pipe.last_latents
            return (time.perf_counter() - t0) * 1e3

        for arm in arms:                          # capture the graph, warm every shape
            request(arm, 10)
            request(arm, 10)
        assert pipe.use_graph and pipe.graph_fallback is None, pipe.graph_fallback
        times = {(a, s): [] for a in arms for s in (10, 50)}
        for _ in range(args.reps):
            for steps in (10, 50):
                for arm in arms:
                    times[(arm, steps)].append(request(arm, steps))
        out = {'scheduler': kind, 'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps,
               'mode': 'graph'}
        for arm in arms:
            t10, t50 = times[(arm, 10)], times[(arm, 50)]
            per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
            out[arm] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                        'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                        'request_ms': {str(s): round(statistics.median(times[(arm, s)]), 2) for s in (10, 50)}}
        out['noise_ms_per_step'] = round(abs(out['planned_1']['ms_per_step'] - out['planned_2']['ms_per_step']), 4)
        planned = (out['planned_1']['ms_per_step'] + out['planned_2']['ms_per_step']) / 2.0
        out['fused_minus_planned_ms_per_step'] = round(out['fused']['ms_per_step'] - planned, 4)
        out['fused_minus_planned_request50_ms'] = round(
            out['fused']['request_ms']['50'] - (out['planned_1']['request_ms']['50'] + out['planned_2']['request_ms']['50']) / 2.0, 2)
        out['bit_equal'] = all(torch.equal(latents[('fused', s)], latents[(a, s)]) for s in (10, 50) for a in arms)
        HW = (args.size // 8) ** 2
        out['per_step_counts'] = {'unmasked': counts(kind, args.batch, HW, dev, False),
                                  'masked': counts(kind, args.batch, HW, dev, True)}
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
