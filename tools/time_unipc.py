#!/usr/bin/env python
'''Per-step cost of the device loop under UniPC against DPM-Solver++ (2M), same build, same process.

SD1.5 synthetic weights, 512 x 512, B = 2, guidance 8, graph mode.  The requests are interleaved in the order dpm_1, unipc,
dpm_2 (two arms of the SAME DPM-Solver++ scheduler class, so their difference is the run-to-run spread of that arm itself):
`--reps` (7) timed requests each at 10 and at 50 steps per arm; per-step cost = (median(50) - median(10)) / 40, which cancels the
text encoder, the VAE decode and every other per-request cost (the method of tools/time_multistep.py).  Spread = half the range
of the per-repetition estimates (t50_k - t10_k) / 40.  Prints one JSON line, the device's clock as the runtime reports it
included.

The expectation is parity: both steps are one launch of the same kernel family after a UNet of 7-15 ms, UniPC's reads three more
rows.  What UniPC buys is fewer steps at the same quality; "10 UniPC steps against 20 DPM-Solver++ steps" is printed as
arithmetic on the measured request times, not as a kernel speed-up.'''
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
    ap.add_argument('--solver-order', type=int, default=2)
    args = ap.parse_args()
    import torch
    from flexdiffuse_amd import SimpleGuide, build, hip
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler, UniPCMultistepScheduler
    dev = torch.device('cuda:0')
    sds = build.synthetic_state_dicts(args.preset, seed=0)
    ptype = build.configs(args.preset)[0].prediction_type
    pipe, clip, tok = build.build_models(sds, args.preset, dev, vae_encoder=False)
    pipe.pause_gc = True
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt([('a photo of a turtle in a forest', 'zeus, oil painting')[i % 2] for i in range(args.batch)])
    scheds = {'dpm_1': DPMSolverMultistepScheduler(prediction_type=ptype),
              'unipc': UniPCMultistepScheduler(prediction_type=ptype, solver_order=args.solver_order),
              'dpm_2': DPMSolverMultistepScheduler(prediction_type=ptype)}

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
    info = hip.device_info(0)
    out = {'preset': args.preset, 'size': args.size, 'batch': args.batch, 'reps': args.reps, 'mode': 'graph',
           'solver_order': args.solver_order,
           'device': {'cu_count': info['cu_count'], 'nominal_clock_mhz': info['clock_khz'] // 1000, 'sustained_clock': 'not sampled'}}
    for kind in scheds:
        t10, t50 = times[(kind, 10)], times[(kind, 50)]
        per = [(b - a) / 40.0 for a, b in zip(t10, t50)]
        out[kind] = {'ms_per_step': round((statistics.median(t50) - statistics.median(t10)) / 40.0, 4),
                     'spread_ms': round((max(per) - min(per)) / 2.0, 4),
                     'request_ms': {str(s): round(statistics.median(times[(kind, s)]), 2) for s in (10, 20, 50)}}
    dpm = (out['dpm_1']['ms_per_step'] + out['dpm_2']['ms_per_step']) / 2.0
    out['noise_ms_per_step'] = round(abs(out['dpm_1']['ms_per_step'] - out['dpm_2']['ms_per_step']), 4)
    out['unipc_minus_dpm_ms_per_step'] = round(out['unipc']['ms_per_step'] - dpm, 4)
    # arithmetic on the step counts: images/s of a 10-step UniPC request against a 20-step DPM-Solver++ request
    out['images_per_s'] = {'unipc_10_steps': round(args.batch * 1e3 / out['unipc']['request_ms']['10'], 3),
                           'dpm_20_steps': round(args.batch * 1e3 / out['dpm_1']['request_ms']['20'], 3)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
