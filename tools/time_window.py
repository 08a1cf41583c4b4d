'''Windowed (MultiDiffusion) sampling, DESIGN.md sec. 7.2 "Cost": per-launch time of fd_window_step_f32 at the full-size shape
next to fd_cfg_ddim_step_f32 at 64x64 / B = 3, and the per-step time of the 512x1024 request against SimpleGuide at batch 3,
same process, alternating, with the box's clock over the timed region.  Also: the masked windowed DDIM step as the three
launches it used to be (step, blend-only, gather) against the one it is now, per step of back-to-back launches; and the
512x1024 request under DPM-Solver++ against the same request under DDIM, interleaved, (30-step - 10-step) / (steps run).
Prints one JSON line.  Usage: python tools/time_window.py'''
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

devmon = subprocess.Popen([sys.executable, os.path.join(ROOT, 'tools', 'devmon.py')], stdin=subprocess.PIPE,
                          stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
import torch  # noqa: E402

import bench  # noqa: E402
from flexdiffuse_amd import SimpleGuide, WindowedGuide, build, ops  # noqa: E402
from flexdiffuse_amd.encode.clip import CLIPEncoder  # noqa: E402
from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler  # noqa: E402

dev = torch.device('cuda:0')
res = {}
T0 = time.time()

# ---- kernels -------------------------------------------------------------------------------------------------------------
grid = (64, 128, 64, 64, 32, 32, 1, 3)
g = torch.Generator().manual_seed(0)
xw = torch.randn((1, 4, 64, 128), generator=g).to(dev)
ew = torch.randn((2 * 3 * 4096, 4), generator=g).to(dev)
wins = torch.empty((3, 4, 64, 64), device=dev)
xs = torch.randn((3, 4, 64, 64), generator=g).to(dev)
es = torch.randn((2 * 3 * 4096, 4), generator=g).to(dev)
coef = (0.6, 0.8, 0.9, 0.43589)


def k_window():
    ops.window_step(xw, wins, ew, 1, 4, grid, 0, True, 7.5, coef, False)


def k_tent():
    ops.window_step(xw, wins, ew, 1, 4, grid, 1, True, 7.5, coef, False)


def k_simple():
    ops.cfg_ddim_step(xs, es, 3, 4, 4096, True, 7.5, coef, False)


z0w, nzw = (torch.randn((1, 4, 64, 128), generator=g).to(dev) for _ in range(2))
maskw = torch.zeros((64, 128))
maskw[:, 60:] = 1.0
maskw[:, 56:60] = torch.tensor([0.2, 0.4, 0.6, 0.8])
maskw = maskw.to(dev)


def k_masked_three():
    '''The masked windowed DDIM step before fd_window_ddim_step_f32: step, blend-only, gather.'''
    ops.window_step(xw, None, ew, 1, 4, grid, 0, True, 7.5, coef, False)
    ops.cfg_ddim_masked_step(xw, None, z0w, nzw, maskw, 1, 4, 64 * 128, k1=0.9, k2=0.43589)
    ops.window_gather(xw, wins, 1, 4, grid)


def k_masked_one():
    ops.window_ddim_step(xw, wins, ew, 1, 4, grid, 0, True, 7.5, coef, False, (z0w, nzw, maskw, 0.9, 0.43589))


def per_launch(fn, n=500):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us


for fn in (k_window, k_tent, k_simple):
    per_launch(fn, 50)
res['kernel_us'] = {'fd_window_step_f32 uniform 64x128/3 windows': [], 'fd_window_step_f32 tent': [],
                    'fd_cfg_ddim_step_f32 64x64 B=3': []}
for _ in range(5):
    for key, fn in zip(res['kernel_us'], (k_window, k_tent, k_simple)):
        res['kernel_us'][key].append(round(per_launch(fn), 3))

for fn in (k_masked_three, k_masked_one):
    per_launch(fn, 50)
res['masked_step_us'] = {'step + blend-only + gather (three launches)': [], 'fd_window_ddim_step_f32 (one launch)': []}
for _ in range(5):
    for key, fn in zip(res['masked_step_us'], (k_masked_three, k_masked_one)):
        res['masked_step_us'][key].append(round(per_launch(fn), 3))

# ---- requests ------------------------------------------------------------------------------------------------------------
sds = build.synthetic_state_dicts('sd15', seed=0)
pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False)
enc = CLIPEncoder(clip, tok)
emb1 = enc.prompt(['a wide valley at dawn, oil painting'])
emb3 = enc.prompt(['a wide valley at dawn, oil painting', 'a photo of a turtle', 'zeus, oil painting'])
lat_w = torch.randn((1, 4, 64, 128), generator=g)
lat_s = torch.randn((3, 4, 64, 64), generator=g)


RAN = [0]                                        # steps the last request ran: its scheduler's timestep list (txt2img)


def wide(steps):
    pipe(guide=WindowedGuide(enc, pipe.unet, 8.0, steps, emb1, window=512, stride=256), init_size=(512, 1024), latents=lat_w,
         output_type='np')
    RAN[0] = len(pipe.scheduler.timesteps)


def simple(steps):
    pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb3), init_size=(512, 512), latents=lat_s, output_type='np')
    RAN[0] = len(pipe.scheduler.timesteps)


REGIONS = {}                                     # key -> [(t0, t1)] wall-clock spans of its 30-step requests, for the clock


STEPS_RUN = {}                                   # key -> (steps the 10-step request ran, steps the 30-step request ran)


def per_step(fn, key=None):
    '''(time of the 30-step request - time of the 10-step request) / (the difference of the steps they RAN): the decode and
    the set-up cancel.  The divisor is read off the scheduler: DDIM's leading spacing, arange(0, T, T // n), makes 31
    timesteps of n = 30 (and 10 of n = 10), DPM-Solver++'s linspace makes 30 -- dividing both by 20 would charge DDIM's
    extra UNet step to its per-step time.'''
    out, ran = [], []
    for steps in (10, 30):
        torch.cuda.synchronize()
        t, w = time.perf_counter(), time.time()
        fn(steps)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
        ran.append(RAN[0])
        if steps == 30 and key is not None:
            REGIONS.setdefault(key, []).append((w, time.time()))
    if key is not None:
        STEPS_RUN[key] = tuple(ran)
    return (out[1] - out[0]) / (ran[1] - ran[0]) * 1e3, out     # ms


def clocks_by_region(proc, t0, t1):
    '''bench.devmon_collect's record over [t0, t1], plus the average gfx clock and power inside each key's own spans: the loops
    are power-capped, so two requests with different activations need not run at the same clock.'''
    raw, _ = proc.communicate(input=b'', timeout=20)
    rec = json.loads(raw.decode().strip().splitlines()[-1])
    samples = rec.get('samples', [])

    def mean(spans, col):
        v = [s[col] for s in samples if len(s) > col and s[col] is not None and any(a <= s[0] <= b for a, b in spans)]
        return (round(sum(v) / len(v), 1), len(v)) if v else (None, 0)
    out = {'clock_source': rec.get('source'), 'clock_device_bdf': rec.get('bdf')}
    for key, spans in [('all requests', [(t0, t1)])] + sorted(REGIONS.items()):
        (clk, n), (pw, _) = mean(spans, 1), mean(spans, 2)
        out[key] = {'avg_sclk_mhz': clk, 'avg_power_w': pw, 'clock_samples': n}
    return out


for fn in (wide, simple):
    fn(10)                                       # warm-up: capture, lazy set-up
res['step_ms'] = {'windowed 512x1024 (3 windows, CFG batch 6)': [], 'SimpleGuide B=3 512x512 (CFG batch 6)': []}
t_req0 = time.time()
for _ in range(3):
    for key, fn in zip(res['step_ms'], (wide, simple)):
        res['step_ms'][key].append(round(per_step(fn, key)[0], 3))

# DPM-Solver++ against DDIM on the windowed request, interleaved: one launch after the UNet on both
ddim_sched, dpm_sched = pipe.scheduler, DPMSolverMultistepScheduler()


def wide_under(sched):
    def fn(steps):
        pipe.scheduler = sched
        try:
            wide(steps)
        finally:
            pipe.scheduler = ddim_sched
    return fn


wide_under(dpm_sched)(10)
res['step_ms_scheduler'] = {'windowed 512x1024 DPM-Solver++': [], 'windowed 512x1024 DDIM': []}
for _ in range(5):
    for key, fn in zip(res['step_ms_scheduler'], (wide_under(dpm_sched), wide_under(ddim_sched))):
        res['step_ms_scheduler'][key].append(round(per_step(fn, key)[0], 3))
T1 = time.time()
res['steps_run'] = {k: list(v) for k, v in STEPS_RUN.items()}
res['graph_fallback'] = pipe.graph_fallback
res['clock_requests'] = clocks_by_region(devmon, t_req0, T1)
res['device'] = torch.cuda.get_device_name(0)
print(json.dumps(res))
