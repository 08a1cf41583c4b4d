'''Windowed (MultiDiffusion) sampling, DESIGN.md sec. 7.2 "Cost": per-launch time of fd_window_step_f32 at the full-size shape
next to fd_cfg_ddim_step_f32 at 64x64 / B = 3, and the per-step time of the 512x1024 request against SimpleGuide at batch 3,
same process, alternating, with the box's clock over the timed region.  Prints one JSON line.  Usage: python tools/time_window.py'''
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

# ---- requests ------------------------------------------------------------------------------------------------------------
sds = build.synthetic_state_dicts('sd15', seed=0)
pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False)
enc = CLIPEncoder(clip, tok)
emb1 = enc.prompt(['a wide valley at dawn, oil painting'])
emb3 = enc.prompt(['a wide valley at dawn, oil painting', 'a photo of a turtle', 'zeus, oil painting'])
lat_w = torch.randn((1, 4, 64, 128), generator=g)
lat_s = torch.randn((3, 4, 64, 64), generator=g)


def wide(steps):
    pipe(guide=WindowedGuide(enc, pipe.unet, 8.0, steps, emb1, window=512, stride=256), init_size=(512, 1024), latents=lat_w,
         output_type='np')


def simple(steps):
    pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, steps, emb3), init_size=(512, 512), latents=lat_s, output_type='np')


def per_step(fn):
    '''(time of 30 steps - time of 10 steps) / 20: the decode and the set-up cancel.'''
    out = []
    for steps in (10, 30):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn(steps)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return (out[1] - out[0]) / 20 * 1e3, out     # ms


for fn in (wide, simple):
    fn(10)                                       # warm-up: capture, lazy set-up
res['step_ms'] = {'windowed 512x1024 (3 windows, CFG batch 6)': [], 'SimpleGuide B=3 512x512 (CFG batch 6)': []}
t_req0 = time.time()
for _ in range(3):
    for key, fn in zip(res['step_ms'], (wide, simple)):
        res['step_ms'][key].append(round(per_step(fn)[0], 3))
T1 = time.time()
res['graph_fallback'] = pipe.graph_fallback
res['clock_requests'] = bench.devmon_collect(devmon, t_req0, T1)
res['device'] = torch.cuda.get_device_name(0)
print(json.dumps(res))
