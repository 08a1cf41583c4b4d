'''Forward time with and without the context-folded cross-attention (ops.XATTN_FOLD), in the form of tools/ab_unet_knob2.py: one process, one
launch plan per arm, interleaved rounds on the same box.  Two warm-up rounds per arm are discarded (the first rounds of a fresh process sit
10-20 us high while the clocks settle), then ROUNDS rounds of FWD forwards per arm; prints the round means, the medians, the spread (max - min)
of the unfolded arm's rounds and the improvement in units of that spread.
    python tools/ab_xattn_fold_forward.py [rounds = 8] [forwards per round = 40]'''
import sys, os, time; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flexdiffuse_amd import build, hip, ops
from flexdiffuse_amd.unet import UNet2DConditionModel
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 8
FWD = int(sys.argv[2]) if len(sys.argv) > 2 else 40
assert ROUNDS >= 6 and FWD >= 20
dev = torch.device('cuda:0')
sds = build.synthetic_state_dicts('sd15', seed=0, parts=('unet',))
unet = UNet2DConditionModel(sds['unet'], build.configs('sd15')[0], dev)
x = torch.randn((8, 4, 64, 64), device=dev); ctx = torch.randn((16, 77, 768), device=dev).half()
t_dev = torch.full((1,), 400.0, device=dev)
assert ops.XATTN_FOLD
plans = {}
for arm, on in (('folded', True), ('unfolded', False)):      # (the context is folded by the first forward; the knob is read per block)
    ops.XATTN_FOLD = on
    unet.forward_nhwc(x, t_dev, ctx, rep=2)
    pool = torch.cuda.MemPool(); plan = hip.Plan()
    with torch.cuda.use_mem_pool(pool, device=dev), plan.record():
        eps = unet.forward_nhwc(x, t_dev, ctx, rep=2)
    plans[arm] = (plan, pool, eps, len(plan))
ops.XATTN_FOLD = True
torch.cuda.synchronize()
res = {a: [] for a in plans}
for r in range(ROUNDS + 2):
    for a in plans:
        plan = plans[a][0]
        for _ in range(3): plan.replay()
        torch.cuda.synchronize(); t0 = time.time()
        for _ in range(FWD): plan.replay()
        torch.cuda.synchronize()
        if r >= 2:
            res[a].append(1e3 * (time.time() - t0) / FWD)
med = {}
for a in plans:
    v = sorted(res[a]); n = len(v)
    med[a] = 0.5 * (v[(n - 1) // 2] + v[n // 2])
    print(f'{a}: {plans[a][3]} launches per forward; ms per forward, {ROUNDS} rounds of {FWD}: {" ".join(f"{t:.3f}" for t in res[a])}; median {med[a]:.3f}')
spread = max(res['unfolded']) - min(res['unfolded'])
gain = med['unfolded'] - med['folded']
a, b = plans['folded'][2].float(), plans['unfolded'][2].float()
print(f'improvement {gain:.3f} ms per forward ({100 * gain / med["unfolded"]:.2f} %); spread of the unfolded arm {spread:.3f} ms; improvement / spread {gain / max(spread, 1e-9):.1f} (a gain needs > 5)')
print(f'max |eps folded - eps unfolded| {float((a - b).abs().max()):.3g}; PSNR {float(10 * torch.log10((b.max() - b.min()) ** 2 / (a - b).pow(2).mean())):.1f} dB')
