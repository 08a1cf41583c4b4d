'''Per-launch times of the context-folded cross-attention against the launches it replaces, at the 16x16 and 8x8 levels of the bench forward
(CFG batch 16, C = 1280, 8 heads, 77 keys): q projection (LayerNorm fold) + fd_attention_f16 + out projection (residual, statistics out) against
launch 1 (tile 24 / 25) + launch 2.  Device events around 50 back-to-back launches of one kind, 5 interleaved rounds, medians in us.
    python tools/ab_xattn_fold.py'''
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from flexdiffuse_amd import hip, ops
dev = torch.device('cuda:0')
C, H, DH, L, B = 1280, 8, 160, 77, 16
g = torch.Generator().manual_seed(0)
wq = torch.randn((C, C), generator=g) * C ** -0.5 * (ops.QK_LOG2E * DH ** -0.5) * 3
q2 = ops.prep_linear_ln(wq, None, 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g), dev)
o2 = ops.prep_linear(torch.randn((C, C), generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.2, dev)
q2t = q2.w.t().contiguous()
k = torch.randn((B * L, C), generator=g).half().to(dev); v = torch.randn((B * L, C), generator=g).half().to(dev)
vt = torch.zeros((B, C, 80), dtype=torch.float16, device=dev); vt[:, :, :L] = v.view(B, L, C).transpose(1, 2)
kf, vf = ops.xattn_fold(k, v, q2t, o2.w, B, L, H)
fold = ops.XFold(kf, vf, ops.xattn_fold_rows(kf, k, q2.bias, L, H), L)


def timed(fn, n=50):
    for _ in range(5): fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


for HW in (256, 64):
    M = B * HW
    x = (torch.randn((M, C), generator=g) * 1.3 + 0.5).half().to(dev)
    xs = x.float().view(M, 8, 160)
    parts = torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).contiguous()
    st = torch.empty((8, M, 2), dtype=torch.float32, device=dev)
    q = ops.gemm(x, q2, ln_stats=parts); o = ops.attention(q, k, vt, B, H, HW, L, DH, q_prescaled=True)
    p = ops.xattn_fold_probs(x, fold, parts, B, HW, L)
    arms = {'q projection (LN fold)': lambda: ops.gemm(x, q2, ln_stats=parts),
            'fd_attention_f16': lambda: ops.attention(q, k, vt, B, H, HW, L, DH, q_prescaled=True),
            'out projection (+res, stats)': lambda: ops.gemm(o, o2, residual=x, ln_stats_out=st),
            'launch 1 tile 24': lambda: ops.xattn_fold_probs(x, fold, parts, B, HW, L, tile=24),
            'launch 2': lambda: ops.xattn_fold_out(p, fold, o2.bias, x, B, HW, ln_stats_out=st)}
    if HW % 128 == 0:
        arms['launch 1 tile 25'] = lambda: ops.xattn_fold_probs(x, fold, parts, B, HW, L, tile=25)

        def forced(t):
            def fn():
                ops.FORCE_TILE = t
                try:
                    ops.xattn_fold_out(p, fold, o2.bias, x, B, HW, ln_stats_out=st)
                finally:
                    ops.FORCE_TILE = 0
            return fn
        arms['launch 2 tile 20'] = forced(20)
        arms['launch 2 tile 13'] = forced(13)
    res = {a: [] for a in arms}
    for r in range(5):
        for a, fn in arms.items():
            res[a].append(timed(fn))
    print(f'--- {HW} rows per sample x {B} samples (M = {M}), default launch 1 tile {ops.xattn_fold_plan(B, HW, C, H, L, parts=8)}')
    med = {}
    for a in arms:
        vs = sorted(res[a]); med[a] = vs[2]
        print(f'{a:32s} median {vs[2]:7.2f} us   rounds {" ".join(f"{t:.2f}" for t in res[a])}')
    old = med['q projection (LN fold)'] + med['fd_attention_f16'] + med['out projection (+res, stats)']
    new = min(med[a] for a in med if a.startswith('launch 1')) + min(med[a] for a in med if a.startswith('launch 2'))
    print(f'three launches {old:.2f} us, two folded launches {new:.2f} us')
