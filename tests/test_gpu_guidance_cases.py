'''csrc/guidance.hip through the C ABI on every order, shape and edge: the case table of tests/guidance_cases.py (N over the row
tiles, the `used` bits and the LDS budget, L from 2 to 96, D from one MFMA k-iteration to 1024, one guide per prompt, ties, zero
tails, denormals) against a float64 reference of the table and the pinned oracle on the device's own table, for all six
(order, reuse) pairs; the tween against the oracle bit for bit at every L; per-prompt status in a batch; the concept override and
the header pull against plain loops; what the entry points refuse; and a recorded fd_guidance_tween replayed after the caller's
parameter struct is gone.  Needs an MI355X.'''
import ctypes
import gc

import numpy as np
import pytest
import torch

import guidance_cases as GC
from oracle import guidance_ref as G

pytestmark = pytest.mark.gpu

IDS = [c.id for c in GC.CASES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def _check_assignment(case, r, order, reuse, what):
    '''idx equals the oracle's on the device's own table; s holds the bits of the table entries the oracle picked.'''
    for b in range(case.B):
        want = G.assign(r.ws[b][:, 1:].astype(np.float64), case.L, reuse, order)
        assert np.array_equal(r.idx[b], want[:, 0].astype(np.int32)), (what, b, r.idx[b], want[:, 0])
        assert np.array_equal(GC.bits(r.s[b]), GC.bits(want[:, 1].astype(np.float32))), (what, b)


def _same_bits(a, b, names):
    return all(np.array_equal(GC.bits(getattr(a, n)), GC.bits(getattr(b, n))) for n in names)


def _check_planted(case, ws):
    '''The intended ties, zeros and denormals exist in the device table (a case whose content does not materialise is broken).'''
    t = ws[0]
    if case.kind in ('ties_rows', 'ties_both'):
        for keep, copy in GC.DUP_ROWS:
            assert np.array_equal(GC.bits(t[keep]), GC.bits(t[copy])), f'rows {keep} and {copy} are not bit-equal in the device table'
            j = int(np.argmax(t[keep][1:])) + 1
            assert t[keep, j] == t[:, j].max(), f'duplicated row {keep} does not hold the best entry of column {j}'
    for keep, copy in GC.dup_cols(case):
        assert np.array_equal(GC.bits(t[:, keep]), GC.bits(t[:, copy])), f'columns {keep} and {copy} are not bit-equal'
    if case.kind in ('zeros', 'denormal'):
        dead = [j for j in range(case.L) if j not in GC.ZERO_LIVE and not (case.kind == 'denormal' and j == GC.DENORMAL_ROW)]
        assert (t[:, dead] == 0).all() and (t[:, list(GC.ZERO_LIVE)] > 0).all()
    if case.kind == 'denormal':
        col = t[:, GC.DENORMAL_ROW]
        assert (col < GC.FLT_MIN).all(), 'the denormal column holds a normal number'
        print(f'denormal column on the device: {int((col > 0).sum())} of {col.size} entries kept, the rest flushed to 0')


@pytest.mark.parametrize('case', GC.CASES, ids=IDS)
def test_guidance_map_case(dev, case):
    '''fd_guidance_map, two launches per (order, reuse) pair: the table within T = 4 E of float64 on every entry (header column
    included), idx / s exactly the oracle's on the device's table, guards intact, identical bits from the second launch, and each
    prompt of a batch bit-equal to that prompt run alone with its own guide.'''
    T = GC.tolerance()
    want = GC.sim64(case)
    for order, reuse in GC.PAIRS:
        what = f'{case.id} order={order} reuse={int(reuse)}'
        r = GC.run_map(case, dev, order, reuse)
        again = GC.run_map(case, dev, order, reuse)
        err = float(np.abs(r.ws.astype(np.float64) - want).max())
        print(f'{what}: |ws - sim64| = {err:.3e} = {err / T:.3f} T')
        assert r.guards and again.guards, what + ': wrote outside ws / idx / s'
        assert err <= T, (what, err, T)
        _check_planted(case, r.ws)
        _check_assignment(case, r, order, reuse, what)
        assert _same_bits(r, again, ('ws', 'idx', 's')), what + ': two identical launches differ'
        if case.B > 1:
            for b in range(case.B):
                one, alt, txt = GC.single(case, b)
                alone = GC.run_map(one, dev, order, reuse, alt, txt)
                assert alone.guards
                for n in ('ws', 'idx', 's'):
                    assert np.array_equal(GC.bits(getattr(r, n)[b]), GC.bits(getattr(alone, n)[0])), (what, b, n)


def _check_tween(case, r, vals, alt, txt, what):
    '''weights and out bit-equal to the oracle fed the device's (idx, s); a prompt on which the oracle divides by zero (adjacent
    equal peaks) reports status 1 and keeps its base.'''
    fl, mu, l0, l1, cl, mg, hm, order, reuse = vals
    for b in range(case.B):
        mapped = GC.mapped_of(r.idx[b], r.s[b])
        a = alt[b if case.batched else 0]
        try:
            o_out, o_w, _ = G.tween(txt[b], a, threshold=(fl, mu), linear=(l0, l1), clustered=cl, max_guidance=mg, header_max=hm,
                                    order=int(order), reuse=bool(reuse), mapped=mapped)
        except ZeroDivisionError:
            assert r.status[b] == 1, (what, b)
            assert np.array_equal(GC.bits(r.out[b]), GC.bits(txt[b])), (what, b)
            continue
        assert r.status[b] == 0, (what, b)
        assert np.array_equal(GC.bits(r.weights[b]), GC.bits(o_w.numpy())), (what, b, 'weights not bit-exact vs oracle')
        assert np.array_equal(GC.bits(r.out[b]), GC.bits(o_out[0].numpy())), (what, b, 'blend not bit-exact vs oracle')


TWEEN_OUT = ('ws', 'idx', 's', 'out', 'weights', 'status')


@pytest.mark.parametrize('case', GC.CASES, ids=IDS)
def test_guidance_tween_case(guidance_goldens, dev, case):
    '''fd_guidance_tween with lin_w = torch.linspace(l0, l1, L) on five parameter sets (four of the goldens' tween_sets and
    'neg_mult' at floor 0, see guidance_cases.tween_sets): the table within T, the assignment as in the map test, weights and out
    bit for bit against the oracle on the device's (idx, s), guards, repeatability and batch = single.'''
    T = GC.tolerance()
    want = GC.sim64(case)
    alt, txt = GC.inputs(case)
    for name, vals in GC.tween_sets(guidance_goldens).items():
        what = f'{case.id} {name}'
        r = GC.run_tween(case, dev, vals)
        again = GC.run_tween(case, dev, vals)
        assert r.guards and again.guards, what + ': wrote outside an output buffer'
        assert float(np.abs(r.ws.astype(np.float64) - want).max()) <= T, what
        _check_assignment(case, r, int(vals[7]), bool(vals[8]), what)
        _check_tween(case, r, vals, alt, txt, what)
        assert _same_bits(r, again, TWEEN_OUT), what + ': two identical launches differ'
        if case.B > 1:
            for b in range(case.B):
                one, a1, t1 = GC.single(case, b)
                alone = GC.run_tween(one, dev, vals, a1, t1)
                assert alone.guards
                for n in TWEEN_OUT:
                    assert np.array_equal(GC.bits(getattr(r, n)[b]), GC.bits(getattr(alone, n)[0])), (what, b, n)


def test_batch_status(dev):
    '''Three prompts, clustered != 0, the middle one with adjacent equal peaks (a two-wide plateau above the mean): status is
    [0, 1, 0] per prompt, the middle out is its base bit for bit, the other two equal their single-prompt runs and the oracle.'''
    from test_gpu_guidance import _realise_profile
    rng = np.random.default_rng(41)
    profiles = [rng.random(76), 0.3 * rng.random(76), rng.random(76)]
    profiles[1][10] = profiles[1][11] = 0.9
    parts = [_realise_profile(p.astype(np.float32)) for p in profiles]
    alt = parts[0][0]
    assert all(np.array_equal(a, alt) for a, _ in parts)
    txt = np.concatenate([t for _, t in parts])
    case = GC.Case(1, 77, alt.shape[-1], B=3)
    vals = (0.5, 0.0, 0.0, 0.0, 0.7, 10.0, 1.0, 1, True)      # the Tweener of test_clustered_kats_on_device, gain 0.7
    r = GC.run_tween(case, dev, vals, alt, txt)
    assert r.guards
    assert GC.bits(r.s[1, 10:11]) == GC.bits(r.s[1, 11:12]) and r.s[1, 10] > r.s[1].mean(), 'the plateau did not materialise'
    assert r.status.tolist() == [0, 1, 0]
    assert np.array_equal(GC.bits(r.out[1]), GC.bits(txt[1]))
    _check_tween(case, r, vals, alt, txt, 'batch status')
    for b in range(3):
        alone = GC.run_tween(case._replace(B=1), dev, vals, alt, txt[b:b + 1])
        assert alone.status.tolist() == [r.status[b]]
        for n in TWEEN_OUT:
            assert np.array_equal(GC.bits(getattr(r, n)[b]), GC.bits(getattr(alone, n)[0])), (b, n)
    assert not np.array_equal(GC.bits(r.out[0]), GC.bits(txt[0])), 'the good prompts must be tweened'


# --------------------------------------------------------------------------------------------------- override, header pull
@pytest.mark.parametrize('D', (32, 320, 768))
def test_concept_override_vs_loop(dev, D):
    '''fd_guidance_concept_override against a plain loop: every combination of ct_idx in (0 = skipped, 1, the largest valid value,
    3) with ct_s in (0.9f exactly, the next float above it, 0.5, 0.95).  Comparing the whole of out bit for bit covers row 0 and
    every unselected row; out sits between guards.'''
    from flexdiffuse_amd import hip
    L, N = 17, 9
    rng = np.random.default_rng(50 + D)
    guide = rng.standard_normal((N, D)).astype(np.float32)
    base = rng.standard_normal((L, D)).astype(np.float32)
    cm_idx = rng.integers(0, N, L).astype(np.int32)
    p9 = np.float32(0.9)
    idx_kinds, s_kinds = (0, 1, L, 3), (p9, np.nextafter(p9, np.float32(1)), np.float32(0.5), np.float32(0.95))
    ct_idx = np.array([idx_kinds[j % 4] for j in range(L - 1)] + [1], np.int32)
    ct_s = np.array([s_kinds[j // 4] for j in range(L - 1)] + [1.0], np.float32)
    want = base.copy()
    for j in range(L - 1):
        c = int(ct_idx[j])
        if c - 1 < 0 or not ct_s[j] > p9:
            continue
        want[j + 1] = guide[cm_idx[c - 1]]
    changed = [j + 1 for j in range(L - 1) if not np.array_equal(want[j + 1], base[j + 1])]
    assert len(changed) == 6 and 0 not in changed        # 3 indices x 2 similarities above 0.9f
    full, out = GC._guarded(torch, L * D, torch.float32, dev)
    out.copy_(torch.from_numpy(base).reshape(-1))
    t = [torch.from_numpy(x).to(dev) for x in (guide, cm_idx, ct_idx, ct_s)]
    hip.call('fd_guidance_concept_override', *(hip.ptr(x) for x in t), hip.ptr(out), N, L, D, hip.stream())
    torch.cuda.synchronize()
    assert np.array_equal(GC.bits(out.cpu().numpy().reshape(L, D)), GC.bits(want))
    assert GC._intact(torch, full, L * D)


@pytest.mark.parametrize('D', (32, 320))
@pytest.mark.parametrize('L', (2, 77))
@pytest.mark.parametrize('B', (1, 3))
def test_header_pull_vs_torch(dev, B, L, D):
    '''Only row 0 of each sample changes, to x + (hdr - x) * 0.85f in three separately rounded fp32 operations.'''
    from flexdiffuse_amd import hip
    g = torch.Generator().manual_seed(60 + B + L + D)
    x = torch.randn((B, L, D), generator=g)
    hdr = torch.randn((D,), generator=g) * 3
    want = x.clone()
    want[:, 0] = x[:, 0] + (hdr - x[:, 0]) * torch.tensor(0.85, dtype=torch.float32)
    full, out = GC._guarded(torch, B * L * D, torch.float32, dev)
    out.copy_(x.reshape(-1))
    dh = hdr.to(dev)
    hip.call('fd_guidance_header_pull', hip.ptr(out), hip.ptr(dh), B, L, D, hip.stream())
    torch.cuda.synchronize()
    assert np.array_equal(GC.bits(out.cpu().numpy().reshape(B, L, D)), GC.bits(want.numpy()))
    assert GC._intact(torch, full, B * L * D)


# --------------------------------------------------------------------------------------------------- refusals
def test_guidance_refusals(dev):
    '''Each malformed call raises ValueError from a check that precedes every launch in csrc/guidance.hip, and launches nothing:
    the sentinel-filled outputs are unchanged after a sync.  The good call straight after each refusal gives the bits of the first
    good call, which is itself checked against the oracle.  Every buffer is large enough for the largest shape attempted.'''
    from flexdiffuse_amd import hip
    case = GC.Case(33, 33, 32, seed=990)
    alt, txt = GC.inputs(case)
    vals = (0.5, 0.5, 0.0, 0.5, 0.5, 0.5, 0.15, 1, True)
    NMAX, LMAX, DMAX = 2049, 97, 64
    ta = torch.zeros(NMAX * DMAX, device=dev)
    tt = torch.zeros(LMAX * DMAX, device=dev)
    ta[:alt.size].copy_(torch.from_numpy(alt).reshape(-1))
    tt[:txt.size].copy_(torch.from_numpy(txt).reshape(-1))
    lin_w = torch.zeros(LMAX, device=dev)
    lin_w[:case.L].copy_(torch.linspace(vals[2], vals[3], steps=case.L))
    outs = {'ws': torch.empty(NMAX * LMAX, device=dev), 'out': torch.empty(LMAX * DMAX, device=dev), 'weights': torch.empty(128, device=dev),
            'idx': torch.empty(128, dtype=torch.int32, device=dev), 's': torch.empty(128, device=dev),
            'status': torch.empty(4, dtype=torch.int32, device=dev)}
    p = GC.params_of(vals)

    def fill():
        for t in outs.values():
            t.fill_(GC.SENTINEL_I if t.dtype == torch.int32 else GC.SENTINEL_F)

    def untouched():
        return all(bool((t == (GC.SENTINEL_I if t.dtype == torch.int32 else GC.SENTINEL_F)).all()) for t in outs.values())

    map_args = dict(alt=hip.ptr(ta), txt=hip.ptr(tt), ws=hip.ptr(outs['ws']), idx=hip.ptr(outs['idx']), s=hip.ptr(outs['s']), B=1,
                    alt_batched=0, N=case.N, L=case.L, D=case.D, order=1, reuse=1)
    tween_args = dict(base=hip.ptr(tt), alt=hip.ptr(ta), lin_w=hip.ptr(lin_w), ws=hip.ptr(outs['ws']), out=hip.ptr(outs['out']),
                      weights=hip.ptr(outs['weights']), idx=hip.ptr(outs['idx']), s=hip.ptr(outs['s']), status=hip.ptr(outs['status']),
                      B=1, alt_batched=0, N=case.N, L=case.L, D=case.D, p=ctypes.byref(p))

    def launch(name, args, **kw):
        fill()
        try:
            hip.call(name, *dict(args, **kw).values(), hip.stream())
        finally:
            torch.cuda.synchronize()
        return {k: t.cpu().numpy().copy() for k, t in outs.items()}

    def same(a, b):
        return all(np.array_equal(GC.bits(a[k]), GC.bits(b[k])) for k in a)

    good_map = launch('fd_guidance_map', map_args)
    good_tween = launch('fd_guidance_tween', tween_args)
    n = case.N * case.L
    ws = good_map['ws'][:n].reshape(case.N, case.L)
    assert float(np.abs(ws - GC.sim64(case)[0]).max()) <= GC.tolerance()
    assert np.array_equal(good_map['idx'][:case.L], G.assign(ws[:, 1:].astype(np.float64), case.L, True, 1)[:, 0].astype(np.int32))
    assert (good_map['ws'][n:] == GC.SENTINEL_F).all() and (good_tween['out'][case.L * case.D:] == GC.SENTINEL_F).all()
    assert np.array_equal(GC.bits(good_tween['ws']), GC.bits(good_map['ws'])) and good_tween['status'][0] == 0

    shapes = [dict(D=48), dict(L=1), dict(L=97), dict(N=0), dict(N=2049, L=16), dict(N=GC.max_rows(77) + 1, L=77),
              dict(N=GC.max_rows(96) + 1, L=96)]
    null = ctypes.c_void_p(0)
    bad_map = shapes + [dict(order=3), dict(order=-1)] + [{k: null} for k in ('alt', 'txt', 'ws', 'idx', 's')]
    for kw in bad_map:
        with pytest.raises(ValueError):
            launch('fd_guidance_map', map_args, **kw)
        assert untouched(), ('fd_guidance_map', kw, 'a refused call wrote to an output')
        assert same(launch('fd_guidance_map', map_args), good_map), kw

    def with_order(order):
        q = GC.params_of(vals)
        q.order = order
        return dict(p=ctypes.byref(q), _keep=q)

    bad_tween = shapes + [with_order(3), with_order(-1)] + [{k: null} for k in ('base', 'lin_w', 'status')] + [dict(p=None)]
    for kw in bad_tween:
        keep = kw.pop('_keep', None)
        with pytest.raises(ValueError):
            launch('fd_guidance_tween', tween_args, **kw)
        assert untouched(), ('fd_guidance_tween', kw, 'a refused call wrote to an output')
        assert same(launch('fd_guidance_tween', tween_args), good_tween), kw
        del keep

    # override with L = 1 and header pull with B = 0: nothing is written either
    gi = torch.zeros(64, dtype=torch.int32, device=dev)
    fill()
    with pytest.raises(ValueError):
        hip.call('fd_guidance_concept_override', hip.ptr(ta), hip.ptr(gi), hip.ptr(gi), hip.ptr(lin_w), hip.ptr(outs['out']), 9, 1, 32,
                 hip.stream())
    with pytest.raises(ValueError):
        hip.call('fd_guidance_header_pull', hip.ptr(outs['out']), hip.ptr(lin_w), 0, 2, 32, hip.stream())
    torch.cuda.synchronize()
    assert untouched()
    assert same(launch('fd_guidance_tween', tween_args), good_tween)


# --------------------------------------------------------------------------------------------------- launch plan
def test_tween_in_a_launch_plan(guidance_goldens, dev):
    '''A recorded fd_guidance_tween holds its own copy of the parameters: after the caller's struct is deleted and same-sized structs
    with other values are written, a replay on new contents of the same base / alt buffers equals a fresh eager call with the
    original parameters, bit for bit.'''
    from flexdiffuse_amd import hip
    case = GC.Case(9, 33, 32, B=2, seed=995)
    vals = GC.tween_sets(guidance_goldens)['defaults']
    other = GC.tween_sets(guidance_goldens)['neg_all']
    alt0, txt0 = GC.inputs(case)
    alt1, txt1 = GC.inputs(case._replace(seed=996))
    B, N, L, D = case.B, case.N, case.L, case.D
    ta, tt = torch.from_numpy(alt0.copy()).to(dev), torch.from_numpy(txt0.copy()).to(dev)
    lin_w = torch.linspace(vals[2], vals[3], steps=L).to(dev)
    sizes = {'ws': (B * N * L, torch.float32), 'out': (B * L * D, torch.float32), 'weights': (B * L, torch.float32),
             'idx': (B * L, torch.int32), 's': (B * L, torch.float32), 'status': (B, torch.int32)}
    bufs = {k: GC._guarded(torch, n, dt, dev) for k, (n, dt) in sizes.items()}

    def refill():
        for full, _ in bufs.values():
            full.fill_(GC.SENTINEL_I if full.dtype == torch.int32 else GC.SENTINEL_F)

    def read():
        torch.cuda.synchronize()
        assert all(GC._intact(torch, full, view.numel()) for full, view in bufs.values())
        return {k: v[1].cpu().numpy().copy() for k, v in bufs.items()}

    p = GC.params_of(vals)
    plan = hip.Plan()
    with plan.record():
        hip.call('fd_guidance_tween', hip.ptr(tt), hip.ptr(ta), hip.ptr(lin_w), *(hip.ptr(bufs[k][1]) for k in
                 ('ws', 'out', 'weights', 'idx', 's', 'status')), B, 0, N, L, D, ctypes.byref(p), hip.stream())
    assert len(plan) == 1
    first = read()
    del p
    gc.collect()
    clutter = [GC.params_of(other) for _ in range(64)]       # same-sized structs with other values, wherever the old one lay
    ta.copy_(torch.from_numpy(alt1.copy()))
    tt.copy_(torch.from_numpy(txt1.copy()))
    refill()
    plan.replay()
    replayed = read()
    fresh = GC.run_tween(case, dev, vals, alt1, txt1)
    assert fresh.guards
    for k in TWEEN_OUT:
        assert np.array_equal(GC.bits(replayed[k]), GC.bits(getattr(fresh, k).reshape(-1))), k
    assert not np.array_equal(GC.bits(replayed['out']), GC.bits(first['out']))
    wrong = GC.run_tween(case, dev, other, alt1, txt1)
    assert not np.array_equal(GC.bits(wrong.weights), GC.bits(fresh.weights)), 'the other parameters must give another result'
    del clutter
