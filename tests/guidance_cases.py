'''One table of fd_guidance_map / fd_guidance_tween cases (csrc/guidance.hip: `k_guidance_sim`, `k_guidance_tween`), seeded fp32
input builders, a float64 reference of the full similarity table, restatements of wrong computations, and device runners whose every
output buffer sits between sentinel guards -- shared by tests/test_guidance_cases.py (CPU: the table reaches what it promises, the
inputs hold what they promise, and the criterion rejects eleven wrong computations) and tests/test_gpu_guidance_cases.py (MI355X:
every case, every (order, reuse) pair, through the C ABI).

Nothing here needs a GPU to import; `run_map` and `run_tween` are the only parts that touch one.

Inputs of a "general" case, per prompt: three quarters of the text rows are small perturbations of one direction u (the cluster),
the rest (columns 1, 5, 9, ...: the outliers) are orthogonal to u.  Guide rows rotate over four kinds: u plus noise (a SPREAD row:
near-equal logits over the whole cluster, so every softmax entry is small and a wrong logit or a wrong denominator moves them all),
a noisy copy of an outlier (a SHARP row: one entry above 0.99), -u plus noise (logits of a few units around zero: the row on which
padding columns at logit 0 would show), and plain Gaussian rows.  Guide-row norms run over 1e-3 .. 1e3, text-row norms over 0.1 .. 10.

The other kinds plant what their names say: bit-identical guide rows in different 32-row tiles / 64-lane groups / sides of row 256
and "hub" rows at 100 and 290 that are the best candidate of two columns each (a `used` mask that forgets them hands them out
twice); bit-identical text rows; columns whose similarities underflow to exactly 0 (the construction of
test_gpu_guidance.py::test_underflow_edge_cases at N = 100 and 300); and one column whose best similarity is a denormal.'''
from __future__ import annotations

import functools
import itertools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import numpy as np

ORDERS = (0, 1, 2)                                  # text, alignment, direct (oracle.guidance_ref.ORDER_*)
PAIRS = tuple(itertools.product(ORDERS, (True, False)))   # the six (order, reuse) pairs
SIM_COLS = 96                                       # columns of the logits tile (SIM_CT * 32)
TWEEN_SHARED_BYTES = 3120                           # sizeof(TweenShared): 7 x 96 + 98 words, 4 x 8 B, 1 word, padded to 8 B
LDS_BUDGET = 150 * 1024                             # check_shapes
FLT_MIN = float(np.finfo(np.float32).tiny)          # smallest normal fp32
GUARD = 64                                          # guard elements on each side of an output buffer (256 B: float4 alignment kept)
SENTINEL_F = -7777.0
SENTINEL_I = -7777

DUP_ROWS = ((3, 40), (5, 70), (10, 300))            # (kept, copy): another 32-row tile; another 64-lane group; across row 256
HUB_ROWS = (100, 290)                               # best candidate of two reserved outlier columns each
ZERO_LIVE = (3, 20)                                 # text rows of a 'zeros' case that keep non-zero similarities
DENORMAL_ROW = 30                                   # text row of the 'denormal' case whose column holds denormals only


def lds_bytes(N: int, L: int) -> int:
    '''check_shapes: the tween kernel's dynamic LDS.'''
    return ((TWEEN_SHARED_BYTES + 15) & ~15) + N * (L | 1) * 4


def max_rows(L: int) -> int:
    '''The largest N that check_shapes admits at this L.'''
    return min(2048, (LDS_BUDGET - ((TWEEN_SHARED_BYTES + 15) & ~15)) // ((L | 1) * 4))


class Case(NamedTuple):
    N: int                    # guide tokens
    L: int                    # text tokens (header included)
    D: int                    # channels
    B: int = 1                # prompts
    batched: bool = False     # one guide per prompt (alt_batched = 1)
    kind: str = 'general'     # general | ties_rows | ties_cols | ties_both | zeros | denormal
    seed: int = 0

    @property
    def id(self) -> str:
        b = '' if self.B == 1 else f'-B{self.B}' + ('own' if self.batched else 'shared')
        return f'{self.kind}-N{self.N}-L{self.L}-D{self.D}{b}'

    @property
    def NC(self) -> int:
        return self.L - 1

    @property
    def Ba(self) -> int:
        return self.B if self.batched else 1


_TABLE = (
    # ---- N over the row tiles and bitmasks, L on both sides of 32 and 64, every D with a row-tail N and both sides of L = 64 --------
    Case(1, 33, 32), Case(5, 77, 64), Case(31, 64, 96), Case(32, 32, 32), Case(33, 65, 64), Case(64, 2, 32), Case(65, 96, 96),
    Case(256, 33, 64), Case(257, 77, 768), Case(33, 32, 768), Case(33, 96, 1024), Case(5, 33, 1024), Case(31, 65, 32),
    Case(40, 77, 96),
    # ---- RM = 8 and bit 31 of `used`; the largest N of the LDS budget at L = 77 and at L = 96 ----------------------------------------
    Case(2048, 16, 32), Case(max_rows(77), 77, 32), Case(max_rows(96), 96, 32),
    # ---- three prompts: one guide for all, and one guide each ------------------------------------------------------------------
    Case(33, 33, 32, B=3), Case(33, 65, 64, B=3, batched=True),
    # ---- ties, zero tails, denormals -------------------------------------------------------------------------------------------
    Case(321, 33, 32, kind='ties_rows'), Case(40, 77, 64, kind='ties_cols'), Case(321, 65, 32, kind='ties_both'),
    Case(100, 77, 64, kind='zeros'), Case(300, 77, 64, kind='zeros'), Case(40, 77, 64, kind='denormal'),
)
CASES = tuple(c._replace(seed=700 + i) for i, c in enumerate(_TABLE))
assert len({c.id for c in CASES}) == len(CASES), 'case ids must be unique'

REQUIRED_PATHS = frozenset(
    ['rows:one_tile', 'rows:full_tiles', 'rows:tail_tile', 'rm:1', 'rm:2', 'rm:8', 'used:bit0_only', 'used:bits0-4', 'used:bit31',
     'slot2:empty', 'slot2:1', 'slot2:13', 'slot2:32', 'stride:L', 'stride:L+1', 'lock:nc1', 'lock:word0', 'lock:word1', 'lock:word2',
     'lock:word2_hi', 'k:one_iter', 'k:quarter_not_pow2', 'k:long', 'norm:8_lanes', 'norm:all_lanes', 'guide:shared', 'guide:own',
     'walk:short_of_rows', 'direct:n_lt_nc', 'direct:n_gt_nc', 'ties:rows_tiles', 'ties:rows_lane_groups', 'ties:rows_across_256',
     'ties:cols', 'zero_tail:two_used_bits', 'zero_tail:two_m_slots', 'denormal', 'lds:limit_L77', 'lds:limit_L96'])


def paths(case: Case) -> set:
    '''The kernel paths this case reaches, derived from the case alone.'''
    N, L, D, NC = case.N, case.L, case.D, case.NC
    p = {'rows:one_tile' if N <= 32 else ('rows:tail_tile' if N % 32 else 'rows:full_tiles'),
         f'rm:{(N + 255) >> 8}',
         'used:bit31' if (N - 1) >> 6 == 31 else ('used:bit0_only' if N <= 64 else f'used:bits0-{(N - 1) >> 6}'),
         'slot2:empty' if L <= 64 else f'slot2:{L - 64}',
         'stride:L' if L & 1 else 'stride:L+1',
         'lock:nc1' if NC == 1 else f'lock:word{(NC - 1) >> 5}',
         'k:one_iter' if D == 32 else 'k:long',
         'norm:all_lanes' if D >= 256 else f'norm:{D // 4}_lanes',
         'guide:own' if case.batched else 'guide:shared',
         'direct:n_lt_nc' if N < NC else 'direct:n_gt_nc' if N > NC else 'direct:n_eq_nc'}
    if NC > 80:
        p.add('lock:word2_hi')
    if (D // 4) & (D // 4 - 1):
        p.add('k:quarter_not_pow2')
    if N < NC:
        p.add('walk:short_of_rows')
    if case.kind in ('ties_rows', 'ties_both'):
        p |= {'ties:rows_tiles', 'ties:rows_lane_groups', 'ties:rows_across_256'}
    if case.kind in ('ties_cols', 'ties_both'):
        p.add('ties:cols')
    if case.kind == 'zeros':
        p.add('zero_tail:two_used_bits' if 64 < N <= 128 else 'zero_tail:two_m_slots' if N > 256 else 'zero_tail:one_wave')
    if case.kind == 'denormal':
        p.add('denormal')
    if case.N == max_rows(L) and L in (77, 96):
        p.add(f'lds:limit_L{L}')
    return p


# --------------------------------------------------------------------------------------------------- inputs
def outlier_rows(L: int):
    '''Text rows orthogonal to the cluster direction.'''
    return [j for j in range(L) if j % 4 == 1]


def reserved_outliers(case: Case) -> int:
    '''Outlier columns kept free of ordinary sharp rows: three for the duplicated guide rows, two for each hub row.'''
    return 3 + 2 * len(HUB_ROWS) if case.kind in ('ties_rows', 'ties_both') else 0


def dup_cols(case: Case):
    '''(kept, copy) text rows made bit-identical: a pair of outliers, and a pair of adjacent cluster rows.'''
    return ((5, 9), (2, 3)) if case.kind == 'ties_cols' else ((33, 41), (2, 3)) if case.kind == 'ties_both' else ()


def _unit(v):
    return v / np.linalg.norm(v)


def _general_prompt(case: Case, rng, u, want_guide: bool):
    '''(txt [L][D], alt [N][D] or None) of one prompt, float64 before rounding.'''
    N, L, D = case.N, case.L, case.D
    out = outlier_rows(L)
    txt = np.empty((L, D))
    for j in range(L):
        g = rng.standard_normal(D)
        txt[j] = (g - (g @ u) * u) * D ** -0.5 if j in out else u + 0.05 * g * D ** -0.5
    for keep, copy in dup_cols(case):
        txt[copy] = txt[keep]
    tscale = 10.0 ** rng.permutation(np.linspace(-1, 1, L))
    for keep, copy in dup_cols(case):
        tscale[copy] = tscale[keep]
    txt_scaled = txt * tscale[:, None]
    if not want_guide:
        return txt_scaled, None
    free = out[reserved_outliers(case):]
    alt = np.empty((N, D))
    for i in range(N):
        h = rng.standard_normal(D) * D ** -0.5
        kind = i % 4 if N > 1 else 0
        if kind == 0:
            alt[i] = u + 0.3 * h
        elif kind == 1:
            alt[i] = _unit(txt[free[(i // 4) % len(free)]]) + 0.02 * h
        elif kind == 2:
            alt[i] = -u + 0.1 * h
        else:
            alt[i] = h
    if N >= 3:
        alt[N // 2 - (N // 2) % 4 + 3 if N >= 8 else N - 1] = sum(_unit(t) for t in txt)     # the bisector of the text rows
    if reserved_outliers(case):
        res = out[:reserved_outliers(case)]
        for k, (keep, _) in enumerate(DUP_ROWS):
            alt[keep] = _unit(txt[res[k]])
        for k, hub in enumerate(HUB_ROWS):
            alt[hub] = _unit(txt[res[3 + 2 * k]]) + _unit(txt[res[4 + 2 * k]])
    ascale = 10.0 ** rng.permutation(np.linspace(-3.3, 3.3, N)) if N > 1 else np.ones(1)
    alt = alt * ascale[:, None]
    if reserved_outliers(case):
        for keep, copy in DUP_ROWS:
            alt[copy] = alt[keep]
    return txt_scaled, alt


def _zeros_prompt(case: Case, rng):
    '''test_gpu_guidance.py::test_underflow_edge_cases at the case's N: every guide row is (nearly) text row 3, every text row but 3
    and 20 points the opposite way, so that their similarities underflow to exactly 0.  kind 'denormal': text row 30 stands at
    cos = 0.05 to the guide rows instead, a logit gap of about 95.'''
    N, L, D = case.N, case.L, case.D
    f32 = np.float32
    alt = rng.standard_normal((N, D)).astype(f32)
    txt = rng.standard_normal((L, D)).astype(f32)
    for j in range(L):
        if j not in ZERO_LIVE:
            txt[j] = -txt[3] * f32(1 + 0.01 * j) + f32(1e-3) * rng.standard_normal(D).astype(f32)
    txt[20] = txt[3] + f32(0.3) * rng.standard_normal(D).astype(f32)
    for i in range(N):
        alt[i] = txt[3] * f32(1.0 + 0.01 * i) + f32(0.05) * rng.standard_normal(D).astype(f32)
    if case.kind == 'denormal':
        v = _unit(txt[3].astype(np.float64))
        w = rng.standard_normal(D)
        w = _unit(w - (w @ v) * v)
        txt[DENORMAL_ROW] = (3.0 * (0.05 * v + (1 - 0.05 ** 2) ** 0.5 * w)).astype(f32)
    return txt, alt


@functools.lru_cache(None)
def inputs(case: Case):
    '''(alt [Ba][N][D], txt [B][L][D]) fp32, exactly what the device is handed.  Cached and shared: callers leave them unchanged.'''
    rng = np.random.default_rng(case.seed)
    if case.kind in ('zeros', 'denormal'):
        assert case.B == 1
        txt, alt = _zeros_prompt(case, rng)
        alt, txt = alt[None], txt[None]
    else:
        u0 = _unit(rng.standard_normal(case.D))
        alts, txts = [], []
        for b in range(case.B):
            u = u0 if not case.batched else _unit(rng.standard_normal(case.D))
            t, a = _general_prompt(case, rng, u, want_guide=(b == 0 or case.batched))
            txts.append(t)
            if a is not None:
                alts.append(a)
        alt, txt = np.stack(alts).astype(np.float32), np.stack(txts).astype(np.float32)
    alt, txt = np.ascontiguousarray(alt), np.ascontiguousarray(txt)
    assert alt.shape == (case.Ba, case.N, case.D) and txt.shape == (case.B, case.L, case.D)
    return alt, txt


def single(case: Case, b: int):
    '''(case, alt, txt) of prompt b run alone with its own guide.'''
    alt, txt = inputs(case)
    return case._replace(B=1, batched=False), alt[b if case.batched else 0][None], txt[b][None]


# --------------------------------------------------------------------------------------------------- float64 reference, table defects
TABLE_DEFECTS = ('pad_leak', 'drop_k_slice', 'norm_short', 'guide0_for_all')


def sim64_of(alt, txt, defect: Optional[str] = None) -> np.ndarray:
    '''[B][N][L] float64: softmax_j(100 cos(alt_i, txt_j)) from the fp32 inputs, header column included.  `defect` restates one
    wrong computation: the padded columns L..95 join the denominator at logit 0; the last quarter of D is left out of the dot
    products; the norms leave out the last 4 floats; every prompt uses guide 0.'''
    assert defect is None or defect in TABLE_DEFECTS
    a, t = np.asarray(alt, np.float64), np.asarray(txt, np.float64)
    B, L, D = t.shape
    if a.shape[0] == 1 or defect == 'guide0_for_all':
        a = np.broadcast_to(a[:1], (B,) + a.shape[1:])
    nd = D - 4 if defect == 'norm_short' else D
    an = np.sqrt((a[..., :nd] ** 2).sum(-1, keepdims=True))
    tn = np.sqrt((t[..., :nd] ** 2).sum(-1, keepdims=True))
    kd = D - D // 4 if defect == 'drop_k_slice' else D
    x = 100.0 * np.einsum('bik,bjk->bij', (a / an)[..., :kd], (t / tn)[..., :kd])
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    den = e.sum(-1, keepdims=True)
    if defect == 'pad_leak':
        den = den + (SIM_COLS - L) * np.exp(-m)
    return e / den


@functools.lru_cache(None)
def sim64(case: Case) -> np.ndarray:
    r = sim64_of(*inputs(case))
    r.setflags(write=False)
    return r


@functools.lru_cache(None)
def oracle_error() -> float:
    '''E: the largest |oracle.guidance_ref.similarity - sim64[:, 1:]| over the whole case table -- what the pinned fp32 oracle itself
    is off by against float64 on these inputs.'''
    from oracle import guidance_ref as G
    worst = 0.0
    for case in CASES:
        alt, txt = inputs(case)
        want = sim64(case)
        for b in range(case.B):
            got = G.similarity(alt[b if case.batched else 0], txt[b])
            worst = max(worst, float(np.abs(got - want[b][:, 1:]).max()))
    return worst


def tolerance() -> float:
    '''T = 4 E: the bound on |device table - sim64|.  The device adds the same D fp32 products in another order than the oracle's
    mat-vec (four K slices of an MFMA chain, combined in fixed order); it is never derived from device output.'''
    return 4.0 * oracle_error()


# --------------------------------------------------------------------------------------------------- assignment defects
ASSIGN_DEFECTS = ('tie_high_row', 'tie_high_col', 'used_forgets_64', 'used_forgets_256', 'zero_col_keeps_0', 'zero_tail_lowest',
                  'denormal_no_lock')


def assign_with(sim: np.ndarray, n_text: int, reuse: bool, order: int, defect: Optional[str] = None) -> np.ndarray:
    '''oracle.guidance_ref.assign restated with one switchable defect (None: the same result as the oracle, which the CPU test
    asserts): ties go to the highest row; ties go to the highest column in alignment order; the `used` mask forgets rows >= 64 /
    >= 256; a column of zeros keeps index 0 under reuse; the zero tail ends on the lowest unused row; a denormal does not lock.'''
    assert defect is None or defect in ASSIGN_DEFECTS
    n_alt, n_col = sim.shape
    out = np.zeros((n_text, 2), dtype=np.float64)
    if order == 2:
        for j in range(min(n_alt, n_col)):
            out[j] = (j, sim[j, j])
        return out
    ii, jj = np.meshgrid(np.arange(n_alt), np.arange(n_col), indexing='ij')
    ii, jj, ss = ii.ravel(), jj.ravel(), sim.ravel()
    ri = -ii if defect == 'tie_high_row' else ii
    if order == 0:
        perm = np.lexsort((ri, -ss, jj))
    else:
        perm = np.lexsort((ri, -jj if defect == 'tie_high_col' else jj, -ss))
    forget = {'used_forgets_64': 64, 'used_forgets_256': 256}.get(defect, n_alt)
    floor = FLT_MIN if defect == 'denormal_no_lock' else 0.0
    used = np.zeros(n_alt, dtype=bool)
    zero_seen = np.zeros(n_col, dtype=bool)
    for k in perm:
        i, j = ii[k], jj[k]
        if (out[j, 1] > 0 and out[j, 1] >= floor) or used[i]:
            continue
        if ss[k] == 0 and zero_seen[j] and ((reuse and defect == 'zero_col_keeps_0') or (not reuse and defect == 'zero_tail_lowest')):
            used[i] = not reuse
            continue
        zero_seen[j] |= ss[k] == 0
        out[j] = (i, ss[k])
        if not reuse and i < forget:
            used[i] = True
    return out


# --------------------------------------------------------------------------------------------------- tween parameter sets
TWEEN_SET_NAMES = ('defaults', 'neg_all', 'hdr_full', 'clust_only')
ADD_SET = 'neg_mult@floor0'     # the golden set 'neg_mult' with threshold_floor = 0: the only way to blend_weights' a + b branch


def tween_sets(goldens) -> dict:
    '''name -> (floor, mult, lin0, lin1, clustered, max_guidance, header_max, order, reuse) read from the goldens' tween_sets/*.
    The last row of a mapping is never written (s = 0), so with a positive floor the threshold stage always holds a zero and
    blend_weights never reaches its a + b branch from a kernel-made mapping; ADD_SET takes 'neg_mult' and sets its floor to 0, so
    that every entry of the threshold vector is the negative multiplier.'''
    names = [str(n) for n in goldens['tween_sets/names']]
    table = {n: tuple(float(v) for v in vals) for n, vals in zip(names, goldens['tween_sets/values'])}
    sets = {n: table[n] for n in TWEEN_SET_NAMES}
    sets[ADD_SET] = (0.0,) + table['neg_mult'][1:]
    return sets


def tween_trace(mapped: np.ndarray, vals, L: int) -> set:
    '''Which stages, blend_weights branches and blend modes the oracle takes for this mapping and parameter set.'''
    from oracle import guidance_ref as G
    fl, mu, l0, l1, cl, mg, hm = vals[:7]
    seen = set()
    real = G.blend_weights

    def spy(a, b):
        seen.add('blend:max' if a.max() >= 0 and b.max() >= 0 else 'blend:add' if a.max() >= 0 else 'blend:min')
        return real(a, b)

    G.blend_weights = spy
    try:
        w = G.tween_weights(mapped, (fl, mu), (l0, l1), cl, hm)
    except ZeroDivisionError:
        return {'plateau'}
    finally:
        G.blend_weights = real
    if mu != 0:
        seen.add('stage:threshold')
    if hm < 1.0 and abs(G.tween_weights(mapped, (fl, mu), (l0, l1), cl, 1.0)[0].item()) > hm:
        seen.add('stage:header_cap')    # the uncapped header weight lies beyond the cap
    for j in range(L):
        iw = min(w[j].item(), mg)
        seen.add('mode:keep' if iw == 0 else 'mode:guide' if abs(iw) >= 1.0 - mapped[j, 1] else 'mode:lerp')
    return seen


REQUIRED_TWEEN = frozenset(['blend:max', 'blend:add', 'blend:min', 'stage:threshold', 'stage:header_cap', 'mode:keep', 'mode:guide',
                            'mode:lerp'])


# --------------------------------------------------------------------------------------------------- device runs
def _guarded(torch, n: int, dtype, dev):
    fill = SENTINEL_I if dtype == torch.int32 else SENTINEL_F
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _intact(torch, buf, n: int) -> bool:
    fill = SENTINEL_I if buf.dtype == torch.int32 else SENTINEL_F
    host = buf.cpu()
    return bool((host[:GUARD] == fill).all()) and bool((host[GUARD + n:] == fill).all())


def params_of(vals):
    from flexdiffuse_amd import hip
    fl, mu, l0, l1, cl, mg, hm, order, reuse = vals
    return hip.fd_tween_params(float(fl), float(mu), float(cl), float(mg), float(hm), int(order), int(bool(reuse)))


def run_map(case: Case, dev, order: int, reuse: bool, alt=None, txt=None) -> SimpleNamespace:
    '''fd_guidance_map through hip.call on guarded, sentinel-filled ws / idx / s: ws [B][N][L] fp32, idx [B][L] int32, s [B][L]
    fp32 on the host, and guards = True when every guard element still holds the sentinel.'''
    import torch
    from flexdiffuse_amd import hip
    if alt is None:
        alt, txt = inputs(case)
    B, N, L, D = case.B, case.N, case.L, case.D
    ta, tt = torch.from_numpy(np.array(alt)).to(dev), torch.from_numpy(np.array(txt)).to(dev)
    bufs = {'ws': _guarded(torch, B * N * L, torch.float32, dev), 'idx': _guarded(torch, B * L, torch.int32, dev),
            's': _guarded(torch, B * L, torch.float32, dev)}
    hip.call('fd_guidance_map', hip.ptr(ta), hip.ptr(tt), hip.ptr(bufs['ws'][1]), hip.ptr(bufs['idx'][1]), hip.ptr(bufs['s'][1]),
             B, int(case.batched), N, L, D, int(order), int(bool(reuse)), hip.stream())
    torch.cuda.synchronize()
    return SimpleNamespace(ws=bufs['ws'][1].cpu().numpy().reshape(B, N, L), idx=bufs['idx'][1].cpu().numpy().reshape(B, L),
                           s=bufs['s'][1].cpu().numpy().reshape(B, L),
                           guards=all(_intact(torch, full, view.numel()) for full, view in bufs.values()))


def run_tween(case: Case, dev, vals, alt=None, txt=None) -> SimpleNamespace:
    '''fd_guidance_tween through hip.call with lin_w = torch.linspace(lin0, lin1, L) and every output between guards: ws, idx, s
    as run_map, out [B][L][D], weights [B][L], status [B], guards.'''
    import ctypes
    import torch
    from flexdiffuse_amd import hip
    if alt is None:
        alt, txt = inputs(case)
    B, N, L, D = case.B, case.N, case.L, case.D
    ta, tt = torch.from_numpy(np.array(alt)).to(dev), torch.from_numpy(np.array(txt)).to(dev)
    lin_w = torch.linspace(vals[2], vals[3], steps=L).to(dev)
    sizes = {'ws': (B * N * L, torch.float32), 'out': (B * L * D, torch.float32), 'weights': (B * L, torch.float32),
             'idx': (B * L, torch.int32), 's': (B * L, torch.float32), 'status': (B, torch.int32)}
    bufs = {k: _guarded(torch, n, dt, dev) for k, (n, dt) in sizes.items()}
    p = params_of(vals)
    hip.call('fd_guidance_tween', hip.ptr(tt), hip.ptr(ta), hip.ptr(lin_w), *(hip.ptr(bufs[k][1]) for k in
             ('ws', 'out', 'weights', 'idx', 's', 'status')), B, int(case.batched), N, L, D, ctypes.byref(p), hip.stream())
    torch.cuda.synchronize()
    host = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    return SimpleNamespace(ws=host['ws'].reshape(B, N, L), out=host['out'].reshape(B, L, D), weights=host['weights'].reshape(B, L),
                           idx=host['idx'].reshape(B, L), s=host['s'].reshape(B, L), status=host['status'],
                           guards=all(_intact(torch, full, view.numel()) for full, view in bufs.values()))


def mapped_of(idx_row: np.ndarray, s_row: np.ndarray) -> np.ndarray:
    '''(L, 2) float64 mapping of one prompt from the device's idx and s.'''
    m = np.zeros((idx_row.shape[0], 2))
    m[:, 0] = idx_row
    m[:, 1] = s_row.astype(np.float64)
    return m


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.int32)
