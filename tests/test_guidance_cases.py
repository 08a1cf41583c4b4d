'''CPU self-test of tests/guidance_cases.py: the case table reaches every path of csrc/guidance.hip that it promises, the inputs hold
the content they promise (spread and sharp rows, exact zeros, a denormal column, ties, guides that cannot be swapped), the bound
T = 4 E comes from the pinned oracle's own error against float64, and the criterion of tests/test_gpu_guidance_cases.py rejects
eleven wrong computations.  Runs without a GPU.'''
import numpy as np
import pytest

import guidance_cases as GC
from oracle import guidance_ref as G

GENERAL = [c for c in GC.CASES if c.kind in ('general', 'ties_rows', 'ties_cols', 'ties_both')]
TWEEN_TRACE_CASES = ('general-N33-L65-D64', 'general-N257-L77-D768', 'general-N65-L96-D96')     # whose mappings the tween parameter sets are traced on


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def table32(case, b=0):
    '''The float64 table rounded to fp32, header column dropped, as float64: what a faultless device table would feed the oracle.'''
    return f32(GC.sim64(case)[b][:, 1:]).astype(np.float64)


def test_table_reaches_every_path():
    reached = set().union(*(GC.paths(c) for c in GC.CASES))
    assert GC.REQUIRED_PATHS <= reached, sorted(GC.REQUIRED_PATHS - reached)
    assert {1, 5, 31, 32, 33, 64, 65, 256, 257, 2048, GC.max_rows(77), GC.max_rows(96)} <= {c.N for c in GC.CASES}
    assert {2, 32, 33, 64, 65, 77, 96} <= {c.L for c in GC.CASES}
    for D in (32, 64, 96, 768, 1024):
        mine = [c for c in GC.CASES if c.D == D]
        assert any(c.N % 32 for c in mine) and any(c.L <= 64 for c in mine) and any(c.L > 64 for c in mine), D
    assert any(c.N == 2048 and c.L == 16 for c in GC.CASES)
    assert {c.N for c in GC.CASES if c.N < c.NC} >= {1, 5, 40}
    assert any(c.B == 3 and not c.batched for c in GC.CASES) and any(c.B == 3 and c.batched for c in GC.CASES)
    assert {c.N for c in GC.CASES if c.kind == 'zeros'} == {100, 300}


def test_lds_limits():
    '''The largest N of check_shapes' LDS budget, from its formula and sizeof(TweenShared) = 3120.'''
    for L in (77, 96):
        n = GC.max_rows(L)
        assert GC.lds_bytes(n, L) <= GC.LDS_BUDGET < GC.lds_bytes(n + 1, L)
    assert (GC.max_rows(77), GC.max_rows(96)) == (488, 387)
    assert GC.lds_bytes(2048, 16) <= GC.LDS_BUDGET


@pytest.mark.parametrize('case', GENERAL, ids=[c.id for c in GENERAL])
def test_general_content(case):
    '''Norms over 1e-3 .. 1e3, a row above 0.99 and a row that is as spread as L allows: largest entry below 0.2 (below 1.5 / L
    where L < 8: two columns cannot share less than a half).  A single guide row (N = 1) is the spread kind.'''
    alt, _ = GC.inputs(case)
    peak = GC.sim64(case).max(-1)                       # [B][N]
    spread = max(0.2, 1.5 / case.L)
    for b in range(case.B):
        assert peak[b].min() < spread, (case.id, b, peak[b].min())
        if case.N >= 4:
            assert peak[b].max() > 0.99, (case.id, b, peak[b].max())
    if case.N >= 4:
        norms = np.linalg.norm(alt.astype(np.float64), axis=-1)
        assert norms.min() <= 1e-3 and norms.max() >= 1e3, (case.id, norms.min(), norms.max())


def test_zero_and_denormal_content():
    for case in GC.CASES:
        if case.kind not in ('zeros', 'denormal'):
            continue
        t = f32(GC.sim64(case)[0])
        dead = [j for j in range(case.L) if j not in GC.ZERO_LIVE and not (case.kind == 'denormal' and j == GC.DENORMAL_ROW)]
        assert (t[:, dead] == 0).all(), case.id
        assert (t[:, list(GC.ZERO_LIVE)] > 0).all(), case.id
        if case.kind == 'denormal':
            col = GC.sim64(case)[0][:, GC.DENORMAL_ROW]
            assert 0 < col.max() < GC.FLT_MIN and col.max() > 1e-44, (col.min(), col.max())
            assert -np.log(col.max()) > 88 and -np.log(col.min()) < 103


def test_ties_content():
    '''The planted duplicates are bit-identical inputs, give equal float64 rows / columns, and are decisive: the kept row wins a
    column in every (order, reuse) pair that walks, and the duplicated outlier columns go to two different rows without reuse.'''
    for case in GC.CASES:
        alt, txt = GC.inputs(case)
        s = GC.sim64(case)[0]
        if case.kind in ('ties_rows', 'ties_both'):
            for keep, copy in GC.DUP_ROWS:
                assert np.array_equal(GC.bits(alt[0, keep]), GC.bits(alt[0, copy]))
                assert np.allclose(s[keep], s[copy], rtol=1e-13, atol=0)
            got = G.assign(table32(case), case.L, True, G.ORDER_ALIGN)
            assert {keep for keep, _ in GC.DUP_ROWS} <= set(got[:, 0].astype(int)), case.id
        if GC.dup_cols(case):
            for keep, copy in GC.dup_cols(case):
                assert np.array_equal(GC.bits(txt[0, keep]), GC.bits(txt[0, copy]))
                assert np.allclose(s[:, keep], s[:, copy], rtol=1e-13, atol=0)
                t = table32(case)
                assert np.array_equal(t[:, keep - 1], t[:, copy - 1])
            keep, copy = GC.dup_cols(case)[0]
            got = G.assign(table32(case), case.L, False, G.ORDER_ALIGN)
            assert got[keep - 1, 0] != got[copy - 1, 0] and got[keep - 1, 1] >= got[copy - 1, 1] > 0


def test_batched_guides_cannot_be_swapped():
    for case in GC.CASES:
        if not case.batched:
            continue
        alt, txt = GC.inputs(case)
        for b in range(case.B):
            own = G.assign(G.similarity(alt[b], txt[b]), case.L, True, G.ORDER_ALIGN)[:, 0]
            for o in range(case.B):
                if o != b:
                    other = G.assign(G.similarity(alt[o], txt[b]), case.L, True, G.ORDER_ALIGN)[:, 0]
                    assert not np.array_equal(own, other), (case.id, b, o)


def test_bound_from_the_oracle():
    '''E = the fp32 oracle's largest error against float64 over the table; T = 4 E.  E is dominated by rounding a logit near 100 to
    fp32 (half an ulp of 100 is 3.8e-6) passed on by the softmax with a factor below one half.'''
    E, T = GC.oracle_error(), GC.tolerance()
    print(f'\nguidance cases: E = {E:.3e} (oracle fp32 vs float64, {len(GC.CASES)} cases), T = 4 E = {T:.3e}')
    assert T == 4 * E
    assert 1e-7 < E < 2e-5, E     # an fp32 logit near 100 cannot be better than 1e-7 nor, summed over D <= 1024, worse than 2e-5


def test_restated_assignment_is_the_oracle():
    '''assign_with(defect=None) is oracle.guidance_ref.assign, on every case and pair (so a defect is the only difference).'''
    for case in GC.CASES:
        if case.N > 500 and case.kind == 'general' and case.N != 2048:
            continue
        t = table32(case)
        for order, reuse in GC.PAIRS:
            assert np.array_equal(GC.assign_with(t, case.L, reuse, order), G.assign(t, case.L, reuse, order)), (case.id, order, reuse)


@pytest.mark.parametrize('defect', GC.TABLE_DEFECTS)
def test_table_defect_is_rejected(defect):
    '''A wrong table must miss the bound by ten times or more on at least one case.'''
    T = GC.tolerance()
    worst = {}
    for case in GC.CASES:
        alt, txt = GC.inputs(case)
        worst[case.id] = float(np.abs(GC.sim64_of(alt, txt, defect) - GC.sim64(case)).max())
    caught = {k: v for k, v in worst.items() if v >= 10 * T}
    print(f'\n{defect}: rejected by {len(caught)} of {len(worst)} cases, worst {max(worst.values()):.3g} = {max(worst.values()) / T:.0f} T')
    assert caught, (defect, max(worst.values()), T)
    if defect == 'pad_leak':       # every case with padding columns holds a row on which they show
        assert all(v >= 10 * T for c, (k, v) in zip(GC.CASES, worst.items()) if c.L < GC.SIM_COLS and c in GENERAL and c.N >= 4), worst


@pytest.mark.parametrize('defect', GC.ASSIGN_DEFECTS)
def test_assignment_defect_is_rejected(defect):
    '''A wrong decision must change idx on at least one case and pair, on the table a faultless device would hold.'''
    kinds = {'tie_high_row': ('ties_rows', 'ties_both'), 'tie_high_col': ('ties_cols', 'ties_both'),
             'used_forgets_64': ('ties_rows', 'ties_both'), 'used_forgets_256': ('ties_rows', 'ties_both'),
             'zero_col_keeps_0': ('zeros',), 'zero_tail_lowest': ('zeros',), 'denormal_no_lock': ('denormal',)}[defect]
    caught = []
    for case in GC.CASES:
        if case.kind not in kinds:
            continue
        t = table32(case)
        for order, reuse in GC.PAIRS:
            if not np.array_equal(GC.assign_with(t, case.L, reuse, order, defect)[:, 0], G.assign(t, case.L, reuse, order)[:, 0]):
                caught.append((case.id, order, reuse))
    print(f'\n{defect}: rejected by {caught}')
    assert caught, defect
    if defect.startswith('used_forgets'):      # both walks that keep a `used` mask must notice
        assert {o for _, o, r in caught if not r} == {0, 1}, caught
    if defect == 'zero_tail_lowest':
        assert {(c, o) for c, o, r in caught if not r} == {(c.id, o) for c in GC.CASES if c.kind == 'zeros' for o in (0, 1)}, caught


def test_tween_sets_take_every_branch(guidance_goldens):
    '''Between them the chosen parameter sets take all three branches of blend_weights, the threshold stage, the header cap and the
    three blend modes, on mappings of the table's own cases.'''
    sets = GC.tween_sets(guidance_goldens)
    assert set(sets) == set(GC.TWEEN_SET_NAMES) | {GC.ADD_SET}
    assert {int(v[7]) for v in sets.values()} == {0, 1, 2} and {bool(v[8]) for v in sets.values()} == {True, False}
    seen = {}
    for case in GC.CASES:
        if case.id not in TWEEN_TRACE_CASES:
            continue
        for name, vals in sets.items():
            mapped = G.assign(table32(case), case.L, bool(vals[8]), int(vals[7]))
            seen[name] = seen.get(name, set()) | GC.tween_trace(mapped, vals, case.L)
    took = set().union(*seen.values())
    print('\n' + '\n'.join(f'{n}: {sorted(s)}' for n, s in seen.items()))
    assert GC.REQUIRED_TWEEN <= took, sorted(GC.REQUIRED_TWEEN - took)
    assert 'blend:add' in seen[GC.ADD_SET] and 'blend:min' in seen['neg_all'] and 'blend:max' in seen['defaults']
