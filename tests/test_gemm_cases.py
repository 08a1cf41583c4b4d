'''CPU checks of tests/gemm_cases.py: the Python restatement of launch_epi / launch_mode returns exactly the launch targets that
csrc/gemm.hip can launch, the case table reaches every one of them (and every arm of the FD_GEMM_* / FD_CONV_TAPFAST switches), and the
acceptance criterion `check` accepts an fp32 emulation of every screened case while rejecting twelve kinds of wrong GEMM.  The tile id
and split factor of a case come from fd_gemm_plan (host logic only), so the library must be built; no device is needed.'''
import os
import re
import sys
from itertools import product
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'flexdiffuse_amd', 'csrc', 'gemm.hip')
ENVS = ({},) + gc.ENV_SETTINGS
LIVE = [c for c in gc.CASES if not gc.refused(c)]


def _b(s):
    return s == 'true'


# ------------------------------------------------------------------------------------------------ the source's launch targets
def source_targets():
    '''{(form, (BM, BN, WM, NS, WN, EPI, CONV, TRANS))} that csrc/gemm.hip can launch, read from: the `switch (best_tile)` lines, the body
    of launch_epi (which EPI sits behind which ALLOW bit / tile-shape condition, and whether it goes through launch<> -- linear and
    convolution -- or launch_mode<..., false, false, ...> -- linear only), every launch_mode<> / launch<> call with literal arguments, and
    the two predicates of launch_mode (persistent form; register-staged fallback).'''
    src = open(SRC).read()
    # -- launch_epi: EPI -> (guard, needs the even-fragment condition, linear and convolution)
    body = src[src.index('static int launch_epi('):src.index('// 1 when fd_gemm_f16 can honour fd_gemm_desc.ln_stats_out')]
    epis, guard, glu = {}, None, False
    for line in body.splitlines():
        if 'if constexpr' in line:
            m = re.search(r'ALLOW & (\d+)', line)
            guard = int(m.group(1)) if m else ('row320' if 'BN == 320 && NS == 2' in line else None)
            assert guard is not None, line
            glu = '(BN / WN / 16) % 2 == 0' in line
        for m in re.finditer(r'(launch|launch_mode)<BM, BN, false, (?:false, )?WM, NS, WN, (\d+)>', line):
            epi = int(m.group(2))
            epis[epi] = (None, False, True) if epi == 0 else (guard, glu, m.group(1) == 'launch')
    assert sorted(epis) == [0, 1, 2, 3, 5, 6, 8, 9, 11, 12], epis
    tpls = set()
    # -- the switch
    sw = src[src.index('switch (best_tile) {'):]
    sw = sw[:sw.index('#ifdef FD_SPLITK_NO_FINISH')]
    lean_ids, generic_ids = {}, {}
    for m in re.finditer(r'(?:case (\d+)|default): rc = (launch_epi|launch)<([^>]*)>\(g, batch, st\)', sw):
        tid, a = int(m.group(1)) if m.group(1) else 1, [x.strip() for x in m.group(3).split(',')]
        if m.group(2) == 'launch_epi':
            BM, BN, WM, NS, WN = (int(x) for x in a[:5])
            allow = sum(int(x) for x in a[5].split('+'))
            lean_ids[tid] = (BM, BN, WM, NS, WN, allow)
            for epi, (gd, need_glu, both) in epis.items():
                ok = gd is None or (gd == 'row320' and BN == 320 and NS == 2) or (gd != 'row320' and allow & gd)
                if ok and (not need_glu or (BN // WN // 16) % 2 == 0):
                    for conv in ((False, True) if both else (False,)):
                        tpls.add((BM, BN, WM, NS, WN, epi, conv, False))
        else:
            BM, BN, WM, NS = int(a[0]), int(a[1]), int(a[3]) if len(a) > 3 else 2, int(a[4]) if len(a) > 4 else 2
            assert not _b(a[2])
            generic_ids[tid] = (BM, BN, WM, NS, 2)
            for conv in (False, True):
                tpls.add((BM, BN, WM, NS, 2, 0, conv, False))
    # -- explicit calls with literal arguments (the small LayerNorm-fold kernels, the transposed stores, the transposed tail)
    for m in re.finditer(r'launch_mode<(\d+), (\d+), (true|false), (true|false), (\d+), (\d+), (\d+), (\d+)>', src):
        BM, BN, TR, CV, WM, NS, WN, EPI = m.groups()
        tpls.add((int(BM), int(BN), int(WM), int(NS), int(WN), int(EPI), _b(CV), _b(TR)))
    for m in re.finditer(r'launch<(\d+), (\d+), true>\(g, batch, st\)', src):
        for conv in (False, True):
            tpls.add((int(m.group(1)), int(m.group(2)), 2, 2, 2, 0, conv, True))
    # -- forms
    lm = src[src.index('static int launch_mode('):src.index('static int launch(GemmArgs')]
    assert 'const bool persistent = NS == 2 && BN != 320 && EPI != 13 && g.K2 == 0 && !g.phase && !g.ln_stats_out && g.ln_parts <= 1 && g.strideBias == 0' in lm
    assert 'if constexpr (EPI != 0) {' in lm and '} else if constexpr (WM != 2 || WN != 2) {' in lm and 'k_gemm_f16<BM, BN, TRANS, CONV>' in lm
    out = set()
    for t in tpls:
        BM, BN, WM, NS, WN, EPI, CONV, TRANS = t
        out.add(('dma', t))
        if NS == 2 and BN != 320 and EPI not in (13, 8, 9, 11, 12):       # (8, 9: ln_stats_out is set; 11, 12: 320 wide)
            out.add(('dmap', t))
        if EPI == 0 and WM == 2 and WN == 2:
            out.add(('reg', t))
    return out, lean_ids, generic_ids


def test_the_tile_tables_are_those_of_the_switch():
    _, lean_ids, generic_ids = source_targets()
    assert lean_ids == gc.LEAN
    assert generic_ids == gc.GENERIC


def restated_targets():
    '''Every (form, tpl) `select` returns over a grid of abstract launches: each tile id x operation flags x full / ragged shapes, one-shot
    (FD_GEMM_PERSIST=0), persistent wherever the predicate allows (=2) and register-staged (FD_GEMM_NO_DMA).'''
    out = set()
    envs = ({'FD_GEMM_PERSIST': '0'}, {'FD_GEMM_PERSIST': '2'}, {'FD_GEMM_NO_DMA': '1'})
    shapes = {}
    for tid, t in list(gc.LEAN.items()) + list(gc.GENERIC.items()) + [(-7, (128, 128))]:
        shapes[tid] = ((2 * t[0], 2 * t[1]), (2 * t[0], t[1]), (t[0] + 1, t[1] + 4))
    for tid in shapes:
        for (M, N), conv, act, res, ln, so, gp, b2, env in product(shapes[tid], (False, True), (gc.ACT_NONE, gc.ACT_SILU, gc.ACT_GEGLU), (False, True),
                                                                   (0, 1, 2), (False, True), (False, True), (False, True), envs):
            if (tid == -7 and not ln) or (ln and conv):
                continue
            g = SimpleNamespace(M=M, N=N, K=64, K2=0, act=act, res=res, ldr=N, ldc=N, bias=True, bias2=b2, rows=M // 2 if M % 2 == 0 else M, out_f32=False,
                                trans=False, trans_n0=0, conv=conv, ln=ln > 0, ln_parts=ln if ln > 1 else 0, stats_out=so, gn_part=gp, gn_out=False,
                                stride_bias=False, batch=1)
            try:
                L = gc.select(g, tid, 1, env)
                out.add((L.form, L.tpl))
            except ValueError:
                pass
    for M, N, conv, ln, n0, env in product((256, 8192), (128, 160), (False, True), (0, 1), (0, 320), envs):
        if ln and conv:
            continue
        g = SimpleNamespace(M=M, N=N + n0, K=64, K2=0, act=gc.ACT_NONE, res=False, ldr=0, ldc=n0, bias=True, bias2=False, rows=128, out_f32=False, trans=not n0,
                            trans_n0=n0, conv=conv, ln=ln > 0 or n0 > 0, ln_parts=0, stats_out=False, gn_part=False, gn_out=False, stride_bias=False, batch=1)
        try:
            L = gc.select(g, 0, 1, env)
            out.add((L.form, L.tpl))
        except ValueError:
            pass
    return out


def test_the_restatement_returns_exactly_the_targets_the_source_can_launch():
    src, _, _ = source_targets()
    mine = restated_targets()
    assert mine == src, f'only restated: {sorted(mine - src)}\nonly in the source: {sorted(src - mine)}'
    assert len(src) > 150


def _reached():
    got = {}
    for env in ENVS:
        cases = LIVE if not env else gc.child_cases(env)[0]
        for c in cases:
            L = gc.expected_launch(c, env)
            got.setdefault((L.form, L.tpl), []).append((c.id, env))
    return got


def test_every_launch_target_is_reached_by_a_case():
    src, _, _ = source_targets()
    got = _reached()
    assert not set(got) - src, sorted(set(got) - src)
    missing = sorted(src - set(got))
    assert not missing, f'{len(missing)} launch targets without a case: {missing}'
    # the one-shot and persistent forms are reached without any switch; only the register-staged kernel needs FD_GEMM_NO_DMA
    plain = {(gc.expected_launch(c).form, gc.expected_launch(c).tpl) for c in LIVE}
    assert {t for t in src if t[0] != 'reg'} <= plain, sorted({t for t in src if t[0] != 'reg'} - plain)


def test_every_switch_changes_the_launch_of_some_case_and_the_finish_kernels_are_reached():
    for env in gc.ENV_SETTINGS:
        run, skipped = gc.child_cases(env)
        assert len(run) >= 3, (env, len(run))
    # settings that make the library refuse what it ran before
    assert gc.child_cases({'FD_GEMM_NO_DMA': '1'})[1] and gc.child_cases({'FD_GEMM_FAST_EPI': '0'})[1]
    fin = {gc.expected_launch(c).finish for c in LIVE}
    assert fin == {None, 'k_splitk_finish', 'k_splitk_finish_gn<2>', 'k_splitk_finish_gn<4>', 'k_splitk_finish_gn<8>', 'k_splitk_finish_gn<16>'}
    assert {c.split for c in LIVE if gc.expected_launch(c).finish == 'k_splitk_finish'} == {2, 4, 8, 16}


# ------------------------------------------------------------------------------------------------ the coverage the table promises
def _slots(tpl):
    BM, BN, WM, NS, WN, EPI = tpl[:6]
    return gc._slots(BM, BN, EPI, NS)


def test_walks_would_show_a_stale_bias_buffer():
    '''Every walk of the persistent kernel (but the split-K one, whose bias the finish pass adds): an eighth of the workgroups or more walk two
    tiles, and the second lies in another tile column than the first (it is slots / 8 places further in the XCD's chunk), so a bias buffer
    that is not flipped between tiles, or a tile index taken from the wrong walk step, changes the result.'''
    n = 0
    for c in LIVE:
        L = gc.expected_launch(c)
        if L.form != 'dmap' or c.split > 1:
            continue
        n += 1
        slots, tn = _slots(L.tpl), gc._cdiv(c.N, L.tpl[1])
        tiles = gc._cdiv(c.M, L.tpl[0]) * tn
        assert tiles * 8 >= slots * 9 and tiles < 2 * slots and tiles % slots and tiles % 8 and (slots // 8) % tn, (c.id, tiles, slots, tn)
    assert n >= 90


def test_lean_tiles_one_shot_and_walking():
    '''Every (tile, EPI, CONV) launch_epi can return, one-shot with 2 x 2 tiles (the row-spanning statistics epilogues: N == BN or whole slabs), and
    -- where a persistent form exists -- on a walk with more tiles than slots, not a multiple of the slots nor of 8, K <= 192; one ragged walk per tile.'''
    src, lean_ids, _ = source_targets()
    launches = [(c, gc.expected_launch(c)) for c in LIVE]
    for tid, (BM, BN, WM, NS, WN, _) in lean_ids.items():
        for form, tpl in sorted(t for t in src if t[1][:5] == (BM, BN, WM, NS, WN) and not t[1][7] and t[1][5] != 13 and t[0] != 'reg'):
            mine = [c for c, L in launches if c.tile == tid and (L.form, L.tpl) == (form, tpl)]
            if form == 'dma':
                assert any(c.M % BM == 0 and c.M >= 2 * BM and (c.N == 2 * BN or tpl[5] in (8, 9, 11, 12)) for c in mine), (tid, form, tpl)
            else:
                ok = [c for c in mine if c.K <= 192 and (t := gc._cdiv(c.M, BM) * gc._cdiv(c.N, BN)) > _slots(tpl) and t % _slots(tpl) and t % 8]
                assert ok, (tid, form, tpl)
                if tpl[5] == 0 and not tpl[6]:
                    assert any(gc.is_ragged(c) for c in ok), (tid, 'ragged walk')
    # EPI 7 through both small kernels
    assert {(128, 128), (64, 64)} <= {L.tpl[:2] for c, L in launches if L.tpl[5] == 7 and not L.tpl[7]}


def test_generic_tiles_transposed_stores_statistics_and_split_k():
    launches = {c.id: gc.expected_launch(c) for c in LIVE}
    by = lambda pred: [c for c in LIVE if pred(c, launches[c.id])]
    for tid in list(range(1, 9)) + [11]:
        for conv in (False, True):
            assert by(lambda c, L: c.tile == tid and L.tpl[5] == 0 and L.tpl[6] == conv and c.act != gc.ACT_GEGLU and not c.ln), (tid, conv)
    # both transposed-store forms, plain and with the fold; the 128x160 form at N = 160, K = 64
    for bn in (64, 160):
        for epi in (0, 7):
            assert by(lambda c, L: L.tpl[7] and L.tpl[1] == bn and L.tpl[5] == epi), (bn, epi)
    assert by(lambda c, L: L.tpl[7] and L.tpl[1] == 160 and c.N == 160 and c.K == 64 and c.M >= 8192)
    assert by(lambda c, L: L.tpl[5] == 13 and c.trans_n0 == 320 and c.N == 480 and c.M // c.rows == 2)
    # row statistics: slabs from tiles 12, 13, 20, 23, finished pairs from tile 16; GroupNorm partial sums from tile 16
    for tid in (12, 13, 20, 23, 16):
        for epi in (8, 9):
            hit = by(lambda c, L: gc.plan(c)[0] == tid and L.tpl[5] == epi)
            assert hit and all((c.N == 320 and tid == 16) or (tid != 16 and c.N // 160 >= 2) for c in hit), (tid, epi)
    for epi in (11, 12):
        assert by(lambda c, L: gc.plan(c)[0] == 16 and L.tpl[5] == epi and not L.tpl[6]) and by(lambda c, L: L.tpl[5] == epi and L.tpl[6])
    # split-K: the finish pass sees a residual, a wrapped residual, a per-sample bias, an activation and an fp32 output; uneven and empty slices
    sk = by(lambda c, L: L.finish == 'k_splitk_finish')
    assert any(c.res for c in sk) and any(c.res_rows for c in sk) and any(c.bias2 for c in sk) and any(c.act for c in sk) and any(c.out_f32 for c in sk)
    assert any(gc._cdiv(c.K + c.K2, 64) % c.split for c in sk)
    assert any(c.K == 320 and c.split == 4 for c in sk)
    empty = [c for c in sk if gc._cdiv(gc._cdiv(c.K + c.K2, 64), c.split) * (c.split - 1) >= gc._cdiv(c.K + c.K2, 64)]
    assert len(empty) >= 2, 'a slice without K-tiles'


def test_every_layout_and_edge_reaches_every_kernel():
    '''padded / k_tail / ragged / alpha / batch / per-batch bias / wrapped residual / per-sample bias / padded transposed rows on k_gemm_f16_dma,
    k_gemm_f16_dmap and (under FD_GEMM_NO_DMA) k_gemm_f16.  Two combinations do not exist: the persistent and the register-staged kernel
    do not stage a per-batch bias (launch_mode's predicate / fd_gemm_f16's argument check).'''
    seen = {}
    for env in ({}, {'FD_GEMM_NO_DMA': '1'}):
        for c in (LIVE if not env else gc.child_cases(env)[0]):
            k = gc.expected_launch(c, env).kernel
            seen.setdefault(k, set()).update(c.edges | ({'ragged'} if gc.is_ragged(c) else set()))
    assert set(seen) == {'k_gemm_f16_dma', 'k_gemm_f16_dmap', 'k_gemm_f16'}
    assert seen['k_gemm_f16_dma'] >= set(gc.EDGES)
    assert seen['k_gemm_f16_dmap'] >= set(gc.EDGES) - {'batch_bias'}, set(gc.EDGES) - seen['k_gemm_f16_dmap']
    assert seen['k_gemm_f16'] >= set(gc.EDGES) - {'batch_bias'}, set(gc.EDGES) - seen['k_gemm_f16']
    # K-tile counts 1, 2, 3, 4 and an odd count > 4 on every tile; 1 and an odd count on the 3-stage tiles
    for tid in list(gc.LEAN) + list(gc.GENERIC):
        counts = {gc._cdiv(c.K + c.K2, 64) for c in LIVE if c.tile == tid and c.split == 1}
        assert {1, 2, 3, 4} <= counts and any(n > 4 and n % 2 for n in counts), (tid, counts)


def test_inputs_are_what_the_table_says():
    for c in LIVE[::7]:
        inp, p = gc.inputs(c), gc.layout_plan(c)
        b = inp['bias'][0]
        d = b[1:] - b[:-1]
        if c.act == gc.ACT_NONE:
            assert bool((d == 0.25).all())                                         # a distinct bias per column
        else:                                                                      # ... within a few units of 0 behind an activation
            bn = gc.expected_launch(c).tpl[1]
            assert bool(((d == 0.25) | (d == -0.25 * (gc.BIAS_PERIOD - 1))).all()) and float(b.abs().max()) <= 3.5
            assert all(bool((b[k * bn:] != b[:c.N - k * bn]).all()) for k in range(1, gc._cdiv(c.N, bn)))    # and distinct between tile columns
        if c.layout == 'padded':
            assert p['ldw'] > c.K + c.K2 and (c.trans or p['ldc'] > (c.trans_n0 or c.n_out)) and p['ldr'] != p['ldc']
            h = gc.host_buffers(c, inp)
            assert float(h['W'].view(c.batch, -1)[0, :c.N * p['ldw']].view(c.N, p['ldw'])[:, c.K + c.K2:].min()) == gc.PAD_IN     # junk right after column K
        if c.ln == 1:
            x = inp['A'][0].double()
            assert float(x.mean(1).abs().max()) > 0.5 and float(x.std(1).max() / x.std(1).min()) > 2


# ------------------------------------------------------------------------------------------------ the criterion, screened with mutants
@pytest.mark.parametrize('case', LIVE, ids=lambda c: c.id)
def test_check_accepts_the_emulation_and_rejects_every_mutant(case):
    '''`check` accepts the fp32 emulation (fp16 operands, fp32 accumulation over reversed 64-wide K chunks, the epilogue in fp32, the output
    rounded to fp16) and rejects each mutant that is a different computation for the case -- on every case, the persistent walks included.
    No output tile of the case's launch is dead: a tenth of its reference or more is at least ten times the bound's absolute term, so
    an error in that tile alone (a wrong tile index, a stale bias) has the relative bound to fail.'''
    inp = gc.inputs(case)
    want = gc.reference(case, inp)
    assert gc.tile_liveness(case, want) >= 0.1, f'a tile with only {gc.tile_liveness(case, want):.2f} of its reference above {gc.LIVE_ABS}'
    cache = {}
    emu = gc.emulate(case, inp, cache=cache)
    r = gc.worst(case, emu, want)
    assert r <= 1.0, f'the emulation misses the bound: err / bound = {r:.3f}'
    for mut in gc.MUTANTS:
        bad = gc.emulate(case, inp, mut, cache)
        assert (bad is None) == (not gc.applies(case, mut))
        if bad is not None:
            assert not gc.check(case, bad, want), f'{mut} passes the bound (err / bound = {gc.worst(case, bad, want):.3f})'


def test_the_screen_shows_every_mutant_to_every_epilogue():
    '''The screen above shows every kernel the K-chunk and bias mutants and every EPI all the mutants that apply to it.'''
    screened = {'kernels': {}, 'epis': {}}
    for case in LIVE:
        L, applied = gc.expected_launch(case), {m for m in gc.MUTANTS if gc.applies(case, m)}
        screened['kernels'].setdefault(L.kernel, set()).update(applied)
        screened['epis'].setdefault(L.tpl[5], set()).update(applied)
    for k in ('k_gemm_f16_dma', 'k_gemm_f16_dmap'):
        assert {'k_chunk', 'bias_next', 'tile_swap'} <= screened['kernels'][k]
    res, ln, b2 = {'res_drop', 'res_row_next', 'res_ldc'}, {'stats_row_xor1', 'colsum_next'}, {'bias2_border'}
    want = {0: res | b2 | {'alpha_ignored', 'geglu_swap', 'tile_swap', 'trans_ld'}, 1: b2 | {'alpha_ignored', 'tile_swap'}, 2: res | b2 | {'tile_swap'},
            3: {'geglu_swap', 'tile_swap'}, 5: ln | {'tile_swap'}, 6: ln | {'geglu_swap', 'tile_swap'}, 7: ln | {'geglu_swap', 'trans_ld'},
            8: {'tile_swap'}, 9: res | {'tile_swap'}, 11: b2, 12: res, 13: ln | {'trans_ld'}}
    assert set(want) == set(screened['epis'])
    for epi, muts in want.items():
        assert muts | {'k_chunk', 'bias_next'} <= screened['epis'][epi], (epi, sorted((muts | {'k_chunk', 'bias_next'}) - screened['epis'][epi]))


STATS = [c for c in LIVE if c.stats_out or c.gn_parts]


@pytest.mark.parametrize('case', STATS, ids=lambda c: c.id)
def test_stats_check_accepts_fp32_sums_and_rejects_a_neighbours(case):
    '''The bound on ln_stats_out / gn_part_out accepts one-pass fp32 statistics of the fp16 rows and rejects those of the row (group) next door.'''
    c16 = gc.emulate(case)['C']
    x = c16.float().reshape(-1, case.N)
    if case.stats_out:
        if gc.expected_launch(case).tpl[1] == 320:
            mean, s2 = x.sum(1) / case.N, (x * x).sum(1) / case.N
            rstd = ((s2 - mean * mean).clamp(min=0) + gc.LN_EPS).rsqrt()
            st = torch.stack([rstd, -mean * rstd], dim=1)
        else:
            xs = x.view(x.shape[0], case.N // 160, 160)
            st = torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=-1).permute(1, 0, 2).contiguous()
        assert gc.stats_check(case, c16, stats=st) <= 1.0
        assert gc.stats_check(case, c16, stats=st.roll(1, dims=-2)) > 1.0
    if case.gn_parts:
        xs = x.view(case.M // case.rows, case.rows // 256, 256, case.gn_parts, case.N // case.gn_parts)
        gp = torch.stack([xs.sum(dim=(2, 4)), (xs * xs).sum(dim=(2, 4))], dim=-1)
        assert gc.stats_check(case, c16, gn_parts=gp) <= 1.0
        assert gc.stats_check(case, c16, gn_parts=gp.roll(1, dims=2)) > 1.0
        assert gc.stats_check(case, c16, gn_parts=gp.roll(1, dims=0)) > 1.0
