'''CPU checks of tests/groupnorm_cases.py: its restatement of the GroupNorm dispatch names exactly the launch targets of
csrc/norm.hip, copies its constants and its launch-shape arithmetic correctly (all three hand copies of it), the table
reaches everything it promises, the refusals are the source's FD_CHECK_ARG conditions, and the acceptance bound passes
an fp32 emulation of every form while refusing twelve kinds of wrong GroupNorm.'''
import os
import re

import pytest
import torch

import groupnorm_cases as GN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'flexdiffuse_amd', 'csrc')
LIVE = GN.CASES
FORM = {c.id: GN.expected_form(c) for c in LIVE}
MUTANT_CAP = 1 << 22      # elements of x: above it a case is screened by the emulation alone (its form keeps smaller cases)


def _read(name):
    with open(os.path.join(CSRC, name), encoding='utf-8') as f:
        return f.read()


def _entry(src, name):
    '''Text of the extern "C" function `name`, from its signature to the next top-level closing brace.'''
    start = src.index(f'extern "C" int {name}(')
    return src[start:src.index('\n}\n', start)]


def _launches(text):
    return set(re.findall(r'hipLaunchKernelGGL\(\s*(\w+)\s*,', text))


def by_form(form):
    return [c for c in LIVE if FORM[c.id]['form'] == form]


# --------------------------------------------------------------------------------------------------- 1. the source
def test_restated_dispatch_names_the_launch_targets_of_the_source():
    src = _read('norm.hip')
    try_slab = src[src.index('static bool gn_try_slab('):src.index('\n}\n', src.index('static bool gn_try_slab('))]
    assert re.search(r'hipLaunchKernelGGL\(\(k_gn_slab<NT, NV>\)', try_slab), 'gn_try_slab no longer launches k_gn_slab<NT, NV>'
    found = {}
    for route, name in GN.ENTRY.items():
        body = _entry(src, name)
        found[route] = _launches(body) | {f'k_gn_slab<{a}, {b}>' for a, b in re.findall(r'gn_try_slab<(\d+), (\d+)>\(', body)}
    restated = {'full': set(GN.KERNELS['slab256'] + GN.KERNELS['slab1024'] + GN.KERNELS['stream']),
                'apply_parts': set(GN.KERNELS['apply_parts']), 'fold': set(GN.KERNELS['fold']), 'fold_parts': set(GN.KERNELS['fold_parts'])}
    assert found == restated, f'launch targets of the source {found} != the restatement {restated}'
    # the order in which fd_groupnorm_nhwc_ld_f16 tries the slabs, and its plain forwarder
    body = _entry(src, 'fd_groupnorm_nhwc_ld_f16')
    assert [(int(a), int(b)) for a, b in re.findall(r'gn_try_slab<(\d+), (\d+)>\(', body)] == list(GN.SLABS)
    assert 'return fd_groupnorm_nhwc_ld_f16(x, C, y, gamma, beta, ws, B, HW, C, G, eps, silu, stream);' in _entry(src, 'fd_groupnorm_nhwc_f16')
    for form in GN.FORMS:
        assert by_form(form), f'no live case runs {GN.KERNELS[form]} ({form})'


def test_restated_constants_still_hold_in_the_source():
    src, slab = _read('norm.hip'), _read('gn_slab.h')
    body = _entry(src, 'fd_groupnorm_nhwc_ld_f16')
    assert re.search(r'HW <= (\d+) && gn_try_slab<1024, 22>', body).group(1) == str(GN.SLAB2_MAX_HW)
    assert re.search(r'#define GN_MAX_CHUNKS (\d+)', src).group(1) == str(GN.GN_MAX_CHUNKS)
    assert re.search(r'#define GNF_ROWS (\d+)', src).group(1) == str(GN.GNF_ROWS)
    assert 'dim3(fd_cdiv(N, GNF_ROWS), B), dim3(%d)' % GN.FOLD_THREADS in src and 'const int nsub = %d / G;' % GN.FOLD_THREADS in src
    assert GN.SLAB_LDS == 160 * 1024 and 'if (bytes > 160 * 1024) break;' in slab and 'hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024' in src
    assert GN.FOLD_LDS == 48 * 1024 and src.count('FD_CHECK_ARG(lds2 <= 48 * 1024') == 2
    assert GN.STATS_LDS == 64 * 1024 and src.count('FD_CHECK_ARG(lds1 <= 64 * 1024') == 2
    assert 'const size_t lds2 = (size_t)GNF_ROWS * C * sizeof(half_t);' in src
    assert src.count('int PL = %d / c8;' % GN.STREAM_LANES) == 2 and 'int pl = %d / c8;' % GN.STREAM_LANES in src
    assert src.count('int nchunk = 256 / B;') == 2 and 'int nc = 256 / B;' in src
    assert 'c8 <= %d' % GN.MAX_C8 in body and 'G <= %d' % GN.MAX_G in body
    assert 'return (int64_t)B * GN_MAX_CHUNKS * G * 2;' in src
    # gn_slab_pick, line by line
    pick = slab[slab.index('static inline int gn_slab_pick('):]
    for line in ('if (C % G || (cpg & 1)) return 0;', 'for (int GB = 1; GB <= 8 && GB <= G; GB *= 2) {',
                 'if (G % GB || (cpg * GB) % 8) continue;', 'if (cb8 > NT || CB / 2 > NT) break;',
                 'const int pl = NT / cb8, J = NT / (CB / 2);', 'if ((HW + pl - 1) / pl > NV) break;',
                 'const size_t bytes = ((size_t)pl * CB + (size_t)J * CB + GB * 2) * sizeof(float);'):
        assert line in pick, f'gn_slab_pick changed: {line!r} is gone; restate it in groupnorm_cases.slab_pick'
    assert 'const int nt = blockDim.x, nsub = nt / G;' in src           # k_gn_apply's nsub


def _c_to_py(text, out_names):
    '''The straight-line integer C of the shape arithmetic as Python source.'''
    lines = []
    for raw in text.split('\n'):
        s = raw.split('//')[0].strip()
        if not s:
            continue
        assert s.endswith(';'), raw
        s = re.sub(r'\b(const|int|size_t)\b', '', s[:-1]).replace('*PL', 'PL_').replace('*threads', 'threads_')
        s = s.replace('*ppc', 'ppc_').replace('*nchunk', 'nchunk_').replace('/', '//').strip()
        m = re.match(r'if \((.*)\) (.*)', s)
        lines.append(f'if {m.group(1)}: {m.group(2)}' if m else s)
    return '\n'.join(lines) + '\nresult = (' + ', '.join(out_names) + ')'


def _shape_copies():
    src = _read('norm.hip')
    a = src[src.index('static void gn_stats_shape('):]
    a = a[a.index('{\n') + 2:a.index('\n}\n')]
    out = {'gn_stats_shape': _c_to_py(a, ('PL_', 'threads_', 'nchunk_', 'ppc_'))}
    for name in ('fd_groupnorm_nhwc_ld_f16', 'fd_groupnorm_apply_parts_f16'):
        body = _entry(src, name)
        assert 'const int c8 = C / 8;' in body, name
        lo = body.index('    int PL = ')
        hi = body.index('nchunk = fd_cdiv(HW, ppc);', lo) + len('nchunk = fd_cdiv(HW, ppc);')
        out[name] = _c_to_py('const int c8 = C / 8;\n' + body[lo:hi], ('PL', 'threads', 'nchunk', 'ppc'))
    return out


def test_three_copies_of_the_streaming_shape_agree_with_the_restatement():
    copies = _shape_copies()
    assert len(copies) == 3
    grid = [(B, HW, C) for B in (1, 2, 3, 16, 129, 255, 256, 257, 300) for HW in (1, 2, 5, 64, 170, 171, 1025, 1500, 4096, 16384)
            for C in (8, 24, 64, 320, 512, 520, 1280, 4096, 4104, 8184, 8192)]
    grid += [(c.B, c.HW, c.C) for c in LIVE]
    for name, code in copies.items():
        prog = compile(code, name, 'exec')
        for B, HW, C in grid:
            env = {'B': B, 'HW': HW, 'C': C, 'GN_MAX_CHUNKS': GN.GN_MAX_CHUNKS, 'fd_cdiv': GN.cdiv}
            exec(prog, env)
            assert env['result'] == GN.stream_shape(B, HW, C), \
                f'the copy of the streaming launch shape in {name} moved: (B, HW, C) = {(B, HW, C)} gives {env["result"]}, the others {GN.stream_shape(B, HW, C)}'
    # both users of gn_stats_shape and of the hand copies hand the same four numbers to the kernels
    src = _read('norm.hip')
    assert src.count('hipLaunchKernelGGL(k_gn_stats, dim3(nchunk, B), dim3(threads), lds1, st, (const half_t*)x, ws') == 2
    assert len(re.findall(r'hipLaunchKernelGGL\(k_gn_apply, dim3\(nchunk, B\), dim3\(threads\), lds2, st,', src)) == 2


def test_unreachable_branches_proven_by_sweep():
    '''GB = 8 is never chosen; `stats LDS too large` cannot fire once C / 8 <= 1024.'''
    for C in range(8, 8193, 8):
        PL1 = max(GN.STREAM_LANES // (C // 8), 1)
        assert PL1 * C * 8 <= GN.STATS_LDS, C                       # PL is at most this, whatever HW
        for G in range(1, 65):
            if C % G:
                continue
            for NT, NV in GN.SLABS:
                for HW in (1, NV, 64, 1024):
                    s = GN.slab_pick(NT, NV, HW, C, G)
                    assert s is None or s['GB'] in (1, 2, 4), (C, G, HW, s)
    assert GN.stream_shape(1, 1, 8192)[0] * 8192 * 8 == GN.STATS_LDS   # the limit is met exactly, at the widest C


# --------------------------------------------------------------------------------------------------- 2. coverage
def _has(pred, what, cases=LIVE):
    assert any(pred(c, FORM[c.id]) for c in cases), f'the table has no case with {what}'


def test_table_covers_every_boundary_of_the_dispatch():
    for form, (NT, NV) in zip(('slab256', 'slab1024'), GN.SLABS):
        _has(lambda c, f: f['form'] == form and c.HW == f['pl'] * NV, f'HW = pl * NV on {form}')
        # one pixel more leaves the kernel (same B, C, G)
        _has(lambda c, f: f['form'] != form and c.route == 'full' and
             (lambda s: s is not None and c.HW - 1 == s['pl'] * NV)(GN.slab_pick(NT, NV, c.HW - 1, c.C, c.G)), f'HW = pl * NV + 1 beyond {form}')
        _has(lambda c, f: f['form'] == form and f['idle'] > 0, f'idle lanes on {form}')
        _has(lambda c, f: f['form'] == form and f['idle'] == 0, f'no idle lane on {form}')
        _has(lambda c, f: f['form'] == form and f['CB'] // 2 == NT, f'CB / 2 = NT on {form}')
        _has(lambda c, f: f['form'] == form and f['nblk'] > 1, f'more than one group block on {form}')
    _has(lambda c, f: f['form'] == 'slab1024' and c.HW == 1024, 'HW = 1024 on slab1024')
    _has(lambda c, f: f['form'] == 'stream' and c.HW == 1025 and GN.slab_pick(1024, 22, 1025, c.C, c.G), 'HW = 1025 that only the gate sends to streaming')
    _has(lambda c, f: f['form'] == 'stream' and c.cpg % 2 == 0 and c.cpg // 2 > 1024, 'CB / 2 beyond NT = 1024')
    slabs = by_form('slab256') + by_form('slab1024')
    assert {FORM[c.id]['GB'] for c in slabs} == {1, 2, 4}, 'GB in {1, 2, 4}'
    js = {FORM[c.id]['J'] for c in slabs}
    assert 1 in js and 2 in js and any(j > 2 for j in js), f'J in (1, 2, > 2): {js}'
    for form in ('slab256', 'stream'):
        _has(lambda c, f: f['form'] == form and c.HW == 1, f'HW = 1 on {form}')


def test_table_covers_the_streaming_pair():
    st = by_form('stream')
    _has(lambda c, f: f['PL'] == 1, 'PL = 1', st)
    _has(lambda c, f: f['PL'] == c.HW > 1, 'PL = HW', st)
    _has(lambda c, f: f['threads'] == 64, '64-thread blocks', st)
    _has(lambda c, f: f['threads'] == 1024, '1024-thread blocks', st)
    _has(lambda c, f: f['idle'] > 0, 'idle lanes', st)
    _has(lambda c, f: f['idle'] == 0, 'no idle lane', st)
    _has(lambda c, f: c.B > 256 and f['nchunk'] == 1, 'one chunk (B > 256)', st)
    _has(lambda c, f: c.B == 1 and f['nchunk'] == GN.GN_MAX_CHUNKS, 'the most chunks (B = 1)', st)
    _has(lambda c, f: 0 < c.HW - (f['nchunk'] - 1) * f['ppc'] < f['PL'], 'a ragged last chunk shorter than PL', st)
    _has(lambda c, f: f['nchunk'] > 4 * f['nsub'], 'more chunks than 4 * nsub in the combine of k_gn_apply', st)
    tails = set()
    for c in st:
        tails |= {k % 4 for k in GN.lane_pixels(c) if k >= 12}
    assert tails == {0, 1, 2, 3}, f'lanes with >= 3 trips of the unrolled loop have tails {sorted(tails)} only'
    # fold shares k_gn_stats: at least its longest-lane case
    assert any(k >= 12 for c in by_form('fold') for k in GN.lane_pixels(c)), 'fold: no lane with 3 trips'
    _has(lambda c, f: min(GN.lane_pixels(c)) < 4, 'lanes with zero trips', st)
    _has(lambda c, f: f['form'] == 'apply_parts' and any(k >= 12 for k in GN.lane_pixels(c)), 'apply_parts with 3 trips of the store loop')
    for form in ('stream', 'apply_parts'):
        cs = by_form(form)
        _has(lambda c, f: c.cpg == 1, f'cpg 1 on {form}', by_form('stream'))
        _has(lambda c, f: c.cpg % 2 == 1 and c.cpg > 1, f'odd cpg on {form}', cs)
        _has(lambda c, f: c.cpg > 64, f'cpg > 64 on {form}', cs)
        _has(lambda c, f: c.G == 1, f'G = 1 on {form}', cs)
        _has(lambda c, f: f['threads'] % c.G != 0, f'G that does not divide the block on {form}', cs)
    _has(lambda c, f: c.G == 64, 'G = 64', st)
    _has(lambda c, f: c.G > f['threads'] // 64, 'more groups than waves', st)
    assert {24, 48} <= {c.G for c in st}


def test_table_covers_the_parts_and_fold_routes():
    for form in ('apply_parts', 'fold_parts'):
        for c in by_form(form):
            assert FORM[c.id]['combine'] == c.chunks > 0
        by_nsub = {}
        for c in by_form(form):
            by_nsub.setdefault(FORM[c.id]['nsub'], set()).add(c.chunks)
        assert any({1, n, 3 * n + 1, 256} <= ks and any(4 * n < k < 256 and k % n for k in ks) for n, ks in by_nsub.items()), \
            f'{form}: no nsub with chunks 1, nsub, 3 nsub + 1, beyond 4 nsub with a remainder, 256: {by_nsub}'
    folds = by_form('fold') + by_form('fold_parts')
    for form in ('fold', 'fold_parts'):
        ns = {c.N for c in by_form(form)}
        assert {8, 16, 24} <= ns and any(n >= 64 and n % 16 == 0 for n in ns), f'{form}: N in {sorted(ns)}'
        _has(lambda c, f: c.C == 1536, f'C = 1536 on {form}', by_form(form))
        _has(lambda c, f: c.G == 64, f'G = 64 on {form}', by_form(form))
        _has(lambda c, f: c.G == 1, f'G = 1 on {form}', by_form(form))
        _has(lambda c, f: c.indicator and c.means == 10, f'indicator weights at means = 10 on {form}', by_form(form))
    assert GN.refusal_code('fold', dict(B=1, HW=1, C=1544, G=8)) == GN.FD_ESHAPE and all(c.C <= 1536 for c in folds)
    _has(lambda c, f: c.N % 16 and c.N > 16, 'a last row block with fewer than 16 rows behind a full one', folds)


def test_every_form_sees_every_layout_mean_activation_and_eps():
    for form in GN.FORMS:
        cs = by_form(form)
        if form != 'fold_parts':                 # it never reads x
            assert {c.layout for c in cs} == set(GN.LAYOUTS), f'{form}: layouts {sorted({c.layout for c in cs})}'
        assert {c.means for c in cs} == {0, 1, 10}, f'{form}: means {sorted({c.means for c in cs})}'
        assert {c.eps for c in cs} == {1e-5, 1e-6}, f'{form}: eps {sorted({c.eps for c in cs})}'
        assert any(c.xscale != 1.0 for c in cs), f'{form}: no case whose variance is near eps'
        assert any(c.B >= 2 for c in cs)
        if form not in ('fold', 'fold_parts'):
            assert {c.silu for c in cs} == {True, False}, f'{form}: silu one way only'
    for c in LIVE:
        assert GN.refusal_code(c.route, dict(c._asdict(), ldx=GN.x_layout(c)['ldx'])) == GN.FD_OK, c.id
        L = GN.x_layout(c)
        assert L['ldx'] % 8 == 0 and L['off'] % 8 == 0 and L['off'] + (c.B * c.HW - 1) * L['ldx'] + c.C <= L['size']
        assert (c.layout == 'contig') == (L['ldx'] == c.C) and (c.layout == 'slice') == (L['off'] > 0)
        assert c.B * c.HW * L['ldx'] < 0x7fffffff and c.numel <= 1 << 25
        if 'stats_lds' in FORM[c.id]:
            assert FORM[c.id]['stats_lds'] <= GN.STATS_LDS


# --------------------------------------------------------------------------------------------------- 4. refusals
def _source_code(route, a):
    '''The first FD_CHECK_ARG of the route's entry point that the arguments fail, evaluated from the source text.'''
    body = _entry(_read('norm.hip'), GN.ENTRY[route])
    C, ldx = a['C'], a.get('ldx', a['C'])
    env = dict(B=a['B'], HW=a['HW'], C=C, G=a['G'], ldx=ldx, N=a.get('N', 16), chunks=a.get('chunks', 1), c8=C // 8,
               x=4096 + a.get('x_mis', 0), y=4096, ws=4096, wg=4096, w_out=4096, gamma=4096, beta=4096, parts=4096, biasf=4096, bias_out=4096,
               lds1=GN.stream_shape(a['B'], a['HW'], C)[0] * C * 8, lds2=GN.GNF_ROWS * C * 2)
    checks = re.findall(r'FD_CHECK_ARG\((.*?),\s*(FD_E\w+),', body, re.S)
    assert len(checks) >= 3, route
    for cond, code in checks:
        py = re.sub(r'\((uintptr_t|long long)\)', '', cond).replace('0x7fffffffLL', '0x7fffffff')
        py = py.replace('&&', ' and ').replace('||', ' or ').replace('/', '//').replace('\n', ' ')
        if not eval(py, {}, dict(env)):
            return {'FD_EINVAL': GN.FD_EINVAL, 'FD_ESHAPE': GN.FD_ESHAPE}[code]
    return GN.FD_OK


def test_refusals_are_the_conditions_of_the_source():
    names = {n for n, _, _ in GN.REFUSALS}
    assert names == {'C%8', 'C%G', 'G=65', 'C=8200', 'ldx<C', 'ldx%8', 'x+8B', 'C=1544', 'chunks=0'}
    for name, route, a in GN.REFUSALS:
        want = GN.refusal_code(route, a)
        assert want != GN.FD_OK, (name, route)
        assert _source_code(route, a) == want, f'{name} on {route}: the source answers {_source_code(route, a)}, the restatement {want}'
    for route in GN.ROUTES:
        assert _source_code(route, GN._GOOD) == GN.FD_OK == GN.refusal_code(route, GN._GOOD)
    for c in LIVE:
        assert _source_code(c.route, dict(c._asdict(), ldx=GN.x_layout(c)['ldx'])) == GN.FD_OK, c.id


# --------------------------------------------------------------------------------------------------- 3. the bound
@pytest.fixture(scope='module')
def screen():
    '''case id -> (emulation's worst ratio, bound / the project's flat bound, {mutant: worst ratio})'''
    out = {}
    for case in LIVE:
        inp = GN.inputs(case)
        good = GN.emulate(case, inp)
        want = GN.reference(case, inp, good)
        ratio = GN.accepted(case, good, inp)
        assert GN.check(case, good, want) == (ratio <= 1.0)
        muts = {}
        if case.numel <= MUTANT_CAP:
            muts = {m: GN.accepted(case, GN.emulate(case, inp, m), inp) for m in GN.MUTANTS if GN.applies(case, m)}
        out[case.id] = (ratio, GN.loose_bound_margin(case, want), muts)
    return out


def test_emulation_passes_check_everywhere(screen):
    worst = {}
    for case in LIVE:
        ratio, _, _ = screen[case.id]
        form = FORM[case.id]['form']
        worst[form] = max(worst.get(form, 0.0), ratio)
        assert ratio <= 1.0, f'{case.id}: the fp32 emulation of {form} is refused at {ratio:.3g} x the bound'
    print('emulation, worst |err| / bound per form: ' + '  '.join(f'{f} {worst[f]:.2f}' for f in GN.FORMS))
    assert set(worst) == set(GN.FORMS)


@pytest.mark.parametrize('case', LIVE, ids=[c.id for c in LIVE])
def test_bound_is_tighter_than_the_flat_bound_and_refuses_every_mutant(screen, case):
    ratio, margin, muts = screen[case.id]
    assert margin < 1.0, f'the derived bound reaches {margin:.3g} x (3e-3 + 3e-3 |want|) somewhere: change the inputs of the case'
    for m, r in muts.items():
        print(f'{m}: {r:.3g} x the bound')
    through = [m for m, r in muts.items() if r <= 1.0]
    assert not through, f'{case.id} lets {through} through the bound'


def test_every_form_saw_every_mutant_that_concerns_it(screen):
    concerns = {'slab256': {'drop_last_pixel', 'slab_pad_in_n', 'group_shift', 'no_ch0', 'prev_sample', 'var_nm1', 'no_eps', 'silu_flip', 'pad_read'},
                'stream': {'drop_last_pixel', 'drop_chunk', 'group_shift', 'prev_sample', 'var_nm1', 'no_eps', 'silu_flip', 'pad_read'},
                'apply_parts': {'drop_chunk', 'prev_sample', 'no_eps', 'silu_flip', 'pad_read'},
                'fold': {'drop_last_pixel', 'drop_chunk', 'group_shift', 'prev_sample', 'no_eps', 'pad_read', 'fold_bias_unrounded', 'fold_extra_row'},
                'fold_parts': {'drop_chunk', 'prev_sample', 'no_eps', 'fold_bias_unrounded', 'fold_extra_row'}}
    concerns['slab1024'] = concerns['slab256'] - {'var_nm1'}      # nothing that small takes the second slab kernel
    seen = {}
    for case in LIVE:
        seen.setdefault(FORM[case.id]['form'], set()).update(screen[case.id][2])
    for form, need in concerns.items():
        assert need <= seen.get(form, set()), f'{form}: no screened case applies {sorted(need - seen.get(form, set()))}'
    assert set().union(*seen.values()) == set(GN.MUTANTS)
    # every live case above the cap has a smaller sibling of its form
    for case in LIVE:
        if case.numel > MUTANT_CAP:
            assert any(c.numel <= MUTANT_CAP for c in by_form(FORM[case.id]['form']))


def test_the_supplied_parts_are_not_the_statistics_of_x():
    for case in by_form('apply_parts') + by_form('fold_parts'):
        inp = GN.inputs(case)
        st = GN.ref_stats(case, inp)
        mean, var, _, _ = GN.group_stats(inp['x16'].double(), case.G)
        moved = (st['mean'] - mean).abs() / var.sqrt().clamp(min=1e-30)
        if case.G > 1:
            assert float(moved[:, 1::2].min()) > 0.4, case.id
        assert float(moved[:, 0::2].max()) < 1e-3, case.id
        assert inp['parts'].shape == (case.B, case.chunks, case.G, 2) and inp['parts'].dtype == torch.float32


# --------------------------------------------------------------------------------------------------- the device driver
class _HostLib:
    '''The five entry points as float64 torch on the HOST memory the pointers name, rounded once: an honest kernel that
    lets the GPU test's driver (layouts, guards, workspace, read-back) run without a device.  `spill` makes it write one
    element past the end of its first output.'''

    def __init__(self, spill=False):
        self.spill = spill

    @staticmethod
    def _view(ptr, n, dtype):
        import ctypes
        ct = ctypes.c_uint16 if dtype == torch.float16 else ctypes.c_float
        return torch.frombuffer((ct * n).from_address(ptr), dtype=dtype)

    def fd_groupnorm_workspace_floats(self, B, G):
        return B * GN.GN_MAX_CHUNKS * G * 2

    def _stats(self, x, ldx, B, HW, C, G, parts=None, chunks=0):
        n = HW * (C // G)
        if parts is not None:
            p = self._view(parts, B * chunks * G * 2, torch.float32).double().reshape(B, chunks, G, 2).sum(1)
            s, q = p[..., 0], p[..., 1]
        else:
            v = torch.as_strided(self._view(x, (B * HW - 1) * ldx + C, torch.float16), (B, HW, C), (HW * ldx, ldx, 1)).double()
            v = v.reshape(B, HW, G, C // G)
            s, q = v.sum((1, 3)), (v * v).sum((1, 3))
        mean = s / n
        return mean, (q / n - mean * mean).clamp(min=0)

    def _apply(self, x, ldx, y, gamma, beta, B, HW, C, G, eps, silu, mean, var):
        code = GN.refusal_code('full', dict(B=B, HW=HW, C=C, G=G, ldx=ldx, x_mis=x % 16))
        if code:
            return code
        v = torch.as_strided(self._view(x, (B * HW - 1) * ldx + C, torch.float16), (B, HW, C), (HW * ldx, ldx, 1)).double()
        g, b = self._view(gamma, C, torch.float32).double(), self._view(beta, C, torch.float32).double()
        cpg = C // G
        t = (v - mean.repeat_interleave(cpg, 1)[:, None]) * ((var + eps) ** -0.5).repeat_interleave(cpg, 1)[:, None] * g + b
        out = self._view(y, B * HW * C + 1, torch.float16)
        out[:B * HW * C] = (t * torch.sigmoid(t) if silu else t).half().reshape(-1)
        if self.spill:
            out[B * HW * C] = 0
        return 0

    def fd_groupnorm_nhwc_ld_f16(self, x, ldx, y, gamma, beta, ws, B, HW, C, G, eps, silu, st):
        if GN.refusal_code('full', dict(B=B, HW=HW, C=C, G=G, ldx=ldx, x_mis=x % 16)):
            return GN.refusal_code('full', dict(B=B, HW=HW, C=C, G=G, ldx=ldx, x_mis=x % 16))
        case = GN.Case(B, HW, C, G)
        f = GN.expected_form(case)
        if f['form'] == 'stream':
            self._view(ws, B * f['nchunk'] * G * 2, torch.float32).fill_(0.5)
        return self._apply(x, ldx, y, gamma, beta, B, HW, C, G, eps, silu, *self._stats(x, ldx, B, HW, C, G))

    def fd_groupnorm_nhwc_f16(self, x, y, gamma, beta, ws, B, HW, C, G, eps, silu, st):
        return self.fd_groupnorm_nhwc_ld_f16(x, C, y, gamma, beta, ws, B, HW, C, G, eps, silu, st)

    def fd_groupnorm_apply_parts_f16(self, x, ldx, y, gamma, beta, parts, chunks, B, HW, C, G, eps, silu, st):
        code = GN.refusal_code('apply_parts', dict(B=B, HW=HW, C=C, G=G, ldx=ldx, x_mis=x % 16, chunks=chunks))
        return code or self._apply(x, ldx, y, gamma, beta, B, HW, C, G, eps, silu, *self._stats(x, ldx, B, HW, C, G, parts, chunks))

    def _fold(self, mean, var, B, C, G, eps, wg, biasf, N, w_out, bias_out):
        cpg = C // G
        w = self._view(wg, N * C, torch.float16).double().reshape(N, C)[None] * ((var + eps) ** -0.5).repeat_interleave(cpg, 1)[:, None]
        w16 = w.half()
        out = self._view(w_out, B * N * C + 1, torch.float16)
        out[:B * N * C] = w16.reshape(-1)
        if self.spill:
            out[B * N * C] = 0
        S = w16.double().reshape(B, N, G, cpg).sum(3)
        self._view(bias_out, B * N, torch.float32)[:] = (self._view(biasf, N, torch.float32).double()[None] - (mean[:, None] * S).sum(2)).float().reshape(-1)
        return 0

    def fd_groupnorm_fold_linear_f16(self, x, ldx, ws, B, HW, C, G, eps, wg, biasf, N, w_out, bias_out, st):
        code = GN.refusal_code('fold', dict(B=B, HW=HW, C=C, G=G, ldx=ldx, x_mis=x % 16, N=N))
        if code:
            return code
        self._view(ws, B * GN.stream_shape(B, HW, C)[2] * G * 2, torch.float32).fill_(0.5)
        return self._fold(*self._stats(x, ldx, B, HW, C, G), B, C, G, eps, wg, biasf, N, w_out, bias_out)

    def fd_groupnorm_fold_linear_parts_f16(self, parts, chunks, B, HW, C, G, eps, wg, biasf, N, w_out, bias_out, st):
        code = GN.refusal_code('fold_parts', dict(B=B, HW=HW, C=C, G=G, N=N, chunks=chunks))
        return code or self._fold(*self._stats(0, 0, B, HW, C, G, parts, chunks), B, C, G, eps, wg, biasf, N, w_out, bias_out)


def _patch(monkeypatch, lib):
    from flexdiffuse_amd import hip

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc:
            raise ValueError(name)

    monkeypatch.setattr(hip, 'lib', lambda: lib)
    monkeypatch.setattr(hip, 'call', call)
    monkeypatch.setattr(hip, 'stream', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)


def test_device_driver_against_a_host_stand_in(monkeypatch):
    '''run_on_device and call_refused with the library replaced by the stand-in: every route and layout hands the kernel
    the operands the reference sees, reads the outputs back from where they were written, and notices a write one
    element past an output, a write beyond the used part of the workspace, and a refusal that is not one.'''
    _patch(monkeypatch, _HostLib())
    small = [c for c in LIVE if c.numel <= 1 << 18]
    assert {c.route for c in small} == set(GN.ROUTES) and {c.layout for c in small} == set(GN.LAYOUTS)
    assert {FORM[c.id]['form'] for c in small} == set(GN.FORMS)
    for case in small:
        inp = GN.inputs(case)
        got = GN.run_on_device(case, 'cpu', inp)
        assert got['untouched'] and got['inputs_kept'], case.id
        assert GN.check(case, got, GN.reference(case, inp, got)), case.id
    for name, route, a in GN.REFUSALS:
        assert GN.call_refused(route, a, 'cpu') == (GN.refusal_code(route, a), True), (name, route)
    _patch(monkeypatch, _HostLib(spill=True))
    for route in GN.ROUTES:
        case = next(c for c in small if c.route == route)
        assert GN.run_on_device(case, 'cpu', GN.inputs(case))['untouched'] is False, route
