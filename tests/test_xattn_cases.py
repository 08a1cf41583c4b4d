'''CPU checks of tests/xattn_cases.py: the table covers every form it promises (one named assertion each, so that deleting the only
case of a kind fails by name), the acceptance criterion accepts an fp32 emulation of k_xattn at no more than half the bound while
rejecting twelve wrong computations on every case they apply to, the restated image layouts place every (key, channel) exactly once,
and the GPU test's own driver runs against a host stand-in of the three library calls.'''
import ctypes
import os

import pytest
import torch

import xattn_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (40, 80)


def _of(d, **kw):
    return [c for c in X.CASES if c.d == d and all(getattr(c, n) == v for n, v in kw.items())]


# --------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('d', DIMS)
def test_table_covers_what_it_promises(d):
    bm = X.row_tile(d)
    cases = _of(d)
    assert bm == {40: 256, 80: 128}[d] and all(c.HW % bm == 0 and 65 <= c.L <= 80 for c in cases)
    for L in range(65, 81):
        assert _of(d, L=L), f'no case with {L} keys at head dim {d}'
    for tiles in (1, 3, 8, 9):
        assert [c for c in cases if c.tiles == tiles], f'no case with {tiles} row tiles at head dim {d}'
    assert [c for c in cases if c.tiles >= 16 and c.tiles % 8 >= 2], f'no grid of 8q + r tiles, q >= 2, r >= 2, at head dim {d}'
    assert [c for c in cases if c.HW == bm and c.B >= 3], f'no case whose every tile is another sample at head dim {d}'
    assert [c for c in cases if c.HW == 3 * bm and c.B >= 2], f'no case with sample borders every third tile at head dim {d}'
    for rep in (1, 2, 3):
        assert _of(d, rep=rep), f'no case with {rep} replicas at head dim {d}'
    assert [c for c in cases if c.rep >= 2 and c.B >= 2], f'replica index and sample index never select the image together at head dim {d}'
    for layout in X.LAYOUTS:
        assert _of(d, layout=layout), f'no {layout} case at head dim {d}'
    # sample strides with gaps are read only with a second context; the part of the buffer behind the last replica needs one
    assert [c for c in _of(d, layout='padded_ld') if c.B >= 2], f'no padded_ld case with two samples at head dim {d}'
    assert [c for c in _of(d, layout='out_slice') if c.rep >= 2], f'no out_slice case with replicas at head dim {d}'
    assert _of(d, stats='fin'), f'no finished-statistics case at head dim {d}'
    for parts in (2, 4, 8):
        assert _of(d, stats=parts, eps=0.0), f'no {parts}-part case with the default eps at head dim {d}'
        assert _of(d, stats=parts, eps=1e-3), f'no {parts}-part case with eps 1e-3 at head dim {d}'
    assert max(c.rep * c.M * c.C for c in cases) <= 5120 * 640


def test_parts_cases_hold_a_low_variance_row_and_a_constant_row():
    for c in X.CASES:
        if c.stats == 'fin':
            continue
        x = X.inputs(c)['x16'].double()
        var = x.var(1, unbiased=False)
        assert 0.3 * c.eff_eps <= float(var[X.LOW_VAR_ROW]) <= 3 * c.eff_eps, (c.id, float(var[X.LOW_VAR_ROW]))
        assert float(var[X.CONST_ROW]) == 0.0 and float(x[X.CONST_ROW, 0]) != 0.0, c.id
        assert float(var.sort().values[2]) > 100 * c.eff_eps, c.id      # every other row is far above eps


def test_inputs_are_what_the_docstring_says():
    c = next(c for c in X.CASES if c.rep >= 2 and c.B >= 2)
    inp = X.inputs(c)
    k = inp['k16'].double()
    norm = k.norm(dim=-1)                                   # [contexts][keys]
    assert int(norm[0].argmax()) == X.spike_key(c) and float(norm[0].max()) > 4 * float(norm[0].median())
    assert float(norm[-1].max()) < 0.1 * float(norm[1].median())
    assert float(inp['v16'].double().mean((0, 1)).abs().max()) > 1.0       # the per-channel offset of V
    assert inp['stats'].dtype == torch.float32 and inp['bias'].dtype == torch.float32 and inp['colsum'].dtype == torch.float32
    assert inp['w16'].shape == (c.C, c.C) and inp['k16'].shape == (c.n_ctx, c.L, c.C)
    # every context is its own
    flat = inp['k16'].reshape(c.n_ctx, -1)
    assert all(not torch.equal(flat[i], flat[j]) for i in range(c.n_ctx) for j in range(i))


def test_remap_restates_the_source_and_is_a_permutation():
    with open(os.path.join(ROOT, 'flexdiffuse_amd', 'csrc', 'xattn.hip'), encoding='utf-8') as f:
        src = f.read()
    assert 'tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;' in src
    assert 'const int nb = gridDim.x, q = nb >> 3, r = nb & 7, xcd = tile & 7, slot = tile >> 3;' in src
    for nb in range(1, 41):
        assert sorted(X.remap(nb, b) for b in range(nb)) == list(range(nb)), nb
        assert (X.confused_tiles(nb) is None) == (nb % 8 == 0 or nb == 1), nb
    assert all(X.remap(nb, b) == b for nb in (1, 3, 8) for b in range(nb))           # identity
    assert [X.remap(16, b) for b in range(16)] == [2 * (b & 7) + (b >> 3) for b in range(16)]   # a plain transpose
    assert [X.remap(9, b) for b in range(9)] == [0, 2, 3, 4, 5, 6, 7, 8, 1]
    assert X.confused_tiles(9) == (2, 1) and X.confused_tiles(20) == (3, 2) and X.confused_tiles(3) == (1, 0)


def test_layouts_are_what_their_tags_say():
    for c in X.CASES:
        p, C = X.layout_plan(c), c.C
        assert p['ldx'] % 8 == 0 and p['ldw'] % 8 == 0 and p['ldo'] % 4 == 0 and p['x_off'] % 8 == 0 and p['o_off'] % 4 == 0
        if c.layout == 'padded_ld':
            assert (p['ldx'], p['ldw'], p['ldo'], p['ldk']) == (C + 8, C + 8, C + 4, C + 8) and p['ldvt'] > X._round8(c.L)
            assert p['sK'] > c.L * p['ldk'] and p['sVt'] > C * p['ldvt']
        if c.layout == 'out_slice':
            assert p['o_off'] == p['o_tail'] == X.GUARD_ROWS * C and p['ldx'] > C and p['x_off'] > 0
        # the last element each view reaches lies inside its buffer
        assert p['x_off'] + (c.M - 1) * p['ldx'] + C <= p['x_size'] and (C - 1) * p['ldw'] + C <= p['w_size']
        assert (c.n_ctx - 1) * p['sK'] + (c.L - 1) * p['ldk'] + C <= p['k_size']
        assert (c.n_ctx - 1) * p['sVt'] + (C - 1) * p['ldvt'] + c.L <= p['vt_size']
        assert p['o_off'] + (c.rep * c.M - 1) * p['ldo'] + C + p['o_tail'] <= p['o_size']
    c = next(c for c in X.CASES if c.layout == 'padded_ld' and c.B >= 2)
    inp = X.inputs(c)
    host, p = X.host_buffers(c, inp), X.layout_plan(c)
    k = torch.as_strided(host['k'], (c.n_ctx, c.L + 3, p['ldk']), (p['sK'], p['ldk'], 1), 0)
    assert torch.equal(k[:, :c.L, :c.C], inp['k16']) and bool((k[:, c.L:] == X.PAD_IN).all()) and bool((k[:, :, c.C:] == X.PAD_IN).all())
    vt = torch.as_strided(host['vt'], (c.n_ctx, c.C, p['ldvt']), (p['sVt'], p['ldvt'], 1), 0)
    assert torch.equal(vt[:, :, :c.L], inp['v16'].transpose(1, 2)) and bool((vt[:, :, c.L:] == X.JUNK).all())
    x = torch.as_strided(host['x'], (c.M, p['ldx']), (p['ldx'], 1), 0)
    assert torch.equal(x[:, :c.C], inp['x16']) and bool((x[:, c.C:] == X.PAD_IN).all())


# --------------------------------------------------------------------------------------------------- the criterion
@pytest.fixture(scope='module')
def screen():
    '''case id -> (worst ratio of the fp32 emulation, {mutant: worst ratio, for the mutants that apply}).'''
    out = {}
    for case in X.CASES:
        inp = X.inputs(case)
        want = X.reference(case, inp)
        assert want.shape == (case.rep * case.M, case.C) and bool(torch.isfinite(want).all())
        good = X.emulate(case, inp)
        assert X.check(good, want) == (X.worst(good, want) <= 1.0)
        bad = {m: X.attend(case, inp, torch.float64, m) for m in X.MUTANTS}
        assert all((b is not None) == X.applies(case, m) for m, b in bad.items())
        out[case.id] = (X.worst(good, want), {m: X.worst(b, want) for m, b in bad.items() if b is not None})
    return out


@pytest.mark.parametrize('case', X.CASES, ids=[c.id for c in X.CASES])
def test_check_accepts_the_emulation_at_half_the_bound_and_rejects_every_mutant(screen, case):
    good, mutants = screen[case.id]
    assert good <= 0.5, f'the fp32 emulation reaches {good:.3g} x the bound'
    for mutant, ratio in mutants.items():
        assert ratio > 1.0, f'{mutant} passes the bound ({ratio:.3g} x) at {case.id}'


def test_every_mutant_applies_to_three_cases_and_to_each_template_it_can(screen):
    for m in X.MUTANTS:
        hit = [c for c in X.CASES if m in screen[c.id][1]]
        assert len(hit) >= 3, (m, [c.id for c in hit])
        dims = {c.d for c in hit}
        assert dims == {'cross_talk': {40}, 'swap_ntiles': {80}}.get(m, {40, 80}), (m, dims)
    assert not X.applies(next(c for c in X.CASES if c.L == 80), 'pad_keys')
    assert X.applies(next(c for c in X.CASES if c.L == 79), 'pad_keys')


def test_unrounded_q_is_a_worse_reference_on_the_spiked_context():
    '''Why the reference rounds Q: with Q left in float64 the same emulation sits several times closer to the bound.'''
    case = next(c for c in X.CASES if c.tiles == 1 and c.rep == 1 and c.stats == 'fin')
    inp = X.inputs(case)
    good = X.emulate(case, inp)
    rounded = X.worst(good, X.reference(case, inp))
    unrounded = X.worst(good, X.attend(case, inp, torch.float64, round_q=False))
    print(f'{case.id}: emulation / bound = {rounded:.3f} against the rounded-Q reference, {unrounded:.3f} against the unrounded one')
    assert unrounded > 2 * rounded


# --------------------------------------------------------------------------------------------------- the images
@pytest.mark.parametrize('d', DIMS)
@pytest.mark.parametrize('L', (1, 16, 64, 65, 77, 80))
def test_image_restatement_places_every_element_once(L, d):
    C = X.HEADS * d
    # all-distinct nonzero fp16 bit patterns, the ones-row's 1.0 left out (L C <= 51200 of them; K in rising, V in falling order)
    bits = torch.arange(1, L * C + 2, dtype=torch.int32)
    bits = bits[bits != X.ONE_BITS][:L * C].to(torch.int16)
    k16, v16 = bits.view(1, L, C).view(torch.float16), bits.flip(0).view(1, L, C).view(torch.float16)
    kimg, vimg = X.pack_images(k16, v16, d)
    kh, vh = kimg.view(X.HEADS, -1), vimg.view(X.HEADS, -1)
    kb, vb = k16.view(torch.int16)[0], v16.view(torch.int16)[0]
    for h in range(X.HEADS):
        nz = kh[h][kh[h] != 0]
        assert sorted(nz.tolist()) == sorted(kb[:, h * d:(h + 1) * d].flatten().tolist()), (h, 'K')
        nz = vh[h][vh[h] != 0]
        ones = [X.ONE_BITS] * L if d == 40 else []
        assert sorted(nz.tolist()) == sorted(vb[:, h * d:(h + 1) * d].flatten().tolist() + ones), (h, 'V^T')
        # where they sit: K key slot kb * 16 + fr at lane (fr, fq); the ones-row is row 40 = d-tile 2, fr 8
        key, ch = X._k_map(d, bool(h & 1))
        real = (ch >= 0) & (key < L)
        assert torch.equal(kh[h][real], kb[:, h * d:(h + 1) * d][key[real], ch[real]]) and int((kh[h][~real] != 0).sum()) == 0
        row, key = X._v_map(d)
        if d == 40:
            assert bool((vh[h][(row == 40) & (key < L)] == X.ONE_BITS).all()) and int(((row == 40) & (key < L)).sum()) == L
            assert int((vh[h][(row > 40) | (key >= L)] != 0).sum()) == 0
        else:
            assert int(row.max()) == 79 and int((vh[h][key >= L] != 0).sum()) == 0
    # at head dim 40 a pair's tails are complementary: no lane slot of the shared fragment is claimed by both heads
    if d == 40:
        _, a = X._k_map(40, False)
        _, b = X._k_map(40, True)
        tail = torch.arange(a.numel()) % 768 >= 512
        assert int(((a >= 0) & (b >= 0) & tail).sum()) == 0 and bool(((a >= 0) | (b >= 0))[tail].all())
        assert sorted(a[tail & (a >= 0)].unique().tolist()) == list(range(32, 40)) and sorted(b[tail & (b >= 0)].unique().tolist()) == list(range(8))
    assert kimg.numel() * 2 == X.IMAGE_BYTES[d] == vimg.numel() * 2


# --------------------------------------------------------------------------------------------------- the driver
def _mem(ptr, n, dtype):
    size = torch.empty((), dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_uint8 * (n * size)).from_address(ptr), dtype=dtype)


def _unpack(kimg, vimg, L, d):
    '''The inverse of X.pack_images for one context: K, V [L][8 d] as int16 bit patterns.'''
    k, v = torch.zeros((X.KEY_SLOTS, X.HEADS * d), dtype=torch.int16), torch.zeros((X.KEY_SLOTS, X.HEADS * d), dtype=torch.int16)
    kh, vh = kimg.view(X.HEADS, -1), vimg.view(X.HEADS, -1)
    for h in range(X.HEADS):
        key, ch = X._k_map(d, bool(h & 1))
        k[key[ch >= 0], h * d + ch[ch >= 0]] = kh[h][ch >= 0]
        row, key = X._v_map(d)
        v[key[row < d], h * d + row[row < d]] = vh[h][row < d]
    return k[:L], v[:L]


def _stand_in(name, *a):
    '''The three library calls as plain torch on the HOST memory their arguments point at: fd_xattn_pack_kv_f16 by the restated
    layouts, fd_ln_finalize_stats_f32 and fd_xattn_q_f16 by the fp32 emulation -- an honest kernel for the GPU test's own driver.'''
    if name == 'fd_xattn_pack_kv_f16':
        K, Vt, kimg, vimg, n, L, heads, d, ldk, ldvt, sK, sVt, _ = a
        C = heads * d
        k = torch.as_strided(_mem(K, (n - 1) * sK + (L - 1) * ldk + C, torch.float16), (n, L, C), (sK, ldk, 1))
        vt = torch.as_strided(_mem(Vt, (n - 1) * sVt + (C - 1) * ldvt + L, torch.float16), (n, C, L), (sVt, ldvt, 1))
        ki, vi = X.pack_images(k.contiguous(), vt.transpose(1, 2).contiguous(), d)
        _mem(kimg, ki.numel(), torch.int16).copy_(ki.flatten())
        _mem(vimg, vi.numel(), torch.int16).copy_(vi.flatten())
        return
    if name == 'fd_ln_finalize_stats_f32':
        parts, out, M, N, k, eps, _ = a
        case = X.Case(1, M, 1, 77, N // X.HEADS, 'contig', k, eps)
        rstd, mr = X.finalize(case, _mem(parts, k * M * 2, torch.float32).view(k, M, 2), torch.float32)
        _mem(out, M * 2, torch.float32).view(M, 2).copy_(torch.stack([rstd, mr], -1))
        return
    assert name == 'fd_xattn_q_f16'
    d = a[0]._obj
    C, M, L, hd = d.heads * d.head_dim, d.M, d.n_keys, d.head_dim
    case = X.Case(M // d.rows_per_sample, d.rows_per_sample, d.n_rep, L, hd, 'contig', d.ln_stats_parts or 'fin', d.ln_fold_eps)
    half = X.IMAGE_BYTES[hd] // 2
    ctx = [_unpack(_mem(d.k_image + 2 * half * i, half, torch.int16), _mem(d.v_image + 2 * half * i, half, torch.int16), L, hd)
           for i in range(case.n_ctx)]
    inp = {'x16': torch.as_strided(_mem(d.x, (M - 1) * d.ldx + C, torch.float16), (M, C), (d.ldx, 1)),
           'w16': torch.as_strided(_mem(d.wq, (C - 1) * d.ldw + C, torch.float16), (C, C), (d.ldw, 1)),
           'bias': _mem(d.bias, C, torch.float32), 'colsum': _mem(d.ln_colsum, C, torch.float32),
           'stats': _mem(d.ln_stats, max(d.ln_stats_parts, 1) * M * 2, torch.float32).view(*((d.ln_stats_parts,) if d.ln_stats_parts else ()), M, 2),
           'k16': torch.stack([k for k, _ in ctx]).view(torch.float16), 'v16': torch.stack([v for _, v in ctx]).view(torch.float16)}
    rows = d.n_rep * M
    torch.as_strided(_mem(d.out, (rows - 1) * d.ldo + C, torch.float16), (rows, C), (d.ldo, 1)).copy_(X.emulate(case, inp))


def test_device_driver_against_a_host_stand_in(monkeypatch):
    '''run_on_device with the library replaced by the stand-in above: every layout and statistics form hands the kernel the operands
    the reference sees, reads the output and the images back from where they were written and notices a write outside the output.'''
    from flexdiffuse_amd import hip
    monkeypatch.setattr(hip, 'call', _stand_in)
    monkeypatch.setattr(hip, 'stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    small = [c for c in X.CASES if c.tiles <= 3 and c.d == 40] + [c for c in X.CASES if c.tiles in (1, 9) and c.d == 80]
    assert {c.layout for c in small} == set(X.LAYOUTS) and {c.stats for c in small} == set(X.STATS) and any(c.rep == 3 for c in small)
    for case in small:
        inp = X.inputs(case)
        r = X.run_on_device(case, 'cpu', inp)
        ki, vi = X.image_reference(case, inp)
        assert r.untouched and X.worst(r.out, X.reference(case, inp)) <= 0.5, case.id
        assert torch.equal(r.kimg, ki) and torch.equal(r.vimg, vi) and torch.equal(r.out, r.again), case.id
        assert (r.fin is None) == (case.stats == 'fin') and (r.fin is None or torch.equal(r.fin, r.out)), case.id

    def spill(name, *a):      # one element behind the last output row
        _stand_in(name, *a)
        if name == 'fd_xattn_q_f16':
            d = a[0]._obj
            ctypes.c_uint16.from_address(d.out + 2 * ((d.n_rep * d.M - 1) * d.ldo + d.heads * d.head_dim)).value = 0

    monkeypatch.setattr(hip, 'call', spill)
    for layout in ('padded_ld', 'out_slice'):
        case = next(c for c in small if c.layout == layout)
        assert X.run_on_device(case, 'cpu').untouched is False, layout
