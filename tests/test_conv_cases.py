'''CPU checks of tests/conv_cases.py: the generalised gemm_cases.im2col (the loaders' geometry, restated) agrees with
torch.nn.functional.conv2d / the parity formula on every case; `check` accepts the fp32 emulation of every case and rejects fourteen
wrong convolutions wherever they are another computation; every loader and tap order is shown every mutant that can exist on it; the
host-side parity filters of ops.prep_conv_up_phases; the descriptor ranges the packed row states of the loaders can hold; and
gemm_cases.CASES is what it was before the convolution geometry became a parameter.  The tile id and split of a case come from
fd_gemm_plan (host logic only), so the library must be built; no device is needed.'''
import ctypes
import hashlib
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc  # noqa: E402
import gemm_cases as gc  # noqa: E402

LIVE = [c for c in cc.CASES if not gc.refused(c)]
ENVS = ({},) + cc.ENV_SETTINGS


def test_gemm_cases_table_is_unchanged():
    '''Ids, seeds and every field of gemm_cases.CASES, as they were before Case.conv gained padding, upsample2x and an input size.'''
    h = hashlib.sha1()
    for c in gc.CASES:
        h.update(repr(tuple(c)).encode())
    assert (len(gc.CASES), h.hexdigest()) == (493, '5df1a460c5e9bc8f474227518efa8bf8ec1b7ed5')
    for c in gc.CASES:
        if c.conv:      # the defaults mean what they meant
            q = c.geom
            assert (q.pad_t, q.pad_l, q.up, q.hi, q.wi) == ((q.kh - 1) // 2, (q.kw - 1) // 2, 0, q.ho * q.stride, q.wo * q.stride)


def test_the_table_is_what_its_docstring_says():
    assert all(gc.refused(c) == c.id.startswith('refuse-') for c in cc.CASES), [c.id for c in cc.CASES if gc.refused(c) != c.id.startswith('refuse-')]
    by = {}
    for env in ENVS:
        for c in (LIVE if not env else cc.child_cases(env)[0]):
            L = gc.expected_launch(c, env)
            by.setdefault(cc.geometry_of(c), set()).add((L.form, L.tpl[0], c.tile, L.tap_fast))
    assert set(by) == set(cc.GEOMETRIES)
    for name, seen in by.items():
        up = cc.GEOMETRIES[name][5]
        # the one-shot LDS-DMA kernel on a 128-row, a 256-row and the 288-row tile
        assert {bm for form, bm, _, _ in seen if form == 'dma'} >= {128, 256, 288}, name
        if up != 2:     # (upsample2x == 2 has neither a persistent nor a register-staged form)
            assert {'dmap', 'reg'} <= {form for form, _, _, _ in seen}, name
            assert {tf for form, _, _, tf in seen if form == 'dmap'} == {False, True}, name
        assert {tf for form, _, _, tf in seen if form == 'dma'} == {False, True}, name
        pp = {t for form, _, t, _ in seen if form == 'pp'}
        assert pp == (set(cc.PP_TILES) if up != 1 and cc.GEOMETRIES[name][7][1] % 8 == 0 else set()), name
    # variants: two input slices, split-K with slices that start inside a tap and inside an input slice, the two epilogue cases
    ids = {c.id for c in LIVE}
    for t in cc.DMA_TILES + (cc.GENERIC_TILE,):
        assert {f's2-c128-t{t}', f'up-c128-t{t}', f's2-c128-split2-t{t}', f's2-c128-split4-t{t}', f'up-c128-split4-t{t}', f's2-odd-res-t{t}', f's2-odd-bias2-t{t}'} <= ids
    assert {f'ph-c128-t{t}' for t in cc.DMA_TILES + cc.PP_TILES} <= ids and {f'ph-t{t}' for t in gc.LEAN} <= ids and {f'ph-straddle-t{t}' for t in gc.LEAN} <= ids
    c = cc.BY_ID['s2-c128-split4-t13']
    per = gc._cdiv(c.K // 64, 4)
    assert c.K // 64 == 18 and (per * 64) % c.geom.cin != 0 and per % (c.geom.kh * c.geom.kw) != 0       # neither order starts a slice at a tap / slice boundary
    # samples that do not align with tiles, on every tile
    for t in cc.DMA_TILES + (cc.GENERIC_TILE,):
        for name in ('s2-odd', 's2-vae-odd', 'up-odd'):
            assert cc.BY_ID[f'{name}-t{t}'].rps % cc.tile_shape(t)[0] != 0
    for t in tuple(gc.LEAN) + cc.PP_TILES:
        c = cc.BY_ID[f'ph-straddle-t{t}']
        assert c.rps % cc.tile_shape(t)[0] != 0 and c.M % cc.tile_shape(t)[0] == 0
    # what the library cannot run
    assert {'refuse-ph-t1', 'refuse-ph-split2-t13', 'refuse-ph-straddle-ragged-t13'} | {f'refuse-up-t{t}' for t in cc.PP_TILES} | \
        {f'refuse-s2-odd-t{t}' for t in cc.PP_TILES} == {c.id for c in cc.CASES if gc.refused(c)}
    skipped = cc.child_cases({'FD_GEMM_NO_DMA': '1'})[1]
    assert {c.id for c in skipped} == {c.id for c in LIVE if c.tile != cc.GENERIC_TILE and (c.tile in gc.LEAN or c.phase)}
    # re-routed: the phase form stays on the one-shot kernel, the ping-pong tiles take no notice of the switches
    for env in cc.ENV_SETTINGS:
        for c in LIVE:
            if 'FD_GEMM_NO_DMA' not in env and (c.tile in gc.PP or (c.phase and 'FD_GEMM_PERSIST' in env)):
                assert gc.expected_launch(c, env)[:3] == gc.expected_launch(c)[:3]


@pytest.mark.parametrize('case', LIVE, ids=lambda c: c.id)
def test_im2col_agrees_with_conv2d(case):
    '''gemm_cases.im2col + one float64 product against F.conv2d / F.interpolate / F.pad (upsample2x == 2: the parity formula) on the same
    rounded operands, to float64 roundoff (1e-12 relative to the largest output: products of fp16 values are exact in float64, the sums differ
    in order only).'''
    inp = gc.inputs(case)
    mine, want = gc.reference(case, inp)['C'], cc.reference(case, inp)['C']
    assert mine.shape == want.shape and mine.dtype == torch.float64
    assert float((mine - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize('case', LIVE, ids=lambda c: c.id)
def test_check_accepts_the_emulation_and_rejects_every_mutant(case):
    '''`check` (3e-3 + 3e-3 |want| on every element) accepts the fp32 emulation and rejects each wrong convolution that is another
    computation for the case -- the K-order mutants in both tap orders.  No output tile is dead (gemm_cases.tile_liveness).'''
    inp = gc.inputs(case)
    want = cc.reference(case, inp)
    assert gc.tile_liveness(case, want) >= 0.1, f'a tile with only {gc.tile_liveness(case, want):.2f} of its reference above {gc.LIVE_ABS}'
    r = gc.worst(case, cc.emulate(case, inp), want)
    assert r <= 1.0, f'the emulation misses the bound: err / bound = {r:.3f}'
    for mut in cc.MUTANTS:
        for tf in ((False, True) if mut in cc.K_ORDER_MUTANTS else (None,)):
            bad = cc.emulate(case, inp, mut, tf)
            assert (bad is None) == (not cc.applies(case, mut))
            if bad is not None:
                assert not gc.check(case, bad, want), f'{mut} (tap-fastest: {tf}) passes the bound (err / bound = {gc.worst(case, bad, want):.3f})'


def test_a_mutant_that_does_not_apply_is_the_same_computation():
    '''`applies` says no only where the wrong geometry reads the same pixels: the emulation through it gives the same bits.'''
    for cid, mut in (('s2-vae-odd-t13', 'edge_wrap'), ('s2-t10', 'pad_sym'), ('s2-t10', 'pad_swap'), ('s2-t10', 'sample_base')):
        case = cc.BY_ID[cid]
        assert not cc.applies(case, mut)
        assert all(torch.equal(gc.conv_taps(case, z, mut, cc.tile_shape(case.tile)[0]), gc.conv_taps(case, z)) for z in range(case.batch))


def test_the_screen_shows_every_mutant_to_every_loader_and_tap_order():
    '''Every mutant applies to a case that runs on each of the four loaders, the K-order mutants in each tap order of the one-shot
    and the persistent LDS-DMA kernel.  What cannot exist: the fused upsample on the ping-pong kernels (fd_gemm_pp_ok refuses it), the phase form on the
    persistent and the register-staged kernel (no parity row map there); the ping-pong kernels are tap-fastest only, the
    register-staged one slice-fastest only.'''
    seen = {}
    for env in ENVS:
        for c in (LIVE if not env else cc.child_cases(env)[0]):
            L = gc.expected_launch(c, env)
            for m in cc.MUTANTS:
                if cc.applies(c, m):
                    seen.setdefault(m, set()).add((L.form, L.tap_fast))
    for m in cc.MUTANTS:
        forms = {f for f, _ in seen[m]}
        want = {'dma', 'pp'} if m.startswith('phase_') else {'dma', 'dmap', 'reg'} if m.startswith('up_') else {'dma', 'dmap', 'reg', 'pp'}
        assert forms == want, (m, forms)
    for m in cc.K_ORDER_MUTANTS:
        assert {('dma', False), ('dma', True), ('dmap', False), ('dmap', True), ('reg', False), ('pp', True)} <= seen[m], (m, seen[m])


# ------------------------------------------------------------------------------------------------ the host-side parity filters
def test_parity_filters_are_the_tap_sums_rounded_once():
    '''ops.prep_conv_up_phases: (1) the float64 sums of the 3x3 taps that land on the same source pixel, put through the parity formula, are
    interpolate(nearest 2x) + conv3x3 -- on an odd non-square input, to float64 roundoff; (2) the stored fp16 filters are those sums rounded
    once: |err| <= 2^-11 |s| (one fp16 rounding) + 3 x 2^-24 sum |taps| (fp32 addition of at most four taps) + 2^-25 (the fp16 subnormal step).'''
    from flexdiffuse_amd import ops
    g = torch.Generator().manual_seed(7)
    cout, cin, H, W = 24, 64, 5, 7
    w = torch.randn((cout, cin, 3, 3), generator=g) * (9 * cin) ** -0.5
    w[0] *= 2.0 ** -14                # into the fp16 subnormals
    b = torch.randn(cout, generator=g)
    cw = ops.prep_conv_up_phases(w, b, 'cpu')
    assert cw.w.shape == (4, cout, 4 * cin) and cw.w.dtype == torch.float16 and (cw.kh, cw.kw, cw.cin, cw.cout) == (2, 2, cin, cout)
    w64 = w.double()
    groups = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}      # parity -> the 3x3 rows (columns) behind window position 0 and 1
    s = torch.zeros((4, cout, 2, 2, cin), dtype=torch.float64)
    sabs = torch.zeros_like(s)
    for py in (0, 1):
        for px in (0, 1):
            for a in (0, 1):
                for c in (0, 1):
                    for i in groups[py][a]:
                        for j in groups[px][c]:
                            s[2 * py + px, :, a, c] += w64[:, :, i, j]
                            sabs[2 * py + px, :, a, c] += w64[:, :, i, j].abs()
    x = torch.randn((2, cin, H, W), generator=g).double()
    want = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w64, b.double(), padding=1).permute(0, 2, 3, 1)
    case = gc.Case('filters', 0, 2 * H * W, cout, 4 * cin, conv=(H, W, cin, 2, 2, 1, 1, 1, 2, H, W), batch=4, rps=H * W)
    got = cc.phase_reference(case, {'A': x.permute(0, 2, 3, 1)[None], 'W': s.reshape(4, cout, 4 * cin), 'bias': b[None]}).reshape(want.shape)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    err = (cw.w.double().reshape(s.shape) - s).abs()
    bound = 2.0 ** -11 * s.abs() + 3 * 2.0 ** -24 * sabs + 2.0 ** -25
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) > 0.0     # (fp16 filters: the rounding is there)


# ------------------------------------------------------------------------------------------------ the ranges of the packed row states
def _plan_rc(case, **over):
    from flexdiffuse_amd import hip
    fake = {n: 0x10000000 + 0x1000000 * i for i, n in enumerate(('A', 'W', 'C', 'bias', 'bias2', 'res', 'ws'))}
    d = gc.build_desc(case, gc.layout_plan(case), fake)
    for k, v in over.items():
        setattr(d, k, v)
    tile, split = ctypes.c_int(0), ctypes.c_int(0)
    return hip.lib().fd_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(split))


def test_the_abi_refuses_geometry_outside_the_packed_row_states():
    '''The LDS-DMA loaders keep (y + 16) << 16 | (x + 16) per row, the ping-pong loader (y + 0x4000) << 16 | (x + 0x4000) per DMA group:
    fd_gemm_f16 refuses (FD_ESHAPE, before any launch) a stride, filter, padding or upsample2x those cannot hold, and accepts the edge.'''
    FD_ESHAPE = -2
    case = cc.BY_ID['s2-t13']
    assert _plan_rc(case) == 0
    for over in ({'stride': 0}, {'stride': -1}, {'pad_t': 17}, {'pad_l': 17}, {'pad_t': -1}, {'pad_l': -1}, {'upsample2x': 3}, {'upsample2x': -1},
                 {'kh': -3, 'kw': -3}, {'in_h': 0}, {'in_w': 0x4000 + 1}, {'stride': 0x4000}):
        assert _plan_rc(case, **over) == FD_ESHAPE, over
    assert _plan_rc(case, pad_t=16, pad_l=16) == 0
    assert _plan_rc(cc.BY_ID['s2-t13']) == 0      # a good call after the refusals
