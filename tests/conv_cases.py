'''The geometry table of the implicit-GEMM convolution: fd_gemm_f16 in convolution mode on every geometry the UNet and the VAE use, on
every loader that turns a GEMM row into input pixels -- k_gemm_f16_dma (one-shot LDS-DMA), k_gemm_f16_dmap (persistent), k_gemm_f16
(register-staged) of csrc/gemm.hip and k_gemm_f16_pp (ping-pong tiles 30..33) of csrc/gemm_pp.hip --, in both tap orders, with the parity
row map of the lean epilogue (csrc/gemm_epilogue.h) for upsample2x == 2.  Built on tests/gemm_cases.py (`G`): its Case, layout_plan,
build_desc, host_buffers, sentinels and guard rows, tolerance / worst / check, run_on_device / run_and_score and --child entry.  Shared by
tests/test_conv_cases.py (CPU) and tests/test_gpu_conv_cases.py (MI355X).  Nothing here needs a GPU to import.

The reference is float64 on the fp16-rounded operands and does not go through the table's own im2col: torch.nn.functional.conv2d on the
NCHW view, F.interpolate(mode='nearest') in front of it for upsample2x == 1, F.pad for the one-sided padding; for upsample2x == 2 the
formula out[b, 2y+py, 2x+px] = sum_{a,c in {0,1}} X[b, y-1+py+a, x-1+px+c] . W[2py+px][:, a, c, :] with zeros outside the image.
tests/test_conv_cases.py holds gemm_cases.im2col (the restated loader geometry, `G.conv_taps`, that the mutants bend) against it.

GEOMETRIES (Cin = 64, K = kh kw Cin; `-c128`: Cin = 128, two input slices, so that the slice-fastest and the tap-fastest K order differ)
  s2           3x3, stride 2, pad (1,1)            16x32 -> 8x16    UNet downsample; Wo % 8 == 0
  s2-odd       3x3, stride 2, pad (1,1)            15x17 -> 8x9     odd input; 72 rows per sample: every tile straddles samples
  s2-vae       3x3, stride 2, pad (0,0), out=in//2 16x32 -> 8x16    bottom / right zeros from the bounds test alone
  s2-vae-odd   3x3, stride 2, pad (0,0), out=in//2 15x33 -> 7x16    the last tap column lies inside the image; 112 rows per sample
  k1x3-s2      1x3, stride 2, pad (0,1)            16x32 -> 8x16    pad_t != pad_l
  up           3x3, stride 1, pad 1, upsample2x=1  4x8   -> 8x16    fused nearest upsample
  up-odd       3x3, stride 1, pad 1, upsample2x=1  5x6   -> 10x12   120 rows per sample
  ph           upsample2x=2, batch 4, 2x2 filters  8x16 low-res     phase form, non-square
  ph-straddle  upsample2x=2, batch 4, 2x2 filters  6x16 low-res     96 rows per sample: a tile (ping-pong: a DMA group's row) crosses samples
  variants: -c128 of s2, up, ph; -c128-split2 / -split4 of s2 and up (18 K-tiles: split 4 starts slices inside a tap and inside an input
  slice); -res and -bias2 (per sample) of s2-odd; -ragged (M % BM != 0: generic epilogue, rows past M) of s2-odd and up-odd.
  M = B x rows per sample with the smallest B that gives whole tiles (at least two); N = two tile widths (one from 256 columns on).

RUN (tile ids: 10 = 128x128, 13 = 256x160, 23 = 288x160, 16 = 256x320 lean tiles; 1 = 128x128 generic tile; 30..33 ping-pong)
  one-shot LDS-DMA     every geometry and variant on tiles 10, 13, 23, 16, 1 (phase: not 1); ph and ph-straddle on all nine lean tiles
  persistent           FD_GEMM_PERSIST=2: every non-phase case of tiles 10, 13, 23 and 1 again (tile 16 has no persistent form)
  register-staged      FD_GEMM_NO_DMA=1: every non-phase case of tile 1 again
  ping-pong            tiles 30..33: s2, s2-vae, s2-vae-odd, k1x3-s2, ph, ph-straddle, s2-c128 (+ split 2 / 4), ph-c128
  tap order            slice-fastest by default, tap-fastest on tile 16 and the ping-pong tiles; FD_CONV_TAPFAST=0 runs tile 16
                       slice-fastest, FD_CONV_TAPFAST=2 runs tiles 10, 13, 23, 1 (phase: all nine) tap-fastest, FD_GEMM_PERSIST=2 with
                       FD_CONV_TAPFAST=2 the persistent kernel tap-fastest (the register-staged kernel is slice-fastest only)
REFUSED (ValueError / FD_ESHAPE before any launch, each followed by a good call)
  upsample2x == 2 on a generic tile, with split-K, with M % BM != 0 (gemm_check_tile); under FD_GEMM_NO_DMA (gemm_check: the parity row
  map exists in the lean epilogue of the LDS-DMA path only); upsample2x == 1 and Wo % 8 != 0 on a ping-pong tile (fd_gemm_pp_ok);
  every lean tile (8 waves or more) under FD_GEMM_NO_DMA (launch_mode: no register-staged form)
RE-ROUTED (predicted by `G.expected_launch`)
  upsample2x == 2 under FD_GEMM_PERSIST=2 stays on the one-shot kernel (launch_mode's predicate); a per-sample bias whose samples
  do not align with the tiles, and every ragged M, run the generic epilogue; the ping-pong tiles take no notice of the three switches.
NOT HERE: the explicit-im2col path and fd_conv3x3_narrow_f16 (tests/test_gpu_layout_cases.py), tile 26, the epilogue matrix (gemm_cases).'''
from __future__ import annotations

import json
import os
import sys
from math import gcd
from typing import Optional

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as G  # noqa: E402
from gemm_cases import Case  # noqa: E402

# the arms of G.ENV_SETTINGS that change a loader or its K order, and the two of them that meet in the persistent kernel walking tap-fastest
ENV_SETTINGS = tuple(e for e in G.ENV_SETTINGS if e in ({'FD_GEMM_PERSIST': '2'}, {'FD_GEMM_NO_DMA': '1'}, {'FD_CONV_TAPFAST': '0'}, {'FD_CONV_TAPFAST': '2'})) + \
    ({'FD_GEMM_PERSIST': '2', 'FD_CONV_TAPFAST': '2'},)
assert len(ENV_SETTINGS) == 5

# name: (kh, kw, stride, pad_t, pad_l, upsample2x, (in_h, in_w), (out_h, out_w))
GEOMETRIES = {
    's2': (3, 3, 2, 1, 1, 0, (16, 32), (8, 16)),
    's2-odd': (3, 3, 2, 1, 1, 0, (15, 17), (8, 9)),
    's2-vae': (3, 3, 2, 0, 0, 0, (16, 32), (8, 16)),
    's2-vae-odd': (3, 3, 2, 0, 0, 0, (15, 33), (7, 16)),
    'k1x3-s2': (1, 3, 2, 0, 1, 0, (16, 32), (8, 16)),
    'up': (3, 3, 1, 1, 1, 1, (4, 8), (8, 16)),
    'up-odd': (3, 3, 1, 1, 1, 1, (5, 6), (10, 12)),
    'ph': (2, 2, 1, 1, 1, 2, (8, 16), (8, 16)),
    'ph-straddle': (2, 2, 1, 1, 1, 2, (6, 16), (6, 16)),
}
DMA_TILES = (10, 13, 23, 16)
GENERIC_TILE = 1
PP_TILES = tuple(sorted(G.PP))


def tile_shape(tile: int):
    return (G.LEAN.get(tile) or G.GENERIC.get(tile) or G.PP[tile])[:2]


def _conv(name: str, cin: int) -> tuple:
    kh, kw, stride, pt, pl, up, (hi, wi), (ho, wo) = GEOMETRIES[name]
    return (ho, wo, cin, kh, kw, stride, pt, pl, up, hi, wi)


def _case(name: str, tile: int, cin: int = 64, ragged: bool = False, cid: Optional[str] = None, **kw) -> Case:
    '''The case of geometry `name` on `tile`: whole tiles, at least two tile rows (ragged: one sample less), one or two tile columns.'''
    conv = _conv(name, cin)
    rows, (bm, bn) = conv[0] * conv[1], tile_shape(tile)
    B = bm // gcd(rows, bm)
    while B * rows < 2 * bm:
        B *= 2
    B -= 1 if ragged else 0
    return Case(cid or f'{name}-t{tile}', tile, B * rows, 2 * bn if bn <= 160 else bn, conv[3] * conv[4] * cin, conv=conv, batch=4 if conv[8] == 2 else 1,
                rps=rows, **kw)


def _build_table():
    T = []

    def add(name, tile, suffix='', prefix='', **kw):
        lay = 'padded' if (len(T) + tile) % 2 else 'contig'
        T.append(_case(name, tile, cid=f'{prefix}{name}{suffix}-t{tile}', layout=lay, **kw))

    for name, q in GEOMETRIES.items():
        phase, up = q[5] == 2, q[5] == 1
        pp_ok = not up and q[7][1] % 8 == 0
        tiles = (tuple(G.LEAN) if phase else DMA_TILES + (GENERIC_TILE,)) + (PP_TILES if pp_ok else ())
        for t in tiles:
            add(name, t)
        short = tuple(t for t in DMA_TILES + (GENERIC_TILE,) + PP_TILES if (t != GENERIC_TILE or not phase) and (pp_ok or t not in G.PP))
        if name in ('s2', 'up', 'ph'):
            for t in short:
                add(name, t, '-c128', cin=128)
        if name in ('s2', 'up'):
            for t in short:
                for split in (2, 4):
                    add(name, t, f'-c128-split{split}', cin=128, split=split)
        if name == 's2-odd':
            for t in short:
                add(name, t, '-res', res=True)
                add(name, t, '-bias2', bias2=True)
        if name in ('s2-odd', 'up-odd'):
            for t in short:
                add(name, t, '-ragged', ragged=True)
    # ---- refused: each is followed by a good call in the GPU test ----
    add('ph', GENERIC_TILE, prefix='refuse-')                         # no lean epilogue, no parity row map
    add('ph', 13, '-split2', 'refuse-', split=2)
    add('ph-straddle', 13, '-ragged', 'refuse-', ragged=True)         # M % BM != 0
    for t in PP_TILES:
        add('up', t, prefix='refuse-')                                # per-lane x >> 1
        add('s2-odd', t, prefix='refuse-')                            # Wo = 9: a DMA group is 8 consecutive pixels of one output row
    return T


CASES = tuple(c._replace(seed=500 + i) for i, c in enumerate(_build_table()))
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), 'case ids must be unique'


def geometry_of(case: Case) -> str:
    cid = case.id[len('refuse-'):] if case.id.startswith('refuse-') else case.id
    return max((n for n in GEOMETRIES if cid == n or cid.startswith(n + '-')), key=len)


def child_cases(env: dict):
    return G.child_cases(env, CASES)


# ------------------------------------------------------------------------------------------------ the reference
def conv_acc(case: Case, inp: dict, z: int = 0):
    '''float64 [M][N]: F.conv2d on the NCHW view of the rounded operands (no bias).'''
    q = case.geom
    x = inp['A'][z].double().permute(0, 3, 1, 2)
    w = inp['W'][z].double().reshape(case.N, q.kh, q.kw, q.cin).permute(0, 3, 1, 2)
    if q.up == 1:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    bottom = max((q.ho - 1) * q.stride + q.kh - q.pad_t - x.shape[2], 0)
    right = max((q.wo - 1) * q.stride + q.kw - q.pad_l - x.shape[3], 0)
    y = F.conv2d(F.pad(x, (q.pad_l, right, q.pad_t, bottom)), w, stride=q.stride)[:, :, :q.ho, :q.wo]
    assert y.shape[2:] == (q.ho, q.wo)
    return y.permute(0, 2, 3, 1).reshape(case.M, case.N)


def phase_reference(case: Case, inp: dict):
    '''out[b, 2y+py, 2x+px] = sum_{a,c} X[b, y-1+py+a, x-1+px+c] . W[2py+px][:, a, c, :] + bias, zeros outside the image -> [1][4 M][N].'''
    q = case.geom
    x = F.pad(inp['A'][0].double(), (0, 0, 1, 1, 1, 1))                           # [B][Hi + 2][Wi + 2][Cin]: X[b, y - 1, x - 1] = x[b, y, x]
    out = torch.zeros((x.shape[0], 2 * q.hi, 2 * q.wi, case.N), dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            w = inp['W'][2 * py + px].double().reshape(case.N, 2, 2, q.cin)
            for a in (0, 1):
                for c in (0, 1):
                    out[:, py::2, px::2] += torch.einsum('byxk,nk->byxn', x[:, py + a:py + a + q.hi, px + c:px + c + q.wi], w[:, a, c])
    return (out + inp['bias'][0].double()).reshape(1, 4 * case.M, case.N)


def reference(case: Case, inp: Optional[dict] = None) -> dict:
    inp = inp if inp is not None else G.inputs(case)
    if case.phase:
        return {'C': phase_reference(case, inp)}
    return G.compute(case, inp, torch.float64, acc_of=lambda z: conv_acc(case, inp, z))


# ------------------------------------------------------------------------------------------------ wrong convolutions
GEOMETRY_MUTANTS = ('edge_wrap', 'pad_sym', 'pad_swap', 'hw_swap', 'stride_one', 'up_ceil', 'up_bounds_low', 'sample_base', 'tap_transpose', 'phase_pad')
K_ORDER_MUTANTS = ('slice_order', 'splitk_restart')
STORE_MUTANTS = ('phase_parity_swap', 'phase_row_pitch')
MUTANTS = GEOMETRY_MUTANTS[:-1] + K_ORDER_MUTANTS + ('phase_parity_swap', 'phase_pad', 'phase_row_pitch')


def _k_blocks(case: Case, mutant: str, tap_fast: bool):
    '''The 64-wide column block of the im2col matrix (columns in (tap, Cin) order) that A contributes to each K-tile of the wrong kernel,
    and the one W contributes.  The K loop visits block tap * slices + slice; tap-fastest: K-tile kt is (tap, slice) = (kt % taps,
    kt // taps); slice-fastest: (kt // slices, kt % slices).  A correct kernel multiplies equal blocks, each once.'''
    q = case.geom
    taps, slices = q.kh * q.kw, q.cin // G.BK
    nkt = taps * slices
    block = (lambda kt: (kt % taps) * slices + kt // taps) if tap_fast else (lambda kt: kt)
    if mutant == 'slice_order':           # A walks tap-fastest, W slice-fastest
        return [(kt % taps) * slices + kt // taps for kt in range(nkt)], list(range(nkt))
    per = G._cdiv(nkt, case.split)         # 'splitk_restart': the counters of a later slice start at (tap 0, slice 0)
    a = [block(kt - kt // per * per) for kt in range(nkt)]
    return a, a


def applies(case: Case, mutant: str) -> bool:
    '''Whether `mutant` is a different computation for this case.'''
    q = case.geom
    if mutant in GEOMETRY_MUTANTS:
        pre = {'pad_sym': (q.pad_t, q.pad_l) == (0, 0) and q.up == 0, 'pad_swap': q.pad_t != q.pad_l and q.up != 2, 'stride_one': q.stride != 1, 'up_ceil': q.up == 1,
               'up_bounds_low': q.up == 1, 'tap_transpose': q.kh == q.kw > 1, 'phase_pad': q.up == 2}.get(mutant, True)
        bm = G.expected_launch(case).tpl[0]
        return pre and any(not torch.equal(G.conv_taps(case, z, mutant, bm), G.conv_taps(case, z)) for z in range(case.batch))
    if mutant == 'slice_order':
        return q.cin > G.BK and q.kh * q.kw > 1
    if mutant == 'splitk_restart':
        return case.split > 1
    return case.phase


def emulate(case: Case, inp: dict, mutant: Optional[str] = None, tap_fast: Optional[bool] = None):
    '''fp32 emulation (gemm_cases.emulate) of the case, or of one wrong convolution; None where the mutant does not apply.  `tap_fast`: the K
    order of the launch (default: the case's own) -- 'splitk_restart' is another computation in each.'''
    if mutant is None:
        return G.emulate(case, inp)
    assert mutant in MUTANTS
    if not applies(case, mutant):
        return None
    if mutant in STORE_MUTANTS:
        return G.compute(case, inp, torch.float32, store_wrong=mutant)
    L = G.expected_launch(case)

    def acc(z):
        a = G.im2col(case, inp['A'][0 if case.phase else z], z, mutant if mutant in GEOMETRY_MUTANTS else None, L.tpl[0])
        w = inp['W'][z]
        if mutant in K_ORDER_MUTANTS:
            ab, wb = _k_blocks(case, mutant, L.tap_fast if tap_fast is None else tap_fast)
            cols = lambda blocks: torch.cat([torch.arange(b * G.BK, (b + 1) * G.BK) for b in blocks])
            a, w = a[:, cols(ab)], w[:, cols(wb)]
        return G._matmul(a, w, torch.float32)
    return G.compute(case, inp, torch.float32, acc_of=acc)


def loader(case: Case, env={}) -> str:
    ''''dma' | 'dmap' | 'reg' | 'pp': which of the four loaders runs the case under `env`.'''
    return G.expected_launch(case, env).form


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--child', 'usage: conv_cases.py --child \'{"env": {...}, "run": [ids], "refuse": [ids], "good": id}\''
    sys.exit(G._child(json.loads(sys.argv[2]), BY_ID, reference))
