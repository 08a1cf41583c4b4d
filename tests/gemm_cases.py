'''One table of fd_gemm_f16 cases for the 2-barrier family of csrc/gemm.hip (tile ids 1..16, 20, 23: k_gemm_f16_dma, the
persistent k_gemm_f16_dmap, the register-staged k_gemm_f16 and the two split-K finish kernels), a Python restatement of
launch_epi / launch_mode, a float64 reference and the acceptance criterion -- shared by tests/test_gemm_cases.py (CPU: the
table reaches every launch target, `check` rejects wrong GEMMs) and tests/test_gpu_gemm_cases.py (MI355X: every case through
the C ABI).  The ping-pong tiles 30..33 have tests/test_gpu_gemm_pp.py.

Nothing here needs a GPU to import.  `run_on_device` (and the `--child` entry at the bottom, one fresh process per FD_GEMM_* /
FD_CONV_TAPFAST setting: the library reads them once per process) is the only part that touches one.

Every case forces its tile (fd_gemm_desc.tile) and split-K factor, so the rule cascade plays no part: the tile id and the
split come from fd_gemm_plan (host logic only), the rest of the launch -- epilogue, convolution form, transposed store,
one-shot / persistent / register-staged kernel, finish kernel -- from `expected_launch`.

Left out: FD_GEMM_PP (it only moves the rule, and the cases force their tiles), the experimental sk_sync, gn_skip_c and operands
>= 2 GiB (the only way to the register-staged kernel besides FD_GEMM_NO_DMA).  Every convolution of THIS table has one geometry --
stride 1, padding (k - 1) // 2, a near-square output; the strided, unpadded, odd-sized, fused-upsample and phase-decomposed
(upsample2x) geometries on every loader, the ping-pong tiles among them, are the table of tests/conv_cases.py, built on this module.'''
from __future__ import annotations

import ctypes
import json
import os
import sys
from collections import namedtuple
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

ACT_NONE, ACT_SILU, ACT_QUICK_GELU, ACT_GELU, ACT_GEGLU = 0, 1, 2, 3, 4
BK = 64
PAD_IN = 100.0        # junk in every input padding column / row gap (finite: a kernel that reads it moves the result by ~100)
SENTINEL = -1234.0    # every element of the output buffers before the launch
GUARD_ROWS = 8        # sentinel rows before and after C (8 rows keep the 16-byte alignment of C for every ldc % 4 == 0)
EPS24 = 2.0 ** -24    # fp32 unit roundoff
LN_EPS = 1e-5
BIAS_PERIOD = 23      # the bias of a case with an activation repeats every 23 columns (see `inputs`)
ENV_SETTINGS = ({'FD_GEMM_FAST_EPI': '0'}, {'FD_GEMM_BIAS_LDS': '0'}, {'FD_GEMM_PERSIST': '0'}, {'FD_GEMM_PERSIST': '2'},
                {'FD_GEMM_NO_DMA': '1'}, {'FD_GEMM_VT_TILE': '0'}, {'FD_CONV_TAPFAST': '0'}, {'FD_CONV_TAPFAST': '2'})

# (BM, BN, WM, NS, WN, ALLOW) of the tiles that go through launch_epi, (BM, BN, WM, NS, WN) of those that go through launch
LEAN = {9: (128, 160, 4, 2, 2, 38), 10: (128, 128, 4, 2, 2, 110), 12: (128, 160, 8, 2, 2, 294), 13: (256, 160, 8, 2, 2, 294),
        23: (288, 160, 6, 2, 2, 294), 14: (256, 128, 8, 2, 2, 110), 15: (256, 256, 4, 2, 4, 110), 16: (256, 320, 4, 2, 4, 294),
        20: (128, 160, 4, 3, 2, 294)}
GENERIC = {1: (128, 128, 2, 2, 2), 2: (128, 160, 2, 2, 2), 3: (128, 64, 2, 2, 2), 4: (64, 64, 2, 2, 2), 5: (256, 160, 4, 2, 2),
           6: (256, 128, 4, 2, 2), 7: (256, 160, 4, 3, 2), 8: (256, 128, 4, 3, 2), 11: (128, 64, 4, 2, 2)}
# (BM, BN, WM, WN) of the ping-pong tiles of csrc/gemm_pp.hip (fd_gemm_pp_tile_shape); tests/conv_cases.py forces them, no case of this table does
PP = {30: (256, 320, 2, 4), 31: (256, 256, 2, 4), 32: (128, 320, 2, 4), 33: (256, 160, 4, 2)}


class Case(NamedTuple):
    id: str
    tile: int
    M: int
    N: int
    K: int
    split: int = 1
    act: int = ACT_NONE
    res: bool = False
    res_rows: int = 0
    bias2: bool = False
    rps: int = 0              # rows_per_sample (0 = M); convolutions: out_h * out_w
    alpha: float = 0.0        # 0 = 1
    out_f32: bool = False
    batch: int = 1            # > 1: gapped batch strides
    batch_bias: bool = False
    conv: Optional[tuple] = None     # (out_h, out_w, in_c, kh, kw, stride[, pad_t, pad_l[, upsample2x[, in_h, in_w]]]): see `geom`
    K2: int = 0
    ln: int = 0               # LayerNorm fold: 1 = finished statistics, 2 / 4 / 8 = ln_stats_parts
    stats_out: bool = False
    gn_parts: int = 0         # gn_part_out with this many groups
    gn_out: int = 0           # gn_out (split-K finish) with this many groups
    trans: bool = False
    trans_n0: int = 0
    layout: str = 'contig'    # 'contig' | 'padded'
    seed: int = 0

    @property
    def n_out(self) -> int:
        return self.N // 2 if self.act == ACT_GEGLU else self.N

    @property
    def rows(self) -> int:    # rows per sample as the kernel sees them
        return self.rps if self.rps > 0 else self.M

    @property
    def geom(self):
        return geom(self.conv)

    @property
    def phase(self) -> bool:  # upsample2x == 2: batch = the four output parities, one shared input, one interleaved output
        return self.conv is not None and self.geom.up == 2

    @property
    def edges(self) -> set:
        '''The layouts and edges of this case (see `EDGES`).'''
        e = {self.layout}
        if self.K % BK:
            e.add('k_tail')
        if self.alpha not in (0.0, 1.0):
            e.add('alpha')
        if self.batch > 1:
            e.add('batch')
        if self.batch_bias:
            e.add('batch_bias')
        if self.res_rows:
            e.add('res_wrap')
        if self.bias2:
            e.add('bias2')
        if self.trans and self.layout == 'padded':
            e.add('trans_pad')
        return e


EDGES = ('padded', 'k_tail', 'ragged', 'alpha', 'batch', 'batch_bias', 'res_wrap', 'bias2', 'trans_pad')

Geom = namedtuple('Geom', 'ho wo cin kh kw stride pad_t pad_l up hi wi')


def geom(conv: tuple) -> Geom:
    '''Case.conv with its defaults filled in: padding ((kh - 1) // 2, (kw - 1) // 2), upsample2x 0 (1: the loader reads a nearest-2x upsampled
    view of the input; 2: the phase-decomposed form, four 2x2 parity filters over the low-resolution input) and an input of out * stride
    (`hi`, `wi`: the size of the stored input; with upsample2x == 1 the loader's bounds are twice that).'''
    ho, wo, cin, kh, kw, stride = conv[:6]
    pad_t, pad_l = conv[6:8] if len(conv) >= 8 else ((kh - 1) // 2, (kw - 1) // 2)
    up = conv[8] if len(conv) >= 9 else 0
    hi, wi = conv[9:11] if len(conv) >= 11 else (ho * stride, wo * stride)
    return Geom(ho, wo, cin, kh, kw, stride, pad_t, pad_l, up, hi, wi)


# ------------------------------------------------------------------------------------------------ the launch, restated
Launch = namedtuple('Launch', 'kernel tpl form finish tap_fast')
# tpl = (BM, BN, WM, NS, WN, EPI, CONV, TRANS); the register-staged kernel is k_gemm_f16<BM, BN, TRANS, CONV> (WM = WN = 2, one stage
# pair, generic epilogue: NS = 2, EPI = 0 in the tuple); form in 'dma' | 'dmap' | 'reg'; finish: None | 'k_splitk_finish' |
# 'k_splitk_finish_gn<S>'; tap_fast: the run-time loop order of the same convolution template that FD_CONV_TAPFAST moves


def _cdiv(a, b):
    return -(-a // b)


def launch_mode(g, split, env, BM, BN, TRANS, CONV, WM=2, NS=2, WN=2, EPI=0):
    '''launch_mode<BM, BN, TRANS, CONV, WM, NS, WN, EPI> of csrc/gemm.hip -> (kernel, tpl, form).  Operands are < 2 GiB in every case.'''
    lds = NS * (BM + BN) * 128 + 4 * BN * 4 + (BM * 2 * 4 if EPI in (5, 6, 7, 13) else 0)
    if 'FD_GEMM_NO_DMA' not in env:
        occ = 1 if (BM >= 256 or lds > 80 * 1024) else 2 if BM * BN >= 128 * 128 else 3 if BM == 128 else 4
        slots = 256 * occ
        nkt = _cdiv(g.K, BK) // split
        mode = int(env.get('FD_GEMM_PERSIST', 1))
        tiles = _cdiv(g.M, BM) * _cdiv(g.N, BN)
        persistent = (NS == 2 and BN != 320 and EPI != 13 and g.K2 == 0 and not getattr(g, 'phase', False) and not g.stats_out and g.ln_parts <= 1 and not g.stride_bias and
                      (mode == 2 or (mode == 1 and nkt <= 20 and tiles > slots)))
        if 1 <= EPI <= 3 and persistent and g.bias2:
            return launch_mode(g, split, env, BM, BN, TRANS, CONV, WM, NS, WN, 0)
        return ('k_gemm_f16_dmap' if persistent else 'k_gemm_f16_dma', (BM, BN, WM, NS, WN, EPI, CONV, TRANS), 'dmap' if persistent else 'dma')
    if g.ln:
        raise ValueError('the LayerNorm fold needs the LDS-DMA path')
    if g.K2:
        raise ValueError('the appended phase needs the LDS-DMA path')
    if EPI != 0:
        return launch_mode(g, split, env, BM, BN, TRANS, CONV, WM, NS, WN, 0)
    if WM != 2 or WN != 2:
        raise ValueError('8-wave tiles need the LDS-DMA path')
    return ('k_gemm_f16', (BM, BN, 2, 2, 2, 0, CONV, TRANS), 'reg')


def launch_epi(g, split, env, BM, BN, WM, NS, WN, ALLOW):
    '''launch_epi<BM, BN, WM, NS, WN, ALLOW> -> (kernel, tpl, form).'''
    lm = lambda epi, conv: launch_mode(g, split, env, BM, BN, False, conv, WM, NS, WN, epi)
    glu_ok = (BN // WN // 16) % 2 == 0
    full = (int(env.get('FD_GEMM_FAST_EPI', 1)) != 0 and split == 1 and not g.out_f32 and not g.trans and int(env.get('FD_GEMM_BIAS_LDS', 1)) != 0 and
            g.M % BM == 0 and g.N % BN == 0 and g.ldc % 8 == 0 and (not g.bias2 or g.rows % BM == 0))
    if g.gn_part:
        if BN == 320 and NS == 2 and full and g.act == ACT_NONE and not g.ln and not g.stats_out and g.N == BN and g.rows % BM == 0 and g.batch == 1 and \
                (not g.res or g.ldr % 4 == 0):
            return lm(12 if g.res else 11, g.conv)
        raise ValueError('gn_part_out needs full 320-wide tiles inside one sample')
    if g.stats_out:
        if ALLOW & 256 and full and (BN != 320 or g.N == BN) and g.act == ACT_NONE and not g.conv and not g.ln and not g.bias2:
            if g.res and g.ldr % 4 == 0:
                return lm(9, False)
            if not g.res:
                return lm(8, False)
        raise ValueError('ln_stats_out needs full tiles of a tile shape with a statistics epilogue')
    small = lambda: launch_mode(g, split, env, 128, 128, False, False, 2, 2, 2, 7)
    if full and g.ln:
        if not g.conv and not g.res:
            if ALLOW & 64 and glu_ok and g.act == ACT_GEGLU:
                return lm(6, False)
            if ALLOW & 32 and g.act == ACT_NONE:
                return lm(5, False)
        return small()
    if g.ln:
        return small()
    if full:
        if ALLOW & 8 and glu_ok and g.act == ACT_GEGLU:
            return lm(3, g.conv)
        if ALLOW & 4 and g.act == ACT_NONE and g.res and g.ldr % 4 == 0:
            return lm(2, g.conv)
        if ALLOW & 2 and g.act == ACT_NONE and not g.res:
            return lm(1, g.conv)
    return lm(0, g.conv)


def select(g, tile, split, env={}) -> Launch:
    '''What gemm_launch launches for the (already planned) tile id and split factor: the part of fd_gemm_f16 behind the rule.  `g` carries
    M, N, K, K2, act, res, ldr, ldc, bias, bias2, rows, out_f32, trans, trans_n0, conv, ln, ln_parts, stats_out, gn_part, gn_out, stride_bias, batch.'''
    dma = 'FD_GEMM_NO_DMA' not in env
    lean_ok = dma and int(env.get('FD_GEMM_FAST_EPI', 1)) != 0 and int(env.get('FD_GEMM_BIAS_LDS', 1)) != 0
    if g.ln_parts > 1 and not dma:
        raise ValueError('ln_stats_parts needs the LDS-DMA path')
    if g.trans_n0:
        if not lean_ok:
            raise ValueError('trans_n0 needs the LDS-DMA path with the lean epilogue')
        return Launch(*launch_mode(g, 1, env, 128, 160, False, False, 4, 2, 2, 13), None, False)
    if g.trans:
        vt160 = int(env.get('FD_GEMM_VT_TILE', 9)) != 0 and g.N % 160 == 0 and g.batch == 1 and g.M >= 8192
        if vt160:
            lm = launch_mode(g, 1, env, 128, 160, True, False, 4, 2, 2, 7 if g.ln else 0)
        else:
            lm = launch_mode(g, 1, env, 128, 64, True, False if g.ln else g.conv, 2, 2, 2, 7 if g.ln else 0)
        return Launch(*lm, None, False)
    if g.stride_bias and not (dma and int(env.get('FD_GEMM_BIAS_LDS', 1)) != 0):
        raise ValueError('batch_stride_bias needs the LDS-DMA path with LDS-staged biases')
    if g.gn_part and not lean_ok:
        raise ValueError('gn_part_out needs the lean epilogue')
    if g.gn_out and split not in (2, 4, 8, 16):
        raise ValueError('gn_out is honoured by split-K launches only')
    up, phase = getattr(g, 'up', False), getattr(g, 'phase', False)
    if phase:
        # gemm_check: only the lean plain epilogue knows the parity row map; gemm_check_tile: a tile that has one, full tiles, no split
        if not lean_ok:
            raise ValueError('upsample2x == 2 needs the lean epilogue on the LDS-DMA path')
        bm, bn = LEAN[tile][:2] if tile in LEAN else PP[tile][:2] if tile in PP else (0, 0)
        if not bm or g.M % bm or g.N % bn or split != 1:
            raise ValueError('upsample2x == 2 needs full tiles of a tile with a lean epilogue and no split-K')
    finish = None
    if split > 1:
        finish = f'k_splitk_finish_gn<{split}>' if g.gn_out else 'k_splitk_finish'
    if tile in PP:
        # fd_gemm_pp_ok / pp_launch of csrc/gemm_pp.hip, as far as the convolution table goes (plain, residual and per-sample-bias epilogues;
        # the forced tile runs whatever FD_GEMM_PERSIST / FD_GEMM_NO_DMA / FD_CONV_TAPFAST say: one kernel, tap-fastest only)
        BM, BN, WM, WN = PP[tile]
        assert g.act == ACT_NONE and not (g.ln or g.stats_out or g.gn_part or g.gn_out or g.K2 or g.trans), 'not restated for the ping-pong tiles'
        if g.M % BM or g.N % BN or g.K % BK:
            raise ValueError('ping-pong tiles need full tiles and K % 64 == 0')
        if g.conv and (g.Wo % 8 or up):
            raise ValueError('ping-pong tiles: an 8-row DMA group is 8 consecutive pixels of one output row; no fused upsample')
        if split > 1 and g.K // BK // split < 2:
            raise ValueError('ping-pong tiles need two K-tiles per slice')
        lean = split == 1 and not g.out_f32 and int(env.get('FD_GEMM_BIAS_LDS', 1)) != 0 and g.ldc % 8 == 0 and (not g.bias2 or g.rows % BM == 0)
        epi = 10 if split > 1 and g.N % 4 == 0 else 2 if lean and g.res and g.ldr % 4 == 0 else 1 if lean and not g.res else 0
        return Launch('k_gemm_f16_pp', (BM, BN, WM, 2, WN, epi, g.conv, False), 'pp', finish, bool(g.conv))
    tap_fast = g.conv and (int(env.get('FD_CONV_TAPFAST', 1)) == 2 or (int(env.get('FD_CONV_TAPFAST', 1)) == 1 and tile == 16))
    if g.ln and tile not in LEAN:
        # small problems: the generic epilogue with the fold compiled in (64x64 for few rows); fd_gemm_plan says 4 or -7
        lm = launch_mode(g, split, env, 64, 64, False, False, 2, 2, 2, 7) if tile == 4 else launch_mode(g, split, env, 128, 128, False, False, 2, 2, 2, 7)
    elif tile in LEAN:
        lm = launch_epi(g, split, env, *LEAN[tile])
    else:
        BM, BN, WM, NS, WN = GENERIC.get(tile, GENERIC[1])
        lm = launch_mode(g, split, env, BM, BN, False, g.conv, WM, NS, WN, 0)
    return Launch(*lm, finish, bool(tap_fast))


def flags(case: Case) -> SimpleNamespace:
    p = layout_plan(case)
    return SimpleNamespace(M=case.M, N=case.N, K=case.K, K2=case.K2, act=case.act, res=case.res, ldr=p['ldr'], ldc=p['ldc'], bias=True,
                           bias2=case.bias2, rows=case.rows, out_f32=case.out_f32, trans=case.trans, trans_n0=case.trans_n0, conv=case.conv is not None,
                           ln=case.ln > 0, ln_parts=case.ln if case.ln > 1 else 0, stats_out=case.stats_out, gn_part=case.gn_parts > 0,
                           gn_out=case.gn_out > 0, stride_bias=case.batch_bias, batch=case.batch,
                           up=case.conv is not None and case.geom.up == 1, phase=case.phase, Wo=case.geom.wo if case.conv else 0)


_plan_cache = {}


def plan(case: Case):
    '''(tile id, split-K factor) from fd_gemm_plan: host logic only, no device.  ValueError where the library refuses the descriptor.'''
    if case not in _plan_cache:
        from flexdiffuse_amd import hip
        p = layout_plan(case)
        fake = {n: 0x10000000 + 0x1000000 * i for i, n in enumerate(('A', 'W', 'C', 'bias', 'bias2', 'res', 'ws', 'ln_stats', 'colsum', 'stats_out', 'A2',
                                                                      'gn_out', 'gn_gamma', 'gn_beta', 'gn_part', 'C2'))}
        d = build_desc(case, p, fake)
        tile, split = ctypes.c_int(0), ctypes.c_int(0)
        rc = hip.lib().fd_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(split))
        _plan_cache[case] = (rc, tile.value, split.value)
    rc, tile, split = _plan_cache[case]
    if rc != 0:
        raise ValueError(f'fd_gemm_plan refused {case.id}: rc {rc}')
    return tile, split


def expected_launch(case: Case, env={}) -> Launch:
    '''The launch fd_gemm_f16 makes for `case` under the FD_GEMM_* / FD_CONV_TAPFAST variables in `env`; ValueError where it answers FD_ESHAPE.
    (The planned tile does not depend on `env`: the cases force it, and of the switches only FD_GEMM_PP enters the rule.  The child processes
    check that against fd_gemm_plan under the setting.)'''
    tile, split = plan(case)
    return select(flags(case), tile, split, env)


def launch_of_desc(d, env={}) -> Launch:
    '''The launch fd_gemm_f16 makes for a finished fd_gemm_desc `d` (one that ops.gemm / ops.conv2d built, say): tile and split from
    fd_gemm_plan, the rest from `select` on the descriptor's own strides and flags.'''
    from flexdiffuse_amd import hip
    tile, split = ctypes.c_int(0), ctypes.c_int(0)
    rc = hip.lib().fd_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(split))
    if rc != 0:
        raise ValueError(f'fd_gemm_plan refused the descriptor: rc {rc}')
    g = SimpleNamespace(M=d.M, N=d.N, K=d.K, K2=d.K2, act=d.act, res=bool(d.residual), ldr=d.ldr, ldc=d.ldc, bias=bool(d.bias), bias2=bool(d.bias2),
                        rows=d.rows_per_sample if d.rows_per_sample > 0 else d.M, out_f32=bool(d.out_f32), trans=bool(d.trans_out), trans_n0=d.trans_n0,
                        conv=bool(d.conv), ln=bool(d.ln_stats), ln_parts=d.ln_stats_parts if d.ln_stats_parts > 1 else 0, stats_out=bool(d.ln_stats_out),
                        gn_part=bool(d.gn_part_out), gn_out=bool(d.gn_out), stride_bias=bool(d.batch_stride_bias), batch=max(d.batch, 1),
                        up=bool(d.conv) and d.upsample2x == 1, phase=bool(d.conv) and d.upsample2x == 2, Wo=d.out_w)
    return select(g, tile.value, split.value, env)


def refused(case: Case, env={}) -> bool:
    try:
        expected_launch(case, env)
        return False
    except ValueError:
        return True


def is_ragged(case: Case) -> bool:
    bm, bn = expected_launch(case).tpl[:2]
    return case.M % bm != 0 or case.N % bn != 0


# ------------------------------------------------------------------------------------------------ layout
def _r(x, m):
    return (x + m - 1) // m * m


def layout_plan(case: Case) -> dict:
    '''Row strides, batch strides and flat buffer sizes (elements).  'padded': lda > K, ldw > K + K2, ldc > N, ldr != ldc (ldc % 8 == 0 and
    ldr % 8 == 0 so that the lean epilogues stay reachable), ld_bias2 > N, trans_ld > rows_per_sample, junk rows behind the statistics.'''
    pad = case.layout == 'padded'
    M, N, K, K2, n_out = case.M, case.N, case.K, case.K2, case.n_out
    p = {}
    if case.conv:
        ho, wo, cin, kh, kw = case.geom[:5]
        assert K == kh * kw * cin and M % (ho * wo) == 0 and cin % BK == 0
        p['B'], p['Hi'], p['Wi'] = M // (ho * wo), case.geom.hi, case.geom.wi
        p['lda'] = cin + 8 if pad else cin            # pixel stride
        p['a_size'] = p['B'] * p['Hi'] * p['Wi'] * p['lda']
    else:
        p['lda'] = _r(K, 8) + (8 if pad else 0)
        p['a_size'] = M * p['lda']
    p['ldw'] = _r(K + K2, 8) + (16 if pad else 0)
    p['w_size'] = N * p['ldw']
    p['lda2'] = K2 + (8 if pad else 0)
    p['ldc'] = (case.trans_n0 if case.trans_n0 else n_out) + (8 if pad else 0)
    p['ldr'] = N + (16 if pad else 0)
    p['ldb2'] = N + (8 if pad else 0)
    p['c_rows'] = M
    if case.trans:
        # C is [sample][N][trans_ld]; "rows" of the flat buffer are the N output rows of every sample
        p['ldt'] = case.rows + (8 if pad else 0)
        p['sT'] = N * p['ldt'] + (16 if pad else 0)
        p['c_len'] = (M // case.rows) * p['sT']
        p['ldc'] = 0
    else:
        p['c_len'] = (4 * M if case.phase else M) * p['ldc']      # phase: [B][2 out_h][2 out_w] pixels, the four parities interleaved
    if case.trans_n0:
        p['ldt'] = case.rows + (8 if pad else 0)
        p['sT'] = (N - case.trans_n0) * p['ldt'] + (16 if pad else 0)
        p['c2_len'] = (M // case.rows) * p['sT']
    # batch strides: gaps behind every batch's matrix
    gap = case.batch > 1
    p['sA'] = p['a_size'] + (64 if gap else 0)
    p['sW'] = p['w_size'] + (64 if gap else 0)
    p['sC'] = p['c_len'] + (GUARD_ROWS * p['ldc'] if gap and not case.stats_out else 0)
    p['sR'] = M * p['ldr'] + (32 if gap else 0)
    p['sBias'] = _r(N, 4) + 4 if case.batch_bias else 0
    p['ZA'] = p['ZC'] = case.batch
    if case.phase:
        # the four parity slices read one input and write one output: batch_stride_a = batch_stride_c = 0, only W has a batch stride
        assert case.batch == 4 and not case.res and not case.batch_bias
        p['sA'] = p['sC'] = p['sR'] = 0
        p['ZA'] = p['ZC'] = 1
    p['guard'] = GUARD_ROWS * max(p['ldc'], 8)
    return p


def build_desc(case: Case, p: dict, ptr: dict):
    '''The fd_gemm_desc of `case` by hand (not through ops.gemm / ops.conv2d); ptr: name -> address.'''
    from flexdiffuse_amd import ops
    d = ops.fd_gemm_desc()
    d.A, d.W, d.C, d.bias = ptr['A'], ptr['W'], ptr['C'], ptr['bias']
    d.M, d.N, d.K = case.M, case.N, case.K
    d.lda, d.ldw, d.ldc = p['lda'], p['ldw'], p['ldc']
    d.rows_per_sample, d.act, d.out_f32, d.alpha = case.rps, case.act, int(case.out_f32), case.alpha
    d.batch = case.batch
    if case.batch > 1:
        d.batch_stride_a, d.batch_stride_w, d.batch_stride_c, d.batch_stride_res = p['sA'], p['sW'], p['sC'], p['sR']
        d.batch_stride_bias = p['sBias']
    if case.res:
        d.residual, d.ldr, d.residual_rows = ptr['res'], p['ldr'], case.res_rows
    if case.bias2:
        d.bias2, d.ld_bias2 = ptr['bias2'], p['ldb2']
    if case.conv:
        q = case.geom
        d.conv, d.in_h, d.in_w, d.in_c, d.out_h, d.out_w = 1, p['Hi'], p['Wi'], q.cin, q.ho, q.wo
        d.kh, d.kw, d.stride, d.pad_t, d.pad_l, d.upsample2x = q.kh, q.kw, q.stride, q.pad_t, q.pad_l, q.up
    if case.K2:
        d.A2, d.lda2, d.K2 = ptr['A2'], p['lda2'], case.K2
    if case.ln:
        d.ln_stats, d.ln_colsum = ptr['ln_stats'], ptr['colsum']
        if case.ln > 1:
            d.ln_stats_parts, d.ln_stats_rows, d.ln_fold_eps = case.ln, stats_rows(case), LN_EPS
    if case.stats_out:
        d.ln_stats_out, d.ln_eps = ptr['stats_out'], LN_EPS
    if case.gn_parts:
        d.gn_part_out, d.gn_groups, d.gn_part_chunks = ptr['gn_part'], case.gn_parts, case.rows // 256
    if case.gn_out:
        d.gn_out, d.gn_gamma, d.gn_beta, d.gn_groups, d.gn_silu, d.gn_eps = ptr['gn_out'], ptr['gn_gamma'], ptr['gn_beta'], case.gn_out, 1, LN_EPS
    if case.trans:
        d.trans_out, d.trans_ld, d.trans_sample_stride = 1, p['ldt'], p['sT']
    if case.trans_n0:
        d.trans_n0, d.C2, d.trans_ld, d.trans_sample_stride = case.trans_n0, ptr['C2'], p['ldt'], p['sT']
    d.tile, d.split_k = case.tile, case.split
    if case.split > 1:
        d.workspace, d.workspace_bytes = ptr['ws'], case.split * case.M * case.N * 4
    return d


def stats_rows(case: Case) -> int:
    return case.M + (8 if case.layout == 'padded' else 0)


# ------------------------------------------------------------------------------------------------ inputs
def _rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def inputs(case: Case) -> dict:
    '''The rounded operands the device receives: fp16 A ([batch][M][K], convolutions [batch][B][Hi][Wi][Cin]), W, A2, residual; fp32 bias
    (a distinct value per column: arange * 0.25 - c, c rotating with the seed; with an activation (arange % 23) * 0.25 - c, within +-3.5), per-sample bias2 of a few units, and for the LayerNorm
    fold the prepared operands: W is the gain-folded fp16 W', colsum its fp32 row sums, the statistics come from float64 on the host.'''
    s, Z, M, N, K = case.seed * 16, case.batch, case.M, case.N, case.K
    p = layout_plan(case)
    inp = {}
    if case.conv:
        cin = case.conv[2]
        a = _rnd((p['ZA'], p['B'], p['Hi'], p['Wi'], cin), s)
    else:
        a = _rnd((Z, M, K), s)
        if case.ln or case.stats_out:
            m = torch.arange(M)
            a = a * (0.5 + (m % 5) * 0.4)[None, :, None] + (((m * 37) % 17 - 8) / 8.0)[None, :, None]    # unequal spreads, non-zero means
    inp['A'] = a.half()
    inp['W'] = (_rnd((Z, N, K + case.K2), s + 1) * (K + case.K2) ** -0.5).half()
    if case.K2:
        inp['A2'] = _rnd((M, case.K2), s + 2).half()
    if case.act == ACT_NONE:
        c = 0.25 * ((case.seed * 37) % N)
        bias = torch.arange(N, dtype=torch.float32) * 0.25 - c
    else:
        # An activation flushes everything below about -8 to 0, where the bound is only atol: a bias that ran over all N columns would leave
        # whole tiles dead.  The column index wraps every BIAS_PERIOD columns instead: the pre-activations stay within a few units of 0,
        # neighbours still differ by 0.25 (5.5 at the wrap), and so do the columns n and n + k BN of any two tile columns of the table (23 is
        # prime and divides no tile width, so k BN % 23 != 0 for k < 23).
        c = 0.25 * (11 + case.seed % 3)
        bias = (torch.arange(N) % BIAS_PERIOD).float() * 0.25 - c
    inp['bias'] = torch.stack([bias + 3.0 * z for z in range(Z)]) if case.batch_bias else bias[None]
    if case.res:
        rr = case.res_rows if case.res_rows else M
        r = _rnd((Z, rr, N), s + 3)
        if case.stats_out or case.gn_parts:
            r = r * 2.0 + torch.arange(rr)[None, :, None] % 7 - 3.0          # row means far from zero
        inp['res'] = r.half()
    if case.bias2:
        ns = _cdiv(M, case.rows)
        inp['bias2'] = (torch.tensor([(1.5 + 1.5 * i) * (-1) ** i for i in range(ns)])[:, None] + 0.5 * _rnd((ns, N), s + 4)).float()
    if case.ln:
        x = inp['A'][0].double()
        inp['colsum'] = inp['W'][0].double().sum(1).float()
        if case.ln == 1:
            mean, var = x.mean(1), x.var(1, unbiased=False)
            rstd = (var + LN_EPS).rsqrt()
            inp['ln_stats'] = torch.stack([rstd, -mean * rstd], dim=1).float()                        # [M][2]
        else:
            k, rows = case.ln, stats_rows(case)
            parts = torch.full((k, rows, 2), PAD_IN, dtype=torch.float32)
            for i, ch in enumerate(x.chunk(k, dim=1)):                                               # raw (sum, sum of squares) slabs
                parts[i, :M, 0], parts[i, :M, 1] = ch.sum(1).float(), (ch * ch).sum(1).float()
            inp['ln_stats'] = parts
    if case.gn_out:
        inp['gn_gamma'] = (1.0 + 0.2 * _rnd((N,), s + 5)).float()
        inp['gn_beta'] = (0.3 * _rnd((N,), s + 6)).float()
    return inp


def conv_taps(case: Case, z: int = 0, wrong: Optional[str] = None, bm: int = 0):
    '''The loaders' geometry, restated: -> [M][kh * kw] int64, the linear pixel index (b * Hi + y) * Wi + x of the stored input that GEMM
    row m = (b, oy, ox) reads for filter tap (ky, kx), -1 where the tap reads zero.  In the view the loader walks -- the stored input, or
    its nearest-2x upsampling with upsample2x == 1 -- the tap is at (oy * stride - pad_t + ky, ox * stride - pad_l + kx); outside the view it
    is zero; upsample2x == 1 halves the coordinates (>> 1).  upsample2x == 2: slice z = 2 py + px has pad (1 - py, 1 - px).
    `wrong`: one of the wrong geometries of tests/conv_cases.py (`bm`: the tile's rows, for 'sample_base').'''
    q = case.geom
    hw, total = q.ho * q.wo, (case.M // (q.ho * q.wo)) * q.hi * q.wi
    m = torch.arange(case.M)
    b, rem = m // hw, m % hw
    if wrong == 'sample_base':
        b = (m // bm * bm) // hw
    oy, ox = rem // q.wo, rem % q.wo
    pt, pl = (1 - (z >> 1), 1 - (z & 1)) if q.up == 2 and wrong != 'phase_pad' else (q.pad_t, q.pad_l)
    if wrong == 'pad_sym':
        pt = pl = 1
    if wrong == 'pad_swap':
        pt, pl = pl, pt
    stride = 1 if wrong == 'stride_one' else q.stride
    ky, kx = torch.arange(q.kh).repeat_interleave(q.kw), torch.arange(q.kw).repeat(q.kh)
    if wrong == 'tap_transpose':
        ky, kx = kx, ky
    iy, ix = (oy * stride - pt)[:, None] + ky[None, :], (ox * stride - pl)[:, None] + kx[None, :]
    up = q.up == 1
    hv, wv = (2 * q.hi, 2 * q.wi) if up and wrong != 'up_bounds_low' else (q.hi, q.wi)
    ok_y, ok_x = (iy >= 0) & (iy < hv), (ix >= 0) & (ix < wv)
    if up:
        r = 1 if wrong == 'up_ceil' else 0
        iy, ix = (iy + r) >> 1, (ix + r) >> 1
    lin = (b[:, None] * q.hi * q.wi + iy * q.hi + ix) if wrong == 'hw_swap' else ((b[:, None] * q.hi + iy) * q.wi + ix)
    ok = (ok_y & (lin >= 0) & (lin < total)) if wrong == 'edge_wrap' else (ok_y & ok_x)
    return torch.where(ok, lin % total, torch.full_like(lin, -1))


def im2col(case: Case, a, z: int = 0, wrong: Optional[str] = None, bm: int = 0):
    '''[B][Hi][Wi][Cin] -> [M][kh * kw * Cin] in the weights' (kh, kw, Cin) order, zero padding: a gather through `conv_taps`.'''
    cin = a.shape[-1]
    flat = torch.cat([a.reshape(-1, cin), torch.zeros((1, cin), dtype=a.dtype)])       # (index -1: the zero pixel)
    return flat[conv_taps(case, z, wrong, bm)].reshape(case.M, -1)


# ------------------------------------------------------------------------------------------------ reference, emulation, mutants
MUTANTS = ('k_chunk', 'bias_next', 'res_drop', 'res_row_next', 'res_ldc', 'alpha_ignored', 'geglu_swap', 'stats_row_xor1', 'colsum_next',
           'bias2_border', 'tile_swap', 'trans_ld')


def applies(case: Case, mutant: str) -> bool:
    '''Whether `mutant` is a different computation for this case at all.'''
    p = layout_plan(case)
    if mutant == 'tile_swap':
        bm, bn = expected_launch(case).tpl[:2]
        return not case.trans and not case.trans_n0 and case.M >= 2 * bm and case.N >= 2 * bn
    return {'k_chunk': True, 'bias_next': True, 'res_drop': case.res, 'res_row_next': case.res,
            'res_ldc': case.res and case.batch == 1 and p['ldr'] != p['ldc'] and not case.trans,
            'alpha_ignored': case.alpha not in (0.0, 1.0), 'geglu_swap': case.act == ACT_GEGLU, 'stats_row_xor1': case.ln > 0,
            'colsum_next': case.ln > 0,
            'bias2_border': case.bias2 and _cdiv(case.M, case.rows) >= 2, 'trans_ld': p.get('ldt', 0) > case.rows}[mutant]


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def _act(x, act):
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    if act == ACT_QUICK_GELU:
        return x * torch.sigmoid(1.702 * x)
    if act == ACT_GELU:
        return _gelu(x)
    return x


def _matmul(a, w, dtype):
    '''a [M][K] @ w[N][K]^T.  float64: one product.  float32: the emulation -- fp32 accumulation over 64-wide K chunks in REVERSED order.'''
    if dtype == torch.float64:
        return a.double() @ w.double().T
    a, w = a.float(), w.float()
    acc = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32)
    for k0 in reversed(range(0, a.shape[1], BK)):
        acc += a[:, k0:k0 + BK] @ w[:, k0:k0 + BK].T
    return acc


def phase_rows(case: Case, z: int, wrong: Optional[str] = None):
    '''upsample2x == 2: the output row (pixel of the [B][2 out_h][2 out_w] map) of every GEMM row m = (b, y, x) of parity slice z = 2 py + px:
    pixel (2 y + py, 2 x + px).  `wrong`: 'phase_parity_swap' | 'phase_row_pitch' of tests/conv_cases.py.'''
    q = case.geom
    m = torch.arange(case.M)
    b, rem = m // (q.ho * q.wo), m % (q.ho * q.wo)
    py, px = (z & 1, z >> 1) if wrong == 'phase_parity_swap' else (z >> 1, z & 1)
    return (b * 2 * q.ho + 2 * (rem // q.wo) + py) * ((1 if wrong == 'phase_row_pitch' else 2) * q.wo) + 2 * (rem % q.wo) + px


def phase_store(case: Case, y4, wrong: Optional[str] = None):
    '''[4][M][N] -> [1][4 M][N]: the interleaved store of the four parity slices (an element no slice writes keeps the sentinel).'''
    out = torch.full((1, 4 * case.M, y4.shape[-1]), SENTINEL, dtype=y4.dtype)
    for z in range(4):
        out[0, phase_rows(case, z, wrong)] = y4[z]
    return out


def phase_slices(case: Case, c):
    '''The inverse of `phase_store`: [1][4 M][N] -> [4][M][N].'''
    return torch.stack([c[0, phase_rows(case, z)] for z in range(4)])


def compute(case: Case, inp: dict, dtype=torch.float64, mutant: Optional[str] = None, cache: Optional[dict] = None, acc_of=None,
            store_wrong: Optional[str] = None) -> Optional[dict]:
    '''The operation of `case` on the rounded operands in `dtype` (float64: the reference; float32: the emulation, output rounded like the
    device's) -> {'C': [batch][M][n_out] (transposed store: [batch][samples][N][rows]; upsample2x == 2: [1][4 M][n_out]), 'C2'}; None where
    the mutant does not apply.
    `cache`: a dict of the caller's that keeps the accumulators (never modified here) between the mutants of one case.
    `acc_of(z)`: the [M][N] accumulator of batch z from elsewhere (tests/conv_cases.py: F.conv2d for the reference, a wrong geometry for a
    mutant) in place of im2col + matmul; `store_wrong`: a wrong parity store (`phase_rows`).'''
    assert mutant is None or mutant in MUTANTS
    if mutant is not None and not applies(case, mutant):
        return None
    M, N, K = case.M, case.N, case.K
    p = layout_plan(case)
    alpha = 1.0 if case.alpha == 0.0 or mutant == 'alpha_ignored' else case.alpha
    rows = torch.arange(M)
    outs = []
    for z in range(case.batch):
        key = (dtype, z, mutant == 'k_chunk')
        if acc_of is not None:
            cache = {key: acc_of(z)}
        if cache is None or key not in cache:
            a = im2col(case, inp['A'][0 if case.phase else z], z) if case.conv else inp['A'][z]
            if case.K2:
                a = torch.cat([a, inp['A2']], dim=1)
            if mutant == 'k_chunk':
                a = a.clone()
                a[:, -8:] = 0
            acc = _matmul(a, inp['W'][z], dtype)
            if cache is not None:
                cache[key] = acc
        acc = acc if cache is None else cache[key]
        bias = inp['bias'][z if case.batch_bias else 0].to(dtype)
        if mutant == 'bias_next':
            bias = bias.roll(-1)
        if case.ln:
            st = inp['ln_stats'].double()
            if case.ln > 1:       # the consumer tiles finalise the producer's partial sums (fd_ln_finalize_stats_f32's arithmetic)
                s1, s2 = st[:, :M, 0].sum(0), st[:, :M, 1].sum(0)
                mean = s1 / K
                rstd = ((s2 / K - mean * mean).clamp(min=0) + LN_EPS).rsqrt()
                st = torch.stack([rstd, -mean * rstd], dim=1)
            if mutant == 'stats_row_xor1':
                st = st[(rows ^ 1).clamp(max=M - 1)]
            cs = inp['colsum'].to(dtype)
            if mutant == 'colsum_next':
                cs = cs.roll(-1)
            st = st.to(dtype)
            y = st[:, :1] * acc + (st[:, 1:] * cs[None, :] + bias[None, :])
        else:
            b = bias[None, :]
            if case.bias2:
                samp = rows // case.rows
                if mutant == 'bias2_border':
                    samp = samp.clone()
                    samp[case.rows] = 0
                b = b + inp['bias2'].to(dtype)[samp]
            y = acc * alpha + b
        if case.act == ACT_GEGLU:
            h = y.view(M, N // 32, 2, 16)
            v, g = (h[:, :, 1], h[:, :, 0]) if mutant == 'geglu_swap' else (h[:, :, 0], h[:, :, 1])
            y = (v * _gelu(g)).reshape(M, N // 2)
        else:
            y = _act(y, case.act)
        if case.res and mutant != 'res_drop':
            rr = case.res_rows if case.res_rows else M
            if mutant == 'res_ldc':
                flat = _strided_fill(inp['res'][z], p['ldr'], M * max(p['ldr'], p['ldc']))
                r = torch.as_strided(flat, (rr, N), (p['ldc'], 1))
            else:
                r = inp['res'][z]
            idx = (rows + (1 if mutant == 'res_row_next' else 0)) % rr
            y = y + r.to(dtype)[idx]
        if dtype != torch.float64:
            y = y if case.out_f32 else y.half()
        outs.append(y)
    y = torch.stack(outs)
    out = {}
    if case.phase:
        return {'C': phase_store(case, y, store_wrong)}
    if mutant == 'tile_swap':
        bm, bn = expected_launch(case).tpl[:2]
        bn = bn // 2 if case.act == ACT_GEGLU else bn
        y = y.clone()
        t10 = y[:, bm:2 * bm, :bn].clone()
        y[:, bm:2 * bm, :bn] = y[:, :bm, bn:2 * bn]
        y[:, :bm, bn:2 * bn] = t10
    ns = M // case.rows
    if case.trans:
        out['C'] = y.view(case.batch, ns, case.rows, N).transpose(2, 3)
    elif case.trans_n0:
        out['C'] = y[:, :, :case.trans_n0]
        out['C2'] = y[0, :, case.trans_n0:].reshape(ns, case.rows, N - case.trans_n0).transpose(1, 2)
    else:
        out['C'] = y
    if mutant == 'trans_ld':
        # the transposed rows written with ld = rows_per_sample into the buffer whose rows are trans_ld apart, read back as the caller reads it
        key = 'C' if case.trans else 'C2'
        t = out[key].reshape(-1, ns, out[key].shape[-2], case.rows)
        got = torch.full((t.shape[0], ns, p['sT']), SENTINEL, dtype=t.dtype)
        got[:, :, :t.shape[2] * case.rows] = t.reshape(t.shape[0], ns, -1)
        out[key] = torch.as_strided(got, t.shape, (ns * p['sT'], p['sT'], p['ldt'], 1)).reshape(out[key].shape)
    if case.gn_out:
        if dtype == torch.float64:
            out['gn_affine'] = (inp['gn_gamma'], inp['gn_beta'])      # `worst` normalises the C the kernel stored (gn_of)
        else:
            out['gn_out'] = gn_of(case, y[0].half(), inp['gn_gamma'], inp['gn_beta']).half()
    return out


def gn_of(case: Case, c16, gamma, beta):
    """float64 GroupNorm + SiLU of the fp16-rounded output rows `c16` [M][N] (fd_gemm_desc.gn_out: the statistics are those of the stored values)."""
    M, N, G = case.M, case.N, case.gn_out
    x = c16.double().cpu().reshape(M // case.rows, case.rows, G, N // G)
    mean = x.mean(dim=(1, 3), keepdim=True)
    var = (x * x).mean(dim=(1, 3), keepdim=True) - mean * mean
    xn = ((x - mean) * (var.clamp(min=0) + LN_EPS).rsqrt()).reshape(M, N) * gamma.double() + beta.double()
    return xn * torch.sigmoid(xn)


def reference(case: Case, inp: Optional[dict] = None) -> dict:
    return compute(case, inp if inp is not None else inputs(case), torch.float64)


def emulate(case: Case, inp: Optional[dict] = None, mutant: Optional[str] = None, cache: Optional[dict] = None):
    return compute(case, inp if inp is not None else inputs(case), torch.float32, mutant, cache)


LIVE_ABS = 3e-2       # ten times the absolute term of the bound: above it the relative term of the bound has something to work on


def tile_liveness(case: Case, want: dict) -> float:
    '''The smallest fraction, over the output tiles of the case's launch, of elements with |want| >= LIVE_ABS.  In a tile whose reference is
    (nearly) all zero -- behind an activation that flushed it -- no error short of atol shows, a wrong tile index among them.'''
    bm, bn = expected_launch(case).tpl[:2]
    bn = bn // 2 if case.act == ACT_GEGLU else bn
    if case.trans:
        y = want['C'].transpose(2, 3).reshape(case.batch, case.M, case.N)
    elif case.trans_n0:
        y = torch.cat([want['C'], want['C2'].transpose(1, 2).reshape(1, case.M, -1)], dim=2)
    elif case.phase:
        y = phase_slices(case, want['C'])
    else:
        y = want['C']
    live = (y.abs() >= LIVE_ABS).double()
    worst_tile = 1.0
    for z in range(live.shape[0]):
        for m0 in range(0, live.shape[1], bm):
            for n0 in range(0, live.shape[2], bn):
                worst_tile = min(worst_tile, float(live[z, m0:m0 + bm, n0:n0 + bn].mean()))
    return worst_tile


# ------------------------------------------------------------------------------------------------ acceptance
def tolerance(case: Case):
    '''The project's own GEMM bounds (test_gpu_gemm_pp.py, test_gemm_every_tile_and_split): 3e-3 + 3e-3 |want| for fp16 outputs -- the fp16
    rounding of the output (2^-11 relative) plus fp32 accumulation order --, 1e-3 + 1e-3 |want| for fp32 outputs (test_gpu_gemm_pp.py's out_f32 arm).'''
    return (1e-3, 1e-3) if case.out_f32 else (3e-3, 3e-3)


def worst(case: Case, got: dict, want: dict) -> float:
    '''max over the elements of every output of |got - want| / (atol + rtol |want|); inf for a non-finite or missing element.'''
    atol, rtol = tolerance(case)
    w = 0.0
    for key in want:
        if key == 'gn_affine':    # GroupNorm + SiLU of the output: against float64 on the fp16 rows the kernel stored, with the bound of
            # test_groupnorm_fused_into_the_splitk_finish (fp16 in, fp16 out)
            at, rt = 4e-3, 4e-3
            g, t = got['gn_out'].double().cpu(), gn_of(case, got['C'][0], *want[key])
            r = (g - t).abs() / (at + rt * t.abs())
            if not bool(torch.isfinite(r).all()):
                return float('inf')
            w = max(w, float(r.max()))
            continue
        at, rt = atol, rtol
        g, t = got[key].double().cpu(), want[key].double().cpu()
        r = (g - t).abs() / (at + rt * t.abs())
        if not bool(torch.isfinite(r).all()):
            return float('inf')
        w = max(w, float(r.max()))
    return w


def check(case: Case, got: dict, want: dict) -> bool:
    '''|err| <= atol + rtol |want| on EVERY element (not normalised by the global maximum: one row with a neighbour's statistics, one column
    with a neighbour's bias or colsum fails it).'''
    return worst(case, got, want) <= 1.0


def stats_check(case: Case, c16, stats=None, gn_parts=None) -> float:
    '''ln_stats_out / gn_part_out against float64 sums of the fp16-rounded rows the kernel stored (`c16` [batch][M][N]); -> the worst
    err / bound.  Bounds as tests/test_gpu_rowops.py derives them for fd_ln_finalize_stats_f32, from the fp32 arithmetic: a sum of n terms
    accumulated in fp32 in any order is off by at most n 2^-24 sum |x| (squares of fp16 values are exact in fp32).  Raw slabs are such
    sums over n = 160 columns; the finished pairs of the 256x320 tile add the variance's cancellation and the reciprocal square root as
    there, with n = 320 in place of the slab count; a GroupNorm partial sum has n = 256 rows x N / groups columns.'''
    x = c16.double().cpu().reshape(-1, case.N)
    w = 0.0
    if stats is not None:
        st = stats.double().cpu()
        if st.dim() == 3:       # [N / 160][rows][2] raw partial sums
            xs = x.view(x.shape[0], case.N // 160, 160)
            for j, (s, ab) in enumerate(((xs.sum(2), xs.abs().sum(2)), ((xs * xs).sum(2), (xs * xs).sum(2)))):
                err = (st[:, :, j].T - s).abs() / (160 * EPS24 * ab + 1e-30)
                w = max(w, float(err.max()) if bool(torch.isfinite(err).all()) else float('inf'))
        else:
            n = case.N
            mean, s2 = x.mean(1), (x * x).mean(1)
            var = (s2 - mean * mean).clamp(min=0)
            rstd = (var + LN_EPS).rsqrt()
            dvar = (n + 3) * EPS24 * (s2 + mean * mean)
            rel = dvar / (2 * (var + LN_EPS)) + 6 * EPS24
            e0 = (st[:, 0] - rstd).abs() / (rel * rstd)
            wb = -mean * rstd
            e1 = (st[:, 1] - wb).abs() / (rel * wb.abs() + rstd * (n + 2) * EPS24 * x.abs().mean(1))
            for e in (e0, e1):
                w = max(w, float(e.max()) if bool(torch.isfinite(e).all()) else float('inf'))
    if gn_parts is not None:
        G, ns = case.gn_parts, case.M // case.rows
        xs = x.view(ns, case.rows // 256, 256, G, case.N // G)
        n = 256 * (case.N // G)
        gp = gn_parts.double().cpu()
        for j, (s, ab) in enumerate(((xs.sum(dim=(2, 4)), xs.abs().sum(dim=(2, 4))), ((xs * xs).sum(dim=(2, 4)),) * 2)):
            err = (gp[..., j] - s).abs() / (n * EPS24 * ab + 1e-30)
            w = max(w, float(err.max()) if bool(torch.isfinite(err).all()) else float('inf'))
    return w


# ------------------------------------------------------------------------------------------------ device run
def _strided_fill(t, ld, size, fill=PAD_IN, dtype=None):
    '''flat buffer of `size` elements full of `fill` with the rows of t ([rows][cols]) every `ld` elements.'''
    buf = torch.full((size,), fill, dtype=dtype or t.dtype)
    torch.as_strided(buf, tuple(t.shape), (ld, 1)).copy_(t)
    return buf


def host_buffers(case: Case, inp: dict) -> dict:
    '''Flat host buffers of the case's layout: junk (PAD_IN) in every input padding, SENTINEL in every output element.'''
    p, Z, M, N = layout_plan(case), case.batch, case.M, case.N
    h = {}
    a = torch.full((max(Z * p['sA'], p['a_size']),), PAD_IN, dtype=torch.float16)
    w = torch.full((Z * p['sW'],), PAD_IN, dtype=torch.float16)
    for z in range(Z):
        if case.conv and z >= p['ZA']:
            pass
        elif case.conv:
            t = inp['A'][z]
            torch.as_strided(a, tuple(t.shape), (p['Hi'] * p['Wi'] * p['lda'], p['Wi'] * p['lda'], p['lda'], 1), z * p['sA']).copy_(t)
        else:
            torch.as_strided(a, (M, case.K), (p['lda'], 1), z * p['sA']).copy_(inp['A'][z])
        torch.as_strided(w, (N, case.K + case.K2), (p['ldw'], 1), z * p['sW']).copy_(inp['W'][z])
    h['A'], h['W'] = a, w
    nb = inp['bias'].shape[0]
    b = torch.zeros((nb * max(p['sBias'], _r(N, 4)),), dtype=torch.float32)       # (the ABI reads whole float4s: zero up to a multiple of 4)
    torch.as_strided(b, (nb, N), (max(p['sBias'], _r(N, 4)), 1)).copy_(inp['bias'])
    h['bias'] = b
    if case.K2:
        h['A2'] = _strided_fill(inp['A2'], p['lda2'], M * p['lda2'])
    if case.res:
        rr = inp['res'].shape[1]
        r = torch.full((Z * p['sR'],), PAD_IN, dtype=torch.float16)
        for z in range(Z):
            torch.as_strided(r, (rr, N), (p['ldr'], 1), z * p['sR']).copy_(inp['res'][z])
        h['res'] = r
    if case.bias2:
        h['bias2'] = _strided_fill(inp['bias2'], p['ldb2'], inp['bias2'].shape[0] * p['ldb2'])
    if case.ln:
        h['ln_stats'], h['colsum'] = inp['ln_stats'].contiguous().view(-1), inp['colsum']
    for k in ('gn_gamma', 'gn_beta'):
        if k in inp:
            h[k] = inp[k]
    cdt = torch.float32 if case.out_f32 else torch.float16
    h['C'] = torch.full((2 * p['guard'] + (p['ZC'] - 1) * p['sC'] + p['c_len'],), SENTINEL, dtype=cdt)
    if case.trans_n0:
        h['C2'] = torch.full((p['c2_len'] + 16,), SENTINEL, dtype=torch.float16)
    if case.stats_out:
        slabs = 1 if case.N == 320 and expected_launch(case).tpl[1] == 320 else case.N // 160
        h['stats_out'] = torch.full((slabs * Z * M * 2,), SENTINEL, dtype=torch.float32)
    if case.gn_parts:
        h['gn_part'] = torch.full(((M // case.rows) * (case.rows // 256) * case.gn_parts * 2,), SENTINEL, dtype=torch.float32)
    if case.gn_out:
        h['gn_out'] = torch.full((M * N,), SENTINEL, dtype=torch.float16)
    if case.split > 1:
        h['ws'] = torch.full((case.split * M * N,), PAD_IN, dtype=torch.float32)
    return h


def _views(case: Case, p: dict, back: dict) -> dict:
    '''The logical outputs inside the flat buffers copied back from the device.'''
    Z, M, ns = case.batch, case.M, case.M // case.rows
    v = {}
    if case.trans:
        v['C'] = torch.as_strided(back['C'], (Z, ns, case.N, case.rows), (p['sC'], p['sT'], p['ldt'], 1), p['guard'])
    elif case.phase:
        v['C'] = torch.as_strided(back['C'], (1, 4 * M, case.n_out), (0, p['ldc'], 1), p['guard'])
    else:
        v['C'] = torch.as_strided(back['C'], (Z, M, case.trans_n0 if case.trans_n0 else case.n_out), (p['sC'], p['ldc'], 1), p['guard'])
    if case.trans_n0:
        v['C2'] = torch.as_strided(back['C2'], (ns, case.N - case.trans_n0, case.rows), (p['sT'], p['ldt'], 1), 0)
    if case.gn_out:
        v['gn_out'] = back['gn_out'].view(M, case.N)
    return v


def run_on_device(case: Case, dev, inp: Optional[dict] = None):
    '''One fd_gemm_f16 call with the descriptor built by hand -> (outputs as `compute` returns them, plus 'stats' / 'gn_parts' where the case
    asks for them; True when every element of the output buffers outside the logical outputs -- padding columns, guard rows, batch gaps --
    still holds the sentinel, bit for bit, and the inputs' buffers are unchanged).  ValueError where the library refuses.'''
    from flexdiffuse_amd import hip
    inp = inp if inp is not None else inputs(case)
    p = layout_plan(case)
    host = host_buffers(case, inp)
    on = {k: t.to(dev) for k, t in host.items()}
    ptr = {k: t.data_ptr() for k, t in on.items()}
    ptr['C'] += p['guard'] * on['C'].element_size()
    for k in ('bias2', 'res', 'ws', 'ln_stats', 'colsum', 'stats_out', 'A2', 'gn_out', 'gn_gamma', 'gn_beta', 'gn_part', 'C2'):
        ptr.setdefault(k, None)
    d = build_desc(case, p, ptr)
    hip.call('fd_gemm_f16', ctypes.byref(d), hip.stream())
    torch.cuda.synchronize()
    back = {k: on[k].cpu() for k in ('C', 'C2', 'gn_out', 'stats_out', 'gn_part') if k in on}
    views = _views(case, p, back)
    out = {k: v.clone() for k, v in views.items()}
    for v in views.values():
        v.fill_(SENTINEL)
    untouched = all(torch.equal(back[k].view(torch.int32 if back[k].dtype == torch.float32 else torch.int16),
                                torch.full_like(back[k], SENTINEL).view(torch.int32 if back[k].dtype == torch.float32 else torch.int16))
                    for k in ('C', 'C2', 'gn_out') if k in back)
    untouched = untouched and all(torch.equal(on[k].cpu(), host[k]) for k in ('A', 'W', 'res', 'bias') if k in host)
    if case.stats_out:
        st = back['stats_out']
        out['stats'] = st.view(-1, case.batch * case.M, 2) if st.numel() > case.batch * case.M * 2 else st.view(case.batch * case.M, 2)
    if case.gn_parts:
        out['gn_parts'] = back['gn_part'].view(case.M // case.rows, case.rows // 256, case.gn_parts, 2)
    return out, bool(untouched)


def run_and_score(case: Case, dev, env={}, ref=None):
    '''-> one result row: the expected kernel, err / bound of the outputs and of the statistics, untouched.  `ref`: another float64 reference
    than `reference` (tests/conv_cases.py: torch.nn.functional.conv2d).'''
    inp = inputs(case)
    got, untouched = run_on_device(case, dev, inp)
    want = (ref or reference)(case, inp)
    ratio = worst(case, got, want)
    sratio = 0.0
    if case.stats_out or case.gn_parts:
        sratio = stats_check(case, got['C'], got.get('stats'), got.get('gn_parts'))
    L = expected_launch(case, env)
    big = lambda r: r if r != float('inf') else 1e30
    return {'id': case.id, 'kernel': L.kernel, 'tpl': list(L.tpl), 'finish': L.finish, 'ratio': big(ratio), 'stats_ratio': big(sratio),
            'untouched': untouched, 'ok': bool(ratio <= 1.0 and sratio <= 1.0 and untouched)}


# ------------------------------------------------------------------------------------------------ the table
def _slots(BM, BN, EPI=0, NS=2):
    """256 CUs x the workgroups per CU launch_mode reckons with."""
    lds = NS * (BM + BN) * 128 + 16 * BN + (BM * 8 if EPI in (5, 6, 7, 13) else 0)
    return 256 * (1 if (BM >= 256 or lds > 80 * 1024) else 2 if BM * BN >= 128 * 128 else 3 if BM == 128 else 4)


def _persistent_tiles(BM, BN, EPI=0, NS=2, tm_multiple=1):
    """(tiles_m, tiles_n) of a walk of the persistent kernel: at least 9/8 of the slots = 256 x occupancy as launch_mode computes it (an eighth of
    the workgroups walk two tiles, the others one), not a multiple of the slot count, not a multiple of 8 (the XCD remap's r != 0 branch), and a
    column count that does not divide slots / 8 -- a workgroup's second tile is slots / 8 places further in its XCD's chunk, so it lies in
    another tile column than its first and needs another bias."""
    slots = _slots(BM, BN, EPI, NS)
    tn = 3 if (slots // 8) % 3 else 5
    tm = -(-(slots * 9 // 8) // tn)
    while (tm * tn) % 8 == 0 or (tm * tn) % slots == 0 or tm % tm_multiple:
        tm += 1
    return tm, tn


def _hw(rows):
    '''out_h x out_w = rows, as square as it gets.'''
    h = int(rows ** 0.5)
    while rows % h:
        h -= 1
    return h, rows // h


def _conv(rows, K):
    '''a convolution geometry with out_h * out_w = rows and kh * kw * Cin = K: 576 = 3x3 x 64, 192 = 1x3 x 64 (left / right padding), 1152 = 3x3 x 128, 64 = 1x1 x 64.'''
    kh, kw, cin = {576: (3, 3, 64), 192: (1, 3, 64), 1152: (3, 3, 128), 64: (1, 1, 64)}[K]
    return _hw(rows) + (cin, kh, kw, 1)


def _build_table():
    T = []
    seen = set()

    def add(name, tile, M, N, K, **kw):
        assert name not in seen, name
        seen.add(name)
        T.append(Case(name, tile, M, N, K, **kw))

    lin_k = (64, 128, 192, 256, 448)           # 1, 2, 3, 4 and 7 K-tiles, rotated over the linear one-shot cases
    rot = [0]

    def next_k(ns):
        rot[0] += 1
        ks = lin_k if ns == 2 else (64, 192, 448, 128, 320)      # NS = 3: 1, 3, 7 (odd), 2, 5
        return ks[rot[0] % len(ks)]

    # ---- the lean-epilogue tiles: every (EPI, CONV) launch_epi can return, one-shot and (NS == 2, BN != 320) persistent ----
    for tile, (BM, BN, WM, NS, WN, ALLOW) in LEAN.items():
        t = f't{tile}'
        M, N = 2 * BM, 2 * BN
        glu = bool(ALLOW & 8) and (BN // WN // 16) % 2 == 0
        pad = lambda i: 'padded' if (tile + i) % 2 else 'contig'
        crows = BM if BM != 288 else 288            # rows per image of the convolutions: one m-tile
        # one-shot
        add(f'{t}-lin-plain', tile, M, N, next_k(NS), layout=pad(0))                                                     # EPI 1
        add(f'{t}-lin-res', tile, M, N, next_k(NS), res=True, layout=pad(1))                                              # EPI 2
        add(f'{t}-lin-res-wrap', tile, 2 * (288 if BM == 288 else 256), N, next_k(NS), res=True, res_rows=288 if BM == 288 else 256, layout=pad(0))
        add(f'{t}-lin-bias2-tile-edge', tile, M, N, next_k(NS), bias2=True, rps=BM, layout=pad(1))                          # EPI 1, border on a tile edge
        add(f'{t}-lin-bias2-mid-tile', tile, M, N, next_k(NS), bias2=True, rps=BM // 2 if BM != 288 else 96, layout=pad(0))  # EPI 0
        add(f'{t}-lin-alpha-batch2', tile, M, N, next_k(NS), alpha=0.5, batch=2, layout=pad(1))                            # EPI 1, blockIdx.z
        add(f'{t}-lin-batch-bias', tile, M, N, next_k(NS), batch=2, batch_bias=True, res=True, layout=pad(0))              # EPI 2, per-batch bias
        add(f'{t}-lin-silu-res', tile, M, N, next_k(NS), act=ACT_SILU, res=True, alpha=2.0, layout=pad(1))                 # EPI 0 (activation)
        add(f'{t}-lin-f32-gelu', tile, M, N, next_k(NS), act=ACT_GELU, out_f32=True, layout=pad(0))                        # EPI 0 (fp32 output)
        add(f'{t}-lin-ragged', tile, BM + 1, BN + 4, next_k(NS), res=True, layout=pad(1))                                  # EPI 0 (ragged)
        add(f'{t}-lin-ragged2-qgelu', tile, 2 * BM - 1, BN + 4, next_k(NS), act=ACT_QUICK_GELU, bias2=True, rps=0, layout=pad(0))
        for K in (72, 200, 520):
            add(f'{t}-lin-ktail{K}', tile, M, N, K, res=K == 200, layout='padded')                                       # EPI 1 / 2, K % 64 != 0
        add(f'{t}-lin-K2', tile, M, N, 128, K2=64, res=True, layout=pad(1))                                                # appended operand
        add(f'{t}-conv-plain', tile, M, N, 576, conv=_conv(crows, 576), layout=pad(1))                                     # EPI 1 conv
        add(f'{t}-conv-res-bias2', tile, M, N, 192, conv=_conv(crows, 192), res=True, bias2=True, rps=crows, layout=pad(0))  # EPI 2 conv
        add(f'{t}-conv-silu', tile, M, N, 576, conv=_conv(crows, 576), act=ACT_SILU, layout=pad(1))                        # EPI 0 conv
        add(f'{t}-conv-ragged', tile, 2 * BM - 1, BN + 4, 192, conv=_conv(2 * BM - 1, 192), res=True, layout=pad(0))
        if glu:
            add(f'{t}-lin-geglu', tile, M, N, next_k(NS), act=ACT_GEGLU, layout=pad(0))                                   # EPI 3
            add(f'{t}-conv-geglu', tile, M, N, 192, conv=_conv(crows, 192), act=ACT_GEGLU, layout=pad(1))
            add(f'{t}-lin-geglu-ragged', tile, BM + 1, BN + 32, next_k(NS), act=ACT_GEGLU, layout=pad(1))                  # EPI 0 GEGLU
        # LayerNorm fold
        if ALLOW & 32:
            add(f'{t}-ln', tile, M, N, next_k(NS), ln=1, layout=pad(0))                                                  # EPI 5
            add(f'{t}-ln-parts{2 << (tile % 3)}', tile, M, N, 320, ln=2 << (tile % 3), layout=pad(1))                      # EPI 5, statistics from partial sums
            add(f'{t}-ln-ragged', tile, BM + 1, BN + 4, next_k(NS), ln=1, layout=pad(1))                                   # -> <128, 128, ..., 7>
        if ALLOW & 64 and glu:
            add(f'{t}-ln-geglu', tile, M, N, next_k(NS), ln=1, act=ACT_GEGLU, layout=pad(1))                              # EPI 6
        # statistics of the output
        if ALLOW & 256:
            if tile == 16:
                add(f'{t}-stats', tile, M, 320, next_k(NS), stats_out=True, layout=pad(0))                               # EPI 8, finished pairs
                add(f'{t}-stats-res', tile, M, 320, next_k(NS), stats_out=True, res=True, layout=pad(1))                  # EPI 9
                add(f'{t}-stats-res-wrap', tile, M, 320, next_k(NS), stats_out=True, res=True, res_rows=256, layout=pad(0))
            else:
                sm = 5 * 288 if tile == 23 else 512          # (tile 23 is the planned tile only at row counts 9 x 2^k x 5 ...)
                add(f'{t}-stats', tile, sm, 640 if tile != 23 else 320, next_k(NS), stats_out=True, layout=pad(0))       # EPI 8, slabs
                add(f'{t}-stats-res', tile, sm, 640 if tile != 23 else 320, next_k(NS), stats_out=True, res=True, layout=pad(1))   # EPI 9
        if tile == 16:
            add(f'{t}-gnparts-lin', tile, 512, 320, next_k(NS), gn_parts=32, rps=256, bias2=True, layout=pad(0))          # EPI 11
            add(f'{t}-gnparts-conv-res', tile, 512, 320, 576, conv=_conv(256, 576), gn_parts=32, rps=256, res=True, layout=pad(1))   # EPI 12 conv
            add(f'{t}-gnparts-conv', tile, 512, 320, 192, conv=_conv(256, 192), gn_parts=32, rps=256, layout=pad(0))      # EPI 11 conv
            add(f'{t}-gnparts-lin-res', tile, 512, 320, next_k(NS), gn_parts=32, rps=256, res=True, layout=pad(1))        # EPI 12
        # persistent walks (K <= 192)
        if NS == 2 and BN != 320:
            tm, tn = _persistent_tiles(BM, BN)
            PM, PN = tm * BM, tn * BN
            add(f'{t}-walk-lin-plain', tile, PM, PN, 128, layout=pad(0))
            add(f'{t}-walk-lin-res', tile, PM, PN, 192, res=True, layout=pad(1))
            add(f'{t}-walk-lin-bias2', tile, PM, PN, 64, bias2=True, rps=BM, layout=pad(0))                                # EPI 1 -> 0 on the persistent kernel
            add(f'{t}-walk-lin-ragged', tile, PM - 1, PN - BN + 4, 72, act=ACT_SILU, res=True, layout='padded')            # EPI 0, ragged walk
            add(f'{t}-walk-conv-plain', tile, PM, PN, 192, conv=_conv(BM, 192), layout=pad(1))
            add(f'{t}-walk-conv-res', tile, PM, PN, 64, conv=_conv(BM, 64), res=True, layout=pad(0))
            add(f'{t}-walk-conv-silu', tile, PM, PN, 192, conv=_conv(BM, 192), act=ACT_SILU, layout=pad(0))                # EPI 0 conv
            if BM == 256:
                add(f'{t}-walk-lin-res-wrap-alpha', tile, PM, PN, 128, res=True, res_rows=256, alpha=0.5, layout=pad(1))
            if tile in (10, 14):
                add(f'{t}-walk-lin-batch2', tile, PM, PN, 64, batch=2, layout=pad(0))
            if glu:
                add(f'{t}-walk-lin-geglu', tile, PM, PN, 128, act=ACT_GEGLU, layout=pad(1))
                add(f'{t}-walk-conv-geglu', tile, PM, PN, 64, conv=_conv(BM, 64), act=ACT_GEGLU, layout=pad(0))
            if ALLOW & 32:
                tm5, _ = _persistent_tiles(BM, BN, 5)
                add(f'{t}-walk-ln', tile, tm5 * BM, PN, 192, ln=1, layout=pad(0))
            if ALLOW & 64 and glu:
                tm6, _ = _persistent_tiles(BM, BN, 6)
                add(f'{t}-walk-ln-geglu', tile, tm6 * BM, PN, 128, ln=1, act=ACT_GEGLU, layout=pad(1))

    # ---- the generic-only tiles: launch<>, linear and convolution, one-shot and (NS == 2) persistent ----
    for tile, (BM, BN, WM, NS, WN) in GENERIC.items():
        t = f't{tile}'
        M, N = 2 * BM, 2 * BN
        pad = lambda i: 'padded' if (tile + i) % 2 else 'contig'
        add(f'{t}-lin-res', tile, M, N, next_k(NS), res=True, layout=pad(0))
        add(f'{t}-lin-silu-alpha-batch2', tile, M, N, next_k(NS), act=ACT_SILU, alpha=0.5, batch=2, layout=pad(1))
        add(f'{t}-lin-batch-bias', tile, M, N, next_k(NS), batch=2, batch_bias=True, layout=pad(0))
        add(f'{t}-lin-bias2-f32', tile, M, N, next_k(NS), bias2=True, rps=BM, out_f32=True, layout=pad(1))
        add(f'{t}-lin-res-wrap', tile, 512, N, next_k(NS), res=True, res_rows=256, layout=pad(0))
        add(f'{t}-lin-ragged', tile, BM + 1, BN + 4, next_k(NS), res=True, layout=pad(1))
        add(f'{t}-lin-ragged2', tile, 2 * BM - 1, BN + 4, next_k(NS), act=ACT_GELU, bias2=True, rps=BM - 1, layout=pad(0))
        for K in (72, 200, 520):
            add(f'{t}-lin-ktail{K}', tile, M, N, K, res=K == 72, layout='padded')
        add(f'{t}-lin-geglu', tile, M, max(N, 64), next_k(NS), act=ACT_GEGLU, layout=pad(0))      # (plan: 160-wide tiles become 128x128 for GEGLU)
        add(f'{t}-lin-K2', tile, M, N, 64, K2=128, layout=pad(1))
        add(f'{t}-conv-res', tile, M, N, 576, conv=_conv(BM, 576), res=True, layout=pad(0))
        add(f'{t}-conv-bias2-ragged', tile, 2 * BM - 1, BN + 4, 192, conv=_conv(2 * BM - 1, 192), bias2=True, rps=2 * BM - 1, layout=pad(1))
        if NS == 2:
            tm, tn = _persistent_tiles(BM, BN)
            add(f'{t}-walk-lin', tile, tm * BM, tn * BN, 192, res=True, layout=pad(1))
            add(f'{t}-walk-lin-ragged', tile, tm * BM - 1, tn * BN - BN + 4, 72, bias2=True, rps=BM, layout='padded')
            add(f'{t}-walk-conv', tile, tm * BM, tn * BN, 192, conv=_conv(BM, 192), act=ACT_SILU, layout=pad(0))
    # the LayerNorm fold on the generic tiles: <128, 128, ..., 7> and <64, 64, ..., 7> (fd_gemm_plan: -7 / 4), one-shot and persistent
    add('t1-ln', 1, 256, 256, 192, ln=1, layout='padded')
    add('t1-ln-geglu-ragged', 1, 129, 160, 128, ln=1, act=ACT_GEGLU)
    add('t1-ln-parts4', 1, 256, 256, 320, ln=4, layout='padded')
    add('t4-ln', 4, 128, 128, 64, ln=1)
    add('t4-ln-ragged-parts2', 4, 65, 68, 448, ln=2, layout='padded')
    add('t4-ln-geglu', 4, 128, 128, 256, ln=1, act=ACT_GEGLU, layout='padded')
    tm, tn = _persistent_tiles(128, 128, 7)
    add('t1-walk-ln', 1, tm * 128, tn * 128, 128, ln=1)
    add('t1-walk-ln-geglu-ragged', 1, tm * 128 - 1, tn * 128 - 96, 72, ln=1, act=ACT_GEGLU, layout='padded')
    tm, tn = _persistent_tiles(64, 64, 7)
    add('t4-walk-ln', 4, tm * 64, tn * 64, 192, ln=1, layout='padded')

    # ---- transposed stores: 128x64 (2x2 waves) and 128x160 (M >= 8192, 160 | N), plain and with the fold; the transposed tail (EPI 13) ----
    add('vt64-plain', 0, 256, 128, 192, trans=True, rps=128, layout='padded')
    add('vt64-ragged', 0, 2 * 136, 68, 72, trans=True, rps=136, layout='padded')         # rows_per_sample % 8 == 0 but no 32-row blocks inside a sample
    add('vt64-odd-rows', 0, 2 * 77, 128, 128, trans=True, rps=77)                        # scalar stores
    add('vt64-silu-alpha', 0, 256, 128, 128, trans=True, rps=128, act=ACT_SILU, alpha=0.5)
    add('vt64-ln', 0, 256, 128, 128, trans=True, rps=128, ln=1, layout='padded')
    add('vt64-ln-parts2', 0, 256, 128, 320, trans=True, rps=64, ln=2)
    add('vt64-conv', 0, 256, 128, 192, trans=True, rps=128, conv=_conv(128, 192), layout='padded')
    add('vt160-plain', 0, 8192, 160, 64, trans=True, rps=4096, layout='padded')
    add('vt160-two-tiles', 0, 8192, 320, 72, trans=True, rps=1024, layout='padded')
    add('vt160-ln', 0, 8192, 160, 64, trans=True, rps=2048, ln=1, layout='padded')
    add('vt160-ln-contig', 0, 8192, 320, 128, trans=True, rps=8192, ln=1)
    tm, tn = _persistent_tiles(128, 64)        # (5 tile columns, the last one ragged: N = 320 would be a 128x160 launch)
    add('vt64-walk', 0, tm * 128, tn * 64 - 16, 64, trans=True, rps=128, layout='padded')
    add('vt64-walk-conv', 0, tm * 128, tn * 64 - 16, 64, trans=True, rps=128, conv=_conv(128, 64))
    tm, tn = _persistent_tiles(128, 64, 7)
    add('vt64-walk-ln', 0, tm * 128, tn * 64 - 16, 128, trans=True, rps=128, ln=1)
    tm, tn = _persistent_tiles(128, 160, tm_multiple=3)
    add('vt160-walk', 0, tm * 128, tn * 160, 64, trans=True, rps=tm * 128 // 3, layout='padded')
    tm, tn = _persistent_tiles(128, 160, 7, tm_multiple=3)
    add('vt160-walk-ln', 0, tm * 128, tn * 160, 128, trans=True, rps=tm * 128 // 3, ln=1, layout='padded')
    add('tail13-two-samples', 0, 256, 480, 192, trans_n0=320, rps=128, ln=1, layout='padded')
    add('tail13-contig', 0, 256, 480, 64, trans_n0=320, rps=128, ln=1)
    add('tail13-parts2', 0, 384, 480, 320, trans_n0=160, rps=96, ln=2, layout='padded')

    # ---- split-K: 2, 4, 8, 16 slices through k_splitk_finish, rotating the finish pass's operands; K-tile counts that do not divide ----
    add('split2-res', 13, 512, 320, 448, split=2, res=True, layout='padded')                                  # 7 K-tiles: 4 + 3
    add('split4-res-wrap', 9, 512, 320, 576, split=4, res=True, res_rows=128)                                  # 9 K-tiles: 3 + 3 + 3 + 0 (an empty slice)
    add('split8-bias2-silu', 12, 256, 320, 1152, split=8, bias2=True, rps=64, act=ACT_SILU, conv=_conv(64, 1152), layout='padded')   # 18: 3 x 6
    add('split16-f32', 16, 512, 640, 1088, split=16, out_f32=True, alpha=0.5, layout='padded')                 # 17 K-tiles: 2 x 8 + 1 and 7 empty slices
    add('split2-ragged-ktail', 10, 129, 132, 520, split=2, act=ACT_GELU, res=True, layout='padded')            # 9 K-tiles, the last one 8 columns
    add('split4-generic-tile', 5, 512, 320, 1152, split=4, res=True, bias2=True, rps=256, conv=_conv(256, 1152))
    add('split2-3stage', 20, 256, 320, 448, split=2, layout='padded')
    add('split2-3stage-generic', 7, 512, 320, 576, split=2, res=True)
    add('split4-K2', 14, 512, 256, 320, K2=192, split=4, res=True, layout='padded')                            # 8 K-tiles over both operands
    add('split4-empty-slice', 13, 512, 320, 320, split=4, res=True, layout='padded')                           # 5 K-tiles: 2 + 2 + 1 + 0
    add('split2-small-tile', 4, 128, 128, 448, split=2, bias2=True, rps=32)
    add('split8-tile23', 23, 576, 320, 1152, split=8, res=True, conv=_conv(288, 1152), layout='padded')
    add('split2-walk', 10, _persistent_tiles(128, 128)[0] * 128, 384, 192, split=2, res=True)                                        # persistent partial pass (nkt = 1)
    for s in (2, 4, 8, 16):    # k_splitk_finish_gn<S>: one small slab each (2 samples x 64 rows x 320 channels, 32 groups)
        add(f'split{s}-gn', (13, 9, 12, 16)[(2, 4, 8, 16).index(s)], 128, 320, 1152, split=s, gn_out=32, rps=64, conv=_conv(64, 1152),
            bias2=s != 4, res=s >= 8, layout='padded' if s in (2, 8) else 'contig')

    # ---- refused: each is followed by a good call in the GPU test ----
    add('refuse-stats-ragged', 13, 500, 640, 128, stats_out=True)                    # ln_stats_out needs whole 128-row tiles
    add('refuse-gnparts-tile13', 13, 512, 320, 128, gn_parts=32, rps=256)            # gn_part_out needs the row-spanning tile
    add('refuse-gn-unsplit', 13, 128, 320, 1152, gn_out=32, rps=64, conv=_conv(64, 1152))
    add('refuse-res-wrap-mid-tile', 13, 512, 320, 128, res=True, res_rows=128)       # a 256-row tile would straddle the wrap
    add('refuse-geglu-res', 14, 512, 256, 128, act=ACT_GEGLU, res=True)
    add('refuse-tail13-rows', 0, 200, 480, 64, trans_n0=320, rps=100, ln=1)
    return T


CASES = tuple(c._replace(seed=100 + i) for i, c in enumerate(_build_table()))
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), 'case ids must be unique'


def child_cases(env: dict, cases=None):
    '''The cases (of `cases`; default: this table) a child process under `env` runs: those the library still accepts whose expected launch
    the setting changes.'''
    run, skipped = [], []
    for c in (CASES if cases is None else cases):
        if refused(c):
            continue
        if refused(c, env):
            skipped.append(c)
        elif expected_launch(c, env) != expected_launch(c):
            run.append(c)
    return run, skipped


def _child(job: dict, by_id: Optional[dict] = None, ref=None) -> int:
    """Runs, in THIS fresh process (the switches are read once per process), the cases the parent names: job = {'env', 'run': ids whose launch
    the setting changes, 'refuse': ids the setting makes the library refuse (ValueError, each followed by the good call 'good': an id of
    'run')}; one JSON line on stdout.
    (The parent decides, with fd_gemm_plan under the default settings; here fd_gemm_plan itself runs under the setting.)
    `by_id`, `ref`: the table and reference of tests/conv_cases.py, whose own --child entry ends up here."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    env = job['env']
    for name, value in env.items():
        assert os.environ.get(name) == value, f'{name} must be set in the child environment'
    dev = torch.device('cuda:0')
    by_id = by_id if by_id is not None else BY_ID
    rows, refusals = [], []
    for c in (by_id[i] for i in job['refuse']):
        try:
            run_on_device(c, dev)
            refusals.append({'id': c.id, 'refused': False})
        except ValueError:
            refusals.append({'id': c.id, 'refused': True})
        refusals[-1]['good_after'] = run_and_score(by_id[job['good']], dev, env, ref)['ok']
    for c in (by_id[i] for i in job['run']):
        rows.append(run_and_score(c, dev, env, ref))      # (fd_gemm_plan under the setting must not refuse what `select` accepts: ValueError here)
    print(json.dumps({'env': env, 'cases': rows, 'refusals': refusals}), flush=True)
    return 0


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--child', 'usage: gemm_cases.py --child \'{"env": {"FD_GEMM_FAST_EPI": "0"}, "run": [ids], "refuse": [ids], "good": id}\''
    sys.exit(_child(json.loads(sys.argv[2])))
