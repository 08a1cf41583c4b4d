'''One table of fd_attention_f16 cases, a Python restatement of its dispatcher, a float64 reference and the
acceptance criterion -- shared by tests/test_attention_cases.py (CPU: the table reaches every launch target and
`check` rejects wrong attention) and tests/test_gpu_attention.py (MI355X: every case through the C ABI).

Nothing here needs a GPU to import.  `run_on_device` (and the `--child` entry at the bottom, one fresh process per
FD_ATTN_* setting) is the only part that touches one.

Inputs follow tests/test_gpu_kernels.py::test_attention / test_attention_prescaled_q: unit normal q, k, v rounded to
fp16, one query row and one late key scaled by 6 (large running-max updates across key tiles), and for prescaled
cases the second half of the last sample's keys scaled by 3 (the lazily advanced maximum is overtaken).  V^T columns
n_k .. round8(n_k) are zero (the ABI's contract) and everything beyond is finite junk that must never be read.'''
from __future__ import annotations

import json
import os
import sys
from typing import NamedTuple, Optional

import torch

QK_LOG2E = 1.4426950408889634
JUNK = 2048.0        # V^T beyond round8(n_k), and the gaps between samples: one such column taken for a key moves O by ~JUNK / n_k
PAD_IN = 100.0       # Q / K padding columns and sample gaps of the strided layouts
SENTINEL = -1234.0   # every byte of the O buffer before the launch
GUARD_ROWS = 5       # out_slice: sentinel rows before and after the output rows
LAZY_CLAMP = 256.0   # 2^LAZY_THR of attention.hip: the largest P the lazy-max kernels form on purpose
LAYOUTS = ('contig', 'merged_qk', 'padded_ld', 'out_slice')
ENV_SETTINGS = ({'FD_ATTN_QT1': '0'}, {'FD_ATTN_QT1': '1'}, {'FD_ATTN_Q2': '0'}, {'FD_ATTN_Q2_64': '0'}, {'FD_ATTN_M32': '0'})


class Case(NamedTuple):
    B: int
    heads: int
    n_q: int
    n_k: int
    d: int
    causal: bool = False
    pre: bool = False
    scale: float = 0.0        # 0 = head_dim^-0.5 (fd_attention_desc.scale = 0)
    layout: str = 'contig'
    seed: int = 0

    @property
    def id(self) -> str:
        return (f'{self.B}x{self.heads}h-{self.n_q}x{self.n_k}-d{self.d}' + ('-causal' if self.causal else '') +
                ('-pre' if self.pre else '') + ('-scale' if self.scale else '') + f'-{self.layout}')

    @property
    def eff_scale(self) -> float:
        return self.scale if self.scale > 0 else self.d ** -0.5


def _c(B, heads, n_q, n_k, d, *flags, layout='contig'):
    '''flags: 'causal', 'pre', 'scale' (= 0.5 * head_dim^-0.5).'''
    assert set(flags) <= {'causal', 'pre', 'scale'} and layout in LAYOUTS
    return Case(B, heads, n_q, n_k, d, 'causal' in flags, 'pre' in flags, 0.5 * d ** -0.5 if 'scale' in flags else 0.0, layout)


_TABLE = [
    # ---- k_attention<96, 6> (head_dim 81..96) and k_attention<128, 8> (97..128): the 4-wave template -------------------------
    _c(2, 3, 129, 65, 88), _c(2, 2, 257, 257, 96, layout='merged_qk'), _c(1, 2, 77, 77, 88, 'causal', layout='padded_ld'),
    _c(2, 2, 200, 136, 96, 'scale', layout='out_slice'), _c(1, 1, 300, 100, 96, 'causal'), _c(1, 1, 17, 8, 88),
    _c(2, 2, 256, 256, 128), _c(1, 3, 130, 130, 104, layout='merged_qk'), _c(2, 1, 100, 77, 128, 'scale', layout='padded_ld'),
    _c(1, 2, 127, 63, 104, layout='out_slice'), _c(1, 2, 64, 200, 120, 'causal'), _c(1, 1, 1, 1, 112),
    # refused: q_prescaled has no kernel at head_dim 81..128
    _c(1, 2, 64, 64, 88, 'pre'), _c(1, 2, 64, 64, 128, 'pre'),
    # ---- k_attention_w8<64, 3, *, true, 1>: head_dim <= 40, denominator from the ones row right after the head ---------------
    _c(2, 4, 129, 65, 8), _c(2, 2, 17, 8, 8, 'pre'), _c(2, 3, 127, 127, 16, 'pre', layout='merged_qk'), _c(1, 2, 64, 63, 16),
    _c(1, 5, 257, 77, 24, layout='padded_ld'), _c(2, 2, 1, 1, 24, 'pre'), _c(2, 2, 256, 320, 32, 'pre', layout='out_slice'),
    _c(1, 2, 2047, 64, 32), _c(2, 8, 256, 77, 40, 'pre'), _c(2, 8, 256, 256, 40, layout='merged_qk'),
    _c(1, 8, 1024, 1024, 40, 'pre', layout='merged_qk'), _c(1, 2, 2047, 1024, 40, 'pre'), _c(1, 2, 2048, 63, 40, 'pre'),
    _c(2, 2, 129, 65, 40, 'scale', layout='padded_ld'), _c(1, 2, 200, 77, 40, 'causal', 'pre'), _c(1, 2, 77, 200, 32, 'causal'),
    # ---- k_attention_w8<64, 3, *, false, 1>: head_dim 41..48 ------------------------------------------------------------------
    _c(2, 2, 130, 200, 48, 'pre'), _c(2, 2, 192, 192, 48, layout='merged_qk'), _c(1, 3, 2047, 65, 48, 'pre', layout='padded_ld'),
    _c(1, 1, 127, 1, 48, layout='out_slice'),
    # ---- k_attention_w8<64, 4, *, false, 1>: head_dim 49..64 ------------------------------------------------------------------
    _c(2, 12, 77, 77, 64, 'causal', layout='merged_qk'), _c(1, 16, 257, 257, 64), _c(2, 2, 129, 8, 56, 'pre', layout='padded_ld'),
    _c(1, 2, 2048, 1023, 64, 'pre'), _c(1, 2, 2047, 1024, 64), _c(2, 2, 100, 100, 64, 'pre', 'scale', layout='out_slice'),
    _c(1, 12, 77, 77, 64, 'causal', 'pre'),
    # ---- k_attention_w8<96, 5, *, false, 1>: head_dim 65..80 ------------------------------------------------------------------
    _c(1, 8, 1024, 1024, 80, 'pre', layout='merged_qk'), _c(1, 8, 2304, 2304, 80, 'pre', layout='merged_qk'),
    _c(1, 8, 1024, 1024, 80), _c(1, 16, 257, 257, 80), _c(2, 2, 129, 65, 72, layout='padded_ld'),
    _c(2, 3, 17, 63, 72, 'pre', layout='out_slice'), _c(1, 2, 250, 250, 80, 'causal', 'scale'),
    # ---- k_attention_w8<160, 10, *, false, 1>: head_dim 129..160 --------------------------------------------------------------
    _c(2, 8, 256, 256, 160, 'pre', layout='merged_qk'), _c(1, 8, 576, 576, 160, 'pre', layout='merged_qk'),
    _c(2, 8, 144, 144, 160, layout='merged_qk'), _c(1, 8, 256, 256, 160), _c(1, 2, 100, 77, 160, 'pre', layout='padded_ld'),
    _c(2, 1, 129, 65, 136, 'scale', layout='out_slice'), _c(1, 3, 127, 1, 152), _c(1, 2, 64, 130, 160, 'causal', 'pre'),
    # ---- k_attention_w8<64, 3, *, true, 2>: n_q >= 2048, n_k >= 64, head_dim <= 40 (40 only when not prescaled) ---------------
    _c(1, 2, 2048, 64, 32, 'pre'), _c(1, 1, 2048, 2048, 40, layout='merged_qk'), _c(2, 2, 2100, 200, 24, layout='padded_ld'),
    _c(2, 1, 2304, 136, 16, 'pre', layout='out_slice'), _c(1, 3, 2048, 64, 8, 'scale'), _c(1, 1, 2500, 2100, 32, 'causal', 'pre'),
    _c(1, 1, 2048, 2300, 40, 'causal'), _c(1, 2, 2048, 1024, 40),
    # ---- k_attention_w8<64, 3, *, false, 2>: head_dim 41..48 ------------------------------------------------------------------
    _c(1, 2, 2200, 1100, 48), _c(2, 2, 2100, 64, 48, 'pre', layout='padded_ld'), _c(2, 1, 2048, 2048, 48, 'pre', layout='merged_qk'),
    _c(1, 1, 2049, 65, 48, 'scale', layout='out_slice'),
    # ---- k_attention_w8<64, 4, *, false, 2>: head_dim 49..64, n_k >= 1024 -----------------------------------------------------
    _c(2, 2, 2304, 2304, 64, 'pre', layout='merged_qk'), _c(2, 2, 2100, 1030, 56, layout='padded_ld'), _c(1, 1, 2048, 1024, 64),
    _c(1, 1, 2048, 2048, 64, 'causal', 'pre', layout='out_slice'), _c(1, 1, 2050, 1024, 56, 'pre', 'scale'),
    # ---- k_attention_w8q2m: head_dim 40, prescaled ----------------------------------------------------------------------------
    _c(1, 2, 2048, 1024, 40, 'pre'), _c(1, 1, 2048, 64, 40, 'pre'), _c(1, 8, 4096, 77, 40, 'pre'),
    _c(2, 2, 2304, 2304, 40, 'pre', layout='merged_qk'), _c(2, 3, 2091, 1093, 40, 'pre', layout='padded_ld'),
    _c(1, 1, 2500, 2500, 40, 'causal', 'pre', layout='out_slice'), _c(1, 1, 2048, 200, 40, 'pre', 'scale'),
    _c(1, 1, 2048, 600, 40, 'causal', 'pre'),
]
CASES = tuple(c._replace(seed=100 + i) for i, c in enumerate(_TABLE))
assert len({c.id for c in CASES}) == len(CASES), 'case ids must be unique'
assert all(c.layout != 'merged_qk' or c.n_q == c.n_k for c in CASES)


# --------------------------------------------------------------------------------------------------- dispatcher
def template_of(name: str) -> str:
    return name.split('<')[0]


def family_of(name: str) -> tuple:
    '''(template, QB): QB, the query blocks per wave, is the last argument of k_attention_w8 and None for the others.'''
    t = template_of(name)
    return t, int(name[:-1].split(', ')[-1]) if t == 'k_attention_w8' else None


def expected_kernel(case: Case, env={}) -> str:
    '''The instantiation fd_attention_f16 launches for `case`, spelled as in the tables of csrc/attention.hip, under the FD_ATTN_* variables in `env`.  ValueError where the library answers FD_ESHAPE.'''
    wide = int(env.get('FD_ATTN_QT1', 2))
    q2 = int(env.get('FD_ATTN_Q2', 1))
    q2_64 = int(env.get('FD_ATTN_Q2_64', 1))
    m32 = int(env.get('FD_ATTN_M32', 1))
    hd, pre = case.d, case.pre
    if hd % 8 or not 8 <= hd <= 160:
        raise ValueError(f'head_dim={hd} unsupported')
    if pre and not (wide == 2 and (hd <= 80 or hd > 128)):
        raise ValueError(f'q_prescaled is not supported for head_dim={hd}')
    p = 'true' if pre else 'false'

    def old(dqk, dv):
        return f'k_attention<{dqk}, {dv}, 1, 8>' if wide else f'k_attention<{dqk}, {dv}>'

    if 48 < hd <= 64 and wide == 2 and q2 and q2_64 and case.n_q >= 2048 and case.n_k >= 1024:
        return f'k_attention_w8<64, 4, {p}, false, 2>'
    if hd <= 48 and wide == 2 and q2 and case.n_q >= 2048 and case.n_k >= 64:
        if hd == 40 and pre and m32:
            return 'k_attention_w8q2m'
        return f'k_attention_w8<64, 3, {p}, {"true" if hd <= 40 else "false"}, 2>'
    if hd <= 48:
        return f'k_attention_w8<64, 3, {p}, {"true" if hd <= 40 else "false"}, 1>' if wide == 2 else old(64, 3)
    if hd <= 64:
        return f'k_attention_w8<64, 4, {p}, false, 1>' if wide == 2 else old(64, 4)
    if hd <= 80:
        return f'k_attention_w8<96, 5, {p}, false, 1>' if wide == 2 else old(96, 5)
    if hd <= 96:
        return 'k_attention<96, 6>'
    if hd <= 128:
        return 'k_attention<128, 8>'
    return f'k_attention_w8<160, 10, {p}, false, 1>' if wide == 2 else old(160, 10)


def refused(case: Case, env={}) -> bool:
    try:
        expected_kernel(case, env)
        return False
    except ValueError:
        return True


def grid_size(case: Case, env={}) -> int:
    rows = 256 if family_of(expected_kernel(case, env)) in (('k_attention_w8', 2), ('k_attention_w8q2m', None)) else 128
    return -(-case.n_q // rows) * case.heads * case.B


# --------------------------------------------------------------------------------------------------- inputs, reference
def _rnd(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def spike_rows(case: Case):
    '''(query row, key row) of sample 0 that are scaled by 6.'''
    return min(3, case.n_q - 1), max(case.n_k - 2, 0)


def inputs(case: Case) -> dict:
    '''q16 / k16 / v16: the fp16 tensors handed to the kernel ([B][n][C]; q16 carries scale * log2(e) for prescaled
    cases); q, k, v: the float64 values the reference sees (exactly what the fp16 inputs encode).'''
    B, C = case.B, case.heads * case.d
    q, k, v = _rnd((B, case.n_q, C), case.seed), _rnd((B, case.n_k, C), case.seed + 1000), _rnd((B, case.n_k, C), case.seed + 2000)
    qi, ki = spike_rows(case)
    q[0, qi] *= 6.0
    k[0, ki] *= 6.0
    if case.pre:
        k[B - 1, case.n_k // 2:] *= 3.0
        f = case.eff_scale * QK_LOG2E
        q16 = (q * f).half()
        qd = q16.double() / f
    else:
        q16 = q.half()
        qd = q16.double()
    k16, v16 = k.half(), v.half()
    return {'q16': q16, 'k16': k16, 'v16': v16, 'q': qd, 'k': k16.double(), 'v': v16.double()}


MUTANTS = ('drop_last_key', 'drop_tile', 'causal_off_by_one', 'junk_column', 'scale_3pct', 'swap_heads', 'clamped_spike')


def _head(q, k, v, case: Case, b: int, mutant: Optional[str]):
    '''softmax(scale q k^T [+ causal mask]) v of one (sample, head): q [n_q][d], k / v [n_k][d] -> [n_q][d], or None
    where the mutant does not apply to this head.'''
    n_q, n_k = q.shape[0], k.shape[0]
    scale = case.eff_scale * (1.03 if mutant == 'scale_3pct' else 1.0)
    key = torch.arange(n_k)
    if mutant == 'drop_last_key':
        k, v, key = k[:-1], v[:-1], key[:-1]
    elif mutant == 'drop_tile':
        j = ((n_k + 63) // 64) // 2          # an interior 64-key tile: neither the first nor the (ragged) last
        keep = (key < 64 * j) | (key >= 64 * j + 64)
        k, v, key = k[keep], v[keep], key[keep]
    elif mutant == 'junk_column':
        # key index round8(n_k): K has no such row (the staging reads zero there), V^T holds the junk
        k = torch.cat([k, torch.zeros_like(k[:1])])
        v = torch.cat([v, torch.full_like(v[:1], JUNK)])
        key = torch.cat([key, key.new_tensor([(n_k + 7) // 8 * 8])])
    s = (q @ k.T) * scale
    if case.causal:
        row = torch.arange(n_q)[:, None] + (1 if mutant == 'causal_off_by_one' else 0)
        s = s.masked_fill(key[None, :] > row, float('-inf'))
    if mutant == 'clamped_spike':
        ki = spike_rows(case)[1]
        if b != 0 or n_k < 2:
            return None
        others = s.clone()
        others[:, ki] = float('-inf')
        m = others.max(dim=1, keepdim=True).values
        u = (s - m).exp()
        p_true = u / u.sum(1, keepdim=True)
        u[:, ki] = u[:, ki].clamp(max=LAZY_CLAMP)
        p = u / u.sum(1, keepdim=True)
        # it is a mutant only where the clamp moves a tenth of some row's probability mass
        if not bool(((p_true[:, ki] - p[:, ki]).abs() >= 0.1).any()):
            return None
        return p @ v
    return s.softmax(-1) @ v


def applies(case: Case, mutant: str) -> bool:
    '''Whether `mutant` is a different computation for this case at all (decided from the case alone; clamped_spike
    additionally looks at the scores, see _head).'''
    seen = case.n_k if not case.causal else min(case.n_k, case.n_q)     # keys some query attends to
    tile = ((case.n_k + 63) // 64) // 2
    # under the causal mask the last key (and the junk column behind it) is a different computation only where rows
    # behind it exist: n_q > n_k.  With n_q == n_k it reaches the last row alone, at a weight of about 1 / n_k; there the
    # edge mutant is causal_off_by_one
    behind = not case.causal or case.n_q > _round8(case.n_k)
    return {'drop_last_key': case.n_k >= 2 and (not case.causal or case.n_q > case.n_k),
            'drop_tile': case.n_k > 128 and seen >= 64 * tile + 64,
            'causal_off_by_one': case.causal and case.n_k >= 2,
            'junk_column': behind, 'scale_3pct': case.n_k >= 2, 'swap_heads': case.heads >= 2,
            'clamped_spike': case.n_k >= 2}[mutant]


def attend(case: Case, inp: dict, dtype=torch.float64, mutant: Optional[str] = None):
    '''[B][n_q][C] attention of `inp` in `dtype`, one (sample, head) at a time; None where the mutant does not apply.'''
    assert mutant is None or mutant in MUTANTS
    if mutant is not None and not applies(case, mutant):
        return None
    B, H, d = case.B, case.heads, case.d
    out = torch.empty((B, case.n_q, H * d), dtype=dtype)
    hit = mutant != 'clamped_spike'
    for b in range(B):
        for h in range(H):
            sl = slice(h * d, h * d + d)
            q, k, v = (inp[n][b][:, sl].to(dtype) for n in ('q', 'k', 'v'))
            o = _head(q, k, v, case, b, mutant)
            if o is None:
                o = _head(q, k, v, case, b, None)
            else:
                hit = True
            out[b, :, sl] = o
    if mutant == 'swap_heads':
        out[:, :, :2 * d] = torch.cat([out[:, :, d:2 * d], out[:, :, :d]], dim=-1)
    return out if hit else None


def reference(case: Case, inp: Optional[dict] = None):
    '''float64 attention of the fp16-rounded inputs: [B][n_q][C].'''
    return attend(case, inp if inp is not None else inputs(case), torch.float64)


# --------------------------------------------------------------------------------------------------- acceptance
ATOL = RTOL = 4e-3


def worst(got, want) -> float:
    '''max over elements of |got - want| / (4e-3 + 4e-3 |want|); inf for a non-finite element.'''
    got, want = got.double().cpu(), want.double().cpu()
    r = (got - want).abs() / (ATOL + RTOL * want.abs())
    if not bool(torch.isfinite(r).all()):
        return float('inf')
    return float(r.max())


def check(got, want) -> bool:
    '''The project's attention bound (test_attention, test_attention_prescaled_q): |err| <= 4e-3 + 4e-3 |want| on every
    element.  It is not loosened for the head dims this table adds: the error terms are the fp16 rounding of each P
    (relative 2^-11, averaged by the fp32 P.V sum), of the ones-row denominator built from the same P, and of the
    stored O (relative 2^-11 = 4.9e-4), none of which grows with head_dim; short heads (8..24) only shorten the fp32
    dot product behind each score.'''
    return worst(got, want) <= 1.0


# --------------------------------------------------------------------------------------------------- device run
def _round8(n: int) -> int:
    return (n + 7) // 8 * 8


def layout_plan(case: Case) -> dict:
    '''Element strides and buffer sizes of the four layouts (all offsets keep the 16-byte alignment of Q, K and V^T
    rows and the 8-byte alignment of O rows that the ABI asks for).'''
    C, n_q, n_k, B = case.heads * case.d, case.n_q, case.n_k, case.B
    nk8 = _round8(n_k)
    p = {'ldq': C, 'ldk': C, 'ldo': C, 'ldvt': nk8 + 8, 'k_off': 0, 'o_off': 0, 'merged': False}
    if case.layout == 'merged_qk':      # unet.py: q, k = qk[:, :C], qk[:, C:]
        p.update(ldq=2 * C, ldk=2 * C, k_off=C, merged=True)
    elif case.layout == 'padded_ld':
        p.update(ldq=C + 8, ldk=C + 16, ldo=C + 12, ldvt=nk8 + 24)
    p['sQ'], p['sK'], p['sO'], p['sVt'] = n_q * p['ldq'], n_k * p['ldk'], n_q * p['ldo'], C * p['ldvt']
    if case.layout == 'padded_ld':
        p['sQ'] += 16
        p['sK'] += 24
        p['sO'] += 4
        p['sVt'] += 8
    p['q_size'], p['k_size'], p['vt_size'], p['o_size'] = B * p['sQ'], B * p['sK'], B * p['sVt'], B * p['sO']
    if case.layout == 'out_slice':      # unet.py: out=o[r*B*HW:(r+1)*B*HW]
        p['o_off'] = GUARD_ROWS * C
        p['o_size'] += 2 * GUARD_ROWS * C
    return p


def host_buffers(case: Case, inp: dict) -> dict:
    '''Flat fp16 host buffers of the case's layout: 'q', 'k' (the same tensor for merged_qk), 'vt', 'o'.'''
    B, C, p = case.B, case.heads * case.d, layout_plan(case)
    q = torch.full((p['q_size'],), PAD_IN, dtype=torch.float16)
    k = q if p['merged'] else torch.full((p['k_size'],), PAD_IN, dtype=torch.float16)
    torch.as_strided(q, (B, case.n_q, C), (p['sQ'], p['ldq'], 1), 0).copy_(inp['q16'])
    torch.as_strided(k, (B, case.n_k, C), (p['sK'], p['ldk'], 1), p['k_off']).copy_(inp['k16'])
    vt = torch.full((p['vt_size'],), JUNK, dtype=torch.float16)
    v = torch.as_strided(vt, (B, C, p['ldvt']), (p['sVt'], p['ldvt'], 1), 0)
    v[:, :, :_round8(case.n_k)] = 0
    v[:, :, :case.n_k] = inp['v16'].transpose(1, 2)
    o = torch.full((p['o_size'],), SENTINEL, dtype=torch.float16)
    return {'q': q, 'k': k, 'vt': vt, 'o': o}


def run_on_device(case: Case, dev, inp: Optional[dict] = None):
    '''One fd_attention_f16 call with the descriptor built by hand -> (O as [B][n_q][C] on the host, True when every
    element of the O buffer outside the [n_q][head_dim * heads] rows is still the sentinel, bit for bit).'''
    import ctypes
    from flexdiffuse_amd import hip, ops
    inp = inp if inp is not None else inputs(case)
    B, C, p = case.B, case.heads * case.d, layout_plan(case)
    host = host_buffers(case, inp)
    q = host['q'].to(dev)
    k = q if p['merged'] else host['k'].to(dev)
    vt, o = host['vt'].to(dev), host['o'].to(dev)
    d = ops.fd_attention_desc()
    d.Q, d.K, d.Vt, d.O = q.data_ptr(), k.data_ptr() + 2 * p['k_off'], vt.data_ptr(), o.data_ptr() + 2 * p['o_off']
    d.ldq, d.ldk, d.ldvt, d.ldo = p['ldq'], p['ldk'], p['ldvt'], p['ldo']
    d.q_sample_stride, d.k_sample_stride, d.vt_sample_stride, d.o_sample_stride = p['sQ'], p['sK'], p['sVt'], p['sO']
    d.batch, d.heads, d.n_q, d.n_k, d.head_dim = B, case.heads, case.n_q, case.n_k, case.d
    d.causal, d.scale, d.q_prescaled = int(case.causal), case.scale, int(case.pre)
    hip.call('fd_attention_f16', ctypes.byref(d), hip.stream())
    torch.cuda.synchronize()
    back = o.cpu()
    view = torch.as_strided(back, (B, case.n_q, C), (p['sO'], p['ldo'], 1), p['o_off'])
    out = view.clone()
    view.fill_(SENTINEL)
    untouched = bool(torch.equal(back.view(torch.int16), torch.full_like(back, SENTINEL).view(torch.int16)))
    return out, untouched


def _child(env: dict) -> int:
    '''Runs, in THIS fresh process (the FD_ATTN_* variables are read once per process), every case whose kernel the
    setting changes; one JSON line on stdout.'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    for name, value in env.items():
        assert os.environ.get(name) == value, f'{name} must be set in the child environment'
    dev = torch.device('cuda:0')
    rows, skipped = [], []
    for case in CASES:
        if refused(case) or (not refused(case, env) and expected_kernel(case, env) == expected_kernel(case)):
            continue
        if refused(case, env):
            skipped.append(case.id)
            continue
        inp = inputs(case)
        got, untouched = run_on_device(case, dev, inp)
        ratio = worst(got, reference(case, inp))
        rows.append({'id': case.id, 'kernel': expected_kernel(case, env), 'ratio': ratio if ratio != float('inf') else 1e30,
                     'ok': bool(ratio <= 1.0 and untouched)})
    print(json.dumps({'env': env, 'cases': rows, 'skipped': skipped}), flush=True)
    return 0


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--child', 'usage: attention_cases.py --child \'{"FD_ATTN_QT1": "0"}\''
    sys.exit(_child(json.loads(sys.argv[2])))
