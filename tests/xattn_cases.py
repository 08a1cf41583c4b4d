'''One table of fd_xattn_q_f16 / fd_xattn_pack_kv_f16 cases (csrc/xattn.hip: `k_xattn<40>`, `k_xattn<80>`, `k_xattn_pack<40|80>`),
a float64 reference on the operands the device receives, a Python restatement of the two packed image layouts and the
acceptance criterion -- shared by tests/test_xattn_cases.py (CPU: the table covers what it promises, `check` accepts an fp32
emulation of the kernel and rejects twelve wrong computations) and tests/test_gpu_xattn.py (MI355X: every case through the C ABI).

Nothing here needs a GPU to import; `run_on_device` is the only part that touches one.

Inputs follow tests/test_gpu_kernels.py::test_fused_q_projection_cross_attention: hidden states with a per-row scale of 0.5..2.5 and
a per-row offset, LayerNorm gain / bias and q weights folded by ops.prep_linear_ln with head_dim^-0.5 log2(e).  One late key of the
first context is scaled by 6 (base-2 logits of several tens: a softmax that is one key wide), every key of the last context by 0.05 (a
near-uniform softmax: there a key too many or too few in the denominator moves every output by 1 / n_keys of its size), and V carries a
per-channel offset of order 1, so that "its size" is not 0.1.  The statistics are handed over as data: finished (rstd, -mean rstd)
pairs, or the producer's partial sums in 2, 4 or 8 slabs; cases of the second kind hold one row whose variance is of the order of the
fold's eps (only there does eps change the result) and one exactly constant row.'''
from __future__ import annotations

import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from attention_cases import ATOL, GUARD_ROWS, JUNK, PAD_IN, QK_LOG2E, RTOL, SENTINEL, check, worst  # noqa: F401  (the criterion is attention's own)

HEADS = 8
KEY_SLOTS = 80                       # 5 key blocks of 16: what the images hold and the kernel contracts over
LAYOUTS = ('contig', 'padded_ld', 'out_slice')
STATS = ('fin', 2, 4, 8)
IMAGE_BYTES = {40: 61440, 80: 102400}   # fd_xattn_image_bytes(8, d): 8 heads x 5 key blocks x (KSF KB + 512 B), K and V^T alike
LOW_VAR_ROW, CONST_ROW = 5, 10       # of the parts cases
ONE_BITS = 0x3C00                    # fp16 1.0


def row_tile(d: int) -> int:
    '''Rows of a workgroup tile (XaCfg<D>::BM).'''
    return {40: 256, 80: 128}[d]


class Case(NamedTuple):
    B: int                    # samples
    HW: int                   # query rows per sample
    rep: int                  # context replicas sharing the queries
    L: int                    # keys
    d: int                    # head dim (8 heads)
    layout: str = 'contig'
    stats: object = 'fin'     # 'fin': finished pairs [M][2]; 2 / 4 / 8: partial slabs [k][M][2]
    eps: float = 0.0          # fd_xattn_desc.ln_fold_eps (0 = 1e-5); only the parts forms read it
    seed: int = 0

    @property
    def id(self) -> str:
        st = 'fin' if self.stats == 'fin' else f'parts{self.stats}' + ('-eps1e-3' if self.eps else '')
        return f'd{self.d}-{self.B}x{self.HW}-rep{self.rep}-L{self.L}-{self.layout}-{st}'

    @property
    def C(self) -> int:
        return HEADS * self.d

    @property
    def M(self) -> int:
        return self.B * self.HW

    @property
    def tiles(self) -> int:
        return self.M // row_tile(self.d)

    @property
    def n_ctx(self) -> int:
        return self.rep * self.B

    @property
    def eff_eps(self) -> float:
        return self.eps if self.eps > 0 else 1e-5


def _both(B, t, rep, L, layout='contig', stats='fin', eps=0.0):
    '''The same case at both head dims; `t` = rows per sample in tiles.'''
    assert layout in LAYOUTS and stats in STATS and eps in (0.0, 1e-3) and (stats != 'fin' or eps == 0.0)
    return [Case(B, t * row_tile(d), rep, L, d, layout, stats, eps) for d in (40, 80)]


_TABLE = (
    # ---- every legal key count on the smallest grid (one tile); layouts, statistics forms and replica counts rotate ---------------
    _both(1, 1, 1, 65) + _both(1, 1, 2, 66, 'padded_ld') + _both(1, 1, 1, 67, 'out_slice', 2) + _both(1, 1, 1, 68, 'contig', 4, 1e-3) +
    _both(1, 1, 1, 69, 'padded_ld', 8) + _both(1, 1, 3, 70, 'out_slice') + _both(1, 1, 1, 71, 'contig', 2, 1e-3) +
    _both(1, 1, 2, 72, 'padded_ld', 4) + _both(1, 1, 1, 73, 'out_slice', 8, 1e-3) + _both(1, 1, 1, 74) + _both(1, 1, 1, 75, 'padded_ld') +
    _both(1, 1, 2, 76, 'out_slice') + _both(1, 1, 3, 77) + _both(1, 1, 1, 78, 'padded_ld', 2, 1e-3) + _both(1, 1, 1, 79, 'out_slice') +
    _both(1, 1, 1, 80) +
    # ---- row-tile counts 3, 8, 9 and 20 (= 8 * 2 + 4), samples of one and of three tiles ------------------------------------------
    _both(3, 1, 1, 77) + _both(1, 3, 1, 66, 'padded_ld', 4) + _both(8, 1, 1, 77, 'out_slice') + _both(3, 3, 2, 79, 'padded_ld', 2, 1e-3) +
    _both(20, 1, 1, 77, 'contig', 8, 1e-3) + _both(2, 1, 3, 65, 'out_slice') + _both(2, 3, 2, 80, 'contig', 4, 1e-3)
)
CASES = tuple(c._replace(seed=300 + i) for i, c in enumerate(_TABLE))
assert len({c.id for c in CASES}) == len(CASES), 'case ids must be unique'


# --------------------------------------------------------------------------------------------------- inputs
def _round8(n: int) -> int:
    return (n + 7) // 8 * 8


def spike_key(case: Case) -> int:
    '''The key of context 0 that is scaled by 6.'''
    return max(case.L - 2, 0)


def partial_sums(x16: torch.Tensor, parts: int) -> torch.Tensor:
    '''[k][M][2] fp32 (sum, sum of squares) over k column slabs of the fp16 rows: what a statistics-emitting producer GEMM writes.'''
    M, C = x16.shape
    xs = x16.double().view(M, parts, C // parts)
    return torch.stack([xs.sum(-1), (xs * xs).sum(-1)], -1).permute(1, 0, 2).contiguous().float()


def inputs(case: Case) -> dict:
    '''Exactly what the device is handed, as host tensors: x16 [M][C], w16 [C][C] (gain and scale folded), bias / colsum fp32 [C],
    stats fp32 ([M][2] finished, or [k][M][2] partial sums), k16 / v16 [rep * B][L][C] (context r * B + b belongs to replica r of
    sample b).'''
    from flexdiffuse_amd import ops
    M, C, d, L = case.M, case.C, case.d, case.L
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn((M, C), generator=g) * (0.5 + torch.rand((M, 1), generator=g) * 2) + torch.randn((M, 1), generator=g) * 1.5
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    wq = torch.randn((C, C), generator=g) * C ** -0.5 * 1.5
    k = torch.randn((case.n_ctx, L, C), generator=g) * 1.2
    v = torch.randn((case.n_ctx, L, C), generator=g) + torch.randn(C, generator=g)
    low = torch.randn(C, generator=g)
    if case.stats != 'fin':
        x[LOW_VAR_ROW] = (low + 2.0) * case.eff_eps ** 0.5
        x[CONST_ROW] = 0.75
    k[0, spike_key(case)] *= 6.0
    if case.n_ctx > 1:
        k[-1] *= 0.05
    x16 = x.half()
    lw = ops.prep_linear_ln(wq * (QK_LOG2E * d ** -0.5), None, gamma, beta, 'cpu')
    if case.stats == 'fin':
        xd = x16.double()
        mean, var = xd.mean(1), xd.var(1, unbiased=False)
        rstd = (var + 1e-5).rsqrt()
        stats = torch.stack([rstd, -mean * rstd], -1).float()
    else:
        stats = partial_sums(x16, case.stats)
    return {'x16': x16, 'w16': lw.w[:, :C].contiguous(), 'bias': lw.bias[:C].clone(), 'colsum': lw.colsum[:C].clone(), 'stats': stats,
            'k16': k.half(), 'v16': v.half()}


# --------------------------------------------------------------------------------------------------- reference, emulation, mutants
MUTANTS = ('drop_last_key', 'pad_keys', 'drop_tail', 'cross_talk', 'swap_heads', 'swap_ntiles', 'replica0', 'prev_sample', 'swap_tiles',
           'stats_row_xor1', 'bias_col_plus1', 'eps_ignored')


def remap(nb: int, b: int, with_r: bool = True) -> int:
    '''Row tile of workgroup b in a grid of nb (the XCD remap of k_xattn); with_r=False: the formula without its remainder term.'''
    q, r, xcd, slot = nb >> 3, nb & 7, b & 7, b >> 3
    if not with_r:
        return xcd * q + slot
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot


def confused_tiles(nb: int):
    '''(right, wrong) tile of the first workgroup that the remap without its remainder term sends elsewhere; None where it sends none.'''
    for b in range(nb):
        if remap(nb, b) != remap(nb, b, False):
            return remap(nb, b), remap(nb, b, False)
    return None


def applies(case: Case, mutant: str) -> bool:
    '''Whether `mutant` is a different computation for this case (decided from the case alone).'''
    return {'drop_last_key': True, 'pad_keys': case.L < KEY_SLOTS, 'drop_tail': True, 'cross_talk': case.d == 40, 'swap_heads': True,
            'swap_ntiles': case.d == 80, 'replica0': case.rep >= 2, 'prev_sample': case.B >= 2,
            'swap_tiles': confused_tiles(case.tiles) is not None, 'stats_row_xor1': True, 'bias_col_plus1': True,
            'eps_ignored': case.stats != 'fin' and case.eps > 0 and case.eps != 1e-5}[mutant]


def finalize(case: Case, stats: torch.Tensor, dtype, eps: Optional[float] = None):
    '''(rstd, -mean rstd) per row in `dtype`: the finished pairs as they are, or fd_ln_finalize_stats_f32's arithmetic (slabs summed in
    their order, var = max(E[x^2] - mean^2, 0)) on the partial sums.'''
    if case.stats == 'fin':
        return stats[:, 0].to(dtype), stats[:, 1].to(dtype)
    eps = case.eff_eps if eps is None else eps
    s = torch.zeros(stats.shape[1:], dtype=dtype)
    for slab in stats:
        s = s + slab.to(dtype)
    inv_n = torch.tensor(1.0 / case.C, dtype=dtype)
    mean = s[:, 0] * inv_n
    var = (s[:, 1] * inv_n - mean * mean).clamp(min=0)
    rstd = (var + torch.tensor(eps, dtype=dtype)).rsqrt()
    return rstd, -mean * rstd


def project(case: Case, inp: dict, dtype=torch.float64, mutant: Optional[str] = None, round_q: bool = True) -> torch.Tensor:
    '''Q [M][C] = acc rstd + (-mean rstd) colsum + bias, ROUNDED TO fp16 as the kernel holds it.  float32: the
    accumulation runs over 64-wide K chunks in reverse order, the fold in fp32.'''
    x, w = inp['x16'].to(dtype), inp['w16'].to(dtype)
    if dtype == torch.float64:
        acc = x @ w.T
    else:
        acc = torch.zeros((case.M, case.C), dtype=dtype)
        for c0 in reversed(range(0, case.C, 64)):
            acc = acc + x[:, c0:c0 + 64] @ w[:, c0:c0 + 64].T
    rstd, mr = finalize(case, inp['stats'], dtype, 1e-5 if mutant == 'eps_ignored' else None)
    if mutant == 'stats_row_xor1':
        pair = torch.arange(case.M) ^ 1
        rstd, mr = rstd[pair], mr[pair]
    bias, cs = inp['bias'].to(dtype), inp['colsum'].to(dtype)
    if mutant == 'bias_col_plus1':
        bias, cs = bias.roll(-1), cs.roll(-1)
    q = acc * rstd[:, None] + (mr[:, None] * cs[None, :] + bias[None, :])
    return q.half() if round_q else q


def _attend(case: Case, q16, k16, v16, dtype, mutant):
    '''[rep][B][HW][8][d]: base-2 softmax over the keys and P V of every (replica, sample, head) at once.  float32: P rounded to
    fp16 before the P V product and before the denominator, as the kernel's MFMA operands are.'''
    B, HW, rep, L, d = case.B, case.HW, case.rep, case.L, case.d
    q = q16.to(dtype).view(B, HW, HEADS, d)
    k = k16.to(dtype).view(rep, B, L, HEADS, d)
    v = v16.to(dtype).view(rep, B, L, HEADS, d)
    if mutant == 'replica0':
        k, v = k[:1].expand(rep, -1, -1, -1, -1), v[:1].expand(rep, -1, -1, -1, -1)
    if mutant == 'prev_sample':
        k, v = k.roll(1, dims=1), v.roll(1, dims=1)
    if mutant == 'swap_ntiles':
        k, v = k.roll(4, dims=3), v.roll(4, dims=3)
    if mutant == 'drop_last_key':
        k, v = k[:, :, :L - 1], v[:, :, :L - 1]
    if mutant == 'pad_keys':
        zeros = torch.zeros((rep, B, KEY_SLOTS - L, HEADS, d), dtype=dtype)
        k, v = torch.cat([k, zeros], 2), torch.cat([v, zeros], 2)
    kk = k
    if mutant == 'drop_tail':
        kk = k.clone()
        if d == 40:
            kk[:, :, :, 0::2, 32:] = 0
            kk[:, :, :, 1::2, :8] = 0
        else:
            kk[..., 64:] = 0
    s = torch.einsum('bqhd,rbkhd->rbhqk', q, kk)
    if mutant == 'cross_talk':
        # the shared fragment of a head pair: A's channels 32..39 | B's channels 0..7 enter BOTH heads' logits
        s = s.clone()
        s[:, :, 0::2] = s[:, :, 0::2] + torch.einsum('bqhd,rbkhd->rbhqk', q[:, :, 1::2, :8], k[:, :, :, 1::2, :8])
        s[:, :, 1::2] = s[:, :, 1::2] + torch.einsum('bqhd,rbkhd->rbhqk', q[:, :, 0::2, 32:], k[:, :, :, 0::2, 32:])
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    if dtype != torch.float64:
        p = p.half().to(dtype)
    o = torch.einsum('rbhqk,rbkhd->rbqhd', p, v) / p.sum(-1).permute(0, 1, 3, 2)[..., None]
    if mutant == 'swap_heads':
        o = o.view(rep, B, HW, HEADS // 2, 2, d).flip(4).reshape(rep, B, HW, HEADS, d)
    return o


def attend(case: Case, inp: dict, dtype=torch.float64, mutant: Optional[str] = None, round_q: bool = True) -> Optional[torch.Tensor]:
    '''[rep * M][C] in `dtype`; None where the mutant does not apply.  round_q=False leaves Q unrounded (only to show why the
    reference rounds it).'''
    assert mutant is None or mutant in MUTANTS
    if mutant is not None and not applies(case, mutant):
        return None
    bm = row_tile(case.d)
    q16 = project(case, inp, dtype, mutant, round_q)
    if mutant == 'prev_sample':     # only the first tile behind each sample border reads the previous sample's images
        o = _attend(case, q16, inp['k16'], inp['v16'], dtype, None).clone()
        o[:, 1:, :bm] = _attend(case, q16, inp['k16'], inp['v16'], dtype, mutant)[:, 1:, :bm]
    else:
        o = _attend(case, q16, inp['k16'], inp['v16'], dtype, mutant)
    out = o.reshape(case.rep, case.M, case.C)
    if mutant == 'swap_tiles':
        a, b = confused_tiles(case.tiles)
        out = out.clone()
        out[:, a * bm:(a + 1) * bm], out[:, b * bm:(b + 1) * bm] = out[:, b * bm:(b + 1) * bm].clone(), out[:, a * bm:(a + 1) * bm].clone()
    return out.reshape(case.rep * case.M, case.C)


def reference(case: Case, inp: Optional[dict] = None) -> torch.Tensor:
    '''float64 on the operands the device receives, Q rounded to fp16: [rep * M][C].'''
    return attend(case, inp if inp is not None else inputs(case), torch.float64)


def emulate(case: Case, inp: dict) -> torch.Tensor:
    '''The kernel's arithmetic in fp32 (reversed K chunks, fp32 fold and finalisation, fp16 Q, fp16 P, fp16 O).'''
    return attend(case, inp, torch.float32).half()


# --------------------------------------------------------------------------------------------------- packed images
@functools.lru_cache(None)
def _k_map(d: int, odd: bool):
    '''half index within one head's K image -> (key slot, channel of the head; -1 = a zero slot), from the comment above k_xattn_pack:
    key block kb (key = kb * 16 + fr, lane = (fr, fq)) = KSF fragments of 8 halfs per lane, then a tail of 4 halfs per lane.'''
    ksf = 1 if d == 40 else 2
    kbh = ksf * 512 + 256
    key, ch = torch.zeros(5 * kbh, dtype=torch.long), torch.full((5 * kbh,), -1, dtype=torch.long)
    for kb in range(5):
        for lane in range(64):
            fr, fq = lane & 15, lane >> 4
            for ks in range(ksf):
                first = (8 if odd else 0) if d == 40 else ks * 32
                for i in range(8):
                    pos = kb * kbh + ks * 512 + lane * 8 + i
                    key[pos] = kb * 16 + fr
                    ch[pos] = first + (fq * 4 + i if i < 4 else 16 + fq * 4 + i - 4)
            for i in range(4):
                pos = kb * kbh + ksf * 512 + lane * 4 + i
                key[pos] = kb * 16 + fr
                if d == 80:
                    ch[pos] = 64 + fq * 4 + i
                elif not odd and fq < 2:
                    ch[pos] = 32 + fq * 4 + i          # A of the pair: its channels 32..39; B's slots stay zero
                elif odd and fq >= 2:
                    ch[pos] = (fq - 2) * 4 + i         # B of the pair: its channels 0..7; A's slots stay zero
    return key, ch


@functools.lru_cache(None)
def _v_map(d: int):
    '''half index within one head's V^T image -> (row = channel; d = the ones-row at head dim 40, beyond = zero, key slot): d-tile dt
    (row = dt * 16 + fr), key groups 0 / 1 of 8 halfs per lane (key blocks 2 kg and 2 kg + 1), key group 2 of 4 halfs (key block 4).'''
    dts = 3 if d == 40 else 5
    row, key = torch.zeros(dts * 1280, dtype=torch.long), torch.zeros(dts * 1280, dtype=torch.long)
    for dt in range(dts):
        for kg in range(3):
            for lane in range(64):
                fr, fq = lane & 15, lane >> 4
                for i in range(4 if kg == 2 else 8):
                    pos = dt * 1280 + kg * 512 + lane * (4 if kg == 2 else 8) + i
                    row[pos] = dt * 16 + fr
                    key[pos] = 64 + fq * 4 + i if kg == 2 else ((2 * kg) * 16 + fq * 4 + i if i < 4 else (2 * kg + 1) * 16 + fq * 4 + i - 4)
    return row, key


def pack_images(k16: torch.Tensor, v16: torch.Tensor, d: int):
    '''K / V [n][L][8 d] fp16 -> (K images, V^T images), each [n][IMAGE_BYTES / 2] int16 (fp16 bit patterns): per context the eight
    heads in order (at head dim 80: n-tile 0 = heads 0..3, n-tile 1 = heads 4..7).  Keys >= L are zero everywhere, ones-row included.'''
    n, L, _ = k16.shape
    kb, vb = k16.view(torch.int16), v16.view(torch.int16)
    kimg, vimg = [], []
    for h in range(HEADS):
        key, ch = _k_map(d, bool(h & 1))
        real = (ch >= 0) & (key < L)
        kimg.append(torch.where(real[None], kb[:, :, h * d:(h + 1) * d][:, key.clamp(max=L - 1), ch.clamp(min=0)], 0))
        row, key = _v_map(d)
        real = (row < d) & (key < L)
        img = torch.where(real[None], vb[:, :, h * d:(h + 1) * d][:, key.clamp(max=L - 1), row.clamp(max=d - 1)], 0)
        if d == 40:
            img = torch.where(((row == d) & (key < L))[None], ONE_BITS, img)
        vimg.append(img)
    kimg, vimg = torch.cat(kimg, 1).to(torch.int16), torch.cat(vimg, 1).to(torch.int16)
    assert kimg.shape[1] * 2 == IMAGE_BYTES[d] and vimg.shape[1] * 2 == IMAGE_BYTES[d]
    return kimg, vimg


def image_reference(case: Case, inp: Optional[dict] = None):
    '''The images fd_xattn_pack_kv_f16 must write for the case's contexts, bit for bit.'''
    inp = inp if inp is not None else inputs(case)
    return pack_images(inp['k16'], inp['v16'], case.d)


# --------------------------------------------------------------------------------------------------- device run
def layout_plan(case: Case) -> dict:
    '''Element strides, offsets and buffer sizes of the three layouts (x, wq rows stay 16-byte aligned, out rows 8-byte aligned).'''
    C, L, M = case.C, case.L, case.M
    p = {'ldx': C, 'ldw': C, 'ldo': C, 'ldk': C, 'ldvt': _round8(L), 'x_off': 0, 'o_off': 0, 'o_tail': 0, 'k_gap': 0, 'vt_gap': 0}
    if case.layout == 'padded_ld':
        p.update(ldx=C + 8, ldw=C + 8, ldo=C + 4, ldk=C + 8, ldvt=_round8(L) + 8, k_gap=3, vt_gap=8)
    elif case.layout == 'out_slice':    # unet.py: out=o[r*B*HW:(r+1)*B*HW]; x = the second half of a twice as wide buffer
        p.update(ldx=2 * C, x_off=C, o_off=GUARD_ROWS * C, o_tail=GUARD_ROWS * C)
    p['sK'] = (L + p['k_gap']) * p['ldk']          # the gap: whole junk rows L .. L + 2 of the sample
    p['sVt'] = C * p['ldvt'] + p['vt_gap']
    p['x_size'], p['w_size'] = M * p['ldx'], C * p['ldw']
    p['k_size'], p['vt_size'] = case.n_ctx * p['sK'], case.n_ctx * p['sVt']
    p['o_size'] = p['o_off'] + case.rep * M * p['ldo'] + p['o_tail']
    return p


def host_buffers(case: Case, inp: dict) -> dict:
    '''Flat host buffers of the case's layout.  Padding columns and gaps of x, wq and K hold PAD_IN; every V^T element that is not
    a (channel, key < L) holds JUNK, the columns L .. round8(L) - 1 included (the packer promises not to read them).'''
    C, L, p = case.C, case.L, layout_plan(case)
    x = torch.full((p['x_size'],), PAD_IN, dtype=torch.float16)
    torch.as_strided(x, (case.M, C), (p['ldx'], 1), p['x_off']).copy_(inp['x16'])
    w = torch.full((p['w_size'],), PAD_IN, dtype=torch.float16)
    torch.as_strided(w, (C, C), (p['ldw'], 1), 0).copy_(inp['w16'])
    k = torch.full((p['k_size'],), PAD_IN, dtype=torch.float16)
    torch.as_strided(k, (case.n_ctx, L, C), (p['sK'], p['ldk'], 1), 0).copy_(inp['k16'])
    vt = torch.full((p['vt_size'],), JUNK, dtype=torch.float16)
    torch.as_strided(vt, (case.n_ctx, C, L), (p['sVt'], p['ldvt'], 1), 0).copy_(inp['v16'].transpose(1, 2))
    o = torch.full((p['o_size'],), SENTINEL, dtype=torch.float16)
    return {'x': x, 'w': w, 'k': k, 'vt': vt, 'o': o}


def pack_on_device(case: Case, dev, host: dict):
    '''One fd_xattn_pack_kv_f16 call into 0xFF-filled image buffers -> (K images, V^T images) as uint8 [rep * B][bytes] on `dev`,
    plus the K / V^T device buffers (kept alive by the caller).'''
    from flexdiffuse_amd import hip
    p = layout_plan(case)
    k, vt = host['k'].to(dev), host['vt'].to(dev)
    kimg = torch.full((case.n_ctx, IMAGE_BYTES[case.d]), 0xFF, dtype=torch.uint8, device=dev)
    vimg = torch.full((case.n_ctx, IMAGE_BYTES[case.d]), 0xFF, dtype=torch.uint8, device=dev)
    hip.call('fd_xattn_pack_kv_f16', k.data_ptr(), vt.data_ptr(), kimg.data_ptr(), vimg.data_ptr(), case.n_ctx, case.L, HEADS, case.d,
             p['ldk'], p['ldvt'], p['sK'], p['sVt'], hip.stream())
    return kimg, vimg, (k, vt)


def build_desc(case: Case, t: dict, stats: torch.Tensor, parts: int):
    '''fd_xattn_desc of the case over the device tensors `t` (x, w, bias, colsum, kimg, vimg, o).'''
    from flexdiffuse_amd import ops
    p = layout_plan(case)
    d = ops.fd_xattn_desc()
    d.x, d.wq, d.bias, d.ln_colsum = t['x'].data_ptr() + 2 * p['x_off'], t['w'].data_ptr(), t['bias'].data_ptr(), t['colsum'].data_ptr()
    d.ln_stats, d.k_image, d.v_image, d.out = stats.data_ptr(), t['kimg'].data_ptr(), t['vimg'].data_ptr(), t['o'].data_ptr() + 2 * p['o_off']
    d.M, d.ldx, d.ldw, d.ldo = case.M, p['ldx'], p['ldw'], p['ldo']
    d.rows_per_sample, d.n_rep, d.n_keys, d.heads, d.head_dim = case.HW, case.rep, case.L, HEADS, case.d
    d.ln_stats_parts, d.ln_fold_eps = parts, case.eps
    return d


def read_output(case: Case, o: torch.Tensor):
    '''(output rows [rep * M][C] on the host, True when every other element of the O buffer is still the sentinel, bit for bit).'''
    p = layout_plan(case)
    back = o.cpu().clone()
    view = torch.as_strided(back, (case.rep * case.M, case.C), (p['ldo'], 1), p['o_off'])
    out = view.clone()
    view.fill_(SENTINEL)
    return out, bool(torch.equal(back.view(torch.int16), torch.full_like(back, SENTINEL).view(torch.int16)))


def run_on_device(case: Case, dev, inp: Optional[dict] = None) -> SimpleNamespace:
    '''Packer and kernel through hip.call with hand-built arguments, so that leading dimensions and base pointers are the case's own:
    out [rep * M][C] and untouched (read_output), kimg / vimg (int16 [rep * B][bytes / 2] on the host), again (the output of a second,
    identical launch into a re-filled buffer) and, for the parts forms, fin (the output of the finished-statistics launch fed by
    ops.ln_finalize_stats with the case's eps).'''
    import ctypes
    from flexdiffuse_amd import hip, ops
    inp = inp if inp is not None else inputs(case)
    host = host_buffers(case, inp)
    kimg, vimg, keep = pack_on_device(case, dev, host)
    t = {'x': host['x'].to(dev), 'w': host['w'].to(dev), 'bias': inp['bias'].to(dev), 'colsum': inp['colsum'].to(dev),
         'kimg': kimg, 'vimg': vimg, 'o': host['o'].to(dev)}
    stats = inp['stats'].to(dev)
    parts = 0 if case.stats == 'fin' else case.stats

    def launch(st, n_parts):
        t['o'].copy_(host['o'])
        d = build_desc(case, t, st, n_parts)
        hip.call('fd_xattn_q_f16', ctypes.byref(d), hip.stream())
        torch.cuda.synchronize()
        return read_output(case, t['o'])

    out, untouched = launch(stats, parts)
    again, untouched2 = launch(stats, parts)
    fin = None
    if parts:
        fin, untouched3 = launch(ops.ln_finalize_stats(stats, case.C, case.eff_eps), 0)
        untouched = untouched and untouched3
    del keep
    return SimpleNamespace(out=out, untouched=untouched and untouched2, again=again, fin=fin,
                           kimg=kimg.cpu().view(torch.int16), vimg=vimg.cpu().view(torch.int16))
