'''One table of cases per layout / gather / elementwise entry point of csrc/elementwise.hip, the inputs, a plain torch reference on the
CPU and the acceptance criterion -- shared by tests/test_layout_cases.py (CPU: the tables cover what they promise, `check` accepts an
fp32 emulation of every kernel and rejects a list of wrong computations) and tests/test_gpu_layout.py (MI355X: every case through the
C ABI, plan replay, refusals).

Nothing here needs a GPU to import; `run_on_device` is the only function that touches one.

Most of these kernels move data or do one or two correctly rounded operations, so their contract is BITS: the integer view of the
output equals the integer view of the reference (where the reference is NaN only NaN-ness is compared).  Three have a bound instead
(DESIGN.md 3.10): the affine of fd_nhwc_f32_to_nchw_f32 (may be one FMA or two roundings), the exp form of fd_axpby_f32 (the device's
expf is another implementation than the host's) and fd_conv3x3_narrow_f16 (36 fp32 additions in the kernel's order).

How a case is run (`stage`, `collect`, `run_on_device`):
  * every output lies in a buffer that is longer (GUARD elements before and behind) and, where the entry point takes a leading
    dimension, wider than the output; the buffer starts as the sentinel PAD, and after the launch everything outside the output must
    still hold the bits it had (`untouched`), while an element inside that was not written fails the comparison with the reference;
  * input padding that the contract says is never read holds NaN;
  * inputs must hold their bits after the launch, and a second identical launch must give the same bits.'''
from __future__ import annotations

import collections
import functools
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

PAD = 7.5                     # what output buffers hold before a launch (fp16 and fp32 alike)
GUARD = 64                    # elements before and behind every output (a multiple of 8: 16-byte alignment survives)
LIMIT_BYTES = 128 << 20       # no buffer of any case is larger
VAE_SCALE = 0.18215
SIGMA = 14.6146               # the largest sigma of the SD 1.x noise schedule

# entry point -> its kernel; kernel -> the block cap of its fd_grid1d(total, cap) call (None: one block per row / no grid-stride cap)
KERNEL = collections.OrderedDict([
    ('fd_cast_f16_to_f32', 'k_cast_back'), ('fd_cast_f32_to_f16', 'k_cast'), ('fd_nchw_f32_to_nhwc_f16', 'k_nchw_to_nhwc'),
    ('fd_nhwc_f32_to_nchw_f32', 'k_nhwc_to_nchw'), ('fd_im2col_f16', 'k_im2col'), ('fd_concat_channels_f16', 'k_concat'),
    ('fd_copy2d_f16', 'k_copy2d'), ('fd_repeat_rows_f16', 'k_repeat_rows'), ('fd_axpby_f32', 'k_axpby'),
    ('fd_embed_tokens_f16', 'k_embed_tokens'), ('fd_vit_assemble_f16', 'k_vit_assemble'), ('fd_region_blend_f32', 'k_region_blend'),
    ('fd_conv3x3_narrow_f16', 'k_conv3x3_narrow')])
ENTRY_POINTS = tuple(KERNEL)
CAP = {'k_nchw_to_nhwc': 4096, 'k_nhwc_to_nchw': 4096, 'k_im2col': 8192, 'k_concat': 8192, 'k_copy2d': 8192, 'k_repeat_rows': 8192,
       'k_axpby': 2048, 'k_cast': 4096, 'k_cast_back': 4096}
BLOCK = 256


def cap_items(entry: str) -> Optional[int]:
    '''Work items (elements or 16-byte granules) one trip of the entry point's grid-stride loop covers at most; None: no cap.'''
    cap = CAP.get(KERNEL[entry])
    return None if cap is None else cap * BLOCK


class Case(NamedTuple):
    entry: str
    tag: str
    p: SimpleNamespace
    seed: int

    @property
    def id(self) -> str:
        return f'{self.entry[3:]}-{self.tag}'


class Ptr(NamedTuple):
    '''A pointer argument: `off` elements into the flat buffer `buf` of the staged case.'''
    buf: str
    off: int = 0


# --------------------------------------------------------------------------------------------------- the rounding-boundary set
@functools.lru_cache(None)
def boundary_set() -> torch.Tensor:
    '''fp32 inputs that decide fp32 -> fp16 rounding: for every pair of adjacent finite halves of either sign the two halves, their
    midpoint (exact in fp32: a tie) and the fp32 neighbour on each side of it; then the overflow threshold (65504, the largest fp32
    below 65520, 65520 = the tie that rounds to inf), +-inf, NaN, +-0 and values below 2^-25 (half of the smallest subnormal).'''
    pos = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.float16).float()     # +0 .. 65504, rising
    mid = ((pos[:-1].double() + pos[1:].double()) / 2).float()
    assert torch.equal(mid.double(), (pos[:-1].double() + pos[1:].double()) / 2)
    inf = torch.tensor(float('inf'))
    below, above = torch.nextafter(mid, -inf), torch.nextafter(mid, inf)
    half_side = torch.cat([pos, mid, below, above])
    extra = torch.tensor([65504.0, 65519.996, 65520.0, float('inf'), float('-inf'), float('nan'), 0.0, -0.0,
                          2.0 ** -26, -2.0 ** -26, 1e-30, -1e-30, 2.0 ** -149, 2.0 ** -25, -2.0 ** -25], dtype=torch.float32)
    return torch.cat([half_side, -half_side, extra])


def _rand(case_or_seed, *shape, scale=1.0, dtype=torch.float32, salt=0):
    seed = case_or_seed.seed if isinstance(case_or_seed, Case) else case_or_seed
    g = torch.Generator().manual_seed(seed * 16 + salt)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def bits_equal(got: torch.Tensor, want: torch.Tensor) -> bool:
    '''Same dtype, shape and bits; where `want` is NaN only NaN-ness is compared.'''
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not want.is_floating_point():
        return bool(torch.equal(got, want))
    nan = torch.isnan(want)
    return bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(_bits(got)[~nan], _bits(want)[~nan]))


# --------------------------------------------------------------------------------------------------- the tables
def _cases(entry, rows):
    return [Case(entry, tag, SimpleNamespace(**p), 0) for tag, p in rows]


def _table():
    t = []
    # ---- casts: every half bit pattern / the rounding-boundary set, and cap + 5 elements
    t += _cases('fd_cast_f16_to_f32', [('all-patterns', dict(n=65536, data='all')), ('cap+5', dict(n=4096 * BLOCK + 5, data='rand'))])
    t += _cases('fd_cast_f32_to_f16', [('boundary', dict(n=boundary_set().numel(), data='boundary')),
                                       ('cap+5', dict(n=4096 * BLOCK + 5, data='rand'))])
    # ---- NCHW fp32 -> NHWC fp16: (B, C, HW, rep, c_pad)
    nb = boundary_set().numel()
    rows = [((3, 4, 64, 1, 4), VAE_SCALE, 'rand'), ((2, 3, 35, 3, 8), 0.5, 'rand'), ((1, 1, 1, 1, 1), VAE_SCALE, 'rand'),
            ((2, 4, 4097, 2, 8), 0.5, 'rand'), ((1, 8, (nb + 7) // 8, 2, 8), 1.0, 'boundary'),
            ((1, 5, 131073, 2, 8), VAE_SCALE, 'rand')]            # 131073 * 8 = cap * 256 + 8 work items, odd HW
    t += _cases('fd_nchw_f32_to_nhwc_f16', [(f'{"x".join(map(str, s))}-{data}-s{scale:g}',
                                             dict(B=s[0], C=s[1], HW=s[2], rep=s[3], c_pad=s[4], scale=scale, data=data))
                                            for s, scale, data in rows])
    # ---- NHWC fp32 -> NCHW fp32 with affine and clamp: (B, C, HW, ld) x (a, b) x clamp01
    rows = []
    for s in ((2, 4, 64, 4), (3, 3, 35, 8), (1, 1, 1, 1)):
        for a, b in ((1.0, 0.0), (0.5, 0.5), (1 / VAE_SCALE, 0.0), (-2.0, 3.0)):
            for clamp in (0, 1):
                rows.append((s, a, b, clamp))
    rows += [((1, 3, 349527, 4), 0.5, 0.5, 1), ((1, 3, 349527, 4), 1 / VAE_SCALE, 0.0, 0)]     # 3 * 349527 = cap * 256 + 5
    t += _cases('fd_nhwc_f32_to_nchw_f32', [(f'{"x".join(map(str, s))}-a{a:.4g}-b{b:g}-clamp{clamp}',
                                             dict(B=s[0], C=s[1], HW=s[2], ld=s[3], a=a, b=b, clamp=clamp)) for s, a, b, clamp in rows])
    # ---- im2col
    def im(B, Hi, Wi, Cin, Ho, Wo, KH, KW, stride, pt, pl, k_pad):
        return dict(B=B, Hi=Hi, Wi=Wi, Cin=Cin, Ho=Ho, Wo=Wo, KH=KH, KW=KW, stride=stride, pad_t=pt, pad_l=pl, k_pad=k_pad)
    t += _cases('fd_im2col_f16', [
        ('conv_in-3x3-s1-p1-cin4', im(2, 8, 8, 4, 8, 8, 3, 3, 1, 1, 1, 40)),
        ('vae-3x3-s2-p0-asym', im(2, 8, 10, 8, 4, 5, 3, 3, 2, 0, 0, 72)),            # rows / columns 8 / 10 are read: outside
        ('clip-14x14-s14-cin3', im(2, 28, 42, 3, 2, 3, 14, 14, 14, 0, 0, 592)),
        ('1x1', im(2, 5, 7, 16, 5, 7, 1, 1, 1, 0, 0, 16)),
        ('1x3-pad0,1', im(2, 5, 9, 8, 5, 9, 1, 3, 1, 0, 1, 32)),
        ('cin1', im(2, 6, 7, 1, 6, 7, 3, 3, 1, 1, 1, 16)),
        ('B3', im(3, 5, 6, 4, 5, 6, 3, 3, 1, 1, 1, 40)),
        ('cap', im(1, 229, 229, 4, 229, 229, 3, 3, 1, 1, 1, 40))])                      # 229^2 * 40 = cap * 256 + 488
    # ---- concat: (M, Ca, Cb); a zero-width half is legal
    t += _cases('fd_concat_channels_f16', [(f'{M}x{Ca}+{Cb}', dict(M=M, Ca=Ca, Cb=Cb)) for M, Ca, Cb in
                                           ((5, 8, 8), (77, 320, 640), (1, 1280, 8), (64, 8, 1280), (3, 0, 16), (3, 16, 0),
                                            (17477, 320, 640))])                        # 17477 * 120 = cap * 256 + 88 granules
    # ---- copy2d / repeat_rows: (rows, cols, lds, s_off, ldd, d_off[, rep])
    shapes = [('dense', (16, 64, 64, 0, 64, 0)), ('lds', (16, 64, 72, 0, 64, 0)), ('ldd', (16, 64, 64, 0, 80, 0)),
              ('both', (16, 64, 72, 0, 80, 0)), ('slices', (9, 64, 192, 64, 136, 8)), ('row1', (1, 320, 328, 0, 320, 0)),
              ('cols8', (300, 8, 16, 8, 24, 8)), ('cap', (52429, 320, 328, 0, 328, 0))]            # 52429 * 40 = cap * 256 + 8 granules
    t += _cases('fd_copy2d_f16', [(n, dict(rows=s[0], cols=s[1], lds=s[2], s_off=s[3], ldd=s[4], d_off=s[5], rep=1)) for n, s in shapes])
    reps = {'dense': 2, 'lds': 3, 'ldd': 1, 'both': 2, 'slices': 3, 'row1': 2, 'cols8': 3, 'cap': 3}
    t += _cases('fd_repeat_rows_f16', [(f'{n}-rep{reps[n]}', dict(rows=s[0], cols=s[1], lds=s[2], s_off=s[3], ldd=s[4], d_off=s[5],
                                                                 rep=reps[n])) for n, s in shapes])
    # ---- axpby, plain form: n x coefficient pairs (the pipeline's), y == NULL, out aliasing x; then the exp form
    def ax(n, a, b, y=True, alias=False, exp=False):
        return dict(n=n, a=a, b=b, y=y, alias=alias, exp=exp)
    t += _cases('fd_axpby_f32', [
        ('n1-add_noise', ax(1, 1.0, SIGMA)), ('n255-unscale-ynull', ax(255, 1 / VAE_SCALE, 0.0, y=False)),
        ('n256-x0', ax(256, 1.0, -SIGMA)), ('n257-derivative', ax(257, 1 / SIGMA, -1 / SIGMA)),
        ('n256-negzero-ynull', ax(256, 1.0, 0.0, y=False)), ('n257-alias', ax(257, 1.0, -SIGMA, alias=True)),
        ('n300-alias-ynull', ax(300, VAE_SCALE, 0.0, y=False, alias=True)),
        ('cap+3', ax(2048 * BLOCK + 3, 1.0, SIGMA)),
        ('exp-n65539', ax(65539, 0.0, 1.0, exp=True)), ('exp-n1000-b0.7', ax(1000, 0.0, 0.7, exp=True))])
    # ---- gathers: (B, L, D, vocab) and (B, T, D)
    t += _cases('fd_embed_tokens_f16', [(f'{B}x{L}x{D}-v{V}', dict(B=B, L=L, D=D, vocab=V)) for B, L, D, V in
                                        ((3, 77, 768, 1000), (1, 1, 8, 2), (2, 5, 257, 50), (2, 77, 1024, 300))])
    t += _cases('fd_vit_assemble_f16', [(f'{B}x{T}x{D}', dict(B=B, T=T, D=D)) for B, T, D in
                                        ((3, 257, 1024), (1, 2, 8), (2, 50, 768), (4, 5, 257))])
    # ---- region blend on a 4 x 13 x 17 canvas: (oy, ox, sh, sw)
    boxes = [('inside', (3, 4, 5, 6)), ('far-bottom', (8, 2, 5, 4)), ('far-right', (2, 11, 4, 6)), ('clip-bottom', (10, 3, 6, 5)),
             ('clip-right', (1, 14, 3, 9)), ('clip-both', (11, 15, 8, 8)), ('whole', (0, 0, 13, 17)), ('1x1', (6, 9, 1, 1)),
             ('origin-at-edge', (13, 0, 2, 2)), ('origin-beyond', (3, 20, 2, 2)), ('sh0', (2, 2, 0, 5)), ('sw-3', (2, 2, 4, -3))]
    t += _cases('fd_region_blend_f32', [(f'{n}-w{w:g}', dict(C=4, H=13, W=17, oy=b[0], ox=b[1], sh=b[2], sw=b[3], blend=w))
                                        for n, b in boxes for w in (0.0, 1.0, 0.37, 1.5)])
    # ---- narrow conv: (B, Cin, H, W, Cout, rep2)
    rows = [((1, 1, 5, 7, 8, 0), True), ((2, 2, 1, 9, 64, 1), True), ((1, 4, 9, 1, 320, 0), True), ((1, 4, 2, 1024, 8, 0), True),
            ((1, 3, 3, 5, 2048, 2), True), ((2, 4, 6, 300, 24, 0), True), ((1, 3, 4, 6, 16, 1), False)]
    t += _cases('fd_conv3x3_narrow_f16', [(f'{"x".join(map(str, s))}{"" if bias else "-nobias"}',
                                           dict(B=s[0], Cin=s[1], H=s[2], W=s[3], Cout=s[4], rep2=s[5], bias=bias, scale=0.5))
                                          for s, bias in rows])
    return tuple(c._replace(seed=500 + i) for i, c in enumerate(t))


CASES = _table()
assert len({c.id for c in CASES}) == len(CASES), 'case ids must be unique'


def cases_of(entry: str):
    return [c for c in CASES if c.entry == entry]


def work_items(case: Case) -> Optional[int]:
    '''What the entry point hands to fd_grid1d as `total`: elements, or 16-byte granules for the uint4 kernels.'''
    p, e = case.p, case.entry
    if e in ('fd_cast_f16_to_f32', 'fd_cast_f32_to_f16', 'fd_axpby_f32'):
        return p.n
    if e == 'fd_nchw_f32_to_nhwc_f16':
        return p.B * p.HW * p.c_pad
    if e == 'fd_nhwc_f32_to_nchw_f32':
        return p.B * p.C * p.HW
    if e == 'fd_im2col_f16':
        return p.B * p.Ho * p.Wo * p.k_pad
    if e == 'fd_concat_channels_f16':
        return p.M * (p.Ca + p.Cb) // 8
    if e in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        return p.rows * (p.cols // 8)
    return None


def blend_box(p):
    '''(sh, sw) after the clip at the far edges; (0, 0) where nothing is left.'''
    sh, sw = min(p.sh, p.H - p.oy), min(p.sw, p.W - p.ox)
    return (sh, sw) if sh > 0 and sw > 0 else (0, 0)


# --------------------------------------------------------------------------------------------------- inputs
def _affine_edges(a32: float, b32: float) -> torch.Tensor:
    '''fp32 x whose affine image lies on, a few fp32 steps beside and far outside both clamp edges.  Beside the edge 0 of an affine
    with b == 0 "a few steps" are small NORMAL numbers: the contract says nothing about subnormal results.'''
    inf = torch.tensor(float('inf'))
    out = []
    for edge in (0.0, 1.0):
        x0 = torch.tensor((edge - b32) / a32, dtype=torch.float32)
        out.append(x0)
        if float(x0) == 0.0:
            out += [torch.tensor(v, dtype=torch.float32) for v in (1e-30, -1e-30, 2.0 ** -120, -2.0 ** -120)]
            continue
        up, dn = x0.clone(), x0.clone()
        for _ in range(3):
            up, dn = torch.nextafter(up, inf), torch.nextafter(dn, -inf)
            out += [up, dn]
    out += [torch.tensor(v, dtype=torch.float32) for v in (1e6, -1e6, 37.5, -37.5, 0.0, -0.0)]
    return torch.stack(out)


def inputs(case: Case) -> dict:
    '''The logical operands of the case as host tensors (dense; `stage` puts them into padded buffers).'''
    p, e = case.p, case.entry
    if e == 'fd_cast_f16_to_f32':
        if p.data == 'all':
            return {'x': torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)}
        return {'x': _rand(case, p.n, scale=3.0, dtype=torch.float16)}
    if e == 'fd_cast_f32_to_f16':
        return {'x': boundary_set().clone() if p.data == 'boundary' else _rand(case, p.n, scale=3.0)}
    if e == 'fd_nchw_f32_to_nhwc_f16':
        n = p.B * p.C * p.HW
        if p.data == 'boundary':
            s = boundary_set()
            x = s.repeat((n + s.numel() - 1) // s.numel())[:n].clone()
        else:
            x = _rand(case, n, scale=6.0)
        return {'x': x.view(p.B, p.C, p.HW)}
    if e == 'fd_nhwc_f32_to_nchw_f32':
        x = _rand(case, p.B * p.HW * p.C, scale=2.0)
        edges = _affine_edges(float(_f32(p.a)), float(_f32(p.b)))
        k = min(edges.numel(), x.numel())
        x[:k] = edges[:k]
        if x.numel() > 2 * edges.numel():          # and once more at the far end: another sample, another channel
            x[-edges.numel():] = edges
        return {'x': x.view(p.B, p.HW, p.C)}
    if e == 'fd_im2col_f16':
        return {'x': _rand(case, p.B, p.Hi, p.Wi, p.Cin, dtype=torch.float16)}
    if e == 'fd_concat_channels_f16':
        return {'a': _rand(case, p.M, p.Ca, dtype=torch.float16), 'b': _rand(case, p.M, p.Cb, dtype=torch.float16, salt=1)}
    if e in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        return {'src': _rand(case, p.rows, p.cols, dtype=torch.float16)}
    if e == 'fd_axpby_f32':
        if p.exp:
            g = torch.Generator().manual_seed(case.seed)
            x = torch.rand(p.n, generator=g) * 60 - 30
            y = torch.randn(p.n, generator=g)
            x[:4] = torch.tensor([0.0, -0.0, 30.0, -30.0])
            y[4:8] = torch.tensor([0.0, -0.0, 1.0, -1.0])
            return {'x': x, 'y': y}
        x = _rand(case, p.n, scale=1.5)
        if p.n > 8:
            x[3], x[4], x[5] = -0.0, 0.0, 1e-30
        inp = {'x': x}
        if p.y:
            y = _rand(case, p.n, salt=1)
            a32, b32 = _f32(p.a), _f32(p.b)
            if p.n > 64 and float(b32) != 0.0:     # pairs whose terms cancel to a few ulp: y = -(a x) / b, moved by 0 .. 3 steps
                k = min(p.n // 2, 4096)
                yc = -(a32 * x[:k]) / b32
                for step in range(1, 4):
                    yc[step::4] = torch.nextafter(yc[step::4], torch.tensor(float('inf')))
                    if step > 1:
                        yc[step::4] = torch.nextafter(yc[step::4], torch.tensor(float('inf')))
                y[:k] = yc
            inp['y'] = y
        return inp
    if e == 'fd_embed_tokens_f16':
        g = torch.Generator().manual_seed(case.seed)
        ids = torch.randint(0, p.vocab, (p.B * p.L,), generator=g)
        tok = _rand(case, p.vocab, p.D, dtype=torch.float16, salt=1)
        pos = _rand(case, p.L, p.D, dtype=torch.float16, salt=2)
        tok[1] = (_rand(case, p.D, salt=3) * 2.0 ** -20).half()          # the fp32 sum with a pos row of size 100 rounds
        l_big = p.L - 1
        pos[l_big] = (100 + _rand(case, p.D, salt=4)).half()
        special = [0, p.vocab - 1, p.vocab - 1, 0]
        if ids.numel() >= 16:
            special += [-1, -5, p.vocab, p.vocab + 7, 1 << 40, -(1 << 40), 7 % p.vocab, 7 % p.vocab]
        ids[:len(special)] = torch.tensor(special)[:ids.numel()]
        ids[l_big] = 1                                                     # row (b = 0, l = l_big): the tiny row on the big one
        if p.B > 1:
            ids[p.L + l_big] = p.vocab - 1
        return {'ids': ids.view(p.B, p.L), 'tok': tok, 'pos': pos}
    if e == 'fd_vit_assemble_f16':
        return {'patches': _rand(case, p.B * (p.T - 1), p.D, dtype=torch.float16), 'cls': _rand(case, p.D, dtype=torch.float16, salt=1),
                'pos': _rand(case, p.T, p.D, dtype=torch.float16, salt=2)}
    if e == 'fd_region_blend_f32':
        dst = _rand(case, p.C, p.H, p.W)
        src = torch.full((p.C, p.H, p.W), float('nan'))
        sh, sw = blend_box(p)
        src[:, p.oy:p.oy + sh, p.ox:p.ox + sw] = _rand(case, p.C, sh, sw, salt=1)
        return {'dst': dst, 'src': src}
    if e == 'fd_conv3x3_narrow_f16':
        w = torch.zeros((p.Cout, 3, 3, 4), dtype=torch.float16)
        w[..., :p.Cin] = _rand(case, p.Cout, 3, 3, p.Cin, scale=0.4, dtype=torch.float16, salt=1)
        inp = {'x': _rand(case, p.B, p.Cin, p.H, p.W, scale=2.0), 'w': w}
        if p.bias:
            inp['bias'] = _rand(case, p.Cout, salt=2)
        return inp
    raise KeyError(e)


# --------------------------------------------------------------------------------------------------- reference, emulations, mutants
MUTANTS = {
    'fd_cast_f16_to_f32': ('one_trip',),
    'fd_cast_f32_to_f16': ('truncate', 'one_trip'),
    'fd_nchw_f32_to_nhwc_f16': ('scale_after_rounding', 'pad_nonzero', 'replica1_unwritten', 'one_trip'),
    'fd_nhwc_f32_to_nchw_f32': ('row_stride_c', 'clamp_first', 'one_trip'),
    'fd_im2col_f16': ('swap_kh_kw', 'pad_t_both', 'drop_sample', 'pad_unwritten', 'one_trip'),
    'fd_concat_channels_f16': ('swap_halves', 'b_stride_ca', 'one_trip'),
    'fd_copy2d_f16': ('swap_ld', 'one_trip'),
    'fd_repeat_rows_f16': ('swap_ld', 'one_trip', 'replica1_unwritten'),
    'fd_axpby_f32': ('fma', 'ynull_passthrough', 'one_trip'),
    'fd_embed_tokens_f16': ('pos_by_row', 'clamp_off_by_one'),
    'fd_vit_assemble_f16': ('patch_b_t',),
    'fd_region_blend_f32': ('convex', 'no_right_clip'),
    'fd_conv3x3_narrow_f16': ('taps_transposed', 'clamp_to_edge', 'replica_differs'),
}


def applies(case: Case, mutant: str) -> bool:
    '''Whether `mutant` is a different computation for this case (decided from the case alone).'''
    p, e = case.p, case.entry
    if mutant == 'one_trip':
        return work_items(case) > cap_items(e) and not (e == 'fd_axpby_f32' and p.exp)
    if mutant == 'replica1_unwritten':
        return p.rep >= 2
    if mutant == 'truncate':
        return True
    if e == 'fd_nchw_f32_to_nhwc_f16':
        return {'scale_after_rounding': p.scale not in (1.0, 0.5) and p.B * p.C * p.HW >= 64,      # a power of two commutes with the rounding
                'pad_nonzero': p.c_pad > p.C}[mutant]
    if e == 'fd_nhwc_f32_to_nchw_f32':
        return {'row_stride_c': p.ld > p.C and p.B * p.HW > 1, 'clamp_first': bool(p.clamp) and (p.a, p.b) != (1.0, 0.0) and p.B * p.HW * p.C > 8}[mutant]
    if e == 'fd_im2col_f16':
        return {'swap_kh_kw': p.KH * p.KW > 1, 'pad_t_both': p.pad_t != p.pad_l, 'drop_sample': p.B > 1,
                'pad_unwritten': p.k_pad > p.KH * p.KW * p.Cin}[mutant]
    if e == 'fd_concat_channels_f16':
        return {'swap_halves': p.Ca > 0 and p.Cb > 0, 'b_stride_ca': p.Ca != p.Cb and p.Cb > 0 and p.M > 1}[mutant]
    if e in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        return p.lds != p.ldd and p.rows > 1
    if e == 'fd_axpby_f32':
        return {'fma': not p.exp and p.y and p.n > 64, 'ynull_passthrough': not p.exp and not p.y and p.a == 1.0 and p.n > 8}[mutant]
    if e == 'fd_embed_tokens_f16':
        return {'pos_by_row': p.B > 1, 'clamp_off_by_one': p.B * p.L >= 16}[mutant]
    if e == 'fd_vit_assemble_f16':
        return p.B > 1
    if e == 'fd_region_blend_f32':
        sh, sw = blend_box(p)
        return {'convex': p.blend not in (0.0, 1.0) and sh > 0, 'no_right_clip': sh > 0 and p.ox + p.sw > p.W}[mutant]
    if e == 'fd_conv3x3_narrow_f16':
        return {'taps_transposed': True, 'clamp_to_edge': True, 'replica_differs': p.rep2 > 0}[mutant]
    raise KeyError((e, mutant))


def _one_trip(out: torch.Tensor, case: Case, width: int, per_item: int = 1) -> torch.Tensor:
    '''`out` ([rows][width], row-major work order) with everything behind the first trip of the grid-stride loop left as PAD.'''
    flat = out.clone().reshape(-1)
    flat[cap_items(case.entry) * per_item:] = PAD
    return flat.view(out.shape)


def im2col_index(p, swap=False, pad_t_both=False, drop_sample=False):
    '''(flat index into x [B][Hi][Wi][Cin], valid) for every element of out [B Ho Wo][k_pad]: k = (kh KW + kw) Cin + ci.'''
    m, k = torch.arange(p.B * p.Ho * p.Wo)[:, None], torch.arange(p.k_pad)[None, :]
    ox, oy, b = m % p.Wo, (m // p.Wo) % p.Ho, m // (p.Wo * p.Ho)
    ci, tap = k % p.Cin, k // p.Cin
    kh, kw = tap // p.KW, tap % p.KW
    if swap:
        kh, kw = kw, kh
    if drop_sample:
        b = b * 0
    iy, ix = oy * p.stride + kh - p.pad_t, ox * p.stride + kw - (p.pad_t if pad_t_both else p.pad_l)
    valid = (k < p.KH * p.KW * p.Cin) & (iy >= 0) & (iy < p.Hi) & (ix >= 0) & (ix < p.Wi)
    idx = ((b * p.Hi + iy) * p.Wi + ix) * p.Cin + ci
    return idx.clamp(0, p.B * p.Hi * p.Wi * p.Cin - 1), valid


def _conv_patches(case: Case, xh: torch.Tensor, edge: bool = False) -> torch.Tensor:
    '''[B H W][3][3][4] of the rounded input `xh` [B][Cin][H][W] (any float dtype), zero (edge: replicated) border.'''
    p = case.p
    x4 = torch.zeros((p.B, 4, p.H, p.W), dtype=xh.dtype)
    x4[:, :p.Cin] = xh
    xp = F.pad(x4, (1, 1, 1, 1), mode='replicate' if edge else 'constant')
    cols = [xp[:, :, ky:ky + p.H, kx:kx + p.W] for ky in range(3) for kx in range(3)]       # 9 x [B][4][H][W]
    return torch.stack(cols, -1).permute(0, 2, 3, 4, 1).reshape(p.B * p.H * p.W, 3, 3, 4)


def compute(case: Case, inp: dict, mode: str = 'ref', mutant: Optional[str] = None) -> SimpleNamespace:
    '''The output of the case as the reference (`mode='ref'`), as an fp32 emulation in the kernel's own operation order ('emu'; 'emu2'
    where the kernel has a second legal form) or as a wrong computation (`mutant`).  Returns value (what the output view holds, rows
    of all replicas / both outputs concatenated) and, for the three bounded contracts, the float64 reference and the bound.'''
    p, e = case.p, case.entry
    assert mutant is None or (mutant in MUTANTS[e] and applies(case, mutant)), (case.id, mutant)
    ns = SimpleNamespace(value=None, exact=None, bound=None)

    if e == 'fd_cast_f16_to_f32':
        ns.value = inp['x'].float().view(-1, 1)
        if mutant == 'one_trip':
            ns.value = _one_trip(ns.value, case, 1)
    elif e == 'fd_cast_f32_to_f16':
        x = inp['x']
        if mutant == 'truncate':
            h = x.half()
            over = (h.float().abs() > x.abs()) & torch.isfinite(x)       # rounded away from zero: one bit pattern back
            ns.value = torch.where(over, _bits(h) - 1, _bits(h)).to(torch.int16).view(torch.float16).view(-1, 1)
        else:
            ns.value = x.half().view(-1, 1)
        if mutant == 'one_trip':
            ns.value = _one_trip(ns.value, case, 1)
    elif e == 'fd_nchw_f32_to_nhwc_f16':
        x = inp['x']
        h = (x.half().float() * _f32(p.scale)).half() if mutant == 'scale_after_rounding' else (x * _f32(p.scale)).half()
        out = torch.full((p.B, p.HW, p.c_pad), PAD if mutant == 'pad_nonzero' else 0.0, dtype=torch.float16)
        out[:, :, :p.C] = h.permute(0, 2, 1)
        ns.value = out.repeat(p.rep, 1, 1).reshape(-1, p.c_pad)
        if mutant == 'replica1_unwritten':
            ns.value[p.B * p.HW:2 * p.B * p.HW] = PAD
        if mutant == 'one_trip':       # all replicas of a work item are written by the thread that owns it
            flat = ns.value.view(p.rep, -1)
            flat[:, cap_items(e):] = PAD
    elif e == 'fd_nhwc_f32_to_nchw_f32':
        x = inp['x']
        a32, b32 = _f32(p.a), _f32(p.b)
        if mutant == 'row_stride_c':
            flat = stage(case, inp).bufs['x']
            x = torch.as_strided(flat, (p.B, p.HW, p.C), (p.HW * p.C, p.C, 1))
        xa = x.double() * a32.double()
        ex = xa + b32.double()
        ns.exact = (ex.clamp(0, 1) if p.clamp else ex).permute(0, 2, 1).reshape(-1, 1)
        ns.bound = (2.0 ** -24 * (xa.abs() + ex.abs()) * (1 + 2.0 ** -20)).permute(0, 2, 1).reshape(-1, 1)
        if mutant == 'clamp_first':
            v = x.clamp(0, 1) * a32 + b32
        elif mode == 'emu2':           # one FMA
            v = ex.float()
            if p.clamp:
                v = v.clamp(0, 1)
        else:                          # two roundings
            v = x * a32 + b32
            if p.clamp:
                v = v.clamp(0, 1)
        ns.value = v.permute(0, 2, 1).reshape(-1, 1).contiguous()
        if mode == 'ref' and mutant is None:
            ns.value = None
        if mutant == 'one_trip':
            ns.value = _one_trip(ns.value, case, 1)
    elif e == 'fd_im2col_f16':
        idx, valid = im2col_index(p, mutant == 'swap_kh_kw', mutant == 'pad_t_both', mutant == 'drop_sample')
        v = torch.where(valid, _bits(inp['x']).reshape(-1)[idx], torch.zeros((), dtype=torch.int16)).view(torch.float16)
        if mutant == 'pad_unwritten':
            v[:, p.KH * p.KW * p.Cin:] = PAD
        ns.value = _one_trip(v, case, p.k_pad) if mutant == 'one_trip' else v
    elif e == 'fd_concat_channels_f16':
        a, b = inp['a'], inp['b']
        if mutant == 'b_stride_ca':
            m, c = torch.arange(p.M)[:, None], torch.arange(p.Cb)[None, :]
            b = b.reshape(-1)[(m * p.Ca + c) % b.numel()]
        v = torch.cat([b, a] if mutant == 'swap_halves' else [a, b], 1)
        ns.value = _one_trip(v, case, p.Ca + p.Cb, 8) if mutant == 'one_trip' else v
    elif e in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        src = inp['src']
        if mutant == 'swap_ld':
            flat = stage(case, inp).bufs['src']
            r, c = torch.arange(p.rows)[:, None], torch.arange(p.cols)[None, :]
            src = flat[(p.s_off + r * p.ldd + c) % flat.numel()]
        if mutant == 'one_trip':
            src = _one_trip(src, case, p.cols, 8)
        ns.value = src.repeat(p.rep, 1)
        if mutant == 'replica1_unwritten':
            ns.value[p.rows:2 * p.rows] = PAD
    elif e == 'fd_axpby_f32':
        x = inp['x']
        a32, b32 = _f32(p.a), _f32(p.b)
        y = inp['y'] if p.y else torch.zeros_like(x)
        if p.exp:
            ex = torch.exp(0.5 * x.double()) * y.double() * b32.double()
            ns.exact, ns.bound = ex.view(-1, 1), (exp_form_k() * 2.0 ** -24 * ex.abs()).view(-1, 1)
            ns.value = None if mode == 'ref' else (torch.exp(_f32(0.5) * x) * y * b32).view(-1, 1)
        else:
            if mutant == 'fma':
                v = ((a32 * x).double() + b32.double() * y.double()).float()       # fma(b, y, a x)
            elif mutant == 'ynull_passthrough':
                v = a32 * x
            else:
                v = a32 * x + b32 * y          # torch evaluates the two products and the sum as three fp32 operations
            ns.value = v.view(-1, 1)
            if mutant == 'one_trip':
                ns.value = _one_trip(ns.value, case, 1)
    elif e == 'fd_embed_tokens_f16':
        ids, tok, pos = inp['ids'].reshape(-1), inp['tok'], inp['pos']
        row = ids.clamp(0, p.vocab - 1)
        if mutant == 'clamp_off_by_one':
            row = torch.where(ids >= p.vocab, torch.tensor(max(p.vocab - 2, 0)), row)
            row = torch.where(ids < 0, torch.tensor(min(1, p.vocab - 1)), row)
        l = torch.arange(p.B * p.L) % p.L
        if mutant == 'pos_by_row':
            l = torch.arange(p.B * p.L).clamp(max=p.L - 1)
        ns.value = (tok[row].float() + pos[l].float()).half()
    elif e == 'fd_vit_assemble_f16':
        row = torch.arange(p.B * p.T)
        t, b = row % p.T, row // p.T
        src = (b * (p.T if mutant == 'patch_b_t' else p.T - 1) + t - 1).clamp(0, p.B * (p.T - 1) - 1)
        v = torch.where((t == 0)[:, None], inp['cls'].float()[None, :], inp['patches'].float()[src])
        ns.value = (v + inp['pos'].float()[t]).half()
    elif e == 'fd_region_blend_f32':
        d, s, w = inp['dst'].clone(), inp['src'], _f32(p.blend)
        sh, sw = blend_box(p)
        if mutant == 'no_right_clip':
            i = torch.arange(p.C * sh * p.sw)
            xx, yy, c = i % p.sw, (i // p.sw) % sh, i // (p.sw * sh)
            at = (((c * p.H + p.oy + yy) * p.W + p.ox + xx) % d.numel()).unique()
            flat = d.view(-1)
            flat[at] = flat[at] + w * (s.reshape(-1)[at] - flat[at])
        elif sh > 0:
            db, sb = d[:, p.oy:p.oy + sh, p.ox:p.ox + sw], s[:, p.oy:p.oy + sh, p.ox:p.ox + sw]
            d[:, p.oy:p.oy + sh, p.ox:p.ox + sw] = ((_f32(1.0) - w) * db + w * sb) if mutant == 'convex' else db + w * (sb - db)
        ns.value = d.view(-1, p.W)
    elif e == 'fd_conv3x3_narrow_f16':
        xh = (inp['x'] * _f32(p.scale)).half()
        M = p.B * p.H * p.W
        bias = inp['bias'] if p.bias else torch.zeros(p.Cout)
        w = inp['w'].transpose(1, 2) if mutant == 'taps_transposed' else inp['w']
        pd = _conv_patches(case, xh.double(), mutant == 'clamp_to_edge').reshape(M, 36)
        wd = w.double().reshape(p.Cout, 36)
        if mode == 'ref' or mutant in ('taps_transposed', 'clamp_to_edge'):
            y = (pd @ wd.T + bias.double()[None, :])
        else:                         # fp32 accumulation from the bias, tap by tap in (ky, kx, ci) order
            pf, wf = pd.float(), wd.float()
            y = bias[None, :].repeat(M, 1)
            for t in range(36):
                y = y + pf[:, t:t + 1] * wf[None, :, t]
        if mutant is None:
            ref_pd = pd if mode == 'ref' else _conv_patches(case, xh.double()).reshape(M, 36)
            ns.exact = (ref_pd @ wd.T + bias.double()[None, :]).repeat(1 + p.rep2, 1)
            mag = bias.double().abs()[None, :] + ref_pd.abs() @ wd.abs().T
            ns.bound = (2.0 ** -11 * ns.exact[:M].abs() + 36 * 2.0 ** -24 * mag * (1 + 2.0 ** -10) + 2.0 ** -25).repeat(1 + p.rep2, 1)
        else:
            r = compute(case, inp, 'ref')
            ns.exact, ns.bound = r.exact, r.bound
        ns.value = None if mode == 'ref' and mutant is None else y.half().repeat(1 + p.rep2, 1)
        if mutant == 'replica_differs':    # the last replica one bit pattern off in one element
            _bits(ns.value)[-1, -1] += 1
    else:
        raise KeyError(e)
    return ns


def reference(case: Case, inp: Optional[dict] = None) -> SimpleNamespace:
    '''What `check` compares with: `value` (bit contracts) or `exact` and `bound` (float64, the bounded contracts).'''
    return compute(case, inp if inp is not None else inputs(case), 'ref')


def emulate(case: Case, inp: dict, form: int = 1) -> torch.Tensor:
    '''The kernel's arithmetic in fp32 in its own operation order; form 2 = the other legal form (the fused affine).'''
    return compute(case, inp, 'emu2' if form == 2 else 'emu').value


def mutate(case: Case, inp: dict, mutant: str) -> Optional[torch.Tensor]:
    '''The output of a wrong computation; None where the mutant does not apply to the case.'''
    return compute(case, inp, 'emu', mutant).value if applies(case, mutant) else None


@functools.lru_cache(None)
def exp_form_k() -> float:
    '''The k of the exp form's bound k 2^-24 |want|: TWICE the worst error, in units of 2^-24 |want|, of torch's fp32 CPU evaluation
    of exp(0.5 x) y b against float64 over the inputs of every exp case.  Never taken from the kernel.  The factor 2: the device's expf
    is another implementation than the host's (OCML specifies about 1 ulp).'''
    worst_u = 0.0
    for case in cases_of('fd_axpby_f32'):
        if not case.p.exp:
            continue
        inp = inputs(case)
        b32 = _f32(case.p.b)
        ex = torch.exp(0.5 * inp['x'].double()) * inp['y'].double() * b32.double()
        got = torch.exp(_f32(0.5) * inp['x']) * inp['y'] * b32
        nz = ex != 0
        worst_u = max(worst_u, float(((got.double() - ex).abs()[nz] / (2.0 ** -24 * ex.abs()[nz])).max()))
    return 2.0 * worst_u


# --------------------------------------------------------------------------------------------------- the criterion
def worst(got: torch.Tensor, want: SimpleNamespace, case: Case) -> float:
    '''Worst |err| / bound of a bounded contract (inf where the bound is 0 and the error is not, or got is not finite); for a bit
    contract 0.0 when the bits agree and inf when they do not.'''
    if want.bound is None:
        return 0.0 if bits_equal(got, want.value) else float('inf')
    if got.shape != want.exact.shape or not bool(torch.isfinite(got).all()):
        return float('inf')
    err = (got.double() - want.exact).abs()
    ratio = torch.where(err <= want.bound, err / want.bound.clamp(min=1e-300), torch.full_like(err, float('inf')))
    return float(ratio.max())


def check(got: torch.Tensor, want: SimpleNamespace, case: Case) -> bool:
    p, e = case.p, case.entry
    want_dtype = {'fd_cast_f16_to_f32': torch.float32, 'fd_nhwc_f32_to_nchw_f32': torch.float32, 'fd_axpby_f32': torch.float32,
                  'fd_region_blend_f32': torch.float32}.get(e, torch.float16)
    if got.dtype != want_dtype or not worst(got, want, case) <= 1.0:
        return False
    if e == 'fd_nhwc_f32_to_nchw_f32' and p.clamp and not bool(((got >= 0) & (got <= 1)).all()):
        return False
    if e == 'fd_conv3x3_narrow_f16':       # the replicas carry the bits of y
        M = p.B * p.H * p.W
        return all(torch.equal(_bits(got[:M]), _bits(got[(r + 1) * M:(r + 2) * M])) for r in range(p.rep2))
    return True


# --------------------------------------------------------------------------------------------------- staging and the device run
def _padded(data: torch.Tensor, ld: int, off: int, fill: float, guard: int = 0, tail: int = 0) -> torch.Tensor:
    '''Flat buffer: `guard` elements, rows of `ld` with `data` [rows][cols] at column `off`, `tail` + `guard` elements; the rest = fill.'''
    rows, cols = data.shape
    assert off + cols <= ld
    buf = torch.full((guard + rows * ld + tail + guard,), fill, dtype=data.dtype)
    torch.as_strided(buf, (rows, cols), (ld, 1), guard + off).copy_(data)
    return buf


def _out(rows: int, cols: int, ld: int, off: int, dtype) -> tuple:
    '''(sentinel-filled flat buffer, view) of an output [rows][cols] at column `off` of rows of `ld`, guards on both sides.'''
    assert off + cols <= ld
    return torch.full((2 * GUARD + rows * ld,), PAD, dtype=dtype), ((rows, cols), (ld, 1), GUARD + off)


def stage(case: Case, inp: Optional[dict] = None) -> SimpleNamespace:
    '''bufs: name -> flat host buffer (inputs with NaN padding, outputs with sentinels and guards); outs: name -> (shape, strides,
    offset) of the output view inside its buffer; args: the C arguments in ABI order without the stream, pointers as Ptr.'''
    p, e = case.p, case.entry
    inp = inp if inp is not None else inputs(case)
    nan = float('nan')
    bufs, outs, a = {}, collections.OrderedDict(), collections.OrderedDict()
    f16, f32 = torch.float16, torch.float32
    if e in ('fd_cast_f16_to_f32', 'fd_cast_f32_to_f16'):
        bufs['x'] = inp['x'].clone()
        bufs['y'], outs['y'] = _out(p.n, 1, 1, 0, f32 if e == 'fd_cast_f16_to_f32' else f16)
        a.update(x=Ptr('x'), y=Ptr('y', GUARD), n=p.n)
    elif e == 'fd_nchw_f32_to_nhwc_f16':
        bufs['x'] = inp['x'].reshape(-1).clone()
        bufs['y'], outs['y'] = _out(p.rep * p.B * p.HW, p.c_pad, p.c_pad, 0, f16)
        a.update(x=Ptr('x'), y=Ptr('y', GUARD), B=p.B, C=p.C, HW=p.HW, rep=p.rep, c_pad=p.c_pad, scale=p.scale)
    elif e == 'fd_nhwc_f32_to_nchw_f32':
        bufs['x'] = _padded(inp['x'].reshape(-1, p.C), p.ld, 0, nan)
        bufs['y'], outs['y'] = _out(p.B * p.C * p.HW, 1, 1, 0, f32)
        a.update(x=Ptr('x'), y=Ptr('y', GUARD), B=p.B, C=p.C, HW=p.HW, ld=p.ld, a=p.a, b=p.b, clamp01=p.clamp)
    elif e == 'fd_im2col_f16':
        bufs['x'] = inp['x'].reshape(-1).clone()
        bufs['y'], outs['y'] = _out(p.B * p.Ho * p.Wo, p.k_pad, p.k_pad, 0, f16)
        a.update(x=Ptr('x'), y=Ptr('y', GUARD), B=p.B, Hi=p.Hi, Wi=p.Wi, Cin=p.Cin, Ho=p.Ho, Wo=p.Wo, KH=p.KH, KW=p.KW, stride=p.stride,
                 pad_t=p.pad_t, pad_l=p.pad_l, k_pad=p.k_pad)
    elif e == 'fd_concat_channels_f16':
        for n, c in (('a', p.Ca), ('b', p.Cb)):
            bufs[n] = torch.cat([inp[n].reshape(-1), torch.full((8,), nan, dtype=f16)])      # never empty; the tail is never read
        bufs['out'], outs['out'] = _out(p.M, p.Ca + p.Cb, p.Ca + p.Cb, 0, f16)
        a.update(a=Ptr('a'), b=Ptr('b'), out=Ptr('out', GUARD), M=p.M, Ca=p.Ca, Cb=p.Cb)
    elif e in ('fd_copy2d_f16', 'fd_repeat_rows_f16'):
        bufs['src'] = _padded(inp['src'], p.lds, p.s_off, nan)
        bufs['dst'], outs['dst'] = _out(p.rep * p.rows, p.cols, p.ldd, p.d_off, f16)
        a.update(src=Ptr('src', p.s_off), lds=p.lds, dst=Ptr('dst', GUARD + p.d_off), ldd=p.ldd, rows=p.rows, cols=p.cols)
        if e == 'fd_repeat_rows_f16':
            a['rep'] = p.rep
    elif e == 'fd_axpby_f32':
        bufs['x'] = _padded(inp['x'].view(-1, 1), 1, 0, PAD, GUARD)
        if p.y:
            bufs['y'] = inp['y'].clone()
        if p.alias:
            outs['x'] = ((p.n, 1), (1, 1), GUARD)
        else:
            bufs['out'], outs['out'] = _out(p.n, 1, 1, 0, f32)
        a.update(x=Ptr('x', GUARD), y=Ptr('y') if p.y else None, out=Ptr('x' if p.alias else 'out', GUARD), n=p.n, a=p.a, b=p.b,
                 exp_half_x=int(p.exp))
    elif e == 'fd_embed_tokens_f16':
        bufs['ids'] = inp['ids'].reshape(-1).clone()
        bufs['tok'] = _padded(inp['tok'], p.D, 0, nan, p.D)             # a NaN row before row 0 and behind row vocab - 1
        bufs['pos'] = _padded(inp['pos'], p.D, 0, nan, p.D)
        bufs['out'], outs['out'] = _out(p.B * p.L, p.D, p.D, 0, f16)
        a.update(ids=Ptr('ids'), tok=Ptr('tok', p.D), pos=Ptr('pos', p.D), out=Ptr('out', GUARD), B=p.B, L=p.L, D=p.D, vocab=p.vocab)
    elif e == 'fd_vit_assemble_f16':
        for n in ('patches', 'cls', 'pos'):
            bufs[n] = _padded(inp[n].view(-1, p.D), p.D, 0, nan, p.D)
        bufs['out'], outs['out'] = _out(p.B * p.T, p.D, p.D, 0, f16)
        a.update(patches=Ptr('patches', p.D), cls=Ptr('cls', p.D), pos=Ptr('pos', p.D), out=Ptr('out', GUARD), B=p.B, T=p.T, D=p.D)
    elif e == 'fd_region_blend_f32':
        bufs['dst'] = _padded(inp['dst'].view(-1, p.W), p.W, 0, PAD, GUARD)
        outs['dst'] = ((p.C * p.H, p.W), (p.W, 1), GUARD)
        bufs['src'] = inp['src'].reshape(-1).clone()
        a.update(dst=Ptr('dst', GUARD), src=Ptr('src'), C=p.C, H=p.H, W=p.W, oy=p.oy, ox=p.ox, sh=p.sh, sw=p.sw, blend=p.blend)
    elif e == 'fd_conv3x3_narrow_f16':
        M = p.B * p.H * p.W
        bufs['x'], bufs['w'] = inp['x'].reshape(-1).clone(), inp['w'].reshape(-1).clone()
        if p.bias:
            bufs['bias'] = inp['bias'].clone()
        ldy, ldy2 = p.Cout + 16, p.Cout + 24
        bufs['y'], outs['y'] = _out(M, p.Cout, ldy, 8, f16)
        if p.rep2:
            bufs['y2'], outs['y2'] = _out(p.rep2 * M, p.Cout, ldy2, 16, f16)
        a.update(x=Ptr('x'), w=Ptr('w'), bias=Ptr('bias') if p.bias else None, y=Ptr('y', GUARD + 8), ldy=ldy,
                 y2=Ptr('y2', GUARD + 16) if p.rep2 else None, ldy2=ldy2 if p.rep2 else 0, rep2=p.rep2, B=p.B, Cin=p.Cin, H=p.H, W=p.W,
                 Cout=p.Cout, scale=p.scale)
    else:
        raise KeyError(e)
    return SimpleNamespace(bufs=bufs, outs=outs, args=a)


def alloc_bytes(case: Case) -> int:
    '''The largest buffer of the staged case.'''
    return max(t.numel() * t.element_size() for t in stage(case).bufs.values())


def resolve(args: dict, base: dict) -> list:
    '''The C argument list: Ptr -> address inside the tensor `base[ptr.buf]` (host or device), None -> NULL.'''
    return [base[v.buf].data_ptr() + v.off * base[v.buf].element_size() if isinstance(v, Ptr) else v for v in args.values()]


def collect(st: SimpleNamespace, after: dict):
    '''(the rows of every output view of `after` concatenated, True when everything OUTSIDE the views still holds the bits the staged
    buffers had).'''
    views, untouched = [], True
    for name, (shape, strides, off) in st.outs.items():
        back = after[name].clone()
        view = torch.as_strided(back, shape, strides, off)
        views.append(view.clone())
        view.copy_(torch.as_strided(st.bufs[name], shape, strides, off))
        untouched = untouched and bool(torch.equal(_bits(back), _bits(st.bufs[name])))
    return torch.cat(views, 0), untouched


def run_on_device(case: Case, dev, inp: Optional[dict] = None, st: Optional[SimpleNamespace] = None) -> SimpleNamespace:
    '''Two identical launches through hip.call with hand-built arguments: out (the output rows), untouched (collect), again (the
    second launch's rows), inputs_unchanged (every pure input holds its bits).'''
    from flexdiffuse_amd import hip
    st = st if st is not None else stage(case, inp)
    d = {n: t.clone().to(dev) for n, t in st.bufs.items()}       # clone: on the host (the CPU test's stand-in) .to() would alias

    def launch():
        for name in st.outs:
            d[name].copy_(st.bufs[name])
        hip.call(case.entry, *resolve(st.args, d), hip.stream())
        torch.cuda.synchronize()
        return collect(st, {n: d[n].cpu() for n in st.outs})

    out, untouched = launch()
    again, untouched2 = launch()
    unchanged = all(torch.equal(_bits(d[n].cpu()), _bits(t)) for n, t in st.bufs.items() if n not in st.outs)
    return SimpleNamespace(out=out, untouched=untouched and untouched2, again=again, inputs_unchanged=unchanged, st=st, dev=d)


# --------------------------------------------------------------------------------------------------- refusals
def _plus(nbytes):
    return lambda ptr: ptr + nbytes


REFUSAL_BASE = {'fd_cast_f16_to_f32': 'all-patterns', 'fd_cast_f32_to_f16': 'boundary', 'fd_nchw_f32_to_nhwc_f16': '2x3x35x3x8-rand-s0.5',
                'fd_nhwc_f32_to_nchw_f32': '3x3x35x8-a0.5-b0.5-clamp1', 'fd_im2col_f16': 'conv_in-3x3-s1-p1-cin4',
                'fd_concat_channels_f16': '5x8+8', 'fd_copy2d_f16': 'both', 'fd_repeat_rows_f16': 'both-rep2',
                'fd_axpby_f32': 'n257-derivative', 'fd_embed_tokens_f16': '2x5x257-v50', 'fd_vit_assemble_f16': '4x5x257',
                'fd_region_blend_f32': 'inside-w0.37', 'fd_conv3x3_narrow_f16': '2x2x1x9x64x1'}

# entry point -> argument overrides the host code must refuse (a value, or a function of the good value; pointers are addresses by then).
# Every one is refused by an FD_CHECK_ARG that precedes the launch in csrc/elementwise.hip.
REFUSALS = {
    'fd_cast_f16_to_f32': [dict(x=None), dict(y=None), dict(n=0), dict(n=-4)],
    'fd_cast_f32_to_f16': [dict(x=None), dict(y=None), dict(n=0), dict(n=-4)],
    'fd_nchw_f32_to_nhwc_f16': [dict(x=None), dict(y=None), dict(B=0), dict(C=0), dict(HW=0), dict(rep=0), dict(B=-1), dict(c_pad=2)],
    'fd_nhwc_f32_to_nchw_f32': [dict(x=None), dict(y=None), dict(B=0), dict(C=0), dict(HW=0), dict(HW=-35), dict(ld=2)],
    'fd_im2col_f16': [dict(x=None), dict(y=None), dict(B=0), dict(Hi=0), dict(Wi=0), dict(Cin=0), dict(Ho=0), dict(Wo=0), dict(KH=0),
                      dict(KW=0), dict(stride=0), dict(KH=-3), dict(KW=-3), dict(stride=-1), dict(pad_t=-1), dict(pad_l=-1),
                      dict(k_pad=32), dict(k_pad=44), dict(k_pad=0)],
    'fd_concat_channels_f16': [dict(a=None), dict(b=None), dict(out=None), dict(M=0), dict(M=-5), dict(Ca=-8), dict(Cb=-8),
                               dict(Ca=-8, Cb=-8), dict(Ca=0, Cb=0), dict(Ca=4), dict(Cb=12), dict(a=_plus(8)), dict(b=_plus(2)),
                               dict(out=_plus(8))],
    'fd_copy2d_f16': [dict(src=None), dict(dst=None), dict(rows=0), dict(cols=0), dict(cols=-8), dict(lds=56), dict(ldd=56),
                      dict(cols=60), dict(lds=68), dict(ldd=68), dict(src=_plus(8)), dict(dst=_plus(2))],
    'fd_repeat_rows_f16': [dict(src=None), dict(dst=None), dict(rows=0), dict(cols=0), dict(rep=0), dict(rep=-1), dict(lds=56),
                           dict(ldd=56), dict(cols=60), dict(lds=68), dict(ldd=68), dict(src=_plus(8)), dict(dst=_plus(2))],
    'fd_axpby_f32': [dict(x=None), dict(out=None), dict(n=0), dict(n=-1)],
    'fd_embed_tokens_f16': [dict(ids=None), dict(tok=None), dict(pos=None), dict(out=None), dict(B=0), dict(L=0), dict(D=0),
                            dict(vocab=0), dict(vocab=-1)],
    'fd_vit_assemble_f16': [dict(patches=None), dict(cls=None), dict(pos=None), dict(out=None), dict(B=0), dict(T=1), dict(T=0), dict(D=0)],
    'fd_region_blend_f32': [dict(dst=None), dict(src=None), dict(C=0), dict(H=0), dict(W=0), dict(oy=-1), dict(ox=-1), dict(oy=-1, ox=-1)],
    'fd_conv3x3_narrow_f16': [dict(x=None), dict(w=None), dict(y=None), dict(y2=None), dict(B=0), dict(H=0), dict(W=0), dict(rep2=-1),
                              dict(Cin=5), dict(Cin=0), dict(Cout=12), dict(Cout=2056), dict(Cout=0), dict(W=1025), dict(ldy=56),
                              dict(ldy=68), dict(ldy2=56), dict(ldy2=68), dict(y=_plus(8)), dict(y2=_plus(2))],
}


def refusal_case(entry: str) -> Case:
    return next(c for c in cases_of(entry) if c.tag == REFUSAL_BASE[entry])


def apply_overrides(arglist: list, names: list, override: dict) -> list:
    out = list(arglist)
    for name, v in override.items():
        i = names.index(name)
        out[i] = v(out[i]) if callable(v) else v
    return out
