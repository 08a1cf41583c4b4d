'''One table of GroupNorm cases for the four consumers in csrc/norm.hip (fd_groupnorm_nhwc[_ld]_f16,
fd_groupnorm_apply_parts_f16, fd_groupnorm_fold_linear_f16, fd_groupnorm_fold_linear_parts_f16) and csrc/gn_slab.h: a
Python restatement of the dispatch and of every launch shape, inputs, float64 references, a derived per-element
acceptance bound, and an fp32 emulation of each form with the kernels' lane -> pixel map and summation order --
shared by tests/test_groupnorm_cases.py (CPU) and tests/test_gpu_groupnorm.py (MI355X, through the C ABI).

Nothing here needs a GPU to import; `run_on_device` is the only part that touches one.

Forms (what one call launches):
    slab256      k_gn_slab<256, 16>                      route full
    slab1024     k_gn_slab<1024, 22>                     route full, HW <= 1024
    stream       k_gn_stats + k_gn_apply                 route full, everything the slabs do not take
    apply_parts  k_gn_apply                              statistics supplied as partial sums
    fold         k_gn_stats + k_gn_fold_linear
    fold_parts   k_gn_fold_linear                        statistics supplied as partial sums

Unreachable, proven by sweep over all legal (C, G) with C <= 8192, G <= 64 (test_groupnorm_cases.py):
    * gn_slab_pick never returns GB = 8: cpg is even there, so GB = 4 already makes cpg * GB a multiple of 8;
    * the `stats LDS too large` refusal cannot fire once C / 8 <= 1024 holds (PL * C * 8 bytes <= 64 KiB).
The table has no case for either and is not to be blamed for it.

Worst |err| / bound of the fp32 CPU emulation over the live cases, per form (measured by
test_groupnorm_cases.py::test_emulation_passes_check_everywhere, which prints them):
    slab256 0.99   slab1024 1.00   stream 1.00   apply_parts 1.00   fold 0.99   fold_parts 1.00
(the one rounding to half, 2^-11 |want|, is met by an element just above a power of two; the statistics terms are
worst-case sums of roundings that a real summation never lines up, so they stay almost unused).'''
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

U24 = 2.0 ** -24          # fp32 unit roundoff
U11 = 2.0 ** -11          # fp16 unit roundoff
FLOOR = 2.0 ** -24        # half of the smallest fp16 subnormal: the rounding error where the output is subnormal
SILU_REL = 2.0 ** -19     # fp32 SiLU: exp argument (|t| <= 17 where exp(-t) matters, 1.5 ulp each), v_exp, add, v_rcp, multiply
JUNK = 100.0              # padding columns / the rest of the wide matrix a slice lives in
SENTINEL = -1234.0        # every output byte before a launch
GUARD = 96                # sentinel elements before and after every output
LAYOUTS = ('contig', 'padded', 'slice')
ROUTES = ('full', 'apply_parts', 'fold', 'fold_parts')
FORMS = ('slab256', 'slab1024', 'stream', 'apply_parts', 'fold', 'fold_parts')
KERNELS = {'slab256': ('k_gn_slab<256, 16>',), 'slab1024': ('k_gn_slab<1024, 22>',), 'stream': ('k_gn_stats', 'k_gn_apply'),
           'apply_parts': ('k_gn_apply',), 'fold': ('k_gn_stats', 'k_gn_fold_linear'), 'fold_parts': ('k_gn_fold_linear',)}
ENTRY = {'full': 'fd_groupnorm_nhwc_ld_f16', 'apply_parts': 'fd_groupnorm_apply_parts_f16',
         'fold': 'fd_groupnorm_fold_linear_f16', 'fold_parts': 'fd_groupnorm_fold_linear_parts_f16'}

# ---- constants copied from the source (test_groupnorm_cases.py checks each against the text) -----------------------
SLABS = ((256, 16), (1024, 22))   # <NT, NV> in the order fd_groupnorm_nhwc_ld_f16 tries them
SLAB2_MAX_HW = 1024               # the gate in front of the second
SLAB_LDS = 160 * 1024
STREAM_LANES = 512                # PL = 512 / (C / 8)
GN_MAX_CHUNKS = 256
STATS_LDS = 64 * 1024
GNF_ROWS = 16
FOLD_LDS = 48 * 1024
FOLD_THREADS = 256
MAX_C8 = 1024
MAX_G = 64
FD_OK, FD_EINVAL, FD_ESHAPE = 0, -1, -2


class Case(NamedTuple):
    B: int
    HW: int
    C: int
    G: int
    silu: bool = True
    eps: float = 1e-5
    layout: str = 'contig'
    means: int = 0            # group mean / group sigma
    route: str = 'full'
    chunks: int = 0           # parts routes
    N: int = 0                # fold routes
    indicator: bool = False   # fold: the rows of wg are group indicators (N = G)
    xscale: float = 1.0       # 2^-8: the variance comes down to eps
    seed: int = 0

    @property
    def id(self) -> str:
        return (f'{self.route}-{self.B}x{self.HW}x{self.C}g{self.G}-m{self.means}-{self.layout}' + ('-silu' if self.silu else '') +
                (f'-eps{self.eps:g}' if self.eps != 1e-5 else '') + (f'-k{self.chunks}' if self.chunks else '') +
                (f'-n{self.N}' if self.N else '') + ('-ind' if self.indicator else '') + ('-tiny' if self.xscale != 1.0 else ''))

    @property
    def cpg(self) -> int:
        return self.C // self.G

    @property
    def numel(self) -> int:
        return self.B * self.HW * self.C


# --------------------------------------------------------------------------------------------------- dispatch
def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def slab_pick(NT: int, NV: int, HW: int, C: int, G: int) -> Optional[dict]:
    '''gn_slab_pick<NT, NV> of gn_slab.h: None where it returns 0.'''
    cpg = C // G
    if C % G or cpg & 1:
        return None
    GB = 1
    while GB <= 8 and GB <= G:
        if G % GB == 0 and (cpg * GB) % 8 == 0:
            CB = cpg * GB
            cb8 = CB // 8
            if cb8 > NT or CB // 2 > NT:
                return None
            pl, J = NT // cb8, NT // (CB // 2)
            if cdiv(HW, pl) > NV:
                return None
            lds = (pl * CB + J * CB + GB * 2) * 4
            if lds > SLAB_LDS:
                return None
            return dict(NT=NT, NV=NV, GB=GB, CB=CB, c8=cb8, pl=pl, J=J, lds=lds, idle=NT - pl * cb8, nblk=G // GB)
        GB *= 2
    return None


def stream_shape(B: int, HW: int, C: int):
    '''(PL, threads, nchunk, ppc): gn_stats_shape and its two hand copies in norm.hip.'''
    c8 = C // 8
    PL = min(max(STREAM_LANES // c8, 1), HW)
    threads = cdiv(c8 * PL, 64) * 64
    nchunk = min(max(256 // B, 1), GN_MAX_CHUNKS)
    ppc = max(cdiv(HW, nchunk), PL)
    return PL, threads, cdiv(HW, ppc), ppc


def expected_form(case: Case) -> dict:
    '''The form a case runs and its launch parameters.'''
    B, HW, C, G = case.B, case.HW, case.C, case.G
    if case.route == 'full':
        for i, (NT, NV) in enumerate(SLABS):
            if i == 1 and HW > SLAB2_MAX_HW:
                break
            s = slab_pick(NT, NV, HW, C, G)
            if s:
                return dict(s, form=f'slab{NT}')
    PL, threads, nchunk, ppc = stream_shape(B, HW, C)
    c8 = C // 8
    d = dict(PL=PL, threads=threads, nchunk=nchunk, ppc=ppc, c8=c8, idle=threads - c8 * PL, stats_lds=PL * C * 8)
    if case.route == 'full':
        return dict(d, form='stream', nsub=threads // G, combine=nchunk)
    if case.route == 'apply_parts':
        return dict(d, form='apply_parts', nsub=threads // G, combine=case.chunks)
    if case.route == 'fold':
        return dict(d, form='fold', nsub=FOLD_THREADS // G, combine=nchunk, blocks=cdiv(case.N, GNF_ROWS))
    return dict(form='fold_parts', nsub=FOLD_THREADS // G, combine=case.chunks, blocks=cdiv(case.N, GNF_ROWS))


def lane_pixels(case: Case):
    '''Streaming forms: the set of (pixels a lane of k_gn_stats / k_gn_apply visits in one chunk) over all lanes and chunks.'''
    f = expected_form(case)
    out = set()
    for k in range(f['nchunk']):
        n = min(case.HW, (k + 1) * f['ppc']) - k * f['ppc']
        out.update({cdiv(n, f['PL']), n // f['PL']} if n % f['PL'] else {n // f['PL']})
    return out


def refusal_code(route: str, a: dict) -> int:
    '''What the entry point of `route` answers to the arguments `a` (keys: B HW C G ldx x_mis N chunks): FD_OK where it
    would launch.  Restates the FD_CHECK_ARG conditions of norm.hip in their order.'''
    B, HW, C, G, ldx, N, chunks = a['B'], a['HW'], a['C'], a['G'], a.get('ldx', a['C']), a.get('N', 16), a.get('chunks', 1)
    mis = a.get('x_mis', 0) % 16 != 0
    dims = B > 0 and HW > 0 and C > 0 and G > 0
    shape = C % 8 == 0 and dims and C % G == 0 and G <= MAX_G
    ld = ldx >= C and ldx % 8 == 0 and not mis
    if route == 'full':
        if not ld:
            return FD_ESHAPE
        if not dims:
            return FD_EINVAL
        return FD_OK if shape and C // 8 <= MAX_C8 else FD_ESHAPE
    if route == 'apply_parts':
        if not (dims and chunks > 0):
            return FD_EINVAL
        return FD_OK if ld and shape and C // 8 <= MAX_C8 else FD_ESHAPE
    if route == 'fold':
        if not (dims and N > 0):
            return FD_EINVAL
        return FD_OK if shape and C // 8 <= MAX_C8 and ld and GNF_ROWS * C * 2 <= FOLD_LDS else FD_ESHAPE
    if not (dims and N > 0 and chunks > 0):
        return FD_EINVAL
    return FD_OK if shape and GNF_ROWS * C * 2 <= FOLD_LDS else FD_ESHAPE


# (name, route, arguments): everything else as in a small good call
_GOOD = dict(B=2, HW=6, C=64, G=8, N=16, chunks=2)
REFUSALS = (
    ('C%8', 'full', dict(_GOOD, C=12, G=4)), ('C%8', 'apply_parts', dict(_GOOD, C=12, G=4)),
    ('C%8', 'fold', dict(_GOOD, C=12, G=4)), ('C%8', 'fold_parts', dict(_GOOD, C=12, G=4)),
    ('C%G', 'full', dict(_GOOD, C=24, G=5)), ('C%G', 'apply_parts', dict(_GOOD, C=24, G=5)),
    ('C%G', 'fold', dict(_GOOD, C=24, G=5)), ('C%G', 'fold_parts', dict(_GOOD, C=24, G=5)),
    ('G=65', 'full', dict(_GOOD, C=520, G=65)), ('G=65', 'apply_parts', dict(_GOOD, C=520, G=65)),
    ('G=65', 'fold', dict(_GOOD, C=520, G=65)), ('G=65', 'fold_parts', dict(_GOOD, C=520, G=65)),
    ('C=8200', 'full', dict(_GOOD, C=8200)), ('C=8200', 'apply_parts', dict(_GOOD, C=8200)),
    ('ldx<C', 'full', dict(_GOOD, ldx=56)), ('ldx<C', 'apply_parts', dict(_GOOD, ldx=56)), ('ldx<C', 'fold', dict(_GOOD, ldx=56)),
    ('ldx%8', 'full', dict(_GOOD, ldx=68)), ('ldx%8', 'apply_parts', dict(_GOOD, ldx=68)), ('ldx%8', 'fold', dict(_GOOD, ldx=68)),
    ('x+8B', 'full', dict(_GOOD, ldx=72, x_mis=8)), ('x+8B', 'apply_parts', dict(_GOOD, ldx=72, x_mis=8)),
    ('x+8B', 'fold', dict(_GOOD, ldx=72, x_mis=8)),
    ('C=1544', 'fold', dict(_GOOD, C=1544)), ('C=1544', 'fold_parts', dict(_GOOD, C=1544)),
    ('chunks=0', 'apply_parts', dict(_GOOD, chunks=0)), ('chunks=0', 'fold_parts', dict(_GOOD, chunks=0)),
)


# --------------------------------------------------------------------------------------------------- the table
def _c(B, HW, C, G, *flags, layout='contig', means=0, route='full', chunks=0, N=0, eps=1e-5):
    '''flags: 'plain' (no SiLU), 'ind' (indicator weights), 'tiny' (x scaled by 2^-8).'''
    assert set(flags) <= {'plain', 'ind', 'tiny'} and layout in LAYOUTS and route in ROUTES and means in (0, 1, 10)
    return Case(B, HW, C, G, 'plain' not in flags, eps, layout, means, route, chunks, N, 'ind' in flags,
                2.0 ** -8 if 'tiny' in flags else 1.0)


_TABLE = [
    # ---- k_gn_slab<256, 16> --------------------------------------------------------------------------------------------
    _c(2, 816, 320, 32, means=10),                         # GB 4, pl 51: HW = pl * NV, one idle lane
    _c(2, 64, 256, 32, 'plain', layout='padded'),          # GB 1, pl 256, J 64, no idle lane
    _c(2, 64, 128, 32, layout='slice', means=1),           # GB 2
    _c(2, 64, 64, 32, 'plain', means=10, eps=1e-6),        # GB 4, cpg 2
    _c(2, 128, 8192, 32, means=1),                         # CB 256, pl 8, J 2: HW = pl * NV
    _c(2, 1, 320, 32, 'plain', means=1),                   # HW 1
    _c(3, 37, 320, 32, 'tiny', layout='padded'),           # var ~ eps
    _c(2, 16, 24, 1, 'plain', means=1),                    # G 1
    _c(2, 33, 1024, 2, layout='slice', means=10),          # CB/2 = NT = 256: J 1, pl 4
    # ---- k_gn_slab<1024, 22> -------------------------------------------------------------------------------------------
    _c(2, 817, 320, 32, means=10),                         # pl * NV + 1 of <256, 16>; pl 204, four idle lanes
    _c(2, 1024, 320, 32, 'plain', layout='padded', means=1),      # the HW <= 1024 gate
    _c(2, 129, 8192, 32, 'plain', layout='slice'),         # pl * NV + 1 of <256, 16> at CB 256; J 8, no idle lane
    _c(1, 704, 8192, 32, means=10),                        # pl 32: HW = pl * NV
    _c(2, 176, 8192, 8, 'plain', means=1, eps=1e-6),       # CB 1024, J 2, pl 8: HW = pl * NV
    _c(2, 88, 8192, 4, means=10),                          # CB 2048: CB/2 = NT, J 1, pl 4: HW = pl * NV
    _c(3, 900, 640, 32, 'tiny', layout='slice'),           # var ~ eps; GB 2
    _c(2, 40, 2048, 1, 'plain', means=1),                  # G 1 (CB/2 = NT)
    # ---- k_gn_stats + k_gn_apply ---------------------------------------------------------------------------------------
    _c(2, 1025, 320, 32, means=10),                        # beyond the gate; PL 12, 86 chunks of 12 (> 4 nsub), the last one of 5
    _c(1, 705, 8192, 32, 'plain'),                         # pl * NV + 1 of <1024, 22>; PL 1, 1024 threads, no idle lane, 235 chunks of 3
    _c(2, 177, 8192, 8, means=1),                          # pl * NV + 1 at CB 1024
    _c(2, 89, 8192, 4, 'plain', means=10),                 # pl * NV + 1 at CB 2048
    _c(2, 50, 8192, 2, layout='padded', means=1),          # CB/2 > 1024
    _c(2, 5, 8184, 8, 'plain', layout='slice', means=10),  # cpg 1023: odd, 16 laps of the group loop; 1024 threads, one idle
    _c(2, 2, 24, 8, means=1),                              # 64 threads, 58 idle; PL = HW; more groups than waves
    _c(2, 1, 24, 8, 'plain'),                              # HW 1
    _c(129, 2295, 24, 8, means=10),                        # one chunk; lanes with 14 and 13 pixels: 3 trips, tails 2 and 1
    _c(129, 2635, 24, 8, 'plain', layout='padded', means=1),      # 16 and 15 pixels: 4 trips tail 0, 3 trips tail 3
    _c(257, 3, 24, 8, means=1),                            # B > 256: nchunk clamps at 1
    _c(1, 1500, 24, 8, 'plain', layout='slice', means=10, eps=1e-6),   # 9 chunks of 170, the last of 140 < PL
    _c(1, 256, 4104, 8, means=1),                          # 256 chunks of one pixel; cpg 513, 576 threads, 63 idle
    _c(2, 40, 64, 64, 'plain', means=10),                  # cpg 1, G 64
    _c(2, 100, 24, 24, layout='padded', means=1),          # G 24: 320 threads, nsub 13
    _c(3, 70, 48, 48, 'plain', 'tiny'),                    # G 48; var ~ eps
    _c(2, 1361, 24, 1, means=1),                           # G 1: one HW beyond <256, 16>
    # ---- k_gn_apply from supplied partial sums: C 320, G 32 -> 512 threads, nsub 16; the four-way unrolled combine --------
    _c(2, 40, 320, 32, means=10, route='apply_parts', chunks=1),
    _c(2, 40, 320, 32, 'plain', layout='padded', means=1, route='apply_parts', chunks=16),
    _c(2, 40, 320, 32, layout='slice', route='apply_parts', chunks=49),
    _c(2, 40, 320, 32, 'plain', means=10, route='apply_parts', chunks=70, eps=1e-6),
    _c(2, 300, 320, 32, means=1, route='apply_parts', chunks=256),
    _c(2, 100, 24, 24, 'plain', layout='padded', means=10, route='apply_parts', chunks=27),    # nsub 13: 2 * 13 + 1
    _c(2, 64, 256, 1, 'tiny', route='apply_parts', chunks=3),                                  # G 1, var ~ eps
    _c(129, 2295, 24, 8, 'plain', means=1, route='apply_parts', chunks=5),                     # the pipelined store loop, 3 trips
    _c(2, 9, 8184, 8, means=1, route='apply_parts', chunks=2, layout='slice'),                 # cpg 1023
    # ---- k_gn_stats + k_gn_fold_linear ---------------------------------------------------------------------------------
    _c(2, 64, 320, 32, means=10, route='fold', N=8),
    _c(2, 1025, 320, 32, layout='padded', means=1, route='fold', N=16),
    _c(3, 40, 1536, 64, layout='slice', route='fold', N=24),
    _c(1, 1500, 24, 8, means=10, route='fold', N=64, eps=1e-6),
    _c(129, 2295, 24, 8, 'ind', means=10, route='fold', N=8),           # rstd and mean read out behind the longest lanes
    _c(2, 100, 320, 32, 'ind', layout='padded', means=10, route='fold', N=32),
    _c(3, 33, 64, 64, 'tiny', route='fold', N=40),
    _c(2, 30, 1536, 1, means=1, route='fold', N=16),
    # ---- k_gn_fold_linear from supplied partial sums: G 32 -> nsub 8 ------------------------------------------------------
    _c(2, 64, 320, 32, means=10, route='fold_parts', chunks=1, N=8),
    _c(2, 64, 320, 32, means=1, route='fold_parts', chunks=8, N=16),
    _c(2, 64, 320, 32, route='fold_parts', chunks=25, N=24),
    _c(2, 64, 320, 32, means=10, route='fold_parts', chunks=38, N=80, eps=1e-6),
    _c(2, 512, 320, 32, 'ind', means=10, route='fold_parts', chunks=256, N=32),
    _c(3, 40, 1536, 64, 'tiny', route='fold_parts', chunks=5, N=24),
    _c(2, 40, 24, 1, means=1, route='fold_parts', chunks=3, N=8),
]
CASES = tuple(c._replace(seed=500 + i) for i, c in enumerate(_TABLE))
assert len({c.id for c in CASES}) == len(CASES)


# --------------------------------------------------------------------------------------------------- inputs
def _rnd(shape, gen):
    return torch.randn(shape, generator=gen)


def spike_pixels(case: Case):
    '''Pixels scaled by 8: the two ends, both sides of every streaming chunk boundary, the last register slot of a slab.'''
    f = expected_form(case)
    px = {0, case.HW - 1}
    if 'ppc' in f:
        for k in range(1, f['nchunk']):
            px.update((k * f['ppc'] - 1, k * f['ppc']))
    if 'pl' in f:
        px.add(f['pl'] * f['NV'] - 1)
    return sorted(p for p in px if 0 <= p < case.HW)


def part_pixels(case: Case):
    '''The pixel ranges behind the supplied partial sums: `chunks` nearly equal pieces (empty ones where chunks > HW).'''
    return [(k * case.HW // case.chunks, (k + 1) * case.HW // case.chunks) for k in range(case.chunks)]


def group_stats(x64, G):
    '''float64 (mean, var, mean |x|, mean x^2) per (sample, group) of [B][HW][C].'''
    B, HW, C = x64.shape
    v = x64.reshape(B, HW, G, C // G)
    mean = v.mean((1, 3))
    ex2 = (v * v).mean((1, 3))
    return mean, (ex2 - mean * mean).clamp(min=0), v.abs().mean((1, 3)), ex2


def inputs(case: Case) -> dict:
    gen = torch.Generator().manual_seed(case.seed)
    B, HW, C, G, cpg = case.B, case.HW, case.C, case.G, case.cpg
    pix = torch.ones(HW)
    pix[spike_pixels(case)] = 8.0
    ch = torch.ones(C)
    ch[0::cpg] = 4.0
    ch[cpg - 1::cpg] = 4.0
    bi, gi = torch.arange(B)[:, None], torch.arange(G)[None, :]
    sig = 0.5 * 2.0 ** (((3 * bi + 5 * gi) % 7) / 3.0)            # the spread differs from group to group and sample to sample
    n = _rnd((B, HW, C), gen) * pix[None, :, None] * (ch[None, :] * sig.repeat_interleave(cpg, 1))[:, None, :] * case.xscale
    rms = (n * n).reshape(B, HW, G, cpg).mean((1, 3)).sqrt()
    sign = 1.0 - 2.0 * ((bi + gi) % 2)
    mu = case.means * sign * (1.0 + 0.1 * ((bi + 2 * gi) % 3 - 1)) * rms
    x16 = (n + mu.repeat_interleave(cpg, 1)[:, None, :]).half()
    inp = {'x16': x16, 'gamma': (1 + 0.2 * _rnd((C,), gen)).float(), 'beta': (0.3 * _rnd((C,), gen)).float()}
    if case.route in ('apply_parts', 'fold_parts'):
        # float64 sums per piece, the mean of every second group moved by half a sigma towards 0 and beyond (the variance the
        # parts imply, E[x^2] - mean^2, grows with it and stays positive), rounded to fp32: NOT the statistics of x
        x64 = x16.double().reshape(B, HW, G, cpg)
        mean, var, _, _ = group_stats(x16.double(), G)
        shift = torch.where(mean >= 0, -1.0, 1.0) * 0.5 * var.sqrt() * (gi % 2)
        parts = torch.zeros((B, case.chunks, G, 2), dtype=torch.float64)
        for k, (a, b) in enumerate(part_pixels(case)):
            parts[:, k, :, 0] = x64[:, a:b].sum((1, 3)) + shift * ((b - a) * cpg)
            parts[:, k, :, 1] = (x64[:, a:b] ** 2).sum((1, 3))
        inp['parts'] = parts.float()
    if case.route in ('fold', 'fold_parts'):
        if case.indicator:
            assert case.N == G
            wg = torch.zeros((case.N, C))
            for g in range(G):
                wg[g, g * cpg:(g + 1) * cpg] = 1.0
        else:
            wg = _rnd((case.N, C), gen) * C ** -0.5
        inp['wg16'] = wg.half()
        inp['biasf'] = (0.3 * _rnd((case.N,), gen)).float()
    return inp


# --------------------------------------------------------------------------------------------------- reference and bound
def adds(case: Case) -> int:
    '''The largest number of fp32 additions between an element and its group's partial sum, from the launch shape.'''
    f = expected_form(case)
    if f['form'] in ('apply_parts', 'fold_parts'):
        return 0                                        # fp32 values in, fp64 from there on
    if f['form'].startswith('slab'):
        # lane: v_dot2 adds two products into the accumulator per register (two roundings at the most); level 1: lanes
        # j, j + J, ...; level 2 is fp64
        return 2 * cdiv(case.HW, f['pl']) + cdiv(f['pl'], f['J'])
    # lane: one add (one fma) per pixel; level 1: PL lanes in turn; group: laps of 64 lanes + six butterfly levels
    return cdiv(min(f['ppc'], case.HW), f['PL']) + f['PL'] + cdiv(case.cpg, 64) + 6


def _silu(t):
    return t * torch.sigmoid(t)


def _per_channel(v, cpg):
    return v.repeat_interleave(cpg, 1)[:, None, :]


def ref_stats(case: Case, inp: dict) -> dict:
    '''float64 mean / var the kernel is to use, with the worst-case error of its fp32 sums (see `check`).'''
    x64 = inp['x16'].double()
    n = case.HW * case.cpg
    if case.route in ('apply_parts', 'fold_parts'):
        p = inp['parts'].double().sum(1)
        mean = p[..., 0] / n
        var = (p[..., 1] / n - mean * mean).clamp(min=0)
        dmean = torch.zeros_like(mean)
        dvar = torch.zeros_like(mean)
    else:
        mean, var, a1, a2 = group_stats(x64, case.G)
        D = adds(case)
        dmean = D * U24 * a1
        dvar = D * U24 * a2 + 2 * mean.abs() * dmean + dmean * dmean
    r = dvar / (var + case.eps)
    assert float(r.max()) < 0.5, f'{case.id}: the statistics bound is void (d var / (var + eps) = {float(r.max()):.3g})'
    rho = (1 - r) ** -0.5 - 1 + 2 * U24                    # relative error of the fp32 rstd the kernel keeps
    return {'mean': mean, 'var': var, 'rstd': (var + case.eps) ** -0.5, 'dmean': dmean + U24 * mean.abs(), 'rho': rho}


def reference(case: Case, inp: dict, got: Optional[dict] = None) -> dict:
    '''float64 reference and per-element bound: {'y', 'y_bound'} or {'w_out', 'w_bound', 'bias_out', 'bias_bound'}.  The
    fold's bias is defined over the kernel's own rounded w_out (the contract in norm.hip), so it needs got['w_out'].'''
    st = ref_stats(case, inp)
    cpg = case.cpg
    if case.route in ('full', 'apply_parts'):
        x = inp['x16'].double()
        g, b = inp['gamma'].double()[None, None, :], inp['beta'].double()[None, None, :]
        mean, rstd, rho, dmean = (_per_channel(st[k], cpg) for k in ('mean', 'rstd', 'rho', 'dmean'))
        t = (x - mean) * rstd * g + b
        sc = rstd * g.abs()
        e_t = sc * ((x - mean).abs() * (rho + 2 * U24) + dmean * (1 + rho)) + 4 * U24 * ((x.abs() + mean.abs()) * sc * (1 + rho) + b.abs())
        if case.silu:
            want = _silu(t)
            e_y = torch.maximum((_silu(t + e_t) - want).abs(), (_silu(t - e_t) - want).abs()) + SILU_REL * want.abs()
        else:
            want, e_y = t, e_t
        return {'y': want, 'y_bound': e_y + U11 * (want.abs() + e_y) + FLOOR}
    wg, bias = inp['wg16'].double(), inp['biasf'].double()
    rstd, rho = _per_channel(st['rstd'], cpg), _per_channel(st['rho'], cpg)           # [B][1][C]
    w = wg[None] * rstd
    e_w = w.abs() * (rho + 2 * U24)
    out = {'w_out': w, 'w_bound': e_w + U11 * (w.abs() + e_w) + FLOOR}
    if got is not None:
        wk = got['w_out'].double().reshape(case.B, case.N, case.G, cpg)
        S = wk.sum(3)                                                                   # [B][N][G]
        run = wk.cumsum(3)[..., 1:].abs().sum(3) * 1.01        # the fp32 adds behind S_g round 2^-24 of each running sum
        m, dm = st['mean'][:, None, :], st['dmean'][:, None, :]
        out['bias_out'] = bias[None] - (m * S).sum(2)
        out['bias_bound'] = ((dm * S.abs() + m.abs() * U24 * run).sum(2) +
                             (case.G + 1) * U24 * (bias.abs()[None] + (m.abs() * S.abs()).sum(2)) + 1e-30)
    return out


def _ratio(got, want, bound) -> float:
    r = (got.double() - want).abs() / bound
    return float(r.max()) if bool(torch.isfinite(r).all()) else float('inf')


def worst(case: Case, got: dict, want: dict) -> float:
    '''max over every output element of |got - want| / bound; inf for a non-finite element.'''
    if 'y' in want:
        return _ratio(got['y'], want['y'], want['y_bound'])
    return max(_ratio(got['w_out'], want['w_out'], want['w_bound']), _ratio(got['bias_out'], want['bias_out'], want['bias_bound']))


def check(case: Case, got: dict, want: dict) -> bool:
    '''Per element, |got - want| <= bound with want the float64 GroupNorm(+SiLU) of the fp16 inputs and the bound the sum
    of what the kernel's arithmetic can lose, nothing picked:

      statistics.  The kernels form sum x and sum x^2 of a group in fp32 and combine in fp64 (taken as exact).  An fp32
        add loses at most 2^-24 of the running sum of |x| (x^2), so with D = adds(case) the deepest chain of additions
        between an element and the partial sum it ends in -- slab: 2 per register (v_dot2 adds a pair) + the level-1 walk
        of ceil(pl / J) lanes; streaming: pixels per lane + PL lanes + ceil(cpg / 64) laps + 6 butterfly levels; supplied
        parts: 0 --
            d mean <= D 2^-24 mean|x|,     d var <= D 2^-24 E[x^2] + 2 |mean| d mean + d mean^2,
        and E[x^2] = var (1 + mean^2 / var): the case's own mean^2 / var sets how much of the variance the sums keep.
            rho = (1 - d var / (var + eps))^-1/2 - 1 + 2 * 2^-24       (relative, rstd; conversion to float, rstd * gamma)
      evaluation.  t = x sc + (beta - mean sc) in fp32, every product and sum rounding 2^-24 of its own size:
            e_t = rstd |gamma| (|x - mean| (rho + 2 * 2^-24) + d mean (1 + rho)) + 4 * 2^-24 ((|x| + |mean|) rstd |gamma| + |beta|)
        SiLU moves that to max |silu(t +- e_t) - silu(t)| and adds 2^-19 |want| for exp / rcp in fp32.
      the one rounding to half: 2^-11 (|want| + e), and 2^-24 absolute where the result is subnormal (SiLU near zero).

    Fold: w_out = half(wg * rstd) carries rho and the rounding; bias_out is compared with biasf - sum_g mean_g S_g over
    the kernel's OWN w_out (S_g its fp64 group sums), so only d mean, the (cpg - 1) fp32 adds behind each S_g (2^-24 of each running sum) and the G
    fmas of the chain remain: no rounding of w_out enters, which is what makes the indicator cases a direct view of
    mean and rstd.'''
    return worst(case, got, want) <= 1.0


def loose_bound_margin(case: Case, want: dict) -> float:
    '''max over elements of bound / (3e-3 + 3e-3 |want|), the project's earlier flat GroupNorm bound: must stay < 1.'''
    pairs = [('y', 'y_bound')] if 'y' in want else [('w_out', 'w_bound'), ('bias_out', 'bias_bound')]
    return max(float((want[b] / (3e-3 + 3e-3 * want[v].abs())).max()) for v, b in pairs if v in want)


# --------------------------------------------------------------------------------------------------- layouts
def x_layout(case: Case) -> dict:
    '''ldx, the element offset of x in its buffer and the buffer's size.'''
    C, rows = case.C, case.B * case.HW
    if case.layout == 'contig':
        return {'ldx': C, 'off': 0, 'size': rows * C}
    if case.layout == 'padded':
        ldx = C + 8 * (1 + case.seed % 3)
        return {'ldx': ldx, 'off': 0, 'size': rows * ldx}
    return {'ldx': C + 40, 'off': 16, 'size': rows * (C + 40)}


def x_buffer(case: Case, inp: dict):
    L = x_layout(case)
    buf = torch.full((L['size'],), JUNK, dtype=torch.float16)
    torch.as_strided(buf, (case.B * case.HW, case.C), (L['ldx'], 1), L['off']).copy_(inp['x16'].reshape(-1, case.C))
    return buf, L


# --------------------------------------------------------------------------------------------------- fp32 emulation
MUTANTS = ('drop_last_pixel', 'drop_chunk', 'slab_pad_in_n', 'group_shift', 'no_ch0', 'prev_sample', 'var_nm1', 'no_eps',
           'silu_flip', 'pad_read', 'fold_bias_unrounded', 'fold_extra_row')
VAR_NM1_VISIBLE = 256      # n / (n - 1) moves rstd by 1 / (2 n): below half an fp16 ulp (2^-12) once n > 2048, and the
                           # table promises to see it only where it is four ulps, n <= 256


def applies(case: Case, mutant: str) -> bool:
    '''Whether the mutant changes what the form of this case computes at all, and by more than one rounding to half can
    hide.  The cases that let a mutant through, by rule and not by name: var_nm1 where a group has more than 256 elements
    (rstd moves by 1 / (2 n)); no_eps where the variance is not near eps (all but the 'tiny' cases); fold_bias_unrounded
    at a group mean of 0 (the term it corrupts is mean * sum of roundings); and every mutant of a
    step the form does not have (a slab has no chunks, supplied parts have no pixels, contiguous x has no padding).'''
    f = expected_form(case)
    form = f['form']
    own_stats = form in ('slab256', 'slab1024', 'stream', 'fold')
    if mutant == 'drop_last_pixel':
        return own_stats
    if mutant == 'drop_chunk':
        return f['combine'] > 1 if 'combine' in f else False
    if mutant == 'slab_pad_in_n':
        return form.startswith('slab') and case.HW % f['pl'] != 0
    if mutant == 'group_shift':
        return own_stats and case.G > 1
    if mutant == 'no_ch0':
        return form.startswith('slab') and f['nblk'] > 1
    if mutant == 'prev_sample':
        return case.B > 1
    if mutant == 'var_nm1':
        return 1 < case.HW * case.cpg <= VAR_NM1_VISIBLE
    if mutant == 'no_eps':
        return case.xscale != 1.0
    if mutant == 'silu_flip':
        return form not in ('fold', 'fold_parts')
    if mutant == 'pad_read':
        return case.layout != 'contig' and form != 'fold_parts' and case.B * case.HW > 1
    if mutant == 'fold_bias_unrounded':
        return form in ('fold', 'fold_parts') and case.means >= 1
    if mutant == 'fold_extra_row':
        return form in ('fold', 'fold_parts') and case.N % GNF_ROWS != 0
    raise KeyError(mutant)


def _seq(t):
    '''Sum over the leading dimension, one fp32 (or fp64) addition after the other.'''
    acc = t[0].clone()
    for i in range(1, t.shape[0]):
        acc = acc + t[i]
    return acc


def _pad_to(t, dim, size):
    if t.shape[dim] == size:
        return t
    shape = list(t.shape)
    shape[dim] = size - t.shape[dim]
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype)], dim)


def emu_stream_parts(xs, f: dict, G: int, drop_chunk: bool = False):
    '''k_gn_stats on [B][HW][C] fp32: lane pl of a chunk walks pixels p0 + pl, + PL, ... adding into one register per
    channel; one thread per channel adds the PL lanes in turn; group g: lane i adds channels i, i + 64, ... and the wave
    folds with xor 32, 16, .. 1.  -> [B][nchunk][G][2] fp32.'''
    B, HW, C = xs.shape
    PL, nchunk, ppc, cpg = f['PL'], f['nchunk'], f['ppc'], C // G
    trips = cdiv(ppc, PL)
    v = _pad_to(xs, 1, nchunk * ppc).reshape(B, nchunk, ppc, C)
    v = _pad_to(v, 2, trips * PL).reshape(B, nchunk, trips, PL, C).permute(2, 3, 0, 1, 4)      # [trips][PL][B][nchunk][C]
    out = []
    for w in (v, v * v):                                   # x * x of an fp16 value is exact in fp32: fma(f, f, q) = q + f * f
        lane = _seq(w)                                     # [PL][B][nchunk][C]
        chan = torch.zeros_like(lane[0]) + lane[0]
        for l in range(1, PL):
            chan = chan + lane[l]
        laps = cdiv(cpg, 64)
        gl = _pad_to(chan.reshape(B, nchunk, G, cpg), 3, laps * 64).reshape(B, nchunk, G, laps, 64)
        acc = torch.zeros_like(gl[..., 0, :])
        for i in range(laps):
            acc = acc + gl[..., i, :]
        idx = torch.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., idx ^ o]
        out.append(acc[..., 0])
    parts = torch.stack(out, -1)
    if drop_chunk:
        parts[:, nchunk - 1] = 0
    return parts


def emu_slab_sums(xs, f: dict, G: int):
    '''gn_slab_body on [B][HW][C] fp32: lane pl keeps pixels pl, pl + PL, ... and adds channel pairs (v_dot2); level 1:
    thread (j, c) adds lanes j, j + J, ...; level 2 in fp64.  -> float64 (sum, sumsq) [B][G].'''
    B, HW, C = xs.shape
    pl, J = f['pl'], f['J']
    nv = cdiv(HW, pl)
    v = _pad_to(xs, 1, nv * pl).reshape(B, nv, pl, C // 2, 2).permute(1, 2, 0, 3, 4)              # [nv][pl][B][C/2][2]
    out = []
    for w in (v, v * v):
        acc = torch.zeros_like(w[0, ..., 0])
        for i in range(nv):
            acc = (acc + w[i, ..., 0]) + w[i, ..., 1]
        steps = cdiv(pl, J)
        lv = _pad_to(acc, 0, steps * J).reshape(steps, J, B, C // 2)
        a = torch.zeros_like(lv[0])
        for s in range(steps):
            a = a + lv[s]
        out.append(a.double().sum(0).reshape(B, G, -1).sum(2))
    return out[0], out[1]


def emulate(case: Case, inp: dict, mutant: Optional[str] = None) -> dict:
    '''The form of `case` in torch fp32 (statistics: the kernels' order of additions; combine in fp64; apply in fp32 and one
    rounding to half), optionally with one mutation.  Fold outputs come with GUARD sentinel elements at both ends, as the
    device test allocates them: {'y'} or {'w_out', 'bias_out', 'w_buf', 'bias_buf'}.'''
    assert mutant is None or (mutant in MUTANTS and applies(case, mutant))
    f = expected_form(case)
    form = f['form']
    B, HW, C, G, cpg = case.B, case.HW, case.C, case.G, case.cpg
    x16 = inp['x16']
    if mutant == 'pad_read':
        buf, L = x_buffer(case, inp)
        x16 = torch.as_strided(buf, (B, HW, C), (HW * C, C, 1), L['off'])
    xf = x16.float()
    n = float(HW * cpg)
    if form in ('apply_parts', 'fold_parts'):
        parts = inp['parts'].clone()
        if mutant == 'drop_chunk':
            parts[:, case.chunks - 1] = 0
        p = parts.double().sum(1)
        s, q = p[..., 0], p[..., 1]
    else:
        xs = xf
        if mutant == 'drop_last_pixel':
            xs = xf.clone()
            xs[:, HW - 1] = 0
        if mutant == 'group_shift':
            xs = torch.roll(xs, -1, 2)
        if form.startswith('slab'):
            s, q = emu_slab_sums(xs, f, G)
            if mutant == 'slab_pad_in_n':
                n = float(cdiv(HW, f['pl']) * f['pl'] * cpg)
        else:
            p = emu_stream_parts(xs, f, G, mutant == 'drop_chunk').double().sum(1)
            s, q = p[..., 0], p[..., 1]
    mean = s / n
    var = (q / n - mean * mean).clamp(min=0)
    if mutant == 'var_nm1':
        var = var * n / (n - 1)
    rstd = (var + (0.0 if mutant == 'no_eps' else case.eps)) ** -0.5
    mean, rstd = mean.float(), rstd.float()
    if mutant == 'prev_sample':
        mean, rstd = torch.roll(mean, 1, 0), torch.roll(rstd, 1, 0)
    if form in ('slab256', 'slab1024', 'stream', 'apply_parts'):
        gamma, beta = inp['gamma'], inp['beta']
        if mutant == 'no_ch0':
            gamma, beta = gamma[:f['CB']].repeat(f['nblk']), beta[:f['CB']].repeat(f['nblk'])
        sc = rstd.repeat_interleave(cpg, 1) * gamma[None]
        sh = beta[None] - mean.repeat_interleave(cpg, 1) * sc
        t = xf * sc[:, None, :] + sh[:, None, :]
        if case.silu != (mutant == 'silu_flip'):
            t = t * torch.sigmoid(t)
        return {'y': t.half()}
    N = case.N
    wf = inp['wg16'].float()[None] * rstd.repeat_interleave(cpg, 1)[:, None, :]                  # [B][N][C] fp32
    w16 = wf.half()
    src = (wf if mutant == 'fold_bias_unrounded' else w16.float()).reshape(B, N, G, cpg)
    gsum = torch.zeros((B, N, G))
    for c in range(cpg):
        gsum = gsum + src[..., c]
    acc = inp['biasf'][None].repeat(B, 1)
    for g in range(G):
        acc = acc - mean[:, g, None] * gsum[:, :, g]
    w_buf = torch.full((GUARD + B * N * C + GUARD,), SENTINEL, dtype=torch.float16)
    w_buf[GUARD:GUARD + B * N * C] = w16.reshape(-1)
    bias_buf = torch.full((GUARD + B * N + GUARD,), SENTINEL, dtype=torch.float32)
    bias_buf[GUARD:GUARD + B * N] = acc.reshape(-1)
    if mutant == 'fold_extra_row':      # the last block of the last sample writes row n0 + rows = N
        w_buf[GUARD + B * N * C:GUARD + B * N * C + min(C, GUARD)] = 0
        bias_buf[GUARD + B * N] = 0
    return {'w_out': w16, 'bias_out': acc, 'w_buf': w_buf, 'bias_buf': bias_buf}


def guards_intact(buf, lo: int, hi: int) -> bool:
    '''Every element of the flat buffer outside [lo, hi) still holds the sentinel, bit for bit.'''
    want = torch.full_like(buf, SENTINEL)
    bits = torch.int16 if buf.dtype == torch.float16 else torch.int32
    return bool(torch.equal(buf[:lo].view(bits), want[:lo].view(bits)) and torch.equal(buf[hi:].view(bits), want[hi:].view(bits)))


def accepted(case: Case, got: dict, inp: dict) -> float:
    '''Worst ratio to the bound; inf where a guard element changed.'''
    if 'w_buf' in got:
        n = case.B * case.N
        if not (guards_intact(got['w_buf'], GUARD, GUARD + n * case.C) and guards_intact(got['bias_buf'], GUARD, GUARD + n)):
            return float('inf')
    return worst(case, got, reference(case, inp, got))


# --------------------------------------------------------------------------------------------------- device run
def run_on_device(case: Case, dev, inp: dict) -> dict:
    '''One call of the route's entry point with buffers allocated here -> outputs on the host plus 'untouched' (every
    guard element of every output, and the workspace tail, kept its bits) and 'inputs_kept'.'''
    from flexdiffuse_amd import hip
    lib = hip.lib()
    B, HW, C, G, N = case.B, case.HW, case.C, case.G, case.N
    f = expected_form(case)
    keep = {}

    def dev_in(name, t):
        keep[name] = (t, t.to(dev))
        return keep[name][1]

    def ptr(t, off_elems=0):
        return t.data_ptr() + off_elems * t.element_size()

    if case.route != 'fold_parts':
        buf, L = x_buffer(case, inp)
        x = dev_in('x', buf)
    if case.route in ('full', 'apply_parts'):
        gamma, beta = dev_in('gamma', inp['gamma']), dev_in('beta', inp['beta'])
        y = torch.full((GUARD + B * HW * C + GUARD,), SENTINEL, dtype=torch.float16).to(dev)
    else:
        wg, biasf = dev_in('wg', inp['wg16'].reshape(-1)), dev_in('biasf', inp['biasf'])
        w = torch.full((GUARD + B * N * C + GUARD,), SENTINEL, dtype=torch.float16).to(dev)
        bo = torch.full((GUARD + B * N + GUARD,), SENTINEL, dtype=torch.float32).to(dev)
    if case.route in ('apply_parts', 'fold_parts'):
        parts = dev_in('parts', inp['parts'].reshape(-1))
    ws = None
    if case.route in ('full', 'fold'):
        nws = int(lib.fd_groupnorm_workspace_floats(B, G))
        assert nws == B * GN_MAX_CHUNKS * G * 2
        ws = torch.full((nws,), SENTINEL, dtype=torch.float32).to(dev)
    st = hip.stream()
    if case.route == 'full' and case.layout == 'contig':
        hip.call('fd_groupnorm_nhwc_f16', ptr(x), ptr(y, GUARD), ptr(gamma), ptr(beta), ptr(ws), B, HW, C, G, case.eps, int(case.silu), st)
    elif case.route == 'full':
        hip.call('fd_groupnorm_nhwc_ld_f16', ptr(x, L['off']), L['ldx'], ptr(y, GUARD), ptr(gamma), ptr(beta), ptr(ws), B, HW, C, G,
                 case.eps, int(case.silu), st)
    elif case.route == 'apply_parts':
        hip.call('fd_groupnorm_apply_parts_f16', ptr(x, L['off']), L['ldx'], ptr(y, GUARD), ptr(gamma), ptr(beta), ptr(parts),
                 case.chunks, B, HW, C, G, case.eps, int(case.silu), st)
    elif case.route == 'fold':
        hip.call('fd_groupnorm_fold_linear_f16', ptr(x, L['off']), L['ldx'], ptr(ws), B, HW, C, G, case.eps, ptr(wg), ptr(biasf), N,
                 ptr(w, GUARD), ptr(bo, GUARD), st)
    else:
        hip.call('fd_groupnorm_fold_linear_parts_f16', ptr(parts), case.chunks, B, HW, C, G, case.eps, ptr(wg), ptr(biasf), N,
                 ptr(w, GUARD), ptr(bo, GUARD), st)
    torch.cuda.synchronize()
    out = {'untouched': True}
    if case.route in ('full', 'apply_parts'):
        yb = y.cpu()
        out['y'] = yb[GUARD:GUARD + B * HW * C].reshape(B, HW, C).clone()
        out['untouched'] = guards_intact(yb, GUARD, GUARD + B * HW * C)
    else:
        wb, bb = w.cpu(), bo.cpu()
        out['w_out'] = wb[GUARD:GUARD + B * N * C].reshape(B, N, C).clone()
        out['bias_out'] = bb[GUARD:GUARD + B * N].reshape(B, N).clone()
        out['untouched'] = guards_intact(wb, GUARD, GUARD + B * N * C) and guards_intact(bb, GUARD, GUARD + B * N)
    if ws is not None:
        used = B * f['nchunk'] * G * 2 if f['form'] in ('stream', 'fold') else 0
        out['untouched'] = out['untouched'] and guards_intact(ws.cpu(), 0, used)
    out['inputs_kept'] = all(torch.equal(h, d.cpu()) for h, d in keep.values())
    return out


def call_refused(route: str, a: dict, dev):
    '''One call that the entry point must refuse, with real buffers of the sizes the arguments imply ->
    (return code, True when every output element kept its bits).  Nothing is launched.'''
    from flexdiffuse_amd import hip
    lib = hip.lib()
    B, HW, C, G, N, chunks = a['B'], a['HW'], a['C'], a['G'], a.get('N', 16), a.get('chunks', 1)
    ldx = a.get('ldx', C)
    f16 = lambda n, v: torch.full((n,), v, dtype=torch.float16).to(dev)
    f32 = lambda n, v: torch.full((n,), v, dtype=torch.float32).to(dev)
    x = f16(B * HW * max(ldx, C) + 16, 1.0)
    xp = x.data_ptr() + a.get('x_mis', 0)
    st = hip.stream()
    if route in ('full', 'apply_parts'):
        outs = [f16(B * HW * C, SENTINEL)]
        gamma, beta = f32(C, 1.0), f32(C, 0.0)
        if route == 'full':
            outs.append(f32(int(lib.fd_groupnorm_workspace_floats(B, G)), SENTINEL))
            rc = lib.fd_groupnorm_nhwc_ld_f16(xp, ldx, outs[0].data_ptr(), gamma.data_ptr(), beta.data_ptr(), outs[1].data_ptr(), B, HW, C, G,
                                              1e-5, 1, st)
        else:
            parts = f32(B * max(chunks, 1) * G * 2, 1.0)
            rc = lib.fd_groupnorm_apply_parts_f16(xp, ldx, outs[0].data_ptr(), gamma.data_ptr(), beta.data_ptr(), parts.data_ptr(), chunks,
                                                  B, HW, C, G, 1e-5, 1, st)
    else:
        wg, biasf = f16(N * C, 1.0), f32(N, 0.0)
        outs = [f16(B * N * C, SENTINEL), f32(B * N, SENTINEL)]
        if route == 'fold':
            outs.append(f32(int(lib.fd_groupnorm_workspace_floats(B, G)), SENTINEL))
            rc = lib.fd_groupnorm_fold_linear_f16(xp, ldx, outs[2].data_ptr(), B, HW, C, G, 1e-5, wg.data_ptr(), biasf.data_ptr(), N,
                                                  outs[0].data_ptr(), outs[1].data_ptr(), st)
        else:
            parts = f32(B * max(chunks, 1) * G * 2, 1.0)
            rc = lib.fd_groupnorm_fold_linear_parts_f16(parts.data_ptr(), chunks, B, HW, C, G, 1e-5, wg.data_ptr(), biasf.data_ptr(), N,
                                                        outs[0].data_ptr(), outs[1].data_ptr(), st)
    torch.cuda.synchronize()
    return rc, all(guards_intact(o.cpu(), 0, 0) for o in outs)
