'''What fd_gemm_f16's host path answers WITHOUT launching -- fd_gemm_plan's return code, tile and split, the refusal text, and
fd_gemm_gn_parts_chunks -- over a grid of descriptors (fake aligned pointers, never dereferenced) that reaches every argument check and
every tile / split the rule can give; plus fd_gemm_can_emit_row_stats / fd_gemm_can_fuse_groupnorm over a grid of their own.  Host logic
only, runs without a device.  The library reads its switches once per process: one child process per setting (default, every entry of
gemm_cases.ENV_SETTINGS, FD_GEMM_PP=0); the switches see every SWITCH_STRIDE-th row.  The golden file keeps, per setting, a SHA-256 per
block of 512 rows, the histogram of (code, tile, split) and the distinct refusal texts with their numbers stripped.

The golden file pins the behaviour of a REFERENCE build, so it is recorded from a library built from the commit BEFORE a refactor of the
host path, never from the code under test:
    FD_LIB_PATH=<reference build>/libflexdiffuse_hip.so python tests/golden/make_gemm_plan_sweep.py --update <commit the build is from>
    python tests/golden/make_gemm_plan_sweep.py                          compare the built library with the golden file
    python tests/golden/make_gemm_plan_sweep.py --rows SETTING BLOCK...  print the rows of some blocks (SETTING: default or NAME=VALUE)
The rows with residual_rows and gn_out together (res_rows_gn_out) are kept out of the blocks: the reference build accepted them and read
past the residual; they must be refused with FD_EINVAL.'''
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, 'gemm_plan_sweep.json')
LAUNCHES = os.path.join(HERE, 'gemm_launches_sd15_b8.json')
RULE_TABLE = os.path.join(HERE, 'gemm_rule_table.json')
BLOCK = 512
SWITCH_STRIDE = 7
FD_EINVAL = -1

# one distinctive piece of the text of every FD_CHECK_ARG site a plan query can reach: the 36 of fd_gemm_f16's own path, the 8 of the softmax form
MESSAGES = ('null pointer', 'M/N/K must be > 0', 'must be multiples of 8', 'pointers must be 16-byte aligned', 'conv needs Cin', 'conv input pixel stride',
            'K != kh*kw*Cin', 'M is not a multiple of out_h*out_w', 'upsample2x == 2 needs batch', 'fd_gemm_f16: lda=', 'A2 / K2 need', 'A2 >= 2 GiB', 'GEGLU needs',
            'ldc must be a multiple of 4', 'bias align', 'ldr must be a multiple of 4', 'needs a residual, a linear GEMM', 'ln_stats needs ln_colsum',
            'ln_stats / ln_colsum must be 16-byte aligned', 'ln_stats with trans_out needs', 'ln_stats_parts must be', 'trans_n0 needs C2', 'trans_n0 needs M',
            'trans_n0: operands >= 2 GiB', 'gn_out needs gn_gamma', 'gn_out needs a plain fp16 output', 'does not fit the finish kernel', 'sk_sync excludes gn_out',
            'ln_stats_out needs N == 320', 'addressing limit', 'batch_stride_bias needs', 'ln_stats / ln_stats_out need the LDS-DMA path',
            'upsample2x == 2: tile', 'with tile # (needs a multiple', 'not possible for this problem', 'ping-pong tile',
            'softmax_group needs a plain LayerNorm-fold', 'softmax_group must be 80', 'softmax_group needs N %', 'rows per launch slice is not a multiple',
            'softmax_group with batch > 1', 'softmax_group: operands >= 2 GiB', 'softmax_group needs the LDS-DMA path', 'softmax_group runs on tile')


def settings():
    import gemm_cases as gc
    return [{}] + [dict(e) for e in gc.ENV_SETTINGS] + [{'FD_GEMM_PP': '0'}]


def setting_name(env):
    return ','.join(f'{k}={v}' for k, v in sorted(env.items())) or 'default'


def strip_numbers(msg):
    return re.sub(r'\d+', '#', msg)


# ------------------------------------------------------------------------------------------------ the grid
def P(i, off=0):
    return 0x10000000 + 0x1000000 * i + off


MS = (64, 192, 1024, 1152, 2048, 4096, 4608, 16384, 65536, 73728)
NS = (4, 64, 128, 160, 256, 320, 512, 640, 1280, 2560, 10240)
KS = (64, 320, 640, 1280, 2560, 5120, 11520, 23040)
CINS = (64, 320, 1280, 2560)
HW = {64: (8, 8), 192: (8, 24), 1024: (32, 32), 1152: (24, 48), 2048: (32, 64), 4096: (64, 64), 4608: (48, 96), 16384: (128, 128), 65536: (64, 64),
      73728: (96, 96)}
WS_BYTES = 1 << 34


def linear(M, N, K):
    return dict(A=P(0), W=P(1), C=P(2), bias=P(3), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, workspace=P(6), workspace_bytes=WS_BYTES)


def conv(M, N, cin, k, stride, up=0):
    ho, wo = HW[M]
    d = linear(M, N, k * k * cin)
    d.update(conv=1, lda=0, in_c=cin, kh=k, kw=k, stride=stride, pad_t=k // 2, pad_l=k // 2, out_h=ho, out_w=wo, in_h=ho * stride, in_w=wo * stride,
             upsample2x=up)
    if up == 1:
        d.update(in_h=ho // 2, in_w=wo // 2)
    if up == 2:   # the phase-decomposed form: four 2x2 convolutions of the low-resolution input
        d.update(kh=2, kw=2, K=4 * cin, ldw=4 * cin, batch=4, pad_t=0, pad_l=0)
    return d


def _with(**kw):
    return lambda d: {**d, **kw}


def _rows_per_sample(d):
    return d['M'] // 2 if d['M'] % 512 == 0 else d['M']


def _variants():
    '''(name, function: base -> descriptor fields); each switches one feature of the descriptor on, some of them in a way the library refuses'''
    v = [('plain', _with())]
    v += [(f'act{a}', _with(act=a)) for a in (1, 2, 3, 4)]
    v += [('f32', _with(out_f32=1)), ('alpha', _with(alpha=0.5)),
          ('res', lambda d: {**d, 'residual': P(5), 'ldr': d['N']}),
          ('res_ldr', lambda d: {**d, 'residual': P(5), 'ldr': d['N'] + 2}),
          ('res_geglu', lambda d: {**d, 'residual': P(5), 'ldr': d['N'], 'act': 4}),
          ('res_rows_none', _with(residual_rows=256))]
    v += [(f'res_rows{r}', lambda d, r=r: {**d, 'residual': P(5), 'ldr': d['N'], 'residual_rows': r or d['M'] // 2}) for r in (0, 32, 256, 288)]
    v += [('bias2', lambda d: {**d, 'bias2': P(4), 'ld_bias2': d['N'], 'rows_per_sample': _rows_per_sample(d)}),
          ('ln', _with(ln_stats=P(7), ln_colsum=P(8))),
          ('ln_nocolsum', _with(ln_stats=P(7))),
          ('ln_align', _with(ln_stats=P(7, 8), ln_colsum=P(8))),
          ('ln_geglu', _with(ln_stats=P(7), ln_colsum=P(8), act=4)),
          ('ln_trans', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'trans_out': 1, 'trans_ld': d['M'], 'M': d['M'] + (2 if d['N'] == 64 else 0)})]
    v += [(f'ln_parts{p}', lambda d, p=p: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'ln_stats_parts': p, 'ln_stats_rows': d['M']}) for p in (2, 3, 4, 8)]
    v += [('ln_out', _with(ln_stats_out=P(9))),
          ('ln_out_res', lambda d: {**d, 'ln_stats_out': P(9), 'residual': P(5), 'ldr': d['N']}),
          ('ln_ln_out', _with(ln_stats=P(7), ln_colsum=P(8), ln_stats_out=P(9))),
          ('trans', lambda d: {**d, 'trans_out': 1, 'trans_ld': d['M'], 'rows_per_sample': _rows_per_sample(d)}),
          ('trans_n0', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'trans_n0': 160 if d['N'] <= 320 else d['N'] // 2, 'C2': P(15),
                                  'trans_ld': _rows_per_sample(d), 'rows_per_sample': _rows_per_sample(d)}),
          ('trans_n0_noc2', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'trans_n0': 160}),
          ('softmax', _with(ln_stats=P(7), ln_colsum=P(8), softmax_group=80, softmax_valid=77)),
          ('softmax_res', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'softmax_group': 80, 'softmax_valid': 77, 'residual': P(5), 'ldr': d['N']}),
          ('softmax40', _with(ln_stats=P(7), ln_colsum=P(8), softmax_group=40, softmax_valid=40)),
          ('softmax_b16', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'softmax_group': 80, 'softmax_valid': 80, 'batch': 16,
                                     'batch_stride_c': d['M'] * d['N'], 'batch_stride_w': d['N'] * d['K'], 'batch_stride_bias': d['N']}),
          ('softmax_b16_nobias', lambda d: {**d, 'ln_stats': P(7), 'ln_colsum': P(8), 'softmax_group': 80, 'softmax_valid': 80, 'batch': 16, 'bias': None}),
          ('gn_out', lambda d: {**d, 'gn_out': P(11), 'gn_gamma': P(12), 'gn_beta': P(13), 'gn_groups': 32, 'rows_per_sample': _rows_per_sample(d)}),
          ('gn_out_skip', lambda d: {**d, 'gn_out': P(11), 'gn_gamma': P(12), 'gn_beta': P(13), 'gn_groups': 32, 'gn_skip_c': 1, 'C': None, 'gn_silu': 1}),
          ('gn_out_nogamma', _with(gn_out=P(11), gn_groups=32)),
          ('gn_out_act', _with(gn_out=P(11), gn_gamma=P(12), gn_beta=P(13), gn_groups=32, act=1)),
          ('gn_out_sync', _with(gn_out=P(11), gn_gamma=P(12), gn_beta=P(13), gn_groups=32, sk_sync=P(10))),
          ('sk_sync', _with(sk_sync=P(10))),
          ('gn_part', lambda d: {**d, 'gn_part_out': P(14), 'gn_groups': 32, 'rows_per_sample': _rows_per_sample(d)}),
          ('gn_groups', lambda d: {**d, 'gn_groups': 32, 'rows_per_sample': _rows_per_sample(d), 'residual': P(5), 'ldr': d['N']}),
          ('batch2', lambda d: {**d, 'batch': 2, 'batch_stride_a': d['M'] * max(d['lda'], 64), 'batch_stride_c': d['M'] * d['N']}),
          ('batch16_bias', lambda d: {**d, 'batch': 16, 'batch_stride_w': d['N'] * d['K'], 'batch_stride_c': d['M'] * d['N'], 'batch_stride_bias': d['N']}),
          ('batch16_ln_out', lambda d: {**d, 'batch': 16, 'batch_stride_w': d['N'] * d['K'], 'batch_stride_c': d['M'] * d['N'], 'ln_stats_out': P(9)}),
          ('stride_bias_b1', lambda d: {**d, 'batch_stride_bias': d['N']}),
          ('k2', lambda d: {**d, 'A2': P(10), 'K2': 320, 'lda2': 320, 'ldw': d['K'] + 320}),
          ('k2_ldw', _with(A2=P(10), K2=320, lda2=320)),
          ('no_ws', _with(workspace=None, workspace_bytes=0)),
          ('ws_two', lambda d: {**d, 'workspace_bytes': 2 * d['M'] * d['N'] * 4}),
          ('split16_small_ws', lambda d: {**d, 'split_k': 16, 'workspace_bytes': 2 * d['M'] * d['N'] * 4}),
          ('ldc_pad', lambda d: {**d, 'ldc': d['N'] + 8}), ('ldc_odd', lambda d: {**d, 'ldc': d['N'] + 2}),
          ('lda_odd', lambda d: {**d, 'lda': d['lda'] + 4}), ('k_odd', lambda d: {**d, 'K': d['K'] + 4}),
          ('a_align', _with(A=P(0, 8))), ('bias_align', _with(bias=P(3, 4))), ('null_w', _with(W=None)), ('m0', _with(M=0))]
    return v


LINEAR_ONLY = ('ln', 'trans_n0', 'softmax', 'res_rows', 'batch16')


def _conv_variants():
    return [('cin', lambda d: {**d, 'in_c': d['in_c'] + 32, 'K': d['K'] + 32 * d['kh'] * d['kw'], 'ldw': d['ldw'] + 32 * d['kh'] * d['kw']}),
            ('pix', lambda d: {**d, 'lda': d['in_c'] + 8 * (1 + d['N'] % 3)}), ('pix_small', lambda d: {**d, 'lda': d['in_c'] - 8}),
            ('k_taps', lambda d: {**d, 'kh': d['kh'] + 1}), ('hw', lambda d: {**d, 'out_h': d['out_h'] + 1}),
            ('up1', lambda d: {**d, 'upsample2x': 1})]


def _big(d, lda):
    '''operands of 2 GiB and more: 73728 rows of `lda` halfs'''
    return {**d, 'M': 73728, 'lda': lda}


def descriptors():
    '''-> [(forced, name, fields)]: the rows of the sweep in a fixed order; `forced`: the descriptor names a tile'''
    out = []
    variants, conv_variants = _variants(), _conv_variants()
    bases = [(f'lin {M}x{N}x{K}', linear(M, N, K)) for M in MS for N in NS for K in KS]
    for k, s in ((3, 1), (3, 2), (1, 1), (1, 2)):
        bases += [(f'conv{k}s{s} {M}x{N}x{c}', conv(M, N, c, k, s)) for M in MS for N in NS for c in CINS]
    for i, (bname, b) in enumerate(bases):
        for j, (vname, f) in enumerate(variants):
            # (every base sees the plain form and a third of the features, in rotation)
            # (... a convolution only every fifth time one that belongs to linear GEMMs)
            if j == 0 or ((i + j) % 3 == 0 and not (b.get('conv') and vname.startswith(LINEAR_ONLY) and (i + j) % 5)):
                out.append((False, f'{bname} {vname}', f(b)))
        if b.get('conv'):
            vname, f = conv_variants[i % len(conv_variants)]
            out.append((False, f'{bname} {vname}', f(b)))
    # the phase-decomposed upsample under every tile
    for M in MS:
        for N in (256, 320, 1280):
            for c in (320, 1280):
                b = conv(M, N, c, 3, 1, up=2)
                out.append((False, f'phase {M}x{N}x{c}', b))
                out += [(False, f'phase {M}x{N}x{c} {n}', f(b)) for n, f in (('b1', _with(batch=1)), ('res', _with(residual=P(5), ldr=N)), ('split2', _with(split_k=2)))]
                out += [(True, f'phase {M}x{N}x{c} tile {t}', {**b, 'tile': t}) for t in range(1, 35)]
    # operands of 2 GiB and more
    for N in (64, 320, 1280):
        for K in (320, 1280):
            b = linear(73728, N, K)
            for lda in (16384, 32768):
                for vname, f in variants:
                    if vname in ('plain', 'act4', 'ln', 'ln_out', 'trans', 'trans_n0', 'softmax', 'batch16_bias', 'k2', 'res'):
                        out.append((False, f'big lda {lda} {N}x{K} {vname}', _big(f(b), lda)))
            out.append((False, f'big a2 {N}x{K}', {**b, 'A2': P(10), 'K2': 320, 'lda2': 16384, 'ldw': K + 320}))
            out.append((False, f'big w {N}x{K}', {**b, 'ldw': 1 << 22}))
            out.append((False, f'big c {N}x{K}', {**b, 'ldc': 32768}))
    # a GroupNorm slab too large for the finish kernel; the softmax form's own checks
    out += [(False, f'gn slab {M}', {**linear(M, 1280, 2560), 'gn_out': P(11), 'gn_gamma': P(12), 'gn_beta': P(13), 'gn_groups': g, 'split_k': 2})
            for M in (1024, 4096, 16384, 65536) for g in (1, 2, 32)]
    sm = dict(ln_stats=P(7), ln_colsum=P(8), softmax_group=80, softmax_valid=77)
    for M in (64, 96, 128, 256, 1024, 4096):
        for N in (160, 320, 1280):
            b = {**linear(M, N, 1280), **sm}
            out += [(bool(t), f'softmax {M}x{N} tile {t} batch {bt}', {**b, 'tile': t, 'batch': bt, 'batch_stride_c': M * N, 'batch_stride_w': N * 1280})
                    for t in (0, 13, 24, 25) for bt in (1, 16)]
            out += [(False, f'softmax {M}x{N} valid {n}', {**b, 'softmax_valid': n}) for n in (0, 1, 80, 81)]
            out += [(False, f'softmax {M}x{N} ldc', {**b, 'ldc': N + 4}), (False, f'softmax {M}x{N} split', {**b, 'split_k': 2})]
    # every tile id x forced split x workspace, on shapes of each kind
    forced_bases = [(f'lin {M}x{N}x{K}', linear(M, N, K)) for M in (192, 1024, 4096, 4608, 65536) for N in (64, 256, 320, 1280) for K in (320, 2560)]
    forced_bases += [(f'conv3 {M}x{N}x320', conv(M, N, 320, 3, 1)) for M in (1024, 4096, 4608, 65536) for N in (64, 256, 320, 1280)]
    forced_variants = [(n, f) for n, f in variants if n in ('plain', 'res_rows256', 'res_rows288', 'act4', 'ln', 'ln_out', 'no_ws', 'gn_part', 'gn_out', 'bias2', 'k2')]
    for i, (bname, b) in enumerate(forced_bases):
        for t in range(0, 35):
            for s in (0, 2, 4, 16):
                picks = [forced_variants[0], forced_variants[1 + (i + t + s) % (len(forced_variants) - 1)], forced_variants[1 + (i + 2 * t + s // 2 + 5) % (len(forced_variants) - 1)]]
                out += [(t > 0, f'{bname} {vname} tile {t} split {s}', {**f(b), 'tile': t, 'split_k': s}) for vname, f in picks]
    # the launches of the bench forward
    for n, r in enumerate(json.load(open(LAUNCHES))['launches']):
        out.append((False, f"bench {n} {r['what']}", {k: (v if not _is_pointer(k) else (None if v is None else P(n % 7, int(v)))) for k, v in r.items()
                                                     if k not in ('what', 'launches')}))
    return out


def res_rows_gn_out():
    '''descriptors with residual_rows and gn_out together, otherwise ones the library runs (split over K)'''
    out = []
    for M in (512, 1024):
        for N in (320, 640, 1280):
            for split in (0, 2, 4):
                b = linear(M, N, 2560)
                out.append({**b, 'gn_out': P(11), 'gn_gamma': P(12), 'gn_beta': P(13), 'gn_groups': 32, 'rows_per_sample': M // 2, 'split_k': split,
                            'residual': P(5), 'ldr': N, 'residual_rows': M // 2})
    return out


_POINTERS = None


def _is_pointer(name):
    global _POINTERS
    if _POINTERS is None:
        from flexdiffuse_amd import ops
        _POINTERS = {n for n, t in ops.fd_gemm_desc._fields_ if t is ctypes.c_void_p}
    return name in _POINTERS


# ------------------------------------------------------------------------------------------------ one process = one setting
def _answers(fields_list):
    '''-> ["rc|tile|split|chunks|refusal text"] of fd_gemm_plan / fd_gemm_gn_parts_chunks'''
    from flexdiffuse_amd import hip, ops
    lib = hip.lib()
    names = {n for n, _ in ops.fd_gemm_desc._fields_}
    tile, split = ctypes.c_int(0), ctypes.c_int(0)
    out = []
    for fields in fields_list:
        assert set(fields) <= names, set(fields) - names
        d = ops.fd_gemm_desc(**fields)
        rc = lib.fd_gemm_plan(ctypes.byref(d), ctypes.byref(tile), ctypes.byref(split))
        msg = lib.fd_last_error().decode('utf-8', 'replace') if rc else ''
        out.append(f'{rc}|{tile.value}|{split.value}|{lib.fd_gemm_gn_parts_chunks(ctypes.byref(d))}|{msg}')
    return out


def _helpers():
    from flexdiffuse_amd import hip
    lib = hip.lib()
    out = []
    for M in (0, 64, 128, 256, 1152, 4096, 4608, 65536, 73728):
        for N in (160, 320, 640, 1280, 2560):
            out += [lib.fd_gemm_can_emit_row_stats(M, N, K, ldc, ldr) for K in (0, 4, 320) for ldc in (N, N + 4, N + 8, 16384) for ldr in (0, N, N + 2)]
            out += [lib.fd_gemm_can_fuse_groupnorm(M, N, rows, g, s) for rows in (0, 64, 256, 1024, M) for g in (0, 1, 32, 48) for s in (1, 2, 3, 4, 8, 16, 32)]
    return out


def run_setting(switch, rows_of=()):
    '''In THIS process (whose environment holds the setting): the summary of the sweep; `rows_of`: blocks whose rows to list'''
    rows = descriptors()
    if switch:
        rows = rows[SWITCH_STRIDE // 2::SWITCH_STRIDE]
    ans = _answers([f for _, _, f in rows])
    hist = {'auto': {}, 'forced': {}}
    for (forced, _, _), a in zip(rows, ans):
        key = ','.join(a.split('|')[:3])
        h = hist['forced' if forced else 'auto']
        h[key] = h.get(key, 0) + 1
    res = {'rows': len(rows), 'blocks': [hashlib.sha256('\n'.join(ans[i:i + BLOCK]).encode()).hexdigest() for i in range(0, len(ans), BLOCK)],
           'auto': hist['auto'], 'forced': hist['forced'], 'messages': sorted({strip_numbers(a.split('|', 4)[4]) for a in ans if not a.startswith('0|')}),
           'helpers': hashlib.sha256(json.dumps(_helpers()).encode()).hexdigest(),
           'res_rows_gn_out': [a.split('|', 4)[::4] for a in _answers(res_rows_gn_out())]}
    if rows_of:
        res['listing'] = [f'{i} {name}: {a}   {json.dumps(f)}' for b in rows_of for i, ((_, name, f), a) in enumerate(zip(rows, ans)) if i // BLOCK == b]
    return res


def run_child(env, rows_of=()):
    e = {k: v for k, v in os.environ.items() if not k.startswith(('FD_GEMM_', 'FD_CONV_'))}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', json.dumps([bool(env)] + list(rows_of))], env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def sweep_all():
    '''{setting name: summary}, one child process per setting'''
    envs = settings()
    with ThreadPoolExecutor(max_workers=min(len(envs), os.cpu_count() or 1)) as ex:
        return dict(zip([setting_name(e) for e in envs], ex.map(run_child, envs)))


def conditions(res):
    '''What keeps the sweep from hiding a change; AssertionError where a summary {setting name: ...} misses one of them.'''
    d = res['default']
    seen = [m for r in res.values() for m in r['messages']]
    missing = [m for m in MESSAGES if not any(strip_numbers(m) in s for s in seen)]
    assert not missing, f'check messages the sweep never reaches: {missing}'
    auto = {tuple(int(x) for x in k.split(',')) for k in d['auto']}
    table = {(0, t['tile'], t['split_k']) for t in json.load(open(RULE_TABLE))}
    assert table <= auto, f'(tile, split) of the rule table the unforced rows never give: {sorted(table - auto)}'
    forced = {int(k.split(',')[1]) for k in d['forced'] if k.startswith('0,')}
    assert set(range(1, 34)) <= forced, f'tile ids no accepted forced row gives: {sorted(set(range(1, 34)) - forced)}'
    accepted = sum(n for h in (d['auto'], d['forced']) for k, n in h.items() if k.startswith('0,'))
    assert 2 * accepted >= d['rows'] >= 50000, (accepted, d['rows'])
    assert all(r['rows'] >= 5000 for r in res.values()), {k: r['rows'] for k, r in res.items()}
    assert len(res) == len(settings())


def main():
    if '--child' in sys.argv:
        switch, *rows_of = json.loads(sys.argv[sys.argv.index('--child') + 1])
        print(json.dumps(run_setting(switch, rows_of)))
        return
    if '--rows' in sys.argv:
        name, *blocks = sys.argv[sys.argv.index('--rows') + 1:]
        env = {} if name == 'default' else dict(kv.split('=') for kv in name.split(','))
        print('\n'.join(run_child(env, [int(b) for b in blocks])['listing']))
        return
    res = sweep_all()
    conditions(res)
    if '--update' in sys.argv:
        commit = sys.argv[sys.argv.index('--update') + 1]
        assert os.environ.get('FD_LIB_PATH'), 'record the golden file from a reference build (FD_LIB_PATH), not from the code under test'
        json.dump({'recorded_from': commit, 'settings': res}, open(GOLDEN, 'w'), indent=0, sort_keys=True)
        print(f'wrote {GOLDEN}: ' + ', '.join(f'{k}: {r["rows"]} rows' for k, r in res.items()))
        return
    gold = json.load(open(GOLDEN))['settings']
    for name, r in res.items():
        bad = [i for i, (a, b) in enumerate(zip(r['blocks'], gold[name]['blocks'])) if a != b]
        print(f'{name}: {r["rows"]} rows, blocks that differ from the golden file: {bad or "none"}' +
              ('' if r['helpers'] == gold[name]['helpers'] else '; the helper grid differs'))


if __name__ == '__main__':
    main()
