'''What the fifteen latent-step entry points (csrc/step.hip, composite.hip, window.hip) answer to a call WITHOUT a device, and what
the fifteen `ops.*_step` wrappers hand to `hip.call` -- host logic only.

Without a device a call that fails an argument check returns FD_EINVAL with its message and launches nothing; a call that passes
every check returns FD_EHIP with "<kernel family>: launch failed: ...".  So "refused, by which check" and "accepted, handed to
which kernel family" are both read here.  Every entry point gets a few valid base calls (`bases`), every single mutation of a
base call is a row (`mutations`), and so is every pair of two mutations that set different arguments.  A row records
(return code, class, kernel family): the class is the first keyword of CLASSES found in the message after the entry point's
name.  tests/golden/step_args_sweep.json holds, per entry point, the distinct answers [code, class, family, message] and per
base call one character per row (an index into the answers); tests/test_step_args_sweep.py replays the rows.

tests/golden/step_wrapper_calls.json: each wrapper called on CPU tensors over its options with `hip.call` replaced by the
recorder of tests/route_trace.py -- the entry name and the normalised argument list, or the AssertionError.

Both files pin a REFERENCE build: they are recorded from a library built from the commit BEFORE a refactor of the host path
(and, for the wrapper calls, with that commit's flexdiffuse_amd/ops.py on the path), never from the code under test:
    FD_LIB_PATH=<reference build>/libflexdiffuse_hip.so python tests/golden/make_step_args_sweep.py --update <commit>
    FD_REFERENCE_TREE=<checkout of that commit> python tests/golden/make_step_args_sweep.py --update-wrappers <commit>
    python tests/golden/make_step_args_sweep.py          compare the built library and the tree with the two files
The recorder refuses to run where it sees a GPU: its accepted rows are calls on host addresses that would really launch.

Intended differences between the reference build and the tree (tests/test_step_args_sweep.py allows these and nothing else):
  (a) fd_cfg_ddim_step_f32 and fd_composite_step_f32 reported every problem as "args"; the class may now be null / sizes.
  (b) rows the reference build accepted although its launch had one buffer written by some threads while others read it may
      be refused (class alias): NEWLY_REFUSED below names them; a pair is covered when one of its mutations is.
No row the reference build refused may be accepted.'''
import ctypes
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, 'step_args_sweep.json')
WRAPPERS = os.path.join(HERE, 'step_wrapper_calls.json')
FD_EINVAL, FD_EHIP = -1, -3

# the first keyword found in the text after "<entry point>: " names the class: the specific ones stand before the words they hold
CLASSES = ('combine-only', 'mask without', 'weights are null', 'blend', 'form', 'K-LMS', 'past 2^32', 'past 2^31', 'per must',
           'negative', 'larger than the canvas', 'stride', 'count rule', 'rescale', 'alias', 'null', 'n_prev', 'sizes', 'args')
FAMILIES = ('k_latent_step', 'k_latent_step_rescale', 'k_window_step', 'k_composite_step')
ALPHABET = ''.join(chr(c) for c in range(35, 127) if chr(c) != '\\')

# (b): entry point -> the single mutations that the reference build accepted and the tree refuses
NEWLY_REFUSED = {'fd_window_step_f32': {'eps_nhwc=windows_out'}}

# ---- the entry points: argument names in order; '*' a pointer, '.' a float, else an integer; the stream follows -------------
_DIMS = 'B C HW ld cfg guidance.'
_DDIM = 'c1. c2. c3. c4. v_prediction'
_MS = 'p. q. a. w0. w1.'
_LIN = 'form n_prev h1* h2* h3* h_out* x_keep_out* x_src* x_scaled_out* z0* noise* mask* ' + _DIMS + \
       ' w0. w1. w2. w3. a0. a1. a2. scale. k1. k2.'
_ADDR = 'seed sample_offset per draw'
_GRID = 'B C ld H W h w stride_y stride_x ny nx blend cfg guidance.'
ENTRIES = {
    'fd_cfg_ddim_step_f32': f'x* eps_nhwc* eps_out* {_DIMS} {_DDIM} do_step',
    'fd_cfg_ddim_masked_step_f32': f'x* eps_nhwc* z0* noise* mask* {_DIMS} {_DDIM} k1. k2.',
    'fd_cfg_multistep_step_f32': f'x* eps_nhwc* m0_out* m1* z0* noise* mask* {_DIMS} {_MS} k1. k2.',
    'fd_cfg_linear_multistep_step_f32': f'x* eps_nhwc* {_LIN}',
    'fd_cfg_ddim_noise_step_f32': f'x* eps_nhwc* z0* noise* mask* {_DIMS} {_DDIM} k1. k2. sigma. {_ADDR}',
    'fd_cfg_multistep_noise_step_f32': f'x* eps_nhwc* m0_out* m1* z0* noise* mask* {_DIMS} {_MS} k1. k2. sn. {_ADDR}',
    'fd_cfg_rescale_ddim_step_f32': f'x* eps_nhwc* eps_out* scale_out* z0* noise* mask* B C HW ld guidance. rescale. {_DDIM} '
                                    'do_step k1. k2. sigma. seed sample_offset draw',
    'fd_cfg_rescale_multistep_step_f32': f'x* eps_nhwc* m0_out* m1* scale_out* z0* noise* mask* B C HW ld guidance. rescale. {_MS} '
                                         'k1. k2. sn. seed sample_offset draw',
    'fd_composite_ddim_step_f32': f'x* eps_nhwc* weights* n_entities eps_out* z0* noise* mask* {_DIMS} {_DDIM} k1. k2. sigma. {_ADDR}',
    'fd_composite_multistep_step_f32': f'x* eps_nhwc* weights* n_entities m0_out* m1* z0* noise* mask* {_DIMS} {_MS} k1. k2. sn. '
                                       f'{_ADDR}',
    'fd_composite_linear_multistep_step_f32': f'x* eps_nhwc* weights* n_entities {_LIN}',
    'fd_composite_step_f32': f'x* eps_nhwc* weights* eps_out* B C HW ld n_entities cfg guidance. {_DDIM} do_step',
    'fd_window_step_f32': f'x* windows_out* eps_nhwc* eps_out* {_GRID} {_DDIM} do_step',
    'fd_window_ddim_step_f32': f'x* windows_out* eps_nhwc* eps_out* z0* noise* mask* {_GRID} {_DDIM} k1. k2. sigma. seed '
                               'sample_offset draw',
    'fd_window_multistep_step_f32': f'x* windows_out* eps_nhwc* m0_out* m1* z0* noise* mask* {_GRID} {_MS} k1. k2. sn. seed '
                                    'sample_offset draw',
}
# the kernel family an accepted call of each entry point names
FAMILY = {n: 'k_window_step' if 'window' in n else 'k_composite_step' if n == 'fd_composite_step_f32' else
          'k_latent_step_rescale' if 'rescale' in n else 'k_latent_step' for n in ENTRIES}
# the classes whose check exists on each entry point (the sweep must reach each at least once)
_NOISE = {'per must', 'negative', 'past 2^32'}
_BLEND = {'mask without', 'alias'}
_COMP = {'negative', 'weights are null'}
_LINC = {'null', 'sizes', 'form', 'n_prev', 'K-LMS'} | _BLEND
_WIN = {'null', 'sizes', 'larger than the canvas', 'stride', 'count rule', 'blend', 'alias'}
REACH = {
    'fd_cfg_ddim_step_f32': {'args', 'null'},
    'fd_cfg_ddim_masked_step_f32': {'null', 'sizes', 'alias'},
    'fd_cfg_multistep_step_f32': {'null', 'sizes'} | _BLEND,
    'fd_cfg_linear_multistep_step_f32': _LINC,
    'fd_cfg_ddim_noise_step_f32': {'null', 'sizes'} | _BLEND | _NOISE,
    'fd_cfg_multistep_noise_step_f32': {'null', 'sizes'} | _BLEND | _NOISE,
    'fd_cfg_rescale_ddim_step_f32': {'null', 'sizes', 'combine-only', 'rescale', 'past 2^31', 'negative', 'past 2^32'} | _BLEND,
    'fd_cfg_rescale_multistep_step_f32': {'null', 'sizes', 'rescale', 'past 2^31', 'negative', 'past 2^32'} | _BLEND,
    'fd_composite_ddim_step_f32': {'null', 'sizes'} | _BLEND | _NOISE | _COMP,
    'fd_composite_multistep_step_f32': {'null', 'sizes'} | _BLEND | _NOISE | _COMP,
    'fd_composite_linear_multistep_step_f32': _LINC | _COMP,
    'fd_composite_step_f32': {'args', 'null', 'weights are null'},
    'fd_window_step_f32': _WIN | {'combine-only'},
    'fd_window_ddim_step_f32': _WIN | {'mask without', 'negative', 'past 2^32', 'past 2^31'},
    'fd_window_multistep_step_f32': _WIN | {'mask without', 'negative', 'past 2^32', 'past 2^31'},
}


def params(entry):
    '''[(name, kind)] of an entry point's arguments: kind '*' pointer, '.' float, '' integer.'''
    return [(w.rstrip('*.'), w[-1] if w[-1] in '*.' else '') for w in ENTRIES[entry].split()]


_BUF = (ctypes.c_float * (64 * 16))()
_NAMES = sorted({n for e in ENTRIES for n, k in params(e) if k == '*'})


def addr(name):
    '''The host address that stands for pointer `name`: 256 bytes apart in one buffer, never dereferenced.'''
    return ctypes.addressof(_BUF) + 256 * _NAMES.index(name)


_VALUES = dict(B=1, C=4, HW=4, ld=4, cfg=1, guidance=7.5, c1=0.6, c2=0.8, c3=0.9, c4=0.3, v_prediction=0, do_step=1, k1=0.7, k2=0.3,
               p=1.0, q=-0.5, a=0.9, w0=0.1, w1=0.05, w2=0.0, w3=0.0, a0=1.0, a1=-0.5, a2=0.0, scale=0.0, sigma=0.0, sn=0.0, seed=5,
               sample_offset=0, per=16, draw=0, rescale=0.7, n_entities=0, form=0, n_prev=0, H=8, W=8, h=4, w=4, stride_y=2,
               stride_x=2, ny=3, nx=3, blend=0)
_STRIDE4 = dict(stride_y=4, stride_x=4, ny=2, nx=2)
_BLENDP = ('z0', 'noise', 'mask')


def _base(entry, off=(), **over):
    '''A valid call: every pointer set but those of `off`, the scalars of _VALUES but those of `over`.'''
    return {n: (None if n in off else addr(n)) if k == '*' else over.get(n, _VALUES[n]) for n, k in params(entry)}


def bases(entry):
    '''[(name, {argument: value})]: the valid calls of an entry point that between them take every option in each state.'''
    b = lambda name, off=(), **over: (name, _base(entry, off, **over))      # noqa: E731
    if entry in ('fd_cfg_ddim_step_f32', 'fd_composite_step_f32'):
        ent = entry == 'fd_composite_step_f32'
        return [b('step', n_entities=2) if ent else b('step'), b('combine', ('x',) + (('weights',) if ent else ()), do_step=0, cfg=0),
                b('step-no-eps_out', ('eps_out',), **({'n_entities': 2} if ent else {}))]
    if entry == 'fd_cfg_ddim_masked_step_f32':
        return [b('step'), b('blend-only', ('eps_nhwc',), ld=0)]
    if entry == 'fd_cfg_multistep_step_f32':
        return [b('order1', ('m1',) + _BLENDP), b('order2-mask')]
    if 'linear' in entry:
        ent = (lambda n: {'n_entities': n}) if 'composite' in entry else (lambda n: {})
        w = lambda n: () if n or 'composite' not in entry else ('weights',)      # noqa: E731
        return [b('plms-0', ('h1', 'h2', 'h3', 'x_scaled_out') + _BLENDP + w(0), **ent(0)),
                b('plms-3-mask', ('x_keep_out', 'x_src') + w(2), n_prev=3, **ent(2)),
                b('klms-1', ('h2', 'h3', 'x_keep_out', 'x_src') + _BLENDP + w(2), form=1, n_prev=1, scale=0.5, **ent(2)),
                b('klms-2-mask', ('h3', 'x_keep_out', 'x_src', 'x_scaled_out') + w(0), form=1, n_prev=2, **ent(0))]
    if entry == 'fd_cfg_ddim_noise_step_f32':
        return [b('noise', _BLENDP, sigma=0.2), b('mask', sigma=0.0)]
    if entry == 'fd_cfg_multistep_noise_step_f32':
        return [b('noise-order1', ('m1',) + _BLENDP, sn=0.2), b('mask-order2', sn=0.0)]
    if entry == 'fd_cfg_rescale_ddim_step_f32':
        return [b('step-mask-noise', sigma=0.2), b('combine', ('x', 'scale_out') + _BLENDP, do_step=0),
                b('step', ('eps_out',) + _BLENDP)]
    if entry == 'fd_cfg_rescale_multistep_step_f32':
        return [b('noise-order1', ('m1',) + _BLENDP, sn=0.2), b('mask-order2', ('scale_out',))]
    if entry == 'fd_composite_ddim_step_f32':
        return [b('entities-mask-noise', n_entities=2, sigma=0.2), b('plain', ('weights', 'eps_out') + _BLENDP)]
    if entry == 'fd_composite_multistep_step_f32':
        return [b('entities-mask-noise', n_entities=2, sn=0.2), b('plain', ('weights', 'm1') + _BLENDP)]
    if entry == 'fd_window_step_f32':
        return [b('step-tent', blend=1), b('combine', ('x', 'windows_out'), do_step=0, cfg=0, **_STRIDE4),
                b('step-bare', ('windows_out', 'eps_out'))]
    if entry == 'fd_window_ddim_step_f32':
        return [b('mask-noise', sigma=0.2), b('plain', ('windows_out', 'eps_out') + _BLENDP, **_STRIDE4)]
    assert entry == 'fd_window_multistep_step_f32', entry
    return [b('mask-noise-order2', sn=0.2, blend=1), b('plain', ('windows_out', 'm1') + _BLENDP, **_STRIDE4)]


def mutations(entry, base):
    '''[(name, {argument: value})]: every single mutation of a base call.  An alias sets a pointer to the address another one
    has in the BASE call, so two mutations that set different arguments never interfere.'''
    have = dict(params(entry))
    ptrs = [n for n, k in params(entry) if k == '*' and base[n] is not None]
    out = [(f'{p}=NULL', {p: None}) for p in ptrs]
    out += [(f'{q}={p}', {q: base[p]}) for p, q in itertools.combinations(ptrs, 2)]
    out += [(f'{n}=0', {n: 0}) for n in ('B', 'C', 'HW') if n in have]
    out.append(('ld=C-1', {'ld': base['C'] - 1}))

    def scalar(name, *values):
        return [(f'{name}={v}', {name: v}) for v in values] if name in have else []
    out += scalar('form', -1, 2) + scalar('n_prev', -1, 4) + scalar('n_entities', -1) + scalar('rescale', -0.1, 1.1)
    out += scalar('blend', 2) + scalar('h', 9) + scalar('stride_y', 0) + scalar('stride_x', 5) + scalar('per', 0, 5)
    out += scalar('draw', -1) + scalar('sample_offset', -1, 2 ** 32)
    if 'ny' in have:
        out.append(('ny+1', {'ny': base['ny'] + 1}))
    if 'rescale' in have:
        out.append(('C*HW=2^31', {'C': 1 << 16, 'HW': 1 << 15, 'ld': 1 << 16}))
    if 'H' in have and 'sample_offset' in have:
        out.append(('C*H*W=2^31', {'C': 1 << 25, 'ld': 1 << 25}))
    return out


def rows(entry, base):
    '''-> (names, [{argument: value}]): the single mutations, then every pair of them that sets different arguments.'''
    muts = mutations(entry, base)
    names, calls = [n for n, _ in muts], [m for _, m in muts]
    for (na, a), (nb, b) in itertools.combinations(muts, 2):
        if not set(a) & set(b):
            names.append(f'{na} & {nb}')
            calls.append({**a, **b})
    return len(muts), names, calls


def classify(entry, rc, msg):
    '''(return code, class, kernel family, message) of an answer.'''
    head, _, text = msg.partition(': ')
    if rc == FD_EINVAL:
        assert head == entry, (entry, msg)
        cls = next((c for c in CLASSES if c in text), None)
        assert cls is not None, f'no class for {msg!r}'
        return [rc, cls, None, msg]
    assert rc == FD_EHIP and text.startswith('launch failed') and head in FAMILIES, (entry, rc, msg)
    return [rc, 'accepted', head, msg]


def no_device():
    import torch
    return torch.cuda.device_count() == 0


def answer(lib, entry, base, change):
    args = {**base, **change}
    rc = getattr(lib, entry)(*[args[n] for n, _ in params(entry)], None)
    return classify(entry, rc, lib.fd_last_error().decode('utf-8', 'replace'))


def sweep(accepted_from=None):
    '''{entry: {'answers': [...], 'bases': [{'name', 'singles', 'rows', 'names', 'row'}]}} of the loaded library.  With
    `accepted_from` (a golden file's 'entries'; for a machine that has a device) the rows that file accepted are not called:
    they keep the golden's answer.'''
    sys.path.insert(0, ROOT)
    from flexdiffuse_amd import hip
    lib = hip.lib()
    assert accepted_from is not None or no_device(), 'a device is present: an accepted row would launch on host addresses'
    out = {}
    for entry in ENTRIES:
        answers, recs = [], []
        for k, (bname, base) in enumerate(bases(entry)):
            gold = accepted_from and accepted_from[entry]
            if not accepted_from:
                ok = answer(lib, entry, base, {})
                assert ok[1:3] == ['accepted', FAMILY[entry]], (entry, bname, ok)
            singles, names, calls = rows(entry, base)
            row = []
            for i, change in enumerate(calls):
                if gold and gold['answers'][ALPHABET.index(gold['bases'][k]['row'][i])][1] == 'accepted':
                    a = gold['answers'][ALPHABET.index(gold['bases'][k]['row'][i])]
                else:
                    a = answer(lib, entry, base, change)
                if a not in answers:
                    answers.append(a)
                row.append(ALPHABET[answers.index(a)])
            recs.append({'name': bname, 'singles': singles, 'rows': len(names), 'names': hashlib.sha1('\n'.join(names).encode()).hexdigest(),
                         'row': ''.join(row)})
        assert len(answers) <= len(ALPHABET), (entry, len(answers))
        out[entry] = {'answers': answers, 'bases': recs}
    return out


def decoded(entry_record):
    '''[(base name, singles, [answer per row])] of one entry point's record.'''
    return [(b['name'], b['singles'], [entry_record['answers'][ALPHABET.index(c)] for c in b['row']]) for b in entry_record['bases']]


def pair_classes(a, b, names):
    '''The classes a refused pair of mutations (named names[0] & names[1]) may report: that of either single mutation -- which
    of two simultaneous violations is reported first is not part of the contract -- and, where each mutation sets a pointer to
    another's address, alias: the two may have been made equal to each other.'''
    both_alias = all('=' in n and not n.endswith('=NULL') and n.split('=')[0] in _NAMES and n.split('=')[1] in _NAMES for n in names)
    return {a, b} | ({'alias'} if both_alias else set())


def conditions(entries):
    '''What keeps the sweep from hiding a change: every class reached on every entry point where its check exists, an accepted
    row of the expected kernel family per entry point, and the pair rule on the recorded answers themselves.'''
    for entry, rec in entries.items():
        seen = {a[1] for a in rec['answers']}
        assert REACH[entry] <= seen, f'{entry}: classes the sweep never reaches: {sorted(REACH[entry] - seen)}'
        assert any(a[2] == FAMILY[entry] for a in rec['answers']), entry
        assert all(a[2] in (None, FAMILY[entry]) for a in rec['answers']), entry
        for (bname, base), (_, singles, ans) in zip(bases(entry), decoded(rec)):
            _, names, _ = rows(entry, base)
            single = dict(zip(names[:singles], ans))
            for name, a in zip(names[singles:], ans[singles:]):
                if a[0] == FD_EINVAL:
                    na, nb = name.split(' & ')
                    assert a[1] in pair_classes(single[na][1], single[nb][1], (na, nb)), (entry, bname, name, a, single[na], single[nb])


# ---- the wrappers ------------------------------------------------------------------------------------------------------------
def wrapper_calls():
    '''{case name: [entry, normalised arguments] | ['AssertionError']}: every `ops.*_step` wrapper on CPU tensors over its options.
    FD_REFERENCE_TREE: the checkout whose flexdiffuse_amd is recorded (default: this tree).'''
    sys.path.insert(0, os.environ.get('FD_REFERENCE_TREE') or ROOT)
    sys.path.insert(1, os.path.dirname(HERE))
    import torch
    from flexdiffuse_amd import hip, ops
    from flexdiffuse_amd.noise import PhiloxNoise
    from route_trace import _arg
    seen = []
    saved = hip.call, hip.stream, hip.require_device
    hip.call, hip.stream, hip.require_device = (lambda name, *a: seen.append([name, [_arg(v) for v in a]])), (lambda: None), (lambda *t: None)
    B, C, HW, n = 2, 4, 16, 2
    grid = (8, 8, 4, 4, 2, 2, 3, 3)
    Wn, hw, canvas = 9, 16, 64
    t = lambda *shape: torch.zeros(shape)      # noqa: E731
    lat = lambda: t(B, C, HW)                   # noqa: E731
    can = lambda: t(B, C, canvas)               # noqa: E731
    eps = lambda rep: t(rep * B * HW, C + 4)[:, :C]          # row stride C + 4     # noqa: E731
    weps = lambda rep: t(rep * B * Wn * hw, C)  # noqa: E731
    masks = {'nomask': None, 'mask': (lat(), lat(), t(HW), 0.7, 0.3)}
    wmasks = {'nomask': None, 'mask': (can(), can(), t(canvas), 0.7, 0.3)}
    noises = {'nonoise': None, 'noise': PhiloxNoise(5, 3)}
    maps = {'w-none': (None, 0), 'w-0': (t(0, HW), 0), 'w-2': (t(n, HW), n)}
    opt = {'none': None}
    d4, m5 = (0.6, 0.8, 0.9, 0.3), (1.0, -0.5, 0.9, 0.1, 0.05)
    out = {}

    def rec(name, f):
        del seen[:]
        try:
            f()
            assert len(seen) == 1, (name, seen)
            out[name] = seen[0]
        except AssertionError:
            out[name] = ['AssertionError']

    P = itertools.product
    try:
        for cfg, do_step, eo in P((0, 1), (0, 1), (0, 1)):
            rec(f'cfg_ddim_step/cfg={cfg}/do_step={do_step}/eps_out={eo}',
                lambda: ops.cfg_ddim_step(lat() if do_step else None, eps(1 + cfg), B, C, HW, bool(cfg), 7.5, d4, True, bool(do_step), lat() if eo else None))
        rec('cfg_ddim_step/defaults', lambda: ops.cfg_ddim_step(lat(), eps(1), B, C, HW, False, 1.0))
        rec('cfg_ddim_step/short-eps', lambda: ops.cfg_ddim_step(lat(), eps(1), B, C, HW, True, 7.5))
        rec('cfg_ddim_step/f64', lambda: ops.cfg_ddim_step(lat().double(), eps(1), B, C, HW, False, 7.5))
        rec('cfg_ddim_step/eps-strided', lambda: ops.cfg_ddim_step(lat(), t(C, B * HW).t(), B, C, HW, False, 7.5))
        for e in (0, 1):
            rec(f'cfg_ddim_masked_step/eps={e}', lambda: ops.cfg_ddim_masked_step(lat(), eps(2) if e else None, lat(), lat(), t(HW), B, C, HW, bool(e), 7.5, d4, False, 0.7, 0.3))
        rec('cfg_ddim_masked_step/defaults', lambda: ops.cfg_ddim_masked_step(lat(), None, lat(), lat(), t(HW), B, C, HW))
        rec('cfg_ddim_masked_step/mask-size', lambda: ops.cfg_ddim_masked_step(lat(), None, lat(), lat(), t(HW + 1), B, C, HW))
        for (mn, mk), m1 in P(masks.items(), (0, 1)):
            rec(f'cfg_multistep_step/{mn}/m1={m1}', lambda: ops.cfg_multistep_step(lat(), eps(2), lat(), lat() if m1 else None, B, C, HW, True, 7.5, m5, mk))
        rec('cfg_multistep_step/short-eps', lambda: ops.cfg_multistep_step(lat(), eps(1), lat(), None, B, C, HW, True, 7.5, m5))
        rec('cfg_multistep_step/m0-size', lambda: ops.cfg_multistep_step(lat(), eps(1), t(B, C, HW + 1), None, B, C, HW, False, 7.5, m5))
        for comp in (0, 1):
            for form, nh, (mn, mk), extra, (wn, (wm, wk)) in P((0, 1), range(4), masks.items(), (0, 1), maps.items() if comp else [('', (None, 0))]):
                name = ('composite_' if comp else 'cfg_') + 'linear_multistep_step'
                kw = {}
                if extra:
                    kw = dict(x_scaled_out=lat(), scale=0.5) if form else dict(x_keep_out=lat(), x_src=lat())
                args = (form, [lat() for _ in range(nh)], lat() if form or not extra else None, B, C, HW, True, 7.5, [0.5] * (nh + 1),
                        (-2.0, 0.5, -0.5) if form else (0.9, 0.1), mk)
                f = (lambda: ops.composite_linear_multistep_step(lat(), eps(2 + wk), wm, *args, **kw)) if comp else \
                    (lambda: ops.cfg_linear_multistep_step(lat(), eps(2), *args, **kw))
                rec(f'{name}/form={form}/hist={nh}/{mn}/extra={extra}/{wn}', f)
            for bad, a in (('hist-4', (0, [lat()] * 4, lat(), B, C, HW, True, 7.5, [0.5], (0.9, 0.1))),
                           ('weights-5', (0, [], lat(), B, C, HW, True, 7.5, [0.5] * 5, (0.9, 0.1))),
                           ('coef-3-plms', (0, [], lat(), B, C, HW, True, 7.5, [0.5], (0.9, 0.1, 0.0))),
                           ('coef-2-klms', (1, [], lat(), B, C, HW, True, 7.5, [0.5], (0.9, 0.1))),
                           ('hist-f16', (0, [lat().half()], lat(), B, C, HW, True, 7.5, [0.5, 0.5], (0.9, 0.1)))):
                rec(f'{name}/{bad}', (lambda: ops.composite_linear_multistep_step(lat(), eps(4), t(n, HW), *a)) if comp else
                    (lambda: ops.cfg_linear_multistep_step(lat(), eps(2), *a)))
        rec('composite_linear_multistep_step/short-eps', lambda: ops.composite_linear_multistep_step(lat(), eps(3), t(n, HW), 0, [], lat(), B, C, HW, True, 7.5, [0.5], (0.9, 0.1)))
        rec('composite_linear_multistep_step/map-size', lambda: ops.composite_linear_multistep_step(lat(), eps(4), t(n, HW + 1), 0, [], lat(), B, C, HW, True, 7.5, [0.5], (0.9, 0.1)))
        for (mn, mk), sg in P(masks.items(), (0.0, 0.2)):
            rec(f'cfg_ddim_noise_step/{mn}/sigma={sg}', lambda: ops.cfg_ddim_noise_step(lat(), eps(2), B, C, HW, True, 7.5, d4, False, sg, noises['noise'], C * HW, 2, mk))
            for m1 in (0, 1):
                rec(f'cfg_multistep_noise_step/{mn}/sn={sg}/m1={m1}',
                    lambda: ops.cfg_multistep_noise_step(lat(), eps(2), lat(), lat() if m1 else None, B, C, HW, True, 7.5, m5, sg, noises['noise'], C * HW, 2, mk))
        rec('cfg_ddim_noise_step/short-eps', lambda: ops.cfg_ddim_noise_step(lat(), eps(1), B, C, HW, True, 7.5, d4, False, 0.2, noises['noise'], 64, 0))
        rec('cfg_multistep_noise_step/short-eps', lambda: ops.cfg_multistep_noise_step(lat(), eps(1), lat(), None, B, C, HW, True, 7.5, m5, 0.2, noises['noise'], 64, 0))
        for (mn, mk), (nn, nz), sg, do_step, eo, so in P(masks.items(), noises.items(), (0.0, 0.2), (0, 1), (0, 1), (0, 1)):
            rec(f'cfg_rescale_ddim_step/{mn}/{nn}/sigma={sg}/do_step={do_step}/eps_out={eo}/scale_out={so}',
                lambda: ops.cfg_rescale_ddim_step(lat() if do_step or mk else None, eps(2), B, C, HW, 7.5, 0.7, d4, True, bool(do_step), lat() if eo else None,
                                                  t(B) if so else None, mk, sg, nz, 3))
        rec('cfg_rescale_ddim_step/defaults', lambda: ops.cfg_rescale_ddim_step(lat(), eps(2), B, C, HW, 7.5, 0.7))
        rec('cfg_rescale_ddim_step/short-eps', lambda: ops.cfg_rescale_ddim_step(lat(), eps(1), B, C, HW, 7.5, 0.7))
        rec('cfg_rescale_ddim_step/scale_out-size', lambda: ops.cfg_rescale_ddim_step(lat(), eps(2), B, C, HW, 7.5, 0.7, scale_out=t(B + 1)))
        for (mn, mk), (nn, nz), sg, m1, so in P(masks.items(), noises.items(), (0.0, 0.2), (0, 1), (0, 1)):
            rec(f'cfg_rescale_multistep_step/{mn}/{nn}/sn={sg}/m1={m1}/scale_out={so}',
                lambda: ops.cfg_rescale_multistep_step(lat(), eps(2), lat(), lat() if m1 else None, B, C, HW, 7.5, 0.7, m5, mk, t(B) if so else None, sg, nz, 3))
        rec('cfg_rescale_multistep_step/defaults', lambda: ops.cfg_rescale_multistep_step(lat(), eps(2), lat(), None, B, C, HW, 7.5, 0.7, m5))
        rec('cfg_rescale_multistep_step/short-eps', lambda: ops.cfg_rescale_multistep_step(lat(), eps(1), lat(), None, B, C, HW, 7.5, 0.7, m5))
        for (wn, (wm, wk)), cfg, do_step, eo in P(maps.items(), (0, 1), (0, 1), (0, 1)):
            if wn != 'w-0':
                rec(f'composite_step/{wn}/cfg={cfg}/do_step={do_step}/eps_out={eo}',
                    lambda: ops.composite_step(lat() if do_step else None, eps(cfg + 1 + wk), wm, B, C, HW, bool(cfg), 7.5, d4, True, bool(do_step), lat() if eo else None))
        rec('composite_step/short-eps', lambda: ops.composite_step(lat(), eps(3), t(n, HW), B, C, HW, True, 7.5))
        rec('composite_step/map-size', lambda: ops.composite_step(lat(), eps(4), t(n, HW + 1), B, C, HW, True, 7.5))
        for (wn, (wm, wk)), (mn, mk), (nn, nz), sg, per, eo in P(maps.items(), masks.items(), noises.items(), (0.0, 0.2), (0, 32), (0, 1)):
            rec(f'composite_ddim_step/{wn}/{mn}/{nn}/sigma={sg}/per={per}/eps_out={eo}',
                lambda: ops.composite_ddim_step(lat(), eps(2 + wk), wm, B, C, HW, True, 7.5, d4, False, mk, sg, nz, per, 2, lat() if eo else None))
            rec(f'composite_multistep_step/{wn}/{mn}/{nn}/sn={sg}/per={per}/m1={eo}',
                lambda: ops.composite_multistep_step(lat(), eps(2 + wk), wm, lat(), lat() if eo else None, B, C, HW, True, 7.5, m5, mk, sg, nz, per, 2))
        rec('composite_ddim_step/defaults', lambda: ops.composite_ddim_step(lat(), eps(1), None, B, C, HW, False, 1.0, d4))
        rec('composite_ddim_step/short-eps', lambda: ops.composite_ddim_step(lat(), eps(3), t(n, HW), B, C, HW, True, 7.5, d4))
        rec('composite_ddim_step/map-size', lambda: ops.composite_ddim_step(lat(), eps(4), t(n, HW + 1), B, C, HW, True, 7.5, d4))
        rec('composite_ddim_step/map-strided', lambda: ops.composite_ddim_step(lat(), eps(4), t(HW, n).t(), B, C, HW, True, 7.5, d4))
        rec('composite_multistep_step/defaults', lambda: ops.composite_multistep_step(lat(), eps(1), None, lat(), None, B, C, HW, False, 1.0, m5))
        rec('composite_multistep_step/short-eps', lambda: ops.composite_multistep_step(lat(), eps(3), t(n, HW), lat(), None, B, C, HW, True, 7.5, m5))
        for cfg, do_step, wo, eo in P((0, 1), (0, 1), (0, 1), (0, 1)):
            rec(f'window_step/cfg={cfg}/do_step={do_step}/windows_out={wo}/eps_out={eo}',
                lambda: ops.window_step(can() if do_step else None, t(B * Wn, C, hw) if wo else None, weps(1 + cfg), B, C, grid, 1, bool(cfg), 7.5, d4, True,
                                        bool(do_step), can() if eo else None))
        rec('window_step/defaults', lambda: ops.window_step(can(), None, weps(1), B, C, grid, 0, False, 1.0))
        rec('window_step/short-eps', lambda: ops.window_step(can(), None, weps(1), B, C, grid, 0, True, 7.5))
        rec('window_step/windows-size', lambda: ops.window_step(can(), t(B * Wn, C, hw + 1), weps(1), B, C, grid, 0, False, 7.5))
        for (mn, mk), (nn, nz), sg, wo, eo in P(wmasks.items(), noises.items(), (0.0, 0.2), (0, 1), (0, 1)):
            rec(f'window_ddim_step/{mn}/{nn}/sigma={sg}/windows_out={wo}/eps_out={eo}',
                lambda: ops.window_ddim_step(can(), t(B * Wn, C, hw) if wo else None, weps(2), B, C, grid, 1, True, 7.5, d4, False, mk, sg, nz, 2, can() if eo else None))
            rec(f'window_multistep_step/{mn}/{nn}/sn={sg}/windows_out={wo}/m1={eo}',
                lambda: ops.window_multistep_step(can(), t(B * Wn, C, hw) if wo else None, weps(2), can(), can() if eo else None, B, C, grid, 1, True, 7.5, m5, mk,
                                                  sg, nz, 2))
        rec('window_ddim_step/defaults', lambda: ops.window_ddim_step(can(), None, weps(1), B, C, grid, 0, False, 1.0, d4))
        rec('window_ddim_step/short-eps', lambda: ops.window_ddim_step(can(), None, weps(1), B, C, grid, 0, True, 7.5, d4))
        rec('window_ddim_step/mask-size', lambda: ops.window_ddim_step(can(), None, weps(1), B, C, grid, 0, False, 7.5, d4, mask=(can(), can(), t(HW), 1.0, 0.0)))
        rec('window_multistep_step/defaults', lambda: ops.window_multistep_step(can(), None, weps(1), can(), None, B, C, grid, 0, False, 1.0, m5))
        rec('window_multistep_step/m0-size', lambda: ops.window_multistep_step(can(), None, weps(1), lat(), None, B, C, grid, 0, False, 7.5, m5))
    finally:
        hip.call, hip.stream, hip.require_device = saved
    return out


def main():
    if '--update-wrappers' in sys.argv:
        commit = sys.argv[sys.argv.index('--update-wrappers') + 1]
        assert os.environ.get('FD_REFERENCE_TREE'), 'record the wrapper calls from a checkout of the reference commit (FD_REFERENCE_TREE)'
        calls = wrapper_calls()
        json.dump({'recorded_from': commit, 'calls': calls}, open(WRAPPERS, 'w'), indent=0, sort_keys=True)
        print(f'wrote {WRAPPERS}: {len(calls)} calls, {sum(v == ["AssertionError"] for v in calls.values())} refused')
        return
    entries = sweep()
    total = sum(b['rows'] for r in entries.values() for b in r['bases'])
    if '--update' in sys.argv:
        commit = sys.argv[sys.argv.index('--update') + 1]
        assert os.environ.get('FD_LIB_PATH'), 'record the golden file from a reference build (FD_LIB_PATH), not from the code under test'
        conditions(entries)
        json.dump({'recorded_from': commit, 'classes': list(CLASSES), 'intended_differences': __doc__.split('Intended differences')[1].strip().splitlines()[1:],
                   'newly_refused': {k: sorted(v) for k, v in NEWLY_REFUSED.items()}, 'entries': entries}, open(GOLDEN, 'w'), indent=0, sort_keys=True)
        print(f'wrote {GOLDEN}: {total} rows')
        return
    gold = json.load(open(GOLDEN))['entries']
    for entry, r in entries.items():
        pairs = [(a, b) for (_, _, x), (_, _, y) in zip(decoded(r), decoded(gold[entry])) for a, b in zip(x, y)]
        print(f'{entry}: {len(pairs)} rows; against the golden file {sum(a[0] != b[0] or a[2] != b[2] for a, b in pairs)} differ in code or '
              f'family, {sum(a[1] != b[1] for a, b in pairs)} in class (tests/test_step_args_sweep.py says which of these are allowed)')
    calls, gold = wrapper_calls(), json.load(open(WRAPPERS))['calls']
    print(f'wrapper calls: {len(calls)}, {sum(calls[k] != gold.get(k) for k in calls) + len(set(gold) - set(calls))} differ from the golden file')


if __name__ == '__main__':
    main()
