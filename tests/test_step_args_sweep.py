'''The host path of the fifteen latent-step entry points, pinned WITHOUT a device against a reference build:
tests/golden/make_step_args_sweep.py calls every entry point of csrc/step.hip, composite.hip and window.hip on host addresses
-- a few valid base calls each, every single mutation of one, every pair of two -- and reads "refused, by which check" (FD_EINVAL
and the message's class) or "accepted, handed to which kernel family" (FD_EHIP, "<family>: launch failed") off the answer.  The
answers must be what tests/golden/step_args_sweep.json holds, recorded from the library of the commit it names (the one before the
fronts were given one checker):
  single mutations   return code, class and the entry point's name in the message equal the golden
  pairs              the return code equals the golden; a refused pair reports the class of one of its two single mutations (which
                     of two simultaneous violations comes first is not part of the contract; `pair_classes`)
The intended differences, and nothing else:
  (a) fd_cfg_ddim_step_f32 and fd_composite_step_f32 said "args" for every problem: that class may become null or sizes;
  (b) a row the reference accepted may be refused (alias) where its launch had one buffer written by some threads while others
      read it: `NEWLY_REFUSED` of the recorder names the single mutations (fd_window_step_f32's windows_out on eps_nhwc: the next
      window batch written over the rows other threads still read); a pair is covered when it holds one of them.
No row the reference refused is accepted.  The accepted rows are calls that would launch, so they are replayed only where no
device is seen; with a device the refused rows alone are compared.
The wrappers: every `ops.*_step` on CPU tensors over its options with `hip.call` recorded must reproduce
tests/golden/step_wrapper_calls.json (same recorder, same commit) exactly.'''
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
ARGS_TO = {'null', 'sizes'}                    # (a): what the class "args" may have become


@pytest.fixture(scope='module')
def sweep():
    import make_step_args_sweep as m
    gold = json.load(open(m.GOLDEN))
    return m, m.sweep(None if m.no_device() else gold['entries']), gold


def _same_class(gold_cls, cls):
    return cls == gold_cls or (gold_cls == 'args' and cls in ARGS_TO)


def test_golden_file_reaches_every_check_and_kernel_family(sweep):
    m, _, gold = sweep
    assert set(gold['entries']) == set(m.ENTRIES) and gold['classes'] == list(m.CLASSES)
    assert gold['newly_refused'] == {k: sorted(v) for k, v in m.NEWLY_REFUSED.items()}
    m.conditions(gold['entries'])


def test_every_row_answers_what_the_reference_build_answered(sweep):
    m, res, gold = sweep
    bad, replayed = [], 0
    for entry in m.ENTRIES:
        allowed = m.NEWLY_REFUSED.get(entry, set())
        for (bname, base), (_, singles, got), (gname, gsingles, want) in zip(m.bases(entry), m.decoded(res[entry]),
                                                                              m.decoded(gold['entries'][entry])):
            _, names, _ = m.rows(entry, base)
            assert (bname, singles, len(names)) == (gname, gsingles, len(want)) == (gname, gsingles, len(got)), (entry, bname)
            single = {}
            for i, (name, g, w) in enumerate(zip(names, got, want)):
                parts = name.split(' & ')
                replayed += 1
                if i < singles:
                    single[name] = (w[1], g[1])
                    ok = g[0] == w[0] and g[2] == w[2] and _same_class(w[1], g[1]) and (g[0] != m.FD_EINVAL or g[3].startswith(entry + ': '))
                else:
                    ok = g[0] == w[0] and g[2] == w[2] and (g[0] != m.FD_EINVAL or any(
                        _same_class(c, g[1]) for c in m.pair_classes(single[parts[0]][0], single[parts[1]][0], parts)))
                if not ok and w[1] == 'accepted' and set(parts) & allowed:            # (b)
                    ok = g[0] == m.FD_EINVAL and g[1] == 'alias'
                if not ok:
                    bad.append(f'{entry} [{bname}] {name}: the reference said {w}, the tree says {g}')
    assert not bad, f'{len(bad)} of {replayed} rows differ:\n' + '\n'.join(bad[:40])
    if not m.no_device():
        pytest.skip('a device is present: the rows the reference accepted would launch on host addresses; the refused rows agree')


def test_wrappers_hand_the_library_what_the_reference_wrappers_handed_it():
    import make_step_args_sweep as m
    gold = json.load(open(m.WRAPPERS))['calls']
    calls = m.wrapper_calls()
    assert set(calls) == set(gold)
    bad = [f'{k}: the reference {gold[k]}, the tree {calls[k]}' for k in calls if calls[k] != gold[k]]
    assert not bad, '\n'.join(bad[:20])
