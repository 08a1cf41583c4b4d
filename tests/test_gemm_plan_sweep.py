'''fd_gemm_f16's host path -- argument checks, tile / split-K rule, the checks behind the rule -- pinned WITHOUT a device against a reference
build: tests/golden/make_gemm_plan_sweep.py asks fd_gemm_plan and fd_gemm_gn_parts_chunks over ~70 000 descriptors under the default setting
and every seventh of them under each FD_GEMM_* / FD_CONV_TAPFAST switch (one child process per setting), and the return codes, tiles, splits
and refusal texts must hash, block by block, to what the committed golden file holds (tests/golden/gemm_plan_sweep.json, recorded from the
library of the commit it names -- the one before the host path was split into check, rule and launch).  A block that differs prints its rows;
`python tests/golden/make_gemm_plan_sweep.py --rows SETTING BLOCK` against a build of that commit (FD_LIB_PATH) prints what they were.
The one intended difference: residual_rows together with gn_out, which that build accepted and computed wrongly, is refused.'''
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)


@pytest.fixture(scope='module')
def sweep():
    import make_gemm_plan_sweep as m
    return m, m.sweep_all(), json.load(open(m.GOLDEN))['settings']


def test_every_setting_answers_what_the_reference_build_answered(sweep):
    m, res, gold = sweep
    assert list(res) == [m.setting_name(e) for e in m.settings()] and set(gold) == set(res)
    for name, r in res.items():
        g = gold[name]
        assert r['rows'] == g['rows'] and len(r['blocks']) == len(g['blocks'])
        bad = [i for i, (a, b) in enumerate(zip(r['blocks'], g['blocks'])) if a != b]
        if bad:
            env = {} if name == 'default' else dict(kv.split('=') for kv in name.split(','))
            listing = m.run_child(env, bad[:2])['listing']
            pytest.fail(f'{name}: blocks {bad} differ from the golden file; the rows of {bad[:2]} now:\n' + '\n'.join(listing))
        assert (r['auto'], r['forced'], r['messages'], r['helpers']) == (g['auto'], g['forced'], g['messages'], g['helpers']), name


def test_the_golden_sweep_reaches_every_check_tile_and_split(sweep):
    '''from the golden file's own histograms and texts: every check's message, every (tile, split) of the rule table among the unforced
    rows, every tile id among the accepted forced rows, half of the default rows accepted, >= 50 000 rows and >= 5 000 under each switch'''
    m, res, gold = sweep
    m.conditions(gold)
    m.conditions(res)


def test_residual_rows_with_gn_out_is_refused(sweep):
    '''k_splitk_finish_gn adds residual row m without the wrap k_splitk_finish has: it would read past a residual of residual_rows rows'''
    m, res, gold = sweep
    for name, r in res.items():
        assert len(r['res_rows_gn_out']) >= 12
        for rc, msg in r['res_rows_gn_out']:
            assert int(rc) == m.FD_EINVAL and 'residual_rows' in msg and 'gn_out' in msg, (name, rc, msg)
    # ... which the reference build accepted
    assert all(int(rc) == 0 for rc, _ in gold['default']['res_rows_gn_out'])
