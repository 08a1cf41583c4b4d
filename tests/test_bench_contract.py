'''The bench line contract (driver + judge read these fields) checked on the newest committed full line profiles/rNN_bench.json -- the output
of the full default `python bench.py` on an MI355X --, on bench.py's argument defaults and on the source-binding of the PMC traffic record.
CPU only; the live line is checked by tests/test_gpu_dist.py with the same checker (tests/bench_contract.py).'''
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    '''The newest committed full default line (profiles/rNN_bench.json).  The same checker runs on a LIVE line in
    tests/test_gpu_dist.py::test_live_mini_bench_line_meets_the_contract.'''
    import glob
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_contract import check_bench_line
    paths = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_bench.json')))
    assert paths, 'no committed bench line under profiles/'
    with open(paths[-1]) as f:
        d = json.loads(f.read().strip().splitlines()[-1])
    check_bench_line(d, full=True)


def test_traffic_record_is_tied_to_the_sources():
    '''bench.py reports `roofline.traffic` from the newest profiles/r*_pmc_traffic.json whose `sources_sha` equals the sha256 of
    today's GEMM sources, and says `traffic_stale: true` otherwise.'''
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ['bench.py']
    try:
        import bench
    finally:
        sys.argv = argv
    sha = bench.sources_sha()
    assert len(sha) == 64 and sha == bench.sources_sha()
    traffic, of, other, stale = bench.pick_traffic_record()
    assert traffic and traffic > 50e6 and isinstance(stale, bool) and ('stale' in of) == stale
    import glob
    matching = [p for p in glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_traffic.json')) if json.load(open(p)).get('sources_sha') == sha]
    assert stale == (not matching)


def test_roofline_aggregation_survives_a_host_stall():
    '''bench.aggregate_brackets: median per launch shape x count.  Round 5's driver line carried a 39 ms host stall inside ONE
    GroupNorm bracket (x the sampling stride = 273 ms of "GroupNorm"); here the same stall moves nothing, and time_budget sums
    to the step.'''
    import numpy as np
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ['bench.py']
    try:
        import bench
    finally:
        sys.argv = argv
    rng = np.random.default_rng(0)
    fam, tag, ms, work = [], [], [], []
    shapes = [(0, 11, 0.100, 1e11), (0, 12, 0.030, 2e10), (1, 21, 0.380, 3e11), (2, 31, 0.029, 4e8), (2, 32, 0.008, 1e7), (3, 41, 0.004, 0.0)]
    for f, t, dur, w in shapes:
        for _ in range(200):
            fam.append(f), tag.append(t), ms.append(dur * (1 + 0.01 * rng.standard_normal()) + 0.005), work.append(w)
    clean = bench.aggregate_brackets(fam, tag, ms, work, work, 0.005)
    i = fam.index(2)
    ms[i] += 39.0                                    # the stall
    hit = bench.aggregate_brackets(fam, tag, ms, work, work, 0.005)
    assert abs(hit['groupnorm']['ms'] - clean['groupnorm']['ms']) < 0.01 * clean['groupnorm']['ms']
    assert hit['groupnorm']['raw_ms'] > clean['groupnorm']['raw_ms'] + 38.0
    assert hit['groupnorm']['worst_bracket_over_median'] > 100 and clean['groupnorm']['worst_bracket_over_median'] < 1.2
    assert abs(clean['gemm']['ms'] - 200 * (0.100 + 0.030)) < 0.3 and clean['gemm']['groups'] == 2 and clean['gemm']['launches'] == 400
    assert abs(clean['gemm']['work'] - 200 * 1.2e11) < 1.0
    step = 140.0
    budget, ok = bench.time_budget(hit, step)
    assert ok and abs(sum(budget.values()) - step) < 1e-9 and budget['gaps_and_host'] > 0
    assert not bench.time_budget(hit, 50.0)[1]
    # with a sampling stride every sampled bracket stands for `stride` launches
    s7 = bench.aggregate_brackets(fam[::7], tag[::7], ms[::7], work[::7], work[::7], 0.005, stride=7)
    assert abs(s7['attention']['ms'] - clean['attention']['ms']) < 0.05 * clean['attention']['ms']


def test_bench_defaults_finish_in_minutes_and_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, timeout=120)
    assert r.returncode == 0
    text = r.stdout.decode()
    for flag in ('--gpus', '--steps', '--warmup', '--launch', '--scheduler', '--img2img', '--guidance', '--preset', '--full',
                 '--dump-outputs'):
        assert flag in text, flag
    # importing bench must not import torch (the N-rank parent stays GPU-free); defaults: N = 1, 8 timed / 2 warm-up passes
    code = ('import sys; sys.argv = ["bench.py"]; sys.path.insert(0, %r); import bench, argparse; '
            'assert "torch" not in sys.modules; print("ok")' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, timeout=120)
    assert r.returncode == 0 and b'ok' in r.stdout, r.stderr.decode()[-500:]


def test_dump_outputs_stays_within_its_size_limit():
    '''bench.dump_outputs: float32 .npy per array; above the limit every array becomes a fixed, seeded sample of its elements.'''
    import numpy as np
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ['bench.py']
    try:
        import bench
    finally:
        sys.argv = argv
    import tempfile
    rng = np.random.default_rng(0)
    arrays = {'latents': rng.standard_normal((4, 4, 8, 8)), 'images': rng.random((4, 64, 64, 3))}
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, arrays)
        for name, a in arrays.items():
            got = np.load(os.path.join(d, name + '.npy'))
            assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
        limit = 16 << 10
        bench.dump_outputs(os.path.join(d, 's1'), arrays, limit=limit)
        bench.dump_outputs(os.path.join(d, 's2'), arrays, limit=limit)
        total = 0
        for name, a in arrays.items():
            s1, s2 = (np.load(os.path.join(d, s, name + '.npy')) for s in ('s1', 's2'))
            assert s1.dtype == np.float32 and s1.ndim == 1 and np.array_equal(s1, s2)
            assert np.isin(s1, a.astype(np.float32).reshape(-1)).all()
            total += s1.nbytes
        assert 0.9 * limit < total <= limit
