'''The library calls of FlexPipeline for every combination of guide, scheduler, eta, step noise, request, debug, loop mode and
fuse switch (tests/route_trace.py: `cases`), recorded on CPU tensors with the library replaced by a recorder -- host logic only,
runs without a device.  tests/test_route_traces.py replays every case against the file.
    python tests/golden/make_route_goldens.py            record and compare with the committed file
    python tests/golden/make_route_goldens.py --update   rewrite tests/golden/route_traces.json (after an INTENDED change of a
                                                         route; a refactor of the loop must leave the file as it is)
The file holds every distinct event, block (the events before the loop, of one step, after the loop) and trace (a request's
blocks) once, and for each outer case key the trace index of each inner key, in the order of `inner`.'''
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
TRACES = os.path.join(HERE, 'route_traces.json')


def _intern(table, index, item):
    k = json.dumps(item)
    if k not in index:
        index[k] = len(table)
        table.append(item)
    return index[k]


def record():
    import route_trace as R
    mp = pytest.MonkeyPatch()
    tabs = {n: ([], {}) for n in ('events', 'blocks', 'traces')}
    cases, count = {}, 0
    for outer, inner in R.cases():
        row = []
        for i in inner:
            blocks = json.loads(json.dumps(R.run_case(mp, outer, i)))
            ids = [_intern(*tabs['blocks'], [_intern(*tabs['events'], e) for e in b]) for b in blocks]
            row.append(_intern(*tabs['traces'], ids))
        cases[R.outer_key(outer)] = row
        count += len(row)
    full = [R.inner_key(i) for i in R.INNER]
    return {'steps': R.TRACE_STEPS, 'case_count': count, 'inner': full, 'cases': cases, 'traces': tabs['traces'][0],
            'blocks': tabs['blocks'][0], 'events': tabs['events'][0]}


def main():
    new = record()
    if '--update' in sys.argv:
        new['parent_commit'] = subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True).stdout.strip()
        with open(TRACES, 'w') as f:
            json.dump(new, f, separators=(',', ':'))
        print(f'wrote {TRACES}: {new["case_count"]} cases, {len(new["traces"])} traces, {len(new["blocks"])} blocks, '
              f'{len(new["events"])} events, {os.path.getsize(TRACES)} bytes')
        return
    old = json.load(open(TRACES))
    same = all(new[k] == old[k] for k in new)
    print(f'{new["case_count"]} cases, {len(new["traces"])} traces: ' + ('as committed' if same else 'DIFFERS from the committed file'))
    sys.exit(0 if same else 1)


if __name__ == '__main__':
    main()
