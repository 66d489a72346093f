"""The engine's routing, characterised: for a grid of small jobs (nets with max / average / mixed pools and a conv no fast kernel
takes, every precision and conv algorithm, even and odd sizes, three weight tables, objective evaluations, an iteration and the ranged
hooks, every per-call switch) the profiler must report exactly the launches, FLOPs and bytes per kernel class that
tests/golden/route_fingerprints.json records -- figures taken on the commit named in that file by
tests/golden/make_route_fingerprints.py, which also defines the cases run here.  The byte formulas distinguish unpooling launches,
mask sources, fused style chunks and skipped outputs, so equal figures mean equal routes.

The figures are sums of integers and of multiples of 1/8 far below 2^53: exact equality, no tolerance.  The fixture keeps one digest
per case over all its figures (the figures of 1053 cases are half a megabyte); a failing case prints what the tree gave, and the
generator's --figures option writes the recorded commit's figures to compare with.
The whole file takes about 6 s on an MI355X."""

import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _generator():
    spec = importlib.util.spec_from_file_location('make_route_fingerprints', os.path.join(GOLDEN, 'make_route_fingerprints.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _generator()
COMMIT, RECORDED = gen.read_fixture()


def test_every_recorded_case_belongs_to_a_group_that_is_run():
    prefixes = {'%s/%s-algo%d/' % g for g in gen.GROUPS}
    assert len(COMMIT) == 40
    assert RECORDED and all(any(k.startswith(p) for p in prefixes) for k in RECORDED)


@pytest.mark.parametrize('net,precision,algo', gen.GROUPS)
def test_routes_are_those_of_the_recorded_commit(net, precision, algo):
    prefix = '%s/%s-algo%d/' % (net, precision, algo)
    want = {k: v for k, v in RECORDED.items() if k.startswith(prefix)}
    got = gen.run_group(net, precision, algo)
    assert sorted(got) == sorted(want)          # no case left out, none added
    wrong = sorted(k for k in want if gen.digest(got[k]) != want[k])
    for k in wrong[:5]:
        print(k, got[k])
    assert not wrong, '%d of %d cases differ from commit %s in a launch count, FLOP or byte figure (first ones printed above)' % (
        len(wrong), len(want), COMMIT[:12])
