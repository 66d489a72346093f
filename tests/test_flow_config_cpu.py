"""CPU side of the optical-flow plumbing: flow.py's parsing and refusals, estimate_flows / fill_flows / run_frames(estimate=...) on a stub
engine (which flows are estimated, from which frames, and that run_frames(estimate=None) calls nothing new), and the argument rules of
tools/stylize_frames.py --estimate-flow with its side files.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import flow_oracle as fo
from style_transfer2_amd import flow, jobs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
H, W = 24, 32


# ------------------------------------------------------------------------------------------ flow.py
def test_defaults_and_checks():
    assert flow.DEFAULTS == {'alpha': 0.06, 'warps': 3, 'iters': 40, 'levels': 0, 'route': 0}
    assert flow.check_flow() == flow.DEFAULTS and flow.check_flow() is not flow.DEFAULTS
    assert flow.check_flow(alpha=0.03, iters=1, warps=16, levels=12, route=1) == {'alpha': 0.03, 'warps': 16, 'iters': 1, 'levels': 12, 'route': 1}
    assert flow.check_flow(alpha=None, iters=np.int64(7)) == dict(flow.DEFAULTS, iters=7)          # None: the default
    assert flow.check_flow(alpha=1e-6)['alpha'] == 1e-6 and flow.check_flow(alpha=1000)['alpha'] == 1000.0
    for bad in (dict(levels=-1), dict(levels=13), dict(warps=0), dict(warps=17), dict(iters=0), dict(iters=1001), dict(route=2), dict(route=-1),
                dict(alpha=0), dict(alpha=9e-7), dict(alpha=1000.5), dict(alpha=float('nan')), dict(alpha=float('inf')), dict(alpha=-0.06),
                dict(alpha='x'), dict(alpha=True), dict(iters=2.5), dict(iters='3'), dict(warps=True), dict(levels=None, iters=[1]), dict(beta=1)):
        with pytest.raises(ValueError):
            flow.check_flow(**bad)
    with pytest.raises(ValueError, match='unknown flow parameter.*beta'):
        flow.check_flow(beta=1)


def test_text_form():
    assert flow.parse_flow('') == flow.DEFAULTS and flow.parse_flow(' default ') == flow.DEFAULTS
    assert flow.parse_flow('alpha=0.03, iters=60') == dict(flow.DEFAULTS, alpha=0.03, iters=60)
    assert flow.parse_flow('levels=1,warps=2,route=1') == dict(flow.DEFAULTS, levels=1, warps=2, route=1)
    for bad in ('alpha', 'alpha=', '=3', 'iters=2.5', 'iters=x', 'alpha=0.03,alpha=0.04', 'iters=0', 'gamma=1', 'alpha=0.03;iters=2', 'alpha=nan'):
        with pytest.raises(ValueError):
            flow.parse_flow(bad)


def test_level_sizes_are_the_oracles():
    for h, w in ((1, 1), (5, 3), (31, 33), (32, 32), (33, 47), (63, 100), (64, 64), (65, 64), (96, 128), (130, 70), (1024, 1024), (1080, 1920)):
        for levels in (0, 1, 2, 12):
            assert flow.level_sizes(h, w, levels) == fo.level_sizes(h, w, levels)


# ------------------------------------------------------------------------------------------ jobs on a stub engine
class Recorder:
    """A transfer that is its own engine and records every call; flow_estimate returns a flow that names its two frames."""
    def __init__(self):
        self.calls = []
        self.engine = self
        self.optimizer_cls = None

    def flow_estimate(self, a, b, **params):
        self.calls.append(('flow_estimate', (int(a[0, 0, 0]), int(b[0, 0, 0])), params))
        return np.full((H, W, 2), 100 * int(a[0, 0, 0]) + int(b[0, 0, 0]), F32)

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            if name == 'start':
                return True
            if name == 'step':
                return np.zeros((H, W, 3), F32), {}
        return call

    def names(self):
        return [name for name, _, _ in self.calls]


def frames(n):
    return [np.full((H, W, 3), t, np.uint8) for t in range(n)]


def tag(f):
    return None if f is None else int(f[0, 0, 0])


def test_estimate_flows_pairs_the_frames_as_run_frames_reads_them():
    rec = Recorder()
    flows, fwd, lt = jobs.estimate_flows(rec, frames(4), long_term=(2,), iters=5)
    assert [tag(f) for f in flows] == [None, 100, 201, 302]            # from frame t, to frame t - 1
    assert [tag(f) for f in fwd] == [None, 1, 102, 203]                # from frame t - 1, to frame t
    assert sorted(lt) == [2]
    assert [tag(f) for f in lt[2][0]] == [None, None, 200, 301] and [tag(f) for f in lt[2][1]] == [None, None, 2, 103]
    assert all(name == 'flow_estimate' and params == {'iters': 5} for name, _, params in rec.calls) and len(rec.calls) == 10
    assert jobs.estimate_flows(Recorder(), frames(1)) == ([None], [None], {})
    for bad in ((1,), (9,), ('2',), (2.0,), (True,)):
        with pytest.raises(ValueError, match='integers from 2 to 8'):
            jobs.estimate_flows(Recorder(), frames(3), long_term=bad)
    with pytest.raises(ValueError, match='differ in size'):
        jobs.estimate_flows(Recorder(), frames(2) + [np.zeros((H, W + 1, 3), np.uint8)])


def test_run_frames_without_estimate_calls_nothing_new():
    rec = Recorder()
    jobs.run_frames(rec, frames(3), frames(1)[0], 2, 40.0)
    names = rec.names()
    assert 'flow_estimate' not in names and 'flow_release' not in names and 'flow_level' not in names
    # ... and the sequence of calls is the one the explicit None gives
    other = Recorder()
    jobs.run_frames(other, frames(3), frames(1)[0], 2, 40.0, estimate=None)
    assert other.names() == names
    inits = [args for name, args, _ in rec.calls if name == 'set_input_from_frame']
    assert all(a == (1, None) for a in inits)               # flows=None still means "no warp"


def test_run_frames_fills_in_what_is_not_given_and_what_is_given_wins():
    rec = Recorder()
    mine = np.full((H, W, 2), -7, F32)
    jobs.run_frames(rec, frames(4), frames(1)[0], 1, 40.0, flows=[None, None, mine, None], long_term={2: None}, estimate={'alpha': 0.1})
    names = rec.names()
    assert names.count('flow_estimate') == 10 and names.count('flow_release') == 1
    assert names.index('flow_release') < names.index('frames_keep')               # every estimate before the first job
    assert all(params == {'alpha': 0.1} for name, _, params in rec.calls if name == 'flow_estimate')
    inits = [tag(args[1]) for name, args, _ in rec.calls if name == 'set_input_from_frame']
    assert inits == [100, -7, 302]
    anchors = [(args[0], tag(args[1]), tag(args[2])) for name, args, _ in rec.calls if name == 'anchor_from_frame']
    assert anchors == [(1, 100, 1), (1, -7, 102), (2, 200, 2), (1, 302, 203), (2, 301, 103)]
    # the same flows given explicitly make the same calls on the job
    flows, fwd, lt = jobs.fill_flows(Recorder(), frames(4), [None, None, mine, None], None, (2,), alpha=0.1)
    other = Recorder()
    jobs.run_frames(other, frames(4), frames(1)[0], 1, 40.0, flows=flows, forward_flows=fwd, long_term=lt)
    strip = lambda calls: [(n, [tag(a) if isinstance(a, np.ndarray) and a.ndim == 3 and a.shape[2] == 2 else None for a in args])      # noqa: E731
                           for n, args, _ in calls if n not in ('flow_estimate', 'flow_release')]
    assert strip(other.calls) == strip(rec.calls)
    with pytest.raises(ValueError, match=r'long_term\[2\]'):
        jobs.run_frames(Recorder(), frames(3), frames(1)[0], 1, 40.0, long_term={2: [None]}, estimate={})


def test_product_code_imports_nothing_of_the_tests():
    for name in ('flow.py', 'jobs.py', 'engine.py'):
        imports = [line.strip() for line in open(os.path.join(ROOT, 'style_transfer2_amd', name)) if line.strip().startswith(('import ', 'from '))]
        assert imports and not [line for line in imports if 'oracle' in line or 'tests' in line]


# ------------------------------------------------------------------------------------------ tools/stylize_frames.py
def _tool():
    spec = importlib.util.spec_from_file_location('stylize_frames_tool', os.path.join(ROOT, 'tools', 'stylize_frames.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_frames_tool_argument_rules(capsys):
    tool = _tool()
    base = ['a.png', 'b.png', '--style', 's.jpg', '--out-dir', 'out']
    ap = tool.parser()
    args = ap.parse_args(base)
    assert (args.estimate_flow, args.flow_alpha, args.flow_iters, args.flow_warps, args.flow_levels, args.save_flows) == (False, None, None, None, None, '')
    assert tool.flow_params(ap, args) is None
    args = ap.parse_args(base + ['--estimate-flow', '--long-term', '2,4'])
    assert tool.flow_params(ap, args) == {}                 # frames alone are enough: no --flows, no map
    args = ap.parse_args(base + ['--estimate-flow', '--flow-alpha', '0.03', '--flow-iters', '60', '--flow-warps', '2', '--flow-levels', '4', '--save-flows', 'd'])
    assert tool.flow_params(ap, args) == {'alpha': 0.03, 'iters': 60, 'warps': 2, 'levels': 4} and args.save_flows == 'd'
    refused = [(['--flow-alpha', '0.03'], 'need --estimate-flow'), (['--flow-iters', '3'], 'need --estimate-flow'), (['--save-flows', 'd'], 'need --estimate-flow'),
               (['--flow-levels', '0'], 'need --estimate-flow'),
               (['--estimate-flow', '--flow-iters', '0'], 'iters 0 is outside'), (['--estimate-flow', '--flow-alpha', '0'], 'alpha'),
               (['--estimate-flow', '--flow-warps', '17'], 'warps 17 is outside'), (['--estimate-flow', '--flow-levels', '13'], 'levels 13 is outside'),
               (['--forward-flows', 'g'], '--forward-flows needs --flows'), (['--flows', 'f', '--long-term', '2'], '--long-term needs --flows')]
    for extra, text in refused:                             # before anything is loaded
        with pytest.raises(SystemExit) as e:
            tool.main(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    assert 'nothing here estimates' not in tool.__doc__ and '--estimate-flow' in tool.__doc__


def test_frames_tool_side_files(tmp_path):
    tool = _tool()
    assert tool.optional_file('', 'a.npy') is None and tool.optional_file(str(tmp_path), 'a.npy') is None
    (tmp_path / 'a.npy').write_bytes(b'')
    assert tool.optional_file(str(tmp_path), 'a.npy') == str(tmp_path / 'a.npy')
    f = lambda v: np.full((2, 3, 2), v, np.float64)         # noqa: E731
    out = tmp_path / 'saved'
    written = tool.save_flows(str(out), ['s0', 's1', 's2'], [None, f(1), f(2)], [None, f(3), f(4)], {2: ([None, None, f(5)], [None, None, f(6)])})
    assert sorted(os.path.basename(p) for p in written) == ['s1.fwd.npy', 's1.npy', 's2.b2.npy', 's2.f2.npy', 's2.fwd.npy', 's2.npy']
    got = {name: np.load(str(out / name)) for name in os.listdir(str(out))}
    assert all(a.dtype == F32 and a.shape == (2, 3, 2) for a in got.values())
    assert [int(got[n][0, 0, 0]) for n in ('s1.npy', 's2.npy', 's1.fwd.npy', 's2.fwd.npy', 's2.b2.npy', 's2.f2.npy')] == [1, 2, 3, 4, 5, 6]
    # the saved directory serves as --flows and as --forward-flows of a later run
    assert tool.side_file(str(out), 's1', ('.fwd.npy', '.npy')) == str(out / 's1.fwd.npy')
    assert tool.long_term_files(str(out), str(out), ['s0', 's1', 's2'], [2]) == {2: ([None, None, str(out / 's2.b2.npy')], [None, None, str(out / 's2.f2.npy')])}
