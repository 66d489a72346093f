"""CPU side of the frame sequences' plumbing: run_frames' refusals of malformed flows, maps and long-term tables before the transfer is
touched, run_job's mutual exclusions and the calls it makes for init_frame / anchor_frames, the calls run_frames makes on a recording
transfer, StyleTransfer.anchor_from_frame, and tools/stylize_frames.py's --forward-flows / --long-term with their side files.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from style_transfer2_amd import jobs
from style_transfer2_amd.transfer import StyleTransfer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
H, W = 24, 32
FRAME = np.zeros((H, W, 3), np.uint8)
FLOW, MAP = np.zeros((H, W, 2), F32), np.ones((H, W), F32)


class Untouched:
    def __getattr__(self, name):
        raise AssertionError('the transfer was touched (%s) before the refusal' % name)


def seq(n, value, first=1):
    return [None] * first + [value] * (n - first)


@pytest.mark.parametrize('kwargs,match', [
    (dict(forward_flows=[None]), 'forward_flows: one entry per frame'),
    (dict(flows=seq(3, FLOW), forward_flows=seq(3, FLOW[:, :-1])), r'forward_flows\[1\]'),
    (dict(flows=seq(3, FLOW[:-1])), r'flows\[1\]'),
    (dict(flows=seq(3, np.zeros((H, W, 3), F32))), r'flows\[1\]'),
    (dict(masks=seq(3, MAP[:, :-1])), r'masks\[1\]'),
    (dict(forward_flows=seq(3, FLOW)), r'forward_flows\[1\] without flows\[1\]'),
    (dict(flows=[None, None, FLOW], forward_flows=seq(3, FLOW)), r'forward_flows\[1\] without flows\[1\]'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={1: (seq(3, FLOW), None)}), 'integers from 2 to 8'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={9: (seq(3, FLOW), None)}), 'integers from 2 to 8'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={'2': (seq(3, FLOW), None)}), 'integers from 2 to 8'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2.0: (seq(3, FLOW), None)}), 'integers from 2 to 8'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={True: (seq(3, FLOW), None)}), 'integers from 2 to 8'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: seq(3, FLOW)}), r'long_term\[2\]: a \(flows, forward_flows or None\) pair'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: (None, None)}), r'long_term\[2\]: a \(flows'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: (seq(2, FLOW), None)}), r'long_term\[2\] flows: one entry per frame'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: (seq(3, FLOW), seq(4, FLOW))}), r'long_term\[2\] forward_flows: one entry per frame'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: (seq(3, FLOW[:-1]), None)}), r'long_term\[2\] flows\[2\]'),
    (dict(flows=seq(3, FLOW), masks=seq(3, MAP), long_term={2: ([None] * 3, seq(3, FLOW))}), r'long_term\[2\] forward_flows\[2\] without its flows\[2\]'),
    (dict(flows=seq(3, FLOW), long_term={2: (seq(3, FLOW), None)}), 'long_term at frame 2 needs a map of frame 1'),
    (dict(flows=seq(3, FLOW), masks=[None, MAP, None], long_term={2: (seq(3, FLOW), None)}), 'long_term at frame 2 needs a map'),
], ids=lambda v: None)
def test_run_frames_refuses_what_is_malformed_before_the_transfer_is_touched(kwargs, match):
    with pytest.raises(ValueError, match=match):
        jobs.run_frames(Untouched(), [FRAME] * 3, FRAME, 2, 10.0, **kwargs)


class Recorder:
    """A transfer that records the calls made on it and on its engine, in order."""
    def __init__(self):
        self.calls = []
        self.engine = self
        self.optimizer_cls = None

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


def test_run_job_refuses_two_ways_to_start_and_two_ways_to_anchor():
    with pytest.raises(ValueError, match='init_frame and init_nchw'):
        jobs.run_job(Untouched(), FRAME, FRAME, 1, init_frame=(1, None), init_nchw=np.zeros((3, H, W), F32))
    with pytest.raises(ValueError, match='anchor_frames and anchor'):
        jobs.run_job(Untouched(), FRAME, FRAME, 1, anchor_frames=(1.0, [(1, None, None, None)]), anchor=False)
    with pytest.raises(ValueError, match='anchor_frames and anchor'):
        jobs.run_job(Untouched(), FRAME, FRAME, 1, anchor_frames=(1.0, [(1, None, None, None)]), anchor=(FRAME, None, 1.0))
    with pytest.raises(ValueError, match='at least one'):
        jobs.run_job(Untouched(), FRAME, FRAME, 1, anchor_frames=(1.0, []))


def test_run_job_applies_the_frame_where_it_applies_the_planes_and_the_anchor_where_it_applies_the_anchor():
    rec = Recorder()
    fwd = FLOW + 1
    jobs.run_job(rec, FRAME, FRAME, 1, init_frame=(1, FLOW), anchor_frames=(40.0, [(1, FLOW, fwd, MAP), (2, FLOW, None, None), (4, None, fwd, None)]))
    names = rec.names()
    assert names.index('set_input') < names.index('set_input_from_frame') < names.index('set_content')
    assert 'set_input_nchw' not in names and 'set_anchor' not in names
    kind, args, kwargs = rec.calls[names.index('set_input_from_frame')]
    assert args[0] == 1 and args[1] is FLOW
    init = rec.calls[names.index('set_input')][1][0]
    assert init.shape == (H, W, 3) and init.dtype == np.uint8 and not init.any()
    anchors = [(args, kwargs) for name, args, kwargs in rec.calls if name == 'anchor_from_frame']
    assert [a[0] for a, _ in anchors] == [1, 2, 4] and [k['accumulate'] for _, k in anchors] == [False, True, True]
    assert all(a[4] == 40.0 for a, _ in anchors) and anchors[0][0][2] is fwd and anchors[0][0][3] is MAP and anchors[2][0][1] is None
    assert max(i for i, n in enumerate(names) if n == 'anchor_from_frame') < names.index('start')


def test_run_frames_keeps_pushes_and_never_reads_the_iterate_back():
    rec = Recorder()
    n = 5
    flows, fwds, masks = seq(n, FLOW), seq(n, FLOW + 1), [None, MAP, None, MAP, MAP]
    b2, f2, b4 = [None, None, FLOW + 2, None, FLOW + 2], [None, None, FLOW + 3, None, None], seq(n, FLOW + 4)
    out = jobs.run_frames(rec, [FRAME] * n, FRAME, 2, 40.0, flows=flows, masks=masks, forward_flows=fwds, long_term={4: (b4, None), 2: (b2, f2)},
                          first_iterations=3)
    assert len(out) == n
    names = rec.names()
    assert names[0] == 'frames_keep' and rec.calls[0][1] == (4,) and names.count('frames_keep') == 1
    assert names.count('frame_push') == n and names[-1] == 'frame_push'
    for banned in ('get_input_nchw', 'set_input_nchw', 'set_anchor_nchw'):
        assert banned not in names
    assert [args for name, args, _ in rec.calls if name == 'set_anchor'] == [(None,)]          # frame 0 turns the term off
    assert names.count('step') + names.count('step_async') == 3 + 2 * (n - 1)
    inits = [args for name, args, _ in rec.calls if name == 'set_input_from_frame']
    assert len(inits) == n - 1 and all(a[0] == 1 and a[1] is FLOW for a in inits)
    # per frame: j = 1 sets, then the older frames in ascending order where t >= j and a flow is given
    per_frame, cur = [], None
    for name, args, kwargs in rec.calls:
        if name == 'frame_push':
            per_frame.append(cur or []); cur = None
        elif name == 'anchor_from_frame':
            cur = (cur or []) + [(args[0], kwargs['accumulate'])]
    assert per_frame == [[], [(1, False)], [(1, False), (2, True)], [(1, False)], [(1, False), (2, True), (4, True)]]
    last = [(args, kwargs) for name, args, kwargs in rec.calls if name == 'anchor_from_frame'][-3:]
    assert last[0][0][3] is MAP and last[1][0][3] is None and last[1][0][2] is None and last[2][0][1] is b4[4]
    # entry 0 of every sequence, and the entries of a long-term table before frame j, are not read: they may be anything
    rec = Recorder()
    jobs.run_frames(rec, [FRAME] * 3, FRAME, 1, 40.0, flows=['x', FLOW, FLOW], masks=[0, MAP, MAP], forward_flows=[(), None, None],
                    long_term={2: (['x', 'y', FLOW], ['x', 'y', None])})
    assert rec.names().count('anchor_from_frame') == 3
    # without long-term frames one frame is kept
    rec = Recorder()
    jobs.run_frames(rec, [FRAME] * 2, FRAME, 1, 40.0)
    assert rec.calls[0][:2] == ('frames_keep', (1,))
    args, kwargs = [(a, k) for name, a, k in rec.calls if name == 'anchor_from_frame'][0]
    assert args[:4] == (1, None, None, None) and kwargs == {'accumulate': False}


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def anchor_from_frame(self, *args):
        self.calls.append(args)

    def set_weights(self, *args):
        pass


class _Model:
    def __init__(self):
        self.engine = _FakeEngine()

    def layers(self):
        return ['data', 'conv1_1']


def test_the_transfer_names_the_trace_of_an_anchor_made_from_a_frame():
    st = StyleTransfer(_Model())
    st.set_weights({'content': {'conv1_1': 1}, 'style': {}, 'deepdream': {}}, {'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2})
    v10 = np.arange(6 + 10, dtype=np.float64)
    assert 'l_loss' in st._make_trace(v10, True).data
    st.anchor_from_frame(2, FLOW, None, MAP, 3.0, accumulate=True)
    assert st.engine.calls == [(2, FLOW, None, MAP, 3.0, True)]
    t = st._make_trace(v10, True).data
    assert 'a_loss' in t and 'a_grad' in t and 'l_loss' not in t


def _tool():
    spec = importlib.util.spec_from_file_location('stylize_frames_tool', os.path.join(ROOT, 'tools', 'stylize_frames.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_frames_tool_parses_the_new_flags_and_finds_the_side_files(tmp_path, capsys):
    tool = _tool()
    base = ['a.png', 'b.png', '--style', 's.jpg', '--out-dir', 'out']
    args = tool.parser().parse_args(base + ['--flows', 'f', '--forward-flows', 'g', '--long-term', '4,2'])
    assert (args.flows, args.forward_flows, args.long_term) == ('f', 'g', [2, 4])
    assert tool.parser().parse_args(base).long_term == [] and tool.parser().parse_args(base).forward_flows == ''
    for bad in ('1', '9', '2,2', 'x', '', '2;4'):
        with pytest.raises(SystemExit):
            tool.parser().parse_args(base + ['--long-term', bad])
        assert '--long-term' in capsys.readouterr().err
    flows, fwd = tmp_path / 'flows', tmp_path / 'fwd'
    flows.mkdir(); fwd.mkdir()
    stems = ['f0', 'f1', 'f2', 'f3', 'f4']
    for name in ('f2.b2.npy', 'f4.b2.npy', 'f4.b4.npy', 'f1.b2.npy'):       # (f1.b2: before the 2nd frame, never read)
        (flows / name).write_bytes(b'')
    for name in ('f2.f2.npy', 'f3.f2.npy'):                                 # (f3.f2: no backward flow beside it, not used)
        (fwd / name).write_bytes(b'')
    got = tool.long_term_files(str(flows), str(fwd), stems, [2, 4])
    assert got == {2: ([None, None, str(flows / 'f2.b2.npy'), None, str(flows / 'f4.b2.npy')], [None, None, str(fwd / 'f2.f2.npy'), None, None]),
                   4: ([None, None, None, None, str(flows / 'f4.b4.npy')], [None] * 5)}
    assert tool.long_term_files(str(flows), '', stems, [4])[4][1] is None
    # what cannot work is refused before anything is loaded
    for argv, text in ((base + ['--forward-flows', 'g'], '--forward-flows needs --flows'),
                       (base + ['--flows', 'f', '--long-term', '2'], '--long-term needs --flows')):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err
