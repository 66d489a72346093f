"""CPU side of the Laplacian term's plumbing: the text form of the levels, the worker's config key (a malformed value fails at start with
the key named), params['laplacian'] in StyleTransfer.set_weights, the trace names, and the refusals of the tile-sharded paths
(jobs.run_tiled_job, tools/stylize.py --laplacian with --grid).  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from style_transfer2_amd import jobs
from style_transfer2_amd.laplacian import check_levels, parse_levels
from style_transfer2_amd.transfer import StyleTransfer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD = ('4', '4:', ':1', '4:x', 'x:1', '3:1', '64:1', '4:0', '4:nan', '4:inf', '4:1,4:2', '1:1,2:1,4:1,8:1', '4:1;16:1', '4:1,', '4.0:1')


def test_text_form_of_the_levels():
    assert parse_levels('4:100,16:100') == [(4, 100.0), (16, 100.0)]
    assert parse_levels(' 4 : 1.5 , 16:-2 ') == [(4, 1.5), (16, -2.0)]
    assert parse_levels('32:1e-3') == [(32, 1e-3)]
    assert parse_levels('') == parse_levels('0') == parse_levels('off') == []
    for bad in BAD:
        with pytest.raises(ValueError):
            parse_levels(bad)
    assert check_levels([(1, 1), (2, 2), (32, -3)]) == [(1, 1.0), (2, 2.0), (32, -3.0)]


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_laplacian(self, levels):
        self.calls.append(list(levels or []))

    def set_weights(self, *args):
        pass


class _FakeTransfer:
    is_running = False

    def __init__(self):
        self.engine = _FakeEngine()
        self.model = self

    def layers(self):
        return ['data']


class _Socks:
    def __init__(self):
        self.sent = []

    def send_pyobj(self, obj):
        self.sent.append(obj)


def test_worker_reads_the_key_and_a_malformed_value_fails_at_start_with_the_key_named():
    sys.path.insert(0, ROOT)
    import worker
    assert worker.read_laplacian({'gpu': '0'}) is None and worker.read_laplacian({'laplacian': ' '}) is None      # absent: no call is made
    assert worker.read_laplacian({'laplacian': '4:100,16:100'}) == [(4, 100.0), (16, 100.0)]
    assert worker.read_laplacian({'laplacian': 'off'}) == []
    for bad in BAD:
        with pytest.raises(ValueError, match='config key laplacian'):
            worker.read_laplacian({'laplacian': bad})
    for config, calls in (({'async_iterate': '0'}, []), ({'async_iterate': '0', 'laplacian': '4:1.5,16:-2'}, [[(4, 1.5), (16, -2.0)]]),
                          ({'async_iterate': '0', 'laplacian': '0'}, [[]])):
        tr, socks = _FakeTransfer(), _Socks()
        worker.Worker(config, sock_in=socks, sock_out=socks, transfer=tr)
        assert tr.engine.calls == calls and [type(m).__name__ for m in socks.sent] == ['WorkerReady']
    tr, socks = _FakeTransfer(), _Socks()
    with pytest.raises(ValueError, match='config key laplacian'):
        worker.Worker({'async_iterate': '0', 'laplacian': '4:1,4:2'}, sock_in=socks, sock_out=socks, transfer=tr)
    assert tr.engine.calls == [] and socks.sent == []


class _Model:
    def __init__(self):
        self.engine = _FakeEngine()

    def layers(self):
        return ['data', 'conv1_1']


def test_set_weights_honours_the_optional_key_and_the_trace_names_the_two_scalars():
    st = StyleTransfer(_Model())
    weights = {'content': {'conv1_1': 1}, 'style': {}, 'deepdream': {}}
    params = {'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2}
    st.set_weights(weights, params)
    assert st.engine.calls == []                                          # without the key the setting is left alone
    st.set_weights(weights, dict(params, laplacian=[(4, 1.5)]))
    st.set_weights(weights, dict(params, laplacian=[]))
    st.set_laplacian([(16, 2.0)])
    assert st.engine.calls == [[(4, 1.5)], [], [(16, 2.0)]]
    values = np.arange(6 + 10, dtype=np.float64)                          # one active layer, the term on
    keys = list(st._make_trace(values, True).data)
    assert keys == ['conv1_1_c_loss', 'conv1_1_c_grad', 'scd_loss', 't_loss', 'p_loss', 'l_loss', 'scd_grad', 't_grad', 'p_grad', 'l_grad',
                    'time', 'loss', 'grad']
    t = st._make_trace(values, True).data
    assert (t['p_loss'], t['l_loss'], t['scd_grad'], t['p_grad'], t['l_grad'], t['loss'], t['grad']) == (8, 9, 10, 12, 13, 14, 15)
    assert list(st._make_trace(values, False).data) == ['conv1_1_c_loss', 'conv1_1_c_grad', 'scd_loss', 't_loss', 'p_loss', 'l_loss', 'loss']
    plain = list(st._make_trace(values[:14], True).data)                  # the term off: the keys of before
    assert plain == [k for k in keys if k not in ('l_loss', 'l_grad')]


def test_tile_sharded_jobs_refuse_the_term_before_anything_is_built():
    img = np.zeros((32, 32, 3), np.uint8)
    with pytest.raises(ValueError, match='tile-sharded'):
        jobs.run_tiled_job({}, img, img, 1, (1, 2), laplacian=[(4, 1.0)])
    with pytest.raises(ValueError, match='tile-sharded'):
        jobs.run_tiled_job({}, img, img, 1, (1, 2), params={'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2, 'laplacian': [(4, 1.0)]})
    import inspect
    assert inspect.signature(jobs.run_job).parameters['laplacian'].default is None


def _stylize():
    spec = importlib.util.spec_from_file_location('stylize_tool', os.path.join(ROOT, 'tools', 'stylize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_refuses_the_term_with_a_grid_and_a_malformed_value(capsys):
    tool = _stylize()
    assert tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png', '--laplacian', '4:100,16:100']).laplacian == '4:100,16:100'
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--laplacian', '4:100', '--grid', '1x2'])
    assert e.value.code == 2 and '--laplacian with --grid' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--laplacian', '3:100'])
    assert e.value.code == 2 and '--laplacian 3:100' in capsys.readouterr().err
