"""CPU side of the photorealism term's plumbing: the worker key ``matting``, the text form W[:EPS], jobs.run_job's argument, the refusals
of the tile-sharded paths (jobs.run_tiled_job, tools/stylize.py --matting with --grid), and the trace names for all eight on/off
combinations of the three optional image-space terms, which StyleTransfer._make_trace asks the engine about.  No GPU."""
import importlib.util
import inspect
import itertools
import os

import numpy as np
import pytest

import worker
from style_transfer2_amd import jobs, matting
from style_transfer2_amd.transfer import StyleTransfer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the text form and the worker key --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('text,want', [('10000', (10000.0, 1e-7)), ('10000:1e-7', (10000.0, 1e-7)), (' 1e4 : 1e-5 ', (1e4, 1e-5)), ('-2.5:1', (-2.5, 1.0)),
                                       ('50:1e-9', (50.0, 1e-9)), ('0', (0.0, 1e-7)), ('off', (0.0, 1e-7)), ('OFF', (0.0, 1e-7)), ('0.0:1e-3', (0.0, 1e-3))])
def test_good_values_of_the_key(text, want):
    assert matting.parse_matting(text) == want
    assert worker.read_matting({'matting': text}) == want


@pytest.mark.parametrize('text', ['abc', '1e4:', ':1e-7', '1e4:1e-7:3', 'nan', 'inf', '-inf', '1e60', '1e-60', '1e4:0', '1e4:1e-10', '1e4:1.5', '1e4:-1e-7',
                                  '1e4:nan', '1e4,1e-7'])
def test_bad_values_of_the_key_name_it(text):
    with pytest.raises(ValueError):
        matting.parse_matting(text)
    with pytest.raises(ValueError, match=r'config key matting = .*W or W:EPS'):
        worker.read_matting({'matting': text})


def test_an_absent_or_empty_key_makes_no_call():
    assert worker.read_matting({}) is None and worker.read_matting({'matting': ''}) is None and worker.read_matting({'matting': '  '}) is None


def test_the_argument_of_run_job():
    assert matting.matting_arg((30.0, 1e-5)) == (30.0, 1e-5) and matting.matting_arg([30, 1e-5]) == (30.0, 1e-5)
    assert matting.matting_arg(1e4) == (1e4, 1e-7) and matting.matting_arg(False) == (0.0, 1e-7) and matting.matting_arg(0) == (0.0, 1e-7)
    for bad in ((1.0,), (1.0, 1e-7, 3), (1.0, 2.0), float('nan'), 'x'):
        with pytest.raises(ValueError):
            matting.matting_arg(bad)
    assert inspect.signature(jobs.run_job).parameters['matting'].default is None

    class Untouched:
        def __getattr__(self, name):
            raise AssertionError('run_job touched the transfer (%s) before it refused' % name)
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match='eps'):
        jobs.run_job(Untouched(), img, img, 1, matting=(1.0, 5.0))


def test_tile_sharded_jobs_refuse_the_term_before_anything_is_built():
    img = np.zeros((32, 32, 3), np.uint8)
    for value in (1e4, (1e4, 1e-7)):
        with pytest.raises(ValueError, match='photorealism term does not run tile-sharded'):
            jobs.run_tiled_job({}, img, img, 1, (1, 2), matting=value)


# ---- the tools -------------------------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name + '_tool', os.path.join(ROOT, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_takes_the_switch_and_refuses_it_with_a_grid(capsys):
    tool = _tool('stylize')
    assert tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png', '--matting', '1e4:1e-6']).matting == '1e4:1e-6'
    assert tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png']).matting == ''
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--matting', '1e4', '--grid', '1x2'])
    assert e.value.code == 2 and '--matting with --grid' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--matting', '1e4:7'])
    assert e.value.code == 2 and '--matting 1e4:7' in capsys.readouterr().err


def test_frames_tool_takes_the_switch():
    tool = _tool('stylize_frames')
    args = tool.parser().parse_args(['a.png', 'b.png', '--style', 's.jpg', '--out-dir', 'out', '--matting', '500'])
    assert args.matting == '500'


# ---- trace names -----------------------------------------------------------------------------------------------------------------------
class _FakeEngine:
    """An engine that says which optional terms are on, as Engine.trace_terms does."""
    def __init__(self):
        self.terms = (False, False, False)
        self.calls = []

    def trace_terms(self):
        return self.terms

    def set_matting(self, weight, eps):
        self.calls.append((weight, eps))

    def set_weights(self, *args):
        pass


class _Model:
    def __init__(self):
        self.engine = _FakeEngine()

    def layers(self):
        return ['data', 'conv1_1']


@pytest.mark.parametrize('terms', list(itertools.product((False, True), repeat=3)), ids=lambda t: ''.join(n for n, on in zip('lam', t) if on) or 'none')
def test_trace_names_for_every_combination_of_the_three_optional_terms(terms):
    st = StyleTransfer(_Model())
    st.set_weights({'content': {'conv1_1': 1}, 'style': {}, 'deepdream': {}}, {'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2})
    st.engine.terms = terms
    on = [n for n, flag in zip('lam', terms) if flag]
    names = ['scd', 't', 'p'] + on
    values = np.arange(6 + 8 + 2 * len(on), dtype=np.float64)
    layer = ['conv1_1_c_loss', 'conv1_1_c_grad']
    want = layer + [n + '_loss' for n in names] + [n + '_grad' for n in names] + ['time', 'loss', 'grad']
    t = st._make_trace(values, True).data
    assert list(t) == want
    k = len(names)
    assert [t[n + '_loss'] for n in names] == list(range(6, 6 + k)) and [t[n + '_grad'] for n in names] == list(range(6 + k, 6 + 2 * k))
    assert (t['loss'], t['grad']) == (6 + 2 * k, 6 + 2 * k + 1)
    t = st._make_trace(values, False).data
    assert list(t) == layer + [n + '_loss' for n in names] + ['loss'] and t['loss'] == 6 + 2 * k


def test_ten_values_are_told_apart_by_the_engine_not_by_their_number():
    st = StyleTransfer(_Model())
    st.set_weights({'content': {'conv1_1': 1}, 'style': {}, 'deepdream': {}}, {'p': 1, 'p_power': 6, 'tv': 1, 'tv_power': 2})
    v10 = np.arange(16, dtype=np.float64)
    seen = []
    for terms, name in (((True, False, False), 'l'), ((False, True, False), 'a'), ((False, False, True), 'm')):
        st.engine.terms = terms
        keys = list(st._make_trace(v10, True).data)
        assert keys[keys.index('p_loss') + 1] == name + '_loss' and keys[keys.index('p_grad') + 1] == name + '_grad'
        seen.append(keys)
    assert len({tuple(k) for k in seen}) == 3
    st.set_matting(5.0)
    st.set_matting(7.0, 1e-3)
    assert st.engine.calls == [(5.0, 1e-7), (7.0, 1e-3)]
