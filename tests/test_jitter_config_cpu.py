"""CPU side of jitter's plumbing: the text form ``R`` / ``R:SEED``, the worker's config key (a malformed value fails at start with the key
named), the shift sequence of style_transfer2_amd.jitter against the restatement under tests/, jobs' keyword arguments, and
tools/stylize.py --jitter (refused with --grid).  No GPU."""
import importlib.util
import inspect
import os
import sys

import pytest

import jitter_oracle as jo
from style_transfer2_amd import jitter, jobs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAD = ('-1', '4097', '3:', ':7', 'x', '3:x', '3.0', '3:7:1', '3,7', '3:-1', '3:18446744073709551616', '1e2', '3 7', '0x3')


def test_text_form():
    assert jitter.parse_jitter('8') == (8, 0) and jitter.parse_jitter(' 8 : 1234 ') == (8, 1234)
    assert jitter.parse_jitter('4096:18446744073709551615') == (4096, jo.MASK64)
    assert jitter.parse_jitter('0') == jitter.parse_jitter('off') == jitter.parse_jitter('OFF') == jitter.parse_jitter('0:5')[:1] + (0,)
    for bad in BAD:
        with pytest.raises(ValueError):
            jitter.parse_jitter(bad)
    assert jitter.check_jitter(3, 7) == (3, 7)
    for bad in ((-1, 0), (4097, 0), (3, -1), (3, 1 << 64), (3.5, 0), (True, 0), ('3', 0), (None, 0)):
        with pytest.raises(ValueError):
            jitter.check_jitter(*bad)


def test_the_products_generator_is_the_restatements():
    assert [jitter.draw(1234567, k) for k in range(3)] == jo.DRAWS_1234567
    for (seed, radius), want in jo.PINS.items():
        assert [jitter.shift(seed, k, radius) for k in range(len(want))] == want
    for seed in (0, 7, jo.MASK64):
        for radius in (1, 3, 16, 4096):
            assert [jitter.shift(seed, k, radius) for k in range(200)] == [jo.shift(seed, k, radius) for k in range(200)]


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_jitter(self, radius, seed=0):
        self.calls.append((radius, seed))


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
    assert worker.read_jitter({'gpu': '0'}) is None and worker.read_jitter({'jitter': ' '}) is None      # absent: no call is made
    assert worker.read_jitter({'jitter': '3:7'}) == (3, 7) and worker.read_jitter({'jitter': '16'}) == (16, 0)
    assert worker.read_jitter({'jitter': 'off'}) == (0, 0) and worker.read_jitter({'jitter': 8}) == (8, 0)
    for bad in BAD:
        with pytest.raises(ValueError, match='config key jitter'):
            worker.read_jitter({'jitter': bad})
    for config, calls in (({'async_iterate': '0'}, []), ({'async_iterate': '0', 'jitter': '3:7'}, [(3, 7)]), ({'async_iterate': '0', 'jitter': '0'}, [(0, 0)])):
        tr, socks = _FakeTransfer(), _Socks()
        worker.Worker(config, sock_in=socks, sock_out=socks, transfer=tr)
        assert tr.engine.calls == calls and [type(m).__name__ for m in socks.sent] == ['WorkerReady']
    tr, socks = _FakeTransfer(), _Socks()
    with pytest.raises(ValueError, match='config key jitter'):
        worker.Worker({'async_iterate': '0', 'jitter': '4097'}, sock_in=socks, sock_out=socks, transfer=tr)
    assert tr.engine.calls == [] and socks.sent == []


def test_jobs_take_the_radius_and_the_seed():
    for fn in (jobs.run_job, jobs.run_frames):
        sig = inspect.signature(fn).parameters
        assert sig['jitter'].default is None and sig['jitter_seed'].default == 0
    assert 'jitter' not in inspect.signature(jobs.run_tiled_job).parameters          # tile-sharded jobs do not run it


def _stylize():
    spec = importlib.util.spec_from_file_location('stylize_tool', os.path.join(ROOT, 'tools', 'stylize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_takes_the_switches_and_refuses_them_with_a_grid(capsys):
    tool = _stylize()
    args = tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png', '--jitter', '8', '--jitter-seed', '1234'])
    assert (args.jitter, args.jitter_seed) == (8, 1234)
    args = tool.parser().parse_args(['c.jpg', 's.jpg', 'o.png'])
    assert args.jitter is None and args.jitter_seed is None
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--jitter', '8', '--grid', '1x2'])
    assert e.value.code == 2 and '--jitter with --grid' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--jitter-seed', '3'])
    assert e.value.code == 2 and '--jitter-seed without --jitter' in capsys.readouterr().err
    for bad in (['--jitter', '4097'], ['--jitter', '-1'], ['--jitter', '3', '--jitter-seed', '-5']):
        with pytest.raises(SystemExit) as e:
            tool.main(['c.jpg', 's.jpg', 'o.png'] + bad)
        assert e.value.code == 2 and '--jitter' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        tool.main(['c.jpg', 's.jpg', 'o.png', '--jitter', '3.5'])
    assert e.value.code == 2
