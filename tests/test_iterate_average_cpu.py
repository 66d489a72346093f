"""CPU side of iterate averaging (st_set_iterate_average; csrc/passes.hip): the NumPy restatement the GPU tests hold the engine to
(tests/average_oracle.py) against vectors recorded from the reference's own ``utils.DecayingMean`` (tests/golden/iterate_average.npz,
made by tests/golden/make_iterate_average.py), the ABI declarations and their binding, the worker's config key and the command-line
flag.  No GPU."""

import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from average_oracle import MEAN, AverageOracle, deprocess
from helpers import load
from style_transfer2_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


def test_restatement_equals_the_reference_class_at_every_item():
    g = load('iterate_average.npz')
    decays = [float(d) for d in g['decays']]
    assert decays == [0.9, 0.5, 0.999]
    for k, d in enumerate(decays):
        items = g['items_%d' % k]
        assert items.dtype == F32 and items.shape == (6, 3, 5, 7)
        for item in items:                                  # the fixture holds what the issue asks for: an exact 0 and a -0.0 per array
            zeros = item[item == 0]
            assert zeros.size == 2 and sorted(np.signbit(zeros)) == [False, True]
        avg = AverageOracle(d)
        for i, item in enumerate(items):
            avg.update(item)
            assert avg.items == i + 1
            assert avg.mean.dtype == F32 and np.array_equal(avg.mean, g['mean_%d' % k][i]), (d, i)
            got = avg.corrected()
            assert got.dtype == F32 and np.array_equal(got, g['corrected_%d' % k][i]), (d, i)
            # bit patterns too: array_equal takes 0.0 == -0.0
            assert np.array_equal(avg.mean.view(np.uint32), g['mean_%d' % k][i].view(np.uint32)), (d, i)


def test_restatement_clears_resamples_and_deprocesses():
    avg = AverageOracle(0.9)
    with pytest.raises(ValueError):
        avg.corrected()
    x = (np.random.RandomState(0).randn(1, 3, 16, 32) * 50).astype(F32)
    avg.update(x)
    assert np.array_equal(avg.mean, F32(0.9) * np.zeros_like(x) + F32(1.0 - 0.9) * x) and avg.corr() == F32(1.0 - 0.9)
    img = avg.image()
    assert img.shape == (16, 32, 3) and img.dtype == F32
    assert np.array_equal(img[3, 5], avg.corrected()[0, :, 3, 5] + MEAN)
    assert np.array_equal(deprocess(x), deprocess(x[0]))
    from style_transfer2_amd import resample
    want = resample.resample_nchw(avg.mean, (24, 40))
    avg.resample((24, 40))
    assert avg.items == 1 and avg.mean.shape == (1, 3, 24, 40) and np.array_equal(avg.mean, want)
    avg.resample((16, 32), new_x=True)
    assert avg.items == 0 and avg.mean is None
    avg.update(x); avg.clear()
    assert avg.items == 0 and avg.mean is None
    for bad in (0.0, 1.0, -0.1, float('nan')):
        with pytest.raises(ValueError):
            AverageOracle(bad)


def test_the_three_symbols_are_declared_in_the_header_and_bound():
    with open(os.path.join(ROOT, 'include', 'st2.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+st_set_iterate_average\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*double\s+decay\s*\)\s*;', header)
    assert re.search(r'\bint\s+st_get_iterate_average\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*decay\s*,\s*int\s*\*\s*items\s*,'
                     r'\s*float\s*\*\s*mean_nchw\s*\)\s*;', header)
    assert re.search(r'\bint\s+st_tile_get_tile_average\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*float\s*\*\s*out_hwc\s*\)\s*;', header)
    assert 'do NOT update it' in header                    # the phase-by-phase entry points: said in the header
    from ctypes import POINTER, c_double, c_int, c_void_p
    assert capi.PROTOTYPES['st_set_iterate_average'] == (c_int, [c_void_p, c_double])
    assert capi.PROTOTYPES['st_get_iterate_average'] == (c_int, [c_void_p, POINTER(c_double), POINTER(c_int), c_void_p])
    assert capi.PROTOTYPES['st_tile_get_tile_average'] == (c_int, [c_void_p, c_void_p])


def _section(**keys):
    import configparser
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {k: str(v) for k, v in keys.items()}})
    return cp['worker']


def test_worker_reads_the_iterate_average_key_with_a_reader_of_its_own():
    sys.path.insert(0, ROOT)
    import worker
    assert 'iterate_average' not in worker.ALGO_KEYS and worker.read_algo_keys(_section(iterate_average=0.9)) == {}
    assert worker.read_iterate_average(_section(gpu=0)) is None            # absent: no call is made
    assert worker.read_iterate_average(_section(iterate_average='')) is None
    assert worker.read_iterate_average(_section(iterate_average=0.9)) == 0.9
    assert worker.read_iterate_average({'iterate_average': ' 0.5 '}) == 0.5
    assert worker.read_iterate_average(_section(iterate_average=0)) == 0.0   # off, said explicitly
    for bad in (1, 1.0, -0.1, 2, 'nan', 'x', 'inf'):
        with pytest.raises(ValueError, match='iterate_average'):
            worker.read_iterate_average(_section(iterate_average=bad))


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_iterate_average(self, decay):
        self.calls.append(decay)


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


def test_worker_hands_the_key_to_the_engine_before_it_reports_ready():
    sys.path.insert(0, ROOT)
    import worker
    for config, calls in (({'async_iterate': '0'}, []), ({'async_iterate': '0', 'iterate_average': '0.9'}, [0.9]),
                          ({'async_iterate': '0', 'iterate_average': '0'}, [0.0])):
        tr, socks = _FakeTransfer(), _Socks()
        worker.Worker(config, sock_in=socks, sock_out=socks, transfer=tr)
        assert tr.engine.calls == calls and [type(m).__name__ for m in socks.sent] == ['WorkerReady']
    tr, socks = _FakeTransfer(), _Socks()
    with pytest.raises(ValueError, match='iterate_average'):
        worker.Worker({'async_iterate': '0', 'iterate_average': '1.5'}, sock_in=socks, sock_out=socks, transfer=tr)
    assert tr.engine.calls == [] and socks.sent == []


def _stylize():
    spec = importlib.util.spec_from_file_location('stylize_tool', os.path.join(ROOT, 'tools', 'stylize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_parses_avg_decay(capsys):
    ap = _stylize().parser()
    assert ap.parse_args(['c.jpg', 's.jpg', 'o.png']).avg_decay is None
    assert ap.parse_args(['c.jpg', 's.jpg', 'o.png', '--avg-decay', '0.9']).avg_decay == 0.9
    assert ap.parse_args(['c.jpg', 's.jpg', 'o.png', '--avg-decay', '0', '--grid', '1x2']).avg_decay == 0.0
    for bad in ('1', '-0.5', 'nan', 'x'):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(['c.jpg', 's.jpg', 'o.png', '--avg-decay', bad])
        assert e.value.code == 2
    assert '--avg-decay' in capsys.readouterr().err


def test_jobs_take_iterate_average():
    import inspect
    from style_transfer2_amd import jobs
    for fn in (jobs.run_job, jobs.run_tiled_job):
        assert inspect.signature(fn).parameters['iterate_average'].default is None
