"""`bench.py --dump-outputs DIR` without a GPU: what bench.dump_outputs writes for a stand-in job (the whole iterate, or a
fixed seeded sample of a large one), and the plain stub run's single timed block of exactly --steps steps."""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench                    # noqa: E402
from style_transfer2_amd.model import HipModel      # noqa: E402


class FakeJob:
    """What dump_outputs reads of a StyleTransfer: the device-resident x (NCHW, mean-subtracted) and the model's deprocess."""
    def __init__(self, h, w):
        self.input = np.random.RandomState(7).randn(1, 3, h, w).astype(np.float32) * 50
        self.model = HipModel.__new__(HipModel)


def test_dump_outputs_writes_the_iterate_as_step_returns_it(tmp_path):
    job = FakeJob(24, 40)
    bench.dump_outputs(job, str(tmp_path / 'out'))
    assert os.listdir(tmp_path / 'out') == ['image.npy']
    img = np.load(tmp_path / 'out' / 'image.npy')
    assert img.dtype == np.float32 and img.shape == (24, 40, 3)
    want = job.input[0].transpose(1, 2, 0) + np.array((123.68, 116.779, 103.939), np.float32)
    assert np.array_equal(img, want)


def test_dump_outputs_samples_a_large_iterate_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 1000)
    job = FakeJob(64, 64)
    for run in ('a', 'b'):
        bench.dump_outputs(job, str(tmp_path / run))
        assert os.listdir(tmp_path / run) == ['image_sample.npy']
    a, b = np.load(tmp_path / 'a' / 'image_sample.npy'), np.load(tmp_path / 'b' / 'image_sample.npy')
    assert a.dtype == np.float32 and a.shape == (1000,) and np.array_equal(a, b)
    assert np.isin(a, HipModel.deprocess(job.model, job.input)).all()


def _run(args):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT')}
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + args, capture_output=True, text=True, timeout=300,
                          env=env, cwd=REPO)


def test_plain_run_times_one_block_of_exactly_the_given_steps():
    out = _run(['--steps', '7', '--warmup', '1', '--engine', 'stub'])
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip())
    assert d['steps'] == 7 and d['timing']['blocks'] == 1 and len(d['timing']['block_ms']) == 1
    assert d['ms_per_step'] == d['timing']['ms_per_step']['median'] and d['ms_per_step'] >= 1.0       # a stub step sleeps 1 ms


def test_dump_outputs_refuses_the_stub_engine(tmp_path):
    out = _run(['--steps', '2', '--engine', 'stub', '--dump-outputs', str(tmp_path / 'x')])
    assert out.returncode == 2 and '--dump-outputs' in out.stderr and not os.path.exists(tmp_path / 'x')
