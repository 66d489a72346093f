"""CPU side of the average-pool fusion switch (st_set_pool_algo; csrc/conv3x3_mfma_bf16.hip): the ABI declaration and its binding,
the worker's config key and the command-line tool's refusal of average pools in tile-sharded mode.  No GPU."""

import os
import re
import subprocess
import sys

import pytest

from style_transfer2_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pool_algo_is_declared_in_the_header_and_bound():
    with open(os.path.join(ROOT, 'include', 'st2.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+st_set_pool_algo\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*int\s+algo\s*\)\s*;', header)
    assert re.search(r'\bint\s+st_get_pool_algo\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*int\s*\*\s*algo\s*\)\s*;', header)
    assert 'st_set_pool_algo' in capi.PROTOTYPES and 'st_get_pool_algo' in capi.PROTOTYPES


def _section(**keys):
    import configparser
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {k: str(v) for k, v in keys.items()}})
    return cp['worker']


def test_worker_reads_the_pool_algo_key():
    sys.path.insert(0, ROOT)
    import worker
    assert worker.ALGO_KEYS['pool_algo'] == (0, 1)
    assert worker.read_algo_keys(_section(pool_algo=1)) == {'pool_algo': 1}
    assert worker.read_algo_keys(_section(pool_algo=0, conv_algo=1)) == {'conv_algo': 1, 'pool_algo': 0}
    assert worker.read_algo_keys(_section(precision='bf16')) == {}
    for bad in (2, 'x'):
        with pytest.raises(ValueError, match='pool_algo'):
            worker.read_algo_keys(_section(pool_algo=bad))


class _FakeLib:
    """Records the ABI calls Engine.set_pool_algo / pool_algo make."""

    def __init__(self):
        self.value, self.calls = 0, []

    def st_set_pool_algo(self, ctx, v):
        self.calls.append(v)
        self.value = v
        return 0

    def st_get_pool_algo(self, ctx, ref):
        ref._obj.value = self.value
        return 0


def test_engine_and_model_validate_pool_algo_before_the_abi():
    from style_transfer2_amd.engine import Engine
    from style_transfer2_amd.model import HipModel
    e = Engine.__new__(Engine)
    e.lib, e._ctx = _FakeLib(), None
    for bad in (2, -1, 'x', None):
        with pytest.raises(ValueError, match='pool_algo'):
            e.set_pool_algo(bad)
    assert e.lib.calls == []
    e.set_pool_algo(1)
    assert e.lib.calls == [1] and e.pool_algo() == 1
    HipModel(None, engine=e)                       # None: no call
    assert e.lib.calls == [1]
    HipModel(None, engine=e, pool_algo=0)
    assert e.lib.calls == [1, 0]
    with pytest.raises(ValueError, match='pool_algo'):
        HipModel(None, engine=e, pool_algo=5)


def test_stylize_refuses_average_pools_with_a_grid_before_it_imports_the_engine(tmp_path):
    """--ave-pools --grid is a usage error (exit status 2, argparse), raised before the package -- let alone the HIP library -- is
    imported: the run needs neither images nor a GPU."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'stylize.py'), 'c.jpg', 's.jpg', 'o.png', '--ave-pools', '--grid', '1x2'],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert 'usage:' in r.stderr and '--ave-pools' in r.stderr and 'tile-sharded' in r.stderr
    assert 'Traceback' not in r.stderr
    with open(os.path.join(ROOT, 'tools', 'stylize.py')) as f:
        text = f.read()
    assert text.index('ap.error(') < text.index('import style_transfer2_amd')
    for flag in ('--ave-pools', '--pool-algo', '--precision'):
        assert flag in text
