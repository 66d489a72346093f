"""CPU side of the split-operand Gram / style-gradient option (st_set_gram_algo; csrc/gram_split.hip): the ABI declaration and its
binding, the arithmetic's floor restated in numpy (split_gemm_oracle.py), the worker's config keys and the argument checks of the
Python engine."""
import configparser
import os
import re
import sys

import numpy as np
import pytest

from split_gemm_oracle import is_bf16, rel_l2, split3, split_gram, split_matmul

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
F32 = np.float32


def test_gram_algo_is_declared_in_the_header_and_bound():
    from style_transfer2_amd import capi
    with open(os.path.join(REPO, 'include', 'st2.h')) as f:
        header = f.read()
    assert re.search(r'\bint\s+st_set_gram_algo\s*\(\s*st_ctx\s*\*\s*ctx\s*,\s*int\s+algo\s*\)\s*;', header)
    assert re.search(r'\bint\s+st_get_algos\s*\(', header)
    assert 'worker.py:109-114, 258-269' in header
    assert 'st_set_gram_algo' in capi.PROTOTYPES and 'st_get_algos' in capi.PROTOTYPES


def test_split3_terms_are_bf16_and_sum_exactly():
    rng = np.random.RandomState(0)
    x = np.concatenate([
        rng.randn(4096).astype(F32) * 40,
        -np.abs(rng.randn(1024)).astype(F32),
        (rng.randn(4096) * np.exp2(rng.randint(-20, 20, 4096))).astype(F32),       # 40 binades
        np.zeros(16, F32), np.array([-0.0, 1.0, -1.0, 255.5, 1 + 2.0 ** -23, -(1 + 2.0 ** -8 + 2.0 ** -23), 3.0e38, 1e-30], F32)])
    x1, x2, x3 = split3(x)
    assert is_bf16(x1) and is_bf16(x2) and is_bf16(x3)
    assert np.array_equal(x1.astype(np.float64) + x2.astype(np.float64) + x3.astype(np.float64), x.astype(np.float64))
    assert np.all(np.abs(x2) <= np.abs(x1) * 2.0 ** -7 + 1e-45) and np.all(np.abs(x3) <= np.abs(x1) * 2.0 ** -15 + 1e-45)


@pytest.mark.parametrize('c,hw', [(64, 4096), (128, 2048), (256, 1024)])
def test_the_dropped_products_leave_a_floor_far_below_fp32_summation(c, hw):
    """ReLU'd randn x 40 features.  Measured here: Gram 3.0e-9 .. 5.0e-9, D @ F 1.5e-8 against float64 (numpy's fp32 BLAS:
    7e-8 .. 9e-8 and 1.0e-7 .. 2.1e-7); the bars are ~3 - 4 x those values, which depend on nothing but numpy."""
    rng = np.random.RandomState(c)
    f = np.maximum(rng.randn(c, hw) * 40, 0).astype(F32)
    f64 = f.astype(np.float64)
    g_err = rel_l2(split_gram(f), f64 @ f64.T)
    d = (rng.randn(c, c) * 1e3).astype(F32)
    s_err = rel_l2(split_matmul(d, f), d.astype(np.float64) @ f64)
    print('C %d hw %d: gram %.3g  D@F %.3g  (fp32 BLAS: %.3g, %.3g)' % (c, hw, g_err, s_err, rel_l2(f @ f.T, f64 @ f64.T),
                                                                     rel_l2(d @ f, d.astype(np.float64) @ f64)))
    assert g_err <= 2e-8
    assert s_err <= 5e-8


def _worker():
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    import worker
    return worker


def _section(**keys):
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {k: str(v) for k, v in keys.items()}})
    return cp['worker']


def test_worker_reads_the_algorithm_keys():
    worker = _worker()
    assert worker.read_algo_keys(_section(gpu=0)) == {}                           # absent keys: no call is made
    assert worker.read_algo_keys(_section(conv_algo=2, gram_algo=1)) == {'conv_algo': 2, 'gram_algo': 1}
    assert worker.read_algo_keys(_section(gram_algo=0)) == {'gram_algo': 0}
    assert worker.read_algo_keys({'conv_algo': ' 1 '}) == {'conv_algo': 1}
    with pytest.raises(ValueError, match='conv_algo'):
        worker.read_algo_keys(_section(conv_algo=7))
    with pytest.raises(ValueError, match='gram_algo'):
        worker.read_algo_keys(_section(gram_algo='x'))
    with pytest.raises(ValueError, match='gram_algo'):
        worker.read_algo_keys(_section(conv_algo=2, gram_algo=2))


def test_the_shipped_config_leaves_both_keys_unset():
    worker = _worker()
    cp = configparser.ConfigParser()
    cp.read(os.path.join(REPO, 'config.ini'))
    assert worker.read_algo_keys(cp['DEFAULT']) == {}
    with open(os.path.join(REPO, 'config.ini')) as f:
        text = f.read()
    assert '# conv_algo = 2' in text and '# gram_algo = 1' in text


class _StubLib:
    def __init__(self):
        self.calls = []

    def st_set_conv_algo(self, ctx, v):
        self.calls.append(('conv', v)); return 0

    def st_set_gram_algo(self, ctx, v):
        self.calls.append(('gram', v)); return 0

    def st_destroy(self, ctx):
        return 0


def _stub_engine():
    from style_transfer2_amd.engine import Engine
    e = Engine.__new__(Engine)
    e.lib, e._ctx = _StubLib(), None
    return e


def test_engine_refuses_unknown_algorithms():
    e = _stub_engine()
    for bad in (3, -1, 'x', 1.5, None):
        with pytest.raises(ValueError):
            e.set_conv_algo(bad)
    for bad in (2, -1, 'x', None):
        with pytest.raises(ValueError):
            e.set_gram_algo(bad)
    assert e.lib.calls == []
    for ok in (0, 1, 2, False, True):
        e.set_conv_algo(ok)
    e.set_gram_algo(0); e.set_gram_algo(1)
    assert e.lib.calls == [('conv', 0), ('conv', 1), ('conv', 2), ('conv', 0), ('conv', 1), ('gram', 0), ('gram', 1)]


def test_hip_model_applies_the_algorithms_after_construction():
    from style_transfer2_amd.model import HipModel
    e = _stub_engine()
    HipModel(None, engine=e)
    assert e.lib.calls == []
    HipModel(None, engine=e, conv_algo=2, gram_algo=1)
    assert e.lib.calls == [('conv', 2), ('gram', 1)]
    with pytest.raises(ValueError):
        HipModel(None, engine=e, gram_algo=5)
