"""The specialised Winograd epilogues (csrc/conv3x3_winograd.hip, EPI != 0) issue the operand loads of every batch of accumulator
rows -- bias, ReLU mask, injected diff -- ahead of the first store, the first groups of them under the MFMAs of the LAST chunk of the
K loop and the rest right after it.  ST2_WINO_EPI=0 keeps the generic epilogue, which loads batch by batch: every comparison here is
ST2_WINO_EPI=1 against ST2_WINO_EPI=0, bit for bit, through HipModel forward / backward (and three lean iterations for the builds
that write the pooled blob only).

What the cases of tests/test_gpu_winograd.py (K >= 64 everywhere) do not reach and these do:
  * reduction depths K = 8, 16, 24, 32: 1, 2, 3, 4 chunks -- three different ways into the last chunk, with one chunk the last is also
    the first after the prologue.  K below 64 never splits K, so the specialised builds run at these sizes.  A data gradient that
    shallow comes from a conv with K OUTPUT channels above a blob of M >= 48 channels (its forward is the direct kernel);
  * K = 64 in one pass (ST2_WINO_SPLITK=0);
  * both tiles: M = 48 and 64 take the half tile, M = 72 and 128 the 128-channel tile; 48 and 72 leave rows beyond M;
  * heights that are no multiple of 4 and odd ones (dead lanes: out-of-range offsets), widths of 32 and of 36 / 40 (a partial tile
    column); the pooled kinds on even heights and widths that are multiples of 4;
  * masked and unmasked data gradients with and without an injected diff; bias_std > 0, so that a bias on the wrong row shows.
The unpooling data gradient cannot be reached below K = 48: its route needs the arg-max map that only a Winograd forward with the
fused pool writes, i.e. a conv of >= 48 output channels, and those are its K.  It runs here at K = 48, 56 (6 and 7 chunks, never
split) and 64 (ST2_WINO_SPLITK=0); its last chunk and epilogue are the masked data gradient's, which the shallow cases cover.

Which build a case launched cannot be asserted from Python.  Kernel table of this file under `rocprofv3 --kernel-trace --stats`
(MI355X, calls per kernel; every one of the twelve specialised builds, and the generic ones of the ST2_WINO_EPI=0 halves):
    conv3x3_wino_f32_128x128                                348
    conv3x3_wino_f32_128x128_anyw                             4
    conv3x3_wino_f32_128x128_dg                              78
    conv3x3_wino_f32_128x128_dgm                            168
    conv3x3_wino_f32_128x128_fwd                             74
    conv3x3_wino_f32_128x128_noout                            6
    conv3x3_wino_f32_128x128_pool                            28
    conv3x3_wino_f32_128x128_poolonly                         6
    conv3x3_wino_f32_128x128_unpool                          36
    conv3x3_wino_f32_128x128_unpool_dgm                      36
    conv3x3_wino_f32_64x256_anyw                              4
    conv3x3_wino_f32_h4_64x128                              456
    conv3x3_wino_f32_h4_64x128_dg                           126
    conv3x3_wino_f32_h4_64x128_dgm                          192
    conv3x3_wino_f32_h4_64x128_fwd                           86
    conv3x3_wino_f32_h4_64x128_noout                          6
    conv3x3_wino_f32_h4_64x128_pool                          52
    conv3x3_wino_f32_h4_64x128_poolonly                       6
    conv3x3_wino_f32_h4_64x128_unpool                        36
    conv3x3_wino_f32_h4_64x128_unpool_dgm                    36
"""

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2

pytestmark = pytest.mark.gpu
F32 = np.float32
DEPTHS = (8, 16, 24, 32)
CHANNELS = (48, 64, 72, 128)


def _both_epilogues(monkeypatch, run):
    """run() under ST2_WINO_EPI=1 and =0 (read per launch)"""
    out = {}
    for epi in ('1', '0'):
        monkeypatch.setenv('ST2_WINO_EPI', epi)
        out[epi] = run()
    return out['1'], out['0']


def _same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (what, i)


def _chain(k, m):
    """conv1_3 forward: K = k (forward kind); conv1_2 data gradient: K = k, M = m, masked by conv1_1"""
    return (('conv', 'conv1_1', 3, m), ('conv', 'conv1_2', m, k), ('conv', 'conv1_3', k, m))


def _pooled(k, m):
    """conv1_3 forward: K = k with the fused pool; conv2_1 data gradient: K = k, M = m, no mask (pool1 below); conv2_2 forward and
    conv1_2 data gradient as in _chain"""
    return _chain(k, m) + (('pool', 'pool1'), ('conv', 'conv2_1', m, k), ('conv', 'conv2_2', k, m))


def _unpooled(k, m):
    """conv1_2 forward: Winograd with the fused pool and its arg-max map; conv1_2 data gradient: K = k, M = m, reads the pooled diff"""
    return (('conv', 'conv1_1', 3, m), ('conv', 'conv1_2', m, k), ('pool', 'pool1'), ('conv', 'conv2_1', k, m))


def _run(topo, h, w, blobs, diff_sets, seed):
    params = oracle.he_init_weights(topo, seed=seed, bias_std=0.3)
    rng = np.random.RandomState(seed + h * w)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)

    def run():
        gpu = st2.HipModel(params, topology=topo)
        f = gpu.forward(x, sorted(set(blobs).union(*diff_sets)))
        r2 = np.random.RandomState(7)
        grads = [gpu.backward({n: r2.randn(*f[n].shape).astype(F32) for n in names}) for names in diff_sets]
        return [f[n] for n in blobs] + grads
    return run


@pytest.mark.parametrize('m', CHANNELS)
@pytest.mark.parametrize('k', DEPTHS + (64,))
def test_forward_and_masked_data_gradient_at_shallow_depths(k, m, monkeypatch):
    """forward kind (conv1_3, K = k) and masked data gradient (conv1_2, K = k) without and with a diff injected at conv1_1, on heights
    that are odd / no multiple of 4 and widths of 32, 36 and 40.  k = 64: one pass (ST2_WINO_SPLITK=0)."""
    if k == 64:
        monkeypatch.setenv('ST2_WINO_SPLITK', '0')
    for h, w in ((7, 36), (10, 40), (5, 32)):
        a, b = _both_epilogues(monkeypatch, _run(_chain(k, m), h, w, ['conv1_1', 'conv1_2', 'conv1_3'],
                                                 (('conv1_3',), ('conv1_3', 'conv1_1'), ('conv1_2', 'conv1_1')), seed=k + m))
        _same(a, b, (k, m, h, w))
        assert float(np.abs(a[-1]).max()) > 0


@pytest.mark.parametrize('m', CHANNELS)
@pytest.mark.parametrize('k', DEPTHS)
def test_pooled_forward_and_unmasked_data_gradient_at_shallow_depths(k, m, monkeypatch):
    """forward + pool kind (conv1_3, K = k; even heights, widths % 4 == 0: with the arg-max map) and the unmasked data gradient
    (conv2_1, K = k, above pool1) without a diff at pool1 and with one."""
    for h, w in ((10, 40), (12, 72), (6, 32)):
        a, b = _both_epilogues(monkeypatch, _run(_pooled(k, m), h, w, ['conv1_3', 'pool1', 'conv2_1', 'conv2_2'],
                                                 (('conv2_2',), ('conv2_2', 'pool1'), ('conv2_1', 'pool1', 'conv1_1')), seed=k + m))
        _same(a, b, (k, m, h, w))
        assert float(np.abs(a[-1]).max()) > 0


@pytest.mark.parametrize('m', CHANNELS)
@pytest.mark.parametrize('k', (48, 56, 64))
def test_unpooling_data_gradient_in_one_pass(k, m, monkeypatch):
    """unpooling masked data gradient (conv1_2, K = k, W % 32 == 0, H even) without and with a diff injected at conv1_1.  One pass
    everywhere (ST2_WINO_SPLITK=0): a split forward has no fused pool, hence no map to unpool through."""
    monkeypatch.setenv('ST2_WINO_SPLITK', '0')
    for h, w in ((6, 32), (10, 64)):
        a, b = _both_epilogues(monkeypatch, _run(_unpooled(k, m), h, w, ['conv1_2', 'pool1', 'conv2_1'],
                                                 (('conv2_1',), ('conv2_1', 'conv1_1'), ('pool1',)), seed=k + m))
        _same(a, b, (k, m, h, w))
        assert float(np.abs(a[-1]).max()) > 0


@pytest.mark.parametrize('k,m', [(8, 48), (16, 64), (24, 72), (32, 128)])
def test_pooled_blob_only_builds_in_lean_iterations_at_shallow_depths(k, m, monkeypatch):
    """pooled-blob-only kind: inside an iteration the full-resolution blob of conv1_3 (pooled, no weight) is not written.  Iterates
    and traces of three Adam steps on a 64 x 96 image."""
    topo = _pooled(k, m)
    params = oracle.he_init_weights(topo, seed=k + m, bias_std=0.2)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (64, 96, 3)).astype(np.uint8), rs(2).randint(0, 256, (40, 36, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (64, 96, 3)).astype(np.uint8))
    weights = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_2': 1}, 'deepdream': {}}

    def run():
        dev = st2.StyleTransfer(st2.HipModel(params, topology=topo))
        dev.set_input(init); dev.set_content(content); dev.set_style(style); dev.reset()
        dev.set_weights(weights, {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2})
        dev.optimizer_cls = st2.AdamOptimizer; dev.set_step_size(10); dev.reset()
        assert dev.start()
        steps = [(np.asarray(i).copy(), dict(t)) for i, t in (dev.step() for _ in range(3))]
        with pytest.raises(st2.StError):
            dev.engine.get_blob('conv1_3')                  # pooled, un-weighted: not written inside the step
        return steps
    for (ia, ta), (ib, tb) in zip(*_both_epilogues(monkeypatch, run)):
        assert np.array_equal(ia, ib)
        for key in ta:
            if key != 'time':
                assert ta[key] == tb[key] or (np.isnan(ta[key]) and np.isnan(tb[key])), key
