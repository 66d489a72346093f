"""GPU tests of the split-operand Gram / style-gradient kernels (csrc/gram_split.hip) behind st_set_gram_algo(ctx, 1), through the
C ABI: the kernels against float64 on the blobs the GPU itself wrote, the objective against the CPU oracle at the fp32 kernels' bars,
whole jobs against the same jobs with the option off, the worker's config keys, and the places where the option promises no effect."""
import collections
import configparser
import os
import pickle
import sys
from collections import deque

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2
from helpers import check_trace, rel_l2

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SPLIT_CLASSES = ('gram_partial_split_bf16x6', 'style_grad_split_bf16x6')
VGG_WEIGHTS = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1}, 'deepdream': {}}
PARAMS4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
# (h, w): a 1 x 4 blob, hw = 36 (not a multiple of 32: a ragged, zero-filled step), hw = 35 (odd: register staging), whole steps
GRAM_SIZES = [(1, 4), (6, 6), (5, 7), (32, 64), (48, 80)]
# Measured on one MI355X over the grid below (C = 128, 256, 512), rel-L2 against the float64 Gram of the same blob: split
# 3.3e-8 .. 9.2e-8 (largest: C = 128 at 48 x 80), the fp32 kernel on the same blobs 3.0e-8 .. 9.1e-8 -- at these sizes both sit on
# the rounding of the fp32 output itself (2^-24 = 6e-8 per entry).  The bar is 3 x the largest split value.
GRAM_TIGHT = 2.76e-7


def launches(engine):
    return collections.Counter({k: v['launches'] for k, v in engine.profile_read().items()})


def gram64(f):
    f = np.asarray(f, np.float64).reshape(f.shape[-3], -1)
    return f @ f.T / f.size


@pytest.mark.parametrize('c', [64, 128, 192, 256, 512])
def test_gram_against_float64_on_the_gpus_own_blob(c):
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, c))
    params = oracle.he_init_weights(topo, seed=c, bias_std=0.1)
    m = st2.HipModel(params, topology=topo)
    eng = m.engine
    assert eng.algos() == (1, 0)
    for h, w in GRAM_SIZES:
        x = (np.random.RandomState(h * w + c).randn(1, 3, h, w) * 40).astype(F32)
        eng.forward(x, 'conv1_2')
        ref = gram64(eng.get_blob('conv1_2'))
        eng.set_gram_algo(0)
        g0 = eng.gram('conv1_2')
        eng.set_gram_algo(1)
        assert eng.algos() == (1, 1)
        g1 = eng.gram('conv1_2')
        e0, e1 = rel_l2(g0, ref), rel_l2(g1, ref)
        print('C %d %dx%d: split %.3g  fp32 kernel %.3g' % (c, h, w, e1, e0))
        assert e1 <= 1e-5, (h, w)
        assert e1 <= GRAM_TIGHT, (h, w, e1)
        # C = 64 is refused (HBM-bound, measured: no gain) and runs the fp32 kernel bit for bit; everything else is taken
        assert np.array_equal(g1, g0) == (c == 64), (h, w)
        assert np.array_equal(g1, g1.T), (h, w)                  # exactly symmetric
        assert np.array_equal(eng.gram('conv1_2'), g1), (h, w)   # bitwise reproducible
    eng.set_gram_algo(0)


def test_refused_shapes_run_the_fp32_kernel_bit_for_bit():
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 200), ('conv', 'conv1_3', 200, 32))
    m = st2.HipModel(oracle.he_init_weights(topo, seed=3, bias_std=0.1), topology=topo)
    x = (np.random.RandomState(5).randn(1, 3, 16, 24) * 40).astype(F32)
    m.engine.forward(x)
    for name, taken in (('data', False), ('conv1_1', False), ('conv1_2', False), ('conv1_3', False)):
        m.engine.set_gram_algo(0)
        g0 = m.engine.gram(name)
        m.engine.set_gram_algo(1)
        assert np.array_equal(m.engine.gram(name), g0) == (not taken), name


def _tiny_job(c, weights, size=(24, 40), **kw):
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, c))
    params = oracle.he_init_weights(topo, seed=1, bias_std=0.1)
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, params))
    dev = st2.StyleTransfer(st2.HipModel(params, topology=topo, **kw))
    rs = np.random.RandomState
    h, w = size
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (20, 28, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, PARAMS4)
    return cpu, dev


@pytest.mark.parametrize('c', [64, 128, 192, 512])
@pytest.mark.parametrize('with_content', [False, True])
def test_style_gradient_first_and_steady_evaluation_match_the_oracle(c, with_content):
    """One style weight on one layer: the first evaluation captures the norm from the unscaled S, the second runs the fused epilogue
    (sw / norm, on top of the content diff when there is one: accumulate).  The bars of tests/test_gpu_parity.py."""
    weights = {'content': {'conv1_2': 0.5} if with_content else {}, 'style': {'conv1_2': 1.0}, 'deepdream': {}}
    cpu, dev = _tiny_job(c, weights, gram_algo=1)
    dev.model.engine.profile_enable(True)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    assert np.isclose(ld, lo, rtol=1e-4) and rel_l2(gd, go) <= 1e-4
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=1e-4)
    x2 = cpu.input + F32(2.0) * np.sign(go)
    lo, go = cpu.opfunc(x2)
    ld, gd = dev.opfunc(x2)
    assert np.isclose(ld, lo, rtol=1e-4) and rel_l2(gd, go) <= 1e-4
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=1e-4)
    n = launches(dev.model.engine)
    new, old = (0, 2) if c == 64 else (2, 0)                     # C = 64 keeps the fp32 kernels
    assert n[SPLIT_CLASSES[0]] == new and n[SPLIT_CLASSES[1]] == new and n['style_grad_mfma_f32'] == old and n['gram_partial_mfma_f32'] == old


def _vgg_job(conv_algo, gram_algo, optimizer='adam', precision='fp32', size=(96, 128)):
    params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    st = st2.StyleTransfer(st2.HipModel(params, precision=precision, conv_algo=conv_algo, gram_algo=gram_algo))
    rs = np.random.RandomState
    h, w = size
    st.set_input(rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8)); st.set_content(rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8))
    st.set_style(rs(2).randint(0, 256, (h - 16, w, 3)).astype(np.uint8)); st.reset()
    st.set_weights(VGG_WEIGHTS, PARAMS4)
    st.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[optimizer]
    st.set_step_size({'adam': 10, 'lbfgs': 1}[optimizer])
    st.reset()
    assert st.start()
    return st


def _run(job, steps):
    out = [job.step() for _ in range(steps)]
    return [t['loss'] for _, t in out], np.asarray(out[-1][0], np.float64)


def test_vgg19_adam_steps_track_the_same_job_on_the_fp32_kernels():
    """Three Adam steps, VGG19 at 96 x 128, under conv algorithm 1 and 2.  Adam's first step is x -= 10 sign(g), so two fp32-grade
    arithmetics differ by what two others already do: the final iterate's MSE against the gram_algo 0 run is held to 2 x the MSE
    between conv algorithms 1 and 2 at gram_algo 0.  Measured on one MI355X: conv 1 vs 2 at gram_algo 0: 5.166e-6; gram_algo 1 vs 0:
    6.7e-9 (conv_algo 1), 5.172e-6 (conv_algo 2); the losses agree to 7 digits."""
    runs = {(ca, ga): _run(_vgg_job(ca, ga), 3) for ca in (1, 2) for ga in (0, 1)}
    yard = float(np.mean((runs[(1, 0)][1] - runs[(2, 0)][1]) ** 2))
    print('MSE conv_algo 1 vs 2 at gram_algo 0: %.4g' % yard)
    for ca in (1, 2):
        l0, x0 = runs[(ca, 0)]
        l1, x1 = runs[(ca, 1)]
        mse = float(np.mean((x1 - x0) ** 2))
        print('conv_algo %d: losses %s vs %s, MSE gram_algo 1 vs 0: %.4g' % (ca, l1, l0, mse))
        assert np.allclose(l1, l0, rtol=1e-4), (ca, l1, l0)
        assert mse <= 2 * yard, (ca, mse, yard)


# ------------------------------------------------------------------------------------------ the worker
class _Socks:
    """In-process stand-in for the worker's PULL / PUSH sockets: scripted inbound messages, everything sent kept."""

    class Again(Exception):
        pass

    def __init__(self, messages, pause_after):
        self.messages, self.pause_after = messages, pause_after
        self.inbound, self.sent = deque(), []

    def recv_pyobj(self, flags=0):
        if not self.inbound:
            if flags:
                raise self.Again()
            return self.messages.Shutdown()
        return pickle.loads(pickle.dumps(self.inbound.popleft()))

    def send_pyobj(self, obj):
        self.sent.append(obj)
        if isinstance(obj, self.messages.Iterate) and sum(isinstance(m, self.messages.Iterate) for m in self.sent) == self.pause_after:
            self.inbound.append(self.messages.PauseIteration())


def test_worker_takes_both_algorithms_from_its_config(tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import messages
    import worker as worker_mod
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {'prototxt': str(tmp_path / 'absent.prototxt'), 'caffemodel': str(tmp_path / 'absent.npz'), 'weights': 'synthetic',
                             'conv_algo': '2', 'gram_algo': '1', 'async_iterate': '0', 'pipeline_iterate': '1'}})
    socks = _Socks(messages, pause_after=4)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (64, 80, 3)).astype(np.uint8), rs(2).randint(0, 256, (48, 64, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (64, 80, 3)).astype(np.uint8))
    socks.inbound.extend([messages.SetImages(None, init, content, style, True), messages.SetWeights(VGG_WEIGHTS, PARAMS4),
                          messages.SetOptimizer('adam', 10), messages.StartIteration()])
    wk = worker_mod.Worker(cp['worker'], sock_in=socks, sock_out=socks)
    assert wk.transfer.model.engine.algos() == (2, 1)
    wk.run()
    kinds = [type(m).__name__ for m in socks.sent]
    assert kinds[0] == 'WorkerReady' and kinds[-1] == 'Shutdown' and kinds.count('Shutdown') == 1
    its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
    assert len(its) >= 4 and kinds == ['WorkerReady'] + ['Iterate'] * len(its) + ['Shutdown']
    assert [m.i for m in its] == list(range(1, len(its) + 1))
    assert all(np.isfinite(m.trace['loss']) and np.all(np.isfinite(m.image)) and m.image.shape == (64, 80, 3) for m in its)
    assert its[-1].trace['loss'] != its[0].trace['loss']
    assert wk.transfer.model.engine.algos() == (2, 1)


# ------------------------------------------------------------------------------------------ no effect where none is promised
def test_bf16_feature_path_ignores_the_option():
    a, b = _vgg_job(1, 0, 'lbfgs', 'bf16', (64, 80)), _vgg_job(1, 1, 'lbfgs', 'bf16', (64, 80))
    b.model.engine.profile_enable(True)
    for _ in range(3):
        ia, ta = a.step()
        ib, tb = b.step()
        assert ta['loss'] == tb['loss'] and np.array_equal(ia, ib)
    n = launches(b.model.engine)
    assert all(n[k] == 0 for k in SPLIT_CLASSES)


def test_option_off_launches_nothing_in_the_new_classes():
    job = _vgg_job(1, None, size=(64, 80))
    job.model.engine.profile_enable(True)
    job.step()
    n = launches(job.model.engine)
    assert all(n[k] == 0 for k in SPLIT_CLASSES) and n['gram_partial_mfma_f32'] == 5 and n['style_grad_mfma_f32'] == 5
    job.model.engine.set_gram_algo(1)
    job.step()
    n2 = launches(job.model.engine)
    assert all(n2[k] == 4 for k in SPLIT_CLASSES), n2            # conv2_1 .. conv5_1; conv1_1 (C = 64) keeps the fp32 kernels


def test_tile_sharded_mode_keeps_the_fp32_kernels():
    """A 1 x 2 in-process tile job with a style blob the split kernels would take (128 channels): bit-identical with the option
    on and off."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    topo = oracle.tiny_topology((64, 128), (1, 1))
    weights = {'content': {'conv2_1': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
    h, w, steps = 64, 128, 2
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (20, 28, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    net_params = oracle.he_init_weights(topo, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 2, topo, 5)
    results = []
    for algo in (0, 1):
        fabric = tiled.InProcessFabric(2, 120.0)
        ranks = []
        for r in range(2):
            backend = HipTileBackend(net_params, grid, r, content, style, init, weights, PARAMS4, step_size=10, topology=topo)
            backend.engine.set_gram_algo(algo)
            backend.comm_init_local(r, 2, fabric)
            ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
        results.append(tiled.run_in_process(ranks, steps, fabric, on_step=lambda r, k, tt, vals: (tt.tile_image(), vals)))
    for r in range(2):
        for k in range(steps):
            assert np.array_equal(results[0][r][k][0], results[1][r][k][0]), (r, k)
            assert np.array_equal(np.asarray(results[0][r][k][1]), np.asarray(results[1][r][k][1])), (r, k)


def test_a_planted_infinity_gives_a_non_finite_gram_under_both_algorithms():
    """A value check.  The split forms Inf - Inf, so entries the fp32 kernel gives as Inf may be NaN: only non-finiteness is promised."""
    topo = (('conv', 'conv1_1', 3, 128),)
    m = st2.HipModel(oracle.he_init_weights(topo, seed=2, bias_std=0.1), topology=topo)
    x = (np.random.RandomState(7).randn(1, 3, 8, 8) * 40).astype(F32)
    x[0, 1, 3, 4] = np.inf
    m.engine.forward(x)
    assert not np.all(np.isfinite(m.engine.get_blob('conv1_1')))
    for algo in (0, 1):
        m.engine.set_gram_algo(algo)
        assert not np.all(np.isfinite(m.engine.gram('conv1_1'))), algo
