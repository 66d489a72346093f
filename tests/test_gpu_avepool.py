"""Average pooling (prototxt ``pool: AVE``) on the MI355X: the stand-alone avepool_fwd / avepool_bwd passes on every precision and
conv algorithm, the routing around the max-pool fusions, the C ABI kind, whole VGG19 with average pools, the optimizers and the
worker.  Oracle: tests/avepool_oracle.py (Caffe's PoolingLayer AVE restated), fed with the GPU's own blobs where one layer is checked.
"""

import collections
import configparser
import ctypes
import os
import pickle
import sys
from collections import deque

import numpy as np
import pytest

import oracle
from oracle.caffe_net import bf16_round, conv3x3_backward_data, conv3x3_forward
import style_transfer2_amd as st2
from style_transfer2_amd import capi, prototxt
from avepool_oracle import AveNetOracle, avepool_backward, avepool_forward
from helpers import check_trace, load, rel_l2, tiny_setup

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24
HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (1, 5), (2, 257), (3, 513), (1, 600), (600, 1), (5, 1030), (16, 32), (64, 96)]
# fp32 with conv algorithm 0 (direct) / 1 (Winograd) / 2 (split-operand Winograd), the lean bf16 flow and bf16-full
PATHS = [('fp32', 0), ('fp32', 1), ('fp32', 2), ('bf16', 1), ('bf16-full', 1)]
# conv1_2 (64 -> 64) is the conv every max-pool fusion serves: Winograd pool epilogue + arg-max map, split-operand pool epilogue,
# bf16 fused pool; conv2_1 reads the pooled blob (bf16 path: the bf16 copy avepool_fwd writes) and its data gradient is the one
# that would unpool
NET = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1', 'ave'), ('conv', 'conv2_1', 64, 64))


def ave(topo, which=None):
    return tuple(('pool', l[1], 'ave') if l[0] == 'pool' and (which is None or l[1] in which) else l for l in topo)


def model(params, topo, precision, algo):
    m = st2.HipModel(params, topology=topo, precision=precision)
    m.engine.set_conv_algo(algo)
    return m


def launches(engine):
    return collections.Counter({k: v['launches'] for k, v in engine.profile_read().items()})


# ------------------------------------------------------------------------------------------ pool blobs
@pytest.mark.parametrize('precision,algo', PATHS)
def test_pool_blob_is_the_caffe_average_of_the_engines_own_conv_blob(precision, algo):
    """st_forward (every blob written) and an objective evaluation with the pool blob weighted (the lean flows): the pooled blob
    equals the oracle's average pooling of the engine's conv1_2 blob bit for bit, and conv2_1 reads it (bf16: through the
    bf16 copy avepool_fwd wrote)."""
    params = oracle.he_init_weights(NET, seed=5, bias_std=0.2)
    gpu = model(params, NET, precision, algo)
    bf16 = precision != 'fp32'
    for h, w in SHAPES:
        rs = np.random.RandomState(h * 7919 + w)
        x = (rs.randn(1, 3, h, w) * 40).astype(F32)
        gpu.engine.profile_enable(True)
        f = gpu.forward(x)
        n = launches(gpu.engine)
        gpu.engine.profile_enable(False)
        ref = avepool_forward(f['conv1_2'][0])
        assert f['pool1'].shape[1:] == ref.shape and np.array_equal(f['pool1'][0], ref), (h, w)
        assert n['avepool_fwd'] == 1 and n['maxpool_fwd'] == 0, (h, w, n)
        xin = bf16_round(f['pool1'][0]) if bf16 else f['pool1'][0]
        wgt = bf16_round(params['conv2_1'][0]) if bf16 else params['conv2_1'][0]
        ref2 = np.maximum(conv3x3_forward(xin, wgt, params['conv2_1'][1]), 0)
        assert rel_l2(f['conv2_1'][0], ref2) <= (3e-5 if bf16 else 1e-5), (h, w, rel_l2(f['conv2_1'][0], ref2))
    # lean evaluations (bf16: the objective; fp32: inside an Adam step): the conv blob below an average pool stays materialised
    rs = np.random.RandomState
    for h, w in ((64, 96), (17, 33)):
        st = st2.StyleTransfer(gpu)
        img = rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8)
        st.set_input(img); st.set_content(img); st.set_style(rs(2).randint(0, 256, (h, w, 3)).astype(np.uint8)); st.reset()
        st.set_weights({'content': {'pool1': 0.1}, 'style': {'conv2_1': 1}, 'deepdream': {}}, {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2})
        st.optimizer_cls = st2.AdamOptimizer; st.set_step_size(10); st.reset()
        assert st.start()
        st.opfunc()
        assert np.array_equal(gpu.engine.get_blob('pool1')[0], avepool_forward(gpu.engine.get_blob('conv1_2')[0]))
        st.step()
        assert np.array_equal(gpu.engine.get_blob('pool1')[0], avepool_forward(gpu.engine.get_blob('conv1_2')[0]))


# ------------------------------------------------------------------------------------------ backward
def _bound(params, f, diffs):
    """Per-element summation bound of the data gradient (fp32): the backward chain on absolute values, 2 * (sum of K + 2) * 2^-24
    times it."""
    m = np.zeros_like(f['conv2_1'][0], np.float64) if 'conv2_1' not in diffs else np.abs(diffs['conv2_1'][0]).astype(np.float64)
    m = conv3x3_backward_data(m.astype(F32), np.abs(params['conv2_1'][0])).astype(np.float64)
    if 'pool1' in diffs:
        m = m + np.abs(diffs['pool1'][0])
    m = avepool_backward(m.astype(F32), f['conv1_2'][0].shape).astype(np.float64) * (f['conv1_2'][0] > 0)
    if 'conv1_2' in diffs:
        m = m + np.abs(diffs['conv1_2'][0])
    m = conv3x3_backward_data(m.astype(F32), np.abs(params['conv1_2'][0])).astype(np.float64) * (f['conv1_1'][0] > 0)
    m = conv3x3_backward_data(m.astype(F32), np.abs(params['conv1_1'][0])).astype(np.float64)
    k = 9 * (64 + 64 + 64) + 2
    return 2.0 * k * U * m + 1e-30


@pytest.mark.parametrize('precision,algo', PATHS)
@pytest.mark.parametrize('inject', [('pool1',), ('conv1_2',), ('pool1', 'conv1_2'), ('conv2_1', 'pool1', 'conv1_2')])
def test_backward_through_the_average_pool(precision, algo, inject):
    params = oracle.he_init_weights(NET, seed=6, bias_std=0.2)
    gpu = model(params, NET, precision, algo)
    bf16 = precision != 'fp32'
    for h, w in ((64, 96), (17, 33), (3, 513)):
        rs = np.random.RandomState(h + w)
        x = (rs.randn(1, 3, h, w) * 40).astype(F32)
        f = gpu.forward(x)
        cpu = AveNetOracle(NET, params, operands='bf16' if bf16 else 'fp32')
        cpu.forward(x)
        cpu.adopt_forward_state(f)
        diffs = {n: rs.randn(*f[n].shape).astype(F32) for n in inject}
        gpu.engine.profile_enable(True)
        gd = gpu.backward(diffs)
        n = launches(gpu.engine)
        gpu.engine.profile_enable(False)
        go = cpu.backward(diffs)
        assert rel_l2(gd, go) <= (5e-5 if bf16 else 1e-5), (h, w, rel_l2(gd, go))
        if not bf16:
            err = np.abs(gd[0].astype(np.float64) - go[0])
            bound = _bound(params, f, diffs)
            assert not (err > bound).any(), (h, w, float((err - bound).max()))
        # the pool's backward is the stand-alone pass (an unpooling data gradient would have consumed it), once
        assert n['avepool_bwd'] == (1 if set(inject) & {'pool1', 'conv2_1'} else 0) and n['maxpool_bwd'] == 0, (h, w, n)


# ------------------------------------------------------------------------------------------ C ABI
def test_abi_kind_2_is_an_average_pool_and_unknown_kinds_are_refused():
    lib = capi.load_library()
    params = oracle.he_init_weights(NET, seed=5, bias_std=0.2)
    for kind, want in ((2, 0), (1, 0), (3, 1), (-1, 1)):
        descs = (capi.LayerDesc * 4)()
        names = [l[1].encode() for l in NET]
        for d, l, nm in zip(descs, NET, names):
            d.kind, d.name = (0 if l[0] == 'conv' else kind), nm
            d.cin, d.cout = (l[2], l[3]) if l[0] == 'conv' else (0, 0)
        ctx = ctypes.c_void_p()
        rc = lib.st_create(ctypes.byref(ctx), 0, descs, 4)
        assert rc == want, (kind, rc)
        if rc:
            assert b'unknown kind' in lib.st_last_error()
            continue
        eng = st2.Engine.__new__(st2.Engine)          # the raw context behind the object view
        eng.lib, eng._ctx, eng.topology, eng.precision = lib, ctx, NET if kind == 2 else oracle.tiny_topology(), 'fp32'
        eng.blob_names = [lib.st_blob_name(ctx, i).decode() for i in range(lib.st_num_blobs(ctx))]
        eng._index = {n: i for i, n in enumerate(eng.blob_names)}
        for name, (wt, b) in params.items():
            wt, b = np.ascontiguousarray(wt), np.ascontiguousarray(b)
            capi.check(lib.st_load_conv_weights(ctx, name.encode(), wt.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)))
        x = (np.random.RandomState(0).randn(1, 3, 16, 20) * 40).astype(F32)
        eng.forward(x)
        got = eng.get_blob('pool1')[0]
        conv = eng.get_blob('conv1_2')[0]
        ref = avepool_forward(conv) if kind == 2 else oracle.caffe_net.maxpool_forward(conv)[0]
        assert np.array_equal(got, ref), kind
        eng.close()


# ------------------------------------------------------------------------------------------ mixed topology
@pytest.mark.parametrize('precision,algo', [('fp32', 1), ('fp32', 2), ('bf16', 1)])
def test_mixed_max_and_average_pools(precision, algo):
    """MAX pools 1-2, AVE pools 3-4: everything below pool3 is the all-MAX net's bit for bit (blobs and the gradient of diffs
    injected there); avepool_fwd / avepool_bwd run once per average pool per evaluation and never for a max pool."""
    topo_max = oracle.VGG19_TOPOLOGY
    topo_mix = ave(topo_max, ('pool3', 'pool4'))
    params = oracle.he_init_weights(topo_max, seed=0)
    a, b = model(params, topo_max, precision, algo), model(params, topo_mix, precision, algo)
    x = (np.random.RandomState(4).randn(1, 3, 96, 128) * 40).astype(F32)
    below = ['conv1_1', 'conv1_2', 'pool1', 'conv2_1', 'conv2_2', 'pool2', 'conv3_1', 'conv3_2', 'conv3_3', 'conv3_4']
    fa = a.forward(x, below)
    b.engine.profile_enable(True)
    fb = b.forward(x, below + ['pool3', 'conv5_1'])
    n_fwd = launches(b.engine)
    b.engine.profile_enable(False)
    for n in below:
        assert np.array_equal(fa[n], fb[n]), n
    assert n_fwd['avepool_fwd'] == 2, n_fwd
    rs = np.random.RandomState(5)
    diffs = {n: rs.randn(*fa[n].shape).astype(F32) for n in ('conv3_4', 'pool2', 'conv1_2')}
    assert np.array_equal(a.backward(diffs), b.backward(diffs))
    b.engine.profile_enable(True)
    b.backward({'conv5_1': rs.randn(*b.forward(x, ['conv5_1'])['conv5_1'].shape).astype(F32)})
    n = launches(b.engine)
    b.engine.profile_enable(False)
    assert n['avepool_fwd'] == 2 and n['avepool_bwd'] == 2, n


# ------------------------------------------------------------------------------------------ whole VGG19 with average pools
VGG_WEIGHTS = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
PARAMS4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}


def test_vgg19_ave_gradient_matches_oracle_at_96x128():
    topo = ave(oracle.VGG19_TOPOLOGY)
    params = oracle.he_init_weights(topo, seed=0)
    cpu = oracle.TransferOracle(AveNetOracle(topo, params, full_forward=False))
    dev = st2.StyleTransfer(st2.HipModel(params, topology=topo))
    rs = np.random.RandomState
    content = rs(1).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    style = rs(2).randint(0, 256, (80, 112, 3)).astype(np.uint8)
    init = rs(3).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(VGG_WEIGHTS, PARAMS4)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    assert rel_l2(gd, go) <= 1e-4
    assert np.isclose(ld, lo, rtol=1e-4)
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=1e-3)
    x2 = cpu.input + F32(2.0) * np.sign(go)
    lo, go = cpu.opfunc(x2)
    ld, gd = dev.opfunc(x2)
    assert np.isclose(ld, lo, rtol=1e-4)
    # An average pool hands gradient to every element of its window, also to the small activations next to the ReLU threshold a
    # max pool passes over, so the ReLU sign flips between two correct fp32 forwards (NetOracle.adopt_forward_state) move the
    # end-to-end gradient more than with max pools: 2.5e-4 measured on this second evaluation.  The bar is 1e-4 unless the forwards
    # do disagree on a sign, and the arithmetic is held to 1e-5 on the GPU's own forward state below.
    names = [l[1] for l in topo[:17]]
    full = dev.model.forward(x2, ['data'] + names)
    net = AveNetOracle(topo, params, full_forward=False)
    own = net.forward(x2, ['data'] + names)
    flips = sum(int(np.sum((own[n] > 0) != (full[n] > 0))) for n in names if n.startswith('conv'))
    err = rel_l2(gd, go)
    assert err <= 1e-4 or (flips > 0 and err <= 1e-3), (err, flips)
    net.adopt_forward_state(full)
    rs5 = np.random.RandomState(5)
    diffs = {n: rs5.randn(*full[n].shape).astype(F32) for n in ['conv5_1', 'pool4', 'conv4_2', 'pool3', 'conv3_1', 'pool1', 'conv1_1']}
    assert rel_l2(dev.model.backward(diffs), net.backward(diffs)) <= 1e-5


def test_vgg19_ave_odd_default_size_225x300():
    """Clipped windows at widths 300, 150, 75, 38, 19.  Average pooling is continuous: only ReLU sign flips separate two correct
    forwards, so the bars are those of the max-pool odd-size test (test_gpu_parity), which also allow for arg-max flips."""
    topo = ave(oracle.VGG19_TOPOLOGY)
    params = oracle.he_init_weights(topo, seed=0)
    rs = np.random.RandomState
    content = rs(1).randint(0, 256, (225, 300, 3)).astype(np.uint8)
    style = rs(2).randint(0, 256, (187, 300, 3)).astype(np.uint8)
    init = rs(3).randint(0, 256, (225, 300, 3)).astype(np.uint8)
    weights = {'content': {'conv4_2': 0.08, 'pool3': 0.01},
               'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1, 'pool4': 0.5},
               'deepdream': {'conv5_1': 0.01}}
    cpu = oracle.TransferOracle(AveNetOracle(topo, params, full_forward=False))
    dev = st2.StyleTransfer(st2.HipModel(params, topology=topo))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, PARAMS4)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    assert gd.shape == go.shape == (1, 3, 225, 300)
    assert np.isclose(ld, lo, rtol=1e-5)
    assert rel_l2(gd, go) <= 5e-3
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=2e-3)


def _job(precision, topo, params, optimizer, size=(256, 320)):
    rs = np.random.RandomState
    h, w = size
    st = st2.StyleTransfer(st2.HipModel(params, topology=topo, precision=precision))
    st.set_input(rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8)); st.set_content(rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8))
    st.set_style(rs(2).randint(0, 256, (h - 16, w, 3)).astype(np.uint8)); st.reset()
    st.set_weights(VGG_WEIGHTS, PARAMS4)
    st.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[optimizer]
    st.set_step_size({'adam': 10, 'lbfgs': 1}[optimizer])
    st.reset()
    assert st.start()
    return st


def test_vgg19_ave_lean_bf16_is_bit_identical_to_bf16_full():
    topo = ave(oracle.VGG19_TOPOLOGY)
    params = oracle.he_init_weights(topo, seed=0)
    lean, full = _job('bf16', topo, params, 'adam'), _job('bf16-full', topo, params, 'adam')
    l1, g1 = lean.opfunc()
    l2, g2 = full.opfunc()
    assert l1 == l2 and np.array_equal(g1, g2)
    for _ in range(3):
        i1, t1 = lean.step()
        i2, t2 = full.step()
        assert t1['loss'] == t2['loss'] and np.array_equal(i1, i2)


# ------------------------------------------------------------------------------------------ optimizers
@pytest.mark.parametrize('kind,step,n', [('adam', 10, 5), ('lbfgs', 1, 3)])
def test_optimizer_trajectories_follow_the_ave_oracle(kind, step, n):
    g = load('transfer_tiny.npz')
    topo, net_params, weights, content, style, init = tiny_setup(g)
    topo = ave(topo)
    params = __import__('json').loads(str(g['params_json']))
    cpu = oracle.TransferOracle(AveNetOracle(topo, net_params))
    dev = st2.StyleTransfer(st2.HipModel(net_params, topology=topo))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params)
    cpu.set_optimizer(kind, step)
    dev.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[kind]
    dev.set_step_size(step); dev.reset()
    assert cpu.start() and dev.start()
    for i in range(n):
        ic, tc = cpu.step()
        idv, td = dev.step()
        if kind == 'adam':
            assert np.isclose(td['loss'], tc['loss'], rtol=1e-4 if i == 0 else 5e-3), (i, td['loss'], tc['loss'])
            assert np.mean((idv - ic) ** 2) <= 1.0, i
        else:
            assert np.isclose(td['loss'], tc['loss'], rtol=1e-3), (i, td['loss'], tc['loss'])
            if i == 0:
                assert np.mean((idv - ic) ** 2) <= 1e-2
    assert list(td) == list(tc)


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


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_worker_runs_a_vgg19_prototxt_with_average_pools(tmp_path, precision):
    sys.path.insert(0, os.path.dirname(HERE))
    import messages
    import worker as worker_mod
    with open(os.path.join(HERE, 'golden', 'vgg19.prototxt')) as f:
        text = f.read().replace('pool: MAX', 'pool: AVE')
    path = tmp_path / 'vgg19_ave.prototxt'
    path.write_text(text)
    assert prototxt.read(str(path), average_pools=True) == ave(oracle.VGG19_TOPOLOGY)
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {'prototxt': str(path), 'caffemodel': str(tmp_path / 'absent.npz'), 'weights': 'synthetic',
                             'precision': precision, 'async_iterate': '0', 'pipeline_iterate': '1'}})
    socks = _Socks(messages, pause_after=4)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (64, 80, 3)).astype(np.uint8), rs(2).randint(0, 256, (48, 64, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (64, 80, 3)).astype(np.uint8))
    socks.inbound.extend([messages.SetImages(None, init, content, style, True), messages.SetWeights(VGG_WEIGHTS, PARAMS4),
                          messages.SetOptimizer('adam', 10), messages.StartIteration()])
    wk = worker_mod.Worker(cp['worker'], sock_in=socks, sock_out=socks)
    assert wk.transfer.model.engine.topology == ave(oracle.VGG19_TOPOLOGY)
    wk.run()
    kinds = [type(m).__name__ for m in socks.sent]
    assert kinds[0] == 'WorkerReady' and kinds[-1] == 'Shutdown' and kinds.count('Shutdown') == 1
    assert socks.sent[0].layers == ['data'] + [l[1] for l in oracle.VGG19_TOPOLOGY] and len(socks.sent[0].layers) == 22
    its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
    assert len(its) >= 4 and kinds == ['WorkerReady'] + ['Iterate'] * len(its) + ['Shutdown']
    assert [m.i for m in its] == list(range(1, len(its) + 1))
    assert all(np.isfinite(m.trace['loss']) and m.image.shape == (64, 80, 3) for m in its)
    assert its[-1].trace['loss'] != its[0].trace['loss']


# ------------------------------------------------------------------------------------------ tile-sharded mode
def test_tile_configure_refuses_a_net_with_average_pools():
    eng = st2.Engine(ave(NET))
    rc = eng.lib.st_tile_configure(eng._ctx, 64, 64, 0, 0, 0, 0, 32, 32)
    assert rc == 1 and b'average pool' in eng.lib.st_last_error()
    eng.close()
