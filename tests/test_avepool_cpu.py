"""Average pooling (prototxt ``pool: AVE``) without a GPU: the parser, the topology helpers and the CPU oracle the GPU tests use.

The oracle (tests/avepool_oracle.py) is held to an explicit restatement of Caffe's loop, element by element and bit for bit, and to
torch's CPU ``avg_pool2d(ceil_mode=True)`` -- an independent implementation with the same clipped-window divisor -- forward and
backward."""

import os

import numpy as np
import pytest

import oracle
from oracle.caffe_net import pooled_size
from style_transfer2_amd import caffemodel, prototxt, tiling, weights
from style_transfer2_amd.engine import VGG19_TOPOLOGY
from avepool_oracle import AveNetOracle, avepool_backward, avepool_forward

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(1, 1), (1, 5), (5, 1), (3, 3), (2, 257), (5, 1030), (7, 6)]


def ave_topology(topo=VGG19_TOPOLOGY, which=None):
    """`topo` with its pools (all, or those named in `which`) switched to average pooling."""
    return tuple(('pool', l[1], 'ave') if l[0] == 'pool' and (which is None or l[1] in which) else l for l in topo)


def stock_text():
    with open(os.path.join(HERE, 'golden', 'vgg19.prototxt')) as f:
        return f.read()


def _pool_layer(**fields):
    body = ''.join('        %s: %s\n' % (k, v) for k, v in fields.items())
    return ('layer { name: "data" type: "Input" top: "data" input_param { shape: { dim: 1 dim: 3 dim: 8 dim: 8 } } }\n'
            'layer { bottom: "data" top: "conv1" name: "conv1" type: "Convolution" convolution_param { num_output: 4 pad: 1 kernel_size: 3 } }\n'
            'layer { bottom: "conv1" top: "conv1" name: "relu1" type: "ReLU" }\n'
            'layer { bottom: "conv1" top: "pool1" name: "pool1" type: "Pooling" pooling_param {\n%s} }\n' % body)


# ------------------------------------------------------------------------------------------ prototxt
@pytest.mark.parametrize('method', ['AVE', '1'])
def test_prototxt_parses_average_pools(method):
    text = _pool_layer(pool=method, kernel_size=2, stride=2)
    assert prototxt.parse(text, average_pools=True) == (('conv', 'conv1', 3, 4), ('pool', 'pool1', 'ave'))
    # a caller that has not asked for average pools keeps the MAX-only subset
    with pytest.raises(ValueError, match='MAX pools only'):
        prototxt.parse(text)


@pytest.mark.parametrize('method', ['MAX', '0'])
def test_prototxt_max_pools_stay_two_tuples(method):
    text = _pool_layer(pool=method, kernel_size=2, stride=2)
    assert prototxt.parse(text) == prototxt.parse(text, average_pools=True) == (('conv', 'conv1', 3, 4), ('pool', 'pool1'))


def test_prototxt_stock_vgg19_switched_to_average_pooling():
    text = stock_text()
    assert prototxt.parse(text) == VGG19_TOPOLOGY
    ave = text.replace('pool: MAX', 'pool: AVE')
    assert ave.count('pool: AVE') == 5
    topo = prototxt.parse(ave, average_pools=True)
    assert topo == ave_topology()
    with pytest.raises(ValueError, match='MAX pool'):
        prototxt.parse(ave)
    assert [l[1] for l in topo] == [l[1] for l in VGG19_TOPOLOGY]


def test_prototxt_write_parse_round_trip_mixed():
    for topo in (ave_topology(), ave_topology(which=('pool3', 'pool4')), VGG19_TOPOLOGY,
                 ave_topology(oracle.tiny_topology((8, 16), (2, 1), final_pool=True))):
        assert prototxt.parse(prototxt.write(topo), average_pools=True) == topo
    assert 'pool: AVE' in prototxt.write(ave_topology(which=('pool5',)))
    with pytest.raises(ValueError):
        prototxt.write((('conv', 'conv1', 3, 4), ('pool', 'pool1', 'stochastic')))


@pytest.mark.parametrize('fields', [
    dict(pool='STOCHASTIC', kernel_size=2, stride=2),
    dict(pool='2', kernel_size=2, stride=2),
    dict(pool='AVE', global_pooling='true'),
    dict(pool='AVE', kernel_size=2, stride=2, global_pooling='true'),
    dict(pool='AVE', kernel_size=2, stride=2, pad=1),
    dict(pool='AVE', kernel_size=3, stride=2),
    dict(pool='AVE', kernel_size=2, stride=1),
    dict(pool='AVE', kernel_h=2, kernel_w=2, stride=2),
    dict(pool='MAX', kernel_size=2, stride=2, pad=1),
])
def test_prototxt_refuses_other_pools(fields):
    with pytest.raises(ValueError):
        prototxt.parse(_pool_layer(**fields), average_pools=True)


# ------------------------------------------------------------------------------------------ topology helpers
def test_tile_grid_refuses_average_pools():
    with pytest.raises(ValueError, match='average pool'):
        tiling.TileGrid(512, 512, 1, 2, ave_topology(which=('pool3',)), 13)
    tiling.TileGrid(512, 512, 1, 2, VGG19_TOPOLOGY, 13)           # the max-pool net still tiles


def test_weights_and_caffemodel_accept_average_pool_topologies(tmp_path):
    topo = ave_topology()
    p_ave, p_max = weights.he_normal(topo, seed=3), weights.he_normal(VGG19_TOPOLOGY, seed=3)
    assert list(p_ave) == list(p_max) == [l[1] for l in VGG19_TOPOLOGY if l[0] == 'conv']
    for n in p_max:
        assert np.array_equal(p_ave[n][0], p_max[n][0]) and np.array_equal(p_ave[n][1], p_max[n][1])
    path = str(tmp_path / 'w.npz')
    weights.save_npz(path, p_max)
    got = weights.load_npz(path, topo)
    assert all(np.array_equal(got[n][0], p_max[n][0]) for n in p_max)
    # the same .caffemodel serves both nets: pools carry no blobs
    small = ave_topology(oracle.tiny_topology((8, 16), (2, 1), final_pool=True))
    params = weights.he_normal(small, seed=1, bias_std=0.1)
    cm = str(tmp_path / 'net.caffemodel')
    caffemodel.write_caffemodel(cm, params)
    got = caffemodel.vgg_params(caffemodel.read_caffemodel(cm), small)
    assert list(got) == list(params)
    assert all(np.array_equal(got[n][0], params[n][0]) and np.array_equal(got[n][1], params[n][1]) for n in params)


# ------------------------------------------------------------------------------------------ the oracle's pool
def _restated_forward(x):
    """Caffe PoolingLayer::Forward_cpu, AVE, pad 0, written as its loops."""
    c, h, w = x.shape
    ho, wo = pooled_size(h), pooled_size(w)
    top = np.zeros((c, ho, wo), F32)
    for ch in range(c):
        for py in range(ho):
            for px in range(wo):
                r0, c0 = 2 * py, 2 * px
                r1, c1 = min(r0 + 2, h), min(c0 + 2, w)
                t = F32(0)
                for r in range(r0, r1):
                    for cc in range(c0, c1):
                        t = F32(t + x[ch, r, cc])
                top[ch, py, px] = F32(t / F32((r1 - r0) * (c1 - c0)))
    return top


def _ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F32)).astype(np.float64)


@pytest.mark.parametrize('h,w', SHAPES)
def test_oracle_avepool_is_caffe_bit_for_bit_and_matches_torch(h, w):
    torch = pytest.importorskip('torch')
    rs = np.random.RandomState(h * 1000 + w)
    x = np.maximum(rs.randn(3, h, w), -0.2).astype(F32)
    got = avepool_forward(x)
    ref = _restated_forward(x) if h * w <= 5000 else None
    if ref is not None:
        assert got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # torch CPU: same clipped divisor (count_include_pad is moot at pad 0)
    xt = torch.from_numpy(x[None].copy()).requires_grad_(True)
    yt = torch.nn.functional.avg_pool2d(xt, 2, 2, ceil_mode=True)
    assert yt.shape[2:] == got.shape[1:]
    assert _ulps(got, yt.detach().numpy()[0]).max() <= 1
    dy = rs.randn(*got.shape).astype(F32)
    yt.backward(torch.from_numpy(dy[None].copy()))
    dx = avepool_backward(dy, x.shape)
    assert dx.shape == x.shape
    assert _ulps(dx, xt.grad.numpy()[0]).max() <= 1


def test_oracle_avepool_hand_case():
    x = np.arange(25, dtype=F32).reshape(1, 5, 5)
    y = avepool_forward(x)
    assert y[0, 0, 2] == (4 + 9) / 2 and y[0, 2, 0] == (20 + 21) / 2 and y[0, 2, 2] == 24 and y[0, 0, 0] == (0 + 1 + 5 + 6) / 4
    dx = avepool_backward(np.ones((1, 3, 3), F32), x.shape)
    assert dx[0, 0, 0] == 0.25 and dx[0, 0, 4] == 0.5 and dx[0, 4, 0] == 0.5 and dx[0, 4, 4] == 1.0


def test_ave_net_oracle_backward_is_the_adjoint_of_its_forward():
    """<backward(d), dx> == <d, d forward / dx . dx> on a tiny conv -> ave pool -> conv net: the chain rules (ReLU mask, unmasked
    injection) are NetOracle's, the pool's adjoint is its own."""
    topo = (('conv', 'conv1_1', 3, 8), ('pool', 'pool1', 'ave'), ('conv', 'conv2_1', 8, 8))
    params = oracle.he_init_weights(topo, seed=0, bias_std=0.1)
    net = AveNetOracle(topo, params)
    rs = np.random.RandomState(0)
    x = (rs.rand(1, 3, 9, 11) * 200 - 100).astype(np.float64)
    f = net.forward(x.astype(F32))
    # (a diff injected at a conv blob enters that conv's backward unmasked -- worker.py's ranged backward -- so it is given masked)
    d = {'conv2_1': (rs.randn(*f['conv2_1'].shape) * (f['conv2_1'] > 0)).astype(F32), 'pool1': rs.randn(*f['pool1'].shape).astype(F32)}
    g = net.backward(d).astype(np.float64)
    dx = rs.randn(*x.shape) * 1e-2
    fp, fm = net.forward((x + dx).astype(F32)), net.forward((x - dx).astype(F32))
    lin = sum(float(np.sum(d[n].astype(np.float64) * (fp[n].astype(np.float64) - fm[n].astype(np.float64)) / 2)) for n in d)
    assert np.isclose(float(np.sum(g * dx)), lin, rtol=2e-2)
    # a max-pool net through the subclass is NetOracle bit for bit
    mtopo = (('conv', 'conv1_1', 3, 8), ('pool', 'pool1'), ('conv', 'conv2_1', 8, 8))
    a, b = AveNetOracle(mtopo, params), oracle.NetOracle(mtopo, params)
    fa, fb = a.forward(x.astype(F32)), b.forward(x.astype(F32))
    assert all(np.array_equal(fa[n], fb[n]) for n in fa)
    assert np.array_equal(a.backward(d), b.backward(d))
