"""Every conv path, whole VGG19 and the fused image pass at tiny and thin image sizes: 1 x 1, 1 x N, N x 1, widths just past a
tile edge.  At these sizes a Winograd 4 x 32 tile or a bf16 64 x 512 tile is almost all padding, split-K divides a handful of
pixels, the Gram sums over hw = 1 .. 4, a pool has one clipped window and the image pass wraps its halo onto the tile itself.
The reference sets no minimum size (a 10:1 panorama at the default 300 px is 30 x 300; conv5_1 then has 2 rows).

Oracle: the CPU restatement (oracle.caffe_net, oracle.TransferOracle), fed with the GPU's own blobs where one layer is checked.
Besides each family's rel-L2 bar every conv output is held to the worst-case summation bound at EVERY element:
    |gpu - ref| <= 2 * K * 2^-24 * M + tiny,   M = the same conv on absolute values, K = the number of products summed,
which a dropped or doubled tap at a border pixel breaks however large the rest of the tensor is.  (For the Winograd kernels the
bound is not a proof -- the transforms re-associate the sum -- but at random data their error is expected to be ~sqrt(K) times
below it.)  Every case asserts which kernel class ran, or the fallback its id names."""

import collections
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle.caffe_net import bf16_round, conv3x3_backward_data, conv3x3_forward, maxpool_forward
import style_transfer2_amd as st2
from helpers import check_trace, rel_l2

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24
TINY = 1e-30
HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (1, 5), (2, 257), (3, 513), (1, 600), (600, 1), (5, 1030)]
PAIRS = [(3, 64), (64, 64), (64, 128), (256, 256), (512, 512)]

# kernel classes of engine.profile_read()
FWD_F32, FWD_WINO, FWD_SPLIT, FWD_BF16 = 'conv3x3_fwd_mfma_f32', 'conv3x3_fwd_wino_f32', 'conv3x3_fwd_wino_split_bf16x6', 'conv3x3_fwd_mfma_bf16'
DG_F32, DG_WINO, DG_SPLIT, DG_BF16 = 'conv3x3_dgrad_mfma_f32', 'conv3x3_dgrad_wino_f32', 'conv3x3_dgrad_wino_split_bf16x6', 'conv3x3_dgrad_mfma_bf16'


# ------------------------------------------------------------------------------------------ which kernel the engine must pick
def _wino_ok(k, m):
    return k >= 8 and k % 8 == 0 and m >= 48


def _split_ok(k, m, w):
    return k % 16 == 0 and m % 64 == 0 and w % 4 == 0


def fwd_class(path, cin, cout, w):
    """Forward class of one conv (cin -> cout, output width w) on path 'direct' | 'wino' | 'split' | 'bf16'."""
    if cin == 3:
        return FWD_F32                      # conv1_1: the fp32 kernel (or, bf16 path, the split-operand first-layer kernel)
    if path == 'bf16':
        return FWD_BF16 if cin % 8 == 0 else FWD_F32
    if path == 'direct' or not _wino_ok(cin, cout):
        return FWD_F32
    return FWD_SPLIT if path == 'split' and _split_ok(cin, cout, w) else FWD_WINO


def dgrad_class(path, cin, cout, w):
    """Data-gradient class of one conv: the transposed problem K = cout, M = cin."""
    if cin == 3:
        return DG_F32                       # conv1_1's small-M kernels (strip walker / tile / VALU; bf16 operands on the bf16 path)
    if path == 'bf16':
        return DG_BF16 if cout % 8 == 0 else DG_F32
    if path == 'direct' or not _wino_ok(cout, cin):
        return DG_F32
    return DG_SPLIT if path == 'split' and _split_ok(cout, cin, w) else DG_WINO


def conv_launches(engine):
    return collections.Counter({k: v['launches'] for k, v in engine.profile_read().items() if k.startswith('conv3x3_')})


def make_model(params, topo, path, precision=None):
    m = st2.HipModel(params, topology=topo, precision=precision or ('bf16' if path == 'bf16' else 'fp32'))
    if path == 'split':
        m.engine.set_conv_algo(2)
    elif path == 'direct':
        m.engine.set_conv_algo(False)
    return m


# ------------------------------------------------------------------------------------------ references and bounds
def conv_ref(x, w, b, bf16):
    """relu(conv(x)) and its element-wise bound on the path's operands (bf16: x and w rounded, products exact in fp32)."""
    if bf16:
        x, w = bf16_round(x), bf16_round(w)
    ref = np.maximum(conv3x3_forward(x, w, b), 0)
    mag = conv3x3_forward(np.abs(x), np.abs(w), np.abs(b))
    k = 9 * x.shape[0] + 1                                          # + the bias
    return ref, 2.0 * k * U * mag.astype(np.float64) + TINY


def assert_within(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref)
    bad = err > bound
    assert not bad.any(), '%s: %d elements beyond the summation bound, worst %.3g > %.3g at %s' % (
        what, int(bad.sum()), float(err[bad].max()), float(bound[bad][np.argmax(err[bad])]), np.argwhere(bad)[0])


def dgrad_bound(convs, masks, dy):
    """Bound of the data gradient through `convs` (top first: [(w, bf16)], the ReLU masks of the blobs between them): the chain of
    backward convs on absolute values, 2 * (sum of the K's) * 2^-24 times it (first order in the rounding errors)."""
    m, k = np.abs(dy[0]), 0
    for i, (w, bf16) in enumerate(convs):
        if i:
            m = m * masks[i - 1]
        w = bf16_round(w) if bf16 else w
        m = conv3x3_backward_data(m.astype(F32), np.abs(w))
        k += 9 * w.shape[0]
    return 2.0 * (k + 2) * U * m.astype(np.float64) + TINY


def adopt_bf16_roundings(got, ref, g2, bound2, w1r):
    """bf16 path, two convs: conv1_1's data gradient reads the diff of conv1_2's data gradient rounded to bf16.  Where that diff lies
    within its own rounding bound of a bf16 rounding midpoint, the GPU and the oracle may round it to different neighbours (one bf16
    ulp, 2^-8 relative) -- the data-gradient counterpart of a ReLU flip.  Those elements are few (~1e-6 / 2^-8); for each, take the
    neighbour the GPU's gradient agrees with (as NetOracle.adopt_forward_state takes its ReLU masks), so that the comparison holds
    the arithmetic to the bar and not the rounding decisions."""
    lo, hi = bf16_round((g2 - bound2).astype(F32)), bf16_round((g2 + bound2).astype(F32))
    r = bf16_round(g2.astype(F32))
    c, h, w = ref.shape
    refp = np.zeros((c, h + 2, w + 2)); refp[:, 1:-1, 1:-1] = ref
    gotp = np.zeros_like(refp); gotp[:, 1:-1, 1:-1] = np.asarray(got, np.float64).reshape(ref.shape)
    valid = np.zeros_like(refp); valid[:, 1:-1, 1:-1] = 1
    n = 0
    for k, y, x in np.argwhere(lo != hi):
        alt = hi[k, y, x] if r[k, y, x] == lo[k, y, x] else lo[k, y, x]
        # col2im of one element: dx[ci, y + ky - 1, x + kx - 1] += w[k, ci, ky, kx] * dy[k, y, x]  (padded coordinates: + 1)
        win = (slice(None), slice(y, y + 3), slice(x, x + 3))
        step = (float(alt) - float(r[k, y, x])) * w1r[k].astype(np.float64) * valid[win]
        if np.sum((gotp[win] - refp[win] - step) ** 2) < np.sum((gotp[win] - refp[win]) ** 2):
            refp[win] += step
            n += 1
    ref = refp[:, 1:-1, 1:-1]
    return ref, n


# ------------------------------------------------------------------------------------------ A. one conv layer at edge shapes
FAMILIES = {                    # id -> (path, env)
    'direct': ('direct', {'ST2_WINO': '0'}),
    'wino': ('wino', {}),
    'wino-cfg0': ('wino', {'ST2_WINO_CFG': '0'}),
    'wino-cfg8': ('wino', {'ST2_WINO_CFG': '8'}),
    'split': ('split', {}),
    'bf16': ('bf16', {}),
    'bf16-cfg3': ('bf16', {'ST2_CONV16_CFG': '3'}),
}
BARS = {'direct': 1e-5, 'wino': 1e-5, 'split': 2e-6, 'bf16': 3e-5}
DG_BARS = {'direct': 3e-5, 'wino': 3e-5, 'split': 6e-6, 'bf16': 5e-5}


def _heavy(pair, shape):
    return pair[0] * pair[1] * shape[0] * shape[1] > 100e6       # the oracle's cost, not the kernel's


def _layer_cases(n_families):
    """Every family sees every shape once and every channel pair at least once (rotated; a pair whose oracle would be slow moves on to the next)."""
    cases = []
    for f in range(n_families):
        for i, shape in enumerate(SHAPES):
            j = (i + f) % len(PAIRS)
            while _heavy(PAIRS[j], shape):
                j = (j + 1) % len(PAIRS)
            cases.append((f, PAIRS[j], shape))
    return cases


def _fallback_tag(path, cin, cout, w):
    f, d = fwd_class(path, cin, cout, w), dgrad_class(path, cin, cout, w)
    want_f = {'direct': FWD_F32, 'wino': FWD_WINO, 'split': FWD_SPLIT, 'bf16': FWD_BF16}[path]
    tags = []
    if f != want_f:
        tags.append('fwd-falls-back-to-' + f)
    if cin != 3 and d != {'direct': DG_F32, 'wino': DG_WINO, 'split': DG_SPLIT, 'bf16': DG_BF16}[path]:
        tags.append('dgrad-falls-back-to-' + d)
    return '-'.join(tags)


def _layer_params():
    names = list(FAMILIES)
    out = []
    for f, (cin, cout), (h, w) in _layer_cases(len(names)):
        path = FAMILIES[names[f]][0]
        tag = _fallback_tag(path, cin, cout, w)
        out.append(pytest.param(names[f], cin, cout, h, w, id='%s-%d-%d-%dx%d%s' % (names[f], cin, cout, h, w, '-' + tag if tag else '')))
    return out


def run_layer_case(family, path, cin, cout, h, w):
    """Forward and data gradient of conv1_2 (cin -> cout; cin == 3: conv1_1 alone) on `path`, against the oracle fed with the GPU's
    own blobs: the family's rel-L2 bar, the element-wise summation bound, the kernel classes that ran."""
    topo = (('conv', 'conv1_1', 3, cout),) if cin == 3 else (('conv', 'conv1_1', 3, cin), ('conv', 'conv1_2', cin, cout))
    params = oracle.he_init_weights(topo, seed=cin + cout + h, bias_std=0.2)
    last = topo[-1][1]
    gpu = make_model(params, topo, path)
    bf16 = path == 'bf16'
    rng = np.random.RandomState(h * 1000 + w)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)
    gpu.engine.profile_enable(True)
    f = gpu.forward(x, [n for _, n, _, _ in topo])
    fwd = conv_launches(gpu.engine)
    below = x[0] if cin == 3 else f['conv1_1'][0]
    wgt, b = params[last]
    ref, bound = conv_ref(below, wgt, b, bf16 and cin != 3)
    got = f[last][0]
    bar = BARS[path] if cin <= 256 else max(BARS[path], 3e-5)
    if path == 'split' and fwd_class(path, cin, cout, w) != FWD_SPLIT:
        bar = 1e-5                                                   # fallen back to the IEEE-fp32 Winograd kernel: its bar
    assert_within(got, ref, bound, '%s forward' % family)
    assert rel_l2(got, ref) <= bar, (family, rel_l2(got, ref))
    want = collections.Counter([fwd_class(path, c_in, c_out, w) for _, _, c_in, c_out in topo])
    assert fwd == want, (family, fwd, want)
    # data gradient on the adopted forward state (same ReLU masks: the backward arithmetic only)
    cpu = oracle.NetOracle(topo, params, operands='bf16' if bf16 else 'fp32')
    cpu.forward(x)
    cpu.adopt_forward_state(f)
    d = rng.randn(*f[last].shape).astype(F32)
    gpu.engine.profile_enable(True)
    gg = gpu.backward({last: d})
    bwd = conv_launches(gpu.engine)
    gc = cpu.backward({last: d})[0].astype(np.float64)
    if bf16 and cin != 3:
        w2r, w1r = bf16_round(params[last][0]), bf16_round(params['conv1_1'][0])
        mask = f['conv1_1'][0] > 0
        g2 = conv3x3_backward_data(bf16_round(d[0]), w2r) * mask
        gc, _ = adopt_bf16_roundings(gg[0], gc, g2, dgrad_bound([(params[last][0], True)], [], d) * mask, w1r)
    dbar = DG_BARS[path] if cin <= 256 else max(DG_BARS[path], 9e-5)
    if path == 'split' and dgrad_class(path, cin, cout, w) != DG_SPLIT:
        dbar = 3e-5
    convs = [(params[n][0], bf16 and params[n][0].shape[0] % 8 == 0) for _, n, _, _ in reversed(topo)]
    masks = [f['conv1_1'][0] > 0] if cin != 3 else []
    assert_within(gg[0], gc, dgrad_bound(convs, masks, d), '%s data gradient' % family)
    assert rel_l2(gg[0], gc) <= dbar, (family, rel_l2(gg[0], gc))
    want = collections.Counter([dgrad_class(path, c_in, c_out, w) for _, _, c_in, c_out in topo])
    assert bwd == want, (family, bwd, want)
    gpu.engine.close()


@pytest.mark.parametrize('family,cin,cout,h,w', _layer_params())
def test_conv_layer_at_edge_shape(family, cin, cout, h, w, monkeypatch):
    path, env = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_layer_case(family, path, cin, cout, h, w)


def _child_forced_direct_cfg():
    """Body of the child process of test_direct_conv_forced_tile_config_at_edge_shapes (ST2_CONV_CFG is read once per process)."""
    for f, (cin, cout), (h, w) in _layer_cases(1):
        run_layer_case('direct-cfg7', 'direct', cin, cout, h, w)
    print('forced-cfg child ok')


def test_direct_conv_forced_tile_config_at_edge_shapes():
    """The direct fp32 kernel with its smallest tile forced (ST2_CONV_CFG=7: 64 channels x 2 x 32 pixels) at every edge shape.  The
    variable is latched at the first launch of a process, so the cases run in a fresh child process."""
    env = dict(os.environ, ST2_CONV_CFG='7', ST2_WINO='0', ST2_NO_HEARTBEAT='1')
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_gpu_edge_sizes as t; t._child_forced_direct_cfg()' % (os.path.dirname(HERE), HERE)
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'forced-cfg child ok' in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------ A'. conv1_1 (3 -> 64)
@pytest.mark.parametrize('h,w', SHAPES, ids=['%dx%d' % s for s in SHAPES])
@pytest.mark.parametrize('kind', ['fp32', 'bf16-split', 'bf16-nosplit'])
def test_first_conv_forward_and_data_gradient_kernels_at_edge_shape(kind, h, w, monkeypatch):
    """conv1_1 forward: the fp32 kernel, the bf16 path's split-operand kernel (ST2_FIRST_SPLIT on) and its fp32-matrix-core stand-in
    (off), all held to the fp32-operand restatement.  Data gradient: fp32 -- the strip walker (default), the tile kernel
    (ST2_DGRAD_FIRST=1) and the VALU kernels (=0); bf16 -- the bf16 strip walker against the tile kernel (ST2_DGRAD_FIRST_STRIP=0)."""
    topo = (('conv', 'conv1_1', 3, 64),)
    params = oracle.he_init_weights(topo, seed=64 + h + w, bias_std=0.3)
    wgt, b = params['conv1_1']
    rng = np.random.RandomState(h * 7 + w)
    x = ((rng.randint(0, 256, (1, 3, h, w)).astype(F32) - F32(120.0)) + rng.rand(1, 3, h, w).astype(F32))     # image-like
    precision = 'fp32' if kind == 'fp32' else 'bf16'
    monkeypatch.setenv('ST2_FIRST_SPLIT', '0' if kind == 'bf16-nosplit' else '1')
    gpu = st2.HipModel(params, topology=topo, precision=precision)
    gpu.engine.profile_enable(True)
    f = gpu.forward(x, ['conv1_1'])
    assert conv_launches(gpu.engine) == collections.Counter({FWD_F32: 1})
    ref, bound = conv_ref(x[0], wgt, b, False)
    err = rel_l2(f['conv1_1'][0], ref)
    assert err <= (3e-7 if kind == 'bf16-split' else 1e-5), err
    assert_within(f['conv1_1'][0], ref, bound, 'conv1_1 forward')
    cpu = oracle.NetOracle(topo, params, operands='bf16' if precision == 'bf16' else 'fp32')
    cpu.forward(x)
    cpu.adopt_forward_state(f)
    diffs = [{'conv1_1': rng.randn(1, 64, h, w).astype(F32)}, {'conv1_1': rng.randn(1, 64, h, w).astype(F32), 'data': rng.randn(*x.shape).astype(F32)}]
    variants = [('ST2_DGRAD_FIRST', None), ('ST2_DGRAD_FIRST', '1'), ('ST2_DGRAD_FIRST', '0')] if precision == 'fp32' else \
        [('ST2_DGRAD_FIRST_STRIP', None), ('ST2_DGRAD_FIRST_STRIP', '0')]
    bf16 = precision == 'bf16'
    for dd in diffs:
        want = cpu.backward(dd)
        bound = dgrad_bound([(wgt, bf16)], [], dd['conv1_1'])
        got = {}
        for var, val in variants:
            if val is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, val)
            gpu.engine.profile_enable(True)
            got[val] = gpu.backward(dd)
            assert conv_launches(gpu.engine) == collections.Counter({DG_F32: 1}), (var, val)
            e = rel_l2(got[val], want)
            assert e <= (5e-5 if bf16 else 2e-6), (var, val, sorted(dd), e)
            extra = 4 * U * (np.abs(want[0]) + np.abs(dd['data'][0])) if 'data' in dd else 0      # the injection's add
            assert_within(got[val][0], want[0].astype(np.float64), bound + extra, 'conv1_1 data gradient %s=%s %s' % (var, val, sorted(dd)))
        if precision == 'fp32':
            assert np.array_equal(got[None], got['1']), 'the strip walker sums in the tile kernel\'s order'
    gpu.engine.close()


# ------------------------------------------------------------------------------------------ B. whole VGG19 at tiny sizes
VGG_SIZES = [(1, 1), (2, 3), (8, 8), (16, 16), (17, 15), (5, 300), (300, 5), (1, 257), (33, 65)]
STYLE_SIZES = [(1, 1), (7, 5), (16, 16)]
VGG_PATHS = ['wino', 'direct', 'split', 'bf16']          # fp32 auto, fp32 ST2_WINO=0, conv algorithm 2, precision='bf16'
VGG_WEIGHTS = {'content': {'conv4_2': 0.08, 'pool3': 0.01},
               'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1, 'pool4': 0.5},
               'deepdream': {'conv5_1': 0.01}}
TOPO17 = oracle.VGG19_TOPOLOGY[:17]                      # conv1_1 .. conv5_1
_VGG_PARAMS = []


def vgg_params():
    if not _VGG_PARAMS:
        _VGG_PARAMS.append(oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0))
    return _VGG_PARAMS[0]


def _vgg_model(path, monkeypatch):
    if path == 'direct':
        monkeypatch.setenv('ST2_WINO', '0')
    m = st2.HipModel(vgg_params(), precision='bf16' if path == 'bf16' else 'fp32')
    if path == 'split':
        m.engine.set_conv_algo(2)
    return m


@pytest.mark.parametrize('path', VGG_PATHS)
@pytest.mark.parametrize('h,w', VGG_SIZES, ids=['%dx%d' % s for s in VGG_SIZES])
def test_vgg19_at_tiny_and_thin_size(h, w, path, monkeypatch):
    """VGG19 to conv5_1 at a size where the deep layers are 1 x 1, 1 x N or N x 1: (1) every conv blob against the oracle primitive
    fed with the GPU's blob below it (the bars of the single-layer cases and the element-wise bound), every pool blob bit for bit,
    the Gram of every style layer; (2) the ranged backward with injections at a conv, a pool and data; (3) the objective twice
    (norm capture, frozen norms) against TransferOracle; (4) one Adam and one L-BFGS step."""
    i = VGG_SIZES.index((h, w))
    sh, sw = STYLE_SIZES[i % len(STYLE_SIZES)]
    params = vgg_params()
    bf16 = path == 'bf16'
    rs = np.random.RandomState
    content, style, init = (rs(1 + i).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2 + i).randint(0, 256, (sh, sw, 3)).astype(np.uint8),
                            rs(3 + i).randint(0, 256, (h, w, 3)).astype(np.uint8))
    gpu = _vgg_model(path, monkeypatch)
    net = oracle.NetOracle(oracle.VGG19_TOPOLOGY, params, full_forward=False, operands='bf16' if bf16 else 'fp32')
    x = net.preprocess(init)
    names = ['data'] + [l[1] for l in TOPO17]
    # (1) forward, layer by layer
    gpu.engine.profile_enable(True)
    f = gpu.forward(x, names)
    fwd = conv_launches(gpu.engine)
    want_f, want_d = collections.Counter(), collections.Counter()
    for k, (kind, name, *ch) in enumerate(TOPO17):
        below = f[names[k]][0]
        if kind == 'pool':
            assert np.array_equal(f[name][0], maxpool_forward(below)[0]), (name, h, w)
            continue
        cin, cout = ch
        wgt, b = params[name]
        cls = fwd_class(path, cin, cout, below.shape[2])
        want_f[cls] += 1
        want_d[dgrad_class(path, cin, cout, below.shape[2])] += 1
        ref, bound = conv_ref(below, wgt, b, bf16 and cls == FWD_BF16)
        bar = {FWD_F32: 1e-5, FWD_WINO: 1e-5, FWD_SPLIT: 2e-6, FWD_BF16: 3e-5}[cls]
        if cin > 256:
            bar = max(bar, 3e-5)
        if np.linalg.norm(ref) > 0:
            assert rel_l2(f[name][0], ref) <= bar, (name, cls, rel_l2(f[name][0], ref))
        assert_within(f[name][0], ref, bound, '%s %s (%s)' % (path, name, cls))
    assert fwd == want_f, (fwd, want_f)
    for name in VGG_WEIGHTS['style']:
        g = gpu.engine.gram(name)
        ref = oracle.gram(f[name])                    # (st_gram contracts the fp32 blob on either path)
        if np.linalg.norm(ref) > 0:
            assert rel_l2(g, ref) <= 1e-5, (name, rel_l2(g, ref))
        else:
            assert not g.any(), name
    # (2) backward on the GPU's forward state, injections at a conv, a pool and data
    net.forward(x, names[1:])
    net.adopt_forward_state(f)
    r2 = rs(5 + i)
    diffs = {n: r2.randn(*f[n].shape).astype(F32) for n in ('conv5_1', 'pool4', 'conv3_2', 'pool1', 'data')}
    gpu.engine.profile_enable(True)
    gg = gpu.backward(diffs)
    assert conv_launches(gpu.engine) == want_d, (conv_launches(gpu.engine), want_d)
    err = rel_l2(gg, net.backward(diffs))
    # bf16: sixteen convs deep every diff is rounded to bf16 sixteen times and two correct implementations round a growing share of
    # its elements the other way -- the whole-network bar of _vgg_pair (tests/test_gpu_bf16.py); six convs deep, the chain bar of
    # test_bf16_chain_with_pools_and_injections
    assert err <= {'wino': 1e-5, 'direct': 1e-5, 'split': 6e-6, 'bf16': 5e-2}[path], err
    if bf16:
        shallow = {n: diffs[n] for n in ('conv3_2', 'pool1', 'data')}
        err = rel_l2(gpu.backward(shallow), net.backward(shallow))
        assert err <= 2e-3, err
    gpu.engine.profile_enable(False)
    # (3) end to end, twice: norm capture, then frozen norms
    params4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 1.5 if i % 2 else 2}
    cpu = oracle.TransferOracle(oracle.NetOracle(oracle.VGG19_TOPOLOGY, params, full_forward=False, operands='bf16' if bf16 else 'fp32'))
    dev = st2.StyleTransfer(gpu)
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(VGG_WEIGHTS, params4)
    for ev in range(2):
        lo, go = cpu.opfunc(cpu.input)
        ld, gd = dev.opfunc()
        assert gd.shape == go.shape == (1, 3, h, w)
        if bf16:
            assert np.isclose(ld, lo, rtol=1e-2), (ev, ld, lo)
            assert rel_l2(gd, go) <= 5e-2, (ev, rel_l2(gd, go))
            check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=5e-2,
                        skip=('time',) + tuple(k for k in cpu.traces[-1].data if k.endswith('_grad')))
        else:
            assert np.isclose(ld, lo, rtol=1e-5), (ev, ld, lo)
            assert rel_l2(gd, go) <= 5e-3, (ev, rel_l2(gd, go))
            e = np.abs(gd - go)[0].max(0)
            assert np.mean(e > 1e-3 * np.abs(go).max()) <= 0.02
            check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=2e-3)
    # (4) one Adam step, one L-BFGS step
    for kind, step in (('adam', 10), ('lbfgs', 1)):
        cpu.set_optimizer(kind, step)
        dev.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[kind]
        dev.set_step_size(step)
        for st in (cpu, dev):
            st.set_input(init); st.reset()
        assert cpu.start() and dev.start()
        _, tc = cpu.step()
        _, td = dev.step()
        assert np.isclose(td['loss'], tc['loss'], rtol=2e-2 if bf16 else 1e-3), (kind, td['loss'], tc['loss'])
        # the iterates compared in NCHW: the reference's deprocess (worker.py:68-71, np.squeeze) drops a unit height or width
        mse = float(np.mean((dev.engine.get_input_nchw().astype(np.float64) - cpu.input) ** 2))
        assert mse <= (4.0 if bf16 else 1.0), (kind, mse)
    gpu.engine.close()


# ------------------------------------------------------------------------------------------ C. the fused image pass at its tile edges
IP_SIZES = [(hh, ww) for hh in (1, 2, 3, 5) for ww in (1, 255, 256, 257, 513)]
IMAGE_ONLY = {'content': {'conv1_1': 0.0}, 'style': {}, 'deepdream': {}}


@pytest.mark.parametrize('powers', [(6, 2), (2.5, 1.25)], ids=['integral', 'fractional'])
@pytest.mark.parametrize('h,w', IP_SIZES, ids=['%dx%d' % s for s in IP_SIZES])
def test_image_pass_at_tile_edges(h, w, powers):
    """image_pass_k stages 4 x 256 tiles with a one-pixel circular neighbourhood: heights below and at the tile height (the halo
    rows wrap onto the tile itself), widths at and one past the tile edge.  Image terms only (no layer is visited): loss, gradient
    and trace of an evaluation, then the iterate and Adam's m and v after three steps, element by element."""
    topo = oracle.tiny_topology((8, 16), (2, 1))
    params = oracle.he_init_weights(topo, seed=0, bias_std=0.1)
    rs = np.random.RandomState(h * 1000 + w)
    content, style, init = (rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(0, 256, (3, 4, 3)).astype(np.uint8),
                            rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
    params4 = {'p': 50, 'p_power': powers[0], 'tv': 5, 'tv_power': powers[1]}
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, params))
    dev = st2.StyleTransfer(st2.HipModel(params, topology=topo))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(IMAGE_ONLY, params4)
    dev.engine.profile_enable(True)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    classes = dev.engine.profile_read()
    assert 'image_pass' in classes and not any(k.startswith(('conv3x3_', 'gram_', 'maxpool_')) for k in classes), sorted(classes)
    dev.engine.profile_enable(False)
    assert np.isclose(ld, lo, rtol=1e-5), (ld, lo)
    assert np.allclose(gd, go, rtol=1e-5, atol=1e-6 * np.abs(go).max()), float(np.abs(gd - go).max())
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=1e-4)
    cpu.set_optimizer('adam', 10)
    dev.optimizer_cls = st2.AdamOptimizer
    dev.set_step_size(10)
    for st in (cpu, dev):
        st.set_input(init); st.reset()
    assert cpu.start() and dev.start()
    for _ in range(3):
        _, tc = cpu.step()
        _, td = dev.step()
        assert np.isclose(td['loss'], tc['loss'], rtol=1e-5), (td['loss'], tc['loss'])
    xd = dev.engine.get_input_nchw()          # NCHW: the reference's deprocess (np.squeeze) drops a unit height or width
    assert np.allclose(xd, cpu.input, rtol=1e-6, atol=1e-3), float(np.abs(xd - cpu.input).max())
    m, v, i1, i2 = dev.engine.adam_get_state()
    opt = cpu.optimizer
    assert (i1, i2) == (opt.g1.items, opt.g2.items) == (3, 3)
    assert np.allclose(m, opt.g1.mean, rtol=1e-4, atol=1e-6 * np.abs(opt.g1.mean).max()), float(np.abs(m - opt.g1.mean).max())
    assert np.allclose(v, opt.g2.mean, rtol=1e-4, atol=1e-6 * np.abs(opt.g2.mean).max()), float(np.abs(v - opt.g2.mean).max())
    dev.engine.close()
