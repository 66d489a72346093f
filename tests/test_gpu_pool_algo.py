"""Average pools fused into the bf16 conv launches (st_set_pool_algo(ctx, 1); csrc/conv3x3_mfma_bf16.hip: forward epilogue kind 6 and
the AVE branch of the general epilogue, the UNPOOL builds that read the sign map, avepool_bwd_map16_k) against the stand-alone
passes (pool_algo 0), which tests/test_gpu_avepool.py holds to the oracle.  Same additions in the same order and power-of-two
factors: everything is compared with np.array_equal.

The tile of a bf16 conv is chosen from the number of workgroups (conv16_resolve): at the small sizes of these tests the default is the
64 x 128 tile, whose waves hold one row each and which therefore pools nothing, max or average.  The cases force the tile they are about
with ST2_CONV16_CFG (0: 64 x 256, 1: 128 x 128, 3: 64 x 512), for both values of the switch alike; one case runs at the smallest size
at which the default selection takes a pooling tile on its own."""

import collections
import configparser
import os
import pickle
import sys
from collections import deque

import numpy as np
import pytest

import oracle
from oracle.caffe_net import bf16_round
import style_transfer2_amd as st2
from style_transfer2_amd import capi, prototxt
import exact_oracle as eo

pytestmark = pytest.mark.gpu
F32 = np.float32
F64 = np.float64
HERE = os.path.dirname(os.path.abspath(__file__))

NET = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 64), ('pool', 'pool1', 'ave'), ('conv', 'conv2_1', 64, 64))
NET128 = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 128), ('conv', 'conv1_3', 128, 128), ('pool', 'pool1', 'ave'),
          ('conv', 'conv2_1', 128, 64))
NET256 = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 128), ('conv', 'conv1_3', 128, 256), ('conv', 'conv1_4', 256, 256),
          ('pool', 'pool1', 'ave'), ('conv', 'conv2_1', 256, 64))
PARAMS4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
VGG_WEIGHTS = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
FWD16, DG16 = 'conv3x3_fwd_mfma_bf16', 'conv3x3_dgrad_mfma_bf16'


def ave(topo, which=None):
    return tuple(('pool', l[1], 'ave') if l[0] == 'pool' and (which is None or l[1] in which) else l for l in topo)


def model(params, topo, precision, algo):
    m = st2.HipModel(params, topology=topo, precision=precision)
    m.engine.set_conv_algo(algo)
    return m


def launches(engine):
    return collections.Counter({k: v['launches'] for k, v in engine.profile_read().items()})


def images(h, w, style_hw=None):
    rs = np.random.RandomState
    sh, sw = style_hw or (h, w)
    return (rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8),
            rs(2).randint(0, 256, (sh, sw, 3)).astype(np.uint8))


def job(topo, params, size, weights, precision='bf16', conv_algo=1):
    init, content, style = images(*size)
    st = st2.StyleTransfer(model(params, topo, precision, conv_algo))
    st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
    st.set_weights(weights, PARAMS4)
    return st


def evaluate(st, algo, n=2):
    """n objective evaluations from the job's initial image under pool_algo `algo` (the first captures the norms, the second is the
    steady state with the fused style term): ([(loss, gradient, trace values)], launches per class of all n)."""
    st.engine.set_pool_algo(algo)
    st.engine.set_input(images(*st.input_shape[2:])[0])
    st.engine.clear_norms()
    st.engine.profile_enable(True)
    out = []
    for _ in range(n):
        loss, grad, values = st.engine.opfunc()
        out.append((loss, grad.copy(), np.array(values)))
    prof = launches(st.engine)
    st.engine.profile_enable(False)
    return out, prof


def assert_same(a, b, what):
    for k, ((l0, g0, t0), (l1, g1, t1)) in enumerate(zip(a, b)):
        assert np.array_equal(l0, l1), '%s: loss of evaluation %d: %r != %r' % (what, k, l0, l1)
        assert np.array_equal(t0, t1), '%s: trace of evaluation %d differs at %s' % (what, k, np.flatnonzero(t0 != t1))
        assert np.isfinite(g0).all() and np.array_equal(g0, g1), '%s: %d gradient elements of evaluation %d differ' % (what, int((g0 != g1).sum()), k)


def head_weights(topo):
    """content on the last blob, style on the first conv and on the last blob; the conv below the pool and the pool carry nothing"""
    last = topo[-1][1]
    return {'content': {last: 0.1}, 'style': {'conv1_1': 1, last: 1}, 'deepdream': {}}


# ------------------------------------------------------------------------------------------ 1. the switch
def test_switch_defaults_to_0_round_trips_and_refuses_other_values():
    eng = st2.Engine(NET)
    assert eng.pool_algo() == 0
    for v in (1, 0, 1):
        eng.set_pool_algo(v)
        assert eng.pool_algo() == v
    with pytest.raises(ValueError, match='pool_algo'):
        eng.set_pool_algo(2)
    assert eng.lib.st_set_pool_algo(eng._ctx, 2) == 1 and b'pool algorithm 2' in eng.lib.st_last_error()      # ST_ERR_ARG
    assert eng.lib.st_set_pool_algo(eng._ctx, -1) == 1
    assert eng.pool_algo() == 1
    assert st2.HipModel(None, topology=NET, pool_algo=1).engine.pool_algo() == 1
    eng.close()


# ------------------------------------------------------------------------------------------ 2. the routes change
VGG41 = ave(oracle.VGG19_TOPOLOGY)[:12]          # ... pool3, conv4_1
W41 = {'content': {'conv4_1': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1}, 'deepdream': {}}


@pytest.mark.parametrize('unpool', ['1', '0'])
def test_every_average_pool_leaves_the_stand_alone_passes(unpool, monkeypatch):
    """VGG19 with average pools up to conv4_1 at 32 x 64 on the 64 x 256 tile: under pool_algo 1 no avepool_fwd / avepool_bwd launch
    is left, pool1 and pool2 are expanded inside the data gradients of conv1_2 and conv2_2, pool3 (conv3_4: K = 256) runs
    avepool_bwd_map16_k; ST2_CONV16_UNPOOL=0: all three do.  The conv classes launch what they launched before."""
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    monkeypatch.setenv('ST2_CONV16_UNPOOL', unpool)
    st = job(VGG41, oracle.he_init_weights(VGG41, seed=0), (32, 64), W41)
    (_, n0), (_, n1) = evaluate(st, 0, n=1), evaluate(st, 1, n=1)
    assert n0['avepool_fwd'] == 3 and n0['avepool_bwd'] == 3 and n0['avepool_bwd_map16'] == 0, n0
    assert n1['avepool_fwd'] == 0 and n1['avepool_bwd'] == 0, n1
    assert n1['avepool_bwd_map16'] == (1 if unpool == '1' else 3), n1
    assert n1[FWD16] == n0[FWD16] and n1[DG16] == n0[DG16] and n0[FWD16] > 0 and n0[DG16] > 0, (n0, n1)
    assert n1['maxpool_bwd'] == 0 and n1['maxpool_fwd'] == 0 and n0['maxpool_bwd'] == 0, n1
    st.engine.close()


# ------------------------------------------------------------------------------------------ 3. bit identity, per build
#        id                      net     size        environment
BUILDS = [
    ('sb-64x256',               NET,    (16, 32),   {'ST2_CONV16_CFG': '0'}),
    ('sb-64x256-ragged',        NET,    (24, 72),   {'ST2_CONV16_CFG': '0'}),
    ('clipped-17x33',           NET,    (17, 33),   {'ST2_CONV16_CFG': '0'}),
    ('clipped-1x5',             NET,    (1, 5),     {'ST2_CONV16_CFG': '0'}),
    ('db-64x256',               NET128, (16, 64),   {'ST2_CONV16_CFG': '0', 'ST2_CONV16_SB_MAXK': '0'}),
    ('128x128',                 NET128, (16, 64),   {'ST2_CONV16_CFG': '1'}),
    ('64x512',                  NET,    (32, 64),   {'ST2_CONV16_CFG': '3'}),
    ('k256',                    NET256, (8, 32),    {'ST2_CONV16_CFG': '0'}),
    # the general epilogue and the legacy-mask unpooling builds at whole windows, a clipped 64 x 512 tile,
    # and the default tile selection at the smallest size at which it takes the 64 x 256 tile for 64 channels (512 workgroups)
    ('general-epilogue',        NET,    (16, 32),   {'ST2_CONV16_CFG': '0', 'ST2_CONV16_EPI': '0'}),
    ('no-sign-maps-64x256',     NET,    (16, 32),   {'ST2_CONV16_CFG': '0', 'ST2_MASK_BITS': '0'}),
    ('no-sign-maps-64x512',     NET,    (32, 64),   {'ST2_CONV16_CFG': '3', 'ST2_MASK_BITS': '0'}),
    ('64x512-clipped',          NET,    (17, 33),   {'ST2_CONV16_CFG': '3'}),
    ('default-tiles',           NET,    (128, 1024), {}),
]


@pytest.mark.parametrize('name,topo,size,env', BUILDS, ids=[b[0] for b in BUILDS])
def test_objective_is_bit_identical_on_every_build(name, topo, size, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    st = job(topo, oracle.he_init_weights(topo, seed=7, bias_std=0.2), size, head_weights(topo))
    (r0, n0), (r1, n1) = evaluate(st, 0), evaluate(st, 1)
    assert n0['avepool_fwd'] == 2 and n0['avepool_bwd'] == 2, (name, n0)
    assert n1['avepool_fwd'] == 0 and n1['avepool_bwd'] == 0, (name, n1)          # the fused route ran, both evaluations
    h, w = size
    k_below = [l for l in topo if l[0] == 'conv'][-2][3]
    in_dgrad = h % 2 == 0 and w % 2 == 0 and k_below <= 128 and env.get('ST2_CONV16_CFG', '0') in ('0', '3')
    assert n1['avepool_bwd_map16'] == (0 if in_dgrad else 2), (name, n1)
    assert n1[FWD16] == n0[FWD16] and n1[DG16] == n0[DG16], (name, n0, n1)
    assert_same(r0, r1, name)
    st.engine.close()


def test_mixed_max_and_average_pools(monkeypatch):
    """VGG19 to conv5_1 with MAX pools 1-2 and AVE pools 3-4 at 32 x 64: equal under 0 and 1, the two average pools leave the stand-alone
    passes, the two max pools launch what they launched before (fused forward, expanded inside conv1_2's and conv2_2's data gradients)."""
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    topo = ave(oracle.VGG19_TOPOLOGY, ('pool3', 'pool4'))[:17]
    st = job(topo, oracle.he_init_weights(topo, seed=0), (32, 64), VGG_WEIGHTS)
    (r0, n0), (r1, n1) = evaluate(st, 0), evaluate(st, 1)
    assert n0['avepool_fwd'] == 4 and n0['avepool_bwd'] == 4 and n1['avepool_fwd'] == 0 and n1['avepool_bwd'] == 0, (n0, n1)
    assert n1['avepool_bwd_map16'] == 4, n1                # conv3_4 and conv4_4: K = 256 and 512
    for cls in ('maxpool_fwd', 'maxpool_bwd', FWD16, DG16):
        assert n1[cls] == n0[cls], (cls, n0, n1)
    assert n0['maxpool_fwd'] == 0 and n0['maxpool_bwd'] == 0, n0
    assert_same(r0, r1, 'mixed')
    st.engine.close()


# ------------------------------------------------------------------------------------------ 4. what stays stand-alone
def test_a_weighted_conv_blob_keeps_its_pool_stand_alone(monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    weights = {'content': {'conv1_2': 0.1, 'conv2_1': 0.1}, 'style': {'conv1_1': 1}, 'deepdream': {}}
    st = job(NET, oracle.he_init_weights(NET, seed=7, bias_std=0.2), (16, 32), weights)
    (r0, n0), (r1, n1) = evaluate(st, 0, n=1), evaluate(st, 1, n=1)
    assert n1['avepool_fwd'] == 1 and n1['avepool_bwd'] == 1 and n1['avepool_bwd_map16'] == 0, n1
    assert n1 == n0
    assert_same(r0, r1, 'weighted conv blob')
    st.engine.close()


@pytest.mark.parametrize('size', [(16, 32), (17, 33)], ids=str)
def test_a_weighted_pool_blob_comes_out_of_the_fused_launch_in_fp32(size, monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    weights = {'content': {'pool1': 0.1, 'conv2_1': 0.1}, 'style': {'conv1_1': 1}, 'deepdream': {}}
    st = job(NET, oracle.he_init_weights(NET, seed=7, bias_std=0.2), size, weights)
    r0, n0 = evaluate(st, 0)
    p0 = st.engine.get_blob('pool1')
    r1, n1 = evaluate(st, 1)
    p1 = st.engine.get_blob('pool1')
    assert n0['avepool_fwd'] == 2 and n1['avepool_fwd'] == 0 and n1['avepool_bwd'] == 0, (n0, n1)
    assert p0.any() and np.array_equal(p0, p1)
    assert_same(r0, r1, 'weighted pool blob')
    st.engine.close()


@pytest.mark.parametrize('precision,conv_algo', [('fp32', 1), ('fp32', 2), ('bf16-full', 1)])
def test_other_precisions_route_as_before(precision, conv_algo, monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    st = job(NET, oracle.he_init_weights(NET, seed=7, bias_std=0.2), (16, 32), head_weights(NET), precision=precision, conv_algo=conv_algo)
    (r0, n0), (r1, n1) = evaluate(st, 0), evaluate(st, 1)
    assert n1 == n0 and n0['avepool_fwd'] == 2 and n0['avepool_bwd'] == 2, (n0, n1)
    assert_same(r0, r1, precision)
    st.engine.close()


# ------------------------------------------------------------------------------------------ 5. the mask is `> 0`, no stray bits
def _avepool_exact(x):
    c, h, w = x.shape
    ho, wo = eo.pooled_size(h), eo.pooled_size(w)
    pad = np.zeros((c, 2 * ho, 2 * wo), F64)
    pad[:, :h, :w] = x
    cnt = np.zeros((2 * ho, 2 * wo), F64)
    cnt[:h, :w] = 1
    s = pad.reshape(c, ho, 2, wo, 2).sum((2, 4))
    n = cnt.reshape(ho, 2, wo, 2).sum((1, 3))
    return s / n, n


def _avepool_backward_exact(dy, n, in_shape):
    c, h, w = in_shape
    return np.ascontiguousarray(np.repeat(np.repeat(dy / n, 2, axis=1), 2, axis=2)[:, :h, :w])


def _integer_case(h, w):
    """The head recipe of tests/exact_oracle.py on NET (3-tap filters of +-1, biases in {-1, 0, 1}, image in [-1, 1] constant on 4 x 4
    blocks), with two changes that make the OBJECTIVE exact as well: conv2_1's bias is 64 (every pre-activation positive), and the
    content features are taken with that bias shifted by s_c = +-1 per channel.  Then F - F_content = -s_c everywhere, the captured
    norm is exactly 2 / n, and with a content weight of 4 the diff injected at conv2_1 is -4 s_c: integers, multiples of 4 (the
    average pool divides by 4, 2 or 1)."""
    for seed in range(32):
        rng = np.random.RandomState(seed * 10007 + h * 101 + w)
        params = {n: (eo.sparse_weights(rng, co, ci, 3), eo.int_bias(rng, co)) for _, n, ci, co in (l for l in NET if l[0] == 'conv')}
        params['conv2_1'] = (params['conv2_1'][0], np.full(64, 64.0))
        x = eo.int_image(rng, h, w, -1, 1, block=4)
        pre = eo.conv3x3_exact(np.maximum(eo.conv3x3_exact(x, *params['conv1_1']), 0), *params['conv1_2'])
        if float((pre == 0).mean()) >= 0.10 and float((pre > 0).mean()) >= 0.20:
            return params, x, rng.choice((-1.0, 1.0), 64)
    raise AssertionError('no seed below 32 gives a tenth of zero pre-activations at %d x %d' % (h, w))


def _integer_reference(params, x, shift, cw):
    """float64 gradient of cw * content loss at conv2_1 for NET with an average pool, the sufficient conditions of exact_oracle
    asserted on the way: (gradient (3, h, w), share of conv1_2 pre-activations that are exactly 0)."""
    c11 = np.maximum(eo.conv3x3_exact(x, *params['conv1_1']), 0)
    eo.assert_exact_domain('bf16', c11, *params['conv1_2'])
    pre12 = eo.conv3x3_exact(c11, *params['conv1_2'])
    c12 = np.maximum(pre12, 0)
    p1, n = _avepool_exact(c12)
    assert eo.bf16_representable(p1) and eo.bf16_representable(c12) and eo.bf16_representable(c11)
    assert eo._is_integer(4 * p1)
    eo.assert_exact_domain('bf16', 4 * p1, *params['conv2_1'])          # (quarters: the same sums in units of 1/4)
    pre21 = eo.conv3x3_exact(p1, *params['conv2_1'])
    assert float(pre21.min()) > 2.0 and float(np.abs(pre21).max()) * 4 < eo.LIMIT          # no ReLU at conv2_1, with either bias
    g = np.broadcast_to((-cw * shift).reshape(64, 1, 1), pre21.shape).astype(F64)
    g = bf16_round(g.astype(F32)).astype(F64)
    eo.assert_exact_domain('bf16', g, eo.transposed_filters(params['conv2_1'][0]))
    g = eo.conv3x3_dgrad_exact(g, params['conv2_1'][0])
    assert eo._is_integer(g / 4)
    # the pooled diff is stored as bf16 (fused: before the division, stand-alone: after it -- the same number), each element of a
    # window receives it divided by the window size where the conv blob is > 0
    g = _avepool_backward_exact(bf16_round(g.astype(F32)).astype(F64), n, c12.shape) * (c12 > 0)
    assert eo._is_integer(g)
    g = bf16_round(g.astype(F32)).astype(F64)
    eo.assert_exact_domain('bf16', g, eo.transposed_filters(params['conv1_2'][0]))
    g = eo.conv3x3_dgrad_exact(g, params['conv1_2'][0]) * (c11 > 0)
    g = bf16_round(g.astype(F32)).astype(F64)
    eo.assert_exact_domain('bf16', g, eo.transposed_filters(params['conv1_1'][0]))
    g = eo.conv3x3_dgrad_exact(g, params['conv1_1'][0])
    assert float(np.abs(g).max()) < eo.LIMIT
    return g, float((pre12 == 0).mean())


@pytest.mark.parametrize('size', [(16, 32), (15, 31)], ids=str)
def test_integer_recipe_gradient_equals_the_float64_reference_under_both_values(size, monkeypatch):
    """Small-integer weights and image: every sum is exact, a tenth or more of conv1_2's pre-activations is exactly 0 (the map's bit
    must be `> 0`, not `>= 0`), and at 15 x 31 the last row and column of windows are clipped (divisors 2 and 1; conv2_1 still has
    64 x 8 x 16 = 2^13 elements, which keeps the objective's 2 / n and the captured norm powers of two).  The gradient of
    the objective (content term at conv2_1 only, no TV / p-norm term) under pool_algo 1 equals the one under 0 and both equal the
    float64 reference, bit for bit."""
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    h, w = size
    cw = 4.0
    params, x, shift = _integer_case(h, w)
    want, zeros = _integer_reference(params, x, shift, cw)
    print('%d x %d: %.1f %% of conv1_2\'s pre-activations are exactly 0' % (h, w, 100 * zeros))
    assert zeros >= 0.10
    shifted = dict(params, conv2_1=(params['conv2_1'][0], params['conv2_1'][1] + shift))
    eng = st2.Engine(NET, precision='bf16')
    x4 = x[None].astype(F32)
    got = {}
    for algo in (0, 1):
        eng.set_pool_algo(algo)
        eng.set_weights(['conv2_1'], [cw], [0], [0], [0, 2, 0, 6])
        eng.load_weights(eo.params32(shifted))
        eng.set_content_nchw(x4)
        eng.load_weights(eo.params32(params))
        eng.set_input_nchw(x4)
        eng.clear_norms()
        eng.profile_enable(True)
        _, grad, _ = eng.opfunc()
        n = launches(eng)
        eng.profile_enable(False)
        assert n['avepool_fwd'] == 1 - algo and n['avepool_bwd'] == 1 - algo, (algo, n)
        got[algo] = grad[0].astype(F64)
    assert want.any()
    for algo in (0, 1):
        bad = got[algo] != want
        assert not bad.any(), 'pool_algo %d: %d of %d elements differ from the float64 reference, first at %s: %r != %r' % (
            algo, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[algo][bad][0], want[bad][0])
    eng.close()


# ------------------------------------------------------------------------------------------ 6. the optimizers
@pytest.mark.parametrize('kind,step', [('adam', 10), ('lbfgs', 1)])
def test_optimizer_trajectories_are_bit_identical(kind, step, monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    topo = ave(oracle.VGG19_TOPOLOGY)[:17]           # ... pool4, conv5_1
    st = job(topo, oracle.he_init_weights(topo, seed=0), (64, 96), VGG_WEIGHTS)
    st.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[kind]
    st.set_step_size(step)
    init = images(64, 96)[0]
    runs = {}
    for algo in (0, 1):
        st.engine.set_pool_algo(algo)
        st.set_input(init)
        st.reset()
        assert st.start()
        st.engine.profile_enable(True)
        losses = []
        for _ in range(3):
            image, trace = st.step()
            losses.append(trace['loss'])
        n = launches(st.engine)
        st.engine.profile_enable(False)
        assert n['avepool_fwd'] == n['avepool_bwd'] and (n['avepool_bwd'] == 0 if algo else n['avepool_bwd'] >= 12), (algo, n)
        assert (n['avepool_bwd_map16'] > 0) == (algo == 1), (algo, n)
        runs[algo] = (losses, image.copy())
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][1]).all() and np.array_equal(runs[0][1], runs[1][1])
    assert len(set(runs[0][0])) == 3
    st.engine.close()


# ------------------------------------------------------------------------------------------ 7. the hooks
def test_hooks_refuse_the_skipped_conv_blob_and_never_pair_a_map_with_the_wrong_reader(monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    # (conv1_1 carries a content weight: its fp32 blob, the ReLU mask st_backward's chain reads for conv1_2, is written by every evaluation)
    weights = {'content': {'conv1_1': 0.1, 'conv2_1': 0.1}, 'style': {'conv2_1': 1}, 'deepdream': {}}
    st = job(NET, oracle.he_init_weights(NET, seed=7, bias_std=0.2), (16, 32), weights)
    eng = st.engine
    _, n = evaluate(st, 1, n=1)
    assert n['avepool_fwd'] == 0
    for hook in (eng.get_blob, eng.gram):
        with pytest.raises(capi.StError, match='conv1_2'):
            hook('conv1_2')
    assert eng.get_blob('conv2_1').any()
    # the answer the backward hook owes for a diff at pool1 on this iterate: every blob written (st_forward), stand-alone pool
    x = eng.get_input_nchw()
    d = np.random.RandomState(9).randn(1, 64, 8, 16).astype(F32)
    eng.forward(x)
    assert eng.get_blob('conv1_2').any() and eng.gram('conv1_2').any()
    mask12 = eng.get_blob('conv1_2') > 0
    want = eng.backward({'pool1': d})
    assert want.any()
    # a lean evaluation under 1 (sign map written, fp32 conv blob skipped), the switch flipped, then st_backward: a refusal that names
    # the state, or that answer -- never a gradient taken through the map by the wrong reader
    for flip_to in (0, 1):
        evaluate(st, 1, n=1)
        eng.set_pool_algo(flip_to)
        try:
            got = eng.backward({'pool1': d})
        except capi.StError as e:
            assert 'not materialised' in str(e) and 'pool1' in str(e), str(e)
        else:
            assert np.array_equal(got, want)
    # ... and the other way round: a lean evaluation under 0 (no map, the fp32 conv blob written), the switch flipped to 1: the
    # stand-alone pass answers
    evaluate(st, 0, n=1)
    eng.set_pool_algo(1)
    assert np.array_equal(eng.backward({'pool1': d}), want)
    assert np.array_equal(eng.get_blob('conv1_2') > 0, mask12)
    eng.close()


# ------------------------------------------------------------------------------------------ 8. the worker
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


def test_worker_reads_pool_algo_and_produces_the_same_first_iterate(tmp_path, monkeypatch):
    monkeypatch.setenv('ST2_CONV16_CFG', '0')
    sys.path.insert(0, os.path.dirname(HERE))
    import messages
    import worker as worker_mod
    with open(os.path.join(HERE, 'golden', 'vgg19.prototxt')) as f:
        text = f.read().replace('pool: MAX', 'pool: AVE')
    path = tmp_path / 'vgg19_ave.prototxt'
    path.write_text(text)
    assert prototxt.read(str(path), average_pools=True) == ave(oracle.VGG19_TOPOLOGY)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (64, 80, 3)).astype(np.uint8), rs(2).randint(0, 256, (48, 64, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (64, 80, 3)).astype(np.uint8))
    first = {}
    for key in (None, '1'):
        section = {'prototxt': str(path), 'caffemodel': str(tmp_path / 'absent.npz'), 'weights': 'synthetic', 'precision': 'bf16',
                   'async_iterate': '0', 'pipeline_iterate': '1'}
        if key is not None:
            section['pool_algo'] = key
        cp = configparser.ConfigParser()
        cp.read_dict({'worker': section})
        socks = _Socks(messages, pause_after=2)
        socks.inbound.extend([messages.SetImages(None, init, content, style, True), messages.SetWeights(VGG_WEIGHTS, PARAMS4),
                              messages.SetOptimizer('adam', 10), messages.StartIteration()])
        wk = worker_mod.Worker(cp['worker'], sock_in=socks, sock_out=socks)
        eng = wk.transfer.model.engine
        assert eng.topology == ave(oracle.VGG19_TOPOLOGY) and eng.pool_algo() == (1 if key else 0)
        eng.profile_enable(True)
        wk.run()
        n = launches(eng)
        assert (n['avepool_bwd'] == 0 and n['avepool_bwd_map16'] > 0) if key else (n['avepool_bwd'] > 0 and n['avepool_bwd_map16'] == 0), n
        its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
        assert len(its) >= 2 and its[0].i == 1 and np.isfinite(its[0].trace['loss'])
        first[key] = (its[0].image.copy(), its[0].trace['loss'])
    assert first[None][1] == first['1'][1] and np.array_equal(first[None][0], first['1'][0])
