"""The integer-exact references of tests/exact_oracle.py, checked on the CPU: against the float32 oracle (which is exact on such
data too), the Winograd exactness bound against a float32 emulation that re-associates every sum at random, and the tie / zero
conditions of the recipes that tests/test_gpu_exact.py runs."""

import numpy as np
import pytest

from oracle.caffe_net import NetOracle, bf16_round, conv3x3_backward_data, conv3x3_forward, maxpool_backward, maxpool_forward
import exact_oracle as eo

F32 = np.float32


@pytest.mark.parametrize('cin,cout,h,w', [(3, 64, 5, 33), (64, 64, 6, 36), (64, 128, 9, 70), (128, 48, 2, 3), (512, 512, 5, 33), (256, 256, 1, 1)])
def test_exact_conv_equals_the_float32_oracle_on_integer_data(cin, cout, h, w):
    """Inside the `direct` domain the oracle's SGEMM is exact whatever order BLAS sums in: equality, forward and data gradient."""
    topo, params, x, dy = eo.layer_recipe(cin, cout, h, w)
    net = eo.ExactNet(topo, params, paths='direct')
    blobs = net.forward(x)
    last = topo[-1][1]
    below = blobs[net.names[-2]]
    wgt, b = params[last]
    assert np.array_equal(conv3x3_forward(below.astype(F32), wgt.astype(F32), b.astype(F32)), net.pre[last])
    assert np.array_equal(conv3x3_backward_data(dy.astype(F32), wgt.astype(F32)), eo.conv3x3_dgrad_exact(dy, wgt))
    # ... and the whole chain, ReLU masks and injection semantics included
    cpu = NetOracle(topo, eo.params32(params))
    f = cpu.forward(x[None].astype(F32))
    for name in f:
        assert np.array_equal(f[name][0], blobs[name]), name
    assert np.array_equal(cpu.backward({last: dy[None].astype(F32)})[0], net.backward({last: dy}))


@pytest.mark.parametrize('h,w', [(9, 13), (16, 24)])
def test_exact_head_equals_the_float32_oracle_pools_and_injections_included(h, w):
    params, x, diffs, _ = eo.head_recipe(h, w)
    for bf16 in (False, True):
        net = eo.ExactNet(eo.HEAD_TOPOLOGY, params, paths=('direct', 'wino', 'split', 'bf16') if bf16 else ('direct', 'wino', 'split'), bf16=bf16)
        blobs = net.forward(x)
        cpu = NetOracle(eo.HEAD_TOPOLOGY, eo.params32(params), operands='bf16' if bf16 else 'fp32')
        f = cpu.forward(x[None].astype(F32))
        for name in f:
            assert np.array_equal(f[name][0], blobs[name]), name
        for names in [eo.HEAD_INJECTIONS] + [(n,) for n in eo.HEAD_INJECTIONS]:
            dd = {n: diffs[n] for n in names}
            assert np.array_equal(cpu.backward({n: v[None].astype(F32) for n, v in dd.items()})[0], net.backward(dd)), (bf16, names)
    # the pool primitives on a hand case with ties: the first maximum takes the diff
    xx = np.array([[[1, 1, 0], [1, 1, 2], [0, 0, 0]]], np.float64)
    pooled, slot = eo.maxpool_exact(xx)
    assert np.array_equal(pooled[0], [[1, 2], [0, 0]]) and np.array_equal(slot[0], [[0, 2], [0, 0]])
    dy = np.array([[[5, 7], [11, 13]]], np.float64)
    assert np.array_equal(eo.maxpool_backward_exact(dy, slot, xx.shape)[0], [[5, 0, 0], [0, 0, 7], [11, 0, 13]])
    assert np.array_equal(eo.maxpool_backward_exact(dy, slot, xx.shape), maxpool_backward(dy.astype(F32), maxpool_forward(xx.astype(F32))[1], xx.shape))


def test_exact_gram_is_one_float32_division_of_the_exact_sums():
    topo, params, x = eo.gram_recipe(200, 5, 7)
    f = eo.ExactNet(topo, params).forward(x)['conv1_1']
    eo.assert_gram_domain(f.reshape(200, -1))
    s = eo.gram_sums_exact(f)
    assert np.array_equal(s, s.T) and np.array_equal(s, np.rint(s))
    g = eo.gram_exact(f)
    assert g.dtype == F32 and np.array_equal(g, g.T)
    f32 = f.reshape(200, -1).astype(F32)
    assert np.array_equal(g, np.dot(f32, f32.T) / F32(f32.size))          # worker.py:114 on exact sums


# the largest K of every recipe of tests/test_gpu_exact.py: part A's layer at 512 -> 512 (forward K = data gradient K = 512), its
# asymmetric pairs, and part B's head (K = 128)
@pytest.mark.parametrize('cin,cout,h,w', [(512, 512, 5, 33), (256, 256, 9, 70), (64, 128, 8, 64), (128, 48, 2, 3), (40, 64, 1, 1)])
def test_winograd_in_float32_is_exact_in_any_order_inside_the_bound(cin, cout, h, w):
    """The bound 144 max|d| max ||g||_1 + |b| < 2^24 itself: float32 Winograd with shuffled channel order, random split-K parts and
    shuffled transform association equals the exact conv, forward and data gradient."""
    topo, params, x, dy = eo.layer_recipe(cin, cout, h, w)
    net = eo.ExactNet(topo, params, paths=('wino', 'split'))
    below = net.forward(x)['conv1_1']
    wgt, b = params['conv1_2']
    rng = np.random.RandomState(h * w + cin)
    for trial in range(2):
        assert np.array_equal(eo.winograd_f32_emulation(below, wgt, b, rng), net.pre['conv1_2']), trial
        eo.assert_exact_domain('wino', dy, eo.transposed_filters(wgt))
        assert np.array_equal(eo.winograd_f32_emulation(dy, eo.transposed_filters(wgt), None, rng), eo.conv3x3_dgrad_exact(dy, wgt)), trial


@pytest.mark.parametrize('h,w', [(8, 32), (9, 13)])
def test_winograd_in_float32_is_exact_on_the_head_recipe(h, w):
    params, x, diffs, _ = eo.head_recipe(h, w)
    net = eo.ExactNet(eo.HEAD_TOPOLOGY, params)
    blobs = net.forward(x)
    rng = np.random.RandomState(h + w)
    for below, name in (('conv1_1', 'conv1_2'), ('pool1', 'conv2_1'), ('conv2_1', 'conv2_2')):
        wgt, b = params[name]
        assert np.array_equal(eo.winograd_f32_emulation(blobs[below], wgt, b, rng), net.pre[name]), name


def test_the_domain_check_refuses_what_leaves_it():
    rng = np.random.RandomState(0)
    g = eo.dense_weights(rng, 8, 512)
    eo.assert_exact_domain('direct', np.full((512, 2, 2), 3000.0), g)
    with pytest.raises(AssertionError, match='2\\^24'):
        eo.assert_exact_domain('wino', np.full((512, 2, 2), 3000.0), g)           # 144 * 3000 * ~3000
    with pytest.raises(AssertionError, match='integers'):
        eo.assert_exact_domain('direct', np.full((512, 2, 2), 0.5), g)
    with pytest.raises(AssertionError, match='bf16'):
        eo.assert_exact_domain('bf16', np.full((512, 2, 2), 257.0), g)
    eo.assert_exact_domain('bf16', np.full((512, 2, 2), 256.0), g)
    with pytest.raises(AssertionError, match='16 significant bits'):
        eo.assert_exact_domain('split', np.full((8, 2, 2), 5000.0), g[:, :8] * 0 + np.eye(8)[:, :, None, None])
    assert np.array_equal(bf16_round(np.array([257, 259], F32)), [256, 260])       # ties to even: what the reference applies to a stored diff


@pytest.mark.parametrize('h,w', [(8, 32), (16, 24), (9, 13), (6, 64)])
def test_head_recipe_is_full_of_ties_and_exact_zeros(h, w):
    """Part B's conditions on the reference alone, at every size the GPU test runs: at every pooled conv blob >= 20 % of the windows
    with a positive maximum are tied, in >= 10 % of all windows the first and the last maximiser differ, >= 5 % of the
    pre-activations are exactly 0.  Every blob and every running diff of the bf16 chain is bf16-representable or is rounded by
    the reference where the path stores it (ExactNet(bf16=True) asserts the former for the conv operands)."""
    params, x, diffs, seed = eo.head_recipe(h, w)
    net = eo.ExactNet(eo.HEAD_TOPOLOGY, params, paths=('direct', 'wino', 'split', 'bf16'), bf16=True)
    blobs = net.forward(x)
    for name in eo.HEAD_POOLED:
        tied, differ, zeros = eo.assert_tie_conditions(net.pre[name], name)
        print('[exact head %dx%d seed %d] %s: %.0f %% of positive windows tied, first != last in %.0f %%, %.0f %% exact zeros' % (
            h, w, seed, name, 100 * tied, 100 * differ, 100 * zeros))
    for name, blob in blobs.items():
        assert eo.bf16_representable(blob), name
    # a last-maximum pool, or a `>=` mask, gives another gradient on this data: the GPU comparison can tell them apart
    g = net.backward({'pool2': diffs['pool2']})
    last_slots = dict(net.slots)
    for below, name in (('conv1_2', 'pool1'), ('conv2_2', 'pool2')):
        c, hh, ww = blobs[below].shape
        ho, wo = blobs[name].shape[1:]
        pad = np.full((c, 2 * ho, 2 * wo), -1.0)
        pad[:, :hh, :ww] = blobs[below]
        win = pad.reshape(c, ho, 2, wo, 2).transpose(0, 1, 3, 2, 4).reshape(c, ho, wo, 4)
        last_slots[name] = 3 - np.argmax(win[..., ::-1], -1)
    net.slots = last_slots
    assert not np.array_equal(net.backward({'pool2': diffs['pool2']}), g)
