"""Parity of the HIP path (through the C ABI) with the CPU oracle and the committed golden vectors.

Run on the GPU box with ``pytest -m gpu``.  Tolerances are stated per test: everything here is
IEEE fp32 on both sides, differing only in summation order (MFMA k-chains vs BLAS), so the bars
are rel-L2 <= 1e-5 for single layers and <= 1e-4 for whole-network gradients.
"""
import json

import numpy as np
import pytest

import oracle
import style_transfer2_amd as st2
from helpers import load, rel_l2, tiny_setup, check_trace

pytestmark = pytest.mark.gpu
F32 = np.float32


def make_models(topo, seed=0, bias_std=0.1):
    params = oracle.he_init_weights(topo, seed=seed, bias_std=bias_std)
    return oracle.NetOracle(topo, params), st2.HipModel(params, topology=topo)


# ------------------------------------------------------------------------------------------ layers
@pytest.mark.parametrize('cin,cout,h,w', [
    (3, 64, 16, 32), (3, 8, 5, 7), (8, 16, 16, 20), (64, 64, 24, 40), (64, 128, 17, 33),
    (128, 256, 12, 12), (256, 512, 8, 8), (512, 512, 9, 6), (6, 8, 9, 12), (16, 8, 31, 65),
    (64, 64, 64, 96), (128, 128, 40, 70)])
def test_single_conv_forward_and_dgrad(cin, cout, h, w):
    """conv3x3+ReLU forward of one layer and its data gradient, odd sizes and every tile config."""
    topo = (('conv', 'conv1_1', 3, cin), ('conv', 'conv1_2', cin, cout)) if cin != 3 else (('conv', 'conv1_1', 3, cout),)
    cpu, gpu = make_models(topo, seed=cin + cout, bias_std=0.2)
    rng = np.random.RandomState(h * w)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)
    last = topo[-1][1]
    fc = cpu.forward(x, [last])[last]
    fg = gpu.forward(x, [last])[last]
    assert fg.shape == fc.shape
    tol = 1e-5 if cin <= 256 else 3e-5      # fp32 k-chain of 9*Cin terms vs BLAS blocking: ~sqrt(K) eps
    assert rel_l2(fg, fc) <= tol, rel_l2(fg, fc)
    assert np.array_equal(fg == 0, fc == 0) or np.mean((fg == 0) != (fc == 0)) < 1e-4   # ReLU pattern
    d = rng.randn(*fc.shape).astype(F32)
    gc = cpu.backward({last: d})
    gg = gpu.backward({last: d})
    assert rel_l2(gg, gc) <= 3 * tol, rel_l2(gg, gc)


def test_pool_ceil_mode_and_first_max():
    topo = (('conv', 'conv1_1', 3, 8), ('pool', 'pool1'), ('conv', 'conv2_1', 8, 8), ('pool', 'pool2'))
    cpu, gpu = make_models(topo, seed=3)
    for h, w in ((9, 13), (8, 8), (1, 5), (7, 2), (33, 65)):
        x = (np.random.RandomState(h).randn(1, 3, h, w) * 40).astype(F32)
        x[0, :, : h // 2] = np.round(x[0, :, : h // 2] / 20) * 20        # plenty of exact ties / zeros
        fc, fg = cpu.forward(x), gpu.forward(x)
        for name in fc:
            assert fg[name].shape == fc[name].shape, (name, h, w)
            assert rel_l2(fg[name], fc[name]) <= 1e-5, (name, h, w)
        d = {'pool2': np.random.RandomState(1).randn(*fc['pool2'].shape).astype(F32),
             'pool1': np.random.RandomState(2).randn(*fc['pool1'].shape).astype(F32)}
        assert rel_l2(gpu.backward(d), cpu.backward(d)) <= 2e-5, (h, w)


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('kernel', ['quad', '1', '0'])
@pytest.mark.parametrize('cout,h,w', [(64, 64, 96), (64, 75, 100), (16, 9, 33), (32, 40, 31), (64, 8, 32), (48, 21, 70), (24, 12, 20), (64, 23, 132)])
def test_first_conv_data_gradient_on_the_matrix_cores(precision, kernel, cout, h, w, monkeypatch):
    """conv1_1's data gradient (3 output channels): Z = A @ dy as one 32-row MFMA tile + 27 shifted adds
    (conv3x3_dgrad_first.hip; ST2_DGRAD_FIRST=0 keeps the VALU kernel) against the oracle fed with the GPU's own forward state,
    with a diff injected at the data blob too; tiles cut by the right / bottom edge, widths that are not multiples of 4, channel
    counts the bf16 variant cannot take (24: falls back)."""
    # 'quad': the fp32 kernel with 16-byte operand loads (aligned widths; other shapes fall through to the VALU kernel);
    # '1' / '0': the four-byte-load matrix-core kernels forced on / everything on the VALU kernels
    monkeypatch.setenv('ST2_DGRAD_FIRST_Q', '1' if kernel == 'quad' else '0')
    monkeypatch.setenv('ST2_DGRAD_FIRST', '0' if kernel == 'quad' else kernel)
    if kernel == 'quad' and precision == 'bf16':
        pytest.skip('the quad kernel is the fp32 path')
    topo = (('conv', 'conv1_1', 3, cout),)
    params = oracle.he_init_weights(topo, seed=cout + h, bias_std=0.2)
    gpu = st2.HipModel(params, topology=topo, precision=precision)
    cpu = oracle.NetOracle(topo, params, operands='bf16' if precision == 'bf16' else 'fp32')
    rng = np.random.RandomState(h * w + cout)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)
    f = gpu.forward(x, ['conv1_1'])
    cpu.forward(x)
    cpu.adopt_forward_state(f)
    for names in (['conv1_1'], ['conv1_1', 'data']):
        diffs = {n: rng.randn(*(f[n].shape if n != 'data' else x.shape)).astype(F32) for n in names}
        err = rel_l2(gpu.backward(diffs), cpu.backward(diffs))
        assert err <= (5e-5 if precision == 'bf16' else 2e-6), (names, err)


@pytest.mark.parametrize('h,w', [(64, 96), (75, 100), (8, 32), (23, 132), (40, 127), (131, 380), (256, 512)])
def test_first_conv_data_gradient_strip_walker_fp32(h, w, monkeypatch):
    """conv1_1's fp32 data gradient at 64 channels, the default since round 4: conv3x3_dgrad_first_f32_strip (a workgroup walks down a
    126-pixel column strip: every row of the diff is read once, three rows in flight, Z = A @ dy on v_mfma_f32_32x32x2_f32, Z rows in
    an LDS ring, 27 shifted adds per pixel) -- the sums of the tile kernel (ST2_DGRAD_FIRST=1) in the same order, bit for bit, and the
    oracle's to 2e-6; with and without a diff injected at the data blob; one partial strip, a second strip one pixel wide (127),
    several strips with ragged last strip / segment."""
    topo = (('conv', 'conv1_1', 3, 64),)
    params = oracle.he_init_weights(topo, seed=64 + h, bias_std=0.2)
    cpu = oracle.NetOracle(topo, params)
    rng = np.random.RandomState(h * w + 64)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)
    cases = [{n: rng.randn(*((1, 64, h, w) if n != 'data' else x.shape)).astype(F32) for n in names} for names in (['conv1_1'], ['conv1_1', 'data'])]
    got = {}
    for kernel in ('strip', 'tile'):
        if kernel == 'tile':
            monkeypatch.setenv('ST2_DGRAD_FIRST', '1')
        else:
            monkeypatch.delenv('ST2_DGRAD_FIRST', raising=False)
        monkeypatch.setenv('ST2_DGRAD_FIRST_Q', '0')
        gpu = st2.HipModel(params, topology=topo)
        f = gpu.forward(x, ['conv1_1'])
        got[kernel] = [gpu.backward(d) for d in cases]
    cpu.forward(x)
    cpu.adopt_forward_state(f)
    for d, a, b in zip(cases, got['strip'], got['tile']):
        assert np.array_equal(a, b)
        assert rel_l2(a, cpu.backward(d)) <= 2e-6


@pytest.mark.parametrize('cout,h,w', [(64, 64, 96), (64, 75, 100), (64, 8, 32), (24, 12, 20), (64, 23, 132), (62, 40, 260), (64, 256, 512)])
def test_first_conv_data_gradient_lds_dma_staging_equals_the_register_staged_kernel(cout, h, w, monkeypatch):
    """conv3x3_dgrad_smallM_dma (round 4: the 4-channel tile staged as aligned quads by LDS-DMA, one barrier per chunk) against the
    register-staged kernel it replaces where the width allows: the same sum in the same order (the compiler contracts multiply-adds
    differently in the two: equal to an ulp, not bit for bit) -- tiles cut by the right / bottom edge, a channel count that is not a
    multiple of the chunk (62), several tiles in x."""
    monkeypatch.setenv('ST2_DGRAD_FIRST_Q', '0')
    monkeypatch.setenv('ST2_DGRAD_FIRST', '0')
    topo = (('conv', 'conv1_1', 3, cout),)
    params = oracle.he_init_weights(topo, seed=cout + h, bias_std=0.2)
    gpu = st2.HipModel(params, topology=topo)
    rng = np.random.RandomState(h * w + cout)
    x = (rng.randn(1, 3, h, w) * 40).astype(F32)
    f = gpu.forward(x, ['conv1_1'])
    got = {}
    for names in (['conv1_1'], ['conv1_1', 'data']):
        diffs = {n: rng.randn(*(f[n].shape if n != 'data' else x.shape)).astype(F32) for n in names}
        for dma in ('1', '0'):
            monkeypatch.setenv('ST2_DGRAD_SMALLM_DMA', dma)
            got[dma] = gpu.backward(diffs)
        assert rel_l2(got['1'], got['0']) <= 3e-7, (names, rel_l2(got['1'], got['0']))
        assert np.isfinite(got['1']).all() and np.abs(got['1']).max() > 0


def test_ranged_backward_injection_rules():
    """worker.py:88-106: unmasked at the start blob, masked from above, pool and data blobs too."""
    topo = oracle.tiny_topology((8, 16), (2, 2), final_pool=True)
    cpu, gpu = make_models(topo, seed=5, bias_std=0.3)
    rng = np.random.RandomState(1)
    x = (rng.randn(1, 3, 18, 23) * 30).astype(F32)
    fc, fg = cpu.forward(x), gpu.forward(x)
    for name in fc:
        assert rel_l2(fg[name], fc[name]) <= 1e-5, name
    cases = (['pool2', 'conv2_1', 'conv1_2', 'pool1', 'data'], ['conv2_2'], ['conv1_1'], ['data'],
             ['pool1', 'conv1_1'], ['conv2_2', 'data'])
    for names in cases:
        diffs = {n: rng.randn(*fc[n].shape).astype(F32) for n in names}
        assert rel_l2(gpu.backward(diffs), cpu.backward(diffs)) <= 2e-5, names
    assert np.array_equal(gpu.backward({}), np.zeros_like(x))


def test_gram_matches_oracle():
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 128), ('pool', 'pool1'), ('conv', 'conv2_1', 128, 200))
    cpu, gpu = make_models(topo, seed=9)
    x = (np.random.RandomState(4).randn(1, 3, 37, 50) * 40).astype(F32)
    fc = cpu.forward(x)
    gpu.forward(x)
    for name in fc:
        g = gpu.engine.gram(name)
        ref = oracle.gram(fc[name])
        assert rel_l2(g, ref) <= 1e-5, name
        assert np.allclose(g, g.T, rtol=1e-5, atol=1e-7 * np.abs(g).max())


@pytest.mark.parametrize('h,w', [(32, 64), (64, 96), (8, 4), (96, 128)])
def test_gram_dma_pipeline_matches_oracle_and_register_staged_kernel(h, w, monkeypatch):
    """h*w % 32 == 0 takes the LDS-DMA Gram kernel (swizzled quads, b128 operand reads); every C-tile shape:
    64 (one 64-tile), 128, 200 (ragged 128-tiles), 512 (upper-triangular tiles mirrored on store)."""
    topo = (('conv', 'conv1_1', 3, 64), ('conv', 'conv1_2', 64, 128), ('conv', 'conv1_3', 128, 200), ('conv', 'conv1_4', 200, 512))
    cpu, gpu = make_models(topo, seed=12)
    x = (np.random.RandomState(h + w).randn(1, 3, h, w) * 40).astype(F32)
    fc = cpu.forward(x)
    gpu.forward(x)
    for name in fc:
        if name == 'data':
            continue
        g = gpu.engine.gram(name)
        assert rel_l2(g, oracle.gram(fc[name])) <= 1e-5, name
        assert np.array_equal(g, g.T), name              # mirrored tiles: exactly symmetric


# ------------------------------------------------- oracle objective on top of the HIP model (B2 seam)
def test_oracle_objective_over_hip_model_matches_golden():
    g = load('transfer_tiny.npz')
    topo, params, weights, content, style, init = tiny_setup(g)
    st = oracle.TransferOracle(st2.HipModel(params, topology=topo))
    st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
    st.set_weights(weights, json.loads(str(g['params_json'])))
    st.set_optimizer('adam', 10)
    for ev in (1, 2):
        loss, grad = st.opfunc(g['std_eval%d_x' % ev].copy())
        assert rel_l2(grad, g['std_eval%d_grad' % ev]) <= 1e-4
        assert np.isclose(loss, g['std_eval%d_loss' % ev], rtol=1e-4)


# --------------------------------------------------------------- the engine path (product) vs golden
def engine_transfer(g, kind, step, params):
    topo, net_params, weights, content, style, init = tiny_setup(g)
    st = st2.StyleTransfer(st2.HipModel(net_params, topology=topo))
    st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
    st.set_weights(weights, params)
    st.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[kind]
    st.set_step_size(step)
    st.reset()
    assert st.start()
    return st


@pytest.mark.parametrize('tag', ['std', 'odd'])
def test_engine_opfunc_two_evals_match_reference_vectors(tag):
    """First evaluation captures the norms, the second uses them frozen (worker.py:253-275)."""
    g = load('transfer_tiny.npz')
    params = json.loads(str(g['params_json' if tag == 'std' else 'params_odd_json']))
    st = engine_transfer(g, 'adam', 10, params)
    for ev in (1, 2):
        loss, grad = st.opfunc(g['%s_eval%d_x' % (tag, ev)])
        assert rel_l2(grad, g['%s_eval%d_grad' % (tag, ev)]) <= 1e-4, ev
        assert np.isclose(loss, g['%s_eval%d_loss' % (tag, ev)], rtol=1e-4), ev
        check_trace(g['%s_eval%d_trace_keys' % (tag, ev)], g['%s_eval%d_trace_vals' % (tag, ev)],
                    st.traces[-1].data, rtol=2e-4)
    loss = st.opfunc(None, return_grad=False)
    assert list(st.traces[-1].data)[-4:] == ['scd_loss', 't_loss', 'p_loss', 'loss']


@pytest.mark.parametrize('p_power,tv_power', [(2.5, 1.7), (3, 2), (1, 2.2), (7.0, 1.0)])
def test_image_terms_with_integral_and_fractional_exponents(p_power, tv_power):
    """TV / p-norm pass (utils.py:285-304 behind worker.py:283-301): integral p-norm exponents run by repeated multiplication,
    fractional ones (and every TV exponent but 2) through powf -- both against the CPU oracle's objective on the same state, two
    evaluations (norm capture, then frozen norms), on an image whose size is no multiple of the pass's 4 x 256 tile."""
    g = load('transfer_tiny.npz')
    topo, net_params, weights, content, style, init = tiny_setup(g)
    params = {'p': 7.0, 'p_power': p_power, 'tv': 3.0, 'tv_power': tv_power}
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, net_params))
    dev = st2.StyleTransfer(st2.HipModel(net_params, topology=topo))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params)
    cpu.set_optimizer('adam', 10)
    dev.optimizer_cls = st2.AdamOptimizer; dev.set_step_size(10); dev.reset()
    assert dev.start()
    x = g['std_eval1_x'].copy()
    for ev in (1, 2):
        lo, go = cpu.opfunc(x.copy())
        ld, gd = dev.opfunc(x.copy())
        assert rel_l2(gd, go) <= 1e-4, (ev, rel_l2(gd, go))
        assert np.isclose(ld, lo, rtol=1e-4)
        for k in ('t_loss', 'p_loss', 't_grad', 'p_grad'):
            assert np.isclose(dev.traces[-1].data[k], cpu.traces[-1].data[k], rtol=2e-4, atol=1e-12), (k, dev.traces[-1].data[k], cpu.traces[-1].data[k])
        x = x + 3.0 * np.sign(go).astype(F32)


@pytest.mark.parametrize('h,w', [(64, 96), (50, 72), (18, 22)])
def test_big_style_gradient_kernel_matches_the_lds_dma_kernels(h, w, monkeypatch):
    """style_grad_big_k (64-bit addressing, register-staged: the style gradient of a blob of 4 GiB or more -- conv1_1 .. conv3_1 of an
    8192 x 8192 image in one engine) forced at test size (ST2_STYLE_FORCE_BIG=1) against the LDS-DMA kernels it stands in for: the
    whole objective twice (first evaluation: raw S and the norm; second: the fused saxpy, accumulated onto a content term), tiles cut
    by the last pixels, channel counts 64 / 128 / 256."""
    topo = oracle.VGG19_TOPOLOGY[:7]
    net_params = oracle.he_init_weights(topo, seed=5, bias_std=0.1)
    weights = {'content': {'conv2_1': 0.3}, 'style': {'conv1_1': 1, 'conv2_1': 0.7, 'conv3_1': 1.5}, 'deepdream': {}}
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (40, 36, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    got = {}
    for big in ('0', '1'):
        monkeypatch.setenv('ST2_STYLE_FORCE_BIG', big)
        dev = st2.StyleTransfer(st2.HipModel(net_params, topology=topo))
        dev.set_input(init); dev.set_content(content); dev.set_style(style); dev.reset()
        dev.set_weights(weights, TILED_PARAMS)
        l1, g1 = dev.opfunc()
        x2 = dev.engine.get_input_nchw() + F32(2.0) * np.sign(g1)
        l2, g2 = dev.opfunc(x2)
        got[big] = (l1, g1, l2, g2, dict(dev.traces[-1].data))
    a, b = got['0'], got['1']
    assert np.isclose(a[0], b[0], rtol=1e-6) and np.isclose(a[2], b[2], rtol=1e-6)
    assert rel_l2(b[1], a[1]) <= 2e-6 and rel_l2(b[3], a[3]) <= 2e-6, (rel_l2(b[1], a[1]), rel_l2(b[3], a[3]))
    for k in a[4]:
        if k != 'time':
            assert np.isclose(b[4][k], a[4][k], rtol=1e-5, atol=1e-12), (k, b[4][k], a[4][k])


@pytest.mark.parametrize('weights', [
    {'content': {}, 'style': {}, 'deepdream': {}},                                     # image terms only: no layer is visited
    {'content': {}, 'style': {}, 'deepdream': {'conv1_1': 0.3}},                       # the shallowest blob only
    {'content': {'conv2_2': 1.0}, 'style': {}, 'deepdream': {}},                       # one deep content layer, no style at all
    {'content': {}, 'style': {'pool1': 2.0}, 'deepdream': {}},                         # a style term on a pool blob only
])
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_degenerate_weight_tables(weights, precision):
    """SetWeights tables the web UI can produce by zeroing sliders (worker.py:231-247 skips layers whose three weights are all
    below 1e-6; with none left only the TV / p-norm terms remain): loss, gradient, trace keys and one Adam step against the oracle."""
    g = load('transfer_tiny.npz')
    topo, net_params, _, content, style, init = tiny_setup(g)
    params = json.loads(str(g['params_json']))
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, net_params, operands='bf16' if precision == 'bf16' else 'fp32'))
    dev = st2.StyleTransfer(st2.HipModel(net_params, topology=topo, precision=precision))
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params)
    cpu.set_optimizer('adam', 10)
    dev.optimizer_cls = st2.AdamOptimizer; dev.set_step_size(10); dev.reset()
    assert cpu.start() and dev.start()
    x = g['std_eval1_x'].copy()
    lo, go = cpu.opfunc(x.copy())
    ld, gd = dev.opfunc(x.copy())
    tol = 2e-3 if precision == 'bf16' else 1e-4
    assert np.isclose(ld, lo, rtol=tol) and rel_l2(gd, go) <= tol, (ld, lo, rel_l2(gd, go))
    assert list(dev.traces[-1].data) == list(cpu.traces[-1].data)
    ic, tc = cpu.step()
    idv, td = dev.step()
    assert list(td) == list(tc) and np.isclose(td['loss'], tc['loss'], rtol=tol)
    assert np.mean((idv - ic) ** 2) <= 1.0


def test_engine_adam_trajectory_matches_reference_vectors():
    """50 Adam steps.  Adam's first steps are sign-like (x -= 10 g/|g|), so pixels whose gradient is at
    fp32 noise level may flip: tight bar on the per-step loss, loose bar on the image (MSE in 0-255
    units <= 1.0 against an image that moves by hundreds of levels)."""
    g = load('transfer_tiny.npz')
    st = engine_transfer(g, 'adam', 10, json.loads(str(g['params_json'])))
    losses, images = [], []
    for i in range(50):
        image, trace = st.step()
        losses.append(trace['loss'])
        if i in (0, 4, 49):
            images.append(image)
    assert np.allclose(losses, g['adam_losses'], rtol=5e-3)
    assert np.isclose(losses[0], g['adam_losses'][0], rtol=1e-4)
    for got, ref in zip(images, g['adam_images']):
        assert np.mean((got - ref) ** 2) <= 1.0
    assert trace['fevals'] == 50
    assert list(trace) == [str(k) for k in g['adam_last_trace_keys']]


def test_engine_lbfgs_trajectory_matches_reference_vectors():
    g = load('transfer_tiny.npz')
    st = engine_transfer(g, 'lbfgs', 1, json.loads(str(g['params_json'])))
    losses, images = [], []
    for i in range(20):
        image, trace = st.step()
        losses.append(trace['loss'])
        if i in (0, 4, 19):
            images.append(image)
    assert np.allclose(losses[:5], g['lbfgs_losses'][:5], rtol=1e-3)
    assert np.allclose(losses, g['lbfgs_losses'], rtol=5e-2)
    assert np.mean((images[0] - g['lbfgs_images'][0]) ** 2) <= 1e-2
    assert np.mean((images[-1] - g['lbfgs_images'][-1]) ** 2) <= 25.0
    assert list(trace) == [str(k) for k in g['lbfgs_last_trace_keys']]


def test_engine_objective_changed_and_same_shape_input_replacement():
    """set_input with an equal shape keeps Adam's v, clears m (optimizers.py:42-46, worker.py:193-195)."""
    g = load('transfer_tiny.npz')
    topo, net_params, weights, content, style, init = tiny_setup(g)
    params = json.loads(str(g['params_json']))
    ora = oracle.TransferOracle(oracle.NetOracle(topo, net_params))
    dev = engine_transfer(g, 'adam', 10, params)
    ora.set_input(init); ora.set_content(content); ora.set_style(style); ora.reset()
    ora.set_weights(weights, params); ora.set_optimizer('adam', 10); ora.start()
    other = np.random.RandomState(7).randint(0, 256, init.shape).astype(np.uint8)
    for i in range(6):
        if i == 3:
            ora.set_input(other)
            dev.set_input(other)
        io, to = ora.step()
        idv, td = dev.step()
        assert np.isclose(td['loss'], to['loss'], rtol=2e-3), i
    assert np.mean((idv - io) ** 2) <= 1.0


def test_content_features_dropped_by_set_weights_come_back_when_a_later_table_needs_them():
    """The reference keeps the content features of every blob (worker.py:204-209); the engine keeps those a content weight reads and
    the content image, and takes the others again when a later SetWeights asks for them (12 -> 0.3 GB at 1024^2 with the default
    table).  Oracle and device side by side through three weight tables: content on conv2_2, on conv1_2 + conv2_2 + data, on none."""
    g = load('transfer_tiny.npz')
    topo, net_params, weights, content, style, init = tiny_setup(g)
    params = json.loads(str(g['params_json']))
    names = [l[1] for l in topo]
    ora = oracle.TransferOracle(oracle.NetOracle(topo, net_params))
    dev = engine_transfer(g, 'adam', 10, params)
    ora.set_input(init); ora.set_content(content); ora.set_style(style); ora.reset()
    ora.set_weights(weights, params); ora.set_optimizer('adam', 10); ora.start()
    deepest, first = names[-1], names[1]
    tables = [{'content': {deepest: 0.08}, 'style': {names[0]: 1.0}, 'deepdream': {}},
              {'content': {first: 0.5, deepest: 0.08, 'data': 0.01}, 'style': {names[0]: 1.0}, 'deepdream': {}},
              {'content': {}, 'style': {names[0]: 1.0, deepest: 0.5}, 'deepdream': {first: 0.02}},
              {'content': {first: 0.5}, 'style': {names[0]: 1.0}, 'deepdream': {}}]
    for k, table in enumerate(tables):
        ora.set_weights(table, params); dev.set_weights(table, params)
        ora.reset(); dev.reset()
        for i in range(2):
            io, to = ora.step()
            idv, td = dev.step()
            assert list(td) == list(to), k
            assert np.isclose(td['loss'], to['loss'], rtol=2e-4), (k, i, td['loss'], to['loss'])
        assert np.mean((idv - io) ** 2) <= 1e-2, k


# ----------------------------------------------------------------------- full VGG19, small image
def test_vgg19_gradient_matches_oracle_at_96x128():
    topo = oracle.VGG19_TOPOLOGY
    params = oracle.he_init_weights(topo, seed=0)
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, params, full_forward=False))
    dev = st2.StyleTransfer(st2.HipModel(params))
    rs = np.random.RandomState
    content = rs(1).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    style = rs(2).randint(0, 256, (80, 112, 3)).astype(np.uint8)
    init = rs(3).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    weights = {'content': {'conv4_2': 0.08},
               'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    params4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params4)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    assert rel_l2(gd, go) <= 1e-4
    assert np.isclose(ld, lo, rtol=1e-4)
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=1e-3)
    # second evaluation with frozen norms, after moving the image
    x2 = cpu.input + F32(2.0) * np.sign(go)
    lo, go = cpu.opfunc(x2)
    ld, gd = dev.opfunc(x2)
    assert rel_l2(gd, go) <= 1e-4


# ------------------------------------------------- full-size (1024^2) size-independent properties
def test_full_size_1024_properties():
    """At BASELINE.json's size the oracle is too slow for a full comparison; check properties that do
    not depend on size: locality (a crop evaluated by the ORACLE equals the same window of the
    full-size HIP blobs away from the crop border), linearity of the ranged backward, Gram trace."""
    topo = oracle.VGG19_TOPOLOGY[:4]            # conv1_1, conv1_2, pool1, conv2_1 at full resolution
    params = oracle.he_init_weights(topo, seed=0)
    cpu, gpu = oracle.NetOracle(topo, params), st2.HipModel(params, topology=topo)
    x = (np.random.RandomState(0).rand(1, 3, 1024, 1024) * 255 - 120).astype(F32)
    fg = gpu.forward(x)
    y0, x0, s = 384, 640, 64
    crop = np.ascontiguousarray(x[:, :, y0:y0 + s, x0:x0 + s])
    fc = cpu.forward(crop)
    m = 4                                        # conv1_1+conv1_2(+conv2_1 at half res) receptive margin
    assert rel_l2(fg['conv1_2'][0, :, y0 + m:y0 + s - m, x0 + m:x0 + s - m], fc['conv1_2'][0, :, m:-m, m:-m]) <= 1e-5
    h0, hx = y0 // 2, x0 // 2
    assert rel_l2(fg['conv2_1'][0, :, h0 + m:h0 + s // 2 - m, hx + m:hx + s // 2 - m], fc['conv2_1'][0, :, m:-m, m:-m]) <= 1e-5
    # linearity of backward in the injected diffs
    rng = np.random.RandomState(5)
    d1 = {'conv2_1': rng.randn(*fg['conv2_1'].shape).astype(F32)}
    d2 = {'conv2_1': rng.randn(*fg['conv2_1'].shape).astype(F32)}
    b1, b2 = gpu.backward(d1), gpu.backward(d2)
    b12 = gpu.backward({'conv2_1': F32(2) * d1['conv2_1'] - F32(0.5) * d2['conv2_1']})
    assert rel_l2(b12, F32(2) * b1 - F32(0.5) * b2) <= 1e-5
    # Gram: trace(G) * n == sum F^2
    gpu.forward(x)
    G = gpu.engine.gram('conv1_1')
    F = fg['conv1_1'].astype(np.float64)
    assert np.isclose(np.trace(G.astype(np.float64)) * F.size, (F ** 2).sum(), rtol=1e-5)


# ------------------------------------------------ BASELINE config 1: the reference's own example images
def test_config1_golden_gate_starry_night_256px_adam_iters():
    """configs[0]: examples/golden_gate.jpg + starry_night.jpg resized by the reference's resize_to_fit to
    fit 256 (192x256 content, 160x256 style; fixture tests/golden/config1_inputs.npz), VGG19 (seeded
    synthetic weights), initial_weights.yaml losses, Adam step 10: HIP engine vs CPU oracle, all 50 iterations (round 5; 30 until
    round 4; `bench.py --examples` runs them with the oracle timed beside the device).
    Tight bar on the per-step loss while the trajectories coincide, loose image bar (Adam is sign-like)."""
    g = np.load(__import__('os').path.join(__import__('helpers').GOLDEN, 'config1_inputs.npz'))
    content, style = g['golden_gate'], g['starry_night']
    init = np.random.RandomState(3).randint(0, 256, content.shape).astype(np.uint8)   # app.py:82,251 noise init
    topo = oracle.VGG19_TOPOLOGY
    params = oracle.he_init_weights(topo, seed=0)
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1},
               'deepdream': {}}
    params4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    # the oracle's 50 iterations are stored (tests/golden/make_trajectories.py: oracle.TransferOracle on these very inputs;
    # tests/test_oracle_golden.py re-runs the first ones on the CPU)
    traj = __import__('helpers').load('oracle_trajectories.npz')
    lc, ic = list(traj['config1_losses']), traj['config1_final']
    first = dict(zip([str(k) for k in traj['config1_first_keys']], traj['config1_first_values']))
    dev = st2.StyleTransfer(st2.HipModel(params))
    dev.set_input(init); dev.set_content(content); dev.set_style(style); dev.reset()
    dev.set_weights(weights, params4)
    dev.optimizer_cls = st2.AdamOptimizer; dev.set_step_size(10); dev.reset()
    assert dev.start()
    ld = []
    assert len(lc) == 50
    for i in range(50):
        idv, td = dev.step()
        ld.append(td['loss'])
        if i == 0:
            assert [str(k) for k in td] == list(first)
            assert np.isclose(td['loss'], first['loss'], rtol=1e-4) and np.isclose(td['grad'], first['grad'], rtol=1e-3)
    assert np.allclose(ld[:10], lc[:10], rtol=2e-3)
    assert np.allclose(ld, lc, rtol=2e-2)
    assert idv.shape == (192, 256, 3) and idv.dtype == F32
    assert np.mean((idv - ic) ** 2) <= 4.0        # 0-255^2 units; the image moved by thousands
    assert np.mean((ic - init) ** 2) > 1000.0


# ----------------------------------------------------------- tile-sharded mode (BASELINE config 5) on the GPU
TILED_TOPO = oracle.tiny_topology((8, 16), (2, 2))
TILED_WEIGHTS = {'content': {'conv2_2': 0.08, 'conv1_2': 0.5}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'pool1': 0.7},
                 'deepdream': {'conv2_1': 0.02}}
TILED_PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}


def _tiled_images(h, w):
    rs = np.random.RandomState
    return (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (20, 28, 3)).astype(np.uint8),
            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))


def test_tiled_single_rank_equals_plain_engine():
    """A 1x1 grid (tile = whole image, ring = the image's own periodic wrap) must reproduce the ordinary
    engine step: same kernels, reductions routed through the tile phases."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 32, 48
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    tt = tiled.TiledTransfer(grid, 0, HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS,
                                                     step_size=10, topology=TILED_TOPO), tiled.Comm())
    ref = st2.StyleTransfer(st2.HipModel(params, topology=TILED_TOPO))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(TILED_WEIGHTS, TILED_PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    for i in range(4):
        vals = tt.step()
        img, tr = ref.step()
        assert np.isclose(vals[-2], tr['loss'], rtol=1e-5), i
        assert np.isclose(vals[-1], tr['grad'], rtol=1e-5), i
        assert np.allclose(tt.tile_image(), img, rtol=0, atol=2e-3), i


@pytest.mark.parametrize('h,w', [(4176, 2208), (4176, 2128)])
def test_production_window_of_configs4_through_the_tile_phases_equals_the_plain_engine(h, w):
    """The two window shapes a rank of the 8192^2 / 2 x 4 job holds -- 4176 x 2208 (a column with neighbours on both sides; levels
    2208 .. 138 wide) and 4176 x 2128 (an edge column; levels 2128, 1064, 532, 266, 133: the any-width conv variants) -- as a 1 x 1
    grid through st_tile_step (solo transport), VGG19 fp32, against the plain engine on the same image: one Adam iteration."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (96, 80, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    params = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    net_params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    ref = st2.StyleTransfer(st2.HipModel(net_params))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(weights, params)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    img, tr = ref.step()
    img = np.asarray(img, F32).copy()
    del ref
    __import__('gc').collect()
    grid = tiling.TileGrid(h, w, 1, 1, oracle.VGG19_TOPOLOGY, 17)
    backend = HipTileBackend(net_params, grid, 0, content, style, init, weights, params, step_size=10)
    backend.comm_init_solo(0, 1)
    tt = tiled.FusedTiledTransfer(grid, 0, backend)
    vals = tt.step()
    assert np.isclose(vals[-2], tr['loss'], rtol=1e-5) and np.isclose(vals[-1], tr['grad'], rtol=1e-4), (vals[-2], tr['loss'])
    mse = float(np.mean((tt.tile_image().astype(np.float64) - img) ** 2))
    print('[window %dx%d] loss %.9g vs %.9g, image MSE %.3g' % (h, w, vals[-2], tr['loss'], mse))
    assert mse <= 0.05


def test_fused_tile_step_on_a_one_rank_rccl_communicator_equals_the_plain_engine(monkeypatch):
    """st_tile_step (every phase and collective enqueued by the engine) on a 1 x 1 grid with a REAL RCCL communicator of one rank:
    st_comm_unique_id / st_comm_init, ncclAllReduce on the phase buffers, and -- test hook ST2_COMM_SELF_VIA_RCCL -- the ring's
    periodic-wrap copies travelling as grouped ncclSend / ncclRecv to the own rank.  Must reproduce the ordinary engine step.
    (More ranks need more GPUs: the multi-rank tests below run the same engine code over a host-staged transport.)"""
    import ctypes
    from style_transfer2_amd import capi, tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    monkeypatch.setenv('ST2_COMM_SELF_VIA_RCCL', '1')
    h, w = 32, 48
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    backend = HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
    uid = ctypes.create_string_buffer(capi.COMM_ID_BYTES)
    capi.check(backend.lib.st_comm_unique_id(uid))
    assert tiled.rendezvous_unique_id(0, 1, lambda: uid.raw) == uid.raw
    backend.comm_init_rccl(uid.raw, 0, 1)
    ft = tiled.FusedTiledTransfer(grid, 0, backend)
    ref = st2.StyleTransfer(st2.HipModel(params, topology=TILED_TOPO))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(TILED_WEIGHTS, TILED_PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    for i in range(4):
        vals = ft.step()
        img, tr = ref.step()
        assert np.isclose(vals[-2], tr['loss'], rtol=1e-5), (i, vals[-2], tr['loss'])
        assert np.isclose(vals[-1], tr['grad'], rtol=1e-5), i
        assert np.allclose(ft.tile_image(), img, rtol=0, atol=2e-3), i
    backend.barrier()
    prof = backend.engine  # the communicator is released with the context
    capi.check(backend.lib.st_comm_destroy(backend.ctx))


@pytest.mark.parametrize('h,w', [(32, 48), (75, 100)])
def test_tiled_lbfgs_single_rank_equals_plain_engine(h, w):
    """optimizer='lbfgs' on a 1x1 grid (every all-reduce a no-op) against the engine's device-resident L-BFGS: the same
    optimizers.py:62-108 recursion, once as host-sequenced st_vec_dot / st_vec_axpy calls on tile vectors, once as the fused
    device state machine (lbfgs.hip).  12 steps: the pair memory (10) rolls over."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    tt = tiled.TiledTransfer(grid, 0, HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS,
                                                     step_size=1, topology=TILED_TOPO), tiled.Comm(), optimizer='lbfgs', step_size=1)
    ref = st2.StyleTransfer(st2.HipModel(params, topology=TILED_TOPO))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(TILED_WEIGHTS, TILED_PARAMS)
    ref.optimizer_cls = st2.LBFGSOptimizer; ref.set_step_size(1); ref.reset()
    assert ref.start()
    for i in range(12):
        vals = tt.step()
        img, tr = ref.step()
        # two fp32 implementations of a quasi-Newton path: tight while the history is short, then they drift apart slowly
        assert np.isclose(vals[-2], tr['loss'], rtol=1e-5 if i < 3 else 5e-3), (i, vals[-2], tr['loss'])
        assert np.mean((tt.tile_image() - img) ** 2) <= (1e-4 if i < 3 else 0.1), i


def test_tiled_bf16_lean_and_full_data_flows_are_bit_identical():
    """The tile phases with bf16 conv operands run the lean data flow (fp32 blobs / diffs only where the fp32 region-of-interest loss
    kernels read them, pools riding on their producing conv, ReLU masks from the bf16 copies); 'bf16-full' writes every fp32 tensor.
    Same arithmetic: identical traces and iterates, through the in-engine step."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 64, 96
    content, style, init = _tiled_images(h, w)
    topo = oracle.VGG19_TOPOLOGY[:7]
    params = oracle.he_init_weights(topo, 0, 0.1)
    weights = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1}, 'deepdream': {}}
    grid = tiling.TileGrid(h, w, 1, 1, topo, 5)
    runs = []
    for precision in ('bf16', 'bf16-full'):
        backend = HipTileBackend(params, grid, 0, content, style, init, weights, TILED_PARAMS, step_size=10, topology=topo, precision=precision)
        backend.comm_init_solo(0, 1)
        ft = tiled.FusedTiledTransfer(grid, 0, backend)
        runs.append([(ft.step(), ft.tile_image()) for _ in range(3)])
    for (va, ia), (vb, ib) in zip(*runs):
        assert np.array_equal(va, vb) and np.array_equal(ia, ib)
    assert np.isfinite(runs[0][-1][0]).all()


def test_tiled_bf16_style_term_on_the_bf16_matrix_cores_tracks_the_fp32_region_kernels(monkeypatch):
    """Tile phases, bf16 operands: the style term's two GEMMs in their region-of-interest bf16 forms (default) against the fp32
    region-of-interest kernels on fp32 blobs (ST2_TILE_STYLE16=0), same windows, same convs: the loss and the iterate agree to the
    accuracy of a bf16-rounded feature operand."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 96, 160
    content, style, init = _tiled_images(h, w)
    topo = oracle.VGG19_TOPOLOGY[:7]
    params = oracle.he_init_weights(topo, 0, 0.1)
    weights = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1}, 'deepdream': {}}
    grid = tiling.TileGrid(h, w, 1, 1, topo, 5)
    runs = {}
    for flag in ('1', '0'):
        monkeypatch.setenv('ST2_TILE_STYLE16', flag)
        backend = HipTileBackend(params, grid, 0, content, style, init, weights, TILED_PARAMS, step_size=10, topology=topo, precision='bf16')
        backend.comm_init_solo(0, 1)
        ft = tiled.FusedTiledTransfer(grid, 0, backend)
        runs[flag] = [(ft.step(), ft.tile_image()) for _ in range(3)]
    for (va, ia), (vb, ib) in zip(runs['1'], runs['0']):
        assert np.isclose(va[-2], vb[-2], rtol=2e-3), (va[-2], vb[-2])
        assert not np.array_equal(va, vb)                        # other kernels really ran
        assert np.mean((ia - ib) ** 2) <= 1.0


def test_tiled_single_rank_with_bf16_convs_tracks_the_bf16_engine():
    """precision='bf16' in the tile backend: the window's convs on the bf16 matrix cores, Gram / style / loss kernels in their fp32
    region-of-interest forms.  Against the plain engine in its bf16 mode (whose Gram and style gradient read the bf16 copies instead):
    the same objective to bf16 accuracy."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 64, 96
    content, style, init = _tiled_images(h, w)
    topo = oracle.VGG19_TOPOLOGY[:7]
    params = oracle.he_init_weights(topo, 0, 0.1)
    weights = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1}, 'deepdream': {}}
    grid = tiling.TileGrid(h, w, 1, 1, topo, 5)
    tt = tiled.TiledTransfer(grid, 0, HipTileBackend(params, grid, 0, content, style, init, weights, TILED_PARAMS,
                                                     step_size=10, topology=topo, precision='bf16'), tiled.Comm())
    ref = st2.StyleTransfer(st2.HipModel(params, topology=topo, precision='bf16'))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(weights, TILED_PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    f32 = st2.StyleTransfer(st2.HipModel(params, topology=topo))
    f32.set_input(init); f32.set_content(content); f32.set_style(style); f32.reset()
    f32.set_weights(weights, TILED_PARAMS)
    f32.optimizer_cls = st2.AdamOptimizer; f32.set_step_size(10); f32.reset()
    assert f32.start()
    for i in range(3):
        vals = tt.step()
        img, tr = ref.step()
        _, tr32 = f32.step()
        assert np.isclose(vals[-2], tr['loss'], rtol=2e-3), (i, vals[-2], tr['loss'])
        assert np.mean((tt.tile_image() - img) ** 2) <= 1.0, i
        if i == 0:
            assert vals[-2] != tr32['loss'] and np.isclose(vals[-2], tr32['loss'], rtol=2e-2)      # bf16 operands really are in use


def _tiled_gpu_rank(rank, world, rows, cols, port, steps, h, w, q, optimizer='adam', fused=False):
    import os, sys
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    dist.init_process_group('gloo', rank=rank, world_size=world)      # one GPU here: ranks share it, data staged via host
    content, style, init = _tiled_images(h, w)
    grid = tiling.TileGrid(h, w, rows, cols, TILED_TOPO, 5)
    backend = HipTileBackend(oracle.he_init_weights(TILED_TOPO, 0, 0.1), grid, rank, content, style, init,
                             TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
    if fused:       # the iteration with its communication inside the engine (st_tile_step); the transport is host-staged gloo here
        backend.comm_init_callbacks(dist, rank, world)
        tt = tiled.FusedTiledTransfer(grid, rank, backend)
    else:
        tt = tiled.TiledTransfer(grid, rank, backend, tiled.Comm(dist, rank, world), optimizer=optimizer,
                                 step_size={'adam': 10, 'lbfgs': 1}[optimizer])
    res = []
    for _ in range(steps):
        vals = tt.step()
        res.append((tt.tile_image(), vals))
    q.put((rank, tuple(grid.tiles[rank]), res))
    dist.barrier()
    dist.destroy_process_group()


def test_tiled_lbfgs_two_ranks_on_one_gpu_match_oracle():
    """Two processes share the GPU, each with its tile of x, of the gradient and of the curvature pairs; the dot products of the
    two-loop recursion cross ranks as scalar all-reduces (gloo here, RCCL on a node).  Against the single-process CPU oracle."""
    import torch.multiprocessing as mp
    h, w, steps, world = 32, 48, 6, 2
    content, style, init = _tiled_images(h, w)
    cpu = oracle.TransferOracle(oracle.NetOracle(TILED_TOPO, oracle.he_init_weights(TILED_TOPO, 0, 0.1)))
    cpu.set_input(init); cpu.set_content(content); cpu.set_style(style); cpu.reset()
    cpu.set_weights(TILED_WEIGHTS, TILED_PARAMS); cpu.set_optimizer('lbfgs', 1)
    assert cpu.start()
    ref = []
    for _ in range(steps):
        img, tr = cpu.step()
        ref.append((np.asarray(img, F32).copy(), dict(tr)))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29100 + __import__('os').getpid() % 150
    procs = [ctx.Process(target=_tiled_gpu_rank, args=(r, world, 1, 2, port, steps, h, w, q, 'lbfgs')) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for step in range(steps):
        full = np.zeros_like(ref[step][0])
        for rank, (y0, x0, y1, x1), res in got:
            full[y0:y1, x0:x1] = res[step][0]
            assert np.isclose(res[step][1][-2], ref[step][1]['loss'], rtol=1e-4 if step < 3 else 1e-2), (step, rank)
        assert np.mean((full - ref[step][0]) ** 2) <= (1e-3 if step < 3 else 1.0), step


@pytest.mark.parametrize('rows,cols,fused', [(1, 2, False), (2, 2, False), (1, 2, True), (2, 2, True)])
def test_tiled_multi_rank_on_one_gpu_matches_oracle(rows, cols, fused):
    """2 / 4 processes share the GPU (each with its own engine + window), exchange through gloo, and must
    reproduce the single-process CPU oracle on the whole image."""
    import torch.multiprocessing as mp
    h, w, steps, world = 32, 48, 3, rows * cols
    content, style, init = _tiled_images(h, w)
    cpu = oracle.TransferOracle(oracle.NetOracle(TILED_TOPO, oracle.he_init_weights(TILED_TOPO, 0, 0.1)))
    cpu.set_input(init); cpu.set_content(content); cpu.set_style(style); cpu.reset()
    cpu.set_weights(TILED_WEIGHTS, TILED_PARAMS); cpu.set_optimizer('adam', 10)
    assert cpu.start()
    ref = []
    for _ in range(steps):
        img, tr = cpu.step()
        ref.append((np.asarray(img, F32).copy(), dict(tr)))
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29900 + (__import__('os').getpid() + rows * 5 + cols + 17 * fused) % 1000
    procs = [ctx.Process(target=_tiled_gpu_rank, args=(r, world, rows, cols, port, steps, h, w, q, 'adam', fused)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for step in range(steps):
        full = np.zeros_like(ref[step][0])
        for rank, (y0, x0, y1, x1), res in got:
            full[y0:y1, x0:x1] = res[step][0]
            assert np.isclose(res[step][1][-2], ref[step][1]['loss'], rtol=1e-4), (step, rank)
            assert np.isclose(res[step][1][-1], ref[step][1]['grad'], rtol=1e-3), (step, rank)
        assert np.mean((full - ref[step][0]) ** 2) <= 1.0, step
    assert np.allclose(full, ref[-1][0], rtol=0, atol=0.5) or np.mean(np.abs(full - ref[-1][0]) > 0.5) < 0.02


def test_phase_driven_and_fused_tile_drivers_agree_bit_for_bit():
    """Both drivers finish the trace through st_tile_trace from the same reduced sums: on a 1 x 1 grid the phase-by-phase driver and
    st_tile_step give the same trace and the same iterate, bit for bit.  TILED_WEIGHTS has content-only, style-only and pool rows and a
    style + deep-dream row: every slot kind of the objective's layout; step 1 takes the two-pass style-norm path, the others the steady one."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 32, 48
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    backends = [HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
                for _ in range(2)]
    phased = tiled.TiledTransfer(grid, 0, backends[0], tiled.Comm())
    backends[1].comm_init_solo(0, 1)
    fused = tiled.FusedTiledTransfer(grid, 0, backends[1])
    for i in range(4):
        vp, vf = phased.step(), fused.step()
        assert vp.shape == (backends[0].engine.trace_len(),) and np.all(np.isfinite(vp)) and vp[-2] > 0
        print('[step %d] largest relative trace difference between the drivers: %.3g' % (i, float(np.max(np.abs(vp - vf) / np.maximum(np.abs(vp), 1e-30)))))
        assert np.array_equal(vp, vf), i
        assert np.array_equal(phased.tile_image(), fused.tile_image()), i


def test_phase_driven_and_fused_tile_drivers_on_two_ranks_finish_the_same_trace_on_every_rank():
    """The 1 x 2 grid with both ranks as threads of this process: within a driver every rank finishes its trace from the same reduced
    sums -- identical vectors; across the drivers the transports may add the ranks' shares in another order -- the bars of
    test_tiled_multi_rank_on_one_gpu_matches_oracle."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w, steps, world = 32, 48, 3, 2
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 2, TILED_TOPO, 5)
    make = lambda r: HipTileBackend(params, grid, r, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
    out = {}
    for fused in (False, True):
        fabric, ranks = ThreadFabric(world), []
        for r in range(world):
            backend = make(r)
            if fused:
                backend.comm_init_host(r, world, lambda v, r=r: fabric.allreduce(r, v), lambda s, rc, r=r: fabric.exchange(r, s, rc))
                ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
            else:
                ranks.append(tiled.TiledTransfer(grid, r, backend, tiled.LocalComm(fabric, r)))
        out[fused] = _run_ranks_as_threads(ranks, steps, fabric)
        for step in range(steps):
            assert np.array_equal(out[fused][0][step][1], out[fused][1][step][1]), (fused, step)
    for step in range(steps):
        for r in range(world):
            (img_p, vp), (img_f, vf) = out[False][r][step], out[True][r][step]
            assert np.isclose(vp[-2], vf[-2], rtol=1e-4) and np.isclose(vp[-1], vf[-1], rtol=1e-3), (step, r)
            assert np.mean((img_p - img_f) ** 2) <= 1.0, (step, r)


def test_tile_trace_refuses_a_context_without_a_complete_evaluation():
    """st_tile_trace: ST_ERR_STATE before st_tile_configure and after st_tile_forward alone (the phase buffers hold no finished
    evaluation, at first or again after one); the NULL context is checked without a GPU in test_boundary.py."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    from ctypes import c_void_p
    h, w = 32, 48
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    plain = st2.HipModel(params, topology=TILED_TOPO).engine
    buf = np.zeros(64, np.float64)
    assert plain.lib.st_tile_trace(plain._ctx, buf.ctypes.data_as(c_void_p)) == 2 and b'st_tile_configure' in plain.lib.st_last_error()
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    backend = HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
    trace = lambda: backend.lib.st_tile_trace(backend.ctx, buf.ctypes.data_as(c_void_p))
    assert trace() == 2
    backend.forward_partials()
    assert trace() == 2 and b'complete evaluation' in backend.lib.st_last_error()
    tiled.TiledTransfer(grid, 0, backend, tiled.Comm()).step()
    assert trace() == 0 and backend.lib.st_tile_trace(backend.ctx, None) == 1
    backend.forward_partials()
    assert trace() == 2


def ThreadFabric(world, timeout=120.0):
    """tiled.InProcessFabric: every rank is a thread of this process (a GPU box admits six processes on its card; BASELINE configs[4]
    has eight ranks)."""
    from style_transfer2_amd import tiled
    return tiled.InProcessFabric(world, timeout)


def _run_ranks_as_threads(ranks, steps, fabric):
    """`steps` iterations of every FusedTiledTransfer in `ranks`, one thread per rank; [(tile image, trace values)] per rank."""
    from style_transfer2_amd import tiled
    return tiled.run_in_process(ranks, steps, fabric, on_step=lambda r, k, tt, vals: (tt.tile_image(), vals))


@pytest.mark.parametrize('precision,loss_rtol', [('fp32', 1e-4), ('bf16', 5e-3)])
def test_fused_tile_step_on_the_eight_rank_2x4_grid_matches_oracle(precision, loss_rtol):
    """BASELINE configs[4]'s layout -- 2 x 4 windows, corner and edge ranks with three and five grid neighbours -- on the HIP path:
    eight engine contexts in this process, one thread each, every iteration one st_tile_step per rank whose all-reduces and strip
    exchanges cross the ranks through ThreadFabric.  The stitched iterates against the single-process CPU oracle."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    rows, cols, h, w, steps = 2, 4, 64, 128, 3
    world = rows * cols
    content, style, init = _tiled_images(h, w)
    net_params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    cpu = oracle.TransferOracle(oracle.NetOracle(TILED_TOPO, net_params, operands='bf16' if precision == 'bf16' else 'fp32'))
    cpu.set_input(init); cpu.set_content(content); cpu.set_style(style); cpu.reset()
    cpu.set_weights(TILED_WEIGHTS, TILED_PARAMS); cpu.set_optimizer('adam', 10)
    assert cpu.start()
    ref = []
    for _ in range(steps):
        img, tr = cpu.step()
        ref.append((np.asarray(img, F32).copy(), dict(tr)))
    grid = tiling.TileGrid(h, w, rows, cols, TILED_TOPO, 5)
    fabric = ThreadFabric(world)
    ranks = []
    for r in range(world):
        backend = HipTileBackend(net_params, grid, r, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10,
                                 topology=TILED_TOPO, precision=precision)
        backend.comm_init_host(r, world, lambda v, r=r: fabric.allreduce(r, v), lambda s, rc, r=r: fabric.exchange(r, s, rc))
        ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
    neighbours = sorted(len(tiled.fused_plans(grid, r)[tiled.PLAN_OVERLAP]) for r in range(world))
    assert neighbours == [3, 3, 3, 3, 5, 5, 5, 5]
    out = _run_ranks_as_threads(ranks, steps, fabric)
    assert fabric.reduces >= 2 * steps and fabric.messages >= 3 * steps * sum(neighbours)
    for step in range(steps):
        full = np.zeros_like(ref[step][0])
        for r in range(world):
            t = grid.tiles[r]
            full[t.y0:t.y1, t.x0:t.x1] = out[r][step][0]
            assert np.isclose(out[r][step][1][-2], ref[step][1]['loss'], rtol=loss_rtol), (step, r)
            assert np.isclose(out[r][step][1][-1], ref[step][1]['grad'], rtol=10 * loss_rtol), (step, r)
            assert np.array_equal(np.asarray(out[r][step][1]), np.asarray(out[0][step][1]))    # every rank derives the same trace from the reduced sums
        assert np.mean((full - ref[step][0]) ** 2) <= 1.0, step


@pytest.mark.parametrize('h,w', [(32, 48), (75, 100)])
def test_fused_tile_lbfgs_on_a_1x1_grid_follows_the_engine_lbfgs(h, w, monkeypatch):
    """st_tile_step with an L-BFGS backend on a 1 x 1 grid (every all-reduce sees one rank, the ring is the image's own periodic wrap)
    against the plain engine's device-resident L-BFGS in the SAME (Gram) form: the same lbfgs.hip recursion, once on the window's
    vectors with the bookkeeping in one kernel, once on the compact tile vector with the sums handed through the all-reduce buffer
    (rounded to fp32 there, as sdot returns them).  12 steps: the pair memory (10) rolls over (optimizers.py:62-108)."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    monkeypatch.setenv('ST2_LBFGS_FORM', 'gram')
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 1, TILED_TOPO, 5)
    backend = HipTileBackend(params, grid, 0, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=1, topology=TILED_TOPO,
                             optimizer='lbfgs')
    backend.comm_init_solo(0, 1)
    ft = tiled.FusedTiledTransfer(grid, 0, backend)
    ref = st2.StyleTransfer(st2.HipModel(params, topology=TILED_TOPO))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(TILED_WEIGHTS, TILED_PARAMS)
    ref.optimizer_cls = st2.LBFGSOptimizer; ref.set_step_size(1); ref.reset()
    assert ref.start()
    for i in range(12):
        vals = ft.step()
        img, tr = ref.step()
        assert np.isclose(vals[-2], tr['loss'], rtol=1e-5 if i < 3 else 5e-3), (i, vals[-2], tr['loss'])
        assert np.mean((ft.tile_image() - img) ** 2) <= (1e-4 if i < 3 else 0.1), i


class _QuietFirst:
    """A FusedTiledTransfer whose first `n` iterations read nothing back (st_tile_step(ctx, NULL))."""
    def __init__(self, ft, n):
        self.ft, self.n, self.k = ft, n, 0

    def step(self):
        self.k += 1
        if self.k <= self.n:
            self.ft.step_async()
            return np.zeros(1)
        return self.ft.step()

    def tile_image(self):
        return self.ft.tile_image()


@pytest.mark.parametrize('optimizer', ['adam', 'lbfgs'])
@pytest.mark.parametrize('cols', [1, 2])
def test_fused_tile_step_without_a_trace_reads_nothing_back_and_changes_nothing(optimizer, cols):
    """st_tile_step(ctx, NULL): the device loop of a headless sharded job -- no trace, no host synchronisation.  Three iterations of
    which the first two are trace-less must leave the same tiles and the same third trace, bit for bit, as three iterations with their
    traces -- one rank and two.  The collective sequence is the SAME with and without a trace (round 5: until then a trace-less call
    skipped the all-reduce of the image-space sums, and ranks that disagreed on NULL for one iteration hung in RCCL instead of failing:
    ADVICE r4); the mixed case -- one rank asks for a trace, the other does not -- is the test below."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 64, 96
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, cols, TILED_TOPO, 5)
    results, reduces = [], []
    for quiet in (2, 0):
        fabric = ThreadFabric(cols)
        ranks = []
        for r in range(cols):
            backend = HipTileBackend(params, grid, r, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10 if optimizer == 'adam' else 1,
                                     topology=TILED_TOPO, optimizer=optimizer)
            if cols == 1:
                backend.comm_init_solo(0, 1)
            else:
                backend.comm_init_local(r, cols, fabric)
            ranks.append(_QuietFirst(tiled.FusedTiledTransfer(grid, r, backend), quiet))
        out = _run_ranks_as_threads(ranks, 3, fabric)
        results.append([(out[r][-1][0], np.asarray(out[r][-1][1])) for r in range(cols)])
        reduces.append(fabric.reduces)
    for r in range(cols):
        assert np.array_equal(results[0][r][0], results[1][r][0]) and np.array_equal(results[0][r][1], results[1][r][1]), r
    if cols > 1:
        assert reduces[0] == reduces[1], reduces              # same collectives either way


def test_ranks_may_disagree_on_asking_for_a_trace():
    """One rank of two passes trace == NULL for an iteration, the other does not: the iteration completes on both (same collectives)
    and leaves the tiles it leaves when both ask -- until round 5 this desynchronised the collective sequence."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w = 64, 96
    content, style, init = _tiled_images(h, w)
    params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    grid = tiling.TileGrid(h, w, 1, 2, TILED_TOPO, 5)
    results = []
    for quiet in ((1, 0), (0, 0)):
        fabric = ThreadFabric(2)
        ranks = []
        for r in range(2):
            backend = HipTileBackend(params, grid, r, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=10, topology=TILED_TOPO)
            backend.comm_init_local(r, 2, fabric)
            ranks.append(_QuietFirst(tiled.FusedTiledTransfer(grid, r, backend), quiet[r]))
        out = _run_ranks_as_threads(ranks, 2, fabric)
        results.append([(out[r][-1][0], np.asarray(out[r][-1][1])) for r in range(2)])
    for r in range(2):
        assert np.array_equal(results[0][r][0], results[1][r][0]) and np.array_equal(results[0][r][1], results[1][r][1]), r


@pytest.mark.parametrize('rows,cols', [(1, 2), (2, 4)])
def test_fused_tile_lbfgs_on_in_process_grids_follows_the_oracle(rows, cols):
    """The reference's default optimizer (worker.py:135-136) over the sharded image, fused: every rank one st_tile_step per iteration,
    the Gram-form recursion on its tile's vectors, ONE all-reduce of the new inner products per step (two on the first), every
    rank deriving the same coefficients.  Against the single-process CPU oracle (chain form, optimizers.py:62-108), 12 steps."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    h, w, steps = 64, 128, 12
    world = rows * cols
    content, style, init = _tiled_images(h, w)
    net_params = oracle.he_init_weights(TILED_TOPO, 0, 0.1)
    cpu = oracle.TransferOracle(oracle.NetOracle(TILED_TOPO, net_params))
    cpu.set_input(init); cpu.set_content(content); cpu.set_style(style); cpu.reset()
    cpu.set_weights(TILED_WEIGHTS, TILED_PARAMS); cpu.set_optimizer('lbfgs', 1)
    assert cpu.start()
    ref = []
    for _ in range(steps):
        img, tr = cpu.step()
        ref.append((np.asarray(img, F32).copy(), dict(tr)))
    grid = tiling.TileGrid(h, w, rows, cols, TILED_TOPO, 5)
    fabric = ThreadFabric(world)
    ranks = []
    for r in range(world):
        backend = HipTileBackend(net_params, grid, r, content, style, init, TILED_WEIGHTS, TILED_PARAMS, step_size=1, topology=TILED_TOPO,
                                 optimizer='lbfgs')
        backend.comm_init_local(r, world, fabric)
        ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
    out = _run_ranks_as_threads(ranks, steps, fabric)
    # per step: 2 (first evaluation: 3) all-reduces of the objective's sums + 1 of the inner products; the first step evaluates twice
    assert fabric.reduces <= 4 * steps + 4, fabric.reduces
    for step in range(steps):
        full = np.zeros_like(ref[step][0])
        for r in range(world):
            t = grid.tiles[r]
            full[t.y0:t.y1, t.x0:t.x1] = out[r][step][0]
            assert np.array_equal(np.asarray(out[r][step][1]), np.asarray(out[0][step][1]))    # every rank derives the same trace
        loss = out[0][step][1][-2]
        # two fp32 implementations of a quasi-Newton path (chain form on the CPU, Gram form here): tight while the history is short
        assert np.isclose(loss, ref[step][1]['loss'], rtol=1e-4 if step < 3 else 2e-2), (step, loss, ref[step][1]['loss'])
        assert np.mean((full - ref[step][0]) ** 2) <= (1e-3 if step < 3 else 1.0), step


@pytest.mark.parametrize('precision,loss_rtol,transport', [('fp32', 2e-5, 'device'), ('bf16', 5e-3, 'host')])
def test_fused_tile_step_vgg19_on_the_2x4_grid_matches_the_single_gpu_engine(precision, loss_rtol, transport):
    """The eight ranks of BASELINE configs[4] with the real network: VGG19 to conv5_1 (80-px aprons), a 2048 x 4096 image cut 2 x 4 --
    windows of 1104 x 1104 (corners) and 1104 x 1184 (the four ranks with neighbours on both sides), eight contexts on the one GPU,
    st_tile_step per rank and iteration, transport = ThreadFabric.  Against the plain engine on the whole image (the largest whose
    conv1 blobs stay below the 4 GiB the Winograd kernels index)."""
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    rows, cols, h, w, steps = 2, 4, 2048, 4096, 2
    world = rows * cols
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (96, 80, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    params = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    net_params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    ref = st2.StyleTransfer(st2.HipModel(net_params, precision=precision))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(weights, params)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    want = [ref.step() for _ in range(steps)]
    want = [(np.asarray(i, F32).copy(), dict(t)) for i, t in want]
    del ref
    __import__('gc').collect()
    grid = tiling.TileGrid(h, w, rows, cols, oracle.VGG19_TOPOLOGY, 17)
    assert sorted((wd.y1 - wd.y0, wd.x1 - wd.x0) for wd in grid.windows) == [(1104, 1104)] * 4 + [(1104, 1184)] * 4
    fabric = ThreadFabric(world, timeout=240.0)
    ranks = []
    for r in range(world):
        backend = HipTileBackend(net_params, grid, r, content, style, init, weights, params, step_size=10, precision=precision)
        if transport == 'device':       # device-to-device copies between the contexts' buffers (tiled.py: the one-GPU big-image driver)
            backend.comm_init_local(r, world, fabric)
        else:                           # staged through host arrays
            backend.comm_init_host(r, world, lambda v, r=r: fabric.allreduce(r, v), lambda s, rc, r=r: fabric.exchange(r, s, rc))
        ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
    out = _run_ranks_as_threads(ranks, steps, fabric)
    for step in range(steps):
        full = np.zeros_like(want[step][0])
        for r in range(world):
            t = grid.tiles[r]
            full[t.y0:t.y1, t.x0:t.x1] = out[r][step][0]
            assert np.isclose(out[r][step][1][-2], want[step][1]['loss'], rtol=loss_rtol), (step, r, out[r][step][1][-2], want[step][1]['loss'])
            assert np.isclose(out[r][step][1][-1], want[step][1]['grad'], rtol=1e-3 if precision == 'fp32' else 3e-2), (step, r)
        mse = float(np.mean((full.astype(np.float64) - want[step][0]) ** 2))
        print('[tiled 2x4 %dx%d %s] step %d: loss %.9g vs %.9g, image MSE %.3g' % (h, w, precision, step, out[0][step][1][-2], want[step][1]['loss'], mse))
        assert mse <= (0.25 if precision == 'fp32' else 1.0), (step, mse)


def test_configs4_full_size_8192_sharded_run_equals_one_engine_on_the_whole_image():
    """BASELINE configs[4] itself -- ONE 8192 x 8192 image, VGG19 to conv5_1, cut 2 x 4 into windows of 4176 x 2128 / 4176 x 2208 -- with
    all eight ranks resident on the one GPU (24.7 GB per fp32 window), one thread per rank, st_tile_step per rank and iteration,
    transport = ThreadFabric, against an INDEPENDENT reference: the plain engine on the whole image.  Round 3 had none (conv1 blobs of
    17 GB against 32-bit buffer offsets) and compared two shardings of the same code; since round 4 one engine addresses tensors of
    4 GiB and more (per-chunk buffer resources in the Winograd kernels, 32-bit element offsets up to 2^32 elements, a 64-bit-addressed
    style gradient), so the sharded run -- aprons, overlap-add, torus ring, all-reduced Gram sums -- is checked against a run that has
    none of them: same loss (rtol 2e-5) and the same image (MSE <= 0.25) after two Adam iterations."""
    import time
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 230 * 2 ** 30:
        pytest.skip('needs 230 GB of free HBM for eight 24.7 GB windows (free: %.0f GB)' % (free / 2 ** 30))
    h = w = 8192
    steps = 2
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (96, 80, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    params = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    net_params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    # ---- one engine on the whole image (the weights first: content features are then kept for conv4_2 only, 2 GB instead of 90)
    t0 = time.time()
    ref = st2.StyleTransfer(st2.HipModel(net_params))
    ref.set_weights(weights, params)
    ref.set_input(init); ref.set_content(content); ref.set_style(style)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    t1 = time.time()
    want = []
    for _ in range(steps):
        img, tr = ref.step()
        want.append((img, dict(tr)))
    t2 = time.time()
    used = (total - torch.cuda.mem_get_info()[0]) / 2 ** 30
    print('[configs[4] one engine, 8192 x 8192] build %.1f s, %d iterations %.2f s, HBM in use %.0f GB; losses %s'
          % (t1 - t0, steps, t2 - t1, used, ['%.9g' % tr['loss'] for _, tr in want]))
    ref_img = np.asarray(want[-1][0], F32).copy()
    ref.engine.close()
    del ref, img
    __import__('gc').collect()
    # ---- the 2 x 4 sharding
    rows, cols = 2, 4
    world = rows * cols
    grid = tiling.TileGrid(h, w, rows, cols, oracle.VGG19_TOPOLOGY, 17)
    fabric = ThreadFabric(world, timeout=300.0)
    backends, ranks = [], []
    t0 = time.time()
    for r in range(world):
        backend = HipTileBackend(net_params, grid, r, content, style, init, weights, params, step_size=10)
        backend.comm_init_local(r, world, fabric)
        backends.append(backend)
        ranks.append(tiled.FusedTiledTransfer(grid, r, backend))
    t1 = time.time()
    out = _run_ranks_as_threads(ranks, steps, fabric)
    t2 = time.time()
    full = np.zeros((h, w, 3), F32)
    for r in range(world):
        t = grid.tiles[r]
        full[t.y0:t.y1, t.x0:t.x1] = out[r][-1][0]
        for step in range(steps):
            assert np.array_equal(np.asarray(out[r][step][1]), np.asarray(out[0][step][1]))
    traces = [out[0][step][1] for step in range(steps)]
    used = (total - torch.cuda.mem_get_info()[0]) / 2 ** 30
    print('[configs[4] 2x4 on one GPU] windows %s; build %.1f s, %d iterations %.2f s (eight ranks time-sliced, device-to-device exchanges), HBM in use %.0f GB; losses %s'
          % (sorted({(wd.y1 - wd.y0, wd.x1 - wd.x0) for wd in grid.windows}), t1 - t0, steps, t2 - t1, used, ['%.9g' % v[-2] for v in traces]))
    for b_ in backends:
        b_.engine.close()
    del backends, ranks, out
    __import__('gc').collect()
    for step in range(steps):
        assert np.isclose(traces[step][-2], want[step][1]['loss'], rtol=2e-5), (step, traces[step][-2], want[step][1]['loss'])
        assert np.isclose(traces[step][-1], want[step][1]['grad'], rtol=1e-3), step
    mse = float(np.mean((full.astype(np.float64) - ref_img) ** 2))
    moved = float(np.mean((ref_img - init.astype(F32)) ** 2))
    print('[configs[4] sharded vs one engine] image MSE %.3g after %d Adam iterations (the image moved by MSE %.3g)' % (mse, steps, moved))
    assert mse <= 0.25 and moved > 50.0


def _tiled_vgg_rank(rank, world, port, steps, h, w, q, fused=False, precision='fp32'):
    import os
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch.distributed as dist
    from style_transfer2_amd import tiled, tiling
    from style_transfer2_amd.tile_backend import HipTileBackend
    dist.init_process_group('gloo', rank=rank, world_size=world)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (96, 80, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    topo = oracle.VGG19_TOPOLOGY
    grid = tiling.TileGrid(h, w, 1, 2, topo, 17)
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    backend = HipTileBackend(oracle.he_init_weights(topo, seed=0), grid, rank, content, style, init, weights,
                             {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}, step_size=10, precision=precision)
    if fused:
        backend.comm_init_callbacks(dist, rank, world)
        tt = tiled.FusedTiledTransfer(grid, rank, backend)
    else:
        tt = tiled.TiledTransfer(grid, rank, backend, tiled.Comm(dist, rank, world))
    res = []
    for _ in range(steps):
        vals = tt.step()
        res.append((tt.tile_image(), vals))
    q.put((rank, tuple(grid.tiles[rank]), tuple(grid.windows[rank]), res))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize('h,w,loss_rtol,fused,precision', [(176, 416, 1e-4, False, 'fp32'), (176, 416, 1e-4, True, 'fp32'), (1024, 4096, 2e-5, True, 'fp32'),
                                                           (176, 416, 5e-3, True, 'bf16'), (512, 2048, 5e-3, True, 'bf16')])
def test_tiled_vgg19_two_ranks_match_single_gpu_engine(h, w, loss_rtol, fused, precision):
    """Full VGG19 to conv5_1 (receptive-field apron 80 px): 2 ranks (1 x 2 grid) vs the plain engine on the whole image.
    176 x 416 is the quick case; 1024 x 4096 is BASELINE configs[4]'s per-rank GEOMETRY on the one GPU there is: windows of
    1024 x 2128 whose levels are 2128, 1064, 532, 266 and 133 wide (the any-width Winograd kernels, ceil-mode pools, 0.9 GB blobs),
    aprons, overlap-add, the torus ring of the TV term -- two ranks sharing the card over host-staged gloo, so still unmeasured on
    xGMI / RCCL hardware.  precision = 'bf16': the windows run the bf16 data flow of the plain engine -- bf16 conv operands, lean fp32
    tensors, the Gram partials and the style gradient on the bf16 matrix cores in their region-of-interest forms (gram16.hip /
    style16.hip: only the tile's pixels of each style blob are contracted / written) -- against the plain engine in its bf16 mode."""
    import torch.multiprocessing as mp
    steps = 2
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (h, w, 3)).astype(np.uint8), rs(2).randint(0, 256, (96, 80, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (h, w, 3)).astype(np.uint8))
    weights = {'content': {'conv4_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1},
               'deepdream': {}}
    ref = st2.StyleTransfer(st2.HipModel(oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0), precision=precision))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(weights, {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2})
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    want = [ref.step() for _ in range(steps)]
    want = [(np.asarray(i, F32).copy(), dict(t)) for i, t in want]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29300 + (__import__('os').getpid() + 7 * fused + h + 13 * (precision == 'bf16')) % 500
    procs = [ctx.Process(target=_tiled_vgg_rank, args=(r, 2, port, steps, h, w, q, fused, precision)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=400) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, tile, window, res in got:
        assert window[3] - window[1] == w // 2 + 80       # tile + the 80-px apron on its inner side
    for step in range(steps):
        full = np.zeros_like(want[step][0])
        for rank, (y0, x0, y1, x1), window, res in got:
            full[y0:y1, x0:x1] = res[step][0]
            assert np.isclose(res[step][1][-2], want[step][1]['loss'], rtol=loss_rtol), (step, rank, res[step][1][-2], want[step][1]['loss'])
            assert np.isclose(res[step][1][-1], want[step][1]['grad'], rtol=1e-3 if precision == 'fp32' else 3e-2), (step, rank)
        mse = float(np.mean((full.astype(np.float64) - want[step][0]) ** 2))
        print('[tiled %dx%d] step %d: loss %.9g vs %.9g, image MSE %.3g, pixels off by > 1: %.2e' % (
            h, w, step, got[0][3][step][1][-2], want[step][1]['loss'], mse, float(np.mean(np.abs(full - want[step][0]) > 1.0))))
        assert mse <= (1.0 if (h < 1024 or precision == 'bf16') else 0.25), (step, mse)   # 0..255 units; Adam's first steps are sign-like (a flipped tiny gradient = 20 levels)


def test_vgg19_odd_default_size_225x300_unaligned_paths():
    """The reference's default initial_size = 300 gives 225 x 300 (config.ini:16): widths 300, 150, 75, 38, 19 exercise
    ceil-mode pooling with clipped windows and the un-aligned (dword DMA) conv variants at VGG widths.

    ReLU / max-pool are discontinuous, so at this size a handful of sign / arg-max flips between two correct fp32
    forwards are expected (oracle.NetOracle.adopt_forward_state explains).  Three checks: forward blobs (tight),
    the whole backward chain on a shared forward state (tight), the end-to-end objective (flip-tolerant)."""
    topo = oracle.VGG19_TOPOLOGY
    params = oracle.he_init_weights(topo, seed=0)
    net = oracle.NetOracle(topo, params, full_forward=False)
    gpu = st2.HipModel(params)
    rs = np.random.RandomState
    content = rs(1).randint(0, 256, (225, 300, 3)).astype(np.uint8)
    style = rs(2).randint(0, 256, (187, 300, 3)).astype(np.uint8)
    init = rs(3).randint(0, 256, (225, 300, 3)).astype(np.uint8)
    # (1) forward
    x = net.preprocess(init)
    names = ['conv1_1', 'pool1', 'conv2_2', 'pool2', 'conv3_4', 'pool3', 'conv4_2', 'pool4', 'conv5_1']
    fc, fg = net.forward(x, names), gpu.forward(x, names)
    flips = 0
    for n in names:
        assert fg[n].shape == fc[n].shape and rel_l2(fg[n], fc[n]) <= 1e-5, n
        flips += int(np.sum((fc[n] > 0) != (fg[n] > 0)))
    assert flips <= 50                     # a few per several million activations, not a pattern
    # (2) ranged backward with injections at conv, pool and data blobs, on the GPU's forward state
    full = gpu.forward(x, ['data'] + [l[1] for l in topo[:17]])
    net.forward(x, list(full))
    net.adopt_forward_state(full)
    diffs = {n: rs(5 + i).randn(*full[n].shape).astype(F32) for i, n in enumerate(['conv5_1', 'pool4', 'conv4_2', 'conv3_1', 'pool1', 'conv1_1'])}
    assert rel_l2(gpu.backward(diffs), net.backward(diffs)) <= 1e-5
    # (3) end to end: loss tight, gradient flip-tolerant, trace values
    weights = {'content': {'conv4_2': 0.08, 'pool3': 0.01},
               'style': {'conv1_1': 1, 'conv2_1': 1, 'conv3_1': 1, 'conv4_1': 1, 'conv5_1': 1, 'pool4': 0.5},
               'deepdream': {'conv5_1': 0.01}}
    params4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
    cpu = oracle.TransferOracle(oracle.NetOracle(topo, params, full_forward=False))
    dev = st2.StyleTransfer(gpu)
    for st in (cpu, dev):
        st.set_input(init); st.set_content(content); st.set_style(style); st.reset()
        st.set_weights(weights, params4)
    lo, go = cpu.opfunc(cpu.input)
    ld, gd = dev.opfunc()
    assert gd.shape == go.shape == (1, 3, 225, 300)
    assert np.isclose(ld, lo, rtol=1e-5)
    assert rel_l2(gd, go) <= 5e-3
    err = np.abs(gd - go)[0].max(0)
    assert np.mean(err > 1e-3 * np.abs(go).max()) <= 0.02      # the disagreement is confined to a few receptive fields
    check_trace(list(cpu.traces[-1].data), list(cpu.traces[-1].data.values()), dev.traces[-1].data, rtol=2e-3)


# ------------------------------------------------------------------- the worker loop on the real engine
@pytest.mark.parametrize('precision,cfg16,pipeline', [('fp32', None, '0'), ('fp32', None, '1'), ('bf16', None, '1'), ('bf16', '0', '0')])
def test_worker_end_to_end_on_gpu_with_resample_and_optimizer_switch(precision, cfg16, pipeline, monkeypatch):
    """The drop-in worker.py driven through its message protocol (in-process sockets) on the HIP engine:
    SetImages / SetWeights / SetOptimizer / Start, iterates, a RESAMPLE of input+content to a new size with a live
    Adam optimizer (host Pillow path, optimizers.py:29-40), an optimizer switch, pause, shutdown.  The script injects a message
    the moment the N-th Iterate is on the wire.  Plain loop: the message is polled before the next iteration.  Pipelined loop
    (the default): iteration N + 1 has been begun by then, so its iterate goes out first and the message acts one iteration
    later -- as any message does that arrives while an iteration is running."""
    import sys, os, pickle
    from collections import deque
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import messages, worker as worker_mod

    class Socks:
        class Again(Exception):
            pass

        def __init__(self):
            self.inbound, self.sent = deque(), []

        def recv_pyobj(self, flags=0):
            if not self.inbound:
                if flags:
                    raise self.Again()
                return messages.Shutdown()
            return pickle.loads(pickle.dumps(self.inbound.popleft()))

        def send_pyobj(self, obj):
            self.sent.append(obj)
            n_it = sum(isinstance(m, messages.Iterate) for m in self.sent)
            script = {3: [messages.SetImages((48, 64), messages.SetImages.RESAMPLE, messages.SetImages.RESAMPLE)],
                      6: [messages.SetOptimizer('lbfgs', 1)],
                      9: [messages.PauseIteration()]}
            if isinstance(obj, messages.Iterate) and n_it in script:
                self.inbound.extend(script.pop(n_it) if n_it in script else [])

    # bf16: the lean data flow (fused pools + arg-max maps when the tile configuration is forced to 0) through a resample
    # to another size, an optimizer switch and a pause -- every buffer of the bf16 path is re-created with the geometry
    if cfg16 is not None:
        monkeypatch.setenv('ST2_CONV16_CFG', cfg16)
    topo = oracle.tiny_topology((8, 16), (2, 2))
    tr = st2.StyleTransfer(st2.HipModel(oracle.he_init_weights(topo, 0, 0.1), topology=topo, precision=precision))
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (32, 40, 3)).astype(np.uint8), rs(2).randint(0, 256, (24, 24, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (32, 40, 3)).astype(np.uint8))
    socks = Socks()
    socks.inbound.extend([messages.SetImages(None, init, content, style, True),
                          messages.SetWeights({'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}},
                                              {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}),
                          messages.SetOptimizer('adam', 10), messages.StartIteration()])
    wk = worker_mod.Worker({'async_iterate': '0', 'pipeline_iterate': pipeline}, sock_in=socks, sock_out=socks, transfer=tr)
    assert wk.pipelined == (pipeline == '1')
    wk.run()
    kinds = [type(m).__name__ for m in socks.sent]
    late = 1 if pipeline == '1' else 0                          # iterations already begun when a message arrives
    assert kinds[0] == 'WorkerReady' and kinds[-1] == 'Shutdown' and kinds.count('Iterate') == 9 + late
    assert kinds == ['WorkerReady'] + ['Iterate'] * (9 + late) + ['Shutdown']
    its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
    # SetOptimizer with a new class resets t (worker.py:387-391)
    assert [m.i for m in its] == list(range(1, 7 + late)) + [1, 2, 3]
    assert its[2 + late].image.shape == (32, 40, 3) and its[3 + late].image.shape == (48, 64, 3)       # resampled after iterate 3 (+ 1)
    assert all(np.isfinite(m.trace['loss']) and m.image.dtype == F32 for m in its)
    assert its[5 + late].trace['loss'] != its[4 + late].trace['loss']        # still iterating after the resample
    assert 'conv1_1_s_grad' in its[-1].trace and its[-1].trace['fevals'] == 3
    assert isinstance(tr.optimizer, st2.LBFGSOptimizer)


@pytest.mark.parametrize('pipeline', ['1', '0'])
def test_worker_async_iterate_on_gpu_keeps_order_one_iterate_per_step_shutdown_last(pipeline):
    """SURVEY 8f item 3 on the real engine: with the sender thread (async_iterate = 1, the default) the wire still
    carries WorkerReady first, exactly one Iterate per step in step order, Shutdown last (reference worker.py:333,
    351-353, 362-363), and the iterates are the ones a synchronous run of the same job produces, bit for bit."""
    import sys, os, pickle, time
    from collections import deque
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import messages, worker as worker_mod

    class Socks:
        class Again(Exception):
            pass

        def __init__(self):
            self.inbound, self.sent = deque(), []

        def recv_pyobj(self, flags=0):
            if not self.inbound:
                if flags:
                    raise self.Again()
                return messages.Shutdown()
            return pickle.loads(pickle.dumps(self.inbound.popleft()))

        def send_pyobj(self, obj):                     # runs on the sender thread
            time.sleep(0.002)                          # a slow wire: the worker runs ahead, the queue fills
            self.sent.append(pickle.loads(pickle.dumps(obj)))
            if sum(isinstance(m, messages.Iterate) for m in self.sent) == 6:
                self.inbound.append(messages.PauseIteration())

    topo = oracle.tiny_topology((8, 16), (2, 2))
    params = oracle.he_init_weights(topo, 0, 0.1)
    rs = np.random.RandomState
    content, style, init = (rs(1).randint(0, 256, (32, 40, 3)).astype(np.uint8), rs(2).randint(0, 256, (24, 24, 3)).astype(np.uint8),
                            rs(3).randint(0, 256, (32, 40, 3)).astype(np.uint8))
    weights = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
    params4 = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}

    def script():
        return [messages.SetImages(None, init, content, style, True), messages.SetWeights(weights, params4),
                messages.SetOptimizer('adam', 10), messages.StartIteration()]

    socks = Socks()
    socks.inbound.extend(script())
    wk = worker_mod.Worker({'async_iterate': '1', 'pipeline_iterate': pipeline}, sock_in=socks, sock_out=socks,
                           transfer=st2.StyleTransfer(st2.HipModel(params, topology=topo)))
    assert isinstance(wk.sock_out, worker_mod.AsyncSender) and wk.pipelined == (pipeline == '1')
    wk.run()
    kinds = [type(m).__name__ for m in socks.sent]
    assert kinds[0] == 'WorkerReady' and kinds[-1] == 'Shutdown' and kinds.count('Shutdown') == 1
    its = [m for m in socks.sent if isinstance(m, messages.Iterate)]
    n = len(its)
    assert n >= 6 and kinds == ['WorkerReady'] + ['Iterate'] * n + ['Shutdown']
    assert [m.i for m in its] == list(range(1, n + 1))                 # one per step, in step order, none lost
    assert [m.trace['fevals'] for m in its] == list(range(1, n + 1))
    # the same job driven synchronously: identical iterates (the sender thread only moves bytes)
    ref = st2.StyleTransfer(st2.HipModel(params, topology=topo))
    ref.set_input(init); ref.set_content(content); ref.set_style(style); ref.reset()
    ref.set_weights(weights, params4)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    for m in its:
        img, tr = ref.step()
        assert np.array_equal(m.image, img) and m.trace['loss'] == tr['loss'], m.i


@pytest.mark.parametrize('kind,step', [('adam', 10), ('lbfgs', 1)])
def test_two_half_iteration_is_the_plain_one_bit_for_bit(kind, step):
    """st_step_begin / st_step_end (iteration k + 1 queued before iterate k is collected) against st_step on a twin job: same
    images, same traces; at most two in flight, st_step refuses while any is, end without begin is an error."""
    g = load('transfer_tiny.npz')
    params = json.loads(str(g['params_json']))
    a, b = engine_transfer(g, kind, step, params), engine_transfer(g, kind, step, params)
    got = []
    a.step_begin()
    for _ in range(6):
        a.step_begin()
        assert a.steps_pending == 2 and a.engine.steps_pending() == 2
        got.append(a.step_end())
    with pytest.raises(st2.StError, match='already in flight'):
        a.engine.step_begin(); a.engine.step_begin()
    with pytest.raises(st2.StError, match='in flight'):
        a.engine.step()
    got.append(a.step_end())                               # the oldest first
    a.engine.step_end()                                    # (the extra begin above; not tracked by the StyleTransfer)
    assert a.engine.steps_pending() == 0
    with pytest.raises(st2.StError, match='no iteration in flight'):
        a.engine.step_end()
    for i, (img, trace, index) in enumerate(got):
        ref_img, ref_trace = b.step()
        assert index == i + 1 and np.array_equal(img, ref_img)
        assert {k: v for k, v in trace.items() if k != 'time'} == {k: v for k, v in ref_trace.items() if k != 'time'}


def test_engine_error_paths_are_loud():
    topo = oracle.tiny_topology((8, 16), (2, 2))
    params = oracle.he_init_weights(topo, 0, 0.1)
    eng = st2.Engine(topo)
    with pytest.raises(st2.StError, match='never loaded'):
        eng.set_content(np.zeros((8, 8, 3), np.uint8))
    eng.load_weights(params)
    with pytest.raises(st2.StError, match='no input image'):
        eng.opfunc()
    eng.set_input(np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(st2.StError, match='content features missing'):
        eng.opfunc()
    eng.set_content(np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(st2.StError, match='different size'):
        eng.opfunc()
    eng.set_content(np.zeros((16, 16, 3), np.uint8))
    with pytest.raises(st2.StError, match='style Gram'):
        eng.opfunc()
    eng.set_style(np.zeros((12, 12, 3), np.uint8))
    with pytest.raises(st2.StError, match='no optimizer'):
        eng.step()
    with pytest.raises(ValueError):
        eng.set_input(np.zeros((4, 4), np.uint8))
    with pytest.raises(KeyError):
        st2.StyleTransfer(st2.HipModel(None, engine=eng)).set_weights({'content': {}}, {})
    eng.close()
