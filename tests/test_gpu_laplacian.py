"""The Laplacian-steered content term on the real engine (``pytest -m gpu``): st_set_laplacian, held per element to the float64
restatement and the derived bars of tests/laplacian_oracle.py, and bit for bit where the term only composes with what exists.

Sizes, the smallest at which each thing can go wrong: 16 x 16 (one cell at p = 16: E = 0), 17 x 33 (one-row and one-column clipped
cells), 37 x 50 (odd in both directions, no 16-byte path), 20 x 260 (crosses the 256-column tile of image_pass_k and the 64-column tile of
the pooling pass), 64 x 64 (16-byte path, every pool size exact).  Tiny VGG-shaped nets, as the neighbouring files use."""
from ctypes import byref, c_longlong
import os
import threading

import numpy as np
import pytest

import messages
import oracle
import style_transfer2_amd as st2
import laplacian_oracle as lo
from quadratic_oracle import ADAM_X_ATOL
from style_transfer2_amd import capi, jobs
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine
from style_transfer2_amd.transfer import LOSS_NAMES, SCALAR_LOSS_NAMES, weight_table
import worker as worker_mod

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO = oracle.tiny_topology((8, 16), (2, 2))
NET = oracle.he_init_weights(TOPO, 0, 0.1)
WEIGHTS = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
SIZES = ((16, 16), (17, 33), (37, 50), (20, 260), (64, 64))
LEVEL_SETS = (((1, 0.7),), ((4, 1.5),), ((16, 2.0),), ((32, 3.0),), ((2, 0.8), (4, -1.3), (16, 2.5)))
THREE = LEVEL_SETS[-1]
size_id = lambda s: '%dx%d' % s                                           # noqa: E731
levels_id = lambda lv: '+'.join(str(p) for p, _ in lv)                    # noqa: E731


def image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def set_weights(eng, weights=WEIGHTS):
    rows, cells = weight_table(weights)
    cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
    eng.set_weights(rows, cols[0], cols[1], cols[2], [PARAMS[k] for k in SCALAR_LOSS_NAMES])


def make(h, w, levels=None, kind=OPT_ADAM, precision='fp32', graph=False):
    old = os.environ.get('ST2_GRAPH')
    os.environ['ST2_GRAPH'] = '1' if graph else '0'                       # (read when the context is created)
    try:
        eng = Engine(TOPO, 0, precision)
    finally:
        if old is None:
            os.environ.pop('ST2_GRAPH', None)
        else:
            os.environ['ST2_GRAPH'] = old
    eng.load_weights(NET)
    eng.set_input(image(3, h, w))
    eng.set_content(image(1, h, w))
    eng.set_style(image(2, 24, 24))
    set_weights(eng)
    eng.optimizer_reset(kind, 10 if kind == OPT_ADAM else 1)
    if levels is not None:
        eng.set_laplacian(levels)
    return eng


def live():
    dev, pin = c_longlong(-1), c_longlong(-1)
    capi.check(capi.load_library().st_live_bytes(byref(dev), byref(pin)))
    return dev.value, pin.value


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def launches(eng):
    return {k: v['launches'] for k, v in eng.profile_read().items()}


def inside(name, got, want, bar):
    ratio, at = lo.worst(got, want, bar)
    got = np.asarray(got, np.float64)
    assert ratio <= 1, ('%s: worst element %r: got %.9g, float64 %.9g, bar %.3g (%.3g x the bar)' % (name, at, got[at], want[at], bar[at], ratio))


@pytest.fixture(scope='module')
def engines():
    """One context per size for the per-element checks (the levels change between the cases; everything else is read only)."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            made[(h, w)] = make(h, w)
        return made[(h, w)]
    yield get
    for eng in made.values():
        eng.close()


# ---- 1. per element against the float64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', LEVEL_SETS, ids=levels_id)
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_targets_differences_gradient_and_trace_meet_their_bars(engines, size, levels):
    h, w = size
    eng = engines(h, w)
    eng.set_laplacian(levels)
    assert eng.laplacian() == [(p, float(wt)) for p, wt in levels] and eng.trace_len() == 3 * 6 + 10      # three active layers
    x, cx = eng.get_input_nchw()[0], eng.get_content_nchw()[0]
    ref = lo.evaluate(x, cx, levels)
    loss, grad, trace = eng.opfunc()
    for l, (p, _) in enumerate(levels):
        T, E, g = eng.laplacian_terms(l)
        assert T.shape == E.shape == (3, -(-h // p), -(-w // p))
        inside('T of pool %d' % p, T, ref['T'][l], ref['T_bar'][l])
        inside('E of pool %d' % p, E, ref['E'][l], ref['E_bar'][l])
        if -(-h // p) == 1 and -(-w // p) == 1:
            assert not T.any() and not E.any()                            # one cell: the stencil has no neighbour
        inside('g_lap (read at level %d)' % l, g[0], ref['g'], ref['g_bar'])
    l_loss, l_grad = trace[-7], trace[-3]
    print('[%dx%d %s] l_loss %.9g (float64 %.9g, bar %.3g), l_grad %.9g (float64 %.9g, bar %.3g)'
          % (h, w, levels_id(levels), l_loss, ref['loss'], ref['loss_bar'], l_grad, ref['l_grad'], ref['l_grad_bar']))
    assert abs(l_loss - ref['loss']) <= ref['loss_bar'], (l_loss, ref['loss'], ref['loss_bar'])
    assert abs(l_grad - ref['l_grad']) <= ref['l_grad_bar'], (l_grad, ref['l_grad'], ref['l_grad_bar'])
    assert loss == F32(trace[-2]) and np.isfinite(grad).all()
    # an evaluation without a gradient: l_loss the same, no l_grad, and the hook refuses the gradient it does not have
    loss2, _, trace2 = eng.opfunc(False)
    assert trace2[-7] == l_loss and trace2[-3] == 0 and loss2 == loss
    with pytest.raises(StError, match=r'st2 error 2: .*no gradient'):
        eng.laplacian_terms(0)
    assert same_bits(eng.laplacian_terms(0, want_grad=False)[1], eng.laplacian_terms(0, want_grad=False)[1])


# ---- 2. composition, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('size', [(37, 50), (20, 260), (64, 64)], ids=size_id)
def test_gradient_and_loss_are_those_of_the_term_off_plus_the_term(size, precision):
    eng = make(size[0], size[1], precision=precision)
    eng.opfunc()                                                          # (captures the norms)
    loss_off, grad_off, trace_off = eng.opfunc()
    eng.set_laplacian(THREE)
    loss_on, grad_on, trace_on = eng.opfunc()
    g_lap = eng.laplacian_terms(0)[2]
    assert g_lap.any()
    assert same_bits(grad_on, grad_off + g_lap)                           # float32 + float32, one rounding
    l_loss = F32(trace_on[-7])
    assert loss_on == F32(loss_off + l_loss) and F32(trace_on[-2]) == loss_on
    assert len(trace_on) == len(trace_off) + 2
    rest = np.delete(trace_on, [len(trace_on) - 7, len(trace_on) - 3])
    assert np.array_equal(rest[:-2], trace_off[:-2])                      # every layer term, scd / tv / p losses and gradients
    assert rest[-1] != trace_off[-1]                                      # (the rms of another gradient)
    eng.set_laplacian(None)
    loss_again, grad_again, trace_again = eng.opfunc()
    assert loss_again == loss_off and same_bits(grad_again, grad_off) and np.array_equal(trace_again, trace_off)
    eng.close()


# ---- 3. off is as good as never ------------------------------------------------------------------------------------------------------
def test_on_and_off_again_leaves_the_bytes_launches_and_memory_of_a_context_that_never_saw_the_call():
    off, never = make(37, 50), make(37, 50)
    for eng in (off, never):
        eng.step()                                                        # (every lazily made buffer of a step exists now)
    before = live()
    off.set_laplacian(THREE)
    assert live()[0] > before[0] and off.trace_len() == never.trace_len() + 2
    off.set_laplacian([])
    assert live() == before and off.trace_len() == never.trace_len() and off.laplacian() == []
    for eng in (off, never):
        eng.profile_enable(True)
        eng.profile_read()
    a, b = off.opfunc(), never.opfunc()
    assert a[0] == b[0] and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    for _ in range(3):
        ra, rb = off.step(), never.step()
        assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
        assert same_bits(off.get_input_nchw(), never.get_input_nchw())
    p_off, p_never = launches(off), launches(never)
    assert p_off == p_never and sum(p_never.values()) > 0 and not any(k.startswith('laplacian') for k in p_never)
    assert live() == before
    # ... and with the term on: three launches more per evaluation with a gradient, each a class of its own, plus the trace's
    off.set_laplacian(THREE)                                              # (content of the input's size: the targets are taken here)
    off.profile_read()
    off.step()
    p_on = launches(off)
    assert [p_on.get('laplacian_' + k) for k in ('pool', 'stencil', 'grad')] == [1, 1, 1]
    assert p_on['image_pass'] == 1
    off.close(); never.close()


# ---- 4. steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [OPT_ADAM, OPT_LBFGS], ids=['adam', 'lbfgs'])
def test_three_steps_are_the_same_bytes_plain_pipelined_and_replayed(kind):
    h, w = 37, 52
    plain, piped, graph = make(h, w, THREE, kind), make(h, w, THREE, kind), make(h, w, THREE, kind, graph=True)
    x0 = plain.get_input_nchw()
    for eng in (plain, piped, graph):
        eng.opfunc()                                                      # (the norms are captured here, in all three alike)
    _, grad0, trace0 = plain.opfunc()
    want, x1_dev = [], None
    for k in range(3):
        want.append(plain.step())
        if k == 0:
            x1_dev = plain.get_input_nchw()
    got = []
    for k in range(3):                                                    # one begin ahead of every end, as the worker loop runs it
        piped.step_begin()
        if k:
            got.append(piped.step_end())
    got.append(piped.step_end())
    replayed = [graph.step() for _ in range(3)]
    for (ia, ta, la), (ib, tb, lb), (ic, tc, lc) in zip(want, got, replayed):
        assert len(ta) == 3 * 6 + 10 and np.isfinite(ta).all()
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb
        assert same_bits(ia, ic) and np.array_equal(ta, tc) and la == lc
    assert same_bits(plain.get_input_nchw(), piped.get_input_nchw()) and same_bits(plain.get_input_nchw(), graph.get_input_nchw())
    if kind == OPT_ADAM:
        assert graph.graph_replays() >= 1 and plain.graph_replays() == 0
        # the trace of the first step is the objective's at the x it started from ...
        assert np.array_equal(want[0][1], trace0)
        # ... and the first iterate is image_pass_k's update, restated in NumPy float32 from the read-back gradient; the bar is
        # ADAM_X_ATOL of tests/test_gpu_quadratic_descent.py::test_adam_follows_float64_through_a_new_input_and_a_new_step_size
        g = grad0[0]
        m = F32(0.9) * F32(0) + F32(1 - 0.9) * g
        v = F32(0.999) * F32(0) + F32(1 - 0.999) * (g * g)
        x1 = x0[0] - (F32(10) * (m / F32(1 - 0.9))) / (np.sqrt(v / F32(1 - 0.999)) + F32(1e-8))
        err = float(np.abs(x1_dev[0] - x1).max())
        print('[first Adam iterate with the term on] max |x_dev - x_numpy| %.3g, bar %g' % (err, ADAM_X_ATOL))
        assert err <= ADAM_X_ATOL
    else:
        # L-BFGS: the step evaluates at the old x first; its trace is the objective's at the NEW x
        _, _, trace1 = plain.opfunc()
        assert np.array_equal(want[-1][1], trace1)
    for eng in (plain, piped, graph):
        eng.close()


# ---- 5. the targets follow the content image ----------------------------------------------------------------------------------------
def test_targets_follow_the_content_image_and_a_misfit_refuses_before_anything_is_enqueued():
    h, w = 17, 33
    levels = ((4, 1.5), (16, -2.0))
    eng = make(h, w, levels)
    eng.opfunc()

    def targets_are_those_of(cx):
        ref = lo.evaluate(eng.get_input_nchw()[0], cx, levels)
        for l in range(len(levels)):
            inside('T %d' % l, eng.laplacian_terms(l)[0], ref['T'][l], ref['T_bar'][l])
        return ref
    first = targets_are_those_of(eng.get_content_nchw()[0])
    eng.set_content(image(7, h, w))
    eng.opfunc()
    second = targets_are_those_of(eng.get_content_nchw()[0])
    assert np.abs(first['T'][0] - second['T'][0]).max() > 100 * second['T_bar'][0].max()      # (another image: the check is not vacuous)
    # resampled content and state: the targets are those of the resampled content at the new size
    eng.resample_state((24, 40))
    with pytest.raises(StError, match=r'st2 error 2: .*resized'):
        eng.laplacian_terms(0)
    x_before, adam_before = eng.get_input_nchw(), eng.adam_get_state()
    eng.profile_enable(True); eng.profile_read()
    for call in (eng.opfunc, eng.step, eng.step_begin):                   # the content is still 17 x 33
        with pytest.raises(StError, match=r'st2 error 2: .*content image of the input.s size'):
            call()
    assert launches(eng) == {} and eng.steps_pending() == 0
    assert same_bits(eng.get_input_nchw(), x_before)
    for a, b in zip(eng.adam_get_state(), adam_before):
        assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b
    eng.profile_enable(False)
    eng.resample_content((24, 40))
    eng.opfunc()
    assert eng.laplacian_terms(0)[0].shape == (3, 6, 10)
    targets_are_those_of(eng.get_content_nchw()[0])
    eng.close()
    # no content image at all
    bare = Engine(TOPO, 0, 'fp32')
    bare.load_weights(NET)
    bare.set_input(image(3, h, w)); bare.set_style(image(2, 24, 24))
    set_weights(bare, {'content': {}, 'style': {'conv1_1': 1}, 'deepdream': {}})
    bare.optimizer_reset(OPT_ADAM, 10)
    bare.opfunc()                                                         # runs without the term
    bare.set_laplacian(levels)
    x_before = bare.get_input_nchw()
    for call in (bare.opfunc, bare.step, bare.step_begin):
        with pytest.raises(StError, match=r'st2 error 2: .*needs a content image'):
            call()
    assert same_bits(bare.get_input_nchw(), x_before) and bare.adam_get_state()[2:] == (0, 0)
    bare.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    eng = make(16, 16)
    for bad, why in ((((3, 1.0),), 'pool size'), (((0, 1.0),), 'pool size'), (((64, 1.0),), 'pool size'), (((4, 1.0), (4, 2.0)), 'same pool size'),
                     (((1, 1.0), (2, 1.0), (4, 1.0), (8, 1.0)), 'between 0 and 3'), (((4, 0.0),), 'finite and non-zero'),
                     (((4, float('nan')),), 'finite and non-zero'), (((4, float('inf')),), 'finite and non-zero'), (((4, 1.0), (8, -float('inf'))), 'finite and non-zero')):
        with pytest.raises(StError, match=r'st2 error 1: .*' + why):
            eng.set_laplacian(bad)
        assert eng.laplacian() == []
    with pytest.raises(StError, match=r'st2 error 1: '):
        capi.check(eng.lib.st_set_laplacian(eng._ctx, 1, None, None))
    eng.set_laplacian(((4, 1.5),))
    with pytest.raises(StError, match=r'st2 error 2: .*no objective evaluation'):                 # the hook before any evaluation
        eng.laplacian_terms(0)
    with pytest.raises(StError, match=r'st2 error 1: .*level'):
        capi.check(eng.lib.st_get_laplacian_terms(eng._ctx, 1, None, None, None))
    eng.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_laplacian(((8, 1.0),))
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_laplacian([])
    eng.step_end()
    assert eng.laplacian() == [(4, 1.5)]
    with pytest.raises(StError, match=r'st2 error 2: .*Laplacian'):                                 # st_tile_configure with the term on
        capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    eng.set_laplacian([])
    with pytest.raises(StError, match=r'st2 error 2: .*off'):
        eng.laplacian_terms(0)
    capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    with pytest.raises(StError, match=r'st2 error 2: .*tile-configured'):                           # the setter on a tile-configured context
        eng.set_laplacian(((4, 1.5),))
    eng.set_laplacian([])                                                                           # (off stays allowed)
    eng.close()


# ---- 7. worker, SetWeights, jobs -------------------------------------------------------------------------------------------------------
def _model():
    return st2.HipModel(NET, topology=TOPO)


def _direct(levels, n, params=PARAMS):
    ref = st2.StyleTransfer(_model())
    ref.set_input(image(3, 32, 40)); ref.set_content(image(1, 32, 40)); ref.set_style(image(2, 24, 24)); ref.reset()
    ref.set_weights(WEIGHTS, params)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    if levels is not None:
        ref.set_laplacian(levels)
    assert ref.start()
    return [ref.step() for _ in range(n)]


@pytest.mark.parametrize('via', ['config', 'set_weights'])
def test_worker_runs_the_term_from_the_config_key_and_from_set_weights(monkeypatch, via):
    """Worker(config) on its own TCP sockets (pyzmq where it is installed, otherwise tests/minizmq.py): with `laplacian = 4:1.5,16:-2`
    in the config, or with params['laplacian'] in SetWeights, the iterates are those of an engine driven by hand with the term on, and
    the trace names l_loss after p_loss and l_grad after p_grad."""
    from test_boundary import zmq_module
    zmq, which = zmq_module(monkeypatch)
    levels = [(4, 1.5), (16, -2.0)]
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app}
    params = dict(PARAMS)
    if via == 'config':
        config['laplacian'] = '4:1.5, 16:-2'
    else:
        params['laplacian'] = levels
    wk = worker_mod.Worker(config, transfer=st2.StyleTransfer(_model()))
    assert wk.transfer.engine.laplacian() == (levels if via == 'config' else [])
    th = threading.Thread(target=wk.run, daemon=True)
    th.start()
    app_out = ctx.socket(zmq.PUSH)
    app_out.connect(config['worker_socket'])
    for m in (messages.SetImages(None, image(3, 32, 40), image(1, 32, 40), image(2, 24, 24), True), messages.SetWeights(WEIGHTS, params),
              messages.SetOptimizer('adam', 10), messages.StartIteration()):
        app_out.send_pyobj(m)
    got = []
    poller = zmq.Poller()
    poller.register(app_in, zmq.POLLIN)
    while sum(isinstance(m, messages.Iterate) for m in got) < 3 and poller.poll(20000):
        got.append(app_in.recv_pyobj())
    app_out.send_pyobj(messages.Shutdown())
    while poller.poll(20000):
        got.append(app_in.recv_pyobj())
        if isinstance(got[-1], messages.Shutdown):
            break
    th.join(30)
    assert wk.transfer.engine.laplacian() == levels
    wk.close()
    app_out.close(0); app_in.close(0); ctx.destroy(0)
    its = [m for m in got if isinstance(m, messages.Iterate)]
    assert len(its) >= 3
    by_hand, plain = _direct(levels, len(its)), _direct(None, 1)
    for m, (img, tr) in zip(its, by_hand):
        assert m.image.dtype == F32 and np.array_equal(m.image, img), 'iterate %d differs' % m.i
        assert list(m.trace) == list(tr) and all(m.trace[k] == tr[k] for k in tr if k != 'time')
    keys = list(its[0].trace)
    assert keys[keys.index('p_loss') + 1] == 'l_loss' and keys[keys.index('p_grad') + 1] == 'l_grad'
    assert [k for k in keys if k not in ('l_loss', 'l_grad')] == list(plain[0][1])
    assert not np.array_equal(its[0].image, plain[0][0])


def test_a_params_dict_without_the_key_leaves_the_setting_alone_and_jobs_take_the_levels():
    st = st2.StyleTransfer(_model())
    st.set_laplacian([(8, 2.0)])
    st.set_weights(WEIGHTS, PARAMS)
    assert st.engine.laplacian() == [(8, 2.0)]
    st.set_weights(WEIGHTS, dict(PARAMS, laplacian=[]))
    assert st.engine.laplacian() == []
    out = jobs.run_job(st, image(1, 32, 40), image(2, 24, 24), 2, optimizer='adam', weights=WEIGHTS, params=PARAMS, laplacian=[(4, 1.5)])
    assert out.shape == (32, 40, 3) and st.engine.laplacian() == [(4, 1.5)] and 'l_loss' in st.traces[-1].data
    st.engine.close()
