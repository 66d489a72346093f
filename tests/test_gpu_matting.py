"""The photorealism term on the real engine (``pytest -m gpu``): st_set_matting, held bit for bit to the restatement of
tests/matting_oracle.py -- the per-window data, the fits, the plane the image pass adds, the returned gradient and the trace scalars.

Sizes, the smallest at which each thing can go wrong: 3 x 3 (one window), 3 x 7 and 7 x 3 (one row, one column of windows), 5 x 5 (the
first pixel that nine windows contain), 17 x 33, 37 x 50 (odd in both directions), 64 x 64 (W % 4 == 0: the image pass and the other
terms take their 16-byte forms; this term's two passes have one form only, 4-byte accesses, so for them 37 x 50 and 64 x 64 differ in
shape alone), and per pass the size that exceeds its 64 x 4 tile by one cell in both directions (matting_plan.h: 7 x 67 for the windows
of the first pass, 5 x 65 for the pixels of the second).  Tiny VGG-shaped nets, as the neighbouring files use.

The trace's `grad`, the rms of the combined gradient, is summed by image_pass_k; matting_oracle.image_pass_grad_rms restates that sum
(its tiles, the fp32 accumulator per thread, block_sum, sum_partials) from the gradient the pass wrote, and the value is held to it bit
for bit like the term's own scalars."""
import os
import re
import threading

import numpy as np
import pytest

import matting_oracle as mo
import messages
import quadratic_oracle as q
import style_transfer2_amd as st2
import test_gpu_laplacian as tl
import worker as worker_mod
from style_transfer2_amd import capi, jobs
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO, NET, WEIGHTS, PARAMS, THREE = tl.TOPO, tl.NET, tl.WEIGHTS, tl.PARAMS, tl.THREE
image, make, live, same_bits, launches, size_id, set_weights = tl.image, tl.make, tl.live, tl.same_bits, tl.launches, tl.size_id, tl.set_weights
BASE_LEN = 3 * 6 + 8                                                       # three active layers
PLAN = open(os.path.join(os.path.dirname(st2.__file__), 'csrc', 'matting_plan.h')).read()
TILE_W, TILE_H = (int(re.search(r'%s = (\d+)' % name, PLAN).group(1)) for name in ('kMatTileW', 'kMatTileH'))
SIZES = ((3, 3), (3, 7), (7, 3), (5, 5), (17, 33), (37, 50), (64, 64), (TILE_H + 3, TILE_W + 3), (TILE_H + 1, TILE_W + 1))
# (eps, weight, the content image: uint8 or float)
CASES = ((1e-9, 0.7, 'u8'), (1e-7, -1.3, 'u8'), (1e-2, 250.0, 'float'))
M_LOSS, M_GRAD, LOSS, GRAD = -7, -3, -2, -1                                # with this term the only optional one


def test_the_oracle_walks_the_tiles_of_the_plan_header():
    assert (mo.TILE_W, mo.TILE_H) == (TILE_W, TILE_H) == (64, 4)
    assert int(re.search(r'kMatMaxBlocks = (\d+)', PLAN).group(1)) == mo.MAX_BLOCKS
    passes = open(os.path.join(os.path.dirname(st2.__file__), 'csrc', 'passes.hip')).read()
    assert re.search(r'constexpr int IP_TY = (\d+), IP_TX = (\d+);', passes).groups() == (str(mo.IP_TY), str(mo.IP_TX))


def content_image(kind, h, w):
    if kind == 'u8':
        return image(7, h, w)
    return (np.random.RandomState(8).rand(h, w, 3) * 255).astype(F32)


def grad_has_the_bits(trace_grad, grad):
    return F32(trace_grad) == mo.image_pass_grad_rms(grad)


@pytest.fixture(scope='module')
def engines():
    """One context per size (the term and the content image change between the cases; everything else is read only)."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            made[(h, w)] = make(h, w)
            made[(h, w)].opfunc()                                         # (captures the norms)
        return made[(h, w)]
    yield get
    for eng in made.values():
        eng.close()


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=lambda c: 'eps%g-w%g-%s' % c)
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_every_plane_and_scalar_has_the_bits_of_the_restatement(engines, size, case):
    h, w = size
    eps, weight, kind = case
    eng = engines(h, w)
    eng.set_matting(0)
    eng.set_content(content_image(kind, h, w))
    loss_off, grad_off, trace_off = eng.opfunc()
    eng.set_matting(weight, eps)
    assert eng.matting() == {'weight': weight, 'eps': eps} and eng.trace_len() == BASE_LEN + 2 and eng.trace_terms() == (False, False, True)
    x, cx = eng.get_input_nchw()[0], eng.get_content_nchw()[0]
    loss, grad, trace = eng.opfunc()
    mu, M, a_pb, extra = eng.matting_terms()
    ref = mo.evaluate(x, cx, weight, eps)
    for name, got in (('mu', mu), ('M', M), ('a_pb', a_pb), ('extra', extra[0])):
        want = ref['g_mat' if name == 'extra' else name]
        assert same_bits(got, want), '%s: %d of %d elements differ, worst %.3g' % (name, (got != want).sum(), got.size, np.abs(got - want).max())
    assert np.isfinite(extra).all() and (h < 4 or extra.any())
    m_loss, m_grad = trace[M_LOSS], trace[M_GRAD]
    print('[%dx%d eps %g w %g %s] m_loss %.9g (restated %.9g), m_grad %.9g (restated %.9g)' % (h, w, eps, weight, kind, m_loss, ref['m_loss'], m_grad, ref['m_grad']))
    assert F32(m_loss) == ref['m_loss'] and F32(m_grad) == ref['m_grad']
    assert len(trace) == BASE_LEN + 2 and loss == F32(F32(loss_off) + F32(m_loss)) and F32(trace[LOSS]) == loss
    assert same_bits(grad, grad_off + extra)                              # float32 + float32, one rounding
    assert grad_has_the_bits(trace[GRAD], grad)
    rest = np.delete(trace, [len(trace) + M_LOSS, len(trace) + M_GRAD])
    assert np.array_equal(rest[:-2], trace_off[:-2])                      # every other term is what it was
    # an evaluation without a gradient: m_loss the same, no m_grad, and the hook refuses the plane it does not have
    loss2, _, trace2 = eng.opfunc(False)
    assert trace2[M_LOSS] == m_loss and trace2[M_GRAD] == 0 and loss2 == loss
    with pytest.raises(StError, match=r'st2 error 2: .*no gradient'):
        eng.matting_terms()
    assert same_bits(eng.matting_terms(want_extra=False)[2], a_pb)


# ---- 2. composition, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('size', [(37, 50), (20, 260), (64, 64)], ids=size_id)      # (20 x 260: two column tiles of image_pass_k)
def test_the_term_composes_with_the_laplacian_and_the_anchor_term(size, precision):
    h, w = size
    weight, eps = -1.3, 1e-7
    anchor = (image(4, h, w), None, 0.7)
    eng = make(h, w, precision=precision)
    eng.opfunc()
    loss_off, grad_off, trace_off = eng.opfunc()
    x, cx = eng.get_input_nchw()[0], eng.get_content_nchw()[0]
    ref = mo.evaluate(x, cx, weight, eps)
    eng.set_matting(weight, eps)
    _, grad_m, trace_m = eng.opfunc()
    g_mat = eng.matting_terms()[3]
    assert same_bits(g_mat[0], ref['g_mat']) and F32(trace_m[M_LOSS]) == ref['m_loss'] and F32(trace_m[M_GRAD]) == ref['m_grad']      # (bf16: the term is fp32)
    assert same_bits(grad_m, grad_off + g_mat)
    eng.set_matting(0)
    eng.set_laplacian(THREE)
    _, _, trace_l = eng.opfunc()
    g_lap = eng.laplacian_terms(0)[2]
    eng.set_matting(weight, eps)                                          # Laplacian + this term
    loss_lm, grad_lm, trace_lm = eng.opfunc()
    assert eng.trace_terms() == (True, False, True) and len(trace_lm) == BASE_LEN + 4
    assert same_bits(eng.matting_terms()[3], g_lap + g_mat) and same_bits(grad_lm, grad_off + (g_lap + g_mat))
    assert trace_lm[-9] == trace_l[-7] and trace_lm[-8] == trace_m[M_LOSS] and trace_lm[-4] == trace_l[-3] and trace_lm[-3] == trace_m[M_GRAD]
    assert loss_lm == F32(F32(F32(loss_off) + F32(trace_lm[-9])) + F32(trace_lm[-8]))
    eng.set_laplacian(None)
    eng.set_matting(0)
    eng.set_anchor(*anchor)
    _, _, trace_a = eng.opfunc()
    g_anc = eng.anchor_terms()[2]
    eng.set_matting(weight, eps)                                          # anchor + this term
    loss_am, grad_am, trace_am = eng.opfunc()
    assert eng.trace_terms() == (False, True, True) and len(trace_am) == BASE_LEN + 4
    assert same_bits(eng.matting_terms()[3], g_anc + g_mat) and same_bits(grad_am, grad_off + (g_anc + g_mat))
    assert trace_am[-9] == trace_a[-7] and trace_am[-8] == trace_m[M_LOSS] and trace_am[-4] == trace_a[-3] and trace_am[-3] == trace_m[M_GRAD]
    eng.set_laplacian(THREE)                                              # all three
    loss_all, grad_all, trace_all = eng.opfunc()
    assert eng.trace_terms() == (True, True, True) and len(trace_all) == 3 * 6 + 14 == eng.trace_len()
    extra = eng.matting_terms()[3]
    assert same_bits(extra, (g_lap + g_anc) + g_mat) and same_bits(eng.anchor_terms()[2], g_lap + g_anc) and same_bits(grad_all, grad_off + extra)
    # [.., p_loss, l_loss, a_loss, m_loss, scd_grad, tv_grad, p_grad, l_grad, a_grad, m_grad, loss, grad]
    l_loss, a_loss, m_loss = trace_all[-11], trace_all[-10], trace_all[-9]
    assert (l_loss, a_loss, m_loss) == (trace_l[-7], trace_a[-7], trace_m[M_LOSS])
    assert (trace_all[-5], trace_all[-4], trace_all[-3]) == (trace_l[-3], trace_a[-3], trace_m[M_GRAD])
    assert loss_all == F32(F32(F32(F32(loss_off) + F32(l_loss)) + F32(a_loss)) + F32(m_loss)) and F32(trace_all[LOSS]) == loss_all
    assert grad_has_the_bits(trace_all[GRAD], grad_all)
    rest = np.delete(trace_all, [len(trace_all) - k for k in (11, 10, 9, 5, 4, 3)])
    assert np.array_equal(rest[:-2], trace_off[:-2])
    # jitter with a pinned shift: the term reads the unshifted iterate and content image
    eng.set_laplacian(None); eng.set_anchor(None)
    eng.set_jitter(4, 11)
    eng.set_jitter_shift(2, -3)
    _, _, trace_j = eng.opfunc()
    assert trace_j[M_LOSS] == trace_m[M_LOSS] and trace_j[M_GRAD] == trace_m[M_GRAD] and same_bits(eng.matting_terms()[3], g_mat)
    eng.set_jitter(0)
    eng.set_matting(0)
    loss_again, grad_again, trace_again = eng.opfunc()
    assert loss_again == loss_off and same_bits(grad_again, grad_off) and np.array_equal(trace_again, trace_off)
    eng.close()


# ---- 3. off is as good as never ------------------------------------------------------------------------------------------------------
def test_on_and_off_again_leaves_the_bytes_launches_and_memory_of_a_context_that_never_saw_the_call():
    h, w = 37, 50
    off, never = make(h, w), make(h, w)
    for eng in (off, never):
        eng.step()                                                        # (every lazily made buffer of a step exists now)
    before = live()
    off.set_matting(0.7)
    windows = (h - 2) * (w - 2)
    assert live()[0] - before[0] == 4 * (3 * h * w + 21 * windows + 3 * h * w + 2 * 1024) and off.trace_len() == never.trace_len() + 2
    off.set_matting(0)
    assert live() == before and off.trace_len() == never.trace_len() and off.matting() is None
    for eng in (off, never):
        eng.profile_enable(True)
        eng.profile_read()
    a, b = off.opfunc(), never.opfunc()
    assert a[0] == b[0] and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    for _ in range(3):
        ra, rb = off.step(), never.step()
        assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    p_off, p_never = launches(off), launches(never)
    assert p_off == p_never and sum(p_never.values()) > 0 and not any(k.startswith('matting') for k in p_never)
    assert live() == before
    # ... and with the term on: the per-window data once, then two launches per evaluation with a gradient and one without
    off.set_matting(0.7)
    assert launches(off) == {'matting_windows': 1}
    off.step()
    p_on = launches(off)
    assert p_on.get('matting_fit') == 1 and p_on.get('matting_apply') == 1 and p_on['image_pass'] == 1 and 'matting_windows' not in p_on
    off.opfunc(False)
    p_on = launches(off)
    assert p_on.get('matting_fit') == 1 and 'matting_apply' not in p_on and p_on['image_pass'] == 1
    off.close(); never.close()


# ---- 4. steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [OPT_ADAM, OPT_LBFGS], ids=['adam', 'lbfgs'])
def test_three_steps_are_the_same_bytes_plain_pipelined_and_replayed(kind):
    h, w = 37, 52

    def one(graph=False):
        eng = make(h, w, None, kind, graph=graph)
        eng.set_matting(40.0, 1e-7)
        return eng
    plain, piped, graph = one(), one(), one(graph=True)
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
        assert len(ta) == BASE_LEN + 2 and np.isfinite(ta).all() and ta[M_LOSS] > 0 and ta[M_GRAD] > 0
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb
        assert same_bits(ia, ic) and np.array_equal(ta, tc) and la == lc
    assert same_bits(plain.get_input_nchw(), piped.get_input_nchw()) and same_bits(plain.get_input_nchw(), graph.get_input_nchw())
    if kind == OPT_ADAM:
        assert graph.graph_replays() >= 1 and plain.graph_replays() == 0
        assert np.array_equal(want[0][1], trace0)                         # the trace of the first step is the objective's at the x it started from
        # the first iterate is image_pass_k's update, restated in NumPy float32 from the gradient st_opfunc returned
        g = grad0[0]
        m = F32(0.9) * F32(0) + F32(1 - 0.9) * g
        v = F32(0.999) * F32(0) + F32(1 - 0.999) * (g * g)
        x1 = x0[0] - (F32(10) * (m / F32(1 - 0.9))) / (np.sqrt(v / F32(1 - 0.999)) + F32(1e-8))
        err = float(np.abs(x1_dev[0] - x1).max())
        print('[first Adam iterate with the term on] max |x_dev - x_numpy| %.3g, bar %g' % (err, q.ADAM_X_ATOL))
        assert err <= q.ADAM_X_ATOL
    else:
        _, _, trace1 = plain.opfunc()                                     # L-BFGS: the step's trace is the objective's at the NEW x
        assert np.array_equal(want[-1][1], trace1)
        # the first step has no curvature pair: x1 = x0 - step * g / rms(g) (quadratic_oracle.LBFGS64), from the gradient st_opfunc returned
        g = grad0.astype(np.float64)
        x1 = x0.astype(np.float64) - 1.0 * g / np.sqrt(np.vdot(g, g) / g.size)
        err = float(np.abs(x1_dev - x1).max())
        print('[first L-BFGS iterate with the term on] max |x_dev - x_64| %.3g, bar %g' % (err, q.ADAM_X_ATOL))
        assert err <= q.ADAM_X_ATOL
    for eng in (plain, piped, graph):
        eng.close()


# ---- 5. the per-window data follow the content image ---------------------------------------------------------------------------------
def test_windows_follow_the_content_image_and_a_misfit_refuses_before_anything_is_enqueued():
    h, w = 17, 33
    weight, eps = 0.7, 1e-7
    eng = make(h, w)
    eng.set_matting(weight, eps)
    eng.opfunc()

    def bits_are_those_of_the_content():
        ref = mo.evaluate(eng.get_input_nchw()[0], eng.get_content_nchw()[0], weight, eps)
        mu, M, a_pb, extra = eng.matting_terms()
        assert same_bits(mu, ref['mu']) and same_bits(M, ref['M']) and same_bits(a_pb, ref['a_pb']) and same_bits(extra[0], ref['g_mat'])
        return ref
    first = bits_are_those_of_the_content()
    eng.set_content(image(7, h, w))
    eng.opfunc()
    second = bits_are_those_of_the_content()
    assert not same_bits(first['mu'], second['mu'])                       # (another image: the check is not vacuous)
    eng.resample_state((24, 40))
    with pytest.raises(StError, match=r'st2 error 2: .*resized'):
        eng.matting_terms()
    x_before, adam_before = eng.get_input_nchw(), eng.adam_get_state()
    eng.profile_enable(True); eng.profile_read()
    for call in (eng.opfunc, eng.step, eng.step_begin):                   # the content is still 17 x 33
        with pytest.raises(StError, match=r'st2 error 2: .*photorealism.*content is 17 x 33, the input 24 x 40'):
            call()
    assert launches(eng) == {} and eng.steps_pending() == 0
    assert same_bits(eng.get_input_nchw(), x_before)
    for a, b in zip(eng.adam_get_state(), adam_before):
        assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b
    eng.profile_enable(False)
    eng.resample_content((24, 40))
    eng.opfunc()
    assert eng.matting_terms()[0].shape == (3, 22, 38)
    bits_are_those_of_the_content()
    eng.close()
    # no content image at all, and an input under 3 x 3
    bare = Engine(TOPO, 0, 'fp32')
    bare.load_weights(NET)
    bare.set_input(image(3, h, w)); bare.set_style(image(2, 24, 24))
    set_weights(bare, {'content': {}, 'style': {'conv1_1': 1}, 'deepdream': {}})
    bare.optimizer_reset(OPT_ADAM, 10)
    bare.opfunc()                                                         # runs without the term
    bare.set_matting(1.0)
    x_before = bare.get_input_nchw()
    for call in (bare.opfunc, bare.step, bare.step_begin):
        with pytest.raises(StError, match=r'st2 error 2: .*needs a content image'):
            call()
    assert same_bits(bare.get_input_nchw(), x_before) and bare.adam_get_state()[2:] == (0, 0)
    bare.set_input(image(3, 2, 9)); bare.set_content(image(1, 2, 9))
    for call in (bare.opfunc, bare.step, bare.step_begin):
        with pytest.raises(StError, match=r'st2 error 2: .*at least 3 x 3.*input is 2 x 9'):
            call()
    bare.set_matting(0)
    bare.opfunc()
    bare.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_and_destroy():
    start = live()
    eng = make(16, 16)
    for bad in (float('nan'), float('inf'), -float('inf'), 1e-60, -1e-60, 1e60):
        with pytest.raises(StError, match=r'st2 error 1: .*weight'):
            eng.set_matting(bad)
        assert eng.matting() is None
    for bad in (0.0, 1e-10, 1.0000001, -1e-7, float('nan'), float('inf')):
        with pytest.raises(StError, match=r'st2 error 1: .*eps'):
            eng.set_matting(1.0, bad)
        assert eng.matting() is None
    with pytest.raises(StError, match=r'st2 error 2: .*off'):
        eng.matting_terms()
    eng.set_matting(1.5, 1e-9)
    eng.set_matting(2.5, 1.0)
    with pytest.raises(StError, match=r'st2 error 2: .*no objective evaluation'):                 # the hook before any evaluation
        eng.matting_terms()
    with pytest.raises(StError, match=r'st2 error 1: .*eps'):             # a refused call changes nothing
        eng.set_matting(1.0, 2.0)
    assert eng.matting() == {'weight': 2.5, 'eps': 1.0}
    eng.opfunc()
    eng.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_matting(1.0)
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_matting(0)
    eng.step_end()
    assert eng.matting()['weight'] == 2.5
    with pytest.raises(StError, match=r'st2 error 2: .*photorealism'):                              # st_tile_configure with the term on
        capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    eng.set_matting(0)
    capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    with pytest.raises(StError, match=r'st2 error 2: .*tile-configured'):                           # the setter on a tile-configured context
        eng.set_matting(1.0)
    eng.set_matting(0)                                                                              # (off stays allowed)
    eng.close()
    # st_destroy with the term on frees its buffers with everything else
    eng = make(16, 16)
    eng.set_matting(1.5)
    eng.step()
    assert live()[0] > start[0]
    eng.close()
    assert live() == start


# ---- 7. worker and jobs ----------------------------------------------------------------------------------------------------------------
def _model():
    return st2.HipModel(NET, topology=TOPO)


def test_worker_runs_the_term_from_the_config_key(monkeypatch):
    """Worker(config) on its own TCP sockets with `matting = 50`: the Iterates carry m_loss after p_loss and m_grad after p_grad, and are
    those of an engine driven by hand with the term on."""
    from test_boundary import zmq_module
    zmq, which = zmq_module(monkeypatch)
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app, 'matting': '50'}
    wk = worker_mod.Worker(config, transfer=st2.StyleTransfer(_model()))
    assert wk.transfer.engine.matting() == {'weight': 50.0, 'eps': 1e-7}
    th = threading.Thread(target=wk.run, daemon=True)
    th.start()
    app_out = ctx.socket(zmq.PUSH)
    app_out.connect(config['worker_socket'])
    for m in (messages.SetImages(None, image(3, 32, 40), image(1, 32, 40), image(2, 24, 24), True), messages.SetWeights(WEIGHTS, PARAMS),
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
    wk.close()
    app_out.close(0); app_in.close(0); ctx.destroy(0)
    its = [m for m in got if isinstance(m, messages.Iterate)]
    assert len(its) >= 3
    ref = st2.StyleTransfer(_model())
    ref.set_input(image(3, 32, 40)); ref.set_content(image(1, 32, 40)); ref.set_style(image(2, 24, 24)); ref.reset()
    ref.set_weights(WEIGHTS, PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    ref.set_matting(50)
    assert ref.start()
    for m in its:
        img, tr = ref.step()
        assert m.image.dtype == F32 and np.array_equal(m.image, img), 'iterate %d differs' % m.i
        assert list(m.trace) == list(tr) and all(m.trace[k] == tr[k] for k in tr if k != 'time')
    keys = list(its[0].trace)
    assert keys[keys.index('p_loss') + 1] == 'm_loss' and keys[keys.index('p_grad') + 1] == 'm_grad'
    assert its[0].trace['m_loss'] > 0 and its[0].trace['m_grad'] > 0
    ref.engine.close()


def test_jobs_take_the_term_and_frames_pass_it_on():
    st = st2.StyleTransfer(_model())
    out = jobs.run_job(st, image(1, 32, 40), image(2, 24, 24), 2, optimizer='adam', weights=WEIGHTS, params=PARAMS, matting=(30.0, 1e-5))
    assert out.shape == (32, 40, 3) and st.engine.matting() == {'weight': 30.0, 'eps': 1e-5} and 'm_loss' in st.traces[-1].data
    jobs.run_job(st, image(1, 32, 40), image(2, 24, 24), 1, optimizer='adam', weights=WEIGHTS, params=PARAMS)
    assert st.engine.matting() is not None                                # None leaves the engine as it is
    jobs.run_job(st, image(1, 32, 40), image(2, 24, 24), 1, optimizer='adam', weights=WEIGHTS, params=PARAMS, matting=False)
    assert st.engine.matting() is None and 'm_loss' not in st.traces[-1].data
    seen = []
    frames = [image(10 + t, 24, 32) for t in range(2)]
    jobs.run_frames(st, frames, image(2, 24, 24), 2, 40.0, callback=lambda i, img, tr: seen.append(tr), optimizer='adam', weights=WEIGHTS, params=PARAMS,
                    matting=20.0)
    assert len(seen) == 4 and all('m_loss' in tr for tr in seen) and 'a_loss' in seen[-1]
    keys = list(seen[-1])
    assert keys[keys.index('a_loss') + 1] == 'm_loss' and keys[keys.index('a_grad') + 1] == 'm_grad'
    st.engine.close()
