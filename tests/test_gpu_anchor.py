"""The anchor term on the real engine (``pytest -m gpu``): st_set_anchor, held per element to the float64 restatement and the derived bars
of tests/anchor_oracle.py, and bit for bit where the term only composes with what exists.

The tiny net and the sizes of tests/test_gpu_laplacian.py: 16 x 16 and 64 x 64 (16-byte path), 17 x 33 and 37 x 50 (odd widths: the scalar
form; 37 x 50 has more pixels than one workgroup takes per trip), 20 x 260 (16-byte path, crosses the 256-column tile of image_pass_k).
Weights 0.7, -1.3 and 250; no map, and a map with 20 % zeros and 10 % of the cells multiplied by 7.5."""
import numpy as np
import pytest

import anchor_oracle as ao
import quadratic_oracle as q
import style_transfer2_amd as st2
import test_gpu_laplacian as tl
from style_transfer2_amd import capi, jobs
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine, _ptr

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO, NET, WEIGHTS, PARAMS, SIZES, THREE = tl.TOPO, tl.NET, tl.WEIGHTS, tl.PARAMS, tl.SIZES, tl.THREE
image, make, live, same_bits, launches, size_id = tl.image, tl.make, tl.live, tl.same_bits, tl.launches, tl.size_id
MAPS = ('none', 'mixed')
BASE_LEN = 3 * 6 + 8                                                       # three active layers


def the_map(h, w, kind):
    return ao.mixed_map(h, w, 5) if kind == 'mixed' else None


def inside(name, got, want, bar):
    ratio, at = ao.worst(got, want, bar)
    got = np.asarray(got, np.float64)
    assert ratio <= 1, ('%s: worst element %r: got %.9g, float64 %.9g, bar %.3g (%.3g x the bar)' % (name, at, got[at], want[at], bar[at], ratio))
    return ratio


@pytest.fixture(scope='module')
def engines():
    """One context per size for the per-element checks (the anchor changes between the cases; everything else is read only)."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            made[(h, w)] = make(h, w)
        return made[(h, w)]
    yield get
    for eng in made.values():
        eng.close()


# ---- 1. per element against the float64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', MAPS)
@pytest.mark.parametrize('weight', ao.WEIGHTS)
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_plane_loss_and_gradient_norm_meet_their_bars(engines, size, weight, kind):
    h, w = size
    eng = engines(h, w)
    eng.set_laplacian(None)
    m = the_map(h, w, kind)
    eng.set_anchor(image(4, h, w), m, weight)
    assert eng.anchor() == {'size': (h, w), 'has_mask': m is not None, 'weight': float(weight)} and eng.trace_len() == BASE_LEN + 2
    x = eng.get_input_nchw()[0]
    loss, grad, trace = eng.opfunc()
    ax, m_dev, extra = eng.anchor_terms()
    assert (m is None and m_dev is None) or same_bits(m_dev, m)
    ref = ao.evaluate(x, ax[0], m, weight)
    r_g = inside('extra', extra[0], ref['g'], ref['g_bar'])
    a_loss, a_grad = trace[-7], trace[-3]
    print('[%dx%d w %g map %s] extra %.3f of its bar; a_loss %.9g (float64 %.9g, bar %.3g); a_grad %.9g (float64 %.9g, bar %.3g)'
          % (h, w, weight, kind, r_g, a_loss, ref['loss'], ref['loss_bar'], a_grad, ref['a_grad'], ref['a_grad_bar']))
    assert abs(a_loss - ref['loss']) <= ref['loss_bar'], (a_loss, ref['loss'], ref['loss_bar'])
    assert abs(a_grad - ref['a_grad']) <= ref['a_grad_bar'], (a_grad, ref['a_grad'], ref['a_grad_bar'])
    assert len(trace) == BASE_LEN + 2 and loss == F32(trace[-2]) and np.isfinite(grad).all()
    if m is not None:
        assert not extra[0][:, m == 0].any()
    # an evaluation without a gradient: a_loss the same, no a_grad, and the hook refuses the plane it does not have
    loss2, _, trace2 = eng.opfunc(False)
    assert trace2[-7] == a_loss and trace2[-3] == 0 and loss2 == loss
    with pytest.raises(StError, match=r'st2 error 2: .*no gradient'):
        eng.anchor_terms()
    assert same_bits(eng.anchor_terms(want_extra=False)[0], ax)
    # the planar entry takes the same planes to the same bits
    eng.set_anchor(ax, m, weight)
    loss3, grad3, trace3 = eng.opfunc()
    assert loss3 == loss and same_bits(grad3, grad) and np.array_equal(trace3, trace) and same_bits(eng.anchor_terms()[2], extra)


# ---- 2. composition, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('size', [(37, 50), (20, 260), (64, 64)], ids=size_id)
def test_gradient_and_loss_are_those_of_the_term_off_plus_the_term(size, precision):
    h, w = size
    m, weight = the_map(h, w, 'mixed'), -1.3
    eng = make(h, w, precision=precision)
    eng.opfunc()                                                          # (captures the norms)
    loss_off, grad_off, trace_off = eng.opfunc()
    eng.set_anchor(image(4, h, w), m, weight)
    loss_on, grad_on, trace_on = eng.opfunc()
    g_anc = eng.anchor_terms()[2]
    assert g_anc.any() and not g_anc[0][:, m == 0].any()                  # where the map is 0 the plane is 0
    assert same_bits(grad_on, grad_off + g_anc)                           # float32 + float32, one rounding
    a_loss = F32(trace_on[-7])
    assert loss_on == F32(loss_off + a_loss) and F32(trace_on[-2]) == loss_on
    assert len(trace_on) == len(trace_off) + 2
    rest = np.delete(trace_on, [len(trace_on) - 7, len(trace_on) - 3])
    assert np.array_equal(rest[:-2], trace_off[:-2])                      # every layer term, scd / tv / p losses and gradients
    assert rest[-1] != trace_off[-1]                                      # (the rms of another gradient)
    # the Laplacian term alone at the same x, then both
    eng.set_anchor(None)
    eng.set_laplacian(THREE)
    loss_lap, grad_lap, trace_lap = eng.opfunc()
    g_lap = eng.laplacian_terms(0)[2]
    eng.set_anchor(image(4, h, w), m, weight)
    loss_both, grad_both, trace_both = eng.opfunc()
    extra = eng.anchor_terms()[2]
    assert same_bits(extra, g_lap + g_anc) and same_bits(grad_both, grad_off + extra)
    assert np.array_equal(extra[0][:, m == 0], g_lap[0][:, m == 0])       # where the map is 0: exactly g_lap's value
    assert len(trace_both) == len(trace_off) + 4
    l_loss, l_grad = trace_both[-9], trace_both[-4]                      # [.., p_loss, l_loss, a_loss, scd_grad, tv_grad, p_grad, l_grad, a_grad, loss, grad]
    assert l_loss == trace_lap[-7] and l_grad == trace_lap[-3] and trace_both[-8] == trace_on[-7] and trace_both[-3] == trace_on[-3]
    assert loss_both == F32(F32(loss_off + F32(l_loss)) + a_loss) and F32(trace_both[-2]) == loss_both
    rest = np.delete(trace_both, [len(trace_both) - k for k in (9, 8, 4, 3)])
    assert np.array_equal(rest[:-2], trace_off[:-2])
    eng.set_anchor(None)
    eng.set_laplacian(None)
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
    off.set_anchor(image(4, h, w), the_map(h, w, 'mixed'), 0.7)
    assert live()[0] - before[0] == 4 * (3 * h * w + h * w + 3 * h * w + 2 * 1024) and off.trace_len() == never.trace_len() + 2
    off.set_anchor(None)
    assert live() == before and off.trace_len() == never.trace_len() and off.anchor() is None
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
    assert p_off == p_never and sum(p_never.values()) > 0 and 'anchor' not in p_never
    assert live() == before
    # ... and with the term on: exactly one launch more per evaluation, a class of its own, and still one image pass
    off.set_anchor(image(4, h, w), the_map(h, w, 'mixed'), 0.7)
    off.profile_read()
    off.step()
    p_on = launches(off)
    assert p_on.get('anchor') == 1 and p_on['image_pass'] == 1
    off.opfunc(False)
    p_on = launches(off)
    assert p_on.get('anchor') == 1 and p_on['image_pass'] == 1
    off.close(); never.close()


# ---- 4. steps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,with_lap', [(OPT_ADAM, False), (OPT_LBFGS, False), (OPT_ADAM, True)], ids=['adam', 'lbfgs', 'adam+laplacian'])
def test_three_steps_are_the_same_bytes_plain_pipelined_and_replayed(kind, with_lap):
    h, w = 37, 52

    def one(graph=False):
        eng = make(h, w, THREE if with_lap else None, kind, graph=graph)
        eng.set_anchor(image(4, h, w), the_map(h, w, 'mixed'), 0.7)
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
        assert len(ta) == BASE_LEN + (4 if with_lap else 2) and np.isfinite(ta).all()
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb
        assert same_bits(ia, ic) and np.array_equal(ta, tc) and la == lc
    assert same_bits(plain.get_input_nchw(), piped.get_input_nchw()) and same_bits(plain.get_input_nchw(), graph.get_input_nchw())
    if kind == OPT_ADAM:
        assert graph.graph_replays() >= 1 and plain.graph_replays() == 0
        assert np.array_equal(want[0][1], trace0)                         # the trace of the first step is the objective's at the x it started from
        # the first iterate is image_pass_k's update, restated in NumPy float32 from the read-back gradient; the bar is ADAM_X_ATOL of
        # tests/quadratic_oracle.py
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
    for eng in (plain, piped, graph):
        eng.close()


# ---- 5. the term alone ---------------------------------------------------------------------------------------------------------------
def alone(h, w, kind, step, ax, m, weight):
    """Empty weight table, tv = p = 0 with powers 2: the objective is the anchor term."""
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    eng.set_content(image(1, h, w)); eng.set_style(image(2, 24, 24))
    eng.set_input_nchw(q.x0(h, w))
    eng.set_weights([], [], [], [], [0, 2, 0, 2])
    eng.optimizer_reset(kind, step)
    eng.set_anchor(ax, m, weight)
    assert eng.trace_len() == 10
    return eng


def test_ten_adam_steps_on_the_term_alone_follow_float64():
    h, w, weight = 20, 36, 0.7
    ax = q.x0(h, w, 9)
    m = ao.mixed_map(h, w, 5)
    eng = alone(h, w, OPT_ADAM, 10, ax, m, weight)

    def objective(x):
        return ao.loss_and_grad_u(np.asarray(x, np.float64)[0] / 255.0, ax[0].astype(np.float64) / 255.0, m, weight)
    ref = q.Adam64(q.x0(h, w), lambda x: (objective(x)[0], objective(x)[1][None]), 10)
    worst = 0.0
    for k in range(10):
        _, trace, loss = eng.step()
        x64, loss64 = ref.step()
        worst = max(worst, q.max_abs(eng.get_input_nchw(), x64))
        assert trace[-2] == loss and trace[3] == loss and not trace[:3].any()       # (a_loss is the whole loss)
    print('[ten Adam steps on the anchor term alone] max |x_dev - x_64| %.3g, bar %g' % (worst, q.ADAM_X_ATOL))
    assert worst <= q.ADAM_X_ATOL
    eng.close()


@pytest.mark.parametrize('kind,step', [(OPT_ADAM, 10), (OPT_LBFGS, 1)], ids=['adam', 'lbfgs'])
def test_pixels_outside_a_binary_map_keep_their_bits(kind, step):
    h, w = 20, 36
    ax = q.x0(h, w, 9)
    m = np.random.RandomState(3).rand(h, w) < 0.5                        # bool: 0 / 1
    eng = alone(h, w, kind, step, ax, m, 250.0)
    x0 = eng.get_input_nchw()
    for _ in range(5):
        eng.step()
    x5 = eng.get_input_nchw()
    assert same_bits(x5[0][:, ~m], x0[0][:, ~m])
    assert (x5[0][:, m] != x0[0][:, m]).mean() > 0.99                     # (and the others moved)
    eng.close()


# ---- 6. size and state ---------------------------------------------------------------------------------------------------------------
def test_the_anchor_does_not_follow_the_input_and_a_misfit_refuses_before_anything_is_enqueued():
    h, w = 17, 33
    eng = make(h, w)
    eng.set_anchor(image(4, h, w), the_map(h, w, 'mixed'), 0.7)
    eng.opfunc()
    eng.resample_state((24, 40))
    eng.resample_content((24, 40))
    assert eng.anchor()['size'] == (h, w)                                 # it stays
    with pytest.raises(StError, match=r'st2 error 2: .*resized'):
        eng.anchor_terms()
    x_before, adam_before = eng.get_input_nchw(), eng.adam_get_state()
    eng.profile_enable(True); eng.profile_read()
    for call in (eng.opfunc, eng.step, eng.step_begin):
        with pytest.raises(StError, match=r'st2 error 2: .*anchor is 17 x 33, the input 24 x 40'):
            call()
    assert launches(eng) == {} and eng.steps_pending() == 0
    assert same_bits(eng.get_input_nchw(), x_before)
    for a, b in zip(eng.adam_get_state(), adam_before):
        assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b
    eng.profile_enable(False)
    eng.set_anchor(image(4, 24, 40), None, 0.7)                           # a new anchor lifts the refusal
    eng.opfunc()
    assert eng.anchor_terms()[2].shape == (1, 3, 24, 40)
    eng.set_input(image(3, h, w))                                         # st_set_input to another size: refused again ...
    eng.set_content(image(1, h, w))
    with pytest.raises(StError, match=r'st2 error 2: .*anchor is 24 x 40, the input 17 x 33'):
        eng.opfunc()
    eng.set_anchor(None)                                                  # ... until the term is turned off
    eng.opfunc()
    eng.close()


def test_refusals_and_destroy():
    start = live()
    eng = make(16, 16)
    img, m = image(4, 16, 16), ao.mixed_map(16, 16, 5)
    for bad in (0.0, -0.0, float('nan'), float('inf'), -float('inf'), 1e-60, 1e60):
        with pytest.raises(StError, match=r'st2 error 1: .*weight'):
            eng.set_anchor(img, m, bad)
        assert eng.anchor() is None
    for bad in (-1e-30, float('nan'), float('inf'), -float('inf')):
        mm = m.copy(); mm[15, 15] = bad
        with pytest.raises(StError, match=r'st2 error 1: .*map'):
            eng.set_anchor(img, mm, 1.0)
        with pytest.raises(StError, match=r'st2 error 1: .*map'):
            eng.set_anchor(np.zeros((3, 16, 16), F32), mm, 1.0)
        assert eng.anchor() is None
    for hh, ww in ((0, 16), (16, 0), (-1, 16)):
        with pytest.raises(StError, match=r'st2 error 1: .*at least 1 x 1'):
            capi.check(eng.lib.st_set_anchor(eng._ctx, _ptr(img), hh, ww, 1, None, 1.0))
        with pytest.raises(StError, match=r'st2 error 1: .*at least 1 x 1'):
            capi.check(eng.lib.st_set_anchor_nchw(eng._ctx, _ptr(np.zeros((3, 16, 16), F32)), hh, ww, None, 1.0))
    with pytest.raises(StError, match=r'st2 error 1: '):
        capi.check(eng.lib.st_set_anchor_nchw(eng._ctx, None, 16, 16, None, 1.0))
    with pytest.raises(ValueError):
        eng.set_anchor(img, m[:, :15], 1.0)
    with pytest.raises(StError, match=r'st2 error 2: .*off'):
        eng.anchor_terms()
    eng.set_anchor(img, m, 1.5)
    eng.set_anchor(img, np.uint8(m > 0) * 255, 2.5)                       # uint8: divided by 255
    with pytest.raises(StError, match=r'st2 error 2: .*no objective evaluation'):                 # the hook before any evaluation
        eng.anchor_terms()
    with pytest.raises(StError, match=r'st2 error 1: .*weight'):          # a refused call changes nothing
        eng.set_anchor(img, None, 0.0)
    assert eng.anchor() == {'size': (16, 16), 'has_mask': True, 'weight': 2.5}
    eng.opfunc()
    assert same_bits(eng.anchor_terms()[1], (m > 0).astype(F32))
    eng.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_anchor(img, None, 1.0)
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_anchor(np.zeros((3, 16, 16), F32), None, 1.0)
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_anchor(None)
    eng.step_end()
    assert eng.anchor()['weight'] == 2.5
    with pytest.raises(StError, match=r'st2 error 2: .*anchor'):                                    # st_tile_configure with the term on
        capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    eng.set_anchor(None)
    capi.check(eng.lib.st_tile_configure(eng._ctx, 16, 16, 0, 0, 0, 0, 16, 16))
    with pytest.raises(StError, match=r'st2 error 2: .*tile-configured'):                           # the setter on a tile-configured context
        eng.set_anchor(img, None, 1.0)
    eng.set_anchor(None)                                                                            # (off stays allowed)
    eng.close()
    # st_destroy with the term on frees its buffers with everything else
    eng = make(16, 16)
    eng.set_anchor(img, m, 1.5)
    eng.step()
    assert live()[0] > start[0]
    eng.close()
    assert live() == start


# ---- 7. frames -----------------------------------------------------------------------------------------------------------------------
def test_run_frames_is_the_same_calls_made_by_hand():
    h, w, iters, weight = 24, 32, 4, 40.0
    frames = [image(10 + t, h, w) for t in range(3)]
    style = image(2, 24, 24)
    flow = np.zeros((h, w, 2), F32)
    flow[..., 0], flow[..., 1] = 2, -1
    flows = [None, flow, -flow]
    masks = [None, ao.mixed_map(h, w, 5), ao.mixed_map(h, w, 6)]
    kw = dict(optimizer='adam', weights=WEIGHTS, params=PARAMS)

    seen = []
    a = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    got = jobs.run_frames(a, frames, style, iters, weight, flows=flows, masks=masks, callback=lambda i, img, tr: seen.append((i, tr)), **kw)
    assert len(got) == 3 and [i for i, _ in seen] == [1, 2, 3, 4] * 3
    assert all('a_loss' not in tr and 'a_grad' not in tr for _, tr in seen[:4])
    for _, tr in seen[4:]:
        keys = list(tr)
        assert keys[keys.index('p_loss') + 1] == 'a_loss' and keys[keys.index('p_grad') + 1] == 'a_grad'
    assert seen[4][1]['a_loss'] == 0 and seen[7][1]['a_loss'] > 0         # a frame starts at its anchor and leaves it
    assert a.engine.anchor() == {'size': (h, w), 'has_mask': True, 'weight': weight}

    b = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    by_hand = [jobs.run_job(b, frames[0], style, iters, anchor=False, **kw)]
    for t in (1, 2):
        prev = b.engine.get_input_nchw()[0]
        shifted = jobs.warp_planar(prev, flows[t])
        assert not same_bits(shifted, prev)
        b.set_input(np.zeros((h, w, 3), np.uint8)); b.engine.set_input_nchw(shifted[None])
        b.set_content(frames[t]); b.set_style(style); b.reset()
        b.set_weights(WEIGHTS, PARAMS)
        b.optimizer_cls = st2.AdamOptimizer; b.set_step_size(10); b.reset()
        b.set_anchor(shifted[None], masks[t], weight)
        assert b.start() and same_bits(b.engine.get_input_nchw(), shifted[None])      # the first x is the warped iterate ...
        for _ in range(iters):
            out, _ = b.step()
        assert same_bits(b.engine.anchor_terms(want_extra=False)[0], shifted[None])    # ... and so is the anchor
        by_hand.append(out)
    for t in range(3):
        assert got[t].dtype == F32 and got[t].shape == (h, w, 3) and same_bits(got[t], by_hand[t]), 'frame %d differs' % t
    assert not same_bits(got[1], got[2])
    a.engine.close(); b.engine.close()
