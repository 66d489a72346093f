"""Jitter on the real engine (``pytest -m gpu``): st_set_jitter / st_set_jitter_shift.  The mode is a pure move around an unchanged
evaluation, so almost everything here is bit for bit: against np.roll, against a mode-off context that is GIVEN the rolled inputs, and
against the mode-off context for the image terms.  The oracle comparisons use the bars of the mode-off tests in tests/test_gpu_parity.py.

Sizes, those of tests/test_gpu_laplacian.py: 16 x 16, 17 x 33 and 37 x 50 (no 16-byte form at the odd widths), 20 x 260 (crosses the
64-lane row tile of roll_k in the scalar form and the 256-pixel one in the 16-byte form), 64 x 64.  Shifts: (2, 4) and (2, 5) tell an
aligned row offset from a misaligned one in the 16-byte form, (H, W) and (-40, 300) check the reduction."""
from ctypes import byref, c_longlong
import threading

import numpy as np
import pytest

import messages
import oracle
import style_transfer2_amd as st2
import jitter_oracle as jo
from helpers import check_trace, rel_l2
from style_transfer2_amd import capi
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine
from style_transfer2_amd.transfer import LOSS_NAMES, SCALAR_LOSS_NAMES, weight_table
import worker as worker_mod

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO = oracle.tiny_topology((8, 16), (2, 2))
NET = oracle.he_init_weights(TOPO, 0, 0.1)
WEIGHTS = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
STYLE_ONLY = {'content': {}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
SIZES = ((16, 16), (17, 33), (37, 50), (20, 260), (64, 64))
NL = 3 * 6                                                                # three active rows: the image part of the trace starts here
size_id = lambda s: '%dx%d' % s                                           # noqa: E731


def shifts_of(h, w):
    return ((0, 0), (1, 0), (0, -1), (-3, 2), (2, 4), (2, 5), (h, w), (-40, 300))


def image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def set_weights(eng, weights=WEIGHTS):
    rows, cells = weight_table(weights)
    cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
    eng.set_weights(rows, cols[0], cols[1], cols[2], [PARAMS[k] for k in SCALAR_LOSS_NAMES])


def make(h, w, kind=OPT_ADAM, precision='fp32', weights=WEIGHTS):
    eng = Engine(TOPO, 0, precision)
    eng.load_weights(NET)
    eng.set_input(image(3, h, w))
    eng.set_content(image(1, h, w))
    eng.set_style(image(2, 24, 24))
    set_weights(eng, weights)
    eng.optimizer_reset(kind, 10 if kind == OPT_ADAM else 1)
    return eng


def live():
    dev, pin = c_longlong(-1), c_longlong(-1)
    capi.check(capi.load_library().st_live_bytes(byref(dev), byref(pin)))
    return dev.value, pin.value


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def first_difference(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    at = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return None if not len(at) else (tuple(at[0]), float(a[tuple(at[0])]), float(b[tuple(at[0])]), len(at))


def launches(eng):
    return {k: v['launches'] for k, v in eng.profile_read().items()}


def convs(counts):
    return sum(v for k, v in counts.items() if k.startswith('conv3x3'))


# ---- 1. the planes the forward read ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_the_forward_reads_numpys_roll_of_the_iterate_bit_for_bit(size):
    h, w = size
    eng = make(h, w)
    x = eng.get_input_nchw()
    for s in shifts_of(h, w):
        eng.set_jitter_shift(*s)
        info = eng.jitter()
        assert info['pinned'] and info['shift'] == s and info['radius'] == 0 and info['k'] == 0
        eng.opfunc()
        xs, scd, used = eng.jitter_terms()
        assert used == s
        assert same_bits(xs, np.roll(x, s, (2, 3))), (s, first_difference(xs, np.roll(x, s, (2, 3))))
        assert same_bits(eng.get_blob('data'), xs)                        # the hooks answer in the shifted coordinates
        assert np.isfinite(scd).all() and scd.any()
        assert same_bits(eng.get_input_nchw(), x)                         # x itself is never moved
    eng.close()


# ---- 2. a shifted evaluation is the mode-off evaluation of the rolled inputs ----------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_shifted_evaluation_has_the_bits_of_the_plain_one_on_rolled_inputs_and_the_image_terms_of_the_unshifted(size, precision):
    h, w = size
    a, b, c = (make(h, w, precision=precision) for _ in range(3))
    x, cx = c.get_input_nchw(), c.get_content_nchw()
    for s in shifts_of(h, w):
        a.set_jitter_shift(*s)
        b.set_jitter(0)
        b.set_input_nchw(np.roll(x, s, (2, 3)))
        b.set_content_nchw(np.roll(cx, s, (2, 3)))
        for eng in (a, b, c):
            eng.clear_norms()
            eng.opfunc()                                                  # (captures the norms)
        (la, ga, ta), (lb, gb, tb), (lc, gc, tc) = a.opfunc(), b.opfunc(), c.opfunc()
        assert len(ta) == len(tb) == len(tc) == NL + 8                    # the trace keeps its length and layout
        assert np.array_equal(ta[:NL], tb[:NL]), s                        # every layer entry
        assert ta[NL] == tb[NL] and ta[NL + 3] == tb[NL + 3], s           # scd_loss, scd_grad
        assert ta[NL + 1] == tc[NL + 1] and ta[NL + 2] == tc[NL + 2] and ta[NL + 4] == tc[NL + 4] and ta[NL + 5] == tc[NL + 5], s      # t_loss, p_loss, tv_grad, p_grad
        # the network gradient: B pinned to (0, 0) evaluates as with the mode off and shows its own through the hook
        b.set_jitter_shift(0, 0)
        lb0, gb0, tb0 = b.opfunc()
        assert lb0 == lb and same_bits(gb0, gb) and np.array_equal(tb0, tb), s
        scd_a, scd_b = a.jitter_terms()[1], b.jitter_terms()[1]
        assert same_bits(np.roll(scd_a, s, (2, 3)), scd_b), (s, first_difference(np.roll(scd_a, s, (2, 3)), scd_b))
        # the combined gradient: the per-pixel arithmetic of the image pass does not depend on position
        want = np.roll(gb, (-s[0], -s[1]), (2, 3))
        assert same_bits(ga, want), (size, s, first_difference(ga, want))
        if (s[0] % h, s[1] % w) != (0, 0):
            assert ta[NL] != tc[NL]                                       # (the shift matters to the network)
        else:
            assert la == lc and same_bits(ga, gc) and np.array_equal(ta, tc)
    for eng in (a, b, c):
        eng.close()


# ---- 3. against the NumPy restatement ------------------------------------------------------------------------------------------------
def transfers(h, w, kind='adam', step=10):
    cpu = jo.JitterOracle(oracle.NetOracle(TOPO, NET))
    dev = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    for st in (cpu, dev):
        st.set_input(image(3, h, w)); st.set_content(image(1, h, w)); st.set_style(image(2, 24, 24)); st.reset()
        st.set_weights(WEIGHTS, PARAMS)
    cpu.set_optimizer(kind, step)
    dev.optimizer_cls = {'adam': st2.AdamOptimizer, 'lbfgs': st2.LBFGSOptimizer}[kind]; dev.set_step_size(step); dev.reset()
    assert cpu.start() and dev.start()
    return cpu, dev


@pytest.mark.parametrize('size', [(17, 33), (20, 260)], ids=size_id)
def test_loss_gradient_and_trace_meet_the_restatement_inside_the_bars_of_a_plain_evaluation(size):
    """Bars: those of test_gpu_parity.py::test_engine_opfunc_two_evals_match_reference_vectors (loss rtol 1e-4, gradient rel-L2 1e-4, trace
    rtol 2e-4) -- by the test above the mode on is a mode-off evaluation of other inputs."""
    h, w = size
    cpu, dev = transfers(h, w)
    x = dev.engine.get_input_nchw()
    worst = {}
    for s in ((0, 0), (-3, 2), (2, 5), (-40, 300)):
        cpu.jitter_shift = s
        if s == (0, 0):
            dev.engine.set_jitter(0)                                      # the mode off, beside the plain restatement
        else:
            dev.engine.set_jitter_shift(*s)
        cpu.norms = {k: {} for k in 'cds'}
        dev.engine.clear_norms()
        for ev in range(2):
            lo, go = cpu.opfunc(x.copy())
            ld, gd = dev.opfunc(x.copy())
            worst[s] = max(worst.get(s, 0), abs(float(ld) - float(lo)) / abs(float(lo)) / 1e-4, rel_l2(gd, go) / 1e-4)
            assert np.isclose(ld, lo, rtol=1e-4) and rel_l2(gd, go) <= 1e-4, (s, ev, ld, lo, rel_l2(gd, go))
            tc = cpu.traces[-1].data
            check_trace(list(tc), list(tc.values()), dev.traces[-1].data, rtol=2e-4)
    print('[%dx%d] worst fraction of the loss / gradient bars: mode off %.3f, on %s'
          % (h, w, worst[(0, 0)], ', '.join('%s %.3f' % (s, v) for s, v in worst.items() if s != (0, 0))))
    dev.engine.close()


# ---- 4. the sequence -----------------------------------------------------------------------------------------------------------------
def test_five_adam_steps_draw_the_generators_shifts_and_equal_steps_with_each_shift_pinned_by_hand():
    h, w = 37, 50
    drawn, pinned = make(h, w), make(h, w)
    drawn.set_jitter(3, 7)
    assert drawn.jitter() == {'radius': 3, 'seed': 7, 'k': 0, 'pinned': False, 'shift': jo.shift(7, 0, 3)}
    drawn.opfunc(); drawn.opfunc(False)
    assert drawn.jitter()['k'] == 0 and drawn.jitter_terms(False)[2] == jo.shift(7, 0, 3)      # st_opfunc uses shift k and leaves k alone
    pinned.set_jitter_shift(*jo.shift(7, 0, 3))
    pinned.opfunc(); pinned.opfunc(False)                                 # (the norms are captured under the same shift in both)
    for k in range(5):
        s = jo.shift(7, k, 3)
        assert s == jo.PINS[(7, 3)][k]
        pinned.set_jitter_shift(*s)
        ia, ta, la = drawn.step()
        ib, tb, lb = pinned.step()
        assert drawn.jitter_terms()[2] == s
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb, k
        assert same_bits(drawn.get_input_nchw(), pinned.get_input_nchw()), k
        info = drawn.jitter()
        assert info['k'] == k + 1 and info['shift'] == jo.shift(7, k + 1, 3)
        assert pinned.jitter()['k'] == 1                                  # (a setter zeroes the count; a pinned shift still counts)
    drawn.optimizer_reset(OPT_ADAM, 10)
    assert drawn.jitter()['k'] == 0 and drawn.jitter()['shift'] == jo.shift(7, 0, 3)
    drawn.step(); drawn.set_jitter(3, 8)
    assert drawn.jitter()['k'] == 0 and drawn.jitter()['shift'] == jo.shift(8, 0, 3)
    drawn.close(); pinned.close()


# ---- 5. pipelined iterations ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('everything', [False, True], ids=['alone', 'with_average_colours_laplacian_anchor'])
def test_two_iterations_in_flight_give_the_bytes_of_plain_steps(everything):
    h, w = 37, 52
    plain, piped = make(h, w), make(h, w)
    for eng in (plain, piped):
        if everything:
            eng.set_iterate_average(0.9)
            eng.set_original_colors(True)
            eng.set_laplacian([(4, 1.5), (16, -2.0)])
            eng.set_anchor(image(5, h, w), None, 0.7)
        eng.set_jitter(3, 7)
    want = [plain.step() for _ in range(4)]
    got = []
    for k in range(4):                                                    # one begin ahead of every end, as the worker loop runs it
        piped.step_begin()
        if k:
            got.append(piped.step_end())
    got.append(piped.step_end())
    for k, ((ia, ta, la), (ib, tb, lb)) in enumerate(zip(want, got)):
        assert len(ta) == NL + (12 if everything else 8) and np.isfinite(ta).all()
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb, k
    assert same_bits(plain.get_input_nchw(), piped.get_input_nchw()) and plain.jitter() == piped.jitter() and plain.jitter()['k'] == 4
    # ... and the shifts moved the result: the same steps with the mode off end elsewhere
    off = make(h, w)
    for _ in range(4):
        off.step()
    assert everything or not same_bits(off.get_input_nchw(), plain.get_input_nchw())
    for eng in (plain, piped, off):
        eng.close()


# ---- 6. L-BFGS ------------------------------------------------------------------------------------------------------------------------
def test_four_lbfgs_steps_follow_the_oracle_whose_shift_is_set_per_step():
    """Tolerance: loss rtol 1e-3, that of test_gpu_parity.py::test_engine_lbfgs_trajectory_matches_reference_vectors for its first five
    steps on a tiny net.  From the second step on the pair is formed from gradients of two consecutive shifts, on both sides."""
    h, w = 32, 40
    cpu, dev = transfers(h, w, 'lbfgs', 1)
    dev.engine.set_jitter(3, 7)
    for k in range(4):
        cpu.jitter_shift = jo.shift(7, k, 3)
        io, to = cpu.step()
        idv, td = dev.step()
        assert dev.engine.jitter_terms()[2] == jo.shift(7, k, 3)          # both evaluations of the first step used shift 0
        assert dev.engine.jitter()['k'] == k + 1
        print('[lbfgs step %d] loss %.9g, oracle %.9g (%.3g of the bar)' % (k, td['loss'], to['loss'], abs(td['loss'] - to['loss']) / abs(to['loss']) / 1e-3))
        assert list(td) == list(to) and np.isclose(td['loss'], to['loss'], rtol=1e-3), (k, td['loss'], to['loss'])
    dev.engine.close()


# ---- 7. off is off -------------------------------------------------------------------------------------------------------------------
def test_on_and_off_again_leaves_the_bytes_launches_and_memory_of_a_context_that_never_saw_the_call():
    off, never = make(37, 50), make(37, 50)
    for eng in (off, never):
        eng.step()                                                        # (every lazily made buffer of a step exists now)
    before = live()
    off.set_jitter(3, 7)
    assert live()[0] > before[0] and off.trace_len() == never.trace_len()
    for _ in range(2):                                                    # shifted content features are in place now
        off.opfunc()
    off.set_jitter(0)
    assert off.jitter() is None
    for call in (off.jitter_terms,):
        with pytest.raises(StError, match=r'st2 error 2: .*jitter is off'):
            call()
    # the content features were those of a shift: they come back as those of (0, 0) -- the bits below are wrong otherwise
    a, b = off.opfunc(), never.opfunc()
    assert a[0] == b[0] and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert live() == before
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
    assert p_off == p_never and sum(p_never.values()) > 0
    assert live() == before
    off.close(); never.close()


# ---- 8. the content forward is paid only when due -------------------------------------------------------------------------------------
def test_content_features_are_taken_again_only_when_the_shift_changes():
    h, w = 37, 50

    def per_eval(eng, call):
        eng.profile_read()
        call()
        return launches(eng)
    plain = make(h, w); plain.profile_enable(True); plain.opfunc()
    base = per_eval(plain, plain.opfunc)
    # style rows only: two roll_k launches more, the same convs
    for weights in (STYLE_ONLY,):
        a, b = make(h, w, weights=weights), make(h, w, weights=weights)
        for eng in (a, b):
            eng.profile_enable(True)
        a.set_jitter(3, 7)
        a.opfunc(); b.opfunc()
        for _ in range(3):
            pa, pb = per_eval(a, a.step), per_eval(b, b.step)
            assert convs(pa) == convs(pb) > 0
            assert pa.get('misc', 0) == pb.get('misc', 0) + 2             # roll and un-roll
            assert pa['finalize'] == pb['finalize'] + 1                   # scd's sums of squares in the shifted order, for scd_grad
            assert {k: v for k, v in pa.items() if k not in ('misc', 'finalize')} == {k: v for k, v in pb.items() if k not in ('misc', 'finalize')}
        a.close(); b.close()
    # a content row and a pinned shift: the first evaluation takes the features, the second finds them
    a = make(h, w); a.profile_enable(True)
    a.set_jitter_shift(-3, 2)
    first = per_eval(a, a.opfunc)
    second = per_eval(a, a.opfunc)
    assert convs(first) > convs(base) and convs(second) == convs(base)
    assert second.get('misc', 0) == base.get('misc', 0) + 2
    step_base = per_eval(plain, plain.step)
    assert convs(per_eval(a, a.step)) == convs(step_base)
    # a drawn shift: every step whose shift differs from the last takes them again (one forward to the deepest content blob)
    a.set_jitter(3, 7)
    extra = convs(first) - convs(base)
    last = (-3 % h, 2 % w)
    for k in range(4):
        s = jo.shift(7, k, 3)
        now = (s[0] % h, s[1] % w)
        p = per_eval(a, a.step)
        assert convs(p) == convs(step_base) + (extra if now != last else 0), (k, s)
        assert p.get('misc', 0) == step_base.get('misc', 0) + (3 if now != last and now != (0, 0) else 2), (k, s)      # + roll of the content
        last = now
    a.close(); plain.close()


# ---- 9. refusals, the worker ----------------------------------------------------------------------------------------------------------
def test_refusals_each_with_its_message():
    eng = make(16, 16)
    for radius in (-1, 4097):
        with pytest.raises(StError, match=r'st2 error 1: .*radius must be 0 \(off\) or inside \[1, 4096\], not %d' % radius):
            eng.set_jitter(radius, 0)
        assert eng.jitter() is None
    with pytest.raises(StError, match=r'st2 error 2: .*jitter is off'):
        eng.jitter_terms()
    eng.set_jitter(4096, jo.MASK64)
    assert eng.jitter()['seed'] == jo.MASK64 and eng.jitter()['shift'] == jo.shift(jo.MASK64, 0, 4096)
    with pytest.raises(StError, match=r'st2 error 2: .*no objective evaluation'):
        eng.jitter_terms()
    eng.opfunc(False)
    assert eng.jitter_terms(False)[2] == jo.shift(jo.MASK64, 0, 4096)
    with pytest.raises(StError, match=r'st2 error 2: .*no gradient'):
        eng.jitter_terms()
    set_weights(eng, {'content': {}, 'style': {}, 'deepdream': {}})
    eng.opfunc()
    with pytest.raises(StError, match=r'st2 error 2: .*no active row'):
        eng.jitter_terms()
    set_weights(eng)
    eng.opfunc()
    eng.jitter_terms()
    eng.resample_state((24, 40))
    with pytest.raises(StError, match=r'st2 error 2: .*resized'):
        eng.jitter_terms()
    eng.resample_content((24, 40))
    eng.opfunc()
    xs, scd, _ = eng.jitter_terms()
    assert xs.shape == scd.shape == (1, 3, 24, 40)
    eng.step_begin()
    for call in (lambda: eng.set_jitter(3, 7), lambda: eng.set_jitter(0), lambda: eng.set_jitter_shift(1, 1)):
        with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
            call()
    eng.step_end()
    assert eng.jitter()['radius'] == 4096
    with pytest.raises(StError, match=r'st2 error 2: .*jitter'):           # st_tile_configure with the mode on
        capi.check(eng.lib.st_tile_configure(eng._ctx, 24, 40, 0, 0, 0, 0, 24, 40))
    eng.set_jitter(0)
    capi.check(eng.lib.st_tile_configure(eng._ctx, 24, 40, 0, 0, 0, 0, 24, 40))
    for call in (lambda: eng.set_jitter(3, 7), lambda: eng.set_jitter_shift(1, 1)):
        with pytest.raises(StError, match=r'st2 error 2: .*tile-configured'):
            call()
    eng.set_jitter(0)                                                     # (off stays allowed)
    eng.close()


def _model():
    return st2.HipModel(NET, topology=TOPO)


def _direct(jitter, n):
    ref = st2.StyleTransfer(_model())
    ref.set_input(image(3, 32, 40)); ref.set_content(image(1, 32, 40)); ref.set_style(image(2, 24, 24)); ref.reset()
    ref.set_weights(WEIGHTS, PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    if jitter is not None:
        ref.engine.set_jitter(*jitter)
    assert ref.start()
    return [ref.step() for _ in range(n)]


def test_worker_runs_the_mode_from_the_config_key(monkeypatch):
    """Worker(config) on its own TCP sockets (pyzmq where it is installed, otherwise tests/minizmq.py) with `jitter = 3:7`: the iterates
    are those of an engine driven by hand with st_set_jitter(3, 7), bit for bit, and the trace keeps its names."""
    from test_boundary import zmq_module
    zmq, which = zmq_module(monkeypatch)
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app, 'jitter': '3:7'}
    wk = worker_mod.Worker(config, transfer=st2.StyleTransfer(_model()))
    assert wk.transfer.engine.jitter()['radius'] == 3 and wk.transfer.engine.jitter()['seed'] == 7
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
    by_hand, plain = _direct((3, 7), len(its)), _direct(None, 1)
    for m, (img, tr) in zip(its, by_hand):
        assert m.image.dtype == F32 and np.array_equal(m.image, img), 'iterate %d differs' % m.i
        assert list(m.trace) == list(tr) and all(m.trace[k] == tr[k] for k in tr if k != 'time')
    assert list(its[0].trace) == list(plain[0][1])
    assert not np.array_equal(its[0].image, plain[0][0])
