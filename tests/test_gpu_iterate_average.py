"""Iterate averaging on the real engine (``pytest -m gpu``): st_set_iterate_average makes st_step / st_step_end hand out the
bias-corrected exponentially weighted mean of the iterates (utils.DecayingMean, utils.py:49-69, over x after every optimizer step).
The engine is held BIT FOR BIT to the NumPy float32 restatement in tests/average_oracle.py (itself pinned to the reference's class by
tests/golden/iterate_average.npz), fed with get_input_nchw() of every step.

Sizes: 16 x 32 (plane a multiple of 4: the 16-byte path), 18 x 34 (plane a multiple of 4, width not: the 16-byte path across row
ends), 17 x 33 (odd plane: the channel planes are misaligned and the one-pixel-per-thread path runs); 725 x 725 and 1450 x 1448, two
steps each, are the smallest at which the threads of either path stride on to further pixels.  Tiny VGG-shaped nets."""
from ctypes import byref, c_longlong
import threading

import numpy as np
import pytest

import messages
import oracle
import style_transfer2_amd as st2
from average_oracle import AverageOracle, deprocess
from helpers import load
from style_transfer2_amd import capi, jobs, tiled, tiling
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS, Engine
from style_transfer2_amd.tile_backend import HipTileBackend
from style_transfer2_amd.transfer import LOSS_NAMES, SCALAR_LOSS_NAMES, weight_table
import worker as worker_mod

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO = oracle.tiny_topology((8, 16), (2, 2))
NET = oracle.he_init_weights(TOPO, 0, 0.1)
WEIGHTS = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
OTHER_WEIGHTS = {'content': {'conv2_1': 0.05}, 'style': {'conv1_2': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
D = 0.9


def image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def set_weights(eng, weights):
    rows, cells = weight_table(weights)
    cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
    eng.set_weights(rows, cols[0], cols[1], cols[2], [PARAMS[k] for k in SCALAR_LOSS_NAMES])


def make(h, w, kind=OPT_ADAM, decay=None):
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    eng.set_input(image(3, h, w))
    eng.set_content(image(1, h, w))
    eng.set_style(image(2, 24, 24))
    set_weights(eng, WEIGHTS)
    eng.optimizer_reset(kind, 10 if kind == OPT_ADAM else 1)
    if decay is not None:
        eng.set_iterate_average(decay)
    return eng


def live():
    dev, pin = c_longlong(-1), c_longlong(-1)
    capi.check(capi.load_library().st_live_bytes(byref(dev), byref(pin)))
    return dev.value, pin.value


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def follows(eng, avg, img):
    """The engine's state and the image it just handed out are the restatement's, fed with the iterate of this step."""
    avg.update(eng.get_input_nchw())
    decay, items, mean = eng.iterate_average()
    assert decay == avg.decay and items == avg.items
    assert np.array_equal(mean, avg.mean), float(np.abs(mean - avg.mean).max())
    if img is not None:
        assert img.dtype == F32 and np.array_equal(img, avg.image()), float(np.abs(img - avg.image()).max())


# ---- 1. bit-exactness against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,kind,steps', [(16, 32, OPT_ADAM, 6), (18, 34, OPT_ADAM, 6), (17, 33, OPT_ADAM, 6), (17, 33, OPT_LBFGS, 4),
                                            # more work than the launch's 2048 workgroups take in one pass: a thread strides to further
                                            # pixels from 2048 * 256 pixels on the one-pixel path (725 x 725 is odd) and from four times as
                                            # many on the 16-byte path (1450 x 1448)
                                            (725, 725, OPT_ADAM, 2), (1450, 1448, OPT_ADAM, 2)])
def test_averaged_image_and_raw_mean_equal_the_restatement_after_every_step(h, w, kind, steps):
    eng = make(h, w, kind, D)
    avg = AverageOracle(D)
    assert eng.iterate_average() == (D, 0, None)
    for _ in range(steps):
        img, _, loss = eng.step()
        assert np.isfinite(loss)
        follows(eng, avg, img)
    # (the averaged image is not the raw iterate: the check above is not vacuous)
    assert not np.array_equal(img, deprocess(eng.get_input_nchw()))
    eng.close()


# ---- 2. the trajectory is undisturbed; mode off launches what a context that never heard of the mode launches ---------------------
def test_trajectory_trace_and_launch_counts_are_those_of_the_mode_off():
    on, off, never = make(16, 32, decay=D), make(16, 32), make(16, 32)
    off.set_iterate_average(D)
    off.set_iterate_average(0.0)                    # on and off again: "off" must be as good as never
    for eng in (on, off, never):
        eng.profile_enable(True)
        eng.profile_read()
    for _ in range(6):
        r_on, r_off, r_never = on.step(), off.step(), never.step()
        assert same_bits(on.get_input_nchw(), off.get_input_nchw()) and same_bits(off.get_input_nchw(), never.get_input_nchw())
        assert np.array_equal(r_on[1], r_off[1]) and np.array_equal(r_off[1], r_never[1]) and r_on[2] == r_off[2] == r_never[2]
        assert same_bits(r_off[0], r_never[0]) and same_bits(r_off[0], deprocess(off.get_input_nchw()))
    p_on, p_off, p_never = ({k: v['launches'] for k, v in e.profile_read().items()} for e in (on, off, never))
    assert p_off == p_never and sum(p_never.values()) > 0
    assert p_on == p_never                          # with an image wanted the averaged step launches no more kernels than the plain one
    for _ in range(2):                              # without an image: exactly one launch more per step, booked as misc
        on.step(want_image=False, want_trace=False); never.step(want_image=False, want_trace=False)
    on.sync(); never.sync()
    p_on, p_never = ({k: v['launches'] for k, v in e.profile_read().items()} for e in (on, never))
    assert p_on.get('misc', 0) == p_never.get('misc', 0) + 2
    assert {k: v for k, v in p_on.items() if k != 'misc'} == {k: v for k, v in p_never.items() if k != 'misc'}
    for eng in (on, off, never):
        eng.close()


# ---- 3. steps that hand out no image count ---------------------------------------------------------------------------------------
def test_steps_without_an_image_update_the_mean():
    quiet, loud = make(17, 33, decay=D), make(17, 33, decay=D)
    for _ in range(3):
        quiet.step(want_image=False, want_trace=False)
        loud.step()
    a, b = quiet.step()[0], loud.step()[0]
    assert same_bits(a, b) and quiet.iterate_average()[1] == 4
    assert same_bits(quiet.iterate_average()[2], loud.iterate_average()[2])
    quiet.close(); loud.close()


# ---- 4. the pipelined halves, one iteration ahead, with and without a frame room ---------------------------------------------------
@pytest.mark.parametrize('h,w', [(16, 32), (17, 33)])
@pytest.mark.parametrize('room', [False, True])
def test_step_begin_and_end_give_the_images_of_step(h, w, room):
    plain, piped = make(h, w, decay=D), make(h, w, decay=D)
    want = [plain.step() for _ in range(6)]
    if room:
        piped.set_frame_room(64, 32)
    got = []

    def collect():
        if room:
            view, trace, loss, buf = piped.step_end(copy=False, room=True)
            assert len(buf) == 4096 + view.nbytes + 32
            got.append((view.copy(), trace, loss))
        else:
            got.append(piped.step_end())
    for k in range(6):                              # one begin ahead of every end, as the worker loop runs it
        piped.step_begin()
        if k:
            collect()
    collect()
    assert piped.steps_pending() == 0
    for (ia, ta, la), (ib, tb, lb) in zip(want, got):
        assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb
    assert same_bits(plain.iterate_average()[2], piped.iterate_average()[2]) and piped.iterate_average()[1] == 6
    plain.close(); piped.close()


# ---- 5. lifetime ------------------------------------------------------------------------------------------------------------------
def test_lifetime_of_the_mean():
    eng = make(16, 32)
    eng.step()                                      # (every lazily made buffer of a step exists now)
    before = live()
    eng.set_iterate_average(D)
    assert live() == (before[0] + 3 * 16 * 32 * 4, before[1])            # one image, counted like everything else
    avg = AverageOracle(D)
    for _ in range(2):
        follows(eng, avg, eng.step()[0])
    # kept across objective_changed and set_weights (and the step size)
    eng.objective_changed()
    set_weights(eng, OTHER_WEIGHTS)
    eng.optimizer_set_step(5)
    assert eng.iterate_average()[1] == 2
    follows(eng, avg, eng.step()[0])
    # cleared by optimizer_reset
    eng.optimizer_reset(OPT_ADAM, 10)
    assert eng.iterate_average() == (D, 0, None)
    with pytest.raises(StError, match=r'st2 error 2: .*empty'):          # the raw mean of an empty average
        capi.check(eng.lib.st_get_iterate_average(eng._ctx, None, None, np.empty((1, 3, 16, 32), F32).ctypes.data))
    avg.clear()
    follows(eng, avg, eng.step()[0])
    # ... by set_input at the same size
    eng.set_input(image(4, 16, 32))
    assert eng.iterate_average() == (D, 0, None)
    avg.clear()
    follows(eng, avg, eng.step()[0])
    # ... by the setter itself
    eng.set_iterate_average(0.5)
    assert eng.iterate_average() == (0.5, 0, None)
    avg = AverageOracle(0.5)
    follows(eng, avg, eng.step()[0])
    # refused values: status 1 and a message; nothing changes
    for bad in (1.0, -0.1, float('nan'), 2.0):
        with pytest.raises(StError, match=r'st2 error 1: .*decay'):
            eng.set_iterate_average(bad)
    assert eng.iterate_average()[:2] == (0.5, 1)
    # refused with an iteration in flight
    eng.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_iterate_average(D)
    img = eng.step_end()[0]
    follows(eng, avg, img)
    # ... and by set_input at another size (the buffer follows the input buffers)
    eng.set_input(image(5, 18, 34)); eng.set_content(image(6, 18, 34))
    assert eng.iterate_average() == (0.5, 0, None)
    avg.clear()
    follows(eng, avg, eng.step()[0])
    assert eng.iterate_average()[2].shape == (1, 3, 18, 34)
    eng.close()


def test_turning_the_mode_off_gives_the_memory_back():
    eng = make(17, 33)
    eng.step()
    before = live()
    eng.set_iterate_average(D)
    eng.step(); eng.step(want_image=False, want_trace=False)
    assert live()[0] == before[0] + 3 * 17 * 33 * 4
    eng.set_iterate_average(0.0)
    assert live() == before and eng.iterate_average() == (0.0, 0, None)
    img = eng.step()[0]
    assert same_bits(img, deprocess(eng.get_input_nchw()))                # the raw iterate again
    eng.close()


# ---- 6. resample ------------------------------------------------------------------------------------------------------------------
def test_resample_state_resamples_the_raw_mean_and_a_new_image_clears_it():
    """The resampled mean is held to Pillow (resample.resample_nchw on the restatement's mean) by the criterion of the existing
    resample test, tests/test_resample.py::same, which is what Pillow itself allows: equal bit for bit except that, on some hosts, one
    element in about 10^4 is 1 ulp off (Pillow's build rounds a sum formed with a fused multiply-add).  The x of the same call is held
    to the same criterion there.  The restatement then continues from the engine's resampled mean, so that the steps after the
    resample are held bit for bit again."""
    from test_resample import same
    eng = make(16, 32, decay=D)
    avg = AverageOracle(D)
    for _ in range(3):
        follows(eng, avg, eng.step()[0])
    x_before = eng.get_input_nchw()
    eng.resample_state((24, 40)); eng.resample_content((24, 40))
    avg.resample((24, 40))                          # Pillow's Lanczos on the raw mean (resample.resample_nchw)
    decay, items, mean = eng.iterate_average()
    assert (decay, items) == (D, 3) and mean.shape == (1, 3, 24, 40)
    off = mean != avg.mean
    print('[resampled mean] %d of %d elements differ from Pillow, largest relative difference %.3g'
          % (int(off.sum()), mean.size, float((np.abs(mean - avg.mean) / np.maximum(np.abs(avg.mean), 1e-30)).max())))
    from style_transfer2_amd import resample
    x_off = eng.get_input_nchw() != resample.resample_nchw(x_before, (24, 40))
    print('[resampled x, same call] %d of %d elements differ from Pillow' % (int(x_off.sum()), x_off.size))
    assert same(mean, avg.mean)
    avg.mean = mean.copy()
    eng.objective_changed()
    for _ in range(2):
        follows(eng, avg, eng.step()[0])
    assert avg.items == 5
    new_x = (np.random.RandomState(7).randn(1, 3, 16, 32) * 40).astype(F32)
    eng.resample_state(None, new_x=new_x); eng.resample_content((16, 32))
    avg.resample((16, 32), new_x=True)
    assert eng.iterate_average() == (D, 0, None)
    eng.objective_changed()
    follows(eng, avg, eng.step()[0])
    assert avg.items == 1
    eng.close()


# ---- 7. tile-sharded --------------------------------------------------------------------------------------------------------------
def _tile_of_window(backend):
    """This rank's tile of the current iterate, preprocessed (3, th, tw): cut from the window st_get_input_nchw returns."""
    t, w = backend.grid.tiles[backend.rank], backend.grid.windows[backend.rank]
    return backend.engine.get_input_nchw()[0][:, t.y0 - w.y0:t.y1 - w.y0, t.x0 - w.x0:t.x1 - w.x0]


def test_fused_tile_steps_average_every_ranks_tile_bit_for_bit():
    """1 x 2 grid over the in-process fabric, 32 x 64, 3 fused Adam steps then 3 fused L-BFGS steps: every rank's
    st_tile_get_tile_average is the restatement over that rank's sequence of tiles.  The sequence is taken preprocessed, from the
    window st_get_input_nchw returns (st_tile_get_tile hands out the same pixels with the channel mean added, which is checked, but
    x + mean - mean does not give x back bit for bit)."""
    h, w = 32, 64
    content, style, init = image(1, h, w), image(2, 24, 40), image(3, h, w)
    grid = tiling.TileGrid(h, w, 1, 2, TOPO, len(TOPO))
    fabric = tiled.InProcessFabric(2, timeout=120.0)
    backends = []
    for r in range(2):
        b = HipTileBackend(NET, grid, r, content, style, init, WEIGHTS, PARAMS, step_size=10, topology=TOPO, iterate_average=D)
        b.comm_init_local(r, 2, fabric)
        backends.append(b)
    ranks = [tiled.FusedTiledTransfer(grid, r, b) for r, b in enumerate(backends)]
    for b, rank in zip(backends, ranks):
        assert not b.averaging() and same_bits(rank.tile_image(), b.tile_image())      # nothing averaged yet: the raw tile
    for kind, step in ((OPT_ADAM, 10), (OPT_LBFGS, 1)):
        for b in backends:
            b.engine.optimizer_reset(kind, step)                                        # (clears the mean)
            assert b.engine.iterate_average() == (D, 0, None)
        avgs = [AverageOracle(D) for _ in backends]
        for i in range(3):
            out = tiled.run_in_process(ranks, 1, fabric)
            assert all(np.isfinite(o[-1][-2]) for o in out)
            for b, rank, avg in zip(backends, ranks, avgs):
                x = _tile_of_window(b)
                assert same_bits(b.tile_image(), deprocess(x))                          # st_tile_get_tile: the raw iterate, as before
                avg.update(x)
                got = b.averaged_image()
                assert b.engine.iterate_average()[1] == i + 1
                assert np.array_equal(got, avg.image()), (kind, i, b.rank, float(np.abs(got - avg.image()).max()))
                assert same_bits(rank.tile_image(), got)                                # what the fused driver hands out
                assert not np.array_equal(got, b.tile_image())
    # the aprons carry the neighbour's mean: the raw means of the two windows agree where the windows overlap
    w0, w1 = grid.windows
    m0, m1 = (b.engine.iterate_average()[2][0] for b in backends)
    x_lo, x_hi = max(w0.x0, w1.x0), min(w0.x1, w1.x1)
    assert x_hi > x_lo and same_bits(m0[:, :, x_lo - w0.x0:x_hi - w0.x0], m1[:, :, x_lo - w1.x0:x_hi - w1.x0])
    for b in backends:
        b.engine.close()


def test_phase_by_phase_tile_driver_does_not_average():
    h, w = 32, 48
    grid = tiling.TileGrid(h, w, 1, 1, TOPO, len(TOPO))
    b = HipTileBackend(NET, grid, 0, image(1, h, w), image(2, 24, 40), image(3, h, w), WEIGHTS, PARAMS, step_size=10, topology=TOPO,
                       iterate_average=D)
    tt = tiled.TiledTransfer(grid, 0, b, tiled.Comm())
    for _ in range(2):
        tt.step()
    assert b.engine.iterate_average() == (D, 0, None) and not b.averaging()
    with pytest.raises(StError, match=r'st2 error 2: .*empty.*st_tile_step'):
        b.averaged_image()
    assert b.tile_image().shape == (h, w, 3)
    b.engine.set_iterate_average(0.0)
    with pytest.raises(StError, match=r'st2 error 2: .*off'):
        b.averaged_image()
    b.engine.close()


def test_run_tiled_job_with_averaging_equals_run_job_with_averaging():
    """The example pair at 256 px, ten Adam iterations, both jobs with iterate_average = 0.9: the bar is the one
    tests/test_gpu_jobs.py holds the same pair of jobs to without averaging (image MSE <= 0.05).  Averaging is a contraction (a
    convex combination of iterates, divided by the sum of its weights), so it cannot widen the distance."""
    from PIL import Image
    src = load('config1_sources.npz')
    content, style = Image.fromarray(src['golden_gate']), Image.fromarray(src['starry_night'])
    params = oracle.he_init_weights(oracle.VGG19_TOPOLOGY, seed=0)
    dev = st2.StyleTransfer(st2.HipModel(params))
    whole = jobs.run_job(dev, content, style, 10, size=256, optimizer='adam', seed=5, iterate_average=D)
    assert dev.engine.iterate_average()[:2] == (D, 10) and not np.array_equal(whole, deprocess(dev.engine.get_input_nchw()))
    tiles = jobs.run_tiled_job(params, content, style, 10, (2, 2), size=256, seed=5, iterate_average=D)
    assert tiles.shape == whole.shape == (192, 256, 3) and tiles.dtype == F32
    mse = float(np.mean((tiles.astype(np.float64) - whole) ** 2))
    print('[tiled job 2x2 at 192x256, iterate_average 0.9] image MSE %.3g against the whole-image job after 10 Adam iterations' % mse)
    assert mse <= 0.05


# ---- 8. the worker, end to end ----------------------------------------------------------------------------------------------------
def _model():
    return st2.HipModel(NET, topology=TOPO)


def _direct(decay, n):
    ref = st2.StyleTransfer(_model())
    ref.set_input(image(3, 32, 40)); ref.set_content(image(1, 32, 40)); ref.set_style(image(2, 24, 24)); ref.reset()
    ref.set_weights(WEIGHTS, PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    if decay:
        ref.engine.set_iterate_average(decay)
    assert ref.start()
    return [ref.step() for _ in range(n)]


def test_worker_with_the_config_key_sends_averaged_iterates(monkeypatch):
    """Worker(config) on its own TCP sockets (pyzmq where it is installed, otherwise tests/minizmq.py) with iterate_average = 0.9: the
    Iterate images are those of an engine driven directly with the mode on; Iterate.i, the trace keys and their order are those of a
    plain run."""
    from test_boundary import zmq_module
    zmq, which = zmq_module(monkeypatch)
    print('[transport] GPU worker ran over', which)
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app, 'iterate_average': '0.9'}
    wk = worker_mod.Worker(config, transfer=st2.StyleTransfer(_model()))
    assert wk.transfer.engine.iterate_average()[0] == 0.9 and wk.pipelined
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
    while sum(isinstance(m, messages.Iterate) for m in got) < 6 and poller.poll(20000):
        got.append(app_in.recv_pyobj())
    app_out.send_pyobj(messages.Shutdown())
    while poller.poll(20000):
        got.append(app_in.recv_pyobj())
        if isinstance(got[-1], messages.Shutdown):
            break
    th.join(30)
    wk.close()
    app_out.close(0); app_in.close(0); ctx.destroy(0)
    kinds = [type(m).__name__ for m in got]
    its = [m for m in got if isinstance(m, messages.Iterate)]
    n = len(its)
    assert n >= 6 and kinds == ['WorkerReady'] + ['Iterate'] * n + ['Shutdown']
    assert [m.i for m in its] == list(range(1, n + 1))
    averaged, plain = _direct(D, n), _direct(0.0, n)
    for m, (img, tr), (raw, tr_plain) in zip(its, averaged, plain):
        assert m.image.dtype == F32 and np.array_equal(m.image, img), 'iterate %d differs' % m.i
        assert list(m.trace) == list(tr_plain) and m.trace['fevals'] == m.i
        assert all(m.trace[k] == tr_plain[k] for k in tr_plain if k != 'time')
    assert not np.array_equal(its[-1].image, plain[-1][0])
