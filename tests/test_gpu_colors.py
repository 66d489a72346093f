"""The content's colours on the real engine (``pytest -m gpu``): luminance-only output (st_set_original_colors) and the colour-matched
style image (st_set_style_color_match / st_set_style_transform).  The luminance forms of csrc/emit.hip and the kernels of csrc/color.hip
are held BIT FOR BIT to the NumPy float32 restatements in tests/color_oracle.py (emission fed with get_input_nchw() and get_content_nchw(); recolour fed with the engine's A, b),
the moments to float64 NumPy within the bound of a double summation, the transform to the float64 oracle within 1 ulp of fp32.

Sizes: 16 x 32 (plane a multiple of 4: the 16-byte path), 18 x 34 (plane a multiple of 4, width not: the 16-byte path across row ends),
17 x 33 (odd plane: the one-pixel-per-thread path).  emit_k (csrc/emit.hip) is launched on at most 2048 workgroups of
256 threads: a thread strides on to further pixels from 2048 * 256 = 524288 pixels on the one-pixel path -- 725 x 725 = 525625, odd, is the
smallest square beyond it -- and from four times as many on the 16-byte path -- 1450 x 1448 = 2099600 (a multiple of 4) against 2097152.
image_moments_k runs at most 256 workgroups of 256 threads, one pixel per thread and pass: 257 x 256 pixels exceed one pass.
Tiny VGG-shaped nets."""
import threading
from ctypes import POINTER, c_float

import numpy as np
import pytest

import color_oracle as co
import messages
import oracle
import style_transfer2_amd as st2
from average_oracle import AverageOracle, deprocess
from style_transfer2_amd import capi, jobs, tile_backend, tiled, tiling
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
STYLE_ONLY = {'content': {}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
D = 0.9
SMALL = [(16, 32), (18, 34), (17, 33)]
STRIDING = [(725, 725), (1450, 1448)]


def image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def set_weights(eng, weights):
    rows, cells = weight_table(weights)
    cols = [[cells[k][r] for r in rows] for k in LOSS_NAMES]
    eng.set_weights(rows, cols[0], cols[1], cols[2], [PARAMS[k] for k in SCALAR_LOSS_NAMES])


def make(h, w, kind=OPT_ADAM, decay=None, colors=True, content=True, weights=WEIGHTS):
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    eng.set_input(image(3, h, w))
    if content:
        eng.set_content(image(1, h, w))
    eng.set_style(image(2, 24, 24))
    set_weights(eng, weights)
    eng.optimizer_reset(kind, 10 if kind == OPT_ADAM else 1)
    if decay is not None:
        eng.set_iterate_average(decay)
    if colors:
        eng.set_original_colors(True)
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def bits_off(a, b):
    return 'largest difference %g' % float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ---- 1. emission, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,kind,steps', [(h, w, k, 3) for h, w in SMALL for k in (OPT_ADAM, OPT_LBFGS)] + [(h, w, OPT_ADAM, 2) for h, w in STRIDING])
def test_step_hands_out_the_iterates_luminance_with_the_contents_chroma(h, w, kind, steps):
    eng = make(h, w, kind)
    assert eng.color_modes()[:2] == (True, 0)
    cx = eng.get_content_nchw()
    for _ in range(steps):
        img, _, loss = eng.step()
        assert np.isfinite(loss)
        want = co.emit_luma(eng.get_input_nchw(), cx)
        assert img.dtype == F32 and same_bits(img, want), bits_off(img, want)
    assert not np.array_equal(img, deprocess(eng.get_input_nchw()))           # (not the raw iterate: the check is not vacuous)
    eng.set_original_colors(False)
    assert same_bits(eng.step()[0], deprocess(eng.get_input_nchw()))          # off: the raw iterate again
    eng.close()


@pytest.mark.parametrize('h,w,kind,steps', [(h, w, k, 3) for h, w in SMALL for k in (OPT_ADAM, OPT_LBFGS)] + [(h, w, OPT_ADAM, 2) for h, w in STRIDING])
def test_with_iterate_averaging_the_mean_state_and_the_image_follow_the_restatements(h, w, kind, steps):
    eng = make(h, w, kind, decay=D)
    avg = AverageOracle(D)
    cx = eng.get_content_nchw()
    for _ in range(steps):
        img = eng.step()[0]
        avg.update(eng.get_input_nchw())
        decay, items, mean = eng.iterate_average()
        assert (decay, items) == (D, avg.items) and same_bits(mean, avg.mean), bits_off(mean, avg.mean)
        want = co.emit_luma_averaged(avg, cx)
        assert same_bits(img, want), bits_off(img, want)
    assert not np.array_equal(img, avg.image()) and not np.array_equal(img, co.emit_luma(eng.get_input_nchw(), cx))
    eng.close()


@pytest.mark.parametrize('h,w', [(16, 32), (17, 33)])
@pytest.mark.parametrize('decay', [None, D])
@pytest.mark.parametrize('depth', [1, 2])
def test_step_begin_and_end_hand_out_the_same_images(h, w, decay, depth):
    """`depth` iterations in flight: every begin's iterate is read (st_get_input_nchw waits for the stream) and the image st_step_end
    hands out for it is the restatement's."""
    eng = make(h, w, decay=decay)
    cx = eng.get_content_nchw()
    avg = AverageOracle(D) if decay else None
    want, got = [], []
    for k in range(6):
        eng.step_begin()
        x = eng.get_input_nchw()
        if avg is not None:
            avg.update(x)
            want.append(co.emit_luma_averaged(avg, cx))
        else:
            want.append(co.emit_luma(x, cx))
        if eng.steps_pending() == depth:
            got.append(eng.step_end()[0])
    while eng.steps_pending():
        got.append(eng.step_end()[0])
    assert len(got) == 6
    for a, b in zip(got, want):
        assert same_bits(a, b), bits_off(a, b)
    eng.close()


@pytest.mark.parametrize('kind', [OPT_ADAM, OPT_LBFGS])
def test_emission_changes_nothing_upstream(kind):
    on, off = make(17, 33, kind, decay=D, colors=True), make(17, 33, kind, decay=D, colors=False)
    for k in range(5):
        (ia, ta, la), (ib, tb, lb) = on.step(), off.step()
        assert same_bits(on.get_input_nchw(), off.get_input_nchw()) and np.array_equal(ta, tb) and la == lb
        assert same_bits(on.iterate_average()[2], off.iterate_average()[2]) and on.iterate_average()[1] == k + 1
        assert not np.array_equal(ia, ib)
    on.close(); off.close()


def test_after_a_resample_emission_follows_the_resampled_tensors():
    eng = make(16, 32)
    for _ in range(2):
        eng.step()
    eng.resample_state((24, 40)); eng.resample_content((24, 40))
    eng.objective_changed()
    cx = eng.get_content_nchw()
    assert cx.shape == (1, 3, 24, 40)
    for _ in range(2):
        img = eng.step()[0]
        want = co.emit_luma(eng.get_input_nchw(), cx)
        assert img.shape == (24, 40, 3) and same_bits(img, want), bits_off(img, want)
    eng.close()


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['no content', 'content of another size'])
def test_a_refused_emission_enqueues_nothing(case):
    def fresh(colors):
        eng = make(16, 32, colors=colors, content=False, weights=STYLE_ONLY)
        if case != 'no content':
            eng.set_content(image(1, 18, 34))
        return eng
    eng, twin = fresh(True), fresh(False)
    pattern = r'st2 error 2: .*no content image' if case == 'no content' else r'st2 error 2: .*18 x 34.*16 x 32'
    for _ in range(2):
        with pytest.raises(StError, match=pattern):
            eng.step()
        with pytest.raises(StError, match=pattern):
            eng.step_begin()
        assert eng.steps_pending() == 0
    # the next legal step (no image wanted), then one with the mode off: the bits of an engine that never saw the refused calls
    eng.step(want_image=False, want_trace=False); twin.step(want_image=False, want_trace=False)
    assert same_bits(eng.get_input_nchw(), twin.get_input_nchw())
    eng.set_original_colors(False)
    (ia, ta, la), (ib, tb, lb) = eng.step(), twin.step()
    assert same_bits(ia, ib) and np.array_equal(ta, tb) and la == lb
    eng.close(); twin.close()


def test_the_mode_is_not_switched_with_an_iteration_in_flight():
    eng = make(16, 32, colors=False)
    eng.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        eng.set_original_colors(True)
    assert eng.color_modes()[0] is False and eng.steps_pending() == 1
    assert same_bits(eng.step_end()[0], deprocess(eng.get_input_nchw()))
    eng.set_original_colors(True)
    assert eng.color_modes()[0] is True
    eng.close()


# ---- 3. moments -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bare():
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    yield eng
    eng.close()


@pytest.mark.parametrize('h,w', SMALL + [(257, 256), (725, 725)])
@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_moments_lie_within_the_bound_of_a_double_summation(bare, h, w, dtype):
    """The nine sums are rebuilt from what the ABI returns (sum_c = (mean_c - kMean_c) N, sum_ck = (cov_ck + m_c m_k) N, in double: that
    adds a few relative 2^-53 of the sum itself, where the bound allows 2 N 2^-53 of the sum of the terms' magnitudes, N >= 512) and
    each must lie within 2 N 2^-53 sum|terms| of float64 NumPy: products of fp32 values are exact in double, only the additions round."""
    r = np.random.RandomState(h * w)
    img = image(h, h, w) if dtype == 'uint8' else r.uniform(0, 255, (h, w, 3)).astype(F32)
    mean, cov = bare.image_moments(img)
    again = bare.image_moments(img)
    assert np.array_equal(mean, again[0]) and np.array_equal(cov, again[1])             # a fixed order: the same bits
    n = h * w
    want, mags = co.moment_sums(co.preprocess(img))
    m = mean - co.MEAN64
    got = np.concatenate([m * n, [(cov[a, b] + m[a] * m[b]) * n for a in range(3) for b in range(a, 3)]])
    bound = 2 * n * 2.0 ** -53 * mags
    print('[moments %dx%d %s] largest |sum - oracle| / bound = %.3g' % (h, w, dtype, float((np.abs(got - want) / bound).max())))
    assert (np.abs(got - want) <= bound).all(), (got - want, bound)
    wm, wc = co.moments(co.preprocess(img))
    assert np.allclose(mean, wm, rtol=1e-12, atol=1e-10) and np.allclose(cov, wc, rtol=1e-9, atol=1e-6) and np.array_equal(cov, cov.T)


# ---- 4. transform, recolour, targets --------------------------------------------------------------------------------------------------
def matched(content, style):
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    eng.set_style_color_match(True)
    eng.set_content(content)
    eng.set_style(style)
    return eng


@pytest.mark.parametrize('kind', ['random style', 'grey style'])
def test_the_engines_transform_is_the_oracles_on_the_engines_own_moments(kind):
    content, style = co.image_pairs()[kind]
    eng = matched(content, style)
    oc, sm, A, b = eng.color_modes()
    assert (oc, sm) == (False, 1) and np.isfinite(A).all() and np.isfinite(b).all()
    (mc, cc), (ms, cs) = eng.image_moments(content), eng.image_moments(style)
    wa, wb = co.transform(mc, cc, ms, cs)
    ua, ub = co.ulps(A, wa), co.ulps(b, wb)
    print('[%s] A within %g ulp, b within %g ulp of float32(oracle)' % (kind, ua, ub))
    assert ua <= 1 and ub <= 1
    a2, b2 = st2.color_transform(mc, cc, ms, cs)                            # the host-only entry point: the same arithmetic
    assert same_bits(A, a2) and same_bits(b, b2)
    assert not np.allclose(A, np.eye(3), atol=1e-3)
    eng.close()


@pytest.mark.parametrize('h,w', [(24, 40), (17, 33)])
def test_recolour_equals_the_restatement_bit_for_bit(h, w):
    """24 x 40: the 16-byte path; 17 x 33 (odd plane): one pixel per thread.  Under colour matching, then under a given transform."""
    content, style = image(1, 16, 32), co.tinted(4, h, w)
    eng = matched(content, style)
    got = eng.style_recolor(style)
    _, _, A, b = eng.color_modes()
    want = co.recolor(co.preprocess(style)[None], A, b)
    assert got.shape == (1, 3, h, w) and same_bits(got, want), bits_off(got, want)
    assert not np.array_equal(got[0], co.preprocess(style))
    A2 = np.array(((0.5, 0.25, -0.125), (0.0625, 1.5, 0.3), (-0.7, 0.2, 0.9)), F32)
    b2 = np.array((3.5, -20.25, 0.1), F32)
    eng.set_style_transform(A2, b2)
    assert eng.color_modes()[1] == 2 and same_bits(eng.color_modes()[2], A2) and same_bits(eng.color_modes()[3], b2)
    got = eng.style_recolor(style)
    want = co.recolor(co.preprocess(style)[None], A2, b2)
    assert same_bits(got, want), bits_off(got, want)
    eng.set_style_transform(None, None)
    assert eng.color_modes()[1] == 0 and same_bits(eng.style_recolor(style)[0], co.preprocess(style))
    for bad_a, bad_b in ((A2, None), (None, b2), (A2 * np.nan, b2)):          # one NULL, a non-finite entry: refused, nothing changes
        pa = None if bad_a is None else np.ascontiguousarray(bad_a, F32).ctypes.data_as(POINTER(c_float))
        pb = None if bad_b is None else np.ascontiguousarray(bad_b, F32).ctypes.data_as(POINTER(c_float))
        with pytest.raises(StError, match=r'st2 error 1'):
            capi.check(eng.lib.st_set_style_transform(eng._ctx, pa, pb))
    assert eng.color_modes()[1] == 0
    eng.close()


@pytest.mark.parametrize('hw', [(24, 40), (16, 32)])
def test_style_targets_are_those_of_the_recoloured_image(hw):
    """(16, 32): the style image has the content's size and is forwarded in the context's own activation set."""
    content, style = image(1, 16, 32), co.tinted(4, *hw)
    eng = matched(content, style)
    names = eng.blob_names
    under = [eng.style_gram(n) for n in names]
    eng.set_style_nchw(eng.style_recolor(style))
    again = [eng.style_gram(n) for n in names]
    for n, a, b in zip(names, under, again):
        assert same_bits(a, b), (n, bits_off(a, b))
    eng.set_style_color_match(False)
    eng.set_style(style)
    plain = [eng.style_gram(n) for n in names]
    assert all(not np.array_equal(a, b) for a, b in zip(under, plain))
    eng.set_style_nchw(co.preprocess(style)[None])                           # the sibling entry point takes the image as it is
    assert all(same_bits(a, b) for a, b in zip(plain, [eng.style_gram(n) for n in names]))
    eng.close()


def test_colour_matching_needs_a_content_image():
    eng = Engine(TOPO, 0, 'fp32')
    eng.load_weights(NET)
    eng.set_style_color_match(True)
    with pytest.raises(StError, match=r'st2 error 2: .*no content image'):
        eng.set_style(image(2, 24, 24))
    with pytest.raises(StError, match=r'st2 error 2: .*no content image'):
        eng.style_recolor(image(2, 24, 24))
    eng.set_content(image(1, 16, 32))
    eng.set_style(image(2, 24, 24))
    kept = [eng.style_gram(n) for n in eng.blob_names]
    eng.set_content(image(5, 16, 32))                                        # a later content image leaves the targets as they are
    assert all(same_bits(a, eng.style_gram(n)) for a, n in zip(kept, eng.blob_names))
    eng.close()


# ---- 5. tile-sharded ------------------------------------------------------------------------------------------------------------------
def _tile_of(backend, nchw):
    t, w = backend.grid.tiles[backend.rank], backend.grid.windows[backend.rank]
    return nchw[0][:, t.y0 - w.y0:t.y1 - w.y0, t.x0 - w.x0:t.x1 - w.x0]


@pytest.mark.parametrize('rows,cols,h,w', [(1, 2, 32, 64), (2, 2, 64, 64)])
def test_every_ranks_tile_takes_the_chroma_of_its_own_window(rows, cols, h, w):
    content, style, init = image(1, h, w), image(2, 24, 40), image(3, h, w)
    grid = tiling.TileGrid(h, w, rows, cols, TOPO, len(TOPO))
    world = rows * cols
    fabric = tiled.InProcessFabric(world, timeout=120.0)
    backends = []
    for r in range(world):
        b = HipTileBackend(NET, grid, r, content, style, init, WEIGHTS, PARAMS, step_size=10, topology=TOPO, iterate_average=D, original_colors=True)
        b.comm_init_local(r, world, fabric)
        backends.append(b)
    ranks = [tiled.FusedTiledTransfer(grid, r, b) for r, b in enumerate(backends)]
    avgs = [AverageOracle(D) for _ in backends]
    for i in range(2):
        tiled.run_in_process(ranks, 1, fabric)
        for b, rank, avg in zip(backends, ranks, avgs):
            x, cx = _tile_of(b, b.engine.get_input_nchw()), _tile_of(b, b.engine.get_content_nchw())
            t = grid.tiles[b.rank]
            assert same_bits(cx, co.preprocess(content[t.y0:t.y1, t.x0:t.x1]))            # the window's own content crop
            want = co.emit_luma(x, cx)
            assert same_bits(b.tile_image(), want), (i, b.rank, bits_off(b.tile_image(), want))
            avg.update(x)
            want = co.emit_luma_averaged(avg, cx)
            got = b.averaged_image()
            assert same_bits(got, want), (i, b.rank, bits_off(got, want))
            assert same_bits(rank.tile_image(), got)
    with pytest.raises(StError, match=r'st2 error 2: .*st_set_style_transform'):
        backends[0].engine.set_style_color_match(True)
    assert backends[0].engine.color_modes()[1] == 0
    backends[0].engine.set_content(image(1, 16, 16))                         # a content of another size: the tile readers refuse
    with pytest.raises(StError, match=r'st2 error 2: .*16 x 16'):
        backends[0].tile_image()
    with pytest.raises(StError, match=r'st2 error 2: .*16 x 16'):
        backends[0].averaged_image()
    for b in backends:
        b.engine.close()


@pytest.mark.parametrize('shard_style', [False, True])
@pytest.mark.parametrize('grid,h,w', [((1, 2), 32, 64), ((2, 2), 64, 64)])
def test_tiled_job_hands_every_rank_the_transform_of_the_whole_images(monkeypatch, shard_style, grid, h, w):
    content, style, init = co.rgb(1, h, w), co.tinted(4, 32, 48), image(3, h, w)
    dev = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    whole = jobs.run_job(dev, content, style, 1, weights=WEIGHTS, params=PARAMS, init=init, match_style_colors=True, original_colors=True)
    oc, sm, A, b = dev.engine.color_modes()
    assert (oc, sm) == (True, 1) and not np.allclose(A, np.eye(3), atol=1e-3)
    made, seen = [], []

    class Recording(HipTileBackend):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)
    monkeypatch.setattr(tile_backend, 'HipTileBackend', Recording)
    tiles = jobs.run_tiled_job(NET, content, style, 1, grid, weights=WEIGHTS, params=PARAMS, init=init, topology=TOPO, shard_style=shard_style,
                               match_style_colors=True, original_colors=True,
                               callback=lambda i, vals: seen.append([m.engine.color_modes() for m in made]))
    assert len(made) == grid[0] * grid[1] and len(seen) == 1
    for oc_r, sm_r, a_r, b_r in seen[0]:
        assert (oc_r, sm_r) == (True, 2)
        assert same_bits(a_r, seen[0][0][2]) and same_bits(b_r, seen[0][0][3])             # the same on every rank
        assert co.ulps(a_r, A) <= 1 and co.ulps(b_r, b) <= 1
    # both jobs keep the content's chroma pixel by pixel: the colour differences of either image are the content's
    assert tiles.shape == whole.shape == (h, w, 3)
    want = content[..., 0].astype(np.float64) - content[..., 1]
    for img in (tiles, whole):
        assert float(np.abs((img[..., 0].astype(np.float64) - img[..., 1]) - want).max()) <= 8 * 2.0 ** -24 * 1024
    mse = float(np.mean((tiles.astype(np.float64) - whole) ** 2))
    print('[tiled job %dx%d, shard_style %s] image MSE %.3g against the whole-image job after one Adam iteration' % (grid + (shard_style, mse)))


# ---- 6. the worker, end to end --------------------------------------------------------------------------------------------------------
def _model():
    return st2.HipModel(NET, topology=TOPO)


def _direct(colors, n):
    ref = st2.StyleTransfer(_model())
    if colors:
        ref.engine.set_original_colors(True); ref.engine.set_style_color_match(True)
    ref.set_input(image(3, 32, 40)); ref.set_content(image(1, 32, 40)); ref.set_style(co.tinted(4, 24, 24)); ref.reset()
    ref.set_weights(WEIGHTS, PARAMS)
    ref.optimizer_cls = st2.AdamOptimizer; ref.set_step_size(10); ref.reset()
    assert ref.start()
    return [ref.step() for _ in range(n)]


def test_worker_with_both_keys_sends_the_images_of_an_engine_with_both_modes(monkeypatch):
    """Worker(config) on its own TCP sockets (pyzmq where it is installed, otherwise tests/minizmq.py) with original_colors = 1 and
    style_color_match = 1: every Iterate.image is the image of a StyleTransfer driven directly with the two modes on, for the same
    messages; the message classes on the wire are the ones a plain run sends."""
    from test_boundary import zmq_module
    zmq, which = zmq_module(monkeypatch)
    print('[transport] GPU worker ran over', which)
    ctx = zmq.Context()
    app_in = ctx.socket(zmq.PULL)
    port_app = app_in.bind_to_random_port('tcp://127.0.0.1')
    probe = ctx.socket(zmq.PULL)
    port_worker = probe.bind_to_random_port('tcp://127.0.0.1')
    probe.close(0)
    config = {'worker_socket': 'tcp://127.0.0.1:%d' % port_worker, 'app_socket': 'tcp://127.0.0.1:%d' % port_app,
              'original_colors': '1', 'style_color_match': '1'}
    wk = worker_mod.Worker(config, transfer=st2.StyleTransfer(_model()))
    assert wk.transfer.engine.color_modes()[:2] == (True, 1) and wk.pipelined
    th = threading.Thread(target=wk.run, daemon=True)
    th.start()
    app_out = ctx.socket(zmq.PUSH)
    app_out.connect(config['worker_socket'])
    for m in (messages.SetImages(None, image(3, 32, 40), image(1, 32, 40), co.tinted(4, 24, 24), True), messages.SetWeights(WEIGHTS, PARAMS),
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
    assert {type(m).__module__ + '.' + type(m).__qualname__ for m in got} == {'messages.WorkerReady', 'messages.Iterate', 'messages.Shutdown'}
    assert [m.i for m in its] == list(range(1, n + 1))
    colored, plain = _direct(True, n), _direct(False, n)
    for m, (img, tr), (raw, tr_plain) in zip(its, colored, plain):
        assert m.image.dtype == F32 and same_bits(m.image, img), 'iterate %d differs' % m.i
        assert list(m.trace) == list(tr_plain) and m.trace['fevals'] == m.i
    assert not np.array_equal(its[-1].image, plain[-1][0])
