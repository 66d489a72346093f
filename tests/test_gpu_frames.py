"""Frame sequences on the real engine (``pytest -m gpu``): st_frames_keep .. st_anchor_from_frame.  The device warp is held to
jobs.warp_planar and the reliability and composition to tests/frames_oracle.py under np.array_equal -- the device computes their float64
operations in their order -- and everything built from them (loss, gradient, trace, whole frame jobs) bit for bit to the same values
handed in through st_set_anchor / st_set_input_nchw.

The tiny net of tests/test_gpu_anchor.py.  Sizes: 1 x 1 (every clamp), 5 x 7 (odd, no 16-byte path), 24 x 32 (16-byte path), 37 x 50 (more
pixels than one workgroup takes per trip), 20 x 260 (16-byte path, a row longer than a workgroup).  Flows: zero, integer, multiples of 1/8,
seeded random in +-6 px, smooth (a mix of reliable and unreliable pixels), samples outside on each side, samples exactly on the last row
and column."""
import numpy as np
import pytest

import frames_oracle as fo
import style_transfer2_amd as st2
import test_gpu_laplacian as tl
from style_transfer2_amd import capi, jobs
from style_transfer2_amd.capi import StError

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO, NET, WEIGHTS, PARAMS = tl.TOPO, tl.NET, tl.WEIGHTS, tl.PARAMS
image, make, live, same_bits, launches, size_id = tl.image, tl.make, tl.live, tl.same_bits, tl.launches, tl.size_id
SIZES = ((1, 1), (5, 7), (24, 32), (37, 50), (20, 260))
FLOWS = ('zero', 'integer', 'eighths', 'random', 'smooth', 'outside', 'edge')


def planes(seed, h, w):
    return (np.random.RandomState(seed).rand(3, h, w) * 255 - 116).astype(F32)


def the_flow(kind, h, w, seed=0):
    rng = np.random.RandomState(seed)
    yy, xx = (v.astype(F32) for v in np.mgrid[0:h, 0:w])
    f = np.zeros((h, w, 2), F32)
    if kind == 'integer':
        f[..., 0], f[..., 1] = 2, -1
    elif kind == 'eighths':
        f = (rng.randint(-24, 25, (h, w, 2)) / 8).astype(F32)
    elif kind == 'random':
        f = rng.uniform(-6, 6, (h, w, 2)).astype(F32)
    elif kind == 'smooth':
        f[..., 0] = 4 * np.sin(2 * np.pi * (xx / 150 + yy / 90 + seed / 7)) + 0.5
        f[..., 1] = 3 * np.cos(2 * np.pi * (xx / 120 - yy / 70 + seed / 5))
    elif kind == 'outside':                                 # a quarter of the image leaves it on each side
        f = rng.uniform(-1, 1, (h, w, 2)).astype(F32)
        f[:, :max(1, w // 4), 0] -= F32(w + 0.5)
        f[:, w - max(1, w // 4):, 0] += F32(w + 0.25)
        f[:max(1, h // 4), :, 1] -= F32(h + 0.75)
        f[h - max(1, h // 4):, :, 1] += F32(h + 0.5)
    elif kind == 'edge':                                    # exactly on the last column; every other row exactly on the last row
        f[..., 0] = (w - 1) - xx
        f[..., 1] = np.where(yy.astype(int) % 2 == 0, (h - 1) - yy, F32(0.25))
    return np.ascontiguousarray(f, F32)


def forward_for(bwd, seed=0):
    """A forward flow that roughly returns the backward one, with noise and a block that does not: reliable and unreliable pixels."""
    rng = np.random.RandomState(100 + seed)
    h, w = bwd.shape[:2]
    fwd = -bwd + (0.2 * rng.randn(h, w, 2)).astype(F32)
    fwd[h // 3:h // 2 + 1, w // 4:w // 2 + 1, 0] += 3
    return np.ascontiguousarray(fwd, F32)


def the_mask(h, w, seed=5):
    rng = np.random.RandomState(seed)
    return np.where(rng.rand(h, w) < 0.2, 0, rng.rand(h, w) * 2).astype(F32)


@pytest.fixture(scope='module')
def engines():
    """Two contexts per size: the one under test, and one that is handed the oracle's arrays through the existing setters."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            made[(h, w)] = (make(h, w), make(h, w))
            made[(h, w)][0].frames_keep(8)
        return made[(h, w)]
    yield get
    for pair in made.values():
        for eng in pair:
            eng.close()


def push(eng, x_chw):
    eng.set_input_nchw(x_chw[None])
    eng.frame_push()


# ---- 1. the warp ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', FLOWS)
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_the_input_from_a_frame_is_warp_planar_bit_for_bit(engines, size, kind):
    h, w = size
    eng, _ = engines(h, w)
    prev, f = planes(7, h, w), the_flow(kind, h, w)
    push(eng, prev)
    eng.set_input_nchw(planes(8, h, w)[None])                # (another iterate: the frame is the store's, not x)
    eng.set_input_from_frame(1, f)
    got = eng.get_input_nchw()[0]
    want = jobs.warp_planar(prev, f)
    assert got.dtype == F32 and np.array_equal(got, want), 'differs in %d of %d values' % ((got != want).sum(), got.size)
    if kind == 'integer':                                   # (-0.0 + 0.0: the warp of a plane is its values, not its bits)
        ys, xs = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(w) + 2, 0, w - 1)
        assert np.array_equal(got, prev[:, ys][:, :, xs])
    eng.set_input_from_frame(1)                             # no flow: a copy
    assert same_bits(eng.get_input_nchw()[0], prev)


def test_the_input_from_a_frame_leaves_the_state_st_set_input_nchw_leaves():
    h, w = 24, 32
    eng, other = make(h, w), make(h, w)
    eng.frames_keep(1)
    prev, f = planes(7, h, w), the_flow('smooth', h, w)
    for e in (eng, other):
        e.set_iterate_average(0.5)
        e.set_anchor(image(4, h, w), the_mask(h, w), 0.7)
        e.set_laplacian(tl.THREE)
        e.step(); e.step()
        assert e.iterate_average(False)[1] == 2
    push(eng, prev)
    assert eng.iterate_average(False)[1] == 0               # (push went through set_input_nchw here)
    eng.step()
    eng.set_input_from_frame(1, f)
    other.step()
    other.set_input_nchw(jobs.warp_planar(prev, f)[None])
    for e in (eng, other):
        assert e.iterate_average(False)[1] == 0             # the mean is cleared
        assert e.anchor_terms(want_extra=False)[0].shape == (1, 3, h, w)      # equal size: the terms' buffers are not called resized
        with pytest.raises(StError, match=r'st2 error [12]: '):              # the activations are those of another iterate
            e.get_blob('conv1_1')
    assert same_bits(eng.get_input_nchw(), other.get_input_nchw())
    for e in (eng, other):
        e.optimizer_reset(tl.OPT_ADAM, 10)
    for _ in range(2):
        ra, rb = eng.step(), other.step()
        assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    eng.close(); other.close()


# ---- 2. reliability, planes and what an evaluation makes of them -------------------------------------------------------------------
@pytest.mark.parametrize('with_mask', [False, True], ids=['no-mask', 'mask'])
@pytest.mark.parametrize('kind', FLOWS)
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_anchor_from_a_frame_is_the_oracles_planes_and_map_and_evaluates_like_them(engines, size, kind, with_mask):
    h, w = size
    eng, other = engines(h, w)
    prev, x, bwd, weight = planes(7, h, w), planes(9, h, w), the_flow(kind, h, w), 0.7
    fwd, mask = forward_for(bwd), the_mask(h, w) if with_mask else None
    push(eng, prev)
    for e in (eng, other):
        e.set_laplacian(None)
        e.set_input_nchw(x[None])
        e.clear_norms()
    eng.anchor_from_frame(1, bwd, fwd, mask, weight)
    assert eng.anchor() == {'size': (h, w), 'has_mask': True, 'weight': weight} and eng.trace_len() == 3 * 6 + 8 + 2
    loss, grad, trace = eng.opfunc()
    ax, m, extra = eng.anchor_terms()
    want_ax, want_m = jobs.warp_planar(prev, bwd), fo.reliability(bwd, fwd, mask)
    assert np.array_equal(ax[0], want_ax), 'planes differ in %d values' % (ax[0] != want_ax).sum()
    assert m.dtype == F32 and np.array_equal(m, want_m), 'the map differs in %d of %d pixels' % ((m != want_m).sum(), m.size)
    other.set_anchor(want_ax[None], want_m, weight)
    loss2, grad2, trace2 = other.opfunc()
    assert loss == loss2 and same_bits(grad, grad2) and np.array_equal(trace, trace2) and same_bits(extra, other.anchor_terms()[2])
    if kind == 'smooth' and h * w > 100 and not with_mask:  # (the case is not one-sided: each value of the map occurs)
        assert 0.05 < m.mean() < 0.95


def test_every_test_of_the_reliability_fires_somewhere_in_the_cases_above():
    fired = np.zeros(3, bool)
    for h, w in SIZES[2:]:
        for kind in FLOWS:
            bwd = the_flow(kind, h, w)
            o, d, b = fo.parts(bwd, forward_for(bwd))
            alone = [o & ~d & ~b, d & ~o & ~b, b & ~o & ~d]
            fired |= [a.any() for a in alone]
    assert fired.all(), fired


@pytest.mark.parametrize('size', [(5, 7), (24, 32)], ids=size_id)
def test_the_other_argument_combinations_and_one_launch_per_call(engines, size):
    h, w = size
    eng, other = engines(h, w)
    prev, x, bwd, weight = planes(7, h, w), planes(9, h, w), the_flow('smooth', h, w), -1.3
    fwd, mask = forward_for(bwd), the_mask(h, w)
    push(eng, prev)
    for e in (eng, other):
        e.set_laplacian(None)
        e.set_input_nchw(x[None])
        e.clear_norms()
    eng.profile_enable(True)
    cases = [(bwd, None, None), (bwd, None, mask), (None, None, None), (None, fwd, None), (None, fwd, mask), (None, None, np.uint8(mask > 0) * 255),
             (bwd, fwd, mask > 0)]
    for b, f, mk in cases:
        eng.profile_read()
        eng.anchor_from_frame(1, b, f, mk, weight)
        assert launches(eng) == {'frames': 1}
        has_map = f is not None or mk is not None
        assert eng.anchor() == {'size': (h, w), 'has_mask': has_map, 'weight': weight} and eng.trace_len() == 3 * 6 + 8 + 2
        with pytest.raises(StError, match=r'st2 error 2: .*no objective evaluation'):
            eng.anchor_terms()
        loss, grad, trace = eng.opfunc()
        ax, m, extra = eng.anchor_terms()
        want_ax = jobs.warp_planar(prev, b) if b is not None else prev
        mk32 = None if mk is None else (mk.astype(F32) / F32(255) if mk.dtype == np.uint8 else mk.astype(F32))
        want_m = fo.reliability(b, f, mk32) if has_map else None
        assert same_bits(ax[0], want_ax) and ((m is None and want_m is None) or same_bits(m, want_m))
        other.set_anchor(want_ax[None], want_m, weight)
        loss2, grad2, trace2 = other.opfunc()
        assert loss == loss2 and same_bits(grad, grad2) and np.array_equal(trace, trace2)
    eng.profile_read()
    eng.set_input_from_frame(1, bwd)
    assert launches(eng) == {'frames': 1}
    eng.profile_enable(False)


# ---- 3. the long-term composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(1, 1), (5, 7), (37, 50), (20, 260)], ids=size_id)
def test_accumulating_frames_1_2_and_4_is_the_composition_and_the_sum_of_the_per_frame_terms(engines, size):
    h, w = size
    eng, other = engines(h, w)
    weight, x = 2.5, planes(9, h, w)
    kept = [planes(20 + k, h, w) for k in range(4)]          # pushed oldest first: frame j is kept[4 - j]
    for p in kept:
        push(eng, p)
    assert eng.frames()['count'] >= 4
    js = (1, 2, 4)
    bwds = {j: the_flow('smooth', h, w, seed=j) for j in js}
    fwds = {j: forward_for(bwds[j], seed=j) for j in js}
    for e in (eng, other):
        e.set_laplacian(None)
        e.set_input_nchw(x[None])
        e.clear_norms()
    for j in js:
        eng.anchor_from_frame(j, bwds[j], fwds[j], None, weight, accumulate=j > 1)
    loss, grad, trace = eng.opfunc()
    ax, M, extra = eng.anchor_terms()
    a = {j: jobs.warp_planar(kept[4 - j], bwds[j]) for j in js}
    c = {j: fo.reliability(bwds[j], fwds[j]) for j in js}
    want_ax, want_M, c_long = a[1], c[1], {1: c[1]}
    for j in js[1:]:
        want_ax, want_M, c_long[j] = fo.compose(want_ax, want_M, a[j], c[j])
    assert np.array_equal(ax[0], want_ax) and np.array_equal(M, want_M)
    assert not (c_long[1] * c_long[2]).any() and not (c_long[1] * c_long[4]).any() and not (c_long[2] * c_long[4]).any()
    total, a_losses = np.zeros((1, 3, h, w), F32), []
    for j in js:                                            # one engine, the three per-frame terms in turn
        other.set_anchor(a[j][None], c_long[j], weight)
        _, _, tr = other.opfunc()
        part = other.anchor_terms()[2]
        assert not (part != 0).any() or not (total != 0)[part != 0].any()      # one term per pixel is non-zero
        total = total + part
        a_losses.append(tr[-7])
    assert np.array_equal(extra, total)
    a_loss, want_loss = trace[-7], float(np.sum(a_losses))
    print('[%dx%d] a_loss %.9g, sum of the per-frame terms %.9g; map mean %.3f' % (h, w, a_loss, want_loss, M.mean()))
    assert abs(a_loss - want_loss) <= 1e-6 * abs(want_loss)
    # a mask on the accumulated call scales what it adds, and the planes follow the pixels it adds to
    mask = the_mask(h, w)
    eng.anchor_from_frame(1, bwds[1], fwds[1], None, weight)
    eng.anchor_from_frame(2, bwds[2], fwds[2], mask, weight, accumulate=True)
    eng.opfunc(False)
    ax2, M2, _ = eng.anchor_terms(want_extra=False)
    w_ax, w_M, _ = fo.compose(a[1], c[1], a[2], fo.reliability(bwds[2], fwds[2], mask))
    assert np.array_equal(ax2[0], w_ax) and np.array_equal(M2, w_M)


# ---- 4. the store --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', [1, 2, 8])
def test_push_order_eviction_and_what_the_getter_reports(depth):
    h, w = 5, 8
    eng = make(h, w)
    before = live()
    assert eng.frames() == {'depth': 0, 'count': 0, 'size': (0, 0)}
    eng.frames_keep(depth)
    assert eng.frames() == {'depth': depth, 'count': 0, 'size': (0, 0)} and live() == before        # allocated by the pushes
    pushed = []
    for k in range(depth + 2):
        pushed.append(planes(30 + k, h, w))
        push(eng, pushed[-1])
        count = min(k + 1, depth)
        assert eng.frames() == {'depth': depth, 'count': count, 'size': (h, w)}
        assert live()[0] - before[0] == 4 * 3 * h * w * count
        for j in range(1, count + 1):
            eng.set_input_from_frame(j)
            assert same_bits(eng.get_input_nchw()[0], pushed[-j]), (k, j)
        if count < depth:
            with pytest.raises(StError, match=r'st2 error 2: .*frame %d is empty' % (count + 1)):
                eng.set_input_from_frame(count + 1)
    if depth > 1:                                           # a smaller depth drops the oldest
        eng.frames_keep(1)
        assert eng.frames() == {'depth': 1, 'count': 1, 'size': (h, w)} and live()[0] - before[0] == 4 * 3 * h * w
        eng.set_input_from_frame(1)
        assert same_bits(eng.get_input_nchw()[0], pushed[-1])
        eng.frames_keep(depth)
        assert eng.frames()['count'] == 1
    # a push at another size drops the rest
    eng.set_input(image(3, 6, 9))
    without = live()[0] - 4 * 3 * h * w * eng.frames()['count']
    eng.frame_push()
    assert live()[0] == without + 4 * 3 * 6 * 9
    assert eng.frames() == {'depth': depth, 'count': 1, 'size': (6, 9)}
    x = eng.get_input_nchw()
    eng.set_input_nchw(np.zeros_like(x))
    eng.set_input_from_frame(1, np.zeros((6, 9, 2), F32))
    assert np.array_equal(eng.get_input_nchw(), x)
    eng.frames_keep(0)
    assert live()[0] == without and eng.frames() == {'depth': 0, 'count': 0, 'size': (0, 0)}
    eng.close()


def test_live_bytes_return_after_keep_0_and_after_close():
    start = live()
    h, w = 16, 16
    eng = make(h, w)
    eng.step()
    before = live()
    eng.frames_keep(3)
    eng.frame_push(); eng.step(); eng.frame_push()
    eng.anchor_from_frame(2, the_flow('smooth', h, w), forward_for(the_flow('smooth', h, w)), the_mask(h, w), 1.5)
    eng.set_input_from_frame(1, the_flow('random', h, w))
    assert live()[0] > before[0] + 2 * 4 * 3 * h * w
    eng.set_anchor(None)
    eng.frames_keep(0)
    assert live() == before
    eng.frames_keep(2)
    eng.frame_push()
    eng.anchor_from_frame(1, the_flow('smooth', h, w), None, None, 1.5)
    eng.step()
    eng.close()
    assert live() == start


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_its_status_and_a_refused_call_changes_nothing():
    h, w = 16, 16
    eng = make(h, w)
    flow, mask = the_flow('smooth', h, w), the_mask(h, w)
    for bad in (9, -1, 100):
        with pytest.raises(StError, match=r'st2 error 1: .*depth'):
            eng.frames_keep(bad)
    with pytest.raises(StError, match=r'st2 error 2: .*no frames are kept'):
        eng.frame_push()
    with pytest.raises(StError, match=r'st2 error 1: .*frame index'):                   # depth 0: no index is valid
        eng.set_input_from_frame(1)
    eng.frames_keep(2)
    for call in (lambda j: eng.set_input_from_frame(j, flow), lambda j: eng.anchor_from_frame(j, flow, None, None, 1.0)):
        for j in (0, -1, 3):
            with pytest.raises(StError, match=r'st2 error 1: .*frame index'):
                call(j)
        with pytest.raises(StError, match=r'st2 error 2: .*frame 1 is empty'):
            call(1)
    eng.frame_push()
    with pytest.raises(StError, match=r'st2 error 2: .*frame 2 is empty: 1 frame\(s\) of 16 x 16 kept, the input is 16 x 16'):
        eng.anchor_from_frame(2, flow, None, None, 1.0)
    x0 = eng.get_input_nchw()
    for bad in (float('nan'), float('inf'), -float('inf')):
        ff = flow.copy(); ff[h - 1, w - 1, 1] = bad
        with pytest.raises(StError, match=r'st2 error 1: .*flow'):
            eng.set_input_from_frame(1, ff)
        with pytest.raises(StError, match=r'st2 error 1: .*flow'):
            eng.anchor_from_frame(1, ff, None, None, 1.0)
        with pytest.raises(StError, match=r'st2 error 1: .*flow'):
            eng.anchor_from_frame(1, flow, ff, None, 1.0)
    for bad in (-1e-30, float('nan'), float('inf')):
        mm = mask.copy(); mm[3, 4] = bad
        with pytest.raises(StError, match=r'st2 error 1: .*map'):
            eng.anchor_from_frame(1, flow, None, mm, 1.0)
    for bad in (0.0, float('nan'), float('inf'), 1e-60, 1e60):
        with pytest.raises(StError, match=r'st2 error 1: .*weight'):
            eng.anchor_from_frame(1, flow, None, mask, bad)
    for bad in (flow[:-1], flow[..., :1], np.zeros((h, w), F32)):
        with pytest.raises(ValueError):
            eng.set_input_from_frame(1, bad)
        with pytest.raises(ValueError):
            eng.anchor_from_frame(1, flow, bad)
    with pytest.raises(ValueError):
        eng.anchor_from_frame(1, flow, None, mask[:, :-1])
    assert eng.anchor() is None and same_bits(eng.get_input_nchw(), x0)
    # accumulating: the term off, on without a map, another weight
    with pytest.raises(StError, match=r'st2 error 2: .*the term is off'):
        eng.anchor_from_frame(1, flow, -flow, None, 1.5, accumulate=True)
    eng.anchor_from_frame(1, flow, None, None, 1.5)
    with pytest.raises(StError, match=r'st2 error 2: .*no map'):
        eng.anchor_from_frame(1, flow, -flow, None, 1.5, accumulate=True)
    eng.anchor_from_frame(1, flow, -flow, None, 1.5)
    with pytest.raises(StError, match=r'st2 error 1: .*weight in force'):
        eng.anchor_from_frame(1, flow, -flow, None, 2.5, accumulate=True)
    eng.opfunc()
    kept = eng.anchor_terms()
    with pytest.raises(StError, match=r'st2 error 1: .*flow'):                          # a refused call changes nothing
        eng.anchor_from_frame(1, flow * np.float32('nan'), None, None, 9.0)
    assert eng.anchor() == {'size': (h, w), 'has_mask': True, 'weight': 1.5}
    assert all(same_bits(a, b) for a, b in zip(eng.anchor_terms(), kept))
    # kept frames of another size than the input's: both sizes are named
    eng.set_input(image(3, 17, 33)); eng.set_content(image(1, 17, 33))
    big = np.zeros((17, 33, 2), F32)
    with pytest.raises(StError, match=r'st2 error 2: .*frames are 16 x 16, the input 17 x 33'):
        eng.set_input_from_frame(1, big)
    with pytest.raises(StError, match=r'st2 error 2: .*frames are 16 x 16, the input 17 x 33'):
        eng.anchor_from_frame(1, big, None, None, 1.5)
    eng.frame_push()                                        # (a push at the new size: the 16 x 16 frame goes)
    with pytest.raises(StError, match=r'st2 error 2: .*anchor is 16 x 16, the input 17 x 33'):
        eng.anchor_from_frame(1, big, -big, None, 1.5, accumulate=True)
    assert eng.frames() == {'depth': 2, 'count': 1, 'size': (17, 33)}
    eng.anchor_from_frame(1, big, -big, None, 1.5)
    # a pipelined iteration in flight
    eng.step_begin()
    for call in (lambda: eng.frames_keep(3), lambda: eng.frames_keep(0), eng.frame_push, lambda: eng.set_input_from_frame(1, big),
                 lambda: eng.anchor_from_frame(1, big, None, None, 1.5), lambda: eng.anchor_from_frame(1, big, -big, None, 1.5, accumulate=True)):
        with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
            call()
    eng.step_end()
    assert eng.frames() == {'depth': 2, 'count': 1, 'size': (17, 33)}
    # a tile-configured context
    eng.set_anchor(None)
    capi.check(eng.lib.st_tile_configure(eng._ctx, 17, 33, 0, 0, 0, 0, 17, 33))
    for call in (lambda: eng.frames_keep(3), eng.frame_push, lambda: eng.set_input_from_frame(1, big), lambda: eng.anchor_from_frame(1, big, None, None, 1.5)):
        with pytest.raises(StError, match=r'st2 error 2: .*tile-configured'):
            call()
    assert eng.anchor() is None
    eng.frames_keep(0)                                      # (off stays allowed)
    assert eng.frames() == {'depth': 0, 'count': 0, 'size': (0, 0)}
    eng.close()


# ---- 6. jobs -------------------------------------------------------------------------------------------------------------------------
def by_hand_setup(b, frame, style):
    b.set_content(frame); b.set_style(style); b.reset()
    b.set_weights(WEIGHTS, PARAMS)
    b.optimizer_cls = st2.AdamOptimizer; b.set_step_size(10); b.reset()


def test_run_frames_with_fractional_flows_is_the_host_seam_made_by_hand_and_reads_no_iterate_back():
    h, w, iters, weight = 24, 32, 4, 40.0
    frames = [image(10 + t, h, w) for t in range(3)]
    style = image(2, 24, 24)
    flows = [None, the_flow('smooth', h, w, 1), the_flow('eighths', h, w, 2)]
    masks = [None, the_mask(h, w, 5), the_mask(h, w, 6)]
    kw = dict(optimizer='adam', weights=WEIGHTS, params=PARAMS)

    a = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    reads, read = [], a.engine.get_input_nchw
    a.engine.get_input_nchw = lambda: reads.append(1) or read()
    got = jobs.run_frames(a, frames, style, iters, weight, flows=flows, masks=masks, **kw)
    assert reads == []                                      # the seam runs on the device
    assert a.engine.anchor() == {'size': (h, w), 'has_mask': True, 'weight': weight} and a.engine.frames() == {'depth': 1, 'count': 1, 'size': (h, w)}

    b = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    by_hand = [jobs.run_job(b, frames[0], style, iters, anchor=False, **kw)]
    for t in (1, 2):
        prev = b.engine.get_input_nchw()[0]
        shifted = jobs.warp_planar(prev, flows[t])
        assert not same_bits(shifted, prev)
        b.set_input(np.zeros((h, w, 3), np.uint8)); b.engine.set_input_nchw(shifted[None])
        by_hand_setup(b, frames[t], style)
        b.set_anchor(shifted[None], masks[t], weight)
        assert b.start()
        for _ in range(iters):
            out, _ = b.step()
        by_hand.append(out)
    for t in range(3):
        assert got[t].dtype == F32 and got[t].shape == (h, w, 3) and same_bits(got[t], by_hand[t]), 'frame %d differs' % t
    assert not same_bits(got[1], got[2])
    a.engine.close(); b.engine.close()


def test_run_frames_with_forward_flows_and_a_long_term_frame_is_the_device_calls_made_by_hand():
    h, w, iters, weight = 24, 32, 3, 40.0
    n = 4
    frames = [image(10 + t, h, w) for t in range(n)]
    style = image(2, 24, 24)
    flows = [None] + [the_flow('smooth', h, w, t) for t in range(1, n)]
    fwds = [None] + [forward_for(flows[t], t) for t in range(1, n)]
    masks = [None, None, the_mask(h, w, 6), None]
    back2 = [None, None] + [the_flow('smooth', h, w, 10 + t) for t in range(2, n)]
    fwd2 = [None, None, forward_for(back2[2], 12), None]
    kw = dict(optimizer='adam', weights=WEIGHTS, params=PARAMS)

    a = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    seen = []
    got = jobs.run_frames(a, frames, style, iters, weight, flows=flows, masks=masks, forward_flows=fwds, long_term={2: (back2, fwd2)},
                          callback=lambda i, img, tr: seen.append(tr), **kw)
    assert a.engine.frames() == {'depth': 2, 'count': 2, 'size': (h, w)}
    assert all('a_loss' not in tr for tr in seen[:iters]) and all('a_loss' in tr for tr in seen[iters:])

    b = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    b.engine.frames_keep(2)
    by_hand = [jobs.run_job(b, frames[0], style, iters, anchor=False, **kw)]
    b.engine.frame_push()
    for t in range(1, n):
        b.set_input(np.zeros((h, w, 3), np.uint8)); b.engine.set_input_from_frame(1, flows[t])
        by_hand_setup(b, frames[t], style)
        b.anchor_from_frame(1, flows[t], fwds[t], masks[t], weight)
        if t >= 2:
            b.anchor_from_frame(2, back2[t], fwd2[t], None, weight, accumulate=True)
        assert b.start()
        for _ in range(iters):
            out, _ = b.step()
        by_hand.append(out)
        b.engine.frame_push()
    for t in range(n):
        assert same_bits(got[t], by_hand[t]), 'frame %d differs' % t
    # the last anchor is the oracle's composition of the two stylised frames before it
    ax, M, _ = a.engine.anchor_terms(want_extra=False)
    assert same_bits(ax, b.engine.anchor_terms(want_extra=False)[0])
    c1, c2 = fo.reliability(flows[3], fwds[3]), fo.reliability(back2[3], None)
    assert np.array_equal(M, np.maximum(c1, c2)) and 0 < c1.mean() < 1
    a.engine.close(); b.engine.close()
