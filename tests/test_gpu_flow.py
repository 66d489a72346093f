"""Optical flow on the real engine (``pytest -m gpu``): st_flow_estimate .. st_get_flow_level.  The device's flow, and every level of
it, is held to tests/flow_oracle.py under np.array_equal -- the device computes the oracle's float32 operations in their order -- the
single-workgroup Jacobi route to the per-iteration one, and the call is shown to leave everything else of a context alone.

Sizes: the thin and odd ones (every clamp, clipped pool windows, widths that are no multiple of 4), one, two and three levels, and both
sides of the single-workgroup bound of 4096 pixels: 64 x 64 and 32 x 128 are on it, 65 x 64 and 41 x 100 just above."""
import os
from ctypes import byref, c_void_p

import numpy as np
import pytest

import flow_oracle as fo
import style_transfer2_amd as st2
import test_gpu_laplacian as tl
from style_transfer2_amd import capi, flow, jobs
from style_transfer2_amd.capi import StError
from style_transfer2_amd.engine import OPT_ADAM, OPT_LBFGS

pytestmark = pytest.mark.gpu
F32 = np.float32
TOPO, NET, WEIGHTS, PARAMS = tl.TOPO, tl.NET, tl.WEIGHTS, tl.PARAMS
image, make, live, same_bits, launches, size_id = tl.image, tl.make, tl.live, tl.same_bits, tl.launches, tl.size_id
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((1, 1), (1, 9), (7, 1), (2, 2), (5, 3), (16, 16), (31, 33), (32, 32), (33, 47), (64, 64), (65, 64), (63, 100), (96, 128), (130, 70),
         (32, 128), (41, 100))
INPUT_SIZES = ((5, 3), (33, 47), (65, 64))
PARAM_SIZES = ((33, 47), (64, 64), (63, 100))
INPUTS = ('noise_u8', 'noise_f32', 'constant', 'clamping_shift')
PARAM_SETS = (dict(warps=1), dict(iters=1), dict(iters=2), dict(levels=1), dict(alpha=0.03), dict(alpha=0.12))
WG_PIXELS = 4096


def pair(kind, h, w):
    """(from, to) HxWx3 images."""
    rng = np.random.RandomState(h * 1000 + w)
    if kind == 'texture':
        return fo.texture(h, w, (1.7, -1.2))[0], fo.texture(h, w)[0]
    if kind == 'noise_u8':
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8), rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 'noise_f32':
        return rng.uniform(0, 255, (h, w, 3)).astype(F32), rng.uniform(0, 255, (h, w, 3)).astype(F32)
    if kind == 'constant':
        return np.full((h, w, 3), 90, np.uint8), np.full((h, w, 3), 200, np.uint8)
    if kind == 'clamping_shift':                            # nearly half the image: the samples of every level run into the border
        return fo.texture(h, w, (0.45 * w, -0.45 * h))[0], fo.texture(h, w)[0]
    raise ValueError(kind)


@pytest.fixture(scope='module')
def eng():
    e = make(16, 16)
    yield e
    e.close()


def held_to_the_oracle(eng, a, b, **params):
    """Both routes against the oracle, level by level from the coarsest; returns the flow."""
    want = fo.estimate_levels(a, b, **params)
    h, w = a.shape[:2]
    sizes = flow.level_sizes(h, w, params.get('levels', 0))
    assert [lv[0].shape for lv in want] == sizes
    flows = {}
    for route in (0, 1):
        got = eng.flow_estimate(a, b, route=route, **params)
        assert got.shape == (h, w, 2) and got.dtype == F32
        for l in range(len(sizes) - 1, -1, -1):
            A, B, f = eng.flow_level(l)
            assert np.array_equal(A, want[l][0]), 'route %d, level %d: the smoothed `from` plane differs in %d values' % (route, l, (A != want[l][0]).sum())
            assert np.array_equal(B, want[l][1]), 'route %d, level %d: the smoothed `to` plane differs in %d values' % (route, l, (B != want[l][1]).sum())
            assert np.array_equal(f, want[l][2]), 'route %d, level %d: the flow differs in %d of %d values' % (route, l, (f != want[l][2]).sum(), f.size)
        assert np.array_equal(got, want[0][2])
        with pytest.raises(StError, match=r'st2 error 1: .*no such level'):
            eng.flow_level(len(sizes))
        flows[route] = got
    assert same_bits(flows[0], flows[1])
    return flows[0]


# ---- 1. bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', SIZES, ids=size_id)
def test_the_flow_of_a_shifted_texture_is_the_oracles_at_every_level_on_both_routes(eng, size):
    h, w = size
    a, b = pair('texture', h, w)
    f = held_to_the_oracle(eng, a, b)
    if min(h, w) >= 16:
        assert np.abs(f).max() > 0.5                        # (a flow is found: the comparison is not one of zeros)


@pytest.mark.parametrize('kind', INPUTS)
@pytest.mark.parametrize('size', INPUT_SIZES, ids=size_id)
def test_other_inputs_are_the_oracles(eng, size, kind):
    a, b = pair(kind, *size)
    f = held_to_the_oracle(eng, a, b)
    if kind == 'constant':
        assert not f.any()
    if kind == 'clamping_shift' and size != (5, 3):        # the case does clamp: some sample point of the result lies outside the image
        h, w = size
        yy, xx = np.mgrid[0:h, 0:w]
        assert ((xx + f[..., 0] > w - 1) | (yy + f[..., 1] < 0)).any()


@pytest.mark.parametrize('params', PARAM_SETS, ids=lambda p: '%s=%s' % next(iter(p.items())))
@pytest.mark.parametrize('size', PARAM_SIZES, ids=size_id)
def test_other_parameters_are_the_oracles(eng, size, params):
    a, b = pair('texture', *size)
    f = held_to_the_oracle(eng, a, b, **params)
    assert not same_bits(f, eng.flow_estimate(a, b))        # (the parameter changes the result)


def test_mixed_and_float_images_take_the_float_upload_and_equal_images_give_zero(eng):
    a, b = pair('noise_u8', 33, 47)
    want = eng.flow_estimate(a, b)
    assert same_bits(eng.flow_estimate(a.astype(F32), b), want) and same_bits(eng.flow_estimate(a.astype(np.float64), b.astype(F32)), want)
    assert not eng.flow_estimate(a, a).any()
    with pytest.raises(ValueError):
        eng.flow_estimate(a, b[:-1])
    with pytest.raises(ValueError):
        eng.flow_estimate(a[..., 0], b[..., 0])


def test_the_routes_launch_what_the_plan_says(eng):
    a, b = pair('texture', 96, 128)                          # levels of 12288, 3072 and 768 pixels: one above the bound, two below
    eng.profile_enable(True)
    try:
        eng.profile_read()
        eng.flow_estimate(a, b)
        got = launches(eng)
        assert got == {'flow_prepare': 1 + 2 + 3 + 3 + 1, 'flow_linearise': 9, 'flow_jacobi': 3 * 40, 'flow_jacobi_one_workgroup': 2 * 3}
        eng.flow_estimate(a, b, route=1)
        got = launches(eng)
        assert got == {'flow_prepare': 10, 'flow_linearise': 9, 'flow_jacobi': 3 * 3 * 40}
        eng.flow_estimate(*pair('texture', 64, 64), iters=7)
        assert launches(eng) == {'flow_prepare': 10, 'flow_linearise': 9, 'flow_jacobi_one_workgroup': 9}
    finally:
        eng.profile_enable(False)


# ---- 2. state --------------------------------------------------------------------------------------------------------------------------
def everything(e):
    """What an estimate must leave alone, as a list of (name, value)."""
    out = [('x', e.get_input_nchw()), ('frames', e.frames()), ('anchor', e.anchor())]
    out += [('anchor_terms %d' % i, v) for i, v in enumerate(e.anchor_terms())]
    for name in ('conv1_1', 'conv2_1', 'conv2_2'):
        for want in ('D', 'raw_S', 'diff', 'norms'):
            try:
                out.append(('%s %s' % (name, want), e.layer_terms(name, (want,))[want]))
            except StError as err:
                out.append(('%s %s' % (name, want), str(err)))
    return out


def alike(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and same_bits(a, b)
    return a == b


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
@pytest.mark.parametrize('kind', [OPT_ADAM, OPT_LBFGS], ids=['adam', 'lbfgs'])
def test_an_estimate_between_two_steps_leaves_the_job_bit_for_bit(kind, precision):
    h, w = 24, 32
    with_flow, without = make(h, w, kind=kind, precision=precision), make(h, w, kind=kind, precision=precision)
    for e in (with_flow, without):
        e.frames_keep(2)
        e.frame_push()
        e.set_anchor(image(4, h, w), None, 0.7)
    first = [e.step() for e in (with_flow, without)]
    f = with_flow.flow_estimate(*pair('texture', 33, 47))   # (another size than the job's)
    assert f.any()
    for (na, va), (nb, vb) in zip(everything(with_flow), everything(without)):
        assert na == nb and alike(va, vb), na
    with_flow.flow_estimate(image(5, h, w), image(6, h, w), iters=3)
    second = [e.step() for e in (with_flow, without)]
    for ra, rb in (first, second):
        assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    for (na, va), (nb, vb) in zip(everything(with_flow), everything(without)):
        assert na == nb and alike(va, vb), na
    for e in (with_flow, without):
        e.close()


def test_live_bytes_return_after_release_and_after_close():
    start = live()
    e = make(16, 16)
    e.step()
    before = live()
    a, b = pair('noise_u8', 33, 47)
    want = e.flow_estimate(a, b)
    grown = live()
    assert grown[0] > before[0] + 4 * 6 * 33 * 47 and grown[1] == before[1]
    e.flow_estimate(*pair('noise_u8', 5, 3))                # a smaller request keeps the buffer
    assert live() == grown
    e.flow_release()
    assert live() == before
    with pytest.raises(StError, match=r'st2 error 2: .*no estimate'):
        e.flow_level(0)
    e.flow_release()                                        # (twice is fine)
    assert same_bits(e.flow_estimate(a, b), want) and live() == grown
    e.close()
    assert live() == start


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_its_status_and_a_refused_call_enqueues_nothing():
    h, w = 16, 16
    e, undisturbed = make(h, w), make(h, w)
    with pytest.raises(StError, match=r'st2 error 2: .*no estimate'):     # before any estimate
        e.flow_level(0)
    a8, b8 = pair('noise_u8', h, w)
    af, bf = pair('noise_f32', h, w)
    out = np.zeros((h, w, 2), F32)
    ptr = lambda v: v.ctypes.data_as(c_void_p) if v is not None else None      # noqa: E731

    def raw(a, b, H=h, W=w, is_u8=1, o=out, use_defaults=False, **par):
        p = flow.DEFAULTS.copy()
        p.update(par)
        cpar = capi.FlowParams(p['levels'], p['warps'], p['iters'], p['alpha'], p['route'])
        capi.check(e.lib.st_flow_estimate(e._ctx, ptr(a), ptr(b), H, W, is_u8, None if use_defaults else byref(cpar), ptr(o)))

    arg = r'st2 error 1: .+'
    for kwargs, text in ((dict(a=None, b=b8), 'required'), (dict(a=a8, b=None), 'required'), (dict(a=a8, b=b8, o=None), 'required'),
                         (dict(a=a8, b=b8, H=0), 'at least 1 x 1'), (dict(a=a8, b=b8, W=0), 'at least 1 x 1'), (dict(a=a8, b=b8, H=-3), 'at least 1 x 1'),
                         (dict(a=a8, b=b8, levels=-1), 'levels'), (dict(a=a8, b=b8, levels=13), 'levels'),
                         (dict(a=a8, b=b8, warps=0), 'warps'), (dict(a=a8, b=b8, warps=17), 'warps'),
                         (dict(a=a8, b=b8, iters=0), 'iters'), (dict(a=a8, b=b8, iters=1001), 'iters'),
                         (dict(a=a8, b=b8, alpha=float('nan')), 'alpha'), (dict(a=a8, b=b8, alpha=float('inf')), 'alpha'),
                         (dict(a=a8, b=b8, alpha=0.9e-6), 'alpha'), (dict(a=a8, b=b8, alpha=1000.5), 'alpha'), (dict(a=a8, b=b8, alpha=-0.06), 'alpha'),
                         (dict(a=a8, b=b8, route=2), 'route'), (dict(a=a8, b=b8, route=-1), 'route')):
        with pytest.raises(StError, match=r'st2 error 1: .*' + text):
            raw(**kwargs)
    for bad in (float('nan'), float('inf'), -float('inf')):
        for which in (0, 1):
            imgs = [af.copy(), bf.copy()]
            imgs[which][h - 1, w - 1, 2] = bad
            with pytest.raises(StError, match=r'st2 error 1: .*finite'):
                raw(imgs[0], imgs[1], is_u8=0)
    with pytest.raises(StError, match=arg):
        capi.check(e.lib.st_flow_estimate(None, ptr(a8), ptr(b8), h, w, 1, None, ptr(out)))
    assert not out.any()                                    # nothing was written
    with pytest.raises(ValueError):                         # the Python side refuses the same before the library is asked
        e.flow_estimate(a8, b8, iters=0)
    with pytest.raises(StError, match=r'st2 error 2: .*no estimate'):     # ... and none of those calls left an estimate
        e.flow_level(0)
    # a pipelined iteration in flight
    e.step_begin(); undisturbed.step_begin()
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        raw(a8, b8)
    with pytest.raises(StError, match=r'st2 error 2: .*in flight'):
        e.flow_estimate(a8, b8)
    ra, rb = e.step_end(), undisturbed.step_end()
    assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    # nothing was enqueued by any of them: the next step is the undisturbed context's
    ra, rb = e.step(), undisturbed.step()
    assert same_bits(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
    # NULL parameters are the defaults; a tile-configured context may estimate
    raw(a8, b8, use_defaults=True)
    want = fo.estimate(a8, b8)
    assert np.array_equal(out, want)
    capi.check(e.lib.st_tile_configure(e._ctx, h, w, 0, 0, 0, 0, h, w))
    assert np.array_equal(e.flow_estimate(a8, b8), want)
    e.close(); undisturbed.close()


# ---- 4. jobs ---------------------------------------------------------------------------------------------------------------------------
def moving_frames(n, h, w):
    return [np.uint8(np.clip(fo.texture(h, w, (1.5 * t, -0.8 * t), 0.01 * t)[0], 0, 255)) for t in range(n)]


def test_run_frames_estimating_is_run_frames_given_the_estimates():
    h, w, iters, weight = 32, 48, 3, 40.0
    frames, style = moving_frames(3, h, w), image(2, 24, 24)
    kw = dict(optimizer='adam', weights=WEIGHTS, params=PARAMS)
    a = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    got = jobs.run_frames(a, frames, style, iters, weight, long_term={2: None}, estimate={}, **kw)
    b = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))
    flows, fwd, lt = jobs.estimate_flows(b.engine, frames, long_term=(2,))
    assert flows[0] is None and fwd[0] is None and sorted(lt) == [2] and lt[2][0][:2] == [None, None] and lt[2][1][:2] == [None, None]
    assert np.array_equal(flows[1], fo.estimate(frames[1], frames[0])) and np.array_equal(fwd[2], fo.estimate(frames[1], frames[2]))
    assert np.array_equal(lt[2][0][2], fo.estimate(frames[2], frames[0])) and np.abs(flows[1]).max() > 0.5
    want = jobs.run_frames(b, frames, style, iters, weight, flows=flows, forward_flows=fwd, long_term=lt, **kw)
    assert len(got) == len(want) == 3
    for t in range(3):
        assert got[t].dtype == want[t].dtype and np.array_equal(got[t], want[t]), t
    plain = st2.StyleTransfer(st2.HipModel(NET, topology=TOPO))      # (the flows matter: without them the frames after the first differ)
    unwarped = jobs.run_frames(plain, frames, style, iters, weight, **kw)
    assert np.array_equal(unwarped[0], got[0]) and not np.array_equal(unwarped[1], got[1])
    for t in (a, b, plain):
        t.engine.close()


def test_the_frames_tool_saves_flows_that_reproduce_its_run(tmp_path):
    from PIL import Image
    import importlib.util
    spec = importlib.util.spec_from_file_location('stylize_frames_tool', os.path.join(ROOT, 'tools', 'stylize_frames.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    h, w = 32, 48
    names = []
    for t, frame in enumerate(moving_frames(3, h, w)):
        names.append(str(tmp_path / ('f%d.png' % t)))
        Image.fromarray(frame).save(names[-1])
    Image.fromarray(image(2, 24, 24)).save(str(tmp_path / 's.png'))
    base = names + ['--style', str(tmp_path / 's.png'), '--size', '48', '--style-size', '24', '--iters', '3', '--long-term', '2']
    saved = str(tmp_path / 'flows')
    tool.main(base + ['--out-dir', str(tmp_path / 'a'), '--estimate-flow', '--save-flows', saved])
    assert sorted(os.listdir(saved)) == ['f1.fwd.npy', 'f1.npy', 'f2.b2.npy', 'f2.f2.npy', 'f2.fwd.npy', 'f2.npy']
    loaded = [np.uint8(jobs.load_rgb(n)) for n in names]
    assert np.array_equal(np.load(os.path.join(saved, 'f2.npy')), fo.estimate(loaded[2], loaded[1]))
    assert np.array_equal(np.load(os.path.join(saved, 'f2.f2.npy')), fo.estimate(loaded[0], loaded[2]))
    tool.main(base + ['--out-dir', str(tmp_path / 'b'), '--flows', saved, '--forward-flows', saved])
    for t in range(3):
        got, want = (np.asarray(Image.open(str(tmp_path / d / ('f%d.png' % t)))) for d in ('b', 'a'))
        assert got.shape == (h, w, 3) and np.array_equal(got, want), t
