"""CPU side of the colour modes (st_set_original_colors, st_set_style_color_match; csrc/color.hip, csrc/color_match.h): the NumPy
restatements the GPU tests hold the engine to (tests/color_oracle.py) against independent float64 formulations, the host-only
st_color_transform of the built library, the worker's config keys and the command-line flags.  No GPU."""

import importlib.util
import os
import sys

import numpy as np
import pytest

import color_oracle as co
from average_oracle import MEAN, AverageOracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
# Every value the emission touches here lies below 512 in magnitude (images in 0 .. 255, iterates within -128 .. 383 of image scale).
# The restatement differs from exact arithmetic with the exact coefficients 0.299, 0.587, 0.114 by: the rounding of d_c (<= 2^-25 * 512);
# the fp32 representation of the three coefficients and the rounding of the three products (each relative 2^-25, on terms whose
# magnitudes sum to at most 512 because the coefficients sum to 1: together <= 2 * 2^-25 * 512) plus the rounding of d carried through
# them (<= 2^-25 * 512); the two additions of l (<= 2 * 2^-25 * 512); cx + mean and the final addition (<= 2^-25 * 512 each): eight terms
# of 2^-25 * 512, inside the bound of 8 * 2^-24 * 512 that allows a handful of fp32 roundings on values below 512.
EMIT_TOL = 8 * 2.0 ** -24 * 512


def _iterate_and_content(seed, h=18, w=34):
    r = np.random.RandomState(seed)
    content = co.rgb(seed + 10, h, w)
    x = (r.uniform(-128, 383, (3, h, w)) - MEAN.reshape(3, 1, 1)).astype(F32)
    return x, co.preprocess(content), content


def _round_trip64(v, cx):
    """Independent of the restatement: RGB -> (Y, B - Y, R - Y) in float64 with the exact Rec.601 coefficients, the iterate's Y with the
    content's colour differences, and back through the inverse transform (G from the luma equation)."""
    kr, kg, kb = 0.299, 0.587, 0.114
    it = v.astype(np.float64) + MEAN.astype(np.float64).reshape(3, 1, 1)
    ct = cx.astype(np.float64) + MEAN.astype(np.float64).reshape(3, 1, 1)
    y_it = kr * it[0] + kg * it[1] + kb * it[2]
    y_ct = kr * ct[0] + kg * ct[1] + kb * ct[2]
    u, w = ct[2] - y_ct, ct[0] - y_ct
    red, blue = y_it + w, y_it + u
    green = (y_it - kr * red - kb * blue) / kg
    return np.stack([red, green, blue], axis=2)


def test_emission_is_the_iterates_luminance_with_the_contents_chroma():
    for seed in range(3):
        x, cx, _ = _iterate_and_content(seed)
        got = co.emit_luma(x, cx)
        assert got.dtype == F32 and got.shape == (18, 34, 3)
        err = float(np.abs(got.astype(np.float64) - _round_trip64(x, cx)).max())
        print('[emission vs float64 round trip] largest difference %.3g (bound %.3g)' % (err, EMIT_TOL))
        assert err <= EMIT_TOL
        # the chroma is the content's: the colour differences of the output are those of the content image
        want = (cx[0] + MEAN[0]).astype(np.float64) - (cx[1] + MEAN[1]).astype(np.float64)
        assert float(np.abs((got[..., 0].astype(np.float64) - got[..., 1]) - want).max()) <= EMIT_TOL
        # ... and it is not the identity: the iterate's own colours are gone
        assert float(np.abs(got - (x + MEAN.reshape(3, 1, 1)).transpose(1, 2, 0)).max()) > 1.0


def test_emission_composes_with_the_iterate_average():
    x, cx, _ = _iterate_and_content(7)
    avg = AverageOracle(0.9)
    avg.update(x[None])
    avg.update((x * F32(0.5))[None])
    got = co.emit_luma_averaged(avg, cx)
    assert np.array_equal(got, co.emit_luma(avg.corrected()[0], cx))
    assert float(np.abs(got.astype(np.float64) - _round_trip64(avg.corrected()[0], cx)).max()) <= EMIT_TOL
    # an iterate equal to the content comes back as the content image
    assert np.array_equal(co.emit_luma(cx, cx), (cx + MEAN.reshape(3, 1, 1)).transpose(1, 2, 0))


@pytest.mark.parametrize('kind', sorted(co.image_pairs()))
def test_transform_gives_the_style_the_contents_moments(kind):
    """A (S_s + eps I) A^T = S_c + eps I, i.e. A S_s A^T = S_c + eps (I - A A^T), and A mu_s + b = mu_c: exact in exact arithmetic, held
    at float64 round-off (relative 1e-9 allows for cond(S_s + eps I) up to 3e5)."""
    content, style = co.image_pairs()[kind]
    (mc, cc), (ms, cs) = co.moments(co.preprocess(content)), co.moments(co.preprocess(style))
    A, b = co.transform64(mc, cc, ms, cs)
    assert np.isfinite(A).all() and np.isfinite(b).all()
    lhs, rhs = A @ cs @ A.T, cc + co.RIDGE * (np.eye(3) - A @ A.T)
    scale = np.abs(cc).max() + co.RIDGE
    assert np.abs(lhs - rhs).max() <= 1e-9 * scale, (kind, np.abs(lhs - rhs).max())
    assert np.abs(A @ (ms - co.MEAN64) + b - (mc - co.MEAN64)).max() <= 1e-9 * 256
    assert np.linalg.cond(cs + co.RIDGE * np.eye(3)) <= 3.1e5
    # moments() against NumPy's own estimators
    p = co.preprocess(style).reshape(3, -1).astype(np.float64)
    assert np.allclose(cs, np.cov(p, bias=True), rtol=1e-10, atol=1e-9) and np.allclose(ms, p.mean(axis=1) + co.MEAN64, rtol=1e-12)
    # the recoloured style image has the content's moments (up to the ridge and the fp32 recolour)
    m2, c2 = co.moments(co.recolor(co.preprocess(style), A.astype(F32), b.astype(F32)))
    assert np.abs(m2 - mc).max() <= 1e-3 and np.abs(c2 - (cc + co.RIDGE * (np.eye(3) - A @ A.T))).max() <= 1e-3 * scale


@pytest.mark.parametrize('kind', sorted(co.image_pairs()))
def test_hand_rolled_cholesky_equals_numpys(kind):
    for img in co.image_pairs()[kind]:
        s = co.moments(co.preprocess(img))[1] + co.RIDGE * np.eye(3)
        L = co.cholesky3(s)
        assert np.allclose(L, np.linalg.cholesky(s), rtol=1e-10, atol=1e-12) and np.allclose(L @ L.T, s, rtol=1e-12)


@pytest.mark.parametrize('kind', sorted(co.image_pairs()))
def test_the_librarys_host_transform_equals_the_oracle(kind):
    """st_color_transform needs no context and no GPU: float32 of the float64 oracle to within 1 ulp."""
    import style_transfer2_amd as st2
    content, style = co.image_pairs()[kind]
    (mc, cc), (ms, cs) = co.moments(co.preprocess(content)), co.moments(co.preprocess(style))
    A, b = st2.color_transform(mc, cc, ms, cs)
    wa, wb = co.transform(mc, cc, ms, cs)
    assert A.dtype == F32 and A.shape == (3, 3) and b.shape == (3,)
    assert co.ulps(A, wa) <= 1 and co.ulps(b, wb) <= 1, (co.ulps(A, wa), co.ulps(b, wb))
    for bad in ((np.nan, 0, 0), (np.inf, 0, 0)):
        with pytest.raises(st2.StError, match='st2 error 1'):
            st2.color_transform(bad, cc, ms, cs)
    neg = cs.copy(); neg[1, 1] = -1.0
    with pytest.raises(st2.StError, match='st2 error 1: .*negative'):
        st2.color_transform(mc, cc, ms, neg)


def test_recolour_restatement_is_the_affine_map():
    s = co.preprocess(co.rgb(3, 9, 11))
    A = np.array(((0.5, 0.25, 0), (-0.125, 1, 0.5), (0, 0, 2)), F32)
    b = np.array((1, -2, 4), F32)
    got = co.recolor(s[None], A, b)
    assert got.shape == (1, 3, 9, 11) and got.dtype == F32
    want = np.einsum('ck,khw->chw', A.astype(np.float64), s.astype(np.float64)) + b.astype(np.float64).reshape(3, 1, 1)
    assert np.abs(got[0] - want).max() <= 4 * 2.0 ** -24 * 1024
    assert np.array_equal(co.recolor(s, np.eye(3, dtype=F32), np.zeros(3, F32)), s)


def _section(**keys):
    import configparser
    cp = configparser.ConfigParser()
    cp.read_dict({'worker': {k: str(v) for k, v in keys.items()}})
    return cp['worker']


def test_worker_reads_the_two_colour_keys():
    sys.path.insert(0, ROOT)
    import worker
    assert worker.read_color_keys(_section(gpu=0, iterate_average=0.9)) == {}                  # absent: no call is made
    assert worker.read_color_keys(_section(original_colors='', style_color_match=' ')) == {}
    assert worker.read_color_keys(_section(original_colors=1)) == {'original_colors': True}
    assert worker.read_color_keys({'original_colors': ' 0 ', 'style_color_match': '1'}) == {'original_colors': False, 'style_color_match': True}
    assert not set(worker.COLOR_KEYS) & set(worker.ALGO_KEYS) and worker.read_algo_keys(_section(original_colors=1)) == {}
    for key in worker.COLOR_KEYS:
        for bad in (2, -1, 'yes', 'true', '0.5', 'nan'):
            with pytest.raises(ValueError, match=key):
                worker.read_color_keys(_section(**{key: bad}))


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def set_original_colors(self, on):
        self.calls.append(('original_colors', on))

    def set_style_color_match(self, on):
        self.calls.append(('style_color_match', on))


class _FakeTransfer:
    is_running = False

    def __init__(self):
        self.engine = _FakeEngine()
        self.model = self

    def layers(self):
        return ['data']


class _Socks:
    def __init__(self):
        self.sent = []

    def send_pyobj(self, obj):
        self.sent.append(obj)


def test_worker_hands_the_colour_keys_to_the_engine_before_it_reports_ready():
    sys.path.insert(0, ROOT)
    import worker
    for extra, calls in (({}, []), ({'original_colors': '1'}, [('original_colors', True)]),
                         ({'original_colors': '0', 'style_color_match': '1'}, [('original_colors', False), ('style_color_match', True)])):
        tr, socks = _FakeTransfer(), _Socks()
        worker.Worker(dict({'async_iterate': '0'}, **extra), sock_in=socks, sock_out=socks, transfer=tr)
        assert tr.engine.calls == calls and [type(m).__name__ for m in socks.sent] == ['WorkerReady']
    tr, socks = _FakeTransfer(), _Socks()
    with pytest.raises(ValueError, match='style_color_match'):
        worker.Worker({'async_iterate': '0', 'style_color_match': 'on'}, sock_in=socks, sock_out=socks, transfer=tr)
    assert tr.engine.calls == [] and socks.sent == []


def _stylize():
    spec = importlib.util.spec_from_file_location('stylize_tool', os.path.join(ROOT, 'tools', 'stylize.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_stylize_knows_the_two_flags():
    ap = _stylize().parser()
    args = ap.parse_args(['c.jpg', 's.jpg', 'o.png'])
    assert args.original_colors is False and args.match_style_colors is False
    args = ap.parse_args(['c.jpg', 's.jpg', 'o.png', '--original-colors'])
    assert args.original_colors is True and args.match_style_colors is False
    args = ap.parse_args(['c.jpg', 's.jpg', 'o.png', '--match-style-colors', '--original-colors', '--grid', '1x2', '--shard-style'])
    assert args.original_colors and args.match_style_colors and args.grid == '1x2'
