"""tests/flow_oracle.py (the optical-flow estimator of include/st2.h in NumPy float32) held to what the definition implies exactly -- a
constant pair, a pair of equal images and a 1 x 1 image give a flow of exactly 0; the level counts follow the pooling rule -- and to
synthetic pairs whose flow is known exactly.  No GPU."""
import numpy as np
import pytest

import flow_oracle as fo
import frames_oracle

F32 = np.float32
H, W = 96, 128
# (shift (dx, dy), rotation) -> measured with this oracle: interior mean end-point error, the same for a flow of zero
CASES = {
    'shift_3.3_-2.1': ((3.3, -2.1), 0.0),
    'shift_0.4_0.3': ((0.4, 0.3), 0.0),
    'shift_1_-1_rot_0.03': ((1.0, -1.0), 0.03),
}
BAR = 0.1                   # px: 4x the errors of the prototype of the definition (0.025, 0.019, 0.026), far below the zero-flow errors


@pytest.fixture(scope='module')
def base():
    return fo.texture(H, W)[0]


@pytest.fixture(scope='module')
def estimates(base):
    """name -> (backward flow, forward flow, dx, dy): estimated once, read by the tests below."""
    out = {}
    for name, (shift, rot) in CASES.items():
        moved, dx, dy = fo.texture(H, W, shift, rot)
        out[name] = (fo.estimate(moved, base), fo.estimate(base, moved), dx, dy)
    return out


def test_a_constant_pair_gives_exactly_zero():
    a = np.full((33, 47, 3), 100, np.uint8)
    b = np.full((33, 47, 3), 180, np.uint8)
    flow = fo.estimate(a, b)
    assert flow.shape == (33, 47, 2) and flow.dtype == F32
    assert not flow.any()                                  # Ix = Iy = 0 everywhere: r multiplies nothing


def test_equal_images_give_exactly_zero(base):
    noise = np.random.default_rng(3).uniform(0, 255, (40, 70, 3)).astype(F32)
    for image in (base, noise):
        assert not fo.estimate(image, image).any()         # c = Bw - A = 0 at u = v = 0, and stays


def test_a_single_pixel_gives_zero():
    flow = fo.estimate(np.full((1, 1, 3), 7, np.uint8), np.full((1, 1, 3), 200, np.uint8))
    assert flow.shape == (1, 1, 2) and not flow.any()


def test_level_counts_follow_the_pooling_rule():
    sizes = {(1, 1): 1, (1, 9): 1, (7, 1): 1, (2, 2): 1, (5, 3): 1, (16, 16): 1, (31, 33): 1, (32, 32): 2, (33, 47): 2, (64, 64): 3,
             (65, 64): 3, (63, 100): 3, (96, 128): 3, (130, 70): 3, (1024, 1024): 7, (512, 512): 6}
    for (h, w), n in sizes.items():
        assert len(fo.level_sizes(h, w)) == n, (h, w)
    assert fo.level_sizes(33, 47) == [(33, 47), (17, 24)]                      # Caffe's ceil mode
    assert fo.level_sizes(65, 64) == [(65, 64), (33, 32), (17, 16)]
    assert fo.level_sizes(5, 3, levels=12) == [(5, 3), (3, 2), (2, 1), (1, 1)]     # an explicit count stops early at 1 x 1
    assert fo.level_sizes(96, 128, levels=1) == [(96, 128)]
    assert len(fo.level_sizes(1 << 20, 1 << 20)) == 12                         # never more than 12
    assert [a.shape for a, _, _ in fo.estimate_levels(np.zeros((33, 47, 3), np.uint8), np.zeros((33, 47, 3), np.uint8))] == [(33, 47), (17, 24)]


@pytest.mark.parametrize('name', sorted(CASES))
def test_known_motion_is_recovered_to_a_tenth_of_a_pixel(estimates, name):
    """Measured with this oracle (interior mean end-point error / the same for a flow of zero):
    shift (3.3, -2.1): 0.0255 / 3.9115 px; shift (0.4, 0.3): 0.0192 / 0.5000 px; shift (1, -1) with a rotation of 0.03 rad: 0.0260 / 1.6417 px."""
    bwd, _, dx, dy = estimates[name]
    err = fo.interior_error(bwd, dx, dy)
    zero = fo.interior_error(np.zeros_like(bwd), dx, dy)
    print('%s: interior error %.4f px, zero flow %.4f px' % (name, err, zero))
    assert err <= BAR
    assert zero > 4 * BAR                                  # the case is not trivially inside the bar


@pytest.mark.parametrize('name', ['shift_3.3_-2.1', 'shift_1_-1_rot_0.03'])
def test_estimated_flow_pairs_pass_the_reliability_tests_inside_the_border(estimates, name):
    """The backward and forward estimates are consistent enough for the frames block: Ruder's map (frames_oracle.reliability) is 1 on at
    least 99 % of the pixels 12 px inside the border.  Measured: 100 % inside for both cases; over the whole image 93.8 % (shift (3.3, -2.1)) and 96.9 % (shift (1, -1) with the rotation)."""
    bwd, fwd, _, _ = estimates[name]
    c = frames_oracle.reliability(bwd, fwd)
    inside = float(c[12:-12, 12:-12].mean())
    print('%s: reliable inside %.4f, over the image %.4f' % (name, inside, float(c.mean())))
    assert inside >= 0.99
