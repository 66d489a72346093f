"""tests/jitter_oracle.py against itself and the plain oracle, on the CPU: the generator's pinned values, and the wrapped objective on a
tiny net -- with shift (0, 0) it is the plain objective; with a shift it is the plain objective of the rolled inputs, its network
gradient rolled back; TV and the p-norm are those of the unshifted iterate.  Two evaluations each: the first captures the norms.  No GPU."""
import numpy as np
import pytest

import oracle
import jitter_oracle as jo

F32 = np.float32
TOPO = oracle.tiny_topology((8, 16), (2, 2))
NET = oracle.he_init_weights(TOPO, 0, 0.1)
WEIGHTS = {'content': {'conv2_2': 0.08}, 'style': {'conv1_1': 1, 'conv2_1': 1}, 'deepdream': {'conv1_2': 0.01}}
PARAMS = {'p': 50, 'p_power': 6, 'tv': 5, 'tv_power': 2}
SHIFTS = ((1, 0), (0, -1), (-3, 2), (17, 33), (-40, 300))


def image(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def make(cls, h, w, weights=WEIGHTS):
    st = cls(oracle.NetOracle(TOPO, NET))
    st.set_input(image(3, h, w)); st.set_content(image(1, h, w)); st.set_style(image(2, 24, 24)); st.reset()
    st.set_weights(weights, PARAMS)
    st.set_optimizer('adam', 10)
    assert st.start()
    return st


def test_generator_pins():
    assert [jo.draw(1234567, k) for k in range(3)] == jo.DRAWS_1234567
    for (seed, radius), want in jo.PINS.items():
        assert [jo.shift(seed, k, radius) for k in range(len(want))] == want
    for radius in (1, 3, 16, 4096):
        for k in range(1000):
            dy, dx = jo.shift(7, k, radius)
            assert -radius <= dy <= radius and -radius <= dx <= radius


def test_roll_moves_a_pixel_down_and_right_and_unroll_undoes_it():
    p = np.arange(3 * 4 * 5, dtype=F32).reshape(1, 3, 4, 5)
    r = jo.roll(p, (1, 2))
    assert r[0, 1, 1, 2] == p[0, 1, 0, 0] and r[0, 2, 0, 0] == p[0, 2, 3, 3]
    for s in SHIFTS:
        assert np.array_equal(jo.unroll(jo.roll(p, s), s), p)
        assert np.array_equal(jo.roll(p, s), jo.roll(p, (s[0] % 4, s[1] % 5)))


def test_shift_zero_is_the_plain_objective():
    a, c = make(jo.JitterOracle, 17, 33), make(oracle.TransferOracle, 17, 33)
    x = a.input.copy()
    for _ in range(2):
        la, ga = a.opfunc(x.copy())
        lc, gc = c.opfunc(x.copy())
        assert np.isclose(la, lc, rtol=1e-6) and np.allclose(ga, gc, rtol=0, atol=1e-6 * np.abs(gc).max())
        ta, tc = a.traces[-1].data, c.traces[-1].data
        assert list(ta) == list(tc)
        assert all(np.isclose(ta[k], tc[k], rtol=1e-6, atol=1e-12) for k in tc if k != 'time')


@pytest.mark.parametrize('s', SHIFTS, ids=str)
def test_a_shifted_evaluation_is_the_plain_one_of_the_rolled_inputs_with_its_network_gradient_rolled_back(s):
    h, w = 17, 33
    a, b, c = make(jo.JitterOracle, h, w), make(oracle.TransferOracle, h, w), make(oracle.TransferOracle, h, w)
    a.jitter_shift = s
    x = a.input.copy()
    b.content = jo.roll(b.content, s)
    b.features = {k: v.copy() for k, v in b.model.forward(b.content).items()}
    for ev in range(2):                                                       # (the norms are captured by the first)
        la, ga = a.opfunc(x.copy())
        lb, gb = b.opfunc(jo.roll(x, s))
        lc, gc = c.opfunc(x.copy())
        ta, tb, tc = a.traces[-1].data, b.traces[-1].data, c.traces[-1].data
        assert list(ta) == list(tb) == list(tc)
        layer_keys = list(ta)[:list(ta).index('scd_loss') + 1] + ['scd_grad']
        assert all(ta[k] == tb[k] for k in layer_keys), ev                    # the same arithmetic on the same numbers
        assert all(ta[k] == tc[k] for k in ('t_loss', 'p_loss', 't_grad', 'p_grad')), ev
        identity = (s[0] % h, s[1] % w) == (0, 0)
        assert (ta['scd_loss'] == tc['scd_loss']) == identity                 # (any other shift matters to the network)
        # the combined gradient: the image terms are roll-equivariant up to the order of their sums
        assert np.allclose(ga, jo.unroll(gb, s), rtol=0, atol=1e-5 * np.abs(gb).max()), ev
        assert np.isclose(la, lb, rtol=1e-5), ev
    assert a.norms == b.norms and (a.norms['c']['conv2_2'] == c.norms['c']['conv2_2']) == identity


def test_without_an_active_row_nothing_is_rolled_and_without_a_gradient_the_trace_is_short():
    a = make(jo.JitterOracle, 16, 16, {'content': {}, 'style': {}, 'deepdream': {}})
    c = make(oracle.TransferOracle, 16, 16, {'content': {}, 'style': {}, 'deepdream': {}})
    a.jitter_shift = (2, 5)
    la, ga = a.opfunc(a.input.copy())
    lc, gc = c.opfunc(c.input.copy())
    assert la == lc and np.array_equal(ga, gc)
    b = make(jo.JitterOracle, 16, 16)
    b.jitter_shift = (2, 5)
    loss = b.opfunc(b.input.copy(), return_grad=False)
    assert list(b.traces[-1].data)[-4:] == ['scd_loss', 't_loss', 'p_loss', 'loss'] and np.isfinite(loss)
