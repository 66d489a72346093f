"""Jitter (include/st2.h: st_set_jitter) restated in NumPy.  TEST INFRASTRUCTURE.

The shift sequence in Python integers (splitmix64, masked to 64 bits), ``roll`` as ``np.roll`` over the two image axes, and a wrapper
around ``oracle.TransferOracle`` whose ``opfunc`` shows the network ``roll(x, s)`` and the content features of ``roll(content, s)``,
and un-rolls the network gradient before the image terms are added -- the definition's four lines, nothing else."""
import numpy as np

import oracle
from oracle import image_norms, objective

MASK64 = (1 << 64) - 1
PINS = {                                                   # (seed, radius): the first shifts, as include/st2.h pins them
    (7, 3): [(-1, -2), (-1, -1), (-2, 0), (-2, 3), (-3, 2), (-3, 3), (-3, 2), (2, -2)],
    (0, 16): [(5, 0), (16, 9), (-9, -10), (-6, 2), (5, 6), (9, -2)],
    (MASK64, 1024): [(-548, 1001), (-1010, 873), (-210, 611), (-662, -816)],
}
DRAWS_1234567 = [6457827717110365317, 3203168211198807973, 9817491932198370423]      # the published splitmix64 vectors


def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, k):
    return mix((seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64)


def shift(seed, k, radius):
    r = draw(seed, k)
    span = 2 * radius + 1
    return int((r >> 32) % span) - radius, int((r & 0xFFFFFFFF) % span) - radius


def roll(planes, s):
    """roll(P, (dy, dx))[..., y, x] = P[..., (y - dy) mod H, (x - dx) mod W] over the last two axes; any integers."""
    return np.roll(planes, (int(s[0]), int(s[1])), (-2, -1))


def unroll(planes, s):
    return roll(planes, (-int(s[0]), -int(s[1])))


class JitterOracle(oracle.TransferOracle):
    """TransferOracle whose network terms are evaluated under ``self.jitter_shift`` (set it per step, as the engine draws one per
    step): the loss terms, the norms and the trace are those of the shifted evaluation, TV and the p-norm those of x itself."""

    jitter_shift = (0, 0)

    def opfunc(self, x, return_grad=True):
        s = self.jitter_shift
        if not self.active_layers():                                          # no network term: nothing is rolled
            return super().opfunc(x, return_grad)
        # the shifted evaluation: x_s against F_c,s.  The image terms it computes are those of x_s -- TV is periodic and the p-norm
        # pointwise, so their VALUES are roll-invariant up to summation order; the restatement takes them from x itself below
        kept = self.features
        if any(abs(self.cells['content'][n]) > objective.EPS_W for n in self.active_layers()):
            self.features = {k: v.copy() for k, v in self.model.forward(roll(self.content, s), self.feature_layers).items()}
        tv_w, p_w = self.params['tv'], self.params['p']
        try:
            self.params = dict(self.params, tv=0, p=0)
            out = super().opfunc(roll(x, s), return_grad)
        finally:
            self.params = dict(self.params, tv=tv_w, p=p_w)
            self.features = kept
        log = self.traces.pop()
        new = objective.TraceLog()
        d = log.data
        loss = np.float32(d['scd_loss'])
        for k, v in d.items():
            if k == 't_loss':
                break
            new.put(k, v)
        tv_value, tv_grad = image_norms.tv_term(x / 255, self.params['tv_power'])
        loss += new.put('t_loss', tv_w * tv_value)
        p_value, p_grad = image_norms.p_term(x / 255, self.params['p_power'])
        loss += new.put('p_loss', p_w * p_value)
        if not return_grad:
            self.traces.append(new)
            return new.put('loss', loss)
        # d scd_loss_s / d x_s: the wrapped call's gradient with zero image weights, un-rolled
        scd = unroll(out[1], s)
        grad = new.put_rms('scd_grad', scd.copy())
        grad += new.put_rms('t_grad', tv_w * tv_grad)
        grad += new.put_rms('p_grad', p_w * p_grad)
        new.put('time', d['time'])
        self.traces.append(new)
        return new.put('loss', loss), new.put_rms('grad', grad)
