"""NumPy float32 restatement of the engine's iterate averaging (st_set_iterate_average; test infrastructure): the reference's
``utils.DecayingMean`` (utils.py:49-69) over the iterates, with the engine's clear and resample rules.

    mean  = f32(d) * mean + f32(1.0 - d) * x        two fp32 products, one fp32 sum; the empty mean is 0;  items += 1
    image = deprocess(mean / f32(1.0 - d ** items)) power and subtraction in double, rounded once; one fp32 division; + channel mean

tests/golden/iterate_average.npz (recorded from the reference's class itself) pins the first two lines; the engine is held to this
restatement bit for bit."""

import numpy as np

from style_transfer2_amd import resample

F32 = np.float32
MEAN = np.array((123.68, 116.779, 103.939), F32)          # worker.py:34


def deprocess(x):
    """(1, 3, H, W) or (3, H, W) preprocessed -> (H, W, 3) float32 RGB: one fp32 addition per element (worker.py:68-71)."""
    x = np.asarray(x, F32)
    x = x[0] if x.ndim == 4 else x
    return np.ascontiguousarray((x + MEAN.reshape(3, 1, 1)).transpose(1, 2, 0))


class AverageOracle:
    def __init__(self, decay):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError('decay must be inside (0, 1)')
        self.decay = decay
        self.clear()

    def clear(self):
        """st_set_iterate_average, st_optimizer_reset, and whatever replaces the iterate (st_set_input*, a resample with a new image)."""
        self.mean = None
        self.items = 0

    def update(self, x):
        """After an optimizer step, with the iterate that step produced."""
        x = np.asarray(x, F32)
        prev = np.zeros_like(x) if self.mean is None else self.mean
        a = F32(self.decay) * prev                         # fp32 array times fp32 scalar: one rounding each
        b = F32(1.0 - self.decay) * x                      # (1 - d) formed in double, then rounded to fp32
        self.mean = a + b
        self.items += 1
        return self.mean

    def corr(self):
        return F32(1.0 - self.decay ** self.items)

    def corrected(self):
        if not self.items:
            raise ValueError('the mean is empty')
        return self.mean / self.corr()

    def image(self):
        return deprocess(self.corrected())

    def resample(self, size, new_x=False):
        """st_resample_state: the raw mean through Pillow's Lanczos (resample.resample_nchw, as x), items kept; a new image clears."""
        if new_x:
            self.clear()
        elif self.items:
            m = self.mean if self.mean.ndim == 4 else self.mean[None]
            self.mean = resample.resample_nchw(m, tuple(size)).reshape(self.mean.shape[:-2] + tuple(size))
