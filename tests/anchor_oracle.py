"""The anchor term of include/st2.h (st_set_anchor) restated in NumPy float64, with per-element error bars that are derived, not measured,
and a float32 emulation of the documented operation order (with seeded defects) that shows the bars can be met and that they bite.

Definition.  u = x / 255, ua = ax / 255, planar (3, H, W); m an (H, W) map of values >= 0 shared by the channels (None: 1 everywhere);
w a non-zero weight.
  d = u - ua;  loss = w * sum m d^2;  g_anc = w * (2 * (m * d))
The device computes e = m * d (e = d without a map), sums (double)e * (double)d, and forms g_anc = w * (2 * e) with w as a float.

The bars.  eps = 2^-24 is the unit roundoff of float32 (round to nearest: every operation's result is within eps relative of the exact
one); x, ax, m and w are taken as exact.
  d.  u' = fl(x / 255) is within eps |u| of u, ua' within eps |ua| of ua; the subtraction adds eps |u' - ua'| <= eps (|u| + |ua|) to
      first order.  Together |d' - d| <= B_d = 2 eps (|u| + |ua|).
  g_anc.  e' = fl(m d') differs from m d by at most m B_d + eps m (|d| + B_d).  The factor 2 is exact.  The conversion of w to
      float32 and the multiplication by it are one eps each of 2 |w| m (|d| + B_d).  That is three eps; the bar takes four, which also
      covers the second-order terms:  B_g = 2 |w| m (B_d + 4 eps (|d| + B_d)).  Where m = 0 the bar is 0 and so is g_anc, exactly.
  loss.  The products e' d' are formed and summed in double (exact to 2^-53).  e' d' differs from m d^2 by at most
      m (2 |d| B_d + B_d^2), plus eps m (|d| + B_d)^2 for the rounding of e' (one).  Each workgroup's partial is rounded to float32 and
      combined by nine float32 additions (ten eps), the total is converted to float32 (one), w is converted and multiplied (two): fourteen
      eps of sum m (|d| + B_d)^2, the bar takes fifteen:
      loss_bar = |w| [sum m (2 |d| B_d + B_d^2) + 15 eps sum m (|d| + B_d)^2].
  a_grad = sqrt(float(sum g^2 / N)): as l_grad of tests/laplacian_oracle.py -- the sum of squares moves by at most
      dG = sum (2 |g| B_g + B_g^2) + 10 eps sum (|g| + B_g)^2, so the value lies in [sqrt(max(G - dG, 0) / N), sqrt((G + dG) / N)], plus
      three eps for the conversion, the division and sqrtf.
"""
import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
SIZES = ((16, 16), (17, 33), (37, 50), (20, 260), (64, 64))
WEIGHTS = (0.7, -1.3, 250.0)


def loss_and_grad_u(u, ua, m, w):
    """float64: (loss, dloss/du) of the definition, on u and ua directly (the finite-difference check differentiates this)."""
    d = u - ua
    mm = np.ones(u.shape[1:]) if m is None else np.asarray(m, np.float64)
    return w * np.sum(mm * d * d), w * 2.0 * mm * d


def evaluate(x, ax, m, w):
    """The oracle: x, ax planar (3, H, W) and m (H, W) or None (any float dtype; taken as exact), w the weight.  Returns a dict with
    the loss and its bar, g (g_anc) with its per-element bar, a_grad with its bar."""
    x, ax = np.asarray(x, np.float64), np.asarray(ax, np.float64)
    mm = np.ones(x.shape[1:]) if m is None else np.asarray(m, np.float64)
    if not np.isfinite(w) or w == 0 or not np.isfinite(mm).all() or (mm < 0).any():
        raise ValueError('weight: finite and non-zero; map: finite and >= 0')
    u, ua = x / 255.0, ax / 255.0
    loss, g = loss_and_grad_u(u, ua, mm, w)
    d = np.abs(u - ua)
    B_d = 2 * EPS * (np.abs(u) + np.abs(ua))
    B_g = 2 * abs(w) * mm * (B_d + 4 * EPS * (d + B_d))
    loss_bar = abs(w) * (np.sum(mm * (2 * d * B_d + B_d * B_d)) + 15 * EPS * np.sum(mm * (d + B_d) ** 2))
    N = g.size
    G = np.sum(g * g)
    dG = np.sum(2 * np.abs(g) * B_g + B_g * B_g) + 10 * EPS * np.sum((np.abs(g) + B_g) ** 2)
    a_grad = np.sqrt(G / N)
    hi, lo = np.sqrt((G + dG) / N), np.sqrt(max(G - dG, 0.0) / N)
    return {'loss': loss, 'loss_bar': loss_bar, 'g': g, 'g_bar': B_g, 'a_grad': a_grad,
            'a_grad_bar': max(hi - a_grad, a_grad - lo) + 3 * EPS * hi}


# ------------------------------------------------------------------------------------------------------------------- float32 emulation
DEFECTS = ('map_shifted', 'map_transposed', 'map_per_channel', 'no2', 'm2_loss')


def emulate32(x, ax, m, w, defect=None):
    """What the device is documented to compute, in NumPy float32 (defect: one of DEFECTS seeds a bug; all but 'no2' need a map).
    Returns the loss (float32 from double sums), g (g_anc) and a_grad."""
    assert defect is None or defect in DEFECTS
    x, ax = np.asarray(x, F32), np.asarray(ax, F32)
    u, ua = x / F32(255), ax / F32(255)
    d = u - ua
    if m is None:
        e = e_loss = d
    else:
        m = np.asarray(m, F32)
        if defect == 'map_shifted':
            m = np.roll(m, 1, axis=1)
        elif defect == 'map_transposed':                    # rows and columns exchanged (the transposed values in (H, W) order)
            m = np.ascontiguousarray(m.T).reshape(m.shape)
        elif defect == 'map_per_channel':                   # the map read with the plane's index instead of the pixel's
            m = np.stack([np.roll(m.reshape(-1), c * 7).reshape(m.shape) for c in range(3)])
        e = e_loss = m * d
        if defect == 'm2_loss':
            e_loss = m * e
    w32 = F32(w)
    loss = w32 * F32(np.sum(e_loss.astype(np.float64) * d.astype(np.float64)))
    g = w32 * ((F32(1) if defect == 'no2' else F32(2)) * e)
    a_grad = F32(np.sqrt(F32(np.sum(g.astype(np.float64) ** 2) / g.size)))
    return {'loss': loss, 'g': g, 'a_grad': a_grad}


def worst(got, want, bar):
    """(excess ratio, index) of the element that misses its bar by most (ratio <= 1: every element is inside)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    bar = np.broadcast_to(bar, err.shape)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at


def ratios(res, ref):
    """{'g', 'loss', 'a_grad'}: the error of `res` (emulate32's dict, or the device's in the same form) in units of each bar of `ref`."""
    return {'g': worst(res['g'], ref['g'], ref['g_bar'])[0],
            'loss': abs(float(res['loss']) - ref['loss']) / ref['loss_bar'],
            'a_grad': abs(float(res['a_grad']) - ref['a_grad']) / ref['a_grad_bar']}


def images(H, W, seed):
    """A preprocessed iterate and anchor (3, H, W) float32 in the range the engine sees (about -128 .. 151)."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(3, H, W) * 255 - 116).astype(F32)
    ax = (rng.rand(3, H, W) * 255 - 116).astype(F32)
    return x, ax


def mixed_map(H, W, seed):
    """(H, W) float32: uniform values, 20 % of the cells 0, 10 % multiplied by 7.5."""
    rng = np.random.RandomState(seed)
    m = rng.rand(H, W)
    pick = rng.rand(H, W)
    m[pick < 0.2] = 0.0
    m[pick > 0.9] *= 7.5
    return m.astype(F32)
