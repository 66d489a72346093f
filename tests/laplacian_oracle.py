"""The Laplacian-steered content term of include/st2.h (st_set_laplacian) restated in NumPy float64, with per-element error bars that are
derived, not measured, and a float32 emulation of the documented operation order (with seeded defects) that shows the bars can be met
and that they bite.

Definition.  u = x / 255, uc = cx / 255, planar (3, H, W).  A level is (p, w).  Per level and channel:
  P(u)[i, j]  mean of u over [i p, (i + 1) p) x [j p, (j + 1) p) clipped to the image, divided by the clipped window's pixel count
  D(q)[i, j]  sum of q[i, j] - q[n] over the existing ones of the four neighbours n
  E = D(P(u)) - T,  T = D(P(uc));  loss = w * sum E^2;  g_lap[c, y, x] = sum over levels of w * 2 * D(E)[c, y // p, x // p] / count

The bars.  eps = 2^-24 is the unit roundoff of float32 (round to nearest: every operation's result is within eps relative of the exact one).
  E.  A cell of P(u) is a sum of at most p^2 values u = fl(x / 255) followed by one division: however the sum is ordered, the computed
      mean m' satisfies |m' - m| <= (p^2 + 1) eps * mean(|u|) to first order (one eps for the division by 255, at most p^2 - 1 for the
      additions, one for the division by the count).  D takes up to four differences and four additions of such means: its computed
      value is within (p^2 + 1 + 6) eps of sum over the existing neighbours of (|m| + |m_n|), generously, which is A(u): the stencil
      with absolute coefficients on the pooled absolute values.  The same holds for T with uc, and the subtraction E = D - T adds one
      more eps of |D| + |T| <= A(u) + A(uc).  Together: |E' - E| <= B_E = (p^2 + 8) eps (A(u) + A(uc)), for any summation order of the
      pool, the division, the stencil and the subtraction.  T alone: (p^2 + 7) eps A(uc) <= (p^2 + 8) eps A(uc).
  g_lap.  The device applies D to E' = E + d with |d| <= B_E.  D is linear: |D(E') - D(E)| <= A(B_E) (absolute stencil of the bar
      itself), and the eight float32 operations of the stencil on E' add at most 8 eps A(|E| + B_E).  The factor 2 is exact; the
      conversion of w to float32, the multiplication by w and the division by the count are one eps each of the level's term, and the
      sum over n levels adds n eps of the sum of the terms' magnitudes.  Per pixel:
        B_g = sum_l |w_l| 2 / count * [A(B_E) + 8 eps A(|E| + B_E)] + (3 + n) eps sum_l |w_l| 2 (|D(E)| + A(B_E)) / count.
  loss.  sum E'^2 differs from sum E^2 by at most sum (2 |E| B_E + B_E^2).  The final conversions: the squares are summed in double
      (exact to 2^-53), but each workgroup's partial is rounded to float32 and combined by nine float32 additions (ten eps), the total is
      converted to float32 (one), w is converted and multiplied (two), and the levels are added (n): (13 + n) eps of sum |w| (|E| + B_E)^2.
  l_grad = sqrt(float(sum g^2 / N)): the sum of squares moves by at most dG = sum (2 |g| B_g + B_g^2) + 10 eps sum (|g| + B_g)^2, so the
      value lies in [sqrt(max(G - dG, 0) / N), sqrt((G + dG) / N)], plus three eps for the conversion, the division and sqrtf.
"""
import numpy as np

EPS = 2.0 ** -24
F32 = np.float32
POOLS = (1, 2, 4, 8, 16, 32)


def validate(levels):
    levels = [tuple(lv) for lv in levels]
    if len(levels) > 3:
        raise ValueError('at most three levels')
    pools = [p for p, _ in levels]
    if any(p not in POOLS for p in pools) or len(set(pools)) != len(pools):
        raise ValueError('pool sizes: distinct, from %r' % (POOLS,))
    if any(not np.isfinite(w) or w == 0 for _, w in levels):
        raise ValueError('weights: finite and non-zero')
    return levels


def counts(H, W, p):
    """(hp, wp) array of the clipped windows' pixel counts."""
    rows = np.minimum(np.arange(0, H, p) + p, H) - np.arange(0, H, p)
    cols = np.minimum(np.arange(0, W, p) + p, W) - np.arange(0, W, p)
    return rows[:, None] * cols[None, :]


def pool(u, p):
    """P(u): (C, H, W) -> (C, hp, wp), in u's dtype (the oracle calls it with float64)."""
    H, W = u.shape[1:]
    s = np.add.reduceat(np.add.reduceat(u, np.arange(0, H, p), axis=1), np.arange(0, W, p), axis=2)
    return s / counts(H, W, p)


def stencil(q, absolute=False):
    """D(q), or with absolute=True A(q): sum over the existing neighbours of (q + q_n) (q >= 0 then)."""
    sgn = 1.0 if absolute else -1.0
    d = np.zeros_like(q)
    d[:, 1:, :] += q[:, 1:, :] + sgn * q[:, :-1, :]
    d[:, :-1, :] += q[:, :-1, :] + sgn * q[:, 1:, :]
    d[:, :, 1:] += q[:, :, 1:] + sgn * q[:, :, :-1]
    d[:, :, :-1] += q[:, :, :-1] + sgn * q[:, :, 1:]
    return d


def upsample(d, p, H, W):
    return np.repeat(np.repeat(d, p, axis=1), p, axis=2)[:, :H, :W]


def loss_and_grad_u(u, uc, levels):
    """float64: (loss, dloss/du) of the definition, on u and uc directly (the finite-difference check differentiates this)."""
    H, W = u.shape[1:]
    loss, g = 0.0, np.zeros_like(u)
    for p, w in levels:
        E = stencil(pool(u, p)) - stencil(pool(uc, p))
        loss += w * np.sum(E * E)
        g += upsample(w * 2.0 * stencil(E) / counts(H, W, p), p, H, W)
    return loss, g


def evaluate(x, cx, levels):
    """The oracle: x, cx planar (3, H, W) (any float dtype; taken as exact), levels [(p, w)].  Returns a dict with per level T, E and
    their bars, the loss with its bar, g_lap with its per-pixel bar, l_grad with its bar."""
    levels = validate(levels)
    x, cx = np.asarray(x, np.float64), np.asarray(cx, np.float64)
    H, W = x.shape[1:]
    u, uc = x / 255.0, cx / 255.0
    n = len(levels)
    out = {'T': [], 'E': [], 'T_bar': [], 'E_bar': [], 'level_loss': []}
    g, g_bar, g_mag = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    loss, loss_bar = 0.0, 0.0
    for p, w in levels:
        cnt = counts(H, W, p)
        Au, Ac = stencil(pool(np.abs(u), p), True), stencil(pool(np.abs(uc), p), True)
        T = stencil(pool(uc, p))
        E = stencil(pool(u, p)) - T
        BE = (p * p + 8) * EPS * (Au + Ac)
        out['T'].append(T); out['E'].append(E)
        out['T_bar'].append((p * p + 8) * EPS * Ac); out['E_bar'].append(BE)
        DE = stencil(E)
        ABE = stencil(BE, True)
        g += upsample(w * 2.0 * DE / cnt, p, H, W)
        g_bar += upsample(abs(w) * 2.0 / cnt * (ABE + 8 * EPS * stencil(np.abs(E) + BE, True)), p, H, W)
        g_mag += upsample(abs(w) * 2.0 * (np.abs(DE) + ABE) / cnt, p, H, W)
        out['level_loss'].append(w * np.sum(E * E))
        loss += w * np.sum(E * E)
        loss_bar += abs(w) * np.sum(2 * np.abs(E) * BE + BE * BE) + (13 + n) * EPS * abs(w) * np.sum((np.abs(E) + BE) ** 2)
    g_bar += (3 + n) * EPS * g_mag
    N = g.size
    G = np.sum(g * g)
    dG = np.sum(2 * np.abs(g) * g_bar + g_bar * g_bar) + 10 * EPS * np.sum((np.abs(g) + g_bar) ** 2)
    l_grad = np.sqrt(G / N)
    hi, lo = np.sqrt((G + dG) / N), np.sqrt(max(G - dG, 0.0) / N)
    out.update(loss=loss, loss_bar=loss_bar, g=g, g_bar=g_bar, l_grad=l_grad,
               l_grad_bar=max(hi - l_grad, l_grad - lo) + 3 * EPS * hi)
    return out


# ------------------------------------------------------------------------------------------------------------------- float32 emulation
DEFECTS = ('divisor', 'periodic', 'swap', 'no2', 'weights', 'target_x')


def _pool32(u, p, defect):
    """The documented order: a window's sum from the sums of its four quarters as (a + b) + (c + d), pixels outside the image 0."""
    C, H, W = u.shape
    hp, wp = -(-H // p), -(-W // p)
    s = np.zeros((C, hp * p, wp * p), F32)
    s[:, :H, :W] = u
    k = p
    while k > 1:
        s = (s[:, 0::2, 0::2] + s[:, 0::2, 1::2]) + (s[:, 1::2, 0::2] + s[:, 1::2, 1::2])
        k //= 2
    cnt = np.full((hp, wp), p * p) if defect == 'divisor' else counts(H, W, p)
    return (s / cnt.astype(F32)).astype(F32)


def _stencil32(q, defect):
    """d from 0, += q - q[n] in the order up, down, left, right over the neighbours that exist."""
    d = np.zeros_like(q)
    if defect == 'periodic':
        for shift, axis in ((1, 1), (-1, 1), (1, 2), (-1, 2)):
            d = d + (q - np.roll(q, shift, axis=axis))
        return d
    d[:, 1:, :] += q[:, 1:, :] - q[:, :-1, :]
    d[:, :-1, :] += q[:, :-1, :] - q[:, 1:, :]
    d[:, :, 1:] += q[:, :, 1:] - q[:, :, :-1]
    d[:, :, :-1] += q[:, :, :-1] - q[:, :, 1:]
    return d


def emulate32(x, cx, levels, defect=None):
    """What the device is documented to compute, in NumPy float32 (defect: one of DEFECTS seeds a bug).  Returns T, E per level, the
    loss (float32 from double sums) and g_lap, l_grad."""
    assert defect is None or defect in DEFECTS
    levels = validate(levels)
    x, cx = np.asarray(x, F32), np.asarray(cx, F32)
    H, W = x.shape[1:]
    u, uc = x / F32(255), cx / F32(255)
    if defect == 'target_x':
        uc = u
    weights = [w for _, w in levels]
    if defect == 'weights' and len(weights) > 1:
        weights[0], weights[1] = weights[1], weights[0]
    Ts, Es = [], []
    g = np.zeros_like(u)
    loss = F32(0)
    for (p, _), w in zip(levels, weights):
        w32 = F32(w)
        cnt = counts(H, W, p).astype(F32)
        T = _stencil32(_pool32(uc, p, defect), defect)
        E = _stencil32(_pool32(u, p, defect), defect) - T
        Ts.append(T); Es.append(E)
        DE = _stencil32(E, defect)
        term = (w32 * ((F32(1) if defect == 'no2' else F32(2)) * DE)) / cnt
        if defect == 'swap':                               # the cell index with y and x exchanged
            yy, xx = np.minimum(np.arange(W) // p, term.shape[1] - 1), np.minimum(np.arange(H) // p, term.shape[2] - 1)
            g = g + term[:, yy[None, :], xx[:, None]]
        else:
            g = g + upsample(term, p, H, W)
        loss = loss + w32 * F32(np.sum(E.astype(np.float64) ** 2))
    l_grad = F32(np.sqrt(F32(np.sum(g.astype(np.float64) ** 2) / g.size)))
    return {'T': Ts, 'E': Es, 'loss': loss, 'g': g, 'l_grad': l_grad}


def worst(got, want, bar):
    """(excess ratio, index) of the element that misses its bar by most (ratio <= 1: every element is inside)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), at


def misses(res, ref):
    """Names of the quantities of `res` (emulate32's dict, or the device's in the same form) outside their bars against `ref`."""
    bad = []
    for l in range(len(ref['E'])):
        if worst(res['T'][l], ref['T'][l], ref['T_bar'][l])[0] > 1:
            bad.append('T%d' % l)
        if worst(res['E'][l], ref['E'][l], ref['E_bar'][l])[0] > 1:
            bad.append('E%d' % l)
    if worst(res['g'], ref['g'], ref['g_bar'])[0] > 1:
        bad.append('g')
    if abs(float(res['loss']) - ref['loss']) > ref['loss_bar']:
        bad.append('loss')
    if abs(float(res['l_grad']) - ref['l_grad']) > ref['l_grad_bar']:
        bad.append('l_grad')
    return bad


def images(H, W, seed):
    """A preprocessed iterate and content image (3, H, W) float32 in the range the engine sees (about -128 .. 151)."""
    rng = np.random.RandomState(seed)
    x = (rng.rand(3, H, W) * 255 - 116).astype(F32)
    cx = (rng.rand(3, H, W) * 255 - 116).astype(F32)
    return x, cx
