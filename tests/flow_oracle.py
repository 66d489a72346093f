"""The optical-flow estimator of include/st2.h (st_flow_estimate) restated in NumPy float32: every operation rounds once, in the order
the header writes it, so the device's result is held to this one with np.array_equal.  Also the synthetic pairs with an exactly known
flow that the quality tests use."""
import numpy as np

f32 = np.float32
MAX_LEVELS = 12
AUTO_MIN_SIDE = 32
DEFAULTS = dict(alpha=0.06, warps=3, iters=40, levels=0)


def luma(image):
    """g = ((0.299f R + 0.587f G) + 0.114f B) / 255f of an HxWx3 image, uint8 or float on the 0 .. 255 scale."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError('an HxWx3 image, got %s' % (image.shape,))
    rgb = image.astype(f32)
    return ((f32(0.299) * rgb[..., 0] + f32(0.587) * rgb[..., 1]) + f32(0.114) * rgb[..., 2]) / f32(255)


def pool2(g):
    """2 x 2 / stride 2 average in Caffe's ceil mode: pixels outside count 0, the divisor is the clipped window's size."""
    h, w = g.shape
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    p = np.zeros((h2 * 2, w2 * 2), f32)
    p[:h, :w] = g
    s = (p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2])
    cy = np.minimum(2, h - 2 * np.arange(h2))
    cx = np.minimum(2, w - 2 * np.arange(w2))
    return s / (cy[:, None] * cx[None, :]).astype(f32)


def shifted(a, dy, dx):
    """a[y + dy, x + dx] with clamped indices."""
    h, w = a.shape
    yy = np.clip(np.arange(h) + dy, 0, h - 1)
    xx = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[yy][:, xx]


def smooth(g):
    t = ((shifted(g, 0, -1) + shifted(g, 0, 1)) + f32(2) * g) * f32(0.25)
    return ((shifted(t, -1, 0) + shifted(t, 1, 0)) + f32(2) * t) * f32(0.25)


def level_sizes(h, w, levels=0):
    sizes = [(h, w)]
    while len(sizes) < MAX_LEVELS:
        h, w = sizes[-1]
        if (min(h, w) < AUTO_MIN_SIDE) if levels == 0 else (len(sizes) >= levels or (h, w) == (1, 1)):
            break
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def pyramid(g, levels=0):
    """The smoothed levels of one image's luma plane, finest first: pooled from the unsmoothed planes, then each smoothed once."""
    raw = [g]
    for _ in level_sizes(g.shape[0], g.shape[1], levels)[1:]:
        raw.append(pool2(raw[-1]))
    return [smooth(r) for r in raw]


def warp(B, u, v):
    h, w = B.shape
    yy, xx = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing='ij')
    sx = np.minimum(np.maximum(xx + u, f32(0)), f32(w - 1))
    sy = np.minimum(np.maximum(yy + v, f32(0)), f32(h - 1))
    x0f, y0f = np.floor(sx), np.floor(sy)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = sx - x0f, sy - y0f
    gx, gy = f32(1) - fx, f32(1) - fy
    top = B[y0, x0] * gx + B[y0, x1] * fx
    bottom = B[y1, x0] * gx + B[y1, x1] * fx
    return top * gy + bottom * fy


def estimate_levels(from_image, to_image, alpha=0.06, warps=3, iters=40, levels=0):
    """[(A_l, B_l, flow_l (h, w, 2))] per level, finest first: what st_get_flow_level hands out."""
    pa, pb = pyramid(luma(from_image), levels), pyramid(luma(to_image), levels)
    a2 = f32(alpha) * f32(alpha)
    out = [None] * len(pa)
    u = v = None
    for l in range(len(pa) - 1, -1, -1):
        A, B = pa[l], pb[l]
        h, w = A.shape
        if u is None:
            u, v = np.zeros((h, w), f32), np.zeros((h, w), f32)
        else:
            yy, xx = np.arange(h) >> 1, np.arange(w) >> 1
            u, v = f32(2) * u[yy][:, xx], f32(2) * v[yy][:, xx]
        for _ in range(warps):
            Bw = warp(B, u, v)
            Ix = f32(0.5) * (shifted(Bw, 0, 1) - shifted(Bw, 0, -1))
            Iy = f32(0.5) * (shifted(Bw, 1, 0) - shifted(Bw, -1, 0))
            c = ((Bw - A) - Ix * u) - Iy * v
            den = (a2 + Ix * Ix) + Iy * Iy
            for _ in range(iters):
                ub = ((shifted(u, -1, 0) + shifted(u, 1, 0)) + (shifted(u, 0, -1) + shifted(u, 0, 1))) * f32(0.25)
                vb = ((shifted(v, -1, 0) + shifted(v, 1, 0)) + (shifted(v, 0, -1) + shifted(v, 0, 1))) * f32(0.25)
                r = ((Ix * ub + Iy * vb) + c) / den
                u, v = ub - Ix * r, vb - Iy * r
        assert u.dtype == f32 and v.dtype == f32
        out[l] = (A, B, np.stack([u, v], axis=-1))
    return out


def estimate(from_image, to_image, **params):
    """f = (dx, dy) per pixel of from_image, (H, W, 2) float32, with from(p) ~ to(p + f(p))."""
    return estimate_levels(from_image, to_image, **params)[0][2]


# ------------------------------------------------------------------------------------------ synthetic pairs
def texture(h, w, shift=(0.0, 0.0), rot=0.0, seed=1):
    """A sum of 24 sinusoids evaluated in float64 at displaced coordinates: (grey HxWx3 float32 image on the 0 .. 255 scale, dx, dy) with
    image(p) = base(p + (dx, dy)(p)): the pair (texture(h, w, shift, rot), texture(h, w)) has exactly the flow (dx, dy).  shift: (dx, dy)
    in pixels; rot: a rotation about the centre in radians, after the shift."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    cy, cx = (h - 1) / 2, (w - 1) / 2
    X, Y = xx + shift[0], yy + shift[1]
    if rot:
        c, s = np.cos(rot), np.sin(rot)
        X, Y = cx + c * (X - cx) - s * (Y - cy), cy + s * (X - cx) + c * (Y - cy)
    g = np.zeros((h, w))
    for _ in range(24):
        wavelength = rng.uniform(6, 60)
        angle = rng.uniform(0, np.pi)
        phase = rng.uniform(0, 2 * np.pi)
        amplitude = rng.uniform(0.3, 1) / 24
        g += amplitude * np.sin(2 * np.pi / wavelength * (np.cos(angle) * X + np.sin(angle) * Y) + phase)
    grey = f32(0.5 + 0.5 * g) * f32(255)
    return np.repeat(grey[..., None], 3, axis=2), X - xx, Y - yy


def interior_error(flow, dx, dy, margin=12):
    """Mean end-point error `margin` pixels inside the border."""
    e = np.sqrt((flow[..., 0] - dx) ** 2 + (flow[..., 1] - dy) ** 2)
    return float(e[margin:-margin, margin:-margin].mean())
