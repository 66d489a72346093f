"""The frame-sequence definitions of include/st2.h restated in NumPy: the reliability of a backward flow against a forward flow in
float64, operation for operation in the header's order (jobs.warp_planar is the warp), and the long-term composition in float32.  The
device computes these doubles in this order, so the engine is held to them with np.array_equal (tests/test_gpu_frames.py);
tests/test_frames_oracle_cpu.py holds this file to hand cases."""
import numpy as np

from style_transfer2_amd import jobs

F32, F64 = np.float32, np.float64


def parts(bwd, fwd):
    """The three tests of the header as boolean (H, W) arrays: (outside, disoccluded, boundary).  bwd, fwd: (H, W, 2) of (dx, dy)."""
    bwd, fwd = np.asarray(bwd, F32), np.asarray(fwd, F32)
    if bwd.ndim != 3 or bwd.shape[2] != 2 or fwd.shape != bwd.shape:
        raise ValueError('two flows (H, W, 2) of one size, got %s and %s' % (bwd.shape, fwd.shape))
    h, w = bwd.shape[:2]
    u, v = bwd[..., 0].astype(F64), bwd[..., 1].astype(F64)
    yy, xx = np.meshgrid(np.arange(h, dtype=F64), np.arange(w, dtype=F64), indexing='ij')
    px, py = xx + u, yy + v
    outside = (px < 0) | (px > w - 1) | (py < 0) | (py > h - 1)
    wt = jobs.warp_planar(np.ascontiguousarray(fwd.transpose(2, 0, 1)), bwd).astype(F64)      # rounded to float32, as the warp is
    wx, wy = wt[0], wt[1]
    ex, ey = wx + u, wy + v
    disoccluded = ex * ex + ey * ey > 0.01 * ((wx * wx + wy * wy) + (u * u + v * v)) + 0.5
    xr, yd = np.minimum(np.arange(w) + 1, w - 1), np.minimum(np.arange(h) + 1, h - 1)
    ux, uy = u[:, xr] - u, u[yd, :] - u
    vx, vy = v[:, xr] - v, v[yd, :] - v
    boundary = (ux * ux + uy * uy) + (vx * vx + vy * vy) > 0.01 * (u * u + v * v) + 0.002
    return outside, disoccluded, boundary


def reliability(bwd, fwd, mask=None):
    """c(bwd, fwd) as float32 (H, W): 0 where any of the three tests holds, else 1; fwd None: 1 everywhere; bwd None: no flow, (0, 0).
    With a mask: float32(c * mask), the product in float64."""
    if fwd is None:
        shape = np.shape(bwd)[:2] if bwd is not None else np.shape(mask)
        c = np.ones(shape, F64)
    else:
        fwd = np.asarray(fwd, F32)
        o, d, b = parts(np.zeros_like(fwd) if bwd is None else bwd, fwd)
        c = np.where(o | d | b, 0.0, 1.0)
    if mask is not None:
        c = c * np.asarray(mask, F32).astype(F64)
    return c.astype(F32)


def compose(ax, M, a_j, c):
    """One accumulating call in float32: m = max(c - M, 0); the planes (3, H, W) take a_j where m > 0; M += m.  Returns (ax, M, m)."""
    ax, M, a_j, c = (np.asarray(v, F32) for v in (ax, M, a_j, c))
    m = np.maximum(c - M, F32(0))
    return np.where(m > 0, a_j, ax).astype(F32), (M + m).astype(F32), m
