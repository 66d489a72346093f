"""NumPy restatements of the engine's colour modes (include/st2.h, csrc/color.hip, csrc/color_match.h; test infrastructure).

Luminance emission, float32, one rounding per operation (x, cx: preprocessed (3, H, W); v = x, or the corrected mean of average_oracle):
    d_c = v_c - cx_c;   l = (0.299f * d_R + 0.587f * d_G) + 0.114f * d_B;   out_c = (cx_c + MEAN_c) + l          -> (H, W, 3)
Moments, float64: mean = sum(p) / N + MEAN, cov = sum(p p^T) / N - (sum(p) / N)(sum(p) / N)^T over the preprocessed float32 values p.
Transform, float64: cov + RIDGE I = L L^T;  A = L_c L_s^-1;  b = (mean_c - MEAN) - A (mean_s - MEAN);  rounded once to float32.
Recolour, float32: s'_c = ((A[c][0] * s_R + A[c][1] * s_G) + A[c][2] * s_B) + b[c]."""

import numpy as np

from average_oracle import MEAN

F32 = np.float32
RIDGE = 1e-5 * 255.0 ** 2                                  # ST_COLOR_RIDGE
MEAN64 = MEAN.astype(np.float64)                           # the channel mean as the kernels hold it (fp32), widened
LUMA = (F32(0.299), F32(0.587), F32(0.114))                # Rec.601


def planes(x):
    x = np.asarray(x, F32)
    return x[0] if x.ndim == 4 else x


def preprocess(image):
    """(H, W, 3) uint8 or float -> (3, H, W) float32: one fp32 subtraction per element (worker.py:63-66 without the channel flip)."""
    return np.ascontiguousarray((np.asarray(image).astype(F32) - MEAN).transpose(2, 0, 1))


def emit_luma(v, cx):
    """The image handed out under st_set_original_colors for the iterate (or corrected mean) v and the content cx."""
    v, cx = planes(v), planes(cx)
    d = v - cx
    l = (LUMA[0] * d[0] + LUMA[1] * d[1]) + LUMA[2] * d[2]
    out = (cx + MEAN.reshape(3, 1, 1)) + l[None]
    assert out.dtype == F32
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def emit_luma_averaged(avg, cx):
    """... with iterate averaging on: the luminance of the corrected mean (avg: an average_oracle.AverageOracle after its update)."""
    return emit_luma(avg.corrected(), cx)


def moment_sums(p):
    """The nine sums {p_R, p_G, p_B, RR, RG, RB, GG, GB, BB} of preprocessed planes in float64, and the sums of the terms' magnitudes."""
    p = planes(p).reshape(3, -1).astype(np.float64)
    terms = [p[0], p[1], p[2]] + [p[a] * p[b] for a in range(3) for b in range(a, 3)]
    return np.array([t.sum() for t in terms]), np.array([np.abs(t).sum() for t in terms])


def moments(p):
    """(mean (3,) in image scale, cov (3, 3)) of preprocessed planes, float64."""
    p = planes(p).reshape(3, -1).astype(np.float64)
    n = p.shape[1]
    m = p.sum(axis=1) / n
    return m + MEAN64, p @ p.T / n - np.outer(m, m)


def cholesky3(s):
    """Hand-rolled lower Cholesky factor of a 3 x 3 matrix, float64."""
    s = np.asarray(s, np.float64)
    L = np.zeros((3, 3))
    L[0, 0] = np.sqrt(s[0, 0])
    L[1, 0] = s[0, 1] / L[0, 0]
    L[2, 0] = s[0, 2] / L[0, 0]
    L[1, 1] = np.sqrt(s[1, 1] - L[1, 0] ** 2)
    L[2, 1] = (s[1, 2] - L[2, 0] * L[1, 0]) / L[1, 1]
    L[2, 2] = np.sqrt(s[2, 2] - L[2, 0] ** 2 - L[2, 1] ** 2)
    return L


def transform64(mean_c, cov_c, mean_s, cov_s):
    """(A, b) in float64: np.linalg.cholesky and a triangular system (A L_s = L_c), no general inverse of a covariance."""
    Lc = np.linalg.cholesky(np.asarray(cov_c, np.float64) + RIDGE * np.eye(3))
    Ls = np.linalg.cholesky(np.asarray(cov_s, np.float64) + RIDGE * np.eye(3))
    A = np.linalg.solve(Ls.T, Lc.T).T
    b = (np.asarray(mean_c, np.float64) - MEAN64) - A @ (np.asarray(mean_s, np.float64) - MEAN64)
    return A, b


def transform(mean_c, cov_c, mean_s, cov_s):
    A, b = transform64(mean_c, cov_c, mean_s, cov_s)
    return A.astype(F32), b.astype(F32)


def recolor(s, A, b):
    """(3, H, W) or (1, 3, H, W) preprocessed style image through the affine map, float32, in the kernel's association."""
    s = np.asarray(s, F32)
    p = planes(s)
    A, b = np.asarray(A, F32).reshape(3, 3), np.asarray(b, F32).reshape(3)
    out = np.stack([((A[c, 0] * p[0] + A[c, 1] * p[1]) + A[c, 2] * p[2]) + b[c] for c in range(3)])
    assert out.dtype == F32
    return out.reshape(s.shape)


def rgb(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def grey(seed, h, w):
    """All three channels equal: a rank-1 colour covariance."""
    return np.repeat(np.random.RandomState(seed).randint(0, 256, (h, w, 1)).astype(np.uint8), 3, axis=2)


def tinted(seed, h, w):
    """A strong cast: red wide, green narrow and tied to red, blue nearly constant."""
    r = np.random.RandomState(seed)
    red = r.randint(100, 256, (h, w))
    out = np.stack([red, red // 4 + r.randint(0, 8, (h, w)), 10 + r.randint(0, 3, (h, w))], axis=2)
    return out.astype(np.uint8)


def image_pairs(h=24, w=40):
    """{name: (content, style)}: a random style, a grey style, a strongly tinted style, a grey content."""
    return {'random style': (rgb(1, h, w), rgb(2, h, w + 8)), 'grey style': (rgb(1, h, w), grey(3, h, w + 8)),
            'tinted style': (rgb(1, h, w), tinted(4, h, w + 8)), 'grey content': (grey(5, h, w), rgb(2, h, w + 8))}


def ulps(a, b):
    """Largest distance between two float32 arrays in units in the last place (of the larger magnitude, at least the smallest normal)."""
    a, b = np.asarray(a, F32).astype(np.float64), np.asarray(b, F32).astype(np.float64)
    scale = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(F32).tiny)
    return float(np.max(np.abs(a - b) / np.spacing(scale.astype(F32)).astype(np.float64)))
