"""The photorealism term (include/st2.h: st_set_matting) restated in NumPy, three ways:

    dense_laplacian      the float64 matting Laplacian L of a tiny image as a dense matrix, one window at a time (Levin et al., eq. 12)
    loss_grad64          the matrix-free float64 loss sum_c u_c' L u_c and gradient 2 L u, by plain per-window least squares
    evaluate             the exact operation order of st2.h: float64 cofactor inverse per window, fp32 passes, the device's partial sums

evaluate never uses np.sum (pairwise, another order): every sum is an explicit nine-tap loop over shifted slices, from 0, row-major.
DEFECTS names the seeded mistakes evaluate can make on request; tests/test_matting_oracle_cpu.py holds each against the right form."""
import numpy as np

F32, F64 = np.float32, np.float64
TILE_W, TILE_H, MAX_BLOCKS = 64, 4, 1024                   # matting_plan.h: kMatTileW, kMatTileH, kMatMaxBlocks
DEFECTS = ('column_major', 'eps_not_over_9', 'clipped_windows', 'no_eps_a2', 'mu_double', 'two_after_w', 'prev_second')
TAPS = tuple((dy, dx) for dy in range(3) for dx in range(3))


# ---- float64 references ------------------------------------------------------------------------------------------------------------
def dense_laplacian(I, eps):
    """I: (3, H, W) float64.  L (H W x H W), summed over the (H - 2)(W - 2) windows that lie wholly inside the image."""
    _, h, w = I.shape
    L = np.zeros((h * w, h * w), F64)
    for ky in range(1, h - 1):
        for kx in range(1, w - 1):
            idx = np.array([(ky + dy - 1) * w + (kx + dx - 1) for dy, dx in TAPS])
            win = I[:, ky - 1:ky + 2, kx - 1:kx + 2].reshape(3, 9)
            mu = win.mean(axis=1, keepdims=True)
            d = win - mu
            cov = d @ d.T / 9.0 + (eps / 9.0) * np.eye(3)
            L[np.ix_(idx, idx)] += np.eye(9) - (1.0 + d.T @ np.linalg.inv(cov) @ d) / 9.0
    return L


def loss_grad64(u, I, eps):
    """u, I: (3, H, W) float64.  (sum_c u_c' L u_c, 2 L u as (3, H, W)), matrix-free: per window the ridge fit of u on I."""
    _, h, w = I.shape
    loss, g = 0.0, np.zeros_like(u, dtype=F64)
    for ky in range(1, h - 1):
        for kx in range(1, w - 1):
            win = I[:, ky - 1:ky + 2, kx - 1:kx + 2].reshape(3, 9)
            d = win - win.mean(axis=1, keepdims=True)
            minv = np.linalg.inv(d @ d.T / 9.0 + (eps / 9.0) * np.eye(3))
            for c in range(3):
                p = u[c, ky - 1:ky + 2, kx - 1:kx + 2].reshape(9)
                dp = p - p.mean()
                a = minv @ (d @ dp / 9.0)
                r = dp - a @ d
                loss += r @ r + eps * (a @ a)
                g[c, ky - 1:ky + 2, kx - 1:kx + 2] += 2.0 * r.reshape(3, 3)
    return loss, g


# ---- the device's sums -------------------------------------------------------------------------------------------------------------
def device_sum(cells):
    """cells: (3, Hc, Wc) float64, one value per cell (window or pixel) and channel.  The sum as the device takes it: workgroups of 256
    threads walk 64 x 4 tiles (thread t: cell (t / 64, t % 64)), a thread adds channel 0, 1, 2 of its cells in double; the workgroup's
    sum is fp32 (shuffle-down tree per wave of 64, then (w0 + w1) + (w2 + w3)); the partials are summed in double by 256 threads and
    a halving tree."""
    _, hc, wc = cells.shape
    ty, tx = -(-hc // TILE_H), -(-wc // TILE_W)
    tiles = ty * tx
    grid = min(tiles, MAX_BLOCKS)
    part = np.zeros(grid, F32)
    for b in range(grid):
        acc = np.zeros((TILE_H, TILE_W), F64)
        for t in range(b, tiles, grid):
            y0, x0 = (t // tx) * TILE_H, (t % tx) * TILE_W
            blk = cells[:, y0:y0 + TILE_H, x0:x0 + TILE_W]
            for c in range(3):
                acc[:blk.shape[1], :blk.shape[2]] += blk[c]
        part[b] = block_sum(acc.astype(F32))
    return sum_partials(part)


def block_sum(v):
    """wave_reduce.h: block_sum of 256 fp32 values, thread t = 64 * wave + lane: a shuffle-down tree per wave, then (w0 + w1) + (w2 + w3)."""
    v = np.array(v, F32).reshape(4, 64)
    off = 32
    while off:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off >>= 1
    return (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])


def sum_partials(part):
    """wave_reduce.h: sum_partials -- 256 threads add every 256th partial in double, then a halving tree."""
    scratch = np.zeros(256, F64)
    for i in range(len(part)):
        scratch[i % 256] += F64(part[i])
    s = 128
    while s:
        scratch[:s] = scratch[:s] + scratch[s:2 * s]
        s >>= 1
    return scratch[0]


IP_TX, IP_TY = 256, 4                                      # passes.hip: the tile of image_pass_k


def image_pass_grad_rms(grad):
    """The trace's `grad` as image_pass_k and finalize_trace_k form it from the combined gradient (3, H, W) the pass wrote: workgroups
    of 256 threads walk tiles of 4 rows x 256 columns of one channel (tile index: column tile fastest, then row tile, then channel;
    block, block + grid, ... with grid = min(tiles, 1024)), thread t adds g * g of column t, row after row, in fp32 (one rounding per
    operation); block_sum, sum_partials, then sqrt(float(sum / (3 H W)))."""
    g = np.asarray(grad, F32).reshape(3, *np.shape(grad)[-2:])
    _, h, w = g.shape
    tx, ty = -(-w // IP_TX), -(-h // IP_TY)
    tiles = 3 * ty * tx
    grid = max(1, min(tiles, MAX_BLOCKS))
    part = np.zeros(grid, F32)
    for b in range(grid):
        acc = np.zeros(IP_TX, F32)
        for t in range(b, tiles, grid):
            x0, y0, ch = (t % tx) * IP_TX, (t // tx % ty) * IP_TY, t // tx // ty
            for y in range(y0, min(y0 + IP_TY, h)):
                row = g[ch, y, x0:x0 + IP_TX]
                acc[:row.size] = acc[:row.size] + row * row
        part[b] = block_sum(acc)
    return np.sqrt(F32(sum_partials(part) / (3.0 * h * w)))


# ---- the operation order of st2.h ----------------------------------------------------------------------------------------------------
def taps(a, order=TAPS):
    """The nine shifted views of planes (.., H, W), each (.., H - 2, W - 2), in visiting order."""
    h, w = a.shape[-2:]
    return [a[..., dy:dy + h - 2, dx:dx + w - 2] for dy, dx in order]


def windows(I, eps, defect=None):
    """mu (3, Hw, Ww) and M (6, Hw, Ww) as float32, from the fp32 planes I: float64, cofactor inverse, one rounding per operation."""
    t = taps(I.astype(F64))
    s = np.zeros_like(t[0])
    for v in t:
        s = s + v
    mu = s / 9.0
    d = [v - mu for v in t]
    cov = {}
    for a in range(3):
        for b in range(a, 3):
            acc = np.zeros_like(mu[0])
            for v in d:
                acc = acc + v[a] * v[b]
            cov[a, b] = acc / 9.0
    e9 = F64(eps) if defect == 'eps_not_over_9' else F64(eps) / 9.0
    s00, s11, s22, s01, s02, s12 = cov[0, 0] + e9, cov[1, 1] + e9, cov[2, 2] + e9, cov[0, 1], cov[0, 2], cov[1, 2]
    c00 = s11 * s22 - s12 * s12
    c01 = s02 * s12 - s01 * s22
    c02 = s01 * s12 - s02 * s11
    det = (s00 * c00 + s01 * c01) + s02 * c02
    c11 = s00 * s22 - s02 * s02
    c12 = s01 * s02 - s00 * s12
    c22 = s00 * s11 - s01 * s01
    M = np.stack([c / det for c in (c00, c01, c02, c11, c12, c22)])
    return (mu if defect == 'mu_double' else mu.astype(F32)), M.astype(F32)


def evaluate(x, cx, weight, eps, prev=(), want_grad=True, defect=None):
    """x, cx: preprocessed planes (3, H, W) float32.  prev: the planes (3, H, W) of the optional terms before this one (g_lap, g_anc), in
    order.  Returns a dict: I, mu, M, a_pb (3, 4, Hw, Ww), J (3, Hw, Ww) float64, sum_j, m_loss, and with a gradient g_mat, extra, sum_g2,
    m_grad."""
    if defect == 'clipped_windows':
        return evaluate_clipped(x, cx, weight, eps, prev)
    x, cx = np.asarray(x, F32), np.asarray(cx, F32)
    _, h, w = x.shape
    u, I = x / F32(255), cx / F32(255)
    order = tuple((dy, dx) for dx in range(3) for dy in range(3)) if defect == 'column_major' else TAPS
    mu, M = windows(I, eps, defect)
    m = {(0, 0): M[0], (0, 1): M[1], (0, 2): M[2], (1, 1): M[3], (1, 2): M[4], (2, 2): M[5]}
    m.update({(b, a): v for (a, b), v in list(m.items())})
    dI = [(v - mu).astype(F32) for v in taps(I, order)]                    # (mu_double: the subtraction in double, then rounded)
    ut = taps(u, order)
    a_pb, J = np.zeros((3, 4, h - 2, w - 2), F32), np.zeros((3, h - 2, w - 2), F64)
    for c in range(3):
        s = np.zeros((h - 2, w - 2), F32)
        for v in ut:
            s = s + v[c]
        pb = s / F32(9)
        dp = [v[c] - pb for v in ut]
        cov = []
        for a in range(3):
            acc = np.zeros_like(pb)
            for di, pi in zip(dI, dp):
                acc = acc + di[a] * pi
            cov.append(acc / F32(9))
        coef = [(m[a, 0] * cov[0] + m[a, 1] * cov[1]) + m[a, 2] * cov[2] for a in range(3)]
        jc = np.zeros_like(J[c])
        for di, pi in zip(dI, dp):
            r = pi - ((coef[0] * di[0] + coef[1] * di[1]) + coef[2] * di[2])
            assert r.dtype == F32
            jc = jc + r.astype(F64) * r.astype(F64)
        if defect != 'no_eps_a2':
            a64 = [v.astype(F64) for v in coef]
            jc = jc + F64(eps) * ((a64[0] * a64[0] + a64[1] * a64[1]) + a64[2] * a64[2])
        J[c] = jc
        a_pb[c, :3], a_pb[c, 3] = coef, pb
    wf = F32(weight)
    sum_j = device_sum(J)
    with np.errstate(over='ignore', under='ignore'):
        out = {'I': I, 'mu': np.asarray(mu, F32), 'M': M, 'a_pb': a_pb, 'J': J, 'sum_j': sum_j, 'm_loss': wf * F32(sum_j), 'm_grad': F32(0)}
    if not want_grad:
        return out
    mu32 = mu if defect == 'mu_double' else mu.astype(F32)
    Lu = np.zeros((3, h, w), F32)
    for dy, dx in TAPS:                                     # window (y - 2 + dy, x - 2 + dx) of pixel (y, x): pixels that window has
        ys, xs = slice(2 - dy, 2 - dy + h - 2), slice(2 - dx, 2 - dx + w - 2)
        di = (I[:, ys, xs] - mu32).astype(F32)
        for c in range(3):
            dp = u[c, ys, xs] - a_pb[c, 3]
            r = dp - ((a_pb[c, 0] * di[0] + a_pb[c, 1] * di[1]) + a_pb[c, 2] * di[2])
            Lu[c, ys, xs] = Lu[c, ys, xs] + r
    with np.errstate(over='ignore', under='ignore'):
        g = F32(2) * (wf * Lu) if defect == 'two_after_w' else wf * (F32(2) * Lu)
    out.update(finish(g, prev, defect, h, w))
    return out


def finish(g, prev, defect, h, w):
    prev = [np.asarray(p, F32).reshape(3, h, w) for p in prev]
    if not prev:
        extra = g
    elif defect == 'prev_second' and len(prev) == 2:        # the other association: g_lap + (g_anc + g_mat)
        extra = prev[0] + (prev[1] + g)
    else:
        before = prev[0] if len(prev) == 1 else prev[0] + prev[1]
        extra = before + g
    sum_g2 = device_sum(g.astype(F64) * g.astype(F64))
    return {'g_mat': g, 'extra': extra, 'sum_g2': sum_g2, 'm_grad': np.sqrt(F32(sum_g2 / (3.0 * h * w)))}


def evaluate_clipped(x, cx, weight, eps, prev=()):
    """The seeded defect `clipped_windows`: a window at EVERY pixel, clipped to the image (4 or 6 pixels at the border), the rest of the
    arithmetic as st2.h orders it.  Loops: tiny images only."""
    x, cx = np.asarray(x, F32), np.asarray(cx, F32)
    _, h, w = x.shape
    u, I = x / F32(255), cx / F32(255)
    Lu, total = np.zeros((3, h, w), F32), F64(0)
    for ky in range(h):
        for kx in range(w):
            px = [(y, xx) for y in range(max(ky - 1, 0), min(ky + 2, h)) for xx in range(max(kx - 1, 0), min(kx + 2, w))]
            n = len(px)
            win = np.array([[F64(I[a, y, xx]) for y, xx in px] for a in range(3)])
            mu = np.array([sum(win[a], F64(0)) / n for a in range(3)])
            d = win - mu[:, None]
            s = np.array([[sum(d[a] * d[b], F64(0)) / n for b in range(3)] for a in range(3)]) + (F64(eps) / n) * np.eye(3)
            M = np.linalg.inv(s).astype(F32)
            mu = mu.astype(F32)
            dI = np.array([[I[a, y, xx] - mu[a] for y, xx in px] for a in range(3)], F32)
            for c in range(3):
                p = np.array([u[c, y, xx] for y, xx in px], F32)
                pb = sum(p, F32(0)) / F32(n)
                dp = p - pb
                cov = np.array([sum(dI[a] * dp, F32(0)) / F32(n) for a in range(3)], F32)
                a = np.array([(M[k, 0] * cov[0] + M[k, 1] * cov[1]) + M[k, 2] * cov[2] for k in range(3)], F32)
                r = dp - ((a[0] * dI[0] + a[1] * dI[1]) + a[2] * dI[2])
                total += sum(r.astype(F64) * r.astype(F64), F64(0)) + F64(eps) * sum(a.astype(F64) ** 2, F64(0))
                for (y, xx), rv in zip(px, r):
                    Lu[c, y, xx] += rv
    wf = F32(weight)
    out = {'sum_j': total, 'm_loss': wf * F32(total)}
    out.update(finish(wf * (F32(2) * Lu), prev, None, h, w))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def planes(kind, h, w, seed):
    """Preprocessed planes (3, H, W) float32 in the range of a mean-subtracted image: noise, a smooth ramp, or noise with a flat patch."""
    rng = np.random.RandomState(seed)
    if kind == 'ramp':
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
        base = np.stack([60 * yy + 90 * xx, 120 * yy * xx + 20, 150 * (1 - xx) + 40 * yy]) + rng.rand(3, 1, 1) * 30
    else:
        base = rng.rand(3, h, w) * 255
        if kind == 'flat':
            base[:, h // 3:h // 3 + 4, w // 3:w // 3 + 5] = rng.rand(3, 1, 1) * 255
    return (base - np.array([104.0, 117.0, 123.0])[:, None, None]).astype(F32)
