"""The style term fused into the bf16 data-gradient conv (conv3x3_mfma_bf16.hip, ST2_STYLE_FUSE), as one float64 reference with a
derived per-element bound, a fixed-order float32 emulation with seedable defects, presence coefficients for the pieces a rel-L2 cannot
see, and the float64 restatement of style_s2_trace_k's trace value.  numpy only; tests/test_gpu_fused_style.py holds the launch's output
(tapped: Engine.tap_diff) to it, tests/test_fused_style_oracle_cpu.py shows the bars reachable and sharp on the CPU.

Operands, all as the launch read them
    d16   (K, h, w)   bf16 values    the diff above the conv (the conv's output blob has K channels)
    w16   (K, C, 3, 3) bf16 values   the conv's weights (forward layout: K outputs, C inputs)
    F16   (C, h, w)   bf16 values    the bf16 copy of the style blob; m = F16 > 0 is the ReLU mask
    D     (C, C)      float32        G - G_style
    coef              float32        sw / norm, ONE float32 division (style16_pack_d_scaled_k)
    c2                float32        2 / (C C n)
    base  (C, h, w)   float32        the blob's own injected diff (content / deep-dream), or None

Reference, float64:   ref = m * convT(w16, d16) + float64(coef) * float64(c2) * (D @ F16) + base
convT is the conv's backward-data (oracle.caffe_net.conv3x3_backward_data, restated here in float64 and held to it on the CPU).

What the launch does, in order: 9 K products (bf16 x bf16: exact in fp32) into fp32 accumulators; the mask in registers; then C / 16
chunks of 16 channels, each with the hi and the lo half of D' = coef * (D * c2) (two fp32 roundings, then hi = bf16(D'), lo =
bf16(D' - hi)), into the SAME accumulators; the epilogue adds base and rounds to the forms it writes.

Per-element bound, u = 2^-24, gamma_n linearised to n u (as in style_grad_oracle); derived, not measured.  With
    A_c = m * convT(|w16|, |d16|),     A_s = |coef c2| * (|D| @ |F16|)
    conv sum        9 K u * A_c                       9 K exact products accumulated in fp32, any order; masked elements carry none
    style chunks    (2 C + 2) u * (|m convT| + A_s)   2 C more accumulations onto the masked conv sum; + 2: the epilogue's additions
    D'              (2^-16 + 2 u) * A_s               D' carried to 16 bits (hi + lo leaves 2^-17 relative; 2^-16 as style_grad_oracle's
                                                      bf16 bar), formed with two fp32 roundings
    inject          2 u * |base|
    bf16 only       + 2^-8 * (|ref| + the sum above)  one round-to-nearest of the fp32 accumulator
An element whose bound is 0 must be exact (style_grad_oracle.worst_ratio).

The last term, corrected: the issue this module answers wrote 2^-9 for it.  bf16 keeps 8 significant bits (one implicit, seven stored),
so the spacing just above a power of two is 2^-7 of the value and round-to-nearest errs by up to half of that, 2^-8 -- as u = 2^-24
belongs to the 24 bits of fp32.  With 2^-9 the exactly rounded float32 chain below (no kernel involved) misses the bound by a factor
of 1.95 at every shape; tests/test_fused_style_oracle_cpu.py holds it to <= 1 with 2^-8 and shows that 2^-9 is not reachable.

In aggregate  rel_l2(out, ref) <= AGG_MARGIN * rel_l2(emulation, ref)  with the emulation below on the same operands (never the kernel),
and every presence coefficient |<out - ref, P> / <P, P>| <= PRESENCE_BAR: P the float64 contribution of the lo half, and of each
16-channel chunk.  A piece the launch left out gives -1.  Once 9 K u A_c dominates the bound, a missing lo half (2^-9 of D', random
signs) passes every element; its coefficient does not.

The trace value: style_s2_trace_k sums c2^2 n (D (D + A))_ij D_ij (A the style target, n = C h w) -- equal to || c2 D F ||^2 where the
Gram G = D + A is that of F.  trace_reference restates it in float64 with the bound the issue of this test sets,
(C + 8) u * c2^2 n * sum |D| (|D + A|) |D|.  (The kernel's own worst case is larger -- the sum over a 32 x 32 tile adds 15 + 6 + 2
further roundings -- but those are relative to the same weight and random; the bar asserted is the smaller one.)  trace_distance
gives how far the formula is from the true || c2 D F16 ||^2: printed and recorded, never asserted (G is the Gram kernel's, not exact)."""
import numpy as np

from style_grad_oracle import AGG_MARGIN, PRESENCE_BAR, U, bar, bf16_nearest, rel_l2, worst_ratio
from split_gemm_oracle import is_bf16

F32 = np.float32
F64 = np.float64
U16 = 2.0 ** -8                 # unit roundoff of bf16, round to nearest (8 significant bits)
TILE_W = 32                     # pixels per row of a conv tile (conv3x3_mfma_bf16.hip: tiles_x = (W + 31) / 32)
CLIPPED_DEFECT = 'left_pixel_clipped_tile'
DEFECTS = ('lo_dropped', 'chunk_dropped', 'left_pixel', 'mask_after', 'no_coef', 'base_overwritten')


def _taps(d):
    """The nine shifted views of d (K, h, w): view (ky, kx) at (y, x) is d[:, y - ky + 1, x - kx + 1], zero outside."""
    K, h, w = d.shape
    p = np.zeros((K, h + 2, w + 2), d.dtype)
    p[:, 1:-1, 1:-1] = d
    return [(ky, kx, p[:, 2 - ky:2 - ky + h, 2 - kx:2 - kx + w]) for ky in range(3) for kx in range(3)]


def conv_t(w, d):
    """Backward-data of the 3 x 3, pad 1 cross-correlation in float64: dx[c, y, x] = sum_k,ky,kx w[k, c, ky, kx] d[k, y - ky + 1, x - kx + 1]."""
    w, d = np.asarray(w, F64), np.asarray(d, F64)
    out = np.zeros((w.shape[1],) + d.shape[1:], F64)
    for ky, kx, v in _taps(d):
        out += np.tensordot(w[:, :, ky, kx], v, axes=(0, 0))
    return out


def coef_of(sw, norm):
    return F32(sw) / F32(norm)


def pack_d(D, coef, c2):
    """(hi, lo) of D' = coef * (D * c2), as style16_pack_d_scaled_k forms them."""
    d = (F32(coef) * (np.ascontiguousarray(D, F32) * F32(c2)).astype(F32)).astype(F32)
    hi = bf16_nearest(d)
    return hi, bf16_nearest((d - hi).astype(F32))


class Reference:
    """ref and the weights of its bound, float64."""

    def __init__(self, w16, d16, F16, D, coef, c2, base=None, style_operand=None):
        """style_operand: the features the style product contracts where they are not F16 -- the fp32 blob, where the separate fp32
        style-gradient kernel ran (a blob the fused launch does not exist for); the mask stays that of F16 (the same signs)."""
        assert is_bf16(w16) and is_bf16(d16) and is_bf16(F16), 'the launch contracts bf16 operands'
        self.K, self.C = w16.shape[0], w16.shape[1]
        self.shape = F16.shape
        assert D.shape == (self.C, self.C) and d16.shape == (self.K,) + F16.shape[1:]
        f = np.asarray(F16 if style_operand is None else style_operand, F64).reshape(self.C, -1)
        self.m = np.asarray(F16) > 0
        self.conv = self.m * conv_t(w16, d16)
        self.A_c = self.m * conv_t(np.abs(w16), np.abs(d16))
        self.scale = float(coef) * float(c2)
        self.style = (self.scale * (np.asarray(D, F64) @ f)).reshape(self.shape)
        self.A_s = (abs(self.scale) * (np.abs(np.asarray(D, F64)) @ np.abs(f))).reshape(self.shape)
        self.base = np.zeros(self.shape, F64) if base is None else np.asarray(base, F64).reshape(self.shape)
        self.ref = self.conv + self.style + self.base

    def bound(self, bf16_only=False, separate=None):
        """separate = 'bf16' / 'fp32': the style term came from that separate style-gradient kernel through the inject buffer
        (ST2_STYLE_FUSE=0, or a blob the fused launch does not exist for): this bound plus style_grad_oracle.scaled_bound of that
        family, |coef| bar B + 2 u (|coef S_ref| + |base|) -- here bar * A_s + 2 u (|style| + |base|)."""
        b = (9 * self.K * U * self.A_c + (2 * self.C + 2) * U * (np.abs(self.conv) + self.A_s) + (2.0 ** -16 + 2 * U) * self.A_s
             + 2 * U * np.abs(self.base))
        if separate is not None:
            b = b + bar(separate, self.C) * self.A_s + 2 * U * (np.abs(self.style) + np.abs(self.base))
        return b + U16 * (np.abs(self.ref) + b) if bf16_only else b

    def branches(self):
        """(share of masked elements, median A_s / A_c and median A_c / A_s over the unmasked ones): both branches of the launch carry weight."""
        a_s, a_c = self.A_s[self.m], self.A_c[self.m]
        with np.errstate(divide='ignore', invalid='ignore'):
            return 1.0 - float(self.m.mean()), float(np.median(a_s / a_c)) if a_s.size else 0.0, float(np.median(a_c / a_s)) if a_s.size else 0.0


def clipped_column(w):
    """First pixel column of the tile column that the blob's right edge clips, or None where the width is whole tiles."""
    return None if w % TILE_W == 0 else (w // TILE_W) * TILE_W


def chunk_groups(C):
    """The 16-channel style chunks in the groups of three the double-buffered builds stage together; the last group is ragged when (C / 16) % 3 != 0."""
    n = C // 16
    return [list(range(g, min(g + 3, n))) for g in range(0, n, 3)]


def emulate(w16, d16, F16, D, coef, c2, base=None, bf16_only=False, defect=None, conv_sum=None):
    """One fixed-order float32 chain: the conv sum (k outer, the nine taps inner), the mask, then hi and lo of D' channel by channel, then
    base; bf16_only: the result rounded to bf16.  conv_sum: emulate_conv's result on the same operands (shared between runs).
    defect: one of DEFECTS -- lo_dropped; chunk_dropped (the last chunk: the last of the ragged group of three where there is one);
    left_pixel (the style operand of pixel (y, x) taken from (y, x - 1), zero at x = 0); mask_after (the mask applied after the style
    chunks); no_coef (D' = D * c2); base_overwritten (base not added).  CLIPPED_DEFECT: left_pixel in the pixels of the clipped last
    tile column only (the conv tile is TILE_W pixels wide), where the blob's width is no multiple of it."""
    assert defect is None or defect in DEFECTS or defect == CLIPPED_DEFECT
    C = w16.shape[1]
    acc = (emulate_conv(w16, d16) if conv_sum is None else conv_sum).copy()
    m = np.asarray(F16) > 0
    if defect != 'mask_after':
        acc *= m
    hi, lo = pack_d(D, F32(1) if defect == 'no_coef' else coef, c2)
    f = np.ascontiguousarray(F16, F32)
    if defect == 'left_pixel':
        f = np.concatenate([np.zeros_like(f[:, :, :1]), f[:, :, :-1]], axis=2)
    if defect == CLIPPED_DEFECT:
        x0 = clipped_column(f.shape[2])
        assert x0 is not None, 'no tile of this blob is clipped in x'
        shifted = np.concatenate([np.zeros_like(f[:, :, :1]), f[:, :, :-1]], axis=2)
        f = np.concatenate([f[:, :, :x0], shifted[:, :, x0:]], axis=2)
    f = f.reshape(C, 1, -1)
    dropped = chunk_groups(C)[-1][-1] if defect == 'chunk_dropped' else -1
    a2 = acc.reshape(C, -1)
    for j in range(C):
        if j // 16 == dropped:
            continue
        a2 += hi[:, j:j + 1] * f[j]
        if defect != 'lo_dropped':
            a2 += lo[:, j:j + 1] * f[j]
    if defect == 'mask_after':
        acc *= m
    if base is not None and defect != 'base_overwritten':
        acc += np.asarray(base, F32).reshape(acc.shape)
    return bf16_nearest(acc) if bf16_only else acc


def emulate_conv(w16, d16):
    """The unmasked conv sum as one float32 chain of exact products: k outer, the nine taps inner."""
    w16, d16 = np.ascontiguousarray(w16, F32), np.ascontiguousarray(d16, F32)
    K, C = w16.shape[:2]
    acc = np.zeros((C,) + d16.shape[1:], F32)
    taps = _taps(d16)
    for k in range(K):
        for ky, kx, v in taps:
            acc += w16[k, :, ky, kx].reshape(C, 1, 1) * v[k]
    return acc


def presence(out, R, D, F16, coef, c2):
    """{piece: least-squares coefficient of out - ref on that piece's own float64 contribution}: 'lo', and 'chunk<i>' for each 16-channel
    chunk.  A piece left out gives -1, one that is there rounding only."""
    C = R.C
    f = np.asarray(F16, F64).reshape(C, -1)
    err = (np.asarray(out, F64) - R.ref).reshape(C, -1)
    _, lo = pack_d(D, coef, c2)
    pieces = {'lo': lo.astype(F64) @ f}
    d = R.scale * np.asarray(D, F64)
    for i in range(C // 16):
        pieces['chunk%d' % i] = d[:, 16 * i:16 * i + 16] @ f[16 * i:16 * i + 16]
    res = {}
    for k, P in pieces.items():
        pp = float(np.vdot(P, P))
        res[k] = float(np.vdot(err, P)) / pp if pp > 0 else 0.0
    return res


def aggregate_ok(out, R, emulation, D, F16, coef, c2, with_presence=True):
    """(ok, figures): the rel-L2 criterion against the emulation's own error, and every piece present."""
    e, e_emu = rel_l2(out, R.ref), rel_l2(emulation, R.ref)
    fig = {'rel_l2': e, 'rel_l2_emulation': e_emu}
    ok = e <= AGG_MARGIN * e_emu
    if with_presence:
        fig['presence'] = presence(out, R, D, F16, coef, c2)
        ok = ok and all(abs(v) <= PRESENCE_BAR for v in fig['presence'].values())
    return ok, fig


def verdict(out, R, emulation, D, F16, coef, c2, bf16_only=False, with_presence=True):
    """{'element': worst ratio, 'where': (c, y, x) of it, 'aggregate': ok, 'figures': ...} -- the two halves of the criterion."""
    bound = R.bound(bf16_only)
    err = np.abs(np.asarray(out, F64).reshape(R.shape) - R.ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ok, fig = aggregate_ok(out, R, emulation, D, F16, coef, c2, with_presence)
    return {'element': worst_ratio(np.asarray(out).reshape(R.shape), R.ref, bound), 'where': tuple(int(i) for i in np.unravel_index(np.argmax(ratio), R.shape)),
            'aggregate': ok, 'figures': fig}


def trace_reference(D, A, c2, n):
    """(value, bound) of style_s2_trace_k's sum in float64: c2^2 n <D (D + A), D>."""
    D, A = np.asarray(D, F64), np.asarray(A, F64)
    s = float(c2) ** 2 * float(n)
    return s * float(np.vdot(D @ (D + A), D)), (D.shape[0] + 8) * U * s * float(np.vdot(np.abs(D) @ np.abs(D + A), np.abs(D)))


def trace_distance(D, A, c2, n, F16):
    """Relative distance of the formula from the true || c2 D F16 ||^2."""
    true = float(np.sum((float(c2) * (np.asarray(D, F64) @ np.asarray(F16, F64).reshape(D.shape[0], -1))) ** 2))
    return abs(trace_reference(D, A, c2, n)[0] - true) / max(true, 1e-300)


def fused_shape(C, h, w):
    """Does the fused launch exist for such a blob?  (engine_style.cpp: the Gram and the gradient on the bf16 copy, which take whole
    64-channel tiles and whole 64-pixel steps -- C = 96 and C = 48 never fuse.)  Elsewhere the separate style-gradient kernel runs and the tapped diff is held per element and in rel-L2."""
    return C % 64 == 0 and (h * w) % 64 == 0


def make_operands(C, K, h, w, seed=0, with_base=True, sw=1.0, conv_weight=1.0):
    """CPU operands in the manner of style_grad_oracle.make_data: ReLU'd randn * 40 features rounded to bf16, D from two Grams, bf16
    weights of He scale and a bf16 diff above, sized so that on the unmasked elements the conv sum weighs conv_weight (a power of two)
    times the style sum."""
    rs = np.random.RandomState(seed + 1000 * C + 10 * K + h * w)
    F = np.maximum(rs.randn(C, h * w) * 40, 0).astype(F32)
    F2 = np.maximum(rs.randn(C, h * w + 7) * 40, 0).astype(F32)
    g = lambda f: (f.astype(F64) @ f.astype(F64).T / f.size).astype(F32)
    D, A = (g(F) - g(F2)).astype(F32), g(F2)
    F16 = bf16_nearest(F).reshape(C, h, w)
    w16 = bf16_nearest((rs.randn(K, C, 3, 3) * np.sqrt(2.0 / (9 * C))).astype(F32))
    c2 = F32(2.0 / (float(C) * C * (C * h * w)))
    S = float(c2) * (np.abs(D.astype(F64)) @ np.abs(F16.reshape(C, -1).astype(F64)))
    norm = F32(np.sqrt(np.mean((float(c2) * (D.astype(F64) @ F16.reshape(C, -1).astype(F64))) ** 2)) or 1.0)
    coef = coef_of(sw, norm)
    # the diff above: randn scaled so that median A_c ~ median A_s
    d = rs.randn(K, h, w).astype(F32)
    a_c = conv_t(np.abs(w16), np.abs(bf16_nearest(d)))
    scale = float(conv_weight) * float(np.median(abs(float(coef)) * S) / max(np.median(a_c), 1e-300))
    d16 = bf16_nearest((d * F32(scale)).astype(F32))
    base = (rs.randn(C, h, w) * np.median(abs(float(coef)) * S)).astype(F32) if with_base else None
    return dict(w16=w16, d16=d16, F16=F16, D=D, coef=coef, c2=c2, base=base), A


__all__ = ['AGG_MARGIN', 'PRESENCE_BAR', 'U', 'DEFECTS', 'conv_t', 'coef_of', 'pack_d', 'Reference', 'chunk_groups', 'emulate', 'emulate_conv',
           'presence', 'aggregate_ok', 'verdict', 'trace_reference', 'trace_distance', 'make_operands', 'fused_shape', 'U16', 'TILE_W', 'CLIPPED_DEFECT', 'clipped_column', 'bf16_nearest', 'rel_l2', 'worst_ratio']
