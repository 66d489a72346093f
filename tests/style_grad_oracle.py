"""The style gradient S = c2 * (D @ F) as a plain GEMM check: a float64 reference with its componentwise weight, one fixed-order
float32 emulation per kernel family, and the bars the GPU kernels are held to (tests/test_gpu_style_grad.py).  numpy only.

    D   (C, C)   float32   G - G_style, as the launch read it (st_get_layer_terms)
    F   (C, hw)  float32   the blob (bf16 family: the blob rounded to bf16, the copy the kernel reads)
    c2           float32   2 / (C * C * n), n the elements of the blob of the WHOLE image

Reference   S_ref = float64(c2) * (float64(D) @ float64(F)),   weight  B = float64(c2) * (|D| @ |F|).

Bars, u = 2^-24, derived and not measured.  Per element |S - S_ref| <= bar * B with
    fp32    (C + 8) u          gamma_C of a C-term fp32 sum in any order; 8 covers the scalar roundings of c2, sw / norm and the epilogue
    split   (C + 8) u          the kernel's claim is "closer to a double-precision product than the fp32 kernel": it gets that kernel's
                               bar.  (On paper its worst case is (6 C + 8) u: six accumulations per channel.)
    bf16    (2 C + 8) u + 2^-16    2 C accumulations (hi and lo of D), plus D carried to 16 bits (hi + lo leaves a residual
                               of 2^-17 relative)
A scaled epilogue dst = coef * S (+ b) gets  coef * bar * B + 2 u (|coef * S_ref| + |b|): the product and the sum round once each.
In aggregate  rel_l2(S, S_ref) <= AGG_MARGIN * rel_l2(emulation, S_ref), the right-hand side computed from the same D and F against the
reference (never against the kernel); the margin covers the kernel's order of summation differing from the chain's.  The split
family's aggregate criterion has a second half, split_presence below: every one of its six partial products is there."""
import numpy as np

from split_gemm_oracle import bf16_nearest, is_bf16, rel_l2, split3

F32 = np.float32
U = 2.0 ** -24
AGG_MARGIN = 3.0
FAMILIES = ('fp32', 'split', 'bf16')
# the six partial products the split kernels keep: (term of D, term of F), h / m / l = the three bf16 terms of split3, largest first
SPLIT_PAIRS = {'hh': (0, 0), 'hm': (0, 1), 'mh': (1, 0), 'hl': (0, 2), 'lh': (2, 0), 'mm': (1, 1)}
SPLIT_ORDER = ('hl', 'lh', 'mm', 'hm', 'mh', 'hh')      # smallest weight first, as the kernels issue them


def c2_of(C, n):
    return F32(2.0 / (float(C) * float(C) * float(n)))


def reference(D, F, c2):
    """(S_ref, B) in float64."""
    D64, F64 = np.asarray(D, np.float64), np.asarray(F, np.float64)
    return float(c2) * (D64 @ F64), float(c2) * (np.abs(D64) @ np.abs(F64))


def bar(family, C):
    if family in ('fp32', 'split'):
        return (C + 8) * U
    if family == 'bf16':
        return (2 * C + 8) * U + 2.0 ** -16
    raise ValueError(family)


def scaled_bound(family, C, coef, S_ref, B, base=None):
    """Per-element bound of dst = coef * S (+ base) against float64(coef) * S_ref (+ base)."""
    coef = abs(float(coef))
    b = 0.0 if base is None else np.abs(np.asarray(base, np.float64))
    return coef * bar(family, C) * B + 2 * U * (coef * np.abs(S_ref) + b)


def _chain(terms, shape, skip=None):
    """sum_j sum_t a_t[:, j] * b_t[j, :] as ONE float32 chain: every product rounded to float32, every addition rounded to float32,
    channel by channel, the terms of one channel in the order given.  skip = (m, j, p): that one product of the first term is left out."""
    acc = np.zeros(shape, F32)
    C = terms[0][0].shape[1]
    for j in range(C):
        for t, (a, b) in enumerate(terms):
            prod = a[:, j:j + 1] * b[j:j + 1, :]          # float32 x float32 -> float32
            if skip is not None and t == 0 and skip[1] == j:
                prod[skip[0], skip[2]] = 0
            acc += prod
    return acc


def emulate_fp32(D, F, c2, drop_product=None):
    """fp32 products, fp32 chain, then one multiplication by c2."""
    D, F = np.ascontiguousarray(D, F32), np.ascontiguousarray(F, F32)
    return _chain([(D, F)], (D.shape[0], F.shape[1]), drop_product) * F32(c2)


def emulate_split(D, F, c2, drop=()):
    """Three-way bf16 split of D and F; the six kept products (each exact in fp32) accumulated in one fp32 chain.  drop: names of
    SPLIT_PAIRS left out (a seeded defect)."""
    sd, sf = split3(D), split3(F)
    terms = [(sd[SPLIT_PAIRS[k][0]], sf[SPLIT_PAIRS[k][1]]) for k in SPLIT_ORDER if k not in drop]
    return _chain(terms, (D.shape[0], F.shape[1])) * F32(c2)


def emulate_bf16(D, F16, c2, drop_lo=False):
    """D = hi + lo (hi = bf16(D), lo = bf16(D - hi)), F already bf16 values; both halves into one fp32 chain."""
    D = np.ascontiguousarray(D, F32)
    F16 = np.ascontiguousarray(F16, F32)
    assert is_bf16(F16), 'the bf16 family contracts the bf16 copy of the blob'
    hi = bf16_nearest(D)
    lo = bf16_nearest((D - hi).astype(F32))
    terms = [(hi, F16)] if drop_lo else [(hi, F16), (lo, F16)]
    return _chain(terms, (D.shape[0], F16.shape[1])) * F32(c2)


EMULATE = {'fp32': emulate_fp32, 'split': emulate_split, 'bf16': emulate_bf16}


def split_presence(S, S_ref, D, F, c2):
    """{name: coefficient} for the six kept partial products P_k = c2 * (D_a @ F_b) of the split family: the least-squares coefficient
    <S - S_ref, P_k> / <P_k, P_k> of the error on that product's own contribution.  A kernel that leaves P_k out has the error
    -P_k + rounding, coefficient -1; one that adds it has rounding only, coefficient ~ e / (|P_k| sqrt(N)) (e the rms rounding error, N
    the elements).  The head term rounds to NEAREST, so the lower terms have random signs and a missing low-order product is an
    incoherent error of 4e-7 .. 2.5e-6 relative: below 3 x the rel-L2 of a correct fp32 chain from C = 200 up (CPU figures in
    tests/test_style_grad_oracle_cpu.py).  The rel-L2 criterion alone does not see it there; this one does at every size."""
    sd = [t.astype(np.float64) for t in split3(D)]
    sf = [t.astype(np.float64) for t in split3(F)]
    err = np.asarray(S, np.float64) - S_ref
    out = {}
    for k, (a, b) in SPLIT_PAIRS.items():
        P = float(c2) * (sd[a] @ sf[b])
        pp = float(np.vdot(P, P))
        out[k] = float(np.vdot(err, P)) / pp if pp > 0 else 0.0
    return out


PRESENCE_BAR = 0.5      # halfway between "added" (0) and "left out" (-1)


def aggregate_ok(family, S, S_ref, emulation, D=None, F=None, c2=None):
    """(ok, figures): rel_l2(S, S_ref) <= AGG_MARGIN * rel_l2(emulation, S_ref), and for the split family every kept partial product
    present (|coefficient| <= PRESENCE_BAR)."""
    e, e_emu = rel_l2(S, S_ref), rel_l2(emulation, S_ref)
    fig = {'rel_l2': e, 'rel_l2_emulation': e_emu}
    ok = e <= AGG_MARGIN * e_emu
    if family == 'split':
        fig['presence'] = split_presence(S, S_ref, D, F, c2)
        ok = ok and all(abs(v) <= PRESENCE_BAR for v in fig['presence'].values())
    return ok, fig


def worst_ratio(S, S_ref, bound):
    """max |S - S_ref| / bound; an element whose bound is 0 must be exact (ratio inf otherwise)."""
    err = np.abs(np.asarray(S, np.float64) - S_ref)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def make_data(C, hw, seed=0):
    """ReLU'd randn * 40 features F (C, hw) and D = Gram(F) - Gram(F') of two such blobs, all float32."""
    rs = np.random.RandomState(seed + 1000 * C + hw)
    F = np.maximum(rs.randn(C, hw) * 40, 0).astype(F32)
    F2 = np.maximum(rs.randn(C, hw + 7) * 40, 0).astype(F32)
    g = lambda f: (f.astype(np.float64) @ f.astype(np.float64).T / f.size).astype(F32)
    return (g(F) - g(F2)).astype(F32), F


__all__ = ['U', 'AGG_MARGIN', 'FAMILIES', 'c2_of', 'reference', 'bar', 'scaled_bound', 'emulate_fp32', 'emulate_split', 'emulate_bf16',
           'EMULATE', 'split_presence', 'PRESENCE_BAR', 'aggregate_ok', 'worst_ratio', 'make_data', 'rel_l2', 'bf16_nearest']
