"""The arithmetic of the split-operand Gram / style-gradient kernels (csrc/gram_split.hip), restated in numpy.

x = x1 + x2 + x3 exactly, every term a bf16: x1 rounded to nearest even, x2 and x3 by truncation (x3 is exact: 24 - 16 bits are
left).  A product keeps its six partial products of weight <= 2,
    a b ~ a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a3 b1 + a2 b2),
each exact in fp32; here they are accumulated in float64, which leaves the floor of the three dropped products."""
import numpy as np

F32 = np.float32
PAIRS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # smallest weight first, as the kernels issue them


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def bf16_nearest(x):
    u = _bits(x).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(F32)


def bf16_trunc(x):
    return (_bits(x) & np.uint32(0xffff0000)).view(F32)


def is_bf16(x):
    return bool(np.all((_bits(x) & np.uint32(0xffff)) == 0))


def split3(x):
    """(x1, x2, x3), fp32 arrays holding bf16 values, x1 + x2 + x3 == x exactly (finite x)."""
    x = np.ascontiguousarray(x, F32)
    x1 = bf16_nearest(x)
    r = (x - x1).astype(F32)          # exact: at most 16 significant bits are left
    x2 = bf16_trunc(r)
    x3 = (r - x2).astype(F32)         # exact, and a bf16
    return x1, x2, x3


def split_matmul(a, b):
    """a @ b from the six kept partial products of the split operands, float64 accumulation."""
    sa = [t.astype(np.float64) for t in split3(a)]
    sb = [t.astype(np.float64) for t in split3(b)]
    out = np.zeros((a.shape[0], b.shape[1]), np.float64)
    for i, j in PAIRS:
        out += sa[i] @ sb[j]
    return out


def split_gram(f):
    """F F^T (no 1 / n) of f = [C][hw]."""
    return split_matmul(f, np.ascontiguousarray(f.T))


def rel_l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
