"""The photorealism term (include/st2.h: st_set_matting): the text form ``W`` or ``W:EPS`` (worker config key ``matting``,
``tools/stylize.py --matting``) and the checks of st_set_matting.  No device, no library: plain parsing."""
import math

import numpy as np

EPS_MIN, EPS_MAX, EPS_DEFAULT = 1e-9, 1.0, 1e-7


def check_matting(weight, eps=EPS_DEFAULT):
    """(weight, eps) as st_set_matting takes them, or ValueError: weight finite, and zero (off) or non-zero as a float32 too; eps in
    [1e-9, 1]."""
    try:
        weight, eps = float(weight), float(eps)
    except (TypeError, ValueError):
        raise ValueError('weight and eps are numbers, not %r and %r' % (weight, eps)) from None
    with np.errstate(over='ignore', under='ignore'):
        w32 = float(np.float32(weight))
    if not math.isfinite(weight) or (weight != 0.0 and (w32 == 0.0 or not math.isfinite(w32))):
        raise ValueError('weight %r is not finite, or not a non-zero float32' % weight)
    if not EPS_MIN <= eps <= EPS_MAX:
        raise ValueError('eps %r is outside [1e-9, 1]' % eps)
    return weight, eps


def parse_matting(text):
    """'10000' -> (10000.0, 1e-7); '10000:1e-5' -> (10000.0, 1e-5); '0' or 'off' -> (0.0, 1e-7) (off).  ValueError on anything else."""
    text = str(text).strip()
    if text.lower() in ('0', 'off'):
        return 0.0, EPS_DEFAULT
    weight, sep, eps = text.partition(':')
    try:
        weight = float(weight.strip())
        eps = float(eps.strip()) if sep else EPS_DEFAULT
    except ValueError:
        raise ValueError('%r is not W or W:EPS' % text) from None
    return check_matting(weight, eps)


def matting_arg(value):
    """run_job's ``matting`` argument -> (weight, eps): a (weight, eps) pair, a weight alone, or False / 0 for off."""
    if value is False or value is None:
        return 0.0, EPS_DEFAULT
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError('matting: (weight, eps), a weight or False, got %r' % (value,))
        return check_matting(*value)
    return check_matting(value)
