"""Optical flow (include/st2.h: st_flow_estimate): the parameter defaults, the text form ``key=value,key=value`` and the checks of
st_flow_estimate.  No device, no library: plain numbers."""

import math

DEFAULTS = {'alpha': 0.06, 'warps': 3, 'iters': 40, 'levels': 0, 'route': 0}
MAX_LEVELS = 12
AUTO_MIN_SIDE = 32          # levels = 0: a level is pooled while its shorter side is at least this
RANGES = {'levels': (0, MAX_LEVELS), 'warps': (1, 16), 'iters': (1, 1000), 'route': (0, 1)}
ALPHA_RANGE = (1e-6, 1e3)


def check_flow(**params):
    """The parameters as st_flow_estimate takes them (a dict with every key of DEFAULTS), or ValueError: levels an integer in [0, 12]
    (0: automatic), warps in [1, 16], iters in [1, 1000], route 0 or 1, alpha finite in [1e-6, 1e3]; an unknown key is refused."""
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise ValueError('unknown flow parameter(s) %s: the parameters are %s' % (', '.join(unknown), ', '.join(sorted(DEFAULTS))))
    out = dict(DEFAULTS)
    for key, value in params.items():
        if value is None:
            continue
        if key == 'alpha':
            if isinstance(value, bool):
                raise ValueError('alpha is a number, not %r' % (value,))
            try:
                alpha = float(value)
            except (TypeError, ValueError):
                raise ValueError('alpha is a number, not %r' % (value,)) from None
            if not math.isfinite(alpha) or not ALPHA_RANGE[0] <= alpha <= ALPHA_RANGE[1]:
                raise ValueError('alpha %r is outside [%g, %g]' % (value, ALPHA_RANGE[0], ALPHA_RANGE[1]))
            out[key] = alpha
            continue
        if isinstance(value, bool):
            raise ValueError('%s is an integer, not %r' % (key, value))
        try:
            if int(value) != value:
                raise ValueError
        except (TypeError, ValueError, OverflowError):
            raise ValueError('%s is an integer, not %r' % (key, value)) from None
        lo, hi = RANGES[key]
        if not lo <= int(value) <= hi:
            raise ValueError('%s %d is outside [%d, %d]' % (key, int(value), lo, hi))
        out[key] = int(value)
    return out


def parse_flow(text):
    """'' or 'default' -> the defaults; 'alpha=0.03,iters=60' -> those over the defaults.  ValueError on anything else."""
    text = str(text).strip()
    if text.lower() in ('', 'default'):
        return dict(DEFAULTS)
    given = {}
    for part in text.split(','):
        key, sep, value = part.partition('=')
        key, value = key.strip(), value.strip()
        if not sep or not key or not value:
            raise ValueError('%r is not key=value' % part.strip())
        if key in given:
            raise ValueError('%s is given twice' % key)
        try:
            given[key] = float(value) if key == 'alpha' else int(value, 10)
        except ValueError:
            raise ValueError('%s: %r is not a number' % (key, value)) from None
    return check_flow(**given)


def level_sizes(h, w, levels=0):
    """[(h, w), ...] of the pyramid st_flow_estimate builds over an h x w image: halved in Caffe's ceil mode while the shorter side is
    at least 32 and fewer than 12 levels exist (levels = 0), or levels - 1 times, stopping early at 1 x 1."""
    sizes = [(int(h), int(w))]
    while len(sizes) < MAX_LEVELS:
        h, w = sizes[-1]
        if (min(h, w) < AUTO_MIN_SIDE) if levels == 0 else (len(sizes) >= levels or (h, w) == (1, 1)):
            break
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes
