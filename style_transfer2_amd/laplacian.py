"""The text form of the Laplacian term's levels, ``4:W,16:W``: pool size, colon, weight, comma-separated (worker config key
``laplacian``, ``tools/stylize.py --laplacian``).  No device, no library: plain parsing and the checks of st_set_laplacian."""
import math

POOLS = (1, 2, 4, 8, 16, 32)
MAX_LEVELS = 3


def check_levels(levels):
    """[(pool, weight)] as st_set_laplacian takes it, or ValueError: at most three levels, pool sizes distinct and from POOLS,
    weights finite and non-zero."""
    levels = [(int(p), float(w)) for p, w in levels]
    if len(levels) > MAX_LEVELS:
        raise ValueError('at most %d levels, not %d' % (MAX_LEVELS, len(levels)))
    for p, w in levels:
        if p not in POOLS:
            raise ValueError('pool size %d is not one of %s' % (p, ', '.join(map(str, POOLS))))
        if not math.isfinite(w) or w == 0:
            raise ValueError('weight %r of pool size %d is not a finite non-zero number' % (w, p))
    if len({p for p, _ in levels}) != len(levels):
        raise ValueError('two levels have the same pool size')
    return levels


def parse_levels(text):
    """'4:100,16:100' -> [(4, 100.0), (16, 100.0)]; '' or '0' or 'off' -> [] (off).  ValueError on anything else."""
    text = str(text).strip()
    if text.lower() in ('', '0', 'off'):
        return []
    levels = []
    for item in text.split(','):
        pool, sep, weight = item.partition(':')
        if not sep:
            raise ValueError('%r is not POOL:WEIGHT' % item.strip())
        try:
            levels.append((int(pool.strip()), float(weight.strip())))
        except ValueError:
            raise ValueError('%r is not POOL:WEIGHT' % item.strip()) from None
    return check_levels(levels)
