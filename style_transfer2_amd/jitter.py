"""Jitter (include/st2.h: st_set_jitter): the text form ``R`` or ``R:SEED`` (worker config key ``jitter``), the checks of
st_set_jitter, and the shift sequence itself.  No device, no library: plain integers."""

MAX_RADIUS = 4096
MASK64 = (1 << 64) - 1


def check_jitter(radius, seed=0):
    """(radius, seed) as st_set_jitter takes them, or ValueError: radius an integer in [0, 4096] (0: off), seed in [0, 2**64)."""
    if isinstance(radius, bool) or isinstance(seed, bool):
        raise ValueError('radius and seed are integers')
    try:
        if int(radius) != radius or int(seed) != seed:
            raise ValueError
    except (TypeError, ValueError, OverflowError):
        raise ValueError('radius and seed are integers, not %r and %r' % (radius, seed)) from None
    radius, seed = int(radius), int(seed)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError('radius %d is outside [0, %d]' % (radius, MAX_RADIUS))
    if not 0 <= seed <= MASK64:
        raise ValueError('seed %d does not fit 64 unsigned bits' % seed)
    return radius, seed


def parse_jitter(text):
    """'8' -> (8, 0); '8:1234' -> (8, 1234); '0' or 'off' -> (0, 0) (off).  ValueError on anything else."""
    text = str(text).strip()
    if text.lower() in ('0', 'off'):
        return 0, 0
    radius, sep, seed = text.partition(':')
    try:
        radius = int(radius.strip(), 10)
        seed = int(seed.strip(), 10) if sep else 0
    except ValueError:
        raise ValueError('%r is not R or R:SEED' % text) from None
    return check_jitter(radius, seed)


def mix(z):
    """splitmix64's output function on a 64-bit unsigned value."""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw(seed, k):
    """r_k: output k + 1 of splitmix64 started at `seed`."""
    return mix((seed + (k + 1) * 0x9E3779B97F4A7C15) & MASK64)


def shift(seed, k, radius):
    """(dy, dx) of optimizer step k, each inside [-radius, radius]."""
    r = draw(seed, k)
    span = 2 * radius + 1
    return int((r >> 32) % span) - radius, int((r & 0xFFFFFFFF) % span) - radius
