#!/usr/bin/env python3
"""Generates tests/golden/iterate_average.npz by RUNNING THE REFERENCE's ``utils.DecayingMean`` (utils.py:49-69), imported unmodified
from /root/reference as make_golden.py imports it, on seeded float32 sequences.

Run once, in the build container (``python tests/golden/make_iterate_average.py``); the fixture is committed, this script stays as
its provenance.  Per decay d in DECAYS: 6 float32 arrays of shape (3, 5, 7), values ~ N(0, 1) * 50 with one element exactly 0.0 and
one -0.0 in every array; after every item the raw mean (``DecayingMean.mean``) and the corrected value (what the call returns).
Keys: ``decays`` (float64), ``items_<k>`` (6, 3, 5, 7), ``mean_<k>`` and ``corrected_<k>`` (6, 3, 5, 7), k the index into decays.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
sys.dont_write_bytecode = True

sys.path.insert(0, REF)
import utils as ref_utils                # noqa: E402
sys.path.remove(REF)

F32 = np.float32
DECAYS = (0.9, 0.5, 0.999)
N_ITEMS, SHAPE = 6, (3, 5, 7)


def sequence(seed):
    rng = np.random.RandomState(seed)
    items = (rng.randn(N_ITEMS, *SHAPE) * 50).astype(F32)
    for i in range(N_ITEMS):                       # one exact zero and one negative zero per array, at moving places
        items[i].flat[(7 * i + 3) % items[i].size] = F32(0.0)
        items[i].flat[(11 * i + 40) % items[i].size] = F32(-0.0)
    return items


def main():
    out = {'decays': np.array(DECAYS, np.float64)}
    for k, d in enumerate(DECAYS):
        items = sequence(100 + k)
        dm = ref_utils.DecayingMean(decay=d)
        means, corrected = [], []
        for item in items:
            value = dm(item)
            assert dm.mean.dtype == F32 and value.dtype == F32, (dm.mean.dtype, value.dtype)
            means.append(dm.mean.copy())
            corrected.append(value.copy())
        out['items_%d' % k] = items
        out['mean_%d' % k] = np.stack(means)
        out['corrected_%d' % k] = np.stack(corrected)
    np.savez_compressed(os.path.join(HERE, 'iterate_average.npz'), **out)
    print('wrote iterate_average.npz', sorted(out))


if __name__ == '__main__':
    main()
