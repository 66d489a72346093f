"""The call-sequence walks of tests/test_gpu_call_sequences.py, checked where no GPU is needed: what they cover, and that the
images they feed are far enough apart for an answer from an earlier state to miss every bar by orders of magnitude."""

import itertools

import numpy as np
import pytest

import sequence_oracle as so


def test_single_walks_follow_every_preparer_by_every_hook_on_every_path():
    """Each case's first walk runs every preparer once (Runner.run calls every hook of HOOKS after each step), and the cases cover
    every path on both nets and all three sizes -- conv algorithm 2 where the split kernel takes a layer."""
    cases = so.cases()
    for i, case in enumerate(cases):
        steps = so.walk('single', i)
        assert sorted(p for step in steps for p in step) == sorted(so.PREPARERS), case
        assert all(len(step) == 1 for step in steps)
    assert {c[:2] for c in cases} == set(so.PATHS)
    for path in so.PATHS:
        jobs = {c[2:] for c in cases if c[:2] == path}
        assert jobs == set(so.JOBS) if path[1] != 2 else jobs == {j for j in so.JOBS if so.split_layers(*j)}, path
    assert set(so.HOOKS) == {'get_blob', 'gram', 'backward', 'opfunc'}
    # which layers conv algorithm 2 takes: conv1_2 and conv4_1 of net A at 20 x 28 (widths 28 and 4), nothing at 33 x 65 (odd widths), three of net B
    assert so.split_layers('A', 20, 28) == ['conv1_2', 'conv4_1']
    assert so.split_layers('A', 33, 65) == []
    assert so.split_layers('B', 24, 40) == ['conv1_2', 'conv2_1', 'conv2_2']


def test_pair_walks_cover_every_ordered_pair_of_preparers():
    pairs = collections_counter()
    for i in range(len(so.cases())):
        steps = so.walk('pairs', i)
        assert steps and all(len(s) == 2 and s[0] != s[1] for s in steps)
        pairs.update(steps)
    want = {(p, q) for p in so.PREPARERS for q in so.PREPARERS if p != q}
    assert set(pairs) == want and all(v == 1 for v in pairs.values())


def collections_counter():
    import collections
    return collections.Counter()


def test_walks_are_deterministic_and_ids_name_path_net_and_walk():
    for i, case in enumerate(so.cases()):
        for kind in ('single', 'pairs'):
            assert so.walk(kind, i) == so.walk(kind, i)
            cid = so.case_id(case, kind)
            assert case[0] in cid and 'net' + case[2] in cid and kind in cid
    ids = [so.case_id(c, k) for c in so.cases() for k in ('single', 'pairs')]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize('net,h,w', list(so.JOBS) + [(n,) + so.other_size(h, w) for n, h, w in so.JOBS],
                         ids=lambda v: str(v))
def test_any_two_pool_images_are_separated_in_every_blob_gram_and_backward(net, h, w):
    """The Runner takes a new image of the pool for every evaluation (cyclically) and asserts the separation of successive ones
    itself; here it is shown for every pair of the pool, at the job's size and at the size resample_input moves to."""
    cpu = so.net_oracle(net)
    snaps = [so.snapshot(cpu, net, h, w, cpu.preprocess(so.image(k, h, w))) for k in range(so.N_IMAGES)]
    worst = min(so.sym_sep(a[key], b[key]) for a, b in itertools.combinations(snaps, 2) for key in a)
    print('smallest separation %.3g' % worst)
    for (i, a), (j, b) in itertools.combinations(enumerate(snaps), 2):
        so.assert_separated(a, b, 'images %d and %d of net %s at %d x %d' % (i, j, net, h, w))
