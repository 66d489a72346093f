"""csrc/jitter_plan.h (validation of the radius, the shift sequence, the reduction of a shift, the source index of a rolled pixel and the
launch grids of roll_k) compiled on its own, under the address and undefined-behaviour sanitizers, into a stand-alone program
(tests/jitter_plan_host_main.cpp: the sanitizer runtime is linked into it).  The program prints every validation case, the shifts of
1 000 consecutive steps for three seeds and five radii, and, for every H and W from 1 to 40 and six shifts, a walk of roll_k's loops over
the planned grid with the header's source-index function; this file holds the output to the Python generator and to np.roll."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jitter_oracle as jo

HERE = os.path.dirname(os.path.abspath(__file__))
OK, RADIUS = 'ok', 'the radius must be 0 (off) or inside [1, 4096]'
VALIDATE = {-2 ** 31: RADIUS, -1: RADIUS, 0: OK, 1: OK, 3: OK, 4096: OK, 4097: RADIUS, 2 ** 31 - 1: RADIUS}
SEEDS, RADII = (0, 7, jo.MASK64), (1, 3, 16, 1024, 4096)


def _clangxx():
    for path in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++'), '/opt/rocm/lib/llvm/bin/clang++'):
        if os.path.exists(path):
            return path
    return shutil.which('amdclang++')


@pytest.fixture(scope='module')
def output(tmp_path_factory):
    cxx = _clangxx()
    if not cxx:
        pytest.skip('no ROCm clang++ on this machine')
    exe = str(tmp_path_factory.mktemp('jitter_plan') / 'jitter_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'jitter_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def pairs(output, tag):
    return [tuple(part.split() for part in line[len(tag) + 1:].split(' -> ')) for line in output if line.startswith(tag + ' ')]


def test_every_validation_case(output):
    got = {int(k[0]): ' '.join(v) for k, v in pairs(output, 'validate')}
    assert got == VALIDATE


def test_the_published_splitmix64_vectors(output):
    got = {(int(k[0]), int(k[1])): int(v[0]) for k, v in pairs(output, 'draw')}
    assert got == {(1234567, k): r for k, r in enumerate(jo.DRAWS_1234567)}


def test_shifts_are_the_python_generators_and_inside_the_radius(output):
    got = {(int(k[0]), int(k[1]), int(k[2])): (int(v[0]), int(v[1])) for k, v in pairs(output, 'shift')}
    assert len(got) == len(SEEDS) * len(RADII) * 1000 + 1
    for (seed, radius, k), s in got.items():
        assert s == jo.shift(seed, k, radius), (seed, radius, k)
        assert -radius <= s[0] <= radius and -radius <= s[1] <= radius
    assert {(seed, radius) for seed, radius, _ in got} == {(seed, radius) for seed in SEEDS for radius in RADII}
    for (seed, radius), want in jo.PINS.items():
        assert [got[(seed, radius, k)] for k in range(len(want))] == want
    assert (jo.MASK64, 4096, jo.MASK64 - 1) in got                          # a counter at which the multiplication wraps
    # every value of a small radius turns up on both axes: the sequence is not stuck
    assert {got[(7, 1, k)][0] for k in range(1000)} == {-1, 0, 1} == {got[(7, 1, k)][1] for k in range(1000)}


def test_reduction_is_pythons_modulus(output):
    got = pairs(output, 'reduce')
    assert len(got) == 13 * 5
    for (d, n), (r,) in got:
        assert int(r) == int(d) % int(n), (d, n, r)


def test_walk_of_the_planned_grid_is_a_permutation_and_equals_numpy_roll(output):
    rolls = pairs(output, 'roll')
    seen = set()
    weights = {}
    for (H, W, dy, dx), (rdy, rdx, form, once, total) in rolls:
        H, W, dy, dx = int(H), int(W), int(dy), int(dx)
        assert (int(rdy), int(rdx)) == (dy % H, dx % W)
        assert int(once) == 1, (H, W, dy, dx, form)                         # every element written once, every source read once
        n = 3 * H * W
        if n not in weights:
            weights[n] = np.arange(1, n + 1, dtype=np.uint64)
        want = np.roll(np.arange(n, dtype=np.uint64).reshape(3, H, W), (dy, dx), (1, 2)).reshape(-1)
        assert int((want * weights[n]).sum(dtype=np.uint64)) == int(total), (H, W, dy, dx, form)
        seen.add((H, W, dy, dx, int(form)))
    for H in range(1, 41):
        for W in range(1, 41):
            for s in ((0, 0), (1, 0), (0, -1), (-3, 2), (H, W), (-40, 300)):
                assert (H, W) + s + (0,) in seen
                assert ((H, W) + s + (1,) in seen) == (W % 4 == 0)          # the 16-byte form where a group of four stays inside a row
    assert (1000, 4, 999, 3, 1) in seen and (333, 5, -1, -1, 0) in seen


def test_plans_refuse_empty_images_and_large_ones_stay_inside_the_grid_caps(output):
    assert 'plan_refused' in output
    # rows, gx, gy, gx_vec, gy_vec, pixels: 8192^2 in one trip per thread; a taller image through the row loop of a capped grid
    assert [line for line in output if line.startswith('big ')] == ['big 24576 128 1536 32 1536 201326592', 'big 1200000 625 65535 157 65535 48000000000']
