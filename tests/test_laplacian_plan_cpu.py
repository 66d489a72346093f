"""csrc/laplacian_plan.h (level validation, cell counts, buffer offsets and launch grids of the Laplacian term) compiled on its own,
under the address and undefined-behaviour sanitizers, into a stand-alone program (tests/laplacian_plan_host_main.cpp: the sanitizer
runtime is linked into it).  The program prints the plan of every pool size at every H and W from 1 to 70, every validation refusal, and
walks the pooling pass's tiles over buffers of exactly the planned size; this file holds the output to the definition in st2.h."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
POOLS = (1, 2, 4, 8, 16, 32)
OK, COUNT, NULL = 'ok', 'between 0 and 3 levels', 'pool and weight arrays are required for one or more levels'
POOL, DUP, WEIGHT = 'a pool size must be one of 1, 2, 4, 8, 16, 32', 'two levels have the same pool size', 'a weight must be finite and non-zero'
VALIDATE = {'off': OK, 'one': OK, 'three': OK, 'every_pool_a': OK, 'every_pool_b': OK, 'negative_count': COUNT, 'four_levels': COUNT,
            'null_pool': NULL, 'null_weight': NULL, 'pool_0': POOL, 'pool_3': POOL, 'pool_64': POOL, 'pool_negative': POOL,
            'duplicate': DUP, 'duplicate_last': DUP, 'weight_zero': WEIGHT, 'weight_negative_zero': WEIGHT, 'weight_nan': WEIGHT,
            'weight_inf': WEIGHT, 'weight_negative_inf': WEIGHT, 'weight_underflows_float': WEIGHT, 'weight_overflows_float': WEIGHT}


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
    exe = str(tmp_path_factory.mktemp('laplacian_plan') / 'laplacian_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'laplacian_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def ceil_div(a, b):
    return -(-a // b)


def grid(n, per_block, cap):
    return max(1, min(ceil_div(n, per_block), cap))


def test_every_validation_case(output):
    got = dict(line[len('validate '):].split(' -> ') for line in output if line.startswith('validate '))
    assert got == VALIDATE


def test_geometry_of_every_pool_size_from_1_to_70(output):
    plans = [line for line in output if line.startswith('plan ')]
    assert len(plans) == len(POOLS) * 70 * 70
    seen = set()
    for line in plans:
        key, val = line[len('plan '):].split(' -> ')
        p, H, W = map(int, key.split())
        seen.add((p, H, W))
        hp, wp = ceil_div(H, p), ceil_div(W, p)
        cells = 3 * hp * wp
        want = [hp, wp, cells, 0, ceil_div(cells, 4) * 4, 3 * H * W, int(W % 4 == 0), ceil_div(H, 32), ceil_div(W, 64),
                grid(3 * ceil_div(H, 32) * ceil_div(W, 64), 1, 8192), grid(cells, 1024, 1024), grid(3 * H * W, 1024, 1024),
                grid(3 * H * W // 4, 256, 1024)]
        assert list(map(int, val.split())) == want, line
    assert seen == {(p, H, W) for p in POOLS for H in range(1, 71) for W in range(1, 71)}
    assert 'plan_size_refused' in output
    big = [line for line in output if line.startswith('big ')]
    assert big == ['big %d %d 8192 1024 1024 1024' % (3 * 10000 * 10000, 3 * 40000 * 40000)]


def test_tile_walk_covers_every_cell_once_inside_the_planned_buffers(output):
    walks = [line for line in output if line.startswith('walk ')]
    assert len(walks) == 4 * 70 * 70 and all(line.endswith(' ok') for line in walks)
    # offsets: the levels back to back in their given order, each rounded up to 4 floats
    for line in walks:
        key, val = line[len('walk '):].split(' -> ')
        pools, H, W = key.split()
        pools = [int(p) for p in pools.split(',') if int(p)]
        H, W = int(H), int(W)
        total, offs, _ = val.split()
        off, want = 0, []
        for p in pools:
            want.append(off)
            off += ceil_div(3 * ceil_div(H, p) * ceil_div(W, p), 4) * 4
        assert int(total) == off and [int(o) for o in offs.split(',')][:len(pools)] == want, line
