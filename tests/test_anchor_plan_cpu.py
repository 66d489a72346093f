"""csrc/anchor_plan.h (validation of the weight, the size and the map, and the launch grids of the anchor term) compiled on its own, under
the address and undefined-behaviour sanitizers, into a stand-alone program (tests/anchor_plan_host_main.cpp: the sanitizer runtime is
linked into it).  The program prints every validation refusal, the plan of every H and W from 1 to 70 with a walk of the launch's
grid-stride loop over a buffer of exactly the planned size, and one large size; this file holds the output to the definition in st2.h."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, WEIGHT = 'ok', 'the weight must be finite and non-zero, as a double and as a float'
SIZE, MAP = 'the image must be at least 1 x 1', 'every value of the map must be finite and not negative'
VALIDATE = {'no_map': OK, 'map': OK, 'map_with_zero_and_large': OK, 'map_negative_zero': OK,
            'weight_zero': WEIGHT, 'weight_negative_zero': WEIGHT, 'weight_nan': WEIGHT, 'weight_inf': WEIGHT, 'weight_negative_inf': WEIGHT,
            'weight_underflows_float': WEIGHT, 'weight_overflows_float': WEIGHT, 'height_zero': SIZE, 'width_zero': SIZE, 'height_negative': SIZE,
            'map_negative': MAP, 'map_nan': MAP, 'map_inf': MAP, 'map_negative_inf': MAP, 'weight_before_map': WEIGHT}


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
    exe = str(tmp_path_factory.mktemp('anchor_plan') / 'anchor_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'anchor_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def grid(n, per_block, cap):
    return max(1, min(-(-n // per_block), cap))


def test_every_validation_case(output):
    got = dict(line[len('validate '):].split(' -> ') for line in output if line.startswith('validate '))
    assert got == VALIDATE


def test_grids_from_1_to_70_cover_every_pixel_once_inside_the_planned_buffer(output):
    plans = [line for line in output if line.startswith('plan ')]
    assert len(plans) == 70 * 70
    seen = set()
    for line in plans:
        key, val = line[len('plan '):].split(' -> ')
        H, W = map(int, key.split())
        seen.add((H, W))
        want = [H * W, 3 * H * W, int(W % 4 == 0), grid(H * W, 256, 1024), grid(H * W // 4, 256, 1024), 1]
        assert list(map(int, val.split())) == want, line
    assert seen == {(H, W) for H in range(1, 71) for W in range(1, 71)}
    assert 'plan_refused' in output
    assert [line for line in output if line.startswith('big ')] == ['big %d %d 1024 1024' % (40000 * 40000, 3 * 40000 * 40000)]
