"""csrc/matting_plan.h (validation, window counts, buffer offsets, tiles and grids of the photorealism term) compiled on its own, under the
address and undefined-behaviour sanitizers, into a stand-alone program (tests/matting_plan_host_main.cpp: the sanitizer runtime is linked
into it).  The program prints every validation refusal and, for 3 x 3, 3 x 300, 37 x 50, the sizes one cell past a tile, a size with
more tiles than workgroups and 8192 x 8192, the plan with a walk of both passes' tile loops; this file holds the output to the
definition in st2.h."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, WEIGHT, EPS = 'ok', 'the weight must be finite, and zero (off) or non-zero as a double and as a float', 'eps must lie in [1e-9, 1]'
SIZE = 'the image must be at least 3 x 3: a window is a 3 x 3 block that lies wholly inside it'
VALIDATE = {'on': OK, 'negative': OK, 'off': OK, 'off_negative_zero': OK, 'eps_low_end': OK, 'eps_high_end': OK,
            'weight_nan': WEIGHT, 'weight_inf': WEIGHT, 'weight_negative_inf': WEIGHT, 'weight_underflows_float': WEIGHT, 'weight_overflows_float': WEIGHT,
            'eps_zero': EPS, 'eps_below': EPS, 'eps_above': EPS, 'eps_negative': EPS, 'eps_nan': EPS, 'eps_inf': EPS, 'weight_before_eps': WEIGHT}
TW, TH, CAP = 64, 4, 1024
SIZES = [(3, 3), (3, 300), (37, 50), (TH + 3, TW + 3), (TH + 1, TW + 1), (300, 1030), (8192, 8192)]


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
    exe = str(tmp_path_factory.mktemp('matting_plan') / 'matting_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'matting_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def test_every_validation_case(output):
    got = dict(line[len('validate '):].split(' -> ') for line in output if line.startswith('validate '))
    assert got == VALIDATE
    assert 'plan_off -> ' + WEIGHT in output                              # (a plan is of a term that is on)
    assert 'plan 2 9 -> refused: ' + SIZE in output and 'plan 9 2 -> refused: ' + SIZE in output


def test_offsets_tiles_and_grids_and_every_cell_once_inside_the_planned_buffers(output):
    plans = dict(line[len('plan '):].split(' -> ') for line in output if line.startswith('plan ') and 'refused' not in line)
    assert sorted(plans) == sorted('%d %d' % s for s in SIZES)
    for H, W in SIZES:
        hw, ww = H - 2, W - 2
        n = hw * ww
        fy, fx, ay, ax = -(-hw // TH), -(-ww // TW), -(-H // TH), -(-W // TW)
        want = [[hw, ww, H * W, 3 * H * W, n], [0, 3 * n, 9 * n, 21 * n], [fy, fx, fy * fx, min(fy * fx, CAP)], [ay, ax, ay * ax, min(ay * ax, CAP)],
                [n, H * W, 0],                                            # windows and pixels visited, none twice or outside
                [21 * n - 1, 3 * H * W - 1]]                              # the last float of each buffer is the last one touched
        got = [list(map(int, part.split())) for part in plans['%d %d' % (H, W)].split(' | ')]
        assert got == want, (H, W)
    big = 8190 * 8190
    assert 21 * big * 4 > 2 ** 32 and 3 * 8192 * 8192 * 4 < 2 ** 32      # (the per-window buffer of the 8192^2 job is past 32-bit byte offsets)


def test_constants_and_lds(output):
    assert 'constants %d %d 256 %d %d %d 2' % (TW, TH, TW + 2, TH + 2, CAP) in output
    assert 'lds %d %d' % (4 * 6 * (TH + 2) * (TW + 2), 4 * 15 * (TH + 2) * (TW + 2)) in output      # 9.3 and 23.2 KiB of the 160 KiB of a CU
