"""csrc/frames_plan.h (validation of the depth, the frame index and the flows, and the launch grids of the frame-sequence launch) compiled
on its own, under the address and undefined-behaviour sanitizers, into a stand-alone program (tests/frames_plan_host_main.cpp: the
sanitizer runtime is linked into it).  The program prints every validation case, the plan of every H and W from 1 to 70 with a walk of
the launch's grid-stride loop over a buffer of exactly the planned size, and two large sizes; this file holds the output to the
definition in st2.h."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
OK, DEPTH, INDEX = 'ok', 'the depth must be between 0 and 8', 'the frame index must be between 1 and the depth'
SIZE, FLOW = 'the image must be at least 1 x 1', 'every value of a flow must be finite'
FLOWS = {'none': OK, 'finite': OK, 'negative_zero': OK, 'nan_last': FLOW, 'inf_last': FLOW, 'negative_inf_last': FLOW, 'height_zero': SIZE,
         'width_negative': SIZE, 'nan_first': FLOW}
CAP = 4096


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
    exe = str(tmp_path_factory.mktemp('frames_plan') / 'frames_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'frames_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def grid(n, per_block, cap):
    return max(1, min(-(-n // per_block), cap))


def test_depth_index_and_flow_validation(output):
    depth = dict(line[len('depth '):].split(' -> ') for line in output if line.startswith('depth '))
    assert depth == {str(d): OK if 0 <= d <= 8 else DEPTH for d in range(-1, 10)}
    index = dict(line[len('index '):].split(' -> ') for line in output if line.startswith('index '))
    assert index == {'0 8': INDEX, '1 8': OK, '8 8': OK, '9 8': INDEX, '-1 8': INDEX, '1 1': OK, '2 1': INDEX, '1 0': INDEX}
    flows = dict(line[len('flow '):].split(' -> ') for line in output if line.startswith('flow '))
    assert flows == FLOWS


def test_grids_from_1_to_70_cover_every_pixel_once_inside_the_planned_buffer(output):
    plans = [line for line in output if line.startswith('plan ')]
    assert len(plans) == 70 * 70
    seen = set()
    for line in plans:
        key, val = line[len('plan '):].split(' -> ')
        H, W = map(int, key.split())
        seen.add((H, W))
        want = [H * W, 3 * H * W, int(W % 4 == 0), grid(H * W, 256, CAP), grid(H * W // 4, 256, CAP), 1]
        assert list(map(int, val.split())) == want, line
    assert seen == {(H, W) for H in range(1, 71) for W in range(1, 71)}
    assert 'plan_refused' in output


def test_an_8192_square_plan_does_not_wrap(output):
    plane = 8192 * 8192
    assert [line for line in output if line.startswith('big ')] == ['big %d %d %d %d %d' % (plane, 3 * plane, CAP, CAP, 3 * plane - 1)]
    assert 70000 * 70000 > 2 ** 32                          # (a pixel count past 32 bits: the sizes are size_t throughout)
    assert [line for line in output if line.startswith('huge ')] == ['huge %d %d %d %d' % (70000 * 70000, 3 * 70000 * 70000, CAP, CAP)]
