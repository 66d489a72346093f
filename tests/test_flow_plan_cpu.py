"""csrc/flow_plan.h (validation of the optical-flow parameters and images, the level geometry, the layout of the block's scratch buffer,
the launch grids and the bound of the single-workgroup Jacobi route) compiled on its own, under the address and undefined-behaviour
sanitizers, into a stand-alone program (tests/flow_plan_host_main.cpp: the sanitizer runtime is linked into it).  This file holds the
program's output to the definition in st2.h and to a restatement of the layout."""
import os
import shutil
import subprocess

import pytest

import flow_oracle as fo

HERE = os.path.dirname(os.path.abspath(__file__))
OK = 'ok'
LEVELS, WARPS, ITERS = 'levels must be between 0 (automatic) and 12', 'warps must be between 1 and 16', 'iters must be between 1 and 1000'
ALPHA, ROUTE = 'alpha must be finite and between 1e-6 and 1e3', 'route must be 0 (automatic) or 1 (one launch per iteration)'
IMAGE, SIZE, VALUE = 'both images and the output are required', 'the images must be at least 1 x 1', 'every value of a float32 image must be finite'
PARAMS = {'defaults': OK, 'levels_-1': LEVELS, 'levels_12': OK, 'levels_13': LEVELS, 'warps_0': WARPS, 'warps_16': OK, 'warps_17': WARPS,
          'iters_0': ITERS, 'iters_1000': OK, 'iters_1001': ITERS, 'alpha_nan': ALPHA, 'alpha_inf': ALPHA, 'alpha_low': ALPHA, 'alpha_1e-6': OK,
          'alpha_1e3': OK, 'alpha_high': ALPHA, 'alpha_negative': ALPHA, 'route_1': OK, 'route_2': ROUTE, 'route_-1': ROUTE}
IMAGES = {'null': IMAGE, 'u8': OK, 'finite': OK, 'height_zero': SIZE, 'width_negative': SIZE, 'nan_last': VALUE, 'negative_inf_last': VALUE,
          'inf_first': VALUE}
SIZES = [(1, 1), (1, 9), (7, 1), (2, 2), (5, 3), (16, 16), (31, 33), (32, 32), (33, 47), (64, 64), (65, 64), (63, 100), (96, 128), (130, 70),
         (32, 128), (41, 100), (512, 512), (1024, 1024), (1080, 1920)]
CAP, WG_PIXELS = 4096, 4096


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
    exe = str(tmp_path_factory.mktemp('flow_plan') / 'flow_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'flow_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    return run.stdout.splitlines()


def table(output, prefix):
    return dict(line[len(prefix):].split(' -> ') for line in output if line.startswith(prefix))


def align4(n):
    return (n + 3) // 4 * 4


def grid(n, per_block, cap):
    return max(1, min(-(-n // per_block), cap))


def total_floats(sizes, is_u8):
    n0 = sizes[0][0] * sizes[0][1]
    stage = align4(-(-(3 * n0 * (1 if is_u8 else 4)) // 4))
    return sum(6 * align4(h * w) for h, w in sizes) + 6 * align4(n0) + align4(2 * n0) + 2 * stage


def test_parameter_and_image_validation(output):
    assert table(output, 'params ') == PARAMS
    assert table(output, 'image ') == IMAGES
    assert 'defaults 0 3 40 0.059999999999999998 0' in output
    assert 'plan_refused' in output


def test_level_geometry_follows_the_pooling_rule(output):
    levels = table(output, 'levels ')
    assert len(levels) == len(SIZES) * 5
    for h, w in SIZES:
        for asked in (0, 1, 2, 5, 12):
            want = fo.level_sizes(h, w, asked)
            assert levels['%d %d %d' % (h, w, asked)] == ' '.join([str(len(want))] + ['%dx%d' % s for s in want]), (h, w, asked)


def test_scratch_regions_neither_overlap_nor_exceed_the_total_and_the_walks_cover_every_level(output):
    plans = table(output, 'plan ')
    assert len(plans) == len(SIZES) * 4
    for h, w in SIZES:
        sizes = fo.level_sizes(h, w)
        for is_u8 in (0, 1):
            for route in (0, 1):
                n, total, layout_ok, walk_ok, one_wg, launches = plans['%d %d %d %d' % (h, w, is_u8, route)].split()
                assert (int(n), int(total), layout_ok, walk_ok) == (len(sizes), total_floats(sizes, is_u8), '1', '1'), (h, w, is_u8, route)
                want_wg = [route == 0 and lh * lw <= WG_PIXELS for lh, lw in sizes]
                assert one_wg == ''.join('1' if f else '0' for f in want_wg)
                # luma, pools, smooths, interleave; per level its start and per warp the linearisation and the Jacobi launches
                assert int(launches) == 1 + (len(sizes) - 1) + len(sizes) + 1 + sum(1 + 3 * (1 + (1 if f else 40)) for f in want_wg)
    assert 'small_ok' in output


def test_the_single_workgroup_bound_is_4096_pixels_of_any_shape(output):
    assert table(output, 'bound ') == {'64 64': '1', '1 4096': '1', '4096 1': '1', '1 4097': '0', '4097 1': '0', '64 65': '0'}


def test_large_plans_do_not_wrap(output):
    big = table(output, 'big ')
    for (h, w), is_u8 in (((8192, 8192), 0), ((70000, 70000), 1)):
        sizes = fo.level_sizes(h, w)
        assert big['%d %d' % (h, w)] == '%d %d %d %d' % (len(sizes), total_floats(sizes, is_u8), grid(h * w, 256, CAP), grid(h * w // 4, 256, CAP))
    assert 70000 * 70000 > 2 ** 32
