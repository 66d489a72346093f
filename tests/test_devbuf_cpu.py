"""csrc/devbuf.h (the one owner type of the engine's device and pinned buffers) on the host, under the address and undefined-behaviour
sanitizers: tests/devbuf_host_main.cpp puts the header's allocation funnel over malloc / free and checks moves, reserve / alloc, failed
allocations, the minimum sizes and containers of buffers.  A stand-alone program: the sanitizer runtime is linked into it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _clangxx():
    for path in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++'), '/opt/rocm/lib/llvm/bin/clang++'):
        if os.path.exists(path):
            return path
    return shutil.which('amdclang++')


def test_devbuf_header_under_host_sanitizers(tmp_path):
    cxx = _clangxx()
    if not cxx:
        pytest.skip('no ROCm clang++ on this machine')
    exe = str(tmp_path / 'devbuf_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'devbuf_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'all checks passed' in run.stdout
