"""csrc/color_match.h (the host side of linear colour transfer: 3 x 3 Cholesky, triangular solve, A and b) compiled on its own, under the
address and undefined-behaviour sanitizers, into a stand-alone program (tests/color_match_host_main.cpp: the sanitizer runtime is linked
into it).  pytest writes the colour moments of the four kinds of image pair to it and reads A, b back as hex floats: they equal float32
of the float64 oracle (tests/color_oracle.py) to within 1 ulp of fp32 -- double round-off times a condition number of 3e5 at most is far
below 2^-24.  The program exercises the header's error returns itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import color_oracle as co

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def _clangxx():
    for path in (os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin', 'clang++'), '/opt/rocm/lib/llvm/bin/clang++'):
        if os.path.exists(path):
            return path
    return shutil.which('amdclang++')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = _clangxx()
    if not cxx:
        pytest.skip('no ROCm clang++ on this machine')
    exe = str(tmp_path_factory.mktemp('color_match') / 'color_match_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'color_match_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def _line(mc, cc, ms, cs):
    upper = lambda c: [c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]]
    return ' '.join(float(v).hex() for v in list(mc) + upper(cc) + list(ms) + upper(cs))


def test_header_under_host_sanitizers_equals_the_oracle(program):
    cases, lines = [], []
    pairs = co.image_pairs()
    for kind in sorted(pairs):
        content, style = pairs[kind]
        (mc, cc), (ms, cs) = co.moments(co.preprocess(content)), co.moments(co.preprocess(style))
        cases.append((kind, co.transform(mc, cc, ms, cs)))
        lines.append(_line(mc, cc, ms, cs))
    lines.append('1 2 3')                                  # a short line is answered, not crashed on
    lines.append(_line(mc, cc, ms, -cs))                   # negative diagonal
    run = subprocess.run([program], input='\n'.join(lines) + '\n', capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    out = run.stdout.splitlines()
    assert out[0] == 'all checks passed' and len(out) == 1 + len(lines)
    for (kind, (wa, wb)), answer in zip(cases, out[1:]):
        words = answer.split()
        assert words[0] == 'ok' and len(words) == 13, (kind, answer)
        vals = np.array([float.fromhex(w) for w in words[1:]])
        assert np.array_equal(vals, vals.astype(F32))      # fp32 values
        A, b = vals[:9].astype(F32).reshape(3, 3), vals[9:].astype(F32)
        ua, ub = co.ulps(A, wa), co.ulps(b, wb)
        print('[%s] A within %g ulp, b within %g ulp of float32(oracle)' % (kind, ua, ub))
        assert ua <= 1 and ub <= 1, (kind, ua, ub)
    assert out[-2].startswith('err expected 18 numbers') and out[-1].startswith('err') and 'negative diagonal' in out[-1]
