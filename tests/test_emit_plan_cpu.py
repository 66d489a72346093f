"""csrc/emit_plan.h (what the pass that hands an image out launches, books and refuses, for each of its five readers) compiled on its own,
under the address and undefined-behaviour sanitizers, into a stand-alone program (tests/emit_plan_host_main.cpp: the sanitizer runtime is
linked into it).  The program prints emit_resolve's plan for every combination of the facts; this file holds that output to TABLE.

TABLE was written from the call sites that emit_resolve replaced -- st_step, st_step_begin, st_tile_step and the two tile readers, each
with an if / else chain of its own over deprocess, average_enqueue, luma_enqueue and luma_staged -- one row per case those chains
distinguished, '*' where a chain did not look at a fact.  The rows are disjoint and cover all 360 combinations (checked below).

streams: for st_step, st_step_begin and st_tile_step the count is the one the ProfScope lines of those call sites booked (booked() below
restates them); the deprocess launch moves 2 (x in, the image out) and was booked with 0 bytes, which tests/golden/route_fingerprints.json
records for every step: book = 0 keeps that figure.  The tile readers' staged launches were not booked and are now: their rows count
what the launch moves (the packed tile in, the content's tile in under luminance, the image out)."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
READERS = ('step', 'begin', 'tile_step', 'tile_x', 'tile_average')
WANT, AVERAGING, LUMA = ('0', '1'), ('off', 'empty', 'items'), ('0', '1')
CONTENT, BUFFER = ('absent', 'other_size', 'fits'), ('ok', 'bad')
DOMAINS = (READERS, WANT, AVERAGING, LUMA, CONTENT, BUFFER)
ON = 'empty|items'
STATE = 2                                                       # ST_ERR_STATE

# reader        want  averaging  luminance  content       buffer   plan: source colour advance image streams book
TABLE = '''
step            0     off        *          *             *        nothing
step            0     empty      *          *             ok       mean_updated add_mean 1 0 2 1
step            0     items      *          *             ok       mean_updated add_mean 1 0 3 1
step            0     %(ON)s     *          *             bad      refuse average_buffer
step            1     off        0          *             *        x add_mean 0 1 2 0
step            1     empty      0          *             ok       mean_updated add_mean 1 1 3 1
step            1     items      0          *             ok       mean_updated add_mean 1 1 4 1
step            1     %(ON)s     0          *             bad      refuse average_buffer
step            1     *          1          absent        *        refuse no_content
step            1     *          1          other_size    *        refuse content_size
step            1     off        1          fits          *        x luma 0 1 3 1
step            1     empty      1          fits          ok       mean_updated luma 1 1 4 1
step            1     items      1          fits          ok       mean_updated luma 1 1 5 1
step            1     %(ON)s     1          fits          bad      refuse average_buffer
begin           *     off        0          *             *        x add_mean 0 1 2 0
begin           *     empty      0          *             ok       mean_updated add_mean 1 1 3 1
begin           *     items      0          *             ok       mean_updated add_mean 1 1 4 1
begin           *     %(ON)s     0          *             bad      refuse average_buffer
begin           *     *          1          absent        *        refuse no_content
begin           *     *          1          other_size    *        refuse content_size
begin           *     off        1          fits          *        x luma 0 1 3 1
begin           *     empty      1          fits          ok       mean_updated luma 1 1 4 1
begin           *     items      1          fits          ok       mean_updated luma 1 1 5 1
begin           *     %(ON)s     1          fits          bad      refuse average_buffer
tile_step       *     off        *          *             *        nothing
tile_step       *     empty      *          *             ok       mean_updated add_mean 1 0 2 1
tile_step       *     items      *          *             ok       mean_updated add_mean 1 0 3 1
tile_step       *     %(ON)s     *          *             bad      refuse average_buffer
tile_x          *     *          0          *             *        x add_mean 0 1 2 1
tile_x          *     *          1          absent        *        refuse no_content
tile_x          *     *          1          other_size    *        refuse content_size
tile_x          *     *          1          fits          *        x luma 0 1 3 1
tile_average    *     off        *          *             *        refuse average_off
tile_average    *     empty      *          *             *        refuse average_empty
tile_average    *     items      0          *             *        mean_read add_mean 0 1 2 1
tile_average    *     items      1          absent        *        refuse no_content
tile_average    *     items      1          other_size    *        refuse content_size
tile_average    *     items      1          fits          *        mean_read luma 0 1 3 1
''' % {'ON': ON}

# the corners of the table, as the program must print them
NAMED = ['step 0 items 1 absent ok -> mean_updated add_mean 1 0 3 1',          # luminance on, no image wanted, averaging: update only, no content needed
         'step 0 off 1 absent ok -> nothing',
         'begin 0 off 0 absent ok -> x add_mean 0 1 2 0',                       # st_step_begin always wants an image
         'tile_step 1 off 1 fits ok -> nothing',
         'tile_step 1 empty 1 absent ok -> mean_updated add_mean 1 0 2 1',
         'tile_x 0 items 0 absent bad -> x add_mean 0 1 2 1',
         'tile_average 0 items 1 fits bad -> mean_read luma 0 1 3 1',
         'begin 1 off 1 absent ok -> refuse 2 no_content',
         'tile_x 1 off 1 other_size ok -> refuse 2 content_size',
         'tile_average 1 off 0 fits ok -> refuse 2 average_off',
         'tile_average 1 empty 1 absent ok -> refuse 2 average_empty']


def expected():
    want = {}
    for line in TABLE.strip().splitlines():
        words = line.split()
        pattern, plan = words[:6], ' '.join(words[6:])
        if plan.startswith('refuse '):
            plan = 'refuse %d %s' % (STATE, plan.split()[1])
        choices = [dom if p == '*' else tuple(p.split('|')) for p, dom in zip(pattern, DOMAINS)]
        for combo, dom in zip(choices, DOMAINS):
            assert set(combo) <= set(dom), line
        for key in itertools.product(*choices):
            assert key not in want, ('two rows claim', key)
            want[key] = plan
    assert set(want) == set(itertools.product(*DOMAINS)) and len(want) == 360
    return want


def booked(key):
    """The streams the ProfScope lines of the replaced call sites counted (None: a launch they did not book)."""
    reader, want, averaging, luma, _, _ = key
    image = reader == 'begin' or (reader == 'step' and want == '1')
    first = averaging == 'empty'
    if reader in ('tile_x', 'tile_average'):
        return None
    if image and luma == '1':                                   # luma_enqueue: x and the content in, the image out; the mean out, and in unless empty
        return 3 + (0 if averaging == 'off' else 1 if first else 2)
    if averaging != 'off':                                      # average_enqueue: x in, mean in (unless empty) and out, the image
        return 2 + (0 if first else 1) + (1 if image else 0)
    return 2                                                    # the deprocess launch: x in, the image out


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
    exe = str(tmp_path_factory.mktemp('emit_plan') / 'emit_plan_host')
    build = subprocess.run([cxx, '-std=c++17', '-g', '-O1', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                            os.path.join(HERE, 'emit_plan_host_main.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout.splitlines()


def test_every_combination_resolves_to_the_row_of_the_replaced_call_sites(output):
    want = expected()
    assert len(output) == len(want)
    seen = set()
    for line in output:
        facts, plan = line.split(' -> ')
        key = tuple(facts.split())
        assert key in want and key not in seen, line
        seen.add(key)
        assert plan == want[key], (line, want[key])
    for line in NAMED:
        assert line in output, line


def test_streams_are_those_the_replaced_call_sites_booked(output):
    checked = 0
    for line in output:
        facts, plan = line.split(' -> ')
        key, words = tuple(facts.split()), plan.split()
        if words[0] in ('nothing', 'refuse'):
            continue
        count = booked(key)
        if count is None:                                       # the tile readers: what the staged launch moves
            count = 3 if words[1] == 'luma' else 2
        assert int(words[4]) == count, (line, count)
        if words[:2] == ['x', 'add_mean']:
            assert int(words[4]) == 2
        assert words[5] == ('0' if words[:2] == ['x', 'add_mean'] and key[0] in ('step', 'begin') else '1'), line
        checked += 1
    assert checked > 100
