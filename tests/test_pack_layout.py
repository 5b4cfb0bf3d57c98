"""The weight packers (the product's cae_pack.cpp, unchanged) under AddressSanitizer + UBSan on the CPU: every packer over
a fixed shape list, the FNV-1a hash of each packed buffer against tests/golden/pack_layout.json.  The golden hashes were
recorded from the packers as they stood inside cae_api.hip before they moved onto one split-f16 writer (that commit's
functions compiled into the same harness), so a layout slip in the shared writer shows here, without a GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_layouts_match_the_recorded_hashes(tmp_path):
    # hipcc as a host compiler: the packers use _Float16, which older g++ does not have in C++
    cxx = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(cxx):
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'pack_layout')
    csrc = os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc')
    cmd = [cxx, '-x', 'c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-I' + csrc, os.path.join(ROOT, 'tests', 'native', 'pack_layout.cpp'), os.path.join(csrc, 'cae_pack.cpp'),
           '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0')
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = dict(line.split() for line in r.stdout.splitlines())
    with open(os.path.join(ROOT, 'tests', 'golden', 'pack_layout.json')) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f'{len(wrong)} packed layouts changed: {wrong[:8]}'
