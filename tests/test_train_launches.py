"""What every entry point of the training C ABI launches, pinned on the CPU.  tests/native/train_launches.cpp includes the
product's cae_train.hip textually, with the HIP host calls replaced by recorders, is compiled for the host only (under
AddressSanitizer + UBSan) and linked WITHOUT the HIP runtime, so it runs anywhere and never opens a GPU.  Per case it
records every memset, launch (kernel by name, grid, block, dynamic LDS, every integer and every pointer's role of the
argument struct), failure text and return code; the FNV-1a hash of each case's lines is compared with
tests/golden/train_launches.json.  The golden was recorded with this same harness from cae_train.hip as it stood at commit
fc2c946, before its launch decisions moved onto one tap-list builder, one halo box and one LDS formula: a grid, an LDS
size or a tap that differs from that commit's shows here.  `<program> <case name>...` prints those cases' lines in full."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    cxx = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(cxx):
        pytest.skip('hipcc not available')
    csrc = os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc')
    obj, exe = str(tmp_path / 'train_launches.o'), str(tmp_path / 'train_launches')
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    cmd = [cxx, '--cuda-host-only', '-x', 'hip', '-std=c++17', '-O1', '-g', '-Wno-unused-command-line-argument']
    cmd += [f for s in san for f in ('-Xarch_host', s)]
    cmd += ['-I' + csrc, '-I' + os.path.join(ROOT, 'include'), '-c', os.path.join(ROOT, 'tests', 'native', 'train_launches.cpp'),
            '-o', obj]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    # the host object may name its (absent) device image: define that symbol at link, there is no HIP runtime to ask for it
    nm = subprocess.run(['nm', '-u', obj], check=True, capture_output=True, text=True).stdout
    defsym = ['-Wl,--defsym=%s=0' % line.split()[-1] for line in nm.splitlines() if '__hip_fatbin' in line]
    clang = os.path.join(os.path.dirname(os.path.realpath(cxx)), '..', 'llvm', 'bin', 'clang++')
    if not os.path.exists(clang):
        clang = '/opt/rocm/llvm/bin/clang++'
    subprocess.run([clang] + san + defsym + [obj, '-o', exe], check=True, capture_output=True, text=True)
    ldd = subprocess.run(['ldd', exe], check=True, capture_output=True, text=True).stdout
    assert 'amdhip' not in ldd and 'hsa-runtime' not in ldd, ldd
    return exe


def test_every_training_launch_matches_the_recorded_hashes(tmp_path):
    exe = _build(tmp_path)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0')
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = dict(line.split() for line in r.stdout.splitlines())
    with open(os.path.join(ROOT, 'tests', 'golden', 'train_launches.json')) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, f'{len(wrong)} cases launch something else than recorded: {wrong[:8]}'
