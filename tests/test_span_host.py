"""The span partition of the plane histograms (csrc/cae_seg_span.hpp: roc_hist_kernel, score_hist_kernel,
tile_byte_hist_kernel) on the CPU: tests/native/span_partition.cpp walks it lane by lane, as the kernels do, over group
widths 4 and 16, every base offset, rows of 1..33 elements, every counted extent, 1..7 blocks and 1..64 lanes, and requires
every counted element exactly once with the right flag, aligned groups and nothing behind the limit.  It also requires
that the same checks call two wrong partitions wrong (no head at offset 1; singles from every block)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_counted_element_is_visited_once_and_wrong_partitions_are_seen(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(cxx):
        pytest.skip('no host compiler available')
    exe = str(tmp_path / 'span_partition')
    cmd = [cxx, '-x', 'c++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           '-I' + os.path.join(ROOT, 'cnn_autoencoder_amd', 'csrc'), os.path.join(ROOT, 'tests', 'native', 'span_partition.cpp'),
           '-o', exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    words = r.stdout.split()
    got = dict(zip(words[0::2], (int(v) for v in words[1::2])))
    # 2 widths x offsets x 7 rows x sum over plane rows of (rows + 1) x sum over rows of (row + 1) x 4 blocks x 3 lanes
    assert got['cases'] == (4 + 16) * (2 + 3 + 4 + 8) * (2 + 3 + 4 + 6 + 9 + 18 + 34) * 4 * 3
    assert got['wrong_head'] > 0 and got['wrong_singles'] > 0
