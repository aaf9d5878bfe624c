"""The launch plan of the one-launch GRU recurrences (csrc/spg_px_plan.h) on the host: tests/px_plan_host_test.cpp under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_px_plan_host(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler (c++, g++ or clang++) on PATH')
    exe = str(tmp_path / 'px_plan_host_test')
    build = subprocess.run([cxx, '-std=c++17', '-O2', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all', os.path.join(HERE, 'px_plan_host_test.cpp'), '-o', exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'px_plan_host_test: ok' in run.stdout
