"""The batched transform from a compiled host: Fft::batch and Fft::divide_by_z_on_coset_batch of include/kogarashi_amd.hpp, driven by
tests/host/ntt_batch_cpp_test.cpp against the oracle's C restatement of fft.rs -- built with g++ (no HIP, no Python in the loop: the
binary links libkogarashi_amd.so and liboracle.so only) and run, the way tests/test_gpu_cpp_host.py runs its program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    from oracle import oracle as O
    O.build()
    exe = str(tmp_path / "ntt_batch_cpp_test")
    lib_dir, ora_dir = os.path.join(ROOT, "kogarashi_amd"), os.path.join(ROOT, "oracle")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "ntt_batch_cpp_test.cpp"),
                           "-L" + lib_dir, "-lkogarashi_amd", "-L" + ora_dir, "-loracle", "-Wl,-rpath," + lib_dir, "-Wl,-rpath," + ora_dir])
    return exe


def test_cpp_batch_compiles_against_the_abi(tmp_path):
    """no GPU needed: the header's batched methods and the test program compile and link against the built library"""
    from kogarashi_amd import build
    build.build()
    assert os.path.exists(_build(tmp_path))


@pytest.mark.gpu
def test_cpp_batch_matches_the_oracle(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok:" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
