"""The counted vmcnt waits of bx3_kernel's loader waves (csrc/bx3_waits.h), proved on the host: tests/native/bx3_waits_host.cpp
replays a loader wave's instruction stream for every PER, ksteps 1 .. 48 and side count 0 .. ksteps + 8 and asserts that the
operands have landed at each barrier (A), that a side store never reads a slot whose request is outstanding (B), that no wait
reaches into the steps it means to leave in flight (C) and that every immediate fits the counter (D).  No GPU: a store that
reads a late DMA cannot be tested on one without waiting for it to happen."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def waits_host(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path_factory.mktemp("bx3_waits") / "bx3_waits_host"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "mms_answer_selection_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "bx3_waits_host.cpp"), "-o", str(exe)])
    return str(exe)


def test_loader_waits_hold_their_invariants(waits_host):
    out = subprocess.run([waits_host], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "invariants A-D hold" in out.stdout


def test_the_model_sees_the_uncovered_request(waits_host):
    """The rule the kernel had before the header counted side step j - 3 among what may stay in flight: request(j - 3)
    was never covered when store(j - 3) read its slot.  The model reports exactly that -- B, and nothing else."""
    out = subprocess.run([waits_host, "--rule", "parent"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("B violated"), out.stdout
    assert "DMAs still outstanding" in lines[0]
