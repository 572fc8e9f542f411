"""The next-up descriptor of the job pipeline's lane hand-off (pbsim3_amd/csrc/handoff.h: publish / take / withdraw) is plain
C++.  tests/handoff_tsan_main.cpp replays the pipeline's threads around it -- the main loop, the two lane threads of the
round in front, the round's own lane threads -- with plain memory in place of the lanes' GPU state; built with
-fsanitize=thread and run here as a program of its own, it fails on a data race as well as on a broken protocol (a
descriptor taken twice, taken after it was withdrawn, a lane that finds another round's head)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pbsim3_amd", "csrc")


def test_descriptor_under_the_thread_sanitizer(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None and os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        cxx = "/opt/rocm/lib/llvm/bin/clang++"
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "handoff_tsan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-I", CSRC, os.path.join(HERE, "handoff_tsan_main.cpp"),
                    "-o", exe, "-lpthread"], check=True)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    if "unexpected memory mapping" in p.stderr and shutil.which("setarch"):
        # an older sanitizer runtime on a kernel with more address-space randomisation than it knows: the same program, the
        # same checks, with the randomisation off for this one process
        p = subprocess.run(["setarch", os.uname().machine, "-R", exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "0 failures" in p.stdout and "ThreadSanitizer" not in p.stderr
