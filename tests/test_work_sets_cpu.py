"""The protocol of the merged rows' reader calls' work buffers (csrc/work_sets.h: what a buffer is laid for, which of its two sets the next
call counts into, the in-doubt window of a call) without a GPU and without the library: tests/native/work_sets_test.cpp includes that header
alone and walks it -- a device call that fails half way among the steps, which no GPU test may provoke."""
import os
import subprocess


def test_work_sets_protocol_under_the_sanitizers(tmp_path):
    """Built with -fsanitize=address,undefined by the host compiler, no HIP header or library: the named call sequences against literal
    states (a scope left without the wait leaves "not laid"; a completed call restores what was laid and flips once; later phases restore
    without flipping; laid anew resets set and dirty count), every sequence of up to five transitions against the invariants."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "work_sets_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "same_amd", "csrc"), os.path.join(root, "tests", "native", "work_sets_test.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
