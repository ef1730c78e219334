"""The window's state machine (csrc/window_state.h: which view and pair list are the window's, what each call requires, leaves and
invalidates) without a GPU and without the library: tests/native/window_state_test.cpp includes that header alone and walks it."""
import os
import subprocess


def test_window_state_machine_under_the_sanitizers(tmp_path):
    """Built with -fsanitize=address,undefined by the host compiler, no HIP header or library: the named call sequences against literal
    states, every sequence of up to five calls against the invariants, every predicate against the expression the calls spelled out."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "window_state_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(root, "same_amd", "csrc"), os.path.join(root, "tests", "native", "window_state_test.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
