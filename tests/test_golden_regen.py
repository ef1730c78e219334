"""The fixtures under tests/golden/ are outputs of the reference itself, made by tools/gen_golden.py where the reference is mounted.
Keeps the generator runnable from a fresh clone (it writes nothing outside its output and temporary directories)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_keeps_its_scratch_out_of_the_tree():
    """gpurun_out/ is git-ignored: a fresh clone does not have it, so the generator must not need it (round 3: FileNotFoundError)."""
    src = open(os.path.join(ROOT, "tools", "gen_golden.py"), encoding="utf-8").read()
    assert "gpurun_out" not in src and "tempfile.mkdtemp(prefix=" in src
