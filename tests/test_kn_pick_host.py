"""CPU test of csrc/kn_pick.h, the dispatcher that turns the run-time lane count, ion count, membrane path, geometry
variant and facet width of a handle into the template arguments of an assembly kernel.  The checks are in
tests/native/kn_pick_check.cpp (plain C++17 with its own main, no HIP): every listed value reaches the callback with that
constant exactly once, an unlisted one returns false without a call, and nested picks under a constexpr predicate reach
exactly the predicate's set over the full product of run-time values."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kn_pick_check.cpp")


def _run(exe, flags):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "20 combinations reached, 0 failure(s)" in p.stdout, (p.returncode, p.stdout, p.stderr)


def test_kn_pick_reaches_exactly_the_listed_values_and_the_built_combinations():
    build = os.path.join(HERE, "native", "_build")
    os.makedirs(build, exist_ok=True)
    _run(os.path.join(build, "kn_pick_check"), ["-O2"])


def test_kn_pick_check_is_clean_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program, instrumented: any report makes it exit non-zero (-fno-sanitize-recover)."""
    _run(str(tmp_path / "kn_pick_check_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
