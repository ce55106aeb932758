"""Deterministic mode, host side (no GPU): the --deterministic row, the C ABI switch and GIC_DETERMINISTIC at library load."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_deterministic_arg_parses_and_defaults_to_zero():
    from gan_image_captioning_amd.args import build_parser, default_args
    assert build_parser().parse_args([]).deterministic == 0
    assert build_parser().parse_args(["--deterministic", "1"]).deterministic == 1
    assert default_args(deterministic=1, device="cpu").deterministic == 1


def test_set_get_round_trip_default_off():
    from gan_image_captioning_amd import _lib as L
    from gan_image_captioning_amd import engine
    assert "gic_set_deterministic" in L.EXPORTED_SYMBOLS and "gic_get_deterministic" in L.EXPORTED_SYMBOLS
    lib = L.load()
    before = lib.gic_get_deterministic()
    try:
        if not os.environ.get("GIC_DETERMINISTIC"):
            assert before == 0
        assert lib.gic_set_deterministic(1) == 0 and lib.gic_get_deterministic() == 1
        assert engine.deterministic()
        engine.set_deterministic(False)
        assert lib.gic_get_deterministic() == 0 and not engine.deterministic()
    finally:
        lib.gic_set_deterministic(before)


def _child_mode(env_value):
    env = dict(os.environ)
    env.pop("GIC_DETERMINISTIC", None)
    if env_value is not None:
        env["GIC_DETERMINISTIC"] = env_value
    code = "from gan_image_captioning_amd import engine; print(int(engine.deterministic()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return int(out.stdout.strip().splitlines()[-1])


def test_environment_variable_sets_the_mode_at_load():
    assert _child_mode("1") == 1
    assert _child_mode("0") == 0
    assert _child_mode(None) == 0
