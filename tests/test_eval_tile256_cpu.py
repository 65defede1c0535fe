"""CPU: the public surface of the 2x256 evaluation tile switch (mobrob_ppo_set_eval_tile256, PPO(eval_tile256=),
examples/control.py --tile256, examples/follow.py --tile256).  The kernel itself: tests/test_eval_tile256_gpu.py."""
import ctypes
import importlib.util
import os
import re

import pytest

from mobrob_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_exported_and_prototyped():
    name = "mobrob_ppo_set_eval_tile256"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobrob_ppo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + name + r"\s*\(\s*mobrob_ppo_engine_t\s*\*\s*e\s*,\s*int32_t\s+on\s*\)\s*;", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.SYMBOLS[name] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3
    assert not name.startswith("mobrob_ppo_plan_")
    planner_calls = sorted(n for n in _lib.SYMBOLS if n.startswith("mobrob_ppo_plan_"))
    assert len(planner_calls) == 10, planner_calls


def test_a_null_engine_is_refused_by_name():
    lib = _lib.load()
    assert lib.mobrob_ppo_set_eval_tile256(None, 1) == _lib.ERR_INVALID
    assert "tile256" in lib.mobrob_ppo_last_error().decode()


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_ppo_rejects_non_bools(bad):
    from mobrob_amd.rl_control.ppo import PPO
    with pytest.raises(TypeError, match="eval_tile256"):
        PPO(_dims=(4, 58, 12), eval_tile256=bad, _init_setup_model=False)


def test_ppo_keeps_the_switch():
    from mobrob_amd.rl_control.ppo import PPO
    assert PPO(_dims=(4, 58, 12), _init_setup_model=False).eval_tile256 is False
    assert PPO(_dims=(4, 58, 12), eval_tile256=True, _init_setup_model=False).eval_tile256 is True


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_cli", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_cli_flags_parse():
    control, follow = _example("control"), _example("follow")
    a = control.build_parser().parse_args(["--env-name", "doggo", "--robots", "64", "--tile256"])
    assert a.tile256 is True and a.robots == 64
    assert control.build_parser().parse_args(["--robots", "64"]).tile256 is False
    f = follow.build_parser().parse_args(["--env-name", "doggo", "--goal", "1,1", "--tile256"])
    assert f.tile256 is True
    assert follow.build_parser().parse_args(["--goal", "1,1"]).tile256 is False
    import inspect
    assert inspect.signature(follow.follow).parameters["tile256"].default is False
    assert inspect.signature(control.simulate_device).parameters["tile256"].default is False
