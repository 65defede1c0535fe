"""CPU: the public surface of the switch that puts calls WITH hazards, walls or teams on the 2x256 evaluation tile
(mobrob_ppo_set_eval_tile256_wide, PPO(eval_tile256_wide=), examples/control.py and examples/follow.py --tile256-wide).
The kernel itself: tests/test_eval_tile256_wide_gpu.py."""
import ctypes
import importlib.util
import inspect
import os
import re

import pytest

from mobrob_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mobrob_ppo_set_eval_tile256_wide"


def test_the_symbol_is_declared_exported_and_prototyped():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mobrob_ppo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+" + NAME + r"\s*\(\s*mobrob_ppo_engine_t\s*\*\s*e\s*,\s*int32_t\s+on\s*\)\s*;", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    assert _lib.SYMBOLS[NAME] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert lib.mobrob_ppo_abi_version() == _lib.ABI_VERSION == 3      # a symbol added, nothing altered


def test_a_null_engine_is_refused_by_name():
    lib = _lib.load()
    assert getattr(lib, NAME)(None, 1) == _lib.ERR_INVALID
    assert "tile256" in lib.mobrob_ppo_last_error().decode()


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0])
def test_ppo_rejects_non_bools(bad):
    from mobrob_amd.rl_control.ppo import PPO
    with pytest.raises(TypeError, match="eval_tile256_wide"):
        PPO(_dims=(4, 58, 12), eval_tile256_wide=bad, _init_setup_model=False)


def test_ppo_keeps_the_switch():
    from mobrob_amd.rl_control.ppo import PPO
    plain = PPO(_dims=(4, 58, 12), _init_setup_model=False)
    assert plain.eval_tile256_wide is False and plain.eval_tile256 is False
    both = PPO(_dims=(4, 58, 12), eval_tile256=True, eval_tile256_wide=True, _init_setup_model=False)
    assert both.eval_tile256_wide is True and both.eval_tile256 is True
    assert PPO(_dims=(4, 58, 12), eval_tile256=True, _init_setup_model=False).eval_tile256_wide is False


def test_the_engine_wrapper_has_the_setter_and_the_property():
    from mobrob_amd.engine import PPOEngine
    assert list(inspect.signature(PPOEngine.set_eval_tile256_wide).parameters) == ["self", "on"]
    assert isinstance(PPOEngine.eval_tile256_wide, property)


def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_cli_wide", os.path.join(ROOT, "examples", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_cli_flags_parse():
    control, follow = _example("control"), _example("follow")
    a = control.build_parser().parse_args(["--env-name", "doggo", "--robots", "64", "--tile256-wide"])
    assert a.tile256_wide is True and a.robots == 64
    assert control.build_parser().parse_args(["--robots", "64", "--tile256"]).tile256_wide is False
    f = follow.build_parser().parse_args(["--env-name", "doggo", "--goal", "0.8,0.8", "--arena", "--solid", "--tile256-wide"])
    assert f.tile256_wide is True and f.solid is True and f.arena is True
    assert follow.build_parser().parse_args(["--goal", "1,1", "--tile256"]).tile256_wide is False
    assert inspect.signature(follow.follow).parameters["tile256_wide"].default is False
    assert inspect.signature(control.simulate_device).parameters["tile256_wide"].default is False
