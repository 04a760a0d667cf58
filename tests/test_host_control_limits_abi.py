"""CPU-only: the entry points of the acceleration limits exist in the built library, include/mppi_hip.h declares them with
the arguments the binding passes, and the mirror knows the key."""
import ctypes as C
import os
import re

from mppi_numba_amd import _lib, barebone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi_hip.h")

DECLARED = {
    "mppi_planner_set_control_limits": "mppi_planner* p, const float accel[2]",
    "mppi_planner_get_control_limits": "mppi_planner* p, float accel[2], int* held",
    "mppi_planner_limit_noise": "mppi_planner* p",
    "mppi_planner_set_applied_control": "mppi_planner* p, int count, const float* u",
    "mppi_planner_get_applied_control": "mppi_planner* p, float* u",
}


def test_the_library_exports_the_new_symbols_and_the_header_declares_them():
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, args in DECLARED.items():
        assert hasattr(lib, name), "libmppi_hip.so does not export %s" % name
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert " ".join(found.group(1).split()) == args, name
        assert len(_lib.SIGNATURES[name]) == len(args.split(",")), name
    assert _lib.SIGNATURES["mppi_planner_set_applied_control"][1] is C.c_int


def test_the_mirror_knows_the_key():
    kinds = [kind for kind in barebone._KINDS if kind.key == "accel_limits"]
    assert len(kinds) == 1
    kind = kinds[0]
    assert kind.setter == "mppi_planner_set_control_limits" and kind.clear == (None,) and kind.offsets is barebone._KEEP
    assert "accel_limits" in barebone._OPTIONAL_KEYS
    for name in ("accel_limits", "applied_control", "set_applied_control", "limit_noise"):
        assert hasattr(barebone.MPPI_Numba, name), name
    assert "params['accel_limits']" in barebone.__doc__
