"""CPU-only: car-like steering (params['drive'] = 'car') above the kernels -- the entry points exist in the built library,
include/mppi_hip.h declares them and the binding passes their arguments; the mirror hands the drive over only when the key
is there or has gone (the recorder of tests/test_barebone_mirror_calls.py); and the two host bounds on the heading
increment (csrc/map_plan.h: map_reach, map_rotation_ok) take max|v| * max|kappa| in car mode."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

from mppi_numba_amd import _lib, barebone
from test_barebone_mirror_calls import Recorder, Run, arr, base, without

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi_hip.h")
PLAN_HEADER = os.path.join(ROOT, "mppi_numba_amd", "csrc", "map_plan.h")

DECLARED = {
    "mppi_planner_set_drive": "mppi_planner* p, int drive",
    "mppi_planner_get_drive": "mppi_planner* p, int* drive",
}


# ---------------------------------------------------------------------------------------------------- ABI
def test_the_library_exports_the_new_symbols_and_the_header_declares_them():
    lib = _lib.load()
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, args in DECLARED.items():
        assert hasattr(lib, name), "libmppi_hip.so does not export %s" % name
        found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "include/mppi_hip.h does not declare %s" % name
        assert " ".join(found.group(1).split()) == args, name
        assert len(_lib.SIGNATURES[name]) == len(args.split(",")), name
    assert _lib.SIGNATURES["mppi_planner_set_drive"][1] is C.c_int
    for name, value in (("MPPI_DRIVE_UNICYCLE", 0), ("MPPI_DRIVE_CAR", 1)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, flags=re.M), name
    assert (_lib.DRIVE_UNICYCLE, _lib.DRIVE_CAR) == (0, 1)
    # mppi_params stays as it is: the drive is no field of it
    struct = re.search(r"typedef struct mppi_params \{(.*?)\} mppi_params;", raw, flags=re.S)
    assert struct and "drive" not in struct.group(1)
    assert not any("drive" in name for name, _ in _lib.Params._fields_)


def test_the_mirror_knows_the_key():
    kinds = [kind for kind in barebone._KINDS if kind.key == "drive"]
    assert len(kinds) == 1
    kind = kinds[0]
    assert kind.setter == "mppi_planner_set_drive" and kind.clear == (0,) and kind.offsets is barebone._KEEP
    assert "drive" in barebone._OPTIONAL_KEYS
    assert isinstance(barebone.MPPI_Numba.drive, property)
    for name in ("curvature_of_steering", "steering_of_curvature"):
        assert callable(getattr(barebone, name)), name
    assert "params['drive']" in barebone.__doc__


# ---------------------------------------------------------------------------------------------------- the mirror's calls
def drive_calls(steps):
    """Per step: the arguments of the mppi_planner_set_drive calls it made, and whether they came ahead of its solve."""
    out = []
    for step in steps:
        names = [call[0] for call in step["calls"]]
        sets = [call[1:] for call in step["calls"] if call[0] == "mppi_planner_set_drive"]
        if sets and "mppi_planner_solve" in names:
            assert names.index("mppi_planner_set_drive") < names.index("mppi_planner_solve"), step["step"]
        out.append(sets)
    return out


def run_scenario(scenario, monkeypatch):
    recorder = Recorder()
    monkeypatch.setattr(_lib, "call", recorder.call)
    monkeypatch.setattr(_lib, "ptr", lambda array, ctype: array)
    run = Run(recorder)
    try:
        scenario(run)
    finally:
        steps = run.close()
    return steps


def test_without_the_key_the_drive_is_never_handed_over(monkeypatch):
    def scenario(r):
        pl = r.make()
        r.step("setup", lambda: pl.setup(base()))
        r.step("solve", pl.solve)
        r.step("solve again", pl.solve)
        r.step("control step", lambda: pl.shift_and_update(arr([0.0, 0.25, 0.5]), np.zeros((4, 2), np.float32)))
        r.step("rollout", pl.rollout)
        r.step("state rollouts", pl.get_state_rollout)
        r.step("closed loop", lambda: pl.closed_loop(3))
    steps = run_scenario(scenario, monkeypatch)
    assert all(step["error"] is None for step in steps)
    assert any(call[0] == "mppi_planner_solve" for step in steps for call in step["calls"])
    assert not any("drive" in call[0] for step in steps for call in step["calls"])


def test_the_drive_is_handed_over_when_the_key_is_there_or_has_gone(monkeypatch):
    def scenario(r):
        pl = r.make()
        r.step("setup", lambda: pl.setup(base(drive="car")))
        r.step("car: first solve", pl.solve)
        r.step("car: second solve", pl.solve)
        pl.params["drive"] = "car"
        r.step("car: the same value again", pl.rollout)
        pl.params["drive"] = "unicycle"
        r.step("unicycle", pl.solve)
        r.step("unicycle: again", pl.solve)
        pl.params["drive"] = "car"
        r.step("car once more", pl.solve)
        pl.params = without(pl.params, "drive")
        r.step("the key removed", pl.solve)
        r.step("the key removed: again", pl.solve)
    steps = run_scenario(scenario, monkeypatch)
    assert all(step["error"] is None for step in steps)
    assert dict(zip([s["step"] for s in steps], drive_calls(steps))) == {
        "construct": [], "setup": [], "car: first solve": [[1]], "car: second solve": [], "car: the same value again": [],
        "unicycle": [[0]], "unicycle: again": [], "car once more": [[1]], "the key removed": [[0]], "the key removed: again": []}


def test_unicycle_from_the_start_is_the_key_left_out(monkeypatch):
    def scenario(r):
        pl = r.make()
        r.step("setup", lambda: pl.setup(base(drive="unicycle")))
        r.step("solve", pl.solve)
    steps = run_scenario(scenario, monkeypatch)
    assert not any("drive" in call[0] for step in steps for call in step["calls"])


def test_a_bad_string_is_refused_ahead_of_any_call(monkeypatch):
    def scenario(r):
        pl = r.make()
        r.step("setup", lambda: pl.setup(base(drive="tank")))
        r.step("tank", pl.solve)
        pl.params["drive"] = 1
        r.step("an int", pl.solve)
        pl.params["drive"] = "Car"
        r.step("another case", pl.rollout)
        pl.params["drive"] = "car"
        r.step("car", pl.solve)
    steps = {step["step"]: step for step in run_scenario(scenario, monkeypatch)}
    for label in ("tank", "an int", "another case"):
        assert steps[label]["calls"] == [], (label, steps[label]["calls"])
        assert "params['drive']" in steps[label]["error"] and "'car'" in steps[label]["error"]
    assert steps["car"]["error"] is None
    assert [call[1:] for call in steps["car"]["calls"] if call[0] == "mppi_planner_set_drive"] == [[1]]


# ---------------------------------------------------------------------------------------------------- the host bounds
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include "%s"
int main() {
  for (;;) {
    MapHeld h;
    std::memset(&h, 0, sizeof(h));
    int with_drive, drive;
    if (std::scanf("%%d %%d %%d %%f %%f %%f %%f %%f %%d %%d", &h.mode, &h.math, &h.T, &h.dt, &h.vrange[0], &h.vrange[1], &h.wrange[0],
                   &h.wrange[1], &with_drive, &drive) != 10)
      break;
    h.res = 1.0f;
    if (with_drive) h.drive = drive;  // (else as the memset left it: a state filled field by field without the new member)
    const MapReach r = map_reach(h);
    std::printf("%%d %%.17g %%.17g\n", (int)map_rotation_ok(h), r.wmax, (double)h.dt * r.wmax * r.trmax_ang);
  }
  return 0;
}
"""

BAREBONE, DET = 3, 0


def test_the_heading_bounds_take_the_product_in_car_mode(tmp_path):
    src = tmp_path / "drive_plan.cpp"
    src.write_text(PROGRAM % os.path.abspath(PLAN_HEADER))
    exe = tmp_path / "drive_plan"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), str(src)])
    pi = float(np.float32(math.pi))
    dt = float(np.float32(0.1))
    # (mode, math, T, dt, v_lo, v_hi, w_lo, w_hi, with_drive, drive) -> rotation, max |w|
    rows = [
        ((BAREBONE, 0, 30, 0.1, 0.0, 2.0, -math.pi, math.pi, 0, 0), (1, pi)),             # the standard task, unicycle: 0.314
        ((BAREBONE, 0, 30, 0.1, 0.0, 2.0, -math.pi, math.pi, 1, 0), (1, pi)),
        ((BAREBONE, 0, 30, 0.1, 0.0, 2.0, -math.pi, math.pi, 1, 1), (0, 2.0 * pi)),       # ... as a car: 0.628, rotation off
        ((BAREBONE, 0, 30, 0.1, 0.0, 2.0, -math.pi / 2, math.pi / 2, 1, 1), (1, 2.0 * float(np.float32(math.pi / 2)))),  # wrange halved: 0.314
        ((BAREBONE, 0, 30, 0.1, 0.0, 2.0, -1.5 * math.pi, 1.5 * math.pi, 1, 0), (0, float(np.float32(1.5 * math.pi)))),  # unicycle rows as today
        ((BAREBONE, 0, 30, 0.1, -3.0, 1.0, -1.0, 0.5, 1, 1), (1, 3.0)),                   # max |v| * max |kappa|, either sign
        ((BAREBONE, 0, 30, 0.1, -3.0, 1.0, -1.0, 1.25, 1, 1), (0, 3.75)),
        ((BAREBONE, 0, 2001, 0.1, 0.0, 2.0, -1.0, 1.0, 1, 1), (0, 2.0)),                  # (the horizon's bound stays)
        ((BAREBONE, 0, 30, 0.1, 0.0, float("inf"), -1.0, 1.0, 1, 1), (0, float("inf"))),
        ((BAREBONE, 0, 30, 0.1, 0.0, 0.0, -1e30, 1e30, 1, 1), (1, 0.0)),                  # a car that cannot move cannot turn
    ]
    text = "".join(" ".join(str(v) for v in state) + "\n" for state, _ in rows)
    out = subprocess.run([str(exe)], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    assert len(out) == len(rows)
    for (state, (rotation, wmax)), line in zip(rows, out):
        got_rot, got_wmax, got_bound = line.split()
        assert int(got_rot) == rotation, (state, line)
        assert float(got_wmax) == wmax, (state, line)
        assert float(got_bound) == dt * wmax or not math.isfinite(wmax), (state, line)
