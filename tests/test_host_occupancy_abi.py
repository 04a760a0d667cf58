"""CPU-only: the entry points of the occupancy grid exist in the built library, include/mppi_hip.h declares them with the
arguments the binding passes, and the mirror knows the key."""
import ctypes as C
import os
import re

import numpy as np

from mppi_numba_amd import _lib, barebone

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mppi_hip.h")

DECLARED = {
    "mppi_planner_set_occupancy": "mppi_planner* p, int on, float x_min, float y_min, float res, int nx, int ny, float inflate, "
                                  "int substeps, const unsigned char* cells",
    "mppi_planner_get_occupancy": "mppi_planner* p, int* on, int* nx, int* ny, unsigned long long* fields_built",
    "mppi_planner_occupancy_refresh": "mppi_planner* p",
    "mppi_planner_get_occupancy_field": "mppi_planner* p, unsigned* out",
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
    assert _lib.SIGNATURES["mppi_planner_set_occupancy"][8] is C.c_int
    assert _lib.SIGNATURES["mppi_planner_set_occupancy"][9] == C.POINTER(C.c_ubyte)


def test_the_mirror_knows_the_key():
    kinds = [kind for kind in barebone._KINDS if kind.key == "occupancy"]
    assert len(kinds) == 1
    kind = kinds[0]
    assert kind.setter == "mppi_planner_set_occupancy" and kind.clear[0] == 0 and kind.offsets is barebone._KEEP
    names = [k.name for k in barebone._KINDS]
    assert names.index("occupancy") < names.index("guide"), "the grid is handed over ahead of the guide"
    assert "occupancy" in barebone._OPTIONAL_KEYS
    for name in ("occupancy_field", "refresh_occupancy", "occupancy_fields_built"):
        assert hasattr(barebone.MPPI_Numba, name), name
    assert "params['occupancy']" in barebone.__doc__ and "512" in barebone.__doc__


def test_the_key_is_read_as_uint8_cells():
    cells = np.zeros((3, 5), np.int64)
    cells[1, 2] = 7
    p = {"occupancy": {"origin": (0.5, -1.0), "resolution": 0.1, "cells": cells, "inflate": 0.2, "substeps": 3}}
    values, substeps, got = barebone._read_occupancy(None, p)
    assert got.dtype == np.uint8 and got.shape == (3, 5) and got.sum() == 1 and got[1, 2] == 1
    np.testing.assert_array_equal(values, np.float32([0.5, -1.0, 0.1, 0.2]))
    assert substeps.tolist() == [3]
    args = barebone._pack_occupancy(None, values, substeps, got)
    assert args[:8] == (1, 0.5, -1.0, float(np.float32(0.1)), 5, 3, float(np.float32(0.2)), 3) and args[8] is got
    for bad in ({"cells": np.zeros((3, 5))}, {"cells": np.zeros(5, np.uint8)}, {"cells": np.zeros((513, 2), np.uint8)},
                {"substeps": 0}, {"substeps": 9}, {"substeps": 2.0}, {"origin": (0.0,)}):
        try:
            barebone._read_occupancy(None, {"occupancy": dict(p["occupancy"], **bad)})
        except ValueError as err:
            assert "occupancy" in str(err)
        else:
            raise AssertionError("accepted %r" % (bad,))
    default = barebone._read_occupancy(None, {"occupancy": {"origin": (0, 0), "resolution": 1.0, "cells": np.ones((2, 2), bool)}})
    assert default[0][3] == 0.0 and default[1].tolist() == [1] and default[2].all()


def test_rasterise_obstacles():
    cells = barebone.rasterise_obstacles((0.0, 0.0), 0.5, (4, 6), segments=np.float32([[[0.0, 1.25], [3.0, 1.25]]]), halfwidth=0.1)
    assert cells.dtype == np.uint8 and cells.shape == (4, 6)
    np.testing.assert_array_equal(cells, np.uint8([[0] * 6, [0] * 6, [1] * 6, [0] * 6]))  # (centres at y = 1.25: row 2)
    discs = barebone.rasterise_obstacles((0.0, 0.0), 0.5, (4, 6), discs=np.float32([[0.75, 0.75]]), radii=[0.5])
    want = np.zeros((4, 6), np.uint8)
    want[1, 1] = want[0, 1] = want[2, 1] = want[1, 0] = want[1, 2] = 1  # (the centre's cell and the four at 0.5: the rim counts)
    np.testing.assert_array_equal(discs, want)
    both = barebone.rasterise_obstacles((0.0, 0.0), 0.5, (4, 6), np.float32([[[0.0, 1.25], [3.0, 1.25]]]), 0.1, np.float32([[0.75, 0.75]]), [0.5])
    np.testing.assert_array_equal(both, cells | want)
    assert not barebone.rasterise_obstacles((0.0, 0.0), 0.5, (4, 6)).any()
