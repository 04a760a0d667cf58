"""The `mppi_numba` alias package: code written against the reference imports the HIP engine
for config / mppi / terrain and finds the reference's host-side helpers (density,
visualization, utils) in a reference checkout; without one they do not resolve (they are out of
this repository's scope) and the ImportError says where to point MPPI_NUMBA_REFERENCE.
IMPORT_CELL: the mppi_numba imports of the reference notebooks' first cell (all five notebooks
start with the same imports)."""
import importlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMPORT_CELL = """
from mppi_numba.density import Density, GaussianMixture
from mppi_numba.terrain import Terrain, TDM_Numba, TractionGrid
from mppi_numba.visualization import TDM_Visualizer, vis_density, vis_density_as_pmf
from mppi_numba.mppi import MPPI_Numba
from mppi_numba.config import Config
import mppi_numba, mppi_numba.density, mppi_numba.mppi, mppi_numba.utils
print(mppi_numba.density.__file__)
print(mppi_numba.mppi.__file__)
print(MPPI_Numba.__module__, TDM_Numba.__module__, Config.__module__)
"""


def run_py(code, pythonpath, env_extra=None):
    env = dict(os.environ, PYTHONPATH=pythonpath, MPLBACKEND="Agg")
    env.pop("MPPI_NUMBA_REFERENCE", None)
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd="/tmp")
    assert out.returncode == 0, out.stderr
    return out.stdout.strip().splitlines()


def test_without_a_reference_the_engine_imports_and_the_helpers_say_where_to_find_them():
    code = ("from mppi_numba.terrain import Terrain, TDM_Numba, TractionGrid\n"
            "from mppi_numba.mppi import MPPI_Numba\n"
            "from mppi_numba.config import Config\n"
            "import mppi_numba.mppi\n"
            "print(mppi_numba.mppi.__file__)\n"
            "print(MPPI_Numba.__module__, TDM_Numba.__module__, Config.__module__)\n"
            "try:\n"
            "    import mppi_numba.density\n"
            "    print('imported')\n"
            "except ImportError as e:\n"
            "    print('MPPI_NUMBA_REFERENCE' in str(e))\n")
    lines = run_py(code, ROOT)
    assert lines[0] == os.path.join(ROOT, "mppi_numba_amd", "mppi.py")
    assert lines[1] == "mppi_numba_amd.mppi mppi_numba_amd.terrain mppi_numba_amd.config"
    assert lines[2] == "True"


def test_the_test_suites_stand_ins_resolve_through_the_same_hook():
    """tests/standins/ (minimal density / visualization / utils for boxes without the reference:
    test infrastructure of tests/test_gpu_notebook_flow.py) is found the way a checkout is."""
    lines = run_py(IMPORT_CELL, ROOT, {"MPPI_NUMBA_REFERENCE": os.path.join(ROOT, "tests", "standins")})
    assert lines[0] == os.path.join(ROOT, "tests", "standins", "density.py")
    assert lines[1] == os.path.join(ROOT, "mppi_numba_amd", "mppi.py")


@pytest.fixture
def reference_checkout(tmp_path):
    """A directory laid out like a checkout of the reference -- its `mppi_numba` package with the host-side helper
    modules -- holding the suite's stand-ins (tests/standins/): what is tested is where the helpers are taken from."""
    pkg = tmp_path / "mppi_numba"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    for name in ("density", "visualization", "utils"):
        shutil.copy(os.path.join(ROOT, "tests", "standins", name + ".py"), str(pkg / (name + ".py")))
    return str(tmp_path)


@pytest.mark.parametrize("how", ["pythonpath", "env"])
def test_import_cell_with_reference_forwards_the_host_helpers(how, reference_checkout):
    if how == "pythonpath":   # the checkout behind this repository on PYTHONPATH
        lines = run_py(IMPORT_CELL, ROOT + ":" + reference_checkout)
    else:
        lines = run_py(IMPORT_CELL, ROOT, {"MPPI_NUMBA_REFERENCE": reference_checkout})
    assert lines[0] == os.path.join(reference_checkout, "mppi_numba", "density.py")
    # the engine modules are never the reference's (they would need numba + CUDA)
    assert lines[1] == os.path.join(ROOT, "mppi_numba_amd", "mppi.py")
    assert lines[2] == "mppi_numba_amd.mppi mppi_numba_amd.terrain mppi_numba_amd.config"
