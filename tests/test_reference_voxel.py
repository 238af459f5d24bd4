"""The REFERENCE's own test of voxel down-sampling, test_voxel_downsample_xd of python/tests/test_core.py, run UNMODIFIED against
this repo: the staged, byte-identical oracle/_ref/pytests/test_core.py is collected by a child pytest whose `ouster.sdk.core` is
the product's ouster_sdk_amd/compat/ouster, with the shim and the invocation of tests/test_reference_python_tests.py (whose
deselection list, written before the product had this function, stays as it is).  The one test is selected by name."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PCAPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGED = os.path.join(ROOT, "oracle", "_ref", "pytests")
SHIM = os.path.join(ROOT, "tests", "ref_shim")
COMPAT = os.path.join(ROOT, "ouster_sdk_amd", "compat")
HELPERS = ("multi.py",)     # imported by test_core.py


@pytest.mark.skipif(not os.path.exists(os.path.join(STAGED, "test_core.py")),
                    reason="oracle/_ref/pytests is staged by `make -C oracle` only where the reference checkout exists")
def test_reference_voxel_downsample_xd_passes_unmodified(tmp_path):
    pkg = tmp_path / "tests"
    pkg.mkdir()
    (pkg / "__init__.py").write_text("")
    for name in ("test_core.py",) + HELPERS:
        shutil.copy(os.path.join(STAGED, name), pkg / name)          # byte-identical copies
    shutil.copy(os.path.join(SHIM, "conftest_for_reference_tests.py"), pkg / "conftest.py")
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join([COMPAT, SHIM, str(tmp_path), ROOT, env.get("PYTHONPATH", "")])
    env["OUSTER_REF_PCAPS"] = PCAPS
    env["OUSTER_REF_STAGED"] = STAGED
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "--rootdir", str(tmp_path), "-c", os.devnull,
                        f"{pkg / 'test_core.py'}::test_voxel_downsample_xd"], env=env, capture_output=True, text=True, timeout=600)
    tail = "\n".join(r.stdout.strip().splitlines()[-40:])
    m = re.search(r"(\d+) passed", r.stdout)
    print(f"reference voxel test: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-400:]}")
    assert r.returncode == 0 and m and int(m.group(1)) == 1 and "failed" not in r.stdout.splitlines()[-1], tail + r.stderr[-2000:]
