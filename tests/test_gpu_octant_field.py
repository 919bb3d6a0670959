"""The ray cast over the octant free-rectangle field against the C oracle, every field bit for bit (run with -m gpu on an MI355X).

The march's lookups after a ray's first jump read the octant array (csrc/mrca_host.h: build_octant_rect_field) or, with
MRCA_FIELD_OCTANTS=0, the quadrant array -- one instruction stream, the layout in FreeRectField's two uniforms.  The variable
is read by mrca_create, so each setting runs in a fresh child process (tests/octant_field_child.py) under a time limit of its
own; a child runs the smallest shapes that reach every instantiation the field object goes through -- Stage-1 (2 worlds x 3
robots), Stage-2, the circle world, Stage-1 in fidelity mode (the raster lidar), one world of 70 robots (the big-world variants)
--, each with lazy_obs 1 and 0, 12 ticks through mrca_step and through mrca_step_many (two ranges where there are two worlds;
launches of three ticks).  In every shape mrca_reset puts robot 0 onto a cell face, one cell from a wall and heading along it.

One child per setting, not one per shape: a child's cost is the interpreter's start and torch's import, the ten envs of a
setting are a few seconds together.  "1" forces the octant array on where the default rule leaves it off (Stage-2's and the
circle world's maps are larger than an XCD's L2)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "octant_field_child.py")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("octants", ["1", "0"], ids=["octants_on", "octants_off"])
def test_every_ray_cast_variant_against_the_c_oracle(octants):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ, MRCA_FIELD_OCTANTS=octants)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), ROOT] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    out = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=300)
    tail = "\n".join((out.stdout + out.stderr).splitlines()[-25:])
    assert out.returncode == 0, f"MRCA_FIELD_OCTANTS={octants}: the child left with {out.returncode}\n{tail}"
    lines = out.stdout.splitlines()
    assert lines[-1] == "all ok" and len([ln for ln in lines if ln.startswith("ok ")]) == 10, tail
