"""libibvh.so asked for BEFORE anything imported torch — what build() followed by smoke() does in a fresh process.  A
PyTorch-ROCm wheel brings its own HIP runtime; the library binds to whichever libamdhip64 is loaded when it comes in, so
lib.load() imports torch first.  Without that the process held two runtimes and the library's first launch on a torch
tensor returned IBVH_ERR_HIP.  Needs a process of its own: in this one torch has long been imported."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = """
import sys
sys.path.insert(0, {root!r})
assert "torch" not in sys.modules
import implicitbvh_amd as ibvh
from implicitbvh_amd import lib
lib.load()                                   # the library first, as in build()
import torch
v = ibvh.generate_spheres(1000, 42, r0=0.01)  # its first launch, into a torch tensor
torch.cuda.synchronize()
c = v.cpu()
assert c.shape == (1000, 4) and bool(torch.isfinite(c).all()) and bool((c[:, 3] > 0).all())
print("LOAD_ORDER_OK")
"""


def test_library_loaded_before_torch_still_launches():
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOAD_ORDER_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
