"""torch tensors and torch streams at the C-ABI, each case in a fresh child process (tests/torch_seam_child.py), one at a time: torch
bundles its own HIP runtime, and which one the library binds depends on import order - the child imports torch first, so that both use
one runtime, and checks that only one is mapped.

  views          strided / offset / from-numpy tensors as device clouds: bitwise the host path;
  side_stream    a context on a torch side stream (dcreg_set_stream), then back on its own stream: bitwise its own stream's records;
  order_side     a cloud written on the caller's stream behind a long device sleep is read after the write;
  order_default  the same on torch's default stream (the legacy null stream) with the context on its own non-blocking stream - with
                 and without dcreg_set_stream(0);
  order_rows     the same for the device inputs that are not clouds - kept normals given from device memory, descriptor rows,
                 correspondence arrays - on the default stream (both contexts) and on a side stream.

After a child ends abnormally (a signal, or the time limit) no further child is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "torch_seam_child.py")
_abnormal = []


@pytest.mark.parametrize("case", ["views", "side_stream", "order_side", "order_default", "order_rows"])
def test_torch_case_in_child(case):
    pytest.importorskip("torch")
    if _abnormal:
        pytest.skip("an earlier child ended abnormally (%s): no further child is started" % _abnormal[0])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, case]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _abnormal.append("%s: time limit" % case)
        pytest.fail("%s: no result within %d s\n%s" % (case, e.timeout, (e.stderr or b"")[-4000:]))
    if p.returncode < 0 or p.returncode in (124, 137):
        _abnormal.append("%s: status %d" % (case, p.returncode))
    assert p.returncode == 0, "%s: status %d\n--- stderr ---\n%s\n--- stdout ---\n%s" % (case, p.returncode, p.stderr[-6000:], p.stdout[-2000:])
