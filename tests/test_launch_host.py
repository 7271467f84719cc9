"""abi_internal.h's launch() on its failure path, without a GPU: tests/launch_fail_main.hip is compiled as a stand-alone
program (its own main, its own fail) and run.  Without a device every launch is refused, and the program checks that the
refusal comes back as RL_ERR_HIP with the kernel's name and HIP's reason; where a device is present it launches nothing
and says so, and this test skips.  Nothing of it is loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_a_refused_launch_names_its_kernel_and_hips_reason(tmp_path):
    exe = str(tmp_path / "launch_fail")
    src = os.path.join(ROOT, "tests", "launch_fail_main.hip")
    cc = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, src],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    if run.stdout.startswith("skipped:"):
        pytest.skip("a device is present: the program launched nothing")
    assert run.stdout.startswith("refused: code -3, 'launch_probe_kernel launch failed: "), run.stdout
