"""The IPC buffer set protocol (container_inc_amd/csrc/ipc.c) and
inccl_boot_agree (bootstrap.c) without a GPU: a stand-alone C program
(tests/c/ipc_set.c) stands in for the HIP entry points, forks three ranks that
meet over the real TCP bootstrap on 127.0.0.1, and records every allocation,
export, free, open and close in a table the ranks share.  It links from ipc.c,
bootstrap.c and itself alone -- no HIP library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    1: "create, n = 1 and n = 4 regions, mixed polled",
    2: "grow twice: old buffers go only after every rank mapped the new ones",
    3: "one rank's hipIpcOpenMemHandle fails, on a create and on a grow",
    4: "one rank's allocation fails",
    5: "local_rc != 0 on one rank",
    6: "release on an empty set and twice in a row; the error words",
    7: "inccl_boot_agree",
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("ipc_set") / "ipc_set"
    csrc = os.path.join(ROOT, "container_inc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, os.path.join(ROOT, "tests", "c", "ipc_set.c"), os.path.join(csrc, "ipc.c"),
                           os.path.join(csrc, "bootstrap.c"), "-o", str(out)])
    return str(out)


@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: f"case{c}")
def test_ipc_set(exe, case):
    r = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0 and f"ipc_set case {case} ok" in r.stdout, CASES[case] + "\n" + r.stderr[-4000:]
