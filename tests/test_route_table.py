"""The communicator's route policy (container_inc_amd/csrc/inccl_route.h) walked
against the route table of DESIGN.md by a stand-alone C program
(tests/c/route_table.c): every operation x kind x transport x engine x world x
knob combination, the table written out in the program as data."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_route_table(tmp_path):
    exe = tmp_path / "route_table"
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "container_inc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "route_table.c"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "route table ok" in r.stdout, r.stdout[-4000:]
    cases = int(r.stdout.split("route table ok:")[1].split()[0])
    assert cases > 10000, r.stdout   # 2 ops x 3 kinds x 2 transports x 6 engines x 3 worlds x 4 switches x sizes
