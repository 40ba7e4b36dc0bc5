"""Packed 16-bit lanes on the host, without a GPU: the lanes' exponent and clamp
(csrc/inccl_scale_rule.h) walked against the spec on the oracle's rule, and the
route a packed call takes (csrc/inccl_route.h inccl_route_packed) walked against
its table -- both by stand-alone C programs built with the address and
undefined-behaviour sanitizers -- the constants of the header and of the Python
mirror, and the hooks' wire_bits."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
          "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I",
          os.path.join(ROOT, "container_inc_amd", "csrc")]


def _run(exe):
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_route_packed(tmp_path):
    exe = tmp_path / "route_packed"
    subprocess.check_call(CFLAGS + [os.path.join(ROOT, "tests", "c", "route_packed.c"), "-o", str(exe)])
    r = _run(exe)
    assert r.returncode == 0 and "route packed ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    cases = int(r.stdout.split("route packed ok:")[1].split()[0])
    assert cases > 7000, r.stdout   # 12 routes x 8 worlds x 20 sizes + the route policy's cases


def test_lane_exponent_and_clamp_equal_the_spec(tmp_path):
    exe = tmp_path / "scale_rule16"
    subprocess.check_call(CFLAGS + ["-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "c", "scale_rule16.c"),
                                    os.path.join(ROOT, "oracle", "inccl_oracle.c"), "-o", str(exe), "-lm"])
    r = _run(exe)
    assert r.returncode == 0 and "scale rule 16 ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert int(r.stdout.split("scale rule 16 ok:")[1].split()[0]) > 7_000_000, r.stdout


def test_constants():
    from container_inc_amd import inccl
    text = open(os.path.join(ROOT, "include", "inccl_amd.h")).read()
    assert "#define INCCL_KIND_P16 5" in text and inccl.KIND_P16 == 5
    assert "#define INCCL_WIRE_Q32 0" in text and "#define INCCL_WIRE_P16 1" in text
    assert (inccl.WIRE_Q32, inccl.WIRE_P16) == (0, 1)


class _Comm:
    """what the hooks touch of a communicator before any collective"""

    def __init__(self):
        self.wires, self.nonfinite = [], []

    def set_wire(self, wire):
        self.wires.append(wire)

    def set_nonfinite(self, on):
        self.nonfinite.append(on)


def test_hook_state_sets_the_wire_once():
    from container_inc_amd import ddp, inccl
    comm = _Comm()
    state = ddp.HookState(comm=comm, scale_exp=inccl.SCALE_BLOCK, wire_bits=16)
    state.apply_wire()
    state.apply_wire()
    assert comm.wires == [inccl.WIRE_P16]
    comm = _Comm()
    state = ddp.HookState(comm=comm, scale_exp=inccl.SCALE_BLOCK)
    assert state.wire_bits == 32
    state.apply_wire()
    state.apply_wire()
    assert comm.wires == [inccl.WIRE_Q32]
    import dataclasses
    assert [f.name for f in dataclasses.fields(ddp.HookState)][-1] == "wire_bits"


@pytest.mark.parametrize("bits", [8, 0, 24, "16"])
def test_hook_state_refuses_another_width_by_name(bits):
    from container_inc_amd import ddp, inccl
    from container_inc_amd._lib import IncclError
    comm = _Comm()
    state = ddp.HookState(comm=comm, scale_exp=inccl.SCALE_BLOCK, wire_bits=bits)
    with pytest.raises(IncclError, match="wire_bits"):
        state.apply_wire()
    assert comm.wires == []


def test_fsdp_hook_applies_the_wire_before_the_collective():
    """the FSDP hooks go through the same state: the width is checked, and the
    wire set, before the communicator is asked to reduce anything"""
    import torch
    from container_inc_amd import ddp, fsdp, inccl
    from container_inc_amd._lib import IncclError
    g = torch.ones(8, dtype=torch.float32)
    with pytest.raises(IncclError, match="wire_bits"):
        fsdp.allreduce_hook(ddp.HookState(comm=_Comm(), scale_exp=inccl.SCALE_BLOCK, wire_bits=8), g)
