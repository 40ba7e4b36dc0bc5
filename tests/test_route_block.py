"""INCCL_SCALE_BLOCK on the host, without a GPU: the route a block-scaled call
takes (csrc/inccl_route.h inccl_route_block) walked against its table, and the
integer scale rule of the per-block kernels (csrc/inccl_scale_rule.h) walked
against the oracle's -- both by stand-alone C programs built with the address
and undefined-behaviour sanitizers -- and the Python sentinel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
          "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I",
          os.path.join(ROOT, "container_inc_amd", "csrc")]


def _run(exe):
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_route_block(tmp_path):
    exe = tmp_path / "route_block"
    subprocess.check_call(CFLAGS + [os.path.join(ROOT, "tests", "c", "route_block.c"), "-o", str(exe)])
    r = _run(exe)
    assert r.returncode == 0 and "route block ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    cases = int(r.stdout.split("route block ok:")[1].split()[0])
    assert cases > 5000, r.stdout   # 12 routes + 2 ops x 2 transports x 6 engines x 4 worlds x 4 switches x sizes


def test_integer_scale_rule_equals_the_oracle(tmp_path):
    exe = tmp_path / "scale_rule"
    subprocess.check_call(CFLAGS + ["-I", os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "c", "scale_rule.c"),
                                    os.path.join(ROOT, "oracle", "inccl_oracle.c"), "-o", str(exe), "-lm"])
    r = _run(exe)
    assert r.returncode == 0 and "scale rule ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
    assert int(r.stdout.split("scale rule ok:")[1].split()[0]) > 7_000_000, r.stdout


def test_scale_block_sentinel():
    from container_inc_amd import inccl
    assert inccl.SCALE_BLOCK == 0x7FFFFFFE and inccl.SCALE_BLOCK != inccl.SCALE_AUTO
    assert inccl.BLOCK_ELEMS == 256
    assert inccl._check_scale(inccl.SCALE_BLOCK) == inccl.SCALE_BLOCK
    assert inccl._check_scale(inccl.SCALE_AUTO) == inccl.SCALE_AUTO
    for k in (inccl.SCALE_BLOCK - 1, inccl.SCALE_MAX + 1, inccl.SCALE_MIN - 1):
        with pytest.raises(ValueError):
            inccl._check_scale(k)


def test_block_mode_header_constants():
    text = open(os.path.join(ROOT, "include", "inccl_amd.h")).read()
    assert "#define INCCL_SCALE_BLOCK 0x7ffffffe" in text and "#define INCCL_BLOCK_ELEMS 256" in text
