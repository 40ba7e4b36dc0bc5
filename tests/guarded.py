"""TEST INFRASTRUCTURE ONLY -- device buffers inside sentinel guards, for the
tests that call the library above the kernel layer (tests/comm_guard_cases.py).

A Buf is n elements of a kind, `shift` elements past a 16-B boundary, in the
middle of one allocation whose other elements hold a sentinel.  bits() checks
both guards before it returns the payload, so a store before element 0 or past
element n fails the test that reads the buffer instead of landing in the slack
torch rounds an allocation up to.

G = 1024 elements either side.  The widest padding an engine could spill at the
sizes of these tests is W * 64 = 512 elements (inccl_shard_elems at W = 8), and
one quad tile of an engine kernel more stays below 1024; so an overrun, real or
from a mutation, stays inside the allocation the test owns.  1024 elements are
4096 B or 2048 B: the payload keeps the allocation's 16-B alignment."""
import numpy as np

G = 1024
SENT = {4: 0x5A5A5A5A, 2: 0x5A5A}
KINDS = {"f32": ("float32", 4), "i32": ("int32", 4), "bf16": ("bfloat16", 2), "f16": ("float16", 2)}


class Buf:
    """n elements of `kind` ("f32", "i32", "bf16", "f16") on the GPU, `shift`
    elements past a 16-B boundary, inside an allocation whose other elements
    hold a sentinel: `bits` (uint32 / uint16 patterns, or values of the kind's
    width) or the sentinel throughout"""

    def __init__(self, dev, kind, n, bits=None, shift=0):
        import torch
        name, w = KINDS[kind]
        dt = np.uint32 if w == 4 else np.uint16
        host = np.full(G + shift + n + G, SENT[w], dt)
        if bits is not None:
            host[G + shift:G + shift + n] = np.ascontiguousarray(bits).view(dt)
        self.kind, self.w, self.n, self.lo = kind, w, n, G + shift
        self.uploaded = host[self.lo:self.lo + n].copy()
        self.raw = torch.from_numpy(host.view(np.int32 if w == 4 else np.int16)).to(dev)
        self.t = self.raw[self.lo:self.lo + n].view(getattr(torch, name))
        assert self.t.data_ptr() % 16 == (shift * w) % 16

    def bits(self):
        """the n elements' bit patterns, after checking both guards"""
        import torch
        torch.cuda.synchronize()
        host = self.raw.cpu().numpy().view(np.uint32 if self.w == 4 else np.uint16)
        assert (host[:self.lo] == SENT[self.w]).all(), "written before element 0"
        assert (host[self.lo + self.n:] == SENT[self.w]).all(), "written past element n"
        return host[self.lo:self.lo + self.n].copy()

    def assert_unchanged(self):
        """both guards, and the payload bit-identical to what was uploaded"""
        np.testing.assert_array_equal(self.bits(), self.uploaded)
