"""The per-block and packed-lane kernels past their grid caps (gpu): every
capped grid-stride loop of inccl_block.hip and inccl_pack.hip taken into its
second pass, bit for bit against tests/block_ref.py, tests/block16_ref.py and
tests/block16_ef_ref.py on the whole bucket.  A NaN compares equal to a NaN
whatever its payload; every other lane by its bits.

Each n is the first cap of its kernel plus a remainder that makes a partial
last block and an odd count.  The caps are read from the launch code
(grid_of(items, per_group, 8) of inccl_launch.h: at most 8 workgroups a CU);
CUs is torch's multi_processor_count, the count num_cus() caches.  Update the
sizes with the geometry, in the same commit:

  k_block_absmax       launch_absmax (inccl_block.hip): grid_of(blocks, kBlkWaves
  k_block_fused_elem   = 4, 8) -> 32 * CUs blocks = 8192 * CUs elements (launch_fused's
                       element branch has the same grid); n = 8192 * CUs + 5 * 256 + 37
  k_stream_block       launch_stream: grid_of(quads, B = 512, 8) -> 16384 * CUs
                       elements; n = 16384 * CUs + 4 * 100 + 3
  k_stream_block_elem  grid_of(elements, kBlock = 256, 8) -> 2048 * CUs;
  k_unpack_block_elem  n = 2048 * CUs + 1003
  k_pack_block         launch_pack (inccl_pack.hip): grid_of(tiles of 512
                       elements, B / 64 = 8, 8) -> 32768 * CUs elements;
                       n = 32768 * CUs + 3 * 512 + 37
  k_pack_block_elem    grid_of(words, kBlock = 256, 8) -> 4096 * CUs elements;
                       n = 4096 * CUs + 2 * 1003 + 1
  k_unpack_block       launch_unpack: grid_of(groups of 8 elements, B = 512, 8)
                       -> 32768 * CUs elements; n = 32768 * CUs + 8 * 100 + 5

k_stream_block_fused launches one workgroup per tile with no cap
(launch_fused: grid_capped(.., kNoCap)): its loop cannot take a second pass and
the sizes of the existing block tests cover its tiles, so it has no size here.
k_words_max has no public entry of its own; the comm tests run it.

The buckets are block_ref.mixed_buckets with a zero block and, in the
second-pass region, a block that holds an Inf and a NaN (flagged where the
non-finite flag applies).  Every output, the residuals included, is a view of
a larger allocation prefilled with a sentinel; both guards are checked."""
import functools

import numpy as np
import pytest

import block16_ef_ref as ef
import block16_ref
import block_ref

pytestmark = pytest.mark.gpu

G = 64                      # guard elements either side: 256 B, the view keeps the allocation's alignment
SENT = 0x5A5A5A5A
KIND_F32, KIND_Q32, KIND_P16 = 0, 1, 5


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


class _Buf:
    """n 4-byte elements on the GPU, `shift` elements past a 16-B boundary,
    inside an allocation whose other elements hold a sentinel: `init` (fp32,
    int32 or uint32) or the sentinel throughout"""

    def __init__(self, dev, n, init=None, shift=0):
        import torch
        host = np.full(G + shift + n + G, SENT, np.uint32)
        if init is not None:
            host[G + shift:G + shift + n] = np.ascontiguousarray(init).view(np.uint32)
        self.n, self.lo = n, G + shift
        self.raw = torch.from_numpy(host.view(np.int32)).to(dev)
        self.i32 = self.raw[self.lo:self.lo + n]
        self.f32 = self.i32.view(torch.float32)
        assert self.i32.data_ptr() % 16 == 4 * shift % 16

    def bits(self):
        """the n elements as uint32, after checking both guards"""
        import torch
        torch.cuda.synchronize()
        host = self.raw.cpu().numpy().view(np.uint32)
        assert (host[:self.lo] == SENT).all(), "written before the output"
        assert (host[self.lo + self.n:] == SENT).all(), "written past n"
        return host[self.lo:self.lo + self.n].copy()

    def floats(self):
        return self.bits().view(np.float32)


def _same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn])


def _buckets(n, R, zero_block, bad_block, seed=0):
    """mixed buckets of n elements with a zero block and a block that holds an
    Inf (bucket 0) and a NaN (the last bucket)"""
    assert 256 * bad_block + 71 <= n and zero_block != bad_block
    bufs = block_ref.mixed_buckets(np.random.default_rng(seed), n, R, zero_block=zero_block)
    bufs[0][256 * bad_block + 5] = np.float32(np.inf)
    bufs[R - 1][256 * bad_block + 70] = np.float32(np.nan)
    return bufs


def _nan_blocks(want, words, n, elem_base=0):
    """block_ref's rule "a flagged block is NaN" on a result computed per block"""
    blk = (elem_base + np.arange(n)) // 256
    out = want.copy()
    out[(words[blk] >> 31) != 0] = np.nan
    return out


def _first_residuals(orc, bufs, R):
    """the residuals an earlier step from zero residuals leaves (ef.step without its result)"""
    vs = ef.add(bufs, ef.zeros_like(bufs))
    words = block_ref.block_words(orc, vs)
    ks16 = block16_ref.block_scales16(orc, words, R)
    res = [ef.residual(orc, v, words, ks16, R)[0] for v in vs]
    assert all(e.any() for e in res)
    return res


# ---- k_block_absmax ----
@functools.lru_cache(maxsize=None)
def _absmax_case(R):
    cap = 8192 * _cus()
    n = cap + 5 * 256 + 37
    b0 = cap // 256                       # the first block of the second pass; b0 + 1 zero, b0 + 3 flagged
    bufs = _buckets(n, R, b0 + 1, b0 + 3)
    orc = _orc()
    words, flagged = block_ref.block_words(orc, bufs), block_ref.block_words(orc, bufs, True)
    assert words[b0 + 1] == 0 and flagged[b0 + 3] >> 31 and not (flagged[:b0 + 3] >> 31).any()
    return bufs, n, words, flagged


def test_block_absmax_aligned(gpu):
    """R = 3, the quad branch, with and without the non-finite flag"""
    from container_inc_amd import inccl
    bufs, n, words, flagged = _absmax_case(3)
    ts = [_Buf(gpu, n, x) for x in bufs]
    for flag, want in ((False, words), (True, flagged)):
        w = _Buf(gpu, block_ref.nblocks(n))
        inccl.block_absmax([t.f32 for t in ts], words=w.i32, nonfinite_flag=flag)
        np.testing.assert_array_equal(w.bits(), want)


def test_block_absmax_unaligned(gpu):
    """R = 2, every bucket one element past 16 B: the element branch"""
    from container_inc_amd import inccl
    bufs, n, words, flagged = _absmax_case(2)
    ts = [_Buf(gpu, n, x, shift=1) for x in bufs]
    for flag, want in ((False, words), (True, flagged)):
        w = _Buf(gpu, block_ref.nblocks(n))
        inccl.block_absmax([t.f32 for t in ts], words=w.i32, nonfinite_flag=flag)
        np.testing.assert_array_equal(w.bits(), want)


def test_block_absmax_with_residuals(gpu):
    """R = 2, block_absmax_ef: the words of bucket + residual, the residuals only read"""
    from container_inc_amd import inccl
    orc = _orc()
    bufs, n, _, _ = _absmax_case(2)
    res = _first_residuals(orc, bufs, 2)
    vs = ef.add(bufs, res)
    ts, rs = [_Buf(gpu, n, x) for x in bufs], [_Buf(gpu, n, e) for e in res]
    for flag in (False, True):
        w = _Buf(gpu, block_ref.nblocks(n))
        inccl.block_absmax_ef([t.f32 for t in ts], [r.f32 for r in rs], words=w.i32, nonfinite_flag=flag)
        np.testing.assert_array_equal(w.bits(), block_ref.block_words(orc, vs, flag))
    for r, e in zip(rs, res):
        np.testing.assert_array_equal(r.bits(), e.view(np.uint32))


# ---- k_block_fused_elem ----
@pytest.mark.parametrize("flag", [False, True], ids=["saturate", "flag"])
@pytest.mark.parametrize("p16", [False, True], ids=["plain", "p16"])
def test_fused_elem(gpu, p16, flag):
    """R = 2, every pointer one element past 16 B, the words written out:
    reduce_f32_block and reduce_f32_block16"""
    from container_inc_amd import inccl
    orc = _orc()
    bufs, n, words, flagged = _absmax_case(2)
    if p16:
        want, _ = block16_ref.reduce_f32_block16(orc, bufs, 2, nonfinite_nan=flag)
    else:
        want, _ = block_ref.reduce_f32_block(orc, bufs, 2, nonfinite_nan=flag)
    ts = [_Buf(gpu, n, x, shift=1) for x in bufs]
    out, w = _Buf(gpu, n, shift=1), _Buf(gpu, block_ref.nblocks(n))
    fn = inccl.reduce_f32_block16 if p16 else inccl.reduce_f32_block
    fn([t.f32 for t in ts], out=out.f32, words=w.i32, nonfinite_flag=flag)
    _same(out.floats(), want)
    np.testing.assert_array_equal(w.bits(), flagged if flag else words)


def test_fused_elem_with_error_feedback(gpu):
    """R = 1, reduce_f32_block16_ef unaligned, from the residuals of an earlier
    step, with the flag: the result, the words and every residual; the second
    pass rewrites its blocks' residuals and zeroes the flagged block's"""
    from container_inc_amd import inccl
    orc = _orc()
    bufs, n, _, _ = _absmax_case(1)
    cap = 8192 * _cus()
    res = _first_residuals(orc, bufs, 1)
    y, new, _ = ef.step(orc, bufs, res, 1, nonfinite_nan=True)
    flagged = slice(cap + 3 * 256, cap + 4 * 256)
    assert res[0][flagged].any() and not new[0][flagged].any()             # zeroed there
    ordinary = slice(cap, cap + 256)
    assert (new[0][ordinary] != res[0][ordinary]).any()                    # rewritten there
    t, r = _Buf(gpu, n, bufs[0], shift=1), _Buf(gpu, n, res[0], shift=1)
    out, w = _Buf(gpu, n, shift=1), _Buf(gpu, block_ref.nblocks(n))
    inccl.reduce_f32_block16_ef([t.f32], [r.f32], out=out.f32, words=w.i32, nonfinite_flag=True)
    _same(out.floats(), y)
    np.testing.assert_array_equal(w.bits(), block_ref.block_words(orc, ef.add(bufs, res), True))
    _same(r.floats(), new[0])
    np.testing.assert_array_equal(t.bits(), bufs[0].view(np.uint32))


# ---- k_stream_block and k_stream_block_elem ----
def _stream_block_case(gpu, n, first_cap, elem_base, shift, zero_block, bad_after):
    """F32 -> Q32 of R = 2 buckets (each alone, then both) and Q32 -> F32 of the
    two partials, on the n elements from elem_base of a bucket of elem_base + n,
    at the bucket's flagged words; the flagged block is bad_after blocks past the
    one the second pass starts in"""
    from container_inc_amd import inccl
    orc = _orc()
    R, N = 2, elem_base + n
    bs = (elem_base + first_cap) // 256    # the bucket's block that holds the second pass's first element
    bufs = _buckets(N, R, zero_block, bs + bad_after)
    words = block_ref.block_words(orc, bufs, True)
    ks = block_ref.block_scales(orc, words, R)
    wt = _Buf(gpu, words.size, words)
    cut = [x[elem_base:] for x in bufs]
    ts = [_Buf(gpu, n, c, shift=shift) for c in cut]
    want_parts = [block_ref.quant_sum_block(orc, [c], ks, elem_base) for c in cut]
    parts = []
    for t, want in zip(ts, want_parts):
        q = _Buf(gpu, n, shift=shift)
        inccl.stream_op_block(KIND_F32, KIND_Q32, [t.f32], wt.i32, out=q.i32, elem_base=elem_base, scale_R=R)
        np.testing.assert_array_equal(q.bits(), want.view(np.uint32))
        parts.append(q)
    q = _Buf(gpu, n, shift=shift)
    inccl.stream_op_block(KIND_F32, KIND_Q32, [t.f32 for t in ts], wt.i32, out=q.i32, elem_base=elem_base)
    np.testing.assert_array_equal(q.bits(), block_ref.quant_sum_block(orc, cut, ks, elem_base).view(np.uint32))
    out = _Buf(gpu, n, shift=shift)
    inccl.stream_op_block(KIND_Q32, KIND_F32, [p.i32 for p in parts], wt.i32, out=out.f32, elem_base=elem_base,
                          scale_R=R)
    want = _nan_blocks(block_ref.sum_dequant_block(orc, want_parts, ks, elem_base), words, n, elem_base)
    assert np.isnan(want[first_cap:]).any() and not np.isnan(want[:first_cap]).any()
    _same(out.floats(), want)
    np.testing.assert_array_equal(wt.bits(), words)


@pytest.mark.parametrize("elem_base", [0, 256])
def test_stream_block(gpu, elem_base):
    """aligned, elem_base % 4 == 0: k_stream_block past 16384 * CUs elements"""
    cap = 16384 * _cus()
    _stream_block_case(gpu, cap + 4 * 100 + 3, cap, elem_base, 0, zero_block=4, bad_after=1)


@pytest.mark.parametrize("elem_base,shift", [(0, 1), (3, 0)], ids=["unaligned", "elem_base3"])
def test_stream_block_elem(gpu, elem_base, shift):
    """unaligned pointers, or elem_base = 3: k_stream_block_elem past 2048 * CUs elements"""
    cap = 2048 * _cus()
    _stream_block_case(gpu, cap + 1003, cap, elem_base, shift, zero_block=cap // 256 + 1, bad_after=2)


# ---- k_pack_block and k_unpack_block ----
@functools.lru_cache(maxsize=None)
def _pack_case():
    """R = 2 buckets of 32768 * CUs + 3 * 512 + 37 elements, their flagged words
    and exponents, each bucket's packed words alone and the packed local sum"""
    orc = _orc()
    cap = 32768 * _cus()
    n = cap + 3 * 512 + 37
    bufs = _buckets(n, 2, cap // 256 + 1, cap // 256 + 3)
    words = block_ref.block_words(orc, bufs, True)
    ks16 = block16_ref.block_scales16(orc, words, 2)
    parts = [block16_ref.pack_quant_sum(orc, [x], ks16, 2) for x in bufs]
    # pack_quant_sum of both buckets is by its definition the wrap-around sum of the two buckets' words
    return bufs, n, words, ks16, parts, orc.sum_q32(parts)


def test_pack_block(gpu):
    """F32 -> P16 aligned: k_pack_block past 32768 * CUs elements (the last 37 elements: k_pack_block_elem)"""
    from container_inc_amd import inccl
    bufs, n, words, _, _, packed = _pack_case()
    wt = _Buf(gpu, words.size, words)
    ts = [_Buf(gpu, n, x) for x in bufs]
    out = _Buf(gpu, (n + 1) // 2)
    inccl.stream_op_block(KIND_F32, KIND_P16, [t.f32 for t in ts], wt.i32, out=out.i32, scale_R=2)
    np.testing.assert_array_equal(out.bits(), packed.view(np.uint32))


def test_unpack_block(gpu):
    """P16 -> F32 aligned, elem_base 0: k_unpack_block past 32768 * CUs elements,
    on the first 32768 * CUs + 8 * 100 + 5 elements of the packed buckets"""
    from container_inc_amd import inccl
    orc = _orc()
    _, _, words, ks16, parts, _ = _pack_case()
    cap = 32768 * _cus()
    n = cap + 8 * 100 + 5
    srcs = [p[:(n + 1) // 2] for p in parts]
    want = block16_ref.unpack_dequant(orc, srcs, ks16, n, nan_blocks=words >> 31)
    assert np.isnan(want[cap:]).any() and not np.isnan(want[:cap]).any()
    wt = _Buf(gpu, words.size, words)
    ts = [_Buf(gpu, s.size, s) for s in srcs]
    out = _Buf(gpu, n)
    inccl.stream_op_block(KIND_P16, KIND_F32, [t.i32 for t in ts], wt.i32, out=out.f32, n=n, scale_R=2)
    _same(out.floats(), want)


def test_pack_block_with_error_feedback(gpu):
    """pack_block16_ef at R = 1 from the residuals of an earlier step, at the
    flagged words of bucket + residual: the words and the residual, which the
    second-pass tiles rewrite (zero in the flagged block)"""
    from container_inc_amd import inccl
    orc = _orc()
    bufs, n, _, _, _, _ = _pack_case()
    bufs = bufs[:1]
    cap = 32768 * _cus()
    res = _first_residuals(orc, bufs, 1)
    vs = ef.add(bufs, res)
    words = block_ref.block_words(orc, vs, True)
    ks16 = block16_ref.block_scales16(orc, words, 1)
    new = ef.residual(orc, vs[0], words, ks16, 1)[0]
    flagged = slice(cap + 3 * 256, cap + 4 * 256)
    assert res[0][flagged].any() and not new[flagged].any()
    tile = slice(cap, cap + 256)
    assert (new[tile] != res[0][tile]).any()
    wt = _Buf(gpu, words.size, words)
    t, r = _Buf(gpu, n, bufs[0]), _Buf(gpu, n, res[0])
    out = _Buf(gpu, (n + 1) // 2)
    inccl.pack_block16_ef([t.f32], [r.f32], wt.i32, out=out.i32, scale_R=1)
    np.testing.assert_array_equal(out.bits(), block16_ref.pack_quant_sum(orc, vs, ks16, 1).view(np.uint32))
    _same(r.floats(), new)
    np.testing.assert_array_equal(t.bits(), bufs[0].view(np.uint32))


# ---- k_pack_block_elem and k_unpack_block_elem ----
@pytest.mark.parametrize("elem_base,shift", [(0, 1), (2, 0)], ids=["unaligned", "elem_base2"])
def test_pack_block_elem(gpu, elem_base, shift):
    """unaligned pointers, or elem_base = 2: k_pack_block_elem past 4096 * CUs elements (2048 * CUs words)"""
    from container_inc_amd import inccl
    orc = _orc()
    cap = 4096 * _cus()
    n = cap + 2 * 1003 + 1
    bufs = _buckets(elem_base + n, 2, cap // 256 + 1, cap // 256 + 3)
    words = block_ref.block_words(orc, bufs, True)
    ks16 = block16_ref.block_scales16(orc, words, 2)
    cut = [x[elem_base:] for x in bufs]
    wt = _Buf(gpu, words.size, words)
    ts = [_Buf(gpu, n, c, shift=shift) for c in cut]
    out = _Buf(gpu, (n + 1) // 2, shift=shift)
    inccl.stream_op_block(KIND_F32, KIND_P16, [t.f32 for t in ts], wt.i32, out=out.i32, elem_base=elem_base, scale_R=2)
    np.testing.assert_array_equal(out.bits(), block16_ref.pack_quant_sum(orc, cut, ks16, 2, elem_base).view(np.uint32))


@pytest.mark.parametrize("elem_base,shift", [(0, 1), (3, 0)], ids=["unaligned", "elem_base3"])
def test_unpack_block_elem(gpu, elem_base, shift):
    """unaligned pointers, or an odd elem_base (the sources start at the word
    that holds element 3; its low lane is skipped): k_unpack_block_elem past
    2048 * CUs elements"""
    from container_inc_amd import inccl
    orc = _orc()
    cap = 2048 * _cus()
    n = cap + 1003
    bufs = _buckets(elem_base + n, 2, cap // 256 + 1, cap // 256 + 2)
    words = block_ref.block_words(orc, bufs, True)
    ks16 = block16_ref.block_scales16(orc, words, 2)
    pb = elem_base & ~1
    parts = [block16_ref.pack_quant_sum(orc, [x[pb:]], ks16, 2, pb) for x in bufs]
    want = block16_ref.unpack_dequant(orc, parts, ks16, n, elem_base, nan_blocks=words >> 31)
    assert np.isnan(want[cap:]).any() and not np.isnan(want[:cap]).any()
    wt = _Buf(gpu, words.size, words)
    ts = [_Buf(gpu, p.size, p, shift=shift) for p in parts]
    out = _Buf(gpu, n, shift=shift)
    inccl.stream_op_block(KIND_P16, KIND_F32, [t.i32 for t in ts], wt.i32, out=out.f32, elem_base=elem_base, n=n,
                          scale_R=2)
    _same(out.floats(), want)
