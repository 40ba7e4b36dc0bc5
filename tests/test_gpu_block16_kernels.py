"""Packed 16-bit lanes, the stateless kernels (gpu): inccl_stream_op_block's
F32 -> P16 and P16 -> F32 pairs and inccl_reduce_f32_block16 against the CPU
reference tests/block16_ref.py, bit-exact.  A NaN compares equal to a NaN
whatever its payload; every other lane by its bits.

Sizes: 37 (one partial block, an odd n: the last word's high lane is zero),
2341 (nine blocks and a partial one, less than one tile) and 10533 = 2 * 4096 +
2341 (full tiles, a ragged one, the tail).  The buckets are
block_ref.mixed_buckets(default_rng(0), ..., zero_block=4) where block 4 exists."""
import functools

import numpy as np
import pytest

import block16_ref
import block_ref

pytestmark = pytest.mark.gpu

RS = [1, 2, 3, 8]
NS = [37, 2341, 10533]


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    np.testing.assert_array_equal(got.view(np.uint32)[~wn], want.view(np.uint32)[~wn])


def _off1(x, dev):
    """x on the GPU starting 4 bytes into an allocation: not 16-B aligned"""
    return _t(np.concatenate([np.zeros(1, x.dtype), x]), dev)[1:]


@functools.lru_cache(maxsize=None)
def _case(R, n):
    """the buckets and their reference, computed once per (R, n)"""
    from oracle import oracle as orc
    orc.build()
    bufs = block_ref.mixed_buckets(np.random.default_rng(0), n, R, zero_block=4 if block_ref.nblocks(n) > 4 else None)
    words = block_ref.block_words(orc, bufs)
    ks = block16_ref.block_scales16(orc, words, R)
    want, ks2 = block16_ref.reduce_f32_block16(orc, bufs, R)
    assert ks2 == ks
    return bufs, want, ks, words, block16_ref.pack_quant_sum(orc, bufs, ks, R)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_pack_and_unpack(gpu, orc, R, n):
    """F32 -> P16: the local sum's words; P16 -> F32 of one source (the sum) and,
    from three buckets on, of three (each the packed local sum of a group of
    buckets); then the same with every source and dst 4 bytes into its
    allocation, which takes the element kernels"""
    from container_inc_amd import inccl
    bufs, want, ks, words, packed = _case(R, n)
    wt = _t(words.view(np.int32), gpu)
    groups = [bufs[i::3] for i in range(3)] if R >= 3 else []
    for put in (_t, _off1):
        ts = [put(x, gpu) for x in bufs]
        out = put(np.full((n + 1) // 2, -1, np.int32), gpu)
        got = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, ts, wt, out=out, scale_R=R)
        assert got.numel() == (n + 1) // 2
        np.testing.assert_array_equal(_np(got), packed)
        if n % 2:
            assert block16_ref.unpack(_np(got)[-1:])[1] == 0     # the zero high lane of the last word
        fout = put(np.full(n, 7.0, np.float32), gpu)
        _same(_np(inccl.stream_op_block(inccl.KIND_P16, inccl.KIND_F32, [put(packed, gpu)], wt, out=fout, n=n,
                                        scale_R=R)), want)
        if groups:
            parts = [block16_ref.pack_quant_sum(orc, g, ks, R) for g in groups]
            gparts = [inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, [put(x, gpu) for x in g], wt, scale_R=R)
                      for g in groups]
            for gp, p in zip(gparts, parts):
                np.testing.assert_array_equal(_np(gp), p)
            _same(_np(inccl.stream_op_block(inccl.KIND_P16, inccl.KIND_F32, [put(p, gpu) for p in parts], wt, n=n,
                                            scale_R=R)), want)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_reduce_f32_block16(gpu, R, n):
    import torch
    from container_inc_amd import inccl
    bufs, want, _, words, _ = _case(R, n)
    ts = [_t(x, gpu) for x in bufs]
    _same(_np(inccl.reduce_f32_block16(ts)), want)
    w = torch.full((block_ref.nblocks(n),), -1, dtype=torch.int32, device=gpu)
    _same(_np(inccl.reduce_f32_block16(ts, words=w)), want)
    np.testing.assert_array_equal(_np(w).view(np.uint32), words)
    # sources and dst one element into their allocations: the element-granular kernel
    w = torch.full((block_ref.nblocks(n),), -1, dtype=torch.int32, device=gpu)
    out = _off1(np.full(n, 7.0, np.float32), gpu)
    _same(_np(inccl.reduce_f32_block16([_off1(x, gpu) for x in bufs], out=out, words=w)), want)
    np.testing.assert_array_equal(_np(w).view(np.uint32), words)


def test_reduce_f32_block16_in_place(gpu):
    """dst may alias srcs[0]"""
    from container_inc_amd import inccl
    bufs, want, _, _, _ = _case(3, 10533)
    ts = [_t(x, gpu) for x in bufs]
    _same(_np(inccl.reduce_f32_block16(ts, out=ts[0])), want)


def test_the_32_bit_form_is_unchanged_beside_it(gpu, orc):
    """the same buckets through inccl_reduce_f32_block: block_ref's result, not the lanes'"""
    from container_inc_amd import inccl
    bufs, want16, _, _, _ = _case(3, 2341)
    want32, _ = block_ref.reduce_f32_block(orc, bufs, 3)
    assert not np.array_equal(want16, want32)
    _same(_np(inccl.reduce_f32_block([_t(x, gpu) for x in bufs])), want32)


@pytest.mark.parametrize("copy", [False, True], ids=["view", "copy"])
@pytest.mark.parametrize("elem_base", [0, 256, 128, 64, 2, 3])
def test_stream_op_block_at_an_offset(gpu, orc, elem_base, copy):
    """The sharded route's stages on a 1500-element cut of the 2341-element
    bucket: each rank's partial packed from the even element at or before
    elem_base, the local sum of the three, and the partials summed and
    dequantised from elem_base on (3: the first word's low lane is skipped) --
    that slice of the whole bucket's result.  view: the cut is a slice of the
    bucket's tensor; copy: a tensor of its own."""
    from container_inc_amd import inccl
    R, n = 3, 1500
    bufs, whole, ks, words, _ = _case(R, 2341)
    wt = _t(words.view(np.int32), gpu)
    pb = elem_base & ~1
    cut = [x[pb:elem_base + n] for x in bufs]
    cts = [_t(c, gpu) for c in cut] if copy else [_t(x, gpu)[pb:elem_base + n] for x in bufs]
    parts = [inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, [c], wt, elem_base=pb, scale_R=R) for c in cts]
    want_parts = [block16_ref.pack_quant_sum(orc, [c], ks, R, pb) for c in cut]
    for p, w in zip(parts, want_parts):
        np.testing.assert_array_equal(_np(p), w)
    local = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, cts, wt, elem_base=pb, scale_R=R)
    np.testing.assert_array_equal(_np(local), block16_ref.pack_quant_sum(orc, cut, ks, R, pb))
    got = inccl.stream_op_block(inccl.KIND_P16, inccl.KIND_F32, parts, wt, elem_base=elem_base, n=n, scale_R=R)
    _same(_np(got), block16_ref.unpack_dequant(orc, want_parts, ks, n, elem_base))
    _same(_np(got), whole[elem_base:elem_base + n])


def test_pack_refuses_an_odd_elem_base(gpu):
    import torch
    from container_inc_amd import inccl
    from container_inc_amd._lib import IncclError
    x = torch.ones(512, dtype=torch.float32, device=gpu)
    w = torch.zeros(3, dtype=torch.int32, device=gpu)
    out = torch.full((256,), 7, dtype=torch.int32, device=gpu)
    with pytest.raises(IncclError, match=r"rc=-1.*odd elem_base"):
        inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, [x], w, out=out, elem_base=3)
    assert (_np(out) == 7).all()
    for pair in ((inccl.KIND_Q32, inccl.KIND_P16), (inccl.KIND_P16, inccl.KIND_Q32), (inccl.KIND_P16, inccl.KIND_P16)):
        with pytest.raises(IncclError, match="rc=-1"):
            inccl.stream_op_block(pair[0], pair[1], [out], w, out=torch.empty_like(out), n=256)


def test_nonfinite_is_per_block(gpu, orc):
    """+Inf in block 2 of buckets 0 and 1: the saturating spec gives that block
    INCCL_SCALE_MIN and +-L per Inf contributor, scaled, with no spill into the
    neighbouring lane; the flag makes that block NaN; every other block is
    bit-identical to the clean result in both modes, through the fused kernel
    and through the two stages"""
    from container_inc_amd import inccl
    R, n = 3, 2341
    bufs, clean, _, _, _ = _case(R, n)
    bad = [x.copy() for x in bufs]
    bad[0][256 * 2 + 5] = bad[1][256 * 2 + 5] = np.float32(np.inf)
    bad[2][256 * 2 + 6] = np.float32(-np.inf)
    bad[2][256 * 2 + 8] = np.float32(np.nan)
    sat, ks = block16_ref.reduce_f32_block16(orc, bad, R)
    nan, ks_nan = block16_ref.reduce_f32_block16(orc, bad, R, nonfinite_nan=True)
    blk = np.arange(n) // 256 == 2
    L = block16_ref.lane_clamp(R)
    assert ks[2] == -64 and np.isnan(nan[blk]).all() and np.isfinite(sat).all()
    # the flagged word of block 2 is the NaN's (the largest flagged word): the rule gives it the zero
    # block's exponent, every lane of the block saturates at L per contributor and still sums inside a lane
    assert ks_nan[2] == 48 and ks_nan[:2] + ks_nan[3:] == ks[:2] + ks[3:]
    assert sat[256 * 2 + 5] == np.float32(2 * L) * np.float32(2.0 ** 64) and sat[256 * 2 + 4] == 0
    assert sat[256 * 2 + 6] == np.float32(-L) * np.float32(2.0 ** 64) and sat[256 * 2 + 7] == 0
    ts = [_t(x, gpu) for x in bad]
    got_sat = _np(inccl.reduce_f32_block16(ts))
    got_nan = _np(inccl.reduce_f32_block16(ts, nonfinite_flag=True))
    _same(got_sat, sat)
    _same(got_nan, nan)
    _same(got_sat[~blk], clean[~blk])
    _same(got_nan[~blk], clean[~blk])
    for flag, want, kk in ((False, sat, ks), (True, nan, ks_nan)):
        w = inccl.block_absmax(ts, nonfinite_flag=flag)
        q = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, ts, w, scale_R=R)
        np.testing.assert_array_equal(_np(q), block16_ref.pack_quant_sum(orc, bad, kk, R))
        _same(_np(inccl.stream_op_block(inccl.KIND_P16, inccl.KIND_F32, [q], w, n=n, scale_R=R)), want)
