"""Per-block auto scaling, the stateless kernels (gpu): inccl_block_absmax_f32,
inccl_reduce_f32_block and inccl_stream_op_block against the CPU reference
tests/block_ref.py, bit-exact.  A NaN compares equal to a NaN whatever its
payload (the spec says "that block is NaN"); every other lane by its bits.

Sizes: 37 (one partial block, a scalar tail with n % 4 = 1), 2341 (nine blocks
and a partial one, less than one tile) and 10533 = 2 * 4096 + 2341 (full tiles
of every geometry, a ragged tile, the tail).  The buckets are
block_ref.mixed_buckets(default_rng(0), ..., zero_block=4) where block 4 exists
(n = 37 has one block, so no zero block there)."""
import functools

import numpy as np
import pytest

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


def _words(t):
    return _np(t).view(np.uint32)


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
    want, ks = block_ref.reduce_f32_block(orc, bufs, R)
    return bufs, want, ks, block_ref.block_words(orc, bufs), block_ref.block_words(orc, bufs, True)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_block_absmax_words(gpu, R, n):
    from container_inc_amd import inccl
    bufs, _, _, words, flagged = _case(R, n)
    ts = [_t(x, gpu) for x in bufs]
    np.testing.assert_array_equal(_words(inccl.block_absmax(ts)), words)
    np.testing.assert_array_equal(_words(inccl.block_absmax(ts, nonfinite_flag=True)), flagged)
    np.testing.assert_array_equal(_words(inccl.block_absmax([_off1(x, gpu) for x in bufs])), words)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_reduce_f32_block(gpu, R, n):
    import torch
    from container_inc_amd import inccl
    bufs, want, ks, words, _ = _case(R, n)
    ts = [_t(x, gpu) for x in bufs]
    _same(_np(inccl.reduce_f32_block(ts)), want)
    w = torch.full((block_ref.nblocks(n),), -1, dtype=torch.int32, device=gpu)
    _same(_np(inccl.reduce_f32_block(ts, words=w)), want)
    np.testing.assert_array_equal(_words(w), words)
    assert [inccl.choose_scale_word(int(x), R)[0] for x in _words(w)] == ks


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_reduce_f32_block_unaligned_sources(gpu, R, n):
    """sources one element into their allocations: the element-granular kernel"""
    import torch
    from container_inc_amd import inccl
    bufs, want, _, words, _ = _case(R, n)
    w = torch.full((block_ref.nblocks(n),), -1, dtype=torch.int32, device=gpu)
    _same(_np(inccl.reduce_f32_block([_off1(x, gpu) for x in bufs], words=w)), want)
    np.testing.assert_array_equal(_words(w), words)


def test_reduce_f32_block_in_place(gpu):
    """dst may alias srcs[0]"""
    from container_inc_amd import inccl
    bufs, want, _, _, _ = _case(3, 10533)
    ts = [_t(x, gpu) for x in bufs]
    _same(_np(inccl.reduce_f32_block(ts, out=ts[0])), want)


@pytest.mark.parametrize("copy", [False, True], ids=["view", "copy"])
@pytest.mark.parametrize("elem_base", [0, 256, 128, 64, 4, 3])
def test_stream_op_block_at_an_offset(gpu, orc, elem_base, copy):
    """The sharded route's stages on a 1500-element cut of the 2341-element
    bucket: each rank's partial quantised at its blocks' exponents (F32 -> Q32),
    the local sum of the three, and the partials summed and dequantised
    (Q32 -> F32) -- that slice of the whole bucket's result.  view: the cut is a
    slice of the bucket's tensor (elem_base = 3: not 16-B aligned); copy: a
    tensor of its own (elem_base = 3: aligned, the block offset alone selects
    the element kernel)."""
    from container_inc_amd import inccl
    R, n = 3, 1500
    bufs, whole, ks, words, _ = _case(R, 2341)
    wt = _t(words.view(np.int32), gpu)
    cut = [x[elem_base:elem_base + n] for x in bufs]
    if copy:
        cts = [_t(c, gpu) for c in cut]
    else:
        cts = [_t(x, gpu)[elem_base:elem_base + n] for x in bufs]
    parts = [inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_Q32, [c], wt, elem_base=elem_base, scale_R=R)
             for c in cts]
    want_parts = [block_ref.quant_sum_block(orc, [c], ks, elem_base) for c in cut]
    for p, w in zip(parts, want_parts):
        np.testing.assert_array_equal(_np(p), w)
    local = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_Q32, cts, wt, elem_base=elem_base)
    np.testing.assert_array_equal(_np(local), block_ref.quant_sum_block(orc, cut, ks, elem_base))
    got = inccl.stream_op_block(inccl.KIND_Q32, inccl.KIND_F32, parts, wt, elem_base=elem_base, scale_R=R)
    _same(_np(got), block_ref.sum_dequant_block(orc, want_parts, ks, elem_base))
    _same(_np(got), whole[elem_base:elem_base + n])


def test_equal_absmax_blocks_give_the_single_scale_result(gpu, orc):
    from container_inc_amd import inccl
    rng = np.random.default_rng(1)
    n = 256 * 4 + 100
    bufs = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(2)]
    for b in range(block_ref.nblocks(n)):
        bufs[b % 2][256 * b + 7] = np.float32(-3.0)
    k = orc.choose_scale(orc.absmax(bufs), 2)
    ts = [_t(x, gpu) for x in bufs]
    got = _np(inccl.reduce_f32_block(ts))
    _same(got, orc.reduce_f32(bufs, k))
    _same(got, _np(inccl.reduce_f32(ts, k)))
    np.testing.assert_array_equal(_words(inccl.block_absmax(ts)),
                                  np.full(block_ref.nblocks(n), np.array([3.0], np.float32).view(np.uint32)[0], np.uint32))


def _edge_amaxes(R):
    """block absmaxes on the edges of the scale rule for R contributors: 0, the
    smallest subnormal, 2^j / R (exact for a power-of-two R: the m == 0.5
    branch; else the fp32 nearest to it) with its neighbours one ulp either
    side, the largest finite value and +Inf"""
    out = [np.float32(0.0), np.float32(1e-45), np.finfo(np.float32).max, np.float32(np.inf)]
    for j in (-120, -20, 0, 3, 30, 100):
        v = np.float32(2.0 ** j / R)
        out += [np.nextafter(v, np.float32(0.0)), v, np.nextafter(v, np.float32(np.inf))]
    return out


@pytest.mark.parametrize("R", RS)
def test_scale_edges(gpu, orc, R):
    from container_inc_amd import inccl
    amax = _edge_amaxes(R)
    nb = len(amax)
    n = 256 * nb - 100                        # the last block (2^100 / R + 1 ulp) is partial
    rng = np.random.default_rng(R)
    bufs = [np.zeros(n, np.float32) for _ in range(R)]
    with np.errstate(over="ignore", invalid="ignore"):
        for b, a in enumerate(amax):
            sl = slice(256 * b, min(n, 256 * b + 256))
            m = np.float64(a) if np.isfinite(a) else 1.0
            for x in bufs:
                x[sl] = (rng.uniform(-0.99, 0.99, sl.stop - sl.start) * m).astype(np.float32)
            bufs[b % R][256 * b + (37 * b) % 150] = -a if b % 2 else a
    words = block_ref.block_words(orc, bufs)
    np.testing.assert_array_equal(words, np.array(amax, np.float32).view(np.uint32))
    want, ks = block_ref.reduce_f32_block(orc, bufs, R)
    assert ks == [orc.choose_scale(float(a), R) for a in amax]
    ts = [_t(x, gpu) for x in bufs]
    import torch
    w = torch.zeros(nb, dtype=torch.int32, device=gpu)
    got = _np(inccl.reduce_f32_block(ts, words=w))
    np.testing.assert_array_equal(_words(w), words)
    assert [inccl.choose_scale_word(int(x), R)[0] for x in _words(w)] == ks
    _same(got, want)
    # the same exponents through the two-stage kernels
    q = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_Q32, ts, w)
    np.testing.assert_array_equal(_np(q), block_ref.quant_sum_block(orc, bufs, ks))
    _same(_np(inccl.stream_op_block(inccl.KIND_Q32, inccl.KIND_F32, [q], w, scale_R=R)), want)


def test_nonfinite_is_per_block(gpu, orc):
    """+Inf in block 2 of bucket 1: the saturating spec gives that block
    INCCL_SCALE_MIN, the flag makes that block NaN; every other block is
    bit-identical to the clean result in both modes."""
    from container_inc_amd import inccl
    R, n = 3, 2341
    bufs, clean, _, _, _ = _case(R, n)
    bad = [x.copy() for x in bufs]
    bad[1][256 * 2 + 5] = np.float32(np.inf)
    sat, ks = block_ref.reduce_f32_block(orc, bad, R)
    nan, _ = block_ref.reduce_f32_block(orc, bad, R, nonfinite_nan=True)
    blk = np.arange(n) // 256 == 2
    assert ks[2] == -64 and np.isnan(nan[blk]).all() and np.isfinite(sat).all()
    ts = [_t(x, gpu) for x in bad]
    got_sat = _np(inccl.reduce_f32_block(ts))
    got_nan = _np(inccl.reduce_f32_block(ts, nonfinite_flag=True))
    _same(got_sat, sat)
    _same(got_nan, nan)
    _same(got_sat[~blk], clean[~blk])
    _same(got_nan[~blk], clean[~blk])
    np.testing.assert_array_equal(_words(inccl.block_absmax(ts, nonfinite_flag=True)),
                                  block_ref.block_words(orc, bad, True))
    # the flagged words through the two-stage kernels: the same NaN block
    w = inccl.block_absmax(ts, nonfinite_flag=True)
    q = inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_Q32, ts, w)
    _same(_np(inccl.stream_op_block(inccl.KIND_Q32, inccl.KIND_F32, [q], w, scale_R=R)), nan)


def test_fixed_exponent_calls_refuse_the_sentinel(gpu):
    import torch
    from container_inc_amd import inccl
    from container_inc_amd._lib import IncclError
    x = torch.ones(512, dtype=torch.float32, device=gpu)
    out = torch.full((512,), 7.0, dtype=torch.float32, device=gpu)
    with pytest.raises(IncclError, match="INCCL_SCALE_BLOCK"):
        inccl.reduce_f32([x, x], inccl.SCALE_BLOCK, out=out)
    with pytest.raises(IncclError, match="INCCL_SCALE_BLOCK"):
        inccl.prepare_reduce_f32([x, x], inccl.SCALE_BLOCK, out=out)
    assert (_np(out) == 7.0).all()
