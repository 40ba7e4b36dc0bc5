"""Error feedback for packed 16-bit lanes, the stateless kernels (gpu):
inccl_block_absmax_f32_ef, inccl_pack_f32_block16_ef and
inccl_reduce_f32_block16_ef against the CPU reference tests/block16_ef_ref.py,
bit for bit on results, words and residuals.  A NaN compares equal to a NaN
whatever its payload; every other lane by its bits.

Sizes as tests/test_gpu_block16_kernels.py: 37 (one partial block, an odd n),
2341 (nine blocks and a partial one, less than one tile) and 10533 (full tiles,
a ragged one, the tail).  Every case runs two chained steps on the same
buckets, so that the second reads the non-zero residuals of the first."""
import functools

import numpy as np
import pytest

import block16_ef_ref as ef
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


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=None)
def _case(R, n):
    """the buckets and the reference's two chained steps, computed once per (R, n):
    (bufs, [(y, residuals, ks, words of v)] per step)"""
    orc = _orc()
    bufs = block_ref.mixed_buckets(np.random.default_rng(0), n, R, zero_block=4 if block_ref.nblocks(n) > 4 else None)
    res, steps = ef.zeros_like(bufs), []
    for _ in range(2):
        words = block_ref.block_words(orc, ef.add(bufs, res))
        y, res, ks = ef.step(orc, bufs, res, R)
        steps.append((y, res, ks, words))
    return bufs, steps


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("R", RS)
def test_absmax_and_fused(gpu, R, n):
    """block_absmax_ef's words and reduce_f32_block16_ef's result, words and
    residuals over two chained steps; then with every pointer 4 bytes into its
    allocation, which takes the per-element kernels"""
    import torch
    from container_inc_amd import inccl
    bufs, steps = _case(R, n)
    for put in (_t, _off1):
        ts = [put(x, gpu) for x in bufs]
        rs = [put(np.zeros(n, np.float32), gpu) for _ in bufs]
        for y, res, _, words in steps:
            np.testing.assert_array_equal(_np(inccl.block_absmax_ef(ts, rs)).view(np.uint32), words)
            w = torch.full((block_ref.nblocks(n),), -1, dtype=torch.int32, device=gpu)
            out = put(np.full(n, 7.0, np.float32), gpu)
            _same(_np(inccl.reduce_f32_block16_ef(ts, rs, out=out, words=w)), y)
            np.testing.assert_array_equal(_np(w).view(np.uint32), words)
            for r, e in zip(rs, res):
                _same(_np(r), e)
        for x, t in zip(bufs, ts):
            _same(_np(t), x)                       # the sources are only read


@pytest.mark.parametrize("R", [1, 3])
def test_fused_in_place(gpu, R):
    """dst may alias srcs[0]"""
    from container_inc_amd import inccl
    n = 10533
    bufs, steps = _case(R, n)
    rs = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    for y, res, _, _ in steps:
        ts = [_t(x, gpu) for x in bufs]
        _same(_np(inccl.reduce_f32_block16_ef(ts, rs, out=ts[0])), y)
        for r, e in zip(rs, res):
            _same(_np(r), e)


@pytest.mark.parametrize("copy", [False, True], ids=["view", "copy"])
@pytest.mark.parametrize("elem_base", [0, 256, 128, 64, 4, 2])
def test_pack_at_an_offset(gpu, elem_base, copy):
    """The sharded route's quantise stage on a 1500-element cut of the
    2341-element bucket, at the whole bucket's words of its second step (the
    residuals it reads are the first step's): the words and the residuals of the
    cut are the reference's at that elem_base, and they are that slice of the
    whole bucket's.  view: the cut is a slice of the bucket's and the residual's
    tensors, whose other elements stay; copy: tensors of their own."""
    from container_inc_amd import inccl
    orc = _orc()
    R, n, N = 3, 1500, 2341
    bufs, steps = _case(R, N)
    (_, res1, _, _), (_, res2, ks, words) = steps
    wt = _t(words.view(np.int32), gpu)
    sl = slice(elem_base, elem_base + n)
    vs = ef.add([x[sl] for x in bufs], [e[sl] for e in res1])
    want_words = block16_ref.pack_quant_sum(orc, vs, ks, R, elem_base)
    whole = block16_ref.pack_quant_sum(orc, ef.add(bufs, res1), ks, R)
    np.testing.assert_array_equal(want_words, whole[elem_base // 2:(elem_base + n) // 2])
    if copy:
        cts, rts, full = [_t(x[sl], gpu) for x in bufs], [_t(e[sl], gpu) for e in res1], None
    else:
        full = [_t(e, gpu) for e in res1]
        cts, rts = [_t(x, gpu)[sl] for x in bufs], [f[sl] for f in full]
    got = inccl.pack_block16_ef(cts, rts, wt, elem_base=elem_base, scale_R=R)
    np.testing.assert_array_equal(_np(got), want_words)
    for v, r, e2 in zip(vs, rts, res2):
        _same(_np(r), ef.residual(orc, v, words, ks, R, elem_base)[0])
        _same(_np(r), e2[sl])
    if full is not None:
        for f, e1, e2 in zip(full, res1, res2):
            want = e1.copy()
            want[sl] = e2[sl]
            _same(_np(f), want)


@pytest.mark.parametrize("elem_base", [0, 4, 2])
def test_pack_with_zero_residuals_is_the_plain_pack(gpu, elem_base):
    """No residuals and zero residuals are one kernel body: at R = 3 and
    n = 2341 (elem_base 0 and 4: four tiles of the vector kernel and a tail;
    2: per word throughout), pack_block16_ef with zero residuals returns exactly
    the words of stream_op_block's F32 -> P16 on the same buckets and words, and
    leaves the reference's residuals.  The call's elements are elements
    elem_base .. of a bucket that is zero before them."""
    from container_inc_amd import inccl
    orc = _orc()
    R, n = 3, 2341
    bufs, _ = _case(R, n)
    words = block_ref.block_words(orc, [np.concatenate([np.zeros(elem_base, np.float32), x]) for x in bufs])
    ks = block16_ref.block_scales16(orc, words, R)
    wt = _t(words.view(np.int32), gpu)
    ts = [_t(x, gpu) for x in bufs]
    rs = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    plain = _np(inccl.stream_op_block(inccl.KIND_F32, inccl.KIND_P16, ts, wt, elem_base=elem_base, scale_R=R))
    got = _np(inccl.pack_block16_ef(ts, rs, wt, elem_base=elem_base, scale_R=R))
    np.testing.assert_array_equal(got, plain)
    np.testing.assert_array_equal(got, block16_ref.pack_quant_sum(orc, bufs, ks, R, elem_base))
    for v, r in zip(ef.add(bufs, ef.zeros_like(bufs)), rs):
        _same(_np(r), ef.residual(orc, v, words, ks, R, elem_base)[0])
    assert any(_np(r).any() for r in rs)


def test_pack_refuses_an_odd_elem_base(gpu):
    import torch
    from container_inc_amd import inccl
    from container_inc_amd._lib import IncclError
    x = torch.ones(512, dtype=torch.float32, device=gpu)
    e = torch.full((512,), 0.25, dtype=torch.float32, device=gpu)
    w = torch.zeros(3, dtype=torch.int32, device=gpu)
    out = torch.full((256,), 7, dtype=torch.int32, device=gpu)
    with pytest.raises(IncclError, match=r"rc=-1.*odd elem_base"):
        inccl.pack_block16_ef([x], [e], w, out=out, elem_base=3)
    assert (_np(out) == 7).all() and (_np(e) == 0.25).all()


def _staged(inccl, ts, rs, R, n, flag=False):
    """absmax_ef -> pack_ef per bucket -> sum_q32 -> P16 -> F32: what R ranks of one bucket each run"""
    w = inccl.block_absmax_ef(ts, rs, nonfinite_flag=flag)
    parts = [inccl.pack_block16_ef([t], [r], w, scale_R=R) for t, r in zip(ts, rs)]
    return inccl.stream_op_block(inccl.KIND_P16, inccl.KIND_F32, [inccl.sum_q32(parts)], w, n=n, scale_R=R), w


def test_edge_values(gpu):
    """A subnormal beside a large element (the residual is the subnormal
    itself), a zero block, half-even ties, and +-FLT_MAX in a block of small
    elements (k_b clamps at -64, the lane's clamp binds, the residual is large
    and finite): fused and staged, two chained steps"""
    from container_inc_amd import inccl
    orc = _orc()
    R, n = 2, 1024
    fmax = np.finfo(np.float32).max
    rng = np.random.default_rng(1)
    bufs = [np.zeros(n, np.float32) for _ in range(R)]
    sub = np.float32(1e-42)
    for r, x in enumerate(bufs):
        x[0:256] = rng.standard_normal(256).astype(np.float32) * np.float32(0.1)
        x[3], x[7 + r] = np.float32(1.0), sub                       # block 0: absmax 1, a subnormal beside it
        x[512:768] = 0                                               # block 1 stays zero; block 2: ties
        x[512] = np.float32(1.0)
        x[513], x[514], x[515], x[516] = (np.float32(c * 2.0 ** -14) for c in (1, 3, -1, -5))
        x[768:1024] = rng.standard_normal(256).astype(np.float32) * np.float32(1e-3)
    bufs[0][770], bufs[1][771] = fmax, -fmax                         # block 3
    res, steps = ef.zeros_like(bufs), []
    for _ in range(2):
        y, res, ks = ef.step(orc, bufs, res, R)
        steps.append((y, res, ks))
    y, res1, ks = steps[0]
    L = block16_ref.lane_clamp(R)
    assert ks == [13, 48, 13, -64]
    assert res1[0][7] == sub and res1[1][8] == sub
    assert not res1[0][256:512].any() and not y[256:512].any()
    assert [float(v) for v in res1[0][513:517]] == [2.0 ** -14, -2.0 ** -14, -2.0 ** -14, -2.0 ** -14]
    assert y[770] == np.float32(L) * np.float32(2.0 ** 64)
    assert res1[0][770] == np.float32(fmax - np.float32(L) * np.float32(2.0 ** 64)) and np.isfinite(res1[0][770])
    assert res1[0][780] == bufs[0][780] != 0                        # a small element of block 3: carried whole
    ts = [_t(x, gpu) for x in bufs]
    fr = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    sr = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    for y, res, _ in steps:
        _same(_np(inccl.reduce_f32_block16_ef(ts, fr)), y)
        _same(_np(_staged(inccl, ts, sr, R, n)[0]), y)
        for a, b, e in zip(fr, sr, res):
            _same(_np(a), e)
            _same(_np(b), e)


def test_nonfinite_is_per_block(gpu):
    """A NaN and +-Inf in block 2.  Saturate mode: those elements leave no
    residual, the block's other elements quantise to 0 and are carried whole.
    INCCL_ABSMAX_FLAG_NONFINITE: the block's results are NaN and its residuals
    0.  Every other block equals the clean run in both modes, fused and staged."""
    from container_inc_amd import inccl
    orc = _orc()
    R, n = 3, 2341
    bufs, steps = _case(R, n)
    clean_y, clean_res, _, _ = steps[0]
    bad = [x.copy() for x in bufs]
    bad[0][256 * 2 + 5] = bad[1][256 * 2 + 5] = np.float32(np.inf)
    bad[2][256 * 2 + 6] = np.float32(-np.inf)
    bad[2][256 * 2 + 8] = np.float32(np.nan)
    blk = np.arange(n) // 256 == 2
    zero = ef.zeros_like(bad)
    sat_y, sat_res, ks = ef.step(orc, bad, zero, R)
    nan_y, nan_res, _ = ef.step(orc, bad, zero, R, nonfinite_nan=True)
    assert ks[2] == -64 and np.isfinite(sat_y).all() and np.isnan(nan_y[blk]).all()
    assert sat_res[0][256 * 2 + 5] == 0 and sat_res[2][256 * 2 + 6] == 0 and sat_res[2][256 * 2 + 8] == 0
    assert sat_res[0][256 * 2 + 9] == bad[0][256 * 2 + 9] != 0
    assert not any(e[blk].any() for e in nan_res)
    ts = [_t(x, gpu) for x in bad]
    for flag, y, res in ((False, sat_y, sat_res), (True, nan_y, nan_res)):
        fr = [_t(z, gpu) for z in zero]
        sr = [_t(z, gpu) for z in zero]
        got = _np(inccl.reduce_f32_block16_ef(ts, fr, nonfinite_flag=flag))
        _same(got, y)
        _same(got[~blk], clean_y[~blk])
        _same(_np(_staged(inccl, ts, sr, R, n, flag)[0]), y)
        for a, b, e, c in zip(fr, sr, res, clean_res):
            _same(_np(a), e)
            _same(_np(b), e)
            _same(_np(a)[~blk], c[~blk])
        # a second step from these residuals: the carried elements come back in
        y2, res2, _ = ef.step(orc, bad, res, R, nonfinite_nan=flag)
        _same(_np(inccl.reduce_f32_block16_ef(ts, fr, nonfinite_flag=flag)), y2)
        for a, e in zip(fr, res2):
            _same(_np(a), e)


def test_fused_equals_the_stages(gpu):
    """R = 3: the one-pass kernel's result and residuals are those of
    absmax_ef -> pack_ef per bucket -> sum_q32 -> P16 -> F32 over two chained
    steps, and with zero residuals the result is the existing P16 path's"""
    from container_inc_amd import inccl
    R, n = 3, 10533
    bufs, steps = _case(R, n)
    ts = [_t(x, gpu) for x in bufs]
    fr = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    sr = [_t(np.zeros(n, np.float32), gpu) for _ in bufs]
    plain = _np(inccl.reduce_f32_block16(ts))
    for i, (y, res, _, words) in enumerate(steps):
        fused = _np(inccl.reduce_f32_block16_ef(ts, fr))
        staged, w = _staged(inccl, ts, sr, R, n)
        _same(fused, _np(staged))
        _same(fused, y)
        np.testing.assert_array_equal(_np(w).view(np.uint32), words)
        if i == 0:
            _same(fused, plain)
        else:
            assert not np.array_equal(fused.view(np.uint32), plain.view(np.uint32))
        for a, b, e in zip(fr, sr, res):
            _same(_np(a), _np(b))
            _same(_np(a), e)
