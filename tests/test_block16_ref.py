"""Packed 16-bit lanes, the CPU reference itself (tests/block16_ref.py): the
packing identity on every word, the clamp binding on no finite lane, the error
bound R_total * 2^-(k_b + 1) + |sum| * 2^-23 on every lane, a shard cut at any
element offset, and both non-finite modes per block.

The last test is the source of DESIGN.md's accuracy table: it prints, and writes
to profiles/pack16/accuracy_cpu.json, the error of the packed mode, of 32-bit
block mode and of "bf16 compress" (every bucket rounded to bf16, summed in fp32)
relative to each block's absmax.  It asserts the spec bound only, never a
ranking: past about 16 contributors the packed mode is the less accurate one."""
import functools
import json
import os

import numpy as np
import pytest

import block16_ref
import block_ref
from conftest import ROOT

NS = [37, 2341, 10533]
RTS = [1, 2, 3, 8, 16]


@functools.lru_cache(maxsize=None)
def _case(n, R):
    from oracle import oracle as orc
    orc.build()
    bufs = block_ref.mixed_buckets(np.random.default_rng(0), n, R, zero_block=4 if block_ref.nblocks(n) > 4 else None)
    words = block_ref.block_words(orc, bufs)
    return bufs, words, block16_ref.block_scales16(orc, words, R)


@pytest.mark.parametrize("R", RTS)
@pytest.mark.parametrize("n", NS)
def test_packing_identity_clamp_and_bound(orc, n, R):
    bufs, words, ks = _case(n, R)
    L = block16_ref.lane_clamp(R)
    assert all(-64 <= k <= 48 for k in ks)
    if block_ref.nblocks(n) > 4:
        assert words[4] == 0 and ks[4] == 48
    # the clamp binds on no finite lane: |q| <= ceil(2^14 / R) <= L before it
    free = [np.concatenate([orc.quantise(np.ascontiguousarray(x[sl]), ks[b]) for sl, b in block_ref._segments(n, 0)])
            for x in bufs]
    lanes = [block16_ref.quant_lanes(orc, x, ks, R) for x in bufs]
    for f, q in zip(free, lanes):
        np.testing.assert_array_equal(f, q)
        assert np.abs(q).max() <= -(-(1 << 14) // R) <= L
    # unpack(sum of packed words) == the lane-wise integer sums, on every word
    want = np.sum(np.stack(lanes).astype(np.int64), axis=0)
    assert np.abs(want).max() <= block16_ref.LANE_MAX
    s = block16_ref.pack_quant_sum(orc, bufs, ks, R)
    assert s.dtype == np.int32 and s.size == (n + 1) // 2
    got = block16_ref.unpack(s)
    np.testing.assert_array_equal(got[:n], want)
    if n % 2:
        assert got[n] == 0                      # the zero high lane of the last word
    # the bound, against the float64 sum
    y, ks2 = block16_ref.reduce_f32_block16(orc, bufs, R)
    assert ks2 == ks
    exact, bound = block_ref.error_bound(bufs, ks, R)
    ratio = np.abs(y.astype(np.float64) - exact) / bound
    print(f"n {n} R_total {R}: worst lane at {ratio.max():.3f} of the bound")
    assert (ratio <= 1.0).all()
    # the mean folds into the dequantise stage, exactly
    avg, _ = block16_ref.reduce_f32_block16(orc, bufs, R, out_shift=2)
    np.testing.assert_array_equal(avg, y * np.float32(0.25))


@pytest.mark.parametrize("elem_base", [0, 256, 128, 64, 2, 3])
def test_shard_at_an_offset_equals_that_slice(orc, elem_base):
    """every rank's cut packed from the even element at or before elem_base, the
    words summed, and n elements from elem_base on dequantised (an odd elem_base
    skips the first word's low lane): that slice of the whole result"""
    R, n = 3, 1500
    bufs, _, ks = _case(2341, R)
    whole, _ = block16_ref.reduce_f32_block16(orc, bufs, R, out_shift=1)
    pb = elem_base & ~1
    parts = [block16_ref.pack_quant_sum(orc, [x[pb:elem_base + n]], ks, R, pb) for x in bufs]
    np.testing.assert_array_equal(block16_ref.pack_quant_sum(orc, [x[pb:elem_base + n] for x in bufs], ks, R, pb),
                                  orc.sum_q32(parts))
    got = block16_ref.unpack_dequant(orc, parts, ks, n, elem_base, out_shift=1)
    np.testing.assert_array_equal(got.view(np.uint32), whole[elem_base:elem_base + n].view(np.uint32))


@pytest.mark.parametrize("R", [2, 3, 8])
def test_nonfinite_is_per_block(orc, R):
    """+Inf at element 256 * 2 + 5 of one or two buckets: under the saturating
    mode only block 2 differs and the lanes of the Inf are +L per Inf contributor
    (every finite element of the block quantises to 0 at k = -64), scaled; under
    the NaN mode only block 2 is NaN"""
    n = 2341
    bufs, _, _ = _case(n, R)
    clean, _ = block16_ref.reduce_f32_block16(orc, bufs, R)
    blk = np.arange(n) // 256 == 2
    L = block16_ref.lane_clamp(R)
    for count in (1, 2):
        bad = [x.copy() for x in bufs]
        for r in range(count):
            bad[r][256 * 2 + 5] = np.float32(np.inf)
        if count == 2:
            bad[-1][256 * 2 + 6] = np.float32(-np.inf)
        sat, ks = block16_ref.reduce_f32_block16(orc, bad, R)
        nan, _ = block16_ref.reduce_f32_block16(orc, bad, R, nonfinite_nan=True)
        assert ks[2] == -64 and np.isfinite(sat).all()
        np.testing.assert_array_equal(sat[~blk], clean[~blk])
        np.testing.assert_array_equal(nan[~blk], clean[~blk])
        assert np.isnan(nan[blk]).all()
        want = np.zeros(int(blk.sum()), np.float32)
        want[5] = np.float32(L * count) * np.float32(2.0 ** 64)
        if count == 2:
            want[6] = np.float32(-L) * np.float32(2.0 ** 64)
        np.testing.assert_array_equal(sat[blk], want)      # the neighbouring lanes are untouched: no spill


def _blockmax_errors(y, exact, amax_elem):
    nz = amax_elem > 0
    rel = np.abs(y.astype(np.float64)[nz] - exact[nz]) / amax_elem[nz]
    return float(rel.max()), float(np.sqrt(np.mean(rel * rel)))


def test_accuracy_table(orc):
    """the table of DESIGN.md (Numerics, "Packed 16-bit lanes"): max and rms error
    relative to the block's absmax, per R_total, for the packed lanes, the 32-bit
    block mode and bf16 compress"""
    rows = []
    for n in (2341, 10533):
        for R in (1, 2, 3, 8, 16, 64):
            bufs, words, ks = _case(n, R)
            exact, bound = block_ref.error_bound(bufs, ks, R)
            amax = np.repeat((words & np.uint32(0x7FFFFFFF)).view(np.float32).astype(np.float64), 256)[:n]
            p16, _ = block16_ref.reduce_f32_block16(orc, bufs, R)
            assert (np.abs(p16.astype(np.float64) - exact) <= bound).all()
            q32, _ = block_ref.reduce_f32_block(orc, bufs, R)
            bf = np.zeros(n, np.float32)
            for x in bufs:
                bf += orc.bf16_to_f32(orc.f32_to_bf16(x))
            row = {"n": n, "R_total": R}
            for name, y in (("p16", p16), ("q32_block", q32), ("bf16_compress", bf)):
                row[name + "_max"], row[name + "_rms"] = _blockmax_errors(y, exact, amax)
            rows.append(row)
            print("n {n:5d} R_total {R_total:2d}: p16 max {p16_max:.2e} rms {p16_rms:.2e} | q32 block max "
                  "{q32_block_max:.2e} rms {q32_block_rms:.2e} | bf16 compress max {bf16_compress_max:.2e} rms "
                  "{bf16_compress_rms:.2e}".format(**row))
    out = os.path.join(ROOT, "profiles", "pack16", "accuracy_cpu.json")
    doc = {"what": "error / block absmax of the sum of R_total buckets, block_ref.mixed_buckets(default_rng(0), n, "
                   "R_total, zero_block=4); bf16_compress: every bucket rounded to bf16, summed in fp32",
           "rows": rows}
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    except OSError as e:   # a read-only checkout: the printed table stands
        print(f"not written ({e})")
