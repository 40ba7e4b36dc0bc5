"""Error feedback for packed 16-bit lanes on the CPU reference alone
(tests/block16_ef_ref.py; no GPU): the telescoping bound holds with feedback on
every lane and fails without it on most, the residual is exact where the clamp
does not bind, zero residuals give the plain packed result -- so the contrast
the GPU tests rely on is known before they run -- and the accuracy table of
DESIGN.md (Numerics, "Error feedback")."""
import functools
import json
import os

import numpy as np
import pytest

import block16_ef_ref as ef
import block16_ref
import block_ref
from conftest import ROOT

N = 2341


@functools.lru_cache(maxsize=None)
def _bufs(R, n=N):
    return block_ref.mixed_buckets(np.random.default_rng(0), n, R, zero_block=4)


@functools.lru_cache(maxsize=None)
def _chains(R, T):
    """the same buckets fed T times, with and without feedback"""
    from oracle import oracle as orc
    orc.build()
    steps = [_bufs(R)] * T
    return steps, ef.chain(orc, steps, R), ef.chain(orc, steps[:1], R, feedback=False) * T


def _sum64(chain):
    return np.sum(np.stack([y.astype(np.float64) for y, _, _ in chain]), axis=0)


@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_telescoping_bound(orc, R, T):
    """sum_t y_t is within sum_r |e_{r,T}| + T R 2^-23 amax_b of T exact sums on
    every lane with feedback; without it at least half of the lanes miss the
    same bound"""
    steps, fb, plain = _chains(R, T)
    exact, bound = ef.telescoping_bound(steps, fb[-1][1], R)
    err = np.abs(_sum64(fb) - exact)
    worst = float(np.max(err[bound > 0] / bound[bound > 0]))
    miss = float(np.mean(np.abs(_sum64(plain) - exact) > bound))
    print(f"R {R} T {T}: with feedback the worst lane is at {worst:.3f} of the bound; without, {miss:.3f} of the "
          f"lanes exceed it")
    assert (err <= bound).all()
    assert miss >= 0.5


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_residual_is_exact_and_small(orc, R):
    """d as float64 equals the float64 difference v - q 2^-k_b, and |e'| <=
    2^-(k_b + 1) where the clamp does not bind, on every step of a chain"""
    res = ef.zeros_like(_bufs(R))
    L = block16_ref.lane_clamp(R)
    for _ in range(4):
        vs = ef.add(_bufs(R), res)
        words = block_ref.block_words(orc, vs)
        ks = block16_ref.block_scales16(orc, words, R)
        k = np.repeat(np.asarray(ks, np.float64), 256)[:N]
        new = []
        for v in vs:
            e, d, q = ef.residual(orc, v, words, ks, R)
            np.testing.assert_array_equal(d.astype(np.float64), v.astype(np.float64) - q.astype(np.float64) * 2.0 ** -k)
            free = np.abs(q) < L
            assert free.all()                    # finite data: the clamp never binds
            assert (np.abs(e.astype(np.float64))[free] <= 2.0 ** -(k[free] + 1)).all()
            np.testing.assert_array_equal(e, d)
            new.append(e)
        res = new


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_zero_residuals_give_the_plain_packed_result(orc, R):
    bufs = _bufs(R)
    y, _, ks = ef.step(orc, bufs, ef.zeros_like(bufs), R, out_shift=1)
    want, ks16 = block16_ref.reduce_f32_block16(orc, bufs, R, out_shift=1)
    np.testing.assert_array_equal(y.view(np.uint32), want.view(np.uint32))
    assert ks == ks16


def test_nonfinite_rules(orc):
    """saturate mode: a NaN or +-Inf element leaves no residual, the finite ones
    of its block are carried whole; flagged mode: the block's residuals are zero"""
    R = 2
    bad = [x.copy() for x in _bufs(R)]
    bad[0][256 * 2 + 5] = np.float32(np.inf)
    bad[1][256 * 2 + 6] = np.float32(np.nan)
    blk = np.arange(N) // 256 == 2
    y, res, ks = ef.step(orc, bad, ef.zeros_like(bad), R)
    assert ks[2] == -64 and np.isfinite(y).all()
    assert res[0][256 * 2 + 5] == 0 and res[1][256 * 2 + 6] == 0
    keep = blk.copy()
    keep[256 * 2 + 5] = False
    np.testing.assert_array_equal(res[0][keep], bad[0][keep])
    y, res, _ = ef.step(orc, bad, ef.zeros_like(bad), R, nonfinite_nan=True)
    assert np.isnan(y[blk]).all() and np.isfinite(y[~blk]).all()
    for e in res:
        assert not e[blk].any() and e[~blk].any()


def _blockmax_error(mean, exact, bufs):
    """max |mean - exact| relative to the block's absmax of x, over the lanes of non-zero blocks"""
    a = np.max(np.stack([np.abs(x.astype(np.float64)) for x in bufs]), axis=0)
    n = a.size
    pad = np.concatenate([a, np.zeros(block_ref.nblocks(n) * 256 - n)]).reshape(-1, 256).max(axis=1)
    amax = np.repeat(pad, 256)[:n]
    nz = amax > 0
    return float(np.max(np.abs(mean[nz] - exact[nz]) / amax[nz]))


def test_accuracy_table(orc):
    """the table of DESIGN.md (Numerics, "Error feedback"): T = 64 steps of the
    same buckets, the worst error of the mean result relative to the block's
    absmax, with and without feedback.  Only the bound is asserted."""
    T, rows = 64, []
    for R in (2, 8, 16, 64):
        bufs = _bufs(R)
        steps = [bufs] * T
        fb = ef.chain(orc, steps, R)
        plain = ef.chain(orc, steps[:1], R, feedback=False) * T
        exact, bound = ef.telescoping_bound(steps, fb[-1][1], R)
        assert (np.abs(_sum64(fb) - exact) <= bound).all()
        row = {"n": N, "R_total": R, "T": T,
               "plain_max": _blockmax_error(_sum64(plain) / T, exact / T, bufs),
               "feedback_max": _blockmax_error(_sum64(fb) / T, exact / T, bufs)}
        rows.append(row)
        print("R_total {R_total:2d} T {T}: mean result's max error / block absmax {plain_max:.2e} without feedback, "
              "{feedback_max:.2e} with it".format(**row))
    out = os.path.join(ROOT, "profiles", "pack16_ef", "accuracy_cpu.json")
    doc = {"what": "max over lanes of |mean_t y_t - exact sum| / block absmax over T steps of the same R_total buckets, "
                   "block_ref.mixed_buckets(default_rng(0), n, R_total, zero_block=4), through block16_ef_ref.chain "
                   "with the residual fed back (feedback) and dropped (plain: the packed wire as it is)",
           "rows": rows}
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    except OSError as e:   # a read-only checkout: the printed table stands
        print(f"not written ({e})")
