"""TEST INFRASTRUCTURE ONLY -- the CPU reference of error feedback for packed
16-bit lanes (inccl_*_ef): tests/block_ref.py's words and tests/block16_ref.py's
lanes applied to bucket + residual, and the residual each bucket is left with.

  v_r    fl32(x_r + e_r)                          one IEEE fp32 add
  w_b    block_ref.block_words over every v_r of every rank
  k_b, L, q_r, words, sum, unpack, y              block16_ref's, on v_r
  d_r    fl32(v_r - (float)q_r * 2^-k_b)          the product is exact; no out_shift
  e_r'   d_r where it is finite, else 0; 0 in every block whose word has bit 31

``bufs`` and ``residuals`` of step are every rank's every bucket (R_total arrays
each); a chain feeds the residuals it got back into the next step."""
from __future__ import annotations

import numpy as np

import block16_ref
import block_ref


def add(bufs, residuals):
    """v_r = fl32(x_r + e_r)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return [(np.asarray(x, np.float32) + np.asarray(e, np.float32)).astype(np.float32)
                for x, e in zip(bufs, residuals)]


def residual(orc, v, words, ks16, R_total: int, elem_base: int = 0):
    """(e', d, q) of one bucket's v at the agreed words: d as float32, before
    the non-finite and flagged-block rules; element i is element elem_base + i
    of the bucket"""
    q = block16_ref.quant_lanes(orc, v, ks16, R_total, elem_base)
    d = np.empty(v.size, np.float32)
    e = np.empty(v.size, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for sl, b in block_ref._segments(v.size, elem_base):
            carried = q[sl].astype(np.float32) * np.float32(2.0 ** -ks16[b])      # exact: |q| <= 2^15
            d[sl] = (v[sl] - carried).astype(np.float32)
            keep = np.isfinite(d[sl]) & (not (int(words[b]) >> 31))
            e[sl] = np.where(keep, d[sl], np.float32(0.0))
    return e, d, q


def step(orc, bufs, residuals, R_total: int, out_shift: int = 0, nonfinite_nan: bool = False):
    """(y, [e_r'], [k_b]) of one call"""
    vs = add(bufs, residuals)
    words = block_ref.block_words(orc, vs, nonfinite_nan)
    ks16 = block16_ref.block_scales16(orc, words, R_total)
    s = block16_ref.pack_quant_sum(orc, vs, ks16, R_total)
    y = block16_ref.unpack_dequant(orc, [s], ks16, vs[0].size, out_shift=out_shift, nan_blocks=words >> 31)
    return y, [residual(orc, v, words, ks16, R_total)[0] for v in vs], ks16


def zeros_like(bufs):
    return [np.zeros(x.size, np.float32) for x in bufs]


def chain(orc, steps, R_total: int, out_shift: int = 0, nonfinite_nan: bool = False, feedback: bool = True):
    """[(y_t, [e_{r,t}], [k_b])] of `steps` (a list of bufs) from zero residuals;
    feedback=False: every step starts from zero residuals again (the plain wire)"""
    res = zeros_like(steps[0])
    out = []
    for bufs in steps:
        y, new, ks = step(orc, bufs, res, R_total, out_shift, nonfinite_nan)
        out.append((y, new, ks))
        res = new if feedback else zeros_like(bufs)
    return out


def telescoping_bound(steps, last_residuals, R_total: int):
    """(exact64, bound) of sum_t y_t with out_shift = 0 against sum_t sum_r x_{r,t}:
    sum_r |e_{r,T}| + T * R_total * 2^-23 * max_t amax_b(x), the half-ulp of each
    x + e add with |v| <= 2 amax_b(x); derived, not measured -- it holds where no
    clamp binds and nothing is non-finite"""
    n = steps[0][0].size
    exact = np.zeros(n, np.float64)
    amax = np.zeros(block_ref.nblocks(n), np.float64)
    for bufs in steps:
        for x in bufs:
            exact += x.astype(np.float64)
            a = np.abs(x.astype(np.float64))
            pad = np.concatenate([a, np.zeros(block_ref.nblocks(n) * block_ref.B - n)])
            amax = np.maximum(amax, pad.reshape(-1, block_ref.B).max(axis=1))
    carried = np.sum(np.stack([np.abs(e.astype(np.float64)) for e in last_residuals]), axis=0)
    return exact, carried + len(steps) * R_total * 2.0 ** -23 * np.repeat(amax, block_ref.B)[:n]
