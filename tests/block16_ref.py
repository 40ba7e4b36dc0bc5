"""TEST INFRASTRUCTURE ONLY -- the CPU reference of packed 16-bit lanes
(INCCL_KIND_P16 / INCCL_WIRE_P16): tests/block_ref.py's blocks and words, the
oracle's quantise / sum_q32 / dequantise and a numpy clip, composed into the
16-bit wire form of a per-block scaled fp32 bucket.

  k_b     max(choose_scale(w_b, R_total) - 16, -64)     (a zero block: 48)
  L       32767 // R_total
  q       clip(sat_i32(rne(x * 2^k_b)), -L, L), NaN -> 0
  word j  q[2j + 1] * 65536 + q[2j] mod 2^32; n odd: the last high lane is 0
  sum     s = sum of words mod 2^32 (orc.sum_q32)
  unpack  lo = sign_extend16(s), hi = (s - lo) >> 16
  y       (float)lane * 2^-(k_b + out_shift); a flagged block (bit 31 of w_b) is NaN

``bufs`` of reduce_f32_block16 is every rank's every bucket (R_total arrays)."""
from __future__ import annotations

import numpy as np

import block_ref

LANE_MAX = 32767
SCALE_MIN = -64


def lane_clamp(R_total: int) -> int:
    return LANE_MAX // R_total


def block_scales16(orc, words, R_total: int):
    return [max(k - 16, SCALE_MIN) for k in block_ref.block_scales(orc, words, R_total)]


def quant_lanes(orc, x, ks16, R_total: int, elem_base: int = 0) -> np.ndarray:
    """one bucket's clamped contributions, element i at the exponent of the
    bucket's block (elem_base + i) // 256"""
    L = lane_clamp(R_total)
    out = np.empty(x.size, np.int32)
    for sl, b in block_ref._segments(x.size, elem_base):
        out[sl] = np.clip(orc.quantise(np.ascontiguousarray(x[sl], dtype=np.float32), ks16[b]), -L, L)
    return out


def pack(q: np.ndarray) -> np.ndarray:
    """int32 words of int32 lanes: word j = q[2j + 1] * 65536 + q[2j] mod 2^32"""
    q = np.asarray(q, np.int64)
    if q.size % 2:
        q = np.concatenate([q, np.zeros(1, np.int64)])
    return ((q[1::2] * 65536 + q[0::2]) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def unpack(s: np.ndarray) -> np.ndarray:
    """the 2 * len(s) lanes of summed words"""
    s = np.asarray(s, np.int32).astype(np.int64)
    lo = ((s & 0xFFFF) ^ 0x8000) - 0x8000
    d = (((s - lo) & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000    # the 32-bit wrapped difference
    hi = d >> 16
    return np.stack([lo, hi], axis=1).reshape(-1).astype(np.int32)


def pack_quant_sum(orc, bufs, ks16, R_total: int, elem_base: int = 0) -> np.ndarray:
    """the int32 words of the wrap-around sum of every bucket's packed words;
    elem_base must be even (a word holds elements 2j, 2j + 1 of the bucket)"""
    assert elem_base % 2 == 0, "a word starts at an even element of the bucket"
    return orc.sum_q32([pack(quant_lanes(orc, x, ks16, R_total, elem_base)) for x in bufs])


def unpack_dequant(orc, word_arrays, ks16, n: int, elem_base: int = 0, out_shift: int = 0, nan_blocks=None):
    """n fp32 results from the sum of `word_arrays`, whose word 0 holds element
    elem_base of the bucket (in its high lane when elem_base is odd)"""
    lanes = unpack(orc.sum_q32([np.ascontiguousarray(w, dtype=np.int32) for w in word_arrays]))
    odd = elem_base & 1
    lanes = np.ascontiguousarray(lanes[odd:odd + n])
    out = np.empty(n, np.float32)
    for sl, b in block_ref._segments(n, elem_base):
        if nan_blocks is not None and nan_blocks[b]:
            out[sl] = np.nan
        else:
            out[sl] = orc.dequantise(np.ascontiguousarray(lanes[sl]), ks16[b]) * np.float32(2.0 ** -out_shift)
    return out


def reduce_f32_block16(orc, bufs, R_total: int, out_shift: int = 0, nonfinite_nan: bool = False):
    """(result, [k_b]) of the packed exchange of `bufs`"""
    words = block_ref.block_words(orc, bufs, nonfinite_nan)
    ks16 = block_scales16(orc, words, R_total)
    s = pack_quant_sum(orc, bufs, ks16, R_total)
    return unpack_dequant(orc, [s], ks16, bufs[0].size, out_shift=out_shift, nan_blocks=words >> 31), ks16
