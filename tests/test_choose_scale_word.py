"""inccl_choose_scale_word (CPU, no compute): the library's host rule from an
absmax word to a scale exponent (the IPC engines' host-agreed auto scale goes
through it), against the oracle -- on single words, and on the words of every
256-element block of a mixed bucket against tests/block_ref.py.  Bit 31 of a
word marks a non-finite input: reported, and kept out of the exponent."""
import ctypes

import numpy as np
import pytest

import block_ref


def _word(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_word_rule_matches_the_float_rule_and_the_oracle(lib, orc):
    from container_inc_amd import inccl
    sub = float(np.float32(1e-40))
    for amax in (0.0, sub, 1e-30, 1e-3, 0.25, 0.5, 1.0, 6.0, 7.999, 1e6, 3e38, float("inf")):
        for R in (1, 2, 3, 8, 64):
            want = orc.choose_scale(amax, R)
            assert inccl.choose_scale_word(_word(amax), R) == (want, False), (amax, R)
            # the flag bit is reported and leaves the exponent alone
            assert inccl.choose_scale_word(_word(amax) | 0x80000000, R) == (want, True), (amax, R)
    assert inccl.choose_scale_word(0, 4) == (inccl.SCALE_MAX, False)
    assert inccl.choose_scale_word(_word(np.inf) | 0x80000000, 4) == (inccl.SCALE_MIN, True)
    assert lib.inccl_choose_scale_word(_word(6.0), 8, None) == 24   # NULL flag pointer
    with pytest.raises(ValueError):
        inccl.choose_scale_word(-1, 2)


def test_auto_rule_word_list_covers_the_rule(orc):
    """The words of the GPU test of the kernels' rule (test_gpu_kernels.py
    test_auto_rule_from_device_word), through the oracle alone: both clamps,
    exponents between them, and both branches of the rule (m == 0.5 or not)."""
    import math

    import auto_rule_words as arw
    from container_inc_amd import inccl
    pairs = [(w, R) for R in arw.RS for w in arw.words(R)]
    assert len(pairs) <= 660 and len(set(pairs)) > 600
    assert sum(1 for w, _ in pairs if w & arw.FLAG) >= len(pairs) // 8
    ks, half, other = set(), 0, 0
    for w, R in pairs:
        if w & arw.FLAG:
            continue
        amax = float(arw.as_float(w))
        k = orc.choose_scale(amax, R)
        ks.add(k)
        if inccl.SCALE_MIN < k < inccl.SCALE_MAX:
            m, e = math.frexp(amax * R)
            assert k == (31 - e if m == 0.5 else 30 - e), (hex(w), R)
            half += m == 0.5
            other += m != 0.5
    assert inccl.SCALE_MIN in ks and inccl.SCALE_MAX in ks
    assert len([k for k in ks if inccl.SCALE_MIN < k < inccl.SCALE_MAX]) > 20
    assert half >= 20 and other >= 20, (half, other)


def test_block_words_give_the_reference_exponents(lib, orc):
    """Per block of a mixed-magnitude bucket (and one poisoned block): the
    library's exponent of every block word is the reference's k_b."""
    from container_inc_amd import inccl
    R = 3
    bufs = block_ref.mixed_buckets(np.random.default_rng(0), 256 * 9 + 37, R, zero_block=4)
    bufs[1][256 * 2 + 5] = np.float32(-np.inf)
    bufs[2][256 * 7 + 1] = np.float32(np.nan)
    _, ks = block_ref.reduce_f32_block(orc, bufs, R)
    assert ks[2] == inccl.SCALE_MIN and ks[4] == inccl.SCALE_MAX and len(set(ks)) > 4
    for flag in (False, True):
        words = block_ref.block_words(orc, bufs, nonfinite_flag=flag)
        got = [inccl.choose_scale_word(int(w), R) for w in words]
        if flag:
            # (a NaN's payload bits stand in its flagged word: its block's exponent is not
            # the clean one and its result is NaN anyway; the Inf block keeps SCALE_MIN)
            assert [nf for _, nf in got] == [b in (2, 7) for b in range(len(ks))]
            assert [k for b, (k, _) in enumerate(got) if b != 7] == [k for b, k in enumerate(ks) if b != 7]
        else:
            assert got == [(k, False) for k in ks]
    nf = ctypes.c_int(7)
    assert lib.inccl_choose_scale_word(int(words[2]), R, ctypes.byref(nf)) == inccl.SCALE_MIN and nf.value == 1
