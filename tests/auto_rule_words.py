"""The absmax words that pin the auto scale rule as the single-scale kernels
resolve it from a device word (tests/test_gpu_kernels.py
test_auto_rule_from_device_word; walked through the oracle alone in
tests/test_choose_scale_word.py): the exponent fields at both ends, around the
clamps and in the middle, with the significands where the rule can turn; 2^j / R
(the m == 0.5 branch where R allows it) with its bit-neighbours; 0, +Inf and a
NaN; and every sixth word once more with bit 31, the non-finite flag."""
import numpy as np

RS = (1, 2, 3, 7, 8, 64)
EXPONENTS = (0, 1, 2, 63, 64, 126, 127, 128, 190, 191, 253, 254)
SIGNIFICANDS = (0, 1, 0x400000, 0x7FFFFF, 0x555555, 0x2AAAAB)
POWERS = (-100, -1, 0, 1, 30, 100)
FLAG = 0x80000000


def words(R):
    """the (word, R) pairs' words for R contributors, flagged copies last"""
    ws = [e << 23 | s for e in EXPONENTS for s in SIGNIFICANDS]
    for j in POWERS:
        w = int(np.array([2.0 ** j / R], np.float32).view(np.uint32)[0])
        ws += [w - 1, w, w + 1]
    ws += [0, 0x7F800000, 0x7FC00000]
    return ws + [w | FLAG for w in ws[::6]]


def as_float(word):
    return np.array([word], np.uint32).view(np.float32)[0]
