"""The single-scale stream family, every instantiation and every pass of its
grid-stride loops (gpu): inccl_stream_op's 9 four-byte and 6 two-byte (IN, OUT)
pairs at R = 1..8 in their vector and element forms, the capped grid of
inccl_set_tuning, the NT = false loads, and k_stream_scalar / k_stream16_scalar
/ k_absmax / k_checksum past their grid caps -- bit for bit against the oracle.

Where the sizes come from (update them with the geometry, in the same commit):

  k_stream_vec      inccl_stream.h Geometry<R>: BLOCK x U quads a tile = 1024 x 1
                    (R = 1, 4..8), 512 x 2 (R = 2) -> 4096 elements; 512 x 1 (R = 3)
                    -> 2048.  8343 = 2 * 4096 + 4 * 37 + 3: full tiles, a ragged
                    tile shorter than one BLOCK, a 3-element tail (k_stream_scalar).
                    6295 = 4096 + 4 * 549 + 3: the ragged tile reaches into the
                    second unrolled quad of R = 2's 512 x 2.
  k_stream16        inccl_kernels.hip B16Geometry<R>: 512 x 1 (R <= 2), 256 x 2
                    (R >= 3) groups of 8 elements -> 4096 elements a tile.
                    8493 = 2 * 4096 + 8 * 37 + 5; 6445 = 4096 + 8 * 293 + 5: the
                    ragged tile reaches into the second group of 256 x 2.
  grid cap          inccl_kernels.hip stream_grid: one workgroup per tile unless
                    inccl_set_tuning caps the grid.  Cap 2: one workgroup takes
                    a full tile and then the ragged one; cap 1: one takes all.
  element kernels   launch_stream_R / launch_stream16_R: grid_of(n, kBlock = 256,
                    8) -> the second pass starts at 2048 * CUs elements.
  k_absmax          launch_absmax: grid_of(quads, kAmBlock * kAmU = 1024, 2) ->
                    2048 * CUs quads of EPQ = 4 (fp32) or 8 (bf16, fp16) elements.
  k_checksum        inccl_k_checksum: grid_of(n / 4, kBlock = 256, 8) ->
                    2048 * CUs quads.

CUs is torch's multi_processor_count, the count num_cus() of inccl_launch.h
caches.  Every output is a view of a larger allocation prefilled with a
sentinel, and the guard elements on both sides are checked after the call.
The tuning is process-global: every test sets it through _tuning(), which
restores (0, True) in a finally."""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1
F32, Q32, Q32BE, BF16, F16 = 0, 1, 2, 3, 4
NAMES = {F32: "F32", Q32: "Q32", Q32BE: "Q32BE", BF16: "BF16", F16: "F16"}
N4 = (2 * 4096 + 4 * 37 + 3, 4096 + 4 * 549 + 3)
N16 = (2 * 4096 + 8 * 37 + 5, 4096 + 8 * 293 + 5)
K32 = 20          # the fixed exponent of the fp32 inputs: |x| > 2048 saturates
K16_IN = 20       # ... of the bf16 / fp16 inputs: 65504 and the infinities saturate
K16_OUT = 15      # ... of Q32 -> BF16 / F16: INT32_MAX * 2^-15 = 65536 overflows a half, 1 * 2^-15 is a half subnormal
G = 64            # guard elements either side of a view: 256 B / 128 B, so the view keeps the allocation's alignment
SENT = {4: 0x5A5A5A5A, 2: 0x5A5A}


@contextlib.contextmanager
def _tuning(grid_cap, nt_loads=True):
    from container_inc_amd import inccl
    inccl.set_tuning(grid_cap, nt_loads)
    try:
        yield
    finally:
        inccl.set_tuning(0, True)


@pytest.fixture(autouse=True)
def _default_tuning_after_every_test():
    yield
    from container_inc_amd import inccl
    inccl.set_tuning(0, True)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _width(kind):
    return 2 if kind in (BF16, F16) else 4


def _view(t, kind):
    """the int32 / int16 tensor t as the torch dtype the wrapper expects of `kind`"""
    import torch
    return t.view({F32: torch.float32, Q32: torch.int32, Q32BE: torch.int32, BF16: torch.bfloat16,
                   F16: torch.float16}[kind])


class _Buf:
    """n elements of `kind` on the GPU, `shift` elements past a 16-B boundary,
    inside an allocation whose other elements hold a sentinel: `bits` (uint32 /
    uint16 patterns) or the sentinel throughout"""

    def __init__(self, dev, kind, n, bits=None, shift=0):
        import torch
        w = _width(kind)
        dt = np.uint32 if w == 4 else np.uint16
        host = np.full(G + shift + n + G, SENT[w], dt)
        if bits is not None:
            host[G + shift:G + shift + n] = np.asarray(bits).view(dt)
        self.w, self.n, self.lo = w, n, G + shift
        self.raw = torch.from_numpy(host.view(np.int32 if w == 4 else np.int16)).to(dev)
        self.t = _view(self.raw[self.lo:self.lo + n], kind)
        assert self.t.data_ptr() % 16 == (shift * w) % 16

    def bits(self):
        """the n elements' bit patterns, after checking both guards"""
        import torch
        torch.cuda.synchronize()
        host = self.raw.cpu().numpy().view(np.uint32 if self.w == 4 else np.uint16)
        assert (host[:self.lo] == SENT[self.w]).all(), "written before the output"
        assert (host[self.lo + self.n:] == SENT[self.w]).all(), "written past n"
        return host[self.lo:self.lo + self.n].copy()


def _orc():
    from oracle import oracle as orc
    orc.build()
    return orc


def _plant(x, values, r):
    """`values`, rotated by r, at the start, inside the second tile, inside the
    ragged tile and over the tail of x"""
    v = np.roll(np.asarray(values, x.dtype), r)
    for off in (0, 4096 + 5, x.size - 3 - 2 * v.size, x.size - v.size):
        x[off:off + v.size] = v


@functools.lru_cache(maxsize=None)
def _inputs4(n):
    """8 fp32 buckets (_grads' specials and values that saturate at K32), 8
    full-range int32 buckets: numpy arrays"""
    rng = np.random.default_rng(n)
    fs, qs = [], []
    for r in range(8):
        x = (rng.standard_normal(n) * 300.0).astype(np.float32)
        _plant(x, [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38, -3e38, 2048.0, -2048.0, 2047.9998, 5000.0, -1e9], r)
        q = rng.integers(INT32_MIN, INT32_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
        _plant(q, [INT32_MIN, INT32_MAX, 0, -1, 1, INT32_MIN + 1], r)
        fs.append(x)
        qs.append(q)
    return fs, qs


def _want4(orc, IN, OUT, fs, qs, R):
    s = orc.quant_sum(fs[:R], K32) if IN == F32 else orc.sum_q32(qs[:R])
    if OUT == F32:
        return orc.dequantise(s, K32).view(np.uint32)
    return orc.encode_be32(s) if OUT == Q32BE else s.view(np.uint32)


def _src_bits4(orc, IN, fs, qs, r):
    if IN == F32:
        return fs[r].view(np.uint32)
    return orc.encode_be32(qs[r]) if IN == Q32BE else qs[r].view(np.uint32)


PAIRS4 = [(i, o) for i in (F32, Q32, Q32BE) for o in (F32, Q32, Q32BE)]


@pytest.mark.parametrize("IN,OUT", PAIRS4, ids=[f"{NAMES[i]}-{NAMES[o]}" for i, o in PAIRS4])
def test_four_byte_kinds(gpu, IN, OUT):
    """all 9 pairs x R = 1..8 x two sizes x grid caps 0, 1, 2, and the first
    size with plain loads (NT = false) under caps 0 and 1"""
    from container_inc_amd import inccl
    orc = _orc()
    sat = orc.quantise(np.array([5000.0, -1e9, 2048.0, 2047.9998], np.float32), K32)
    assert list(sat[:3]) == [INT32_MAX, INT32_MIN, INT32_MAX] and sat[3] < INT32_MAX   # the inputs do saturate at K32
    for n in N4:
        fs, qs = _inputs4(n)
        srcs = [_Buf(gpu, IN, n, _src_bits4(orc, IN, fs, qs, r)) for r in range(8)]
        for R in range(1, 9):
            want = _want4(orc, IN, OUT, fs, qs, R)
            for cap, nt in [(0, True), (1, True), (2, True)] + ([(0, False), (1, False)] if n == N4[0] else []):
                out = _Buf(gpu, OUT, n)
                with _tuning(cap, nt):
                    inccl.stream_op(IN, OUT, [s.t for s in srcs[:R]], out=out.t, scale_exp=K32)
                np.testing.assert_array_equal(out.bits(), want, err_msg=f"n {n} R {R} cap {cap} nt {nt}")
        for s, r in zip(srcs, range(8)):
            np.testing.assert_array_equal(s.bits(), _src_bits4(orc, IN, fs, qs, r))     # the sources are only read


def test_in_place_under_one_workgroup(gpu):
    """dst aliases srcs[0], one workgroup takes every tile (cap 1): F32 -> F32 at R = 2"""
    from container_inc_amd import inccl
    orc = _orc()
    n = N4[0]
    fs, qs = _inputs4(n)
    srcs = [_Buf(gpu, F32, n, fs[r].view(np.uint32)) for r in range(2)]
    with _tuning(1):
        inccl.stream_op(F32, F32, [s.t for s in srcs], out=srcs[0].t, scale_exp=K32)
    np.testing.assert_array_equal(srcs[0].bits(), _want4(orc, F32, F32, fs, qs, 2))
    np.testing.assert_array_equal(srcs[1].bits(), fs[1].view(np.uint32))


# ---- two-byte kinds ----
def _bits16(kind, x):
    """fp32 values as bf16 (truncated) or fp16 (numpy's rounding) bit patterns"""
    x = np.asarray(x, np.float32)
    if kind == BF16:
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(over="ignore"):
        return x.astype(np.float16).view(np.uint16)


# NaN, +-Inf, the smallest subnormal, -0, the largest finite value of either sign
SPECIALS16 = {BF16: [0x7FC0, 0x7F80, 0xFF80, 0x0001, 0x8000, 0x7F7F, 0xFF7F, 0xFFC1],
              F16: [0x7E00, 0x7C00, 0xFC00, 0x0001, 0x8000, 0x7BFF, 0xFBFF, 0xFE01]}
# Q32 -> 16: sums (bucket 0 holds them, every other bucket 0 there) whose narrowing is an exact tie
# -- 2^m + 1 and 2^m + 3 at m = the format's significand bits, so that round to nearest even goes down
# for the first and up for the second -- then the overflow and the subnormal sums of K16_OUT
TIES = {BF16: [257, 259, -257, -259], F16: [2049, 2051, -2049, -2051]}
TIE_RESULTS = {BF16: [256, 260, -256, -260], F16: [2048, 2052, -2048, -2052]}
EDGE_SUMS = [INT32_MAX, INT32_MIN, 1, 3, -1]


@functools.lru_cache(maxsize=None)
def _inputs16(kind, n):
    """8 buckets of the 2-byte format with its specials; 8 int32 buckets whose
    planted sums (TIES, EDGE_SUMS) survive any R: only bucket 0 is non-zero there"""
    rng = np.random.default_rng(n + kind)
    hs, qs = [], []
    for r in range(8):
        h = _bits16(kind, rng.standard_normal(n) * 2.0)
        _plant(h, SPECIALS16[kind], r)
        q = rng.integers(INT32_MIN, INT32_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
        for off in _planted_at(n):
            q[off:off + 9] = (TIES[kind] + EDGE_SUMS) if r == 0 else 0
        hs.append(h)
        qs.append(q)
    return hs, qs


def _planted_at(n):
    """where the constructed sums sit: the first tile, the second, the ragged one, the tail"""
    return (16, 4096 + 40, n - 64, n - 9)


def _want16(orc, IN, OUT, hs, qs, R):
    f = "bf16" if BF16 in (IN, OUT) else "f16"
    if IN == Q32:
        return getattr(orc, f"sum_dequant_{f}")(qs[:R], K16_OUT)
    if OUT == Q32:
        return getattr(orc, f"quant_sum_{f}")(hs[:R], K16_IN).view(np.uint32)
    return getattr(orc, f"reduce_{f}")(hs[:R], K16_IN)


def _assert_constructed_cases(orc, kind, want, n):
    """the oracle's own Q32 -> 16 output shows the ties and, for fp16, the overflow and the subnormals"""
    scale = np.float32(2.0 ** -K16_OUT)
    for off in _planted_at(n):
        got = want[off:off + 9]
        ties = _bits16(kind, np.array(TIE_RESULTS[kind], np.float32) * scale)
        np.testing.assert_array_equal(got[:4], ties)
        inexact = np.array(TIES[kind], np.float32) * scale
        if kind == F16:
            assert (ties.view(np.float16).astype(np.float32) != inexact).all()        # each was rounded: down, up, ...
            assert list(got[4:6]) == [0x7C00, 0xFC00]                                  # +-65536 overflow to +-Inf
            assert list(got[6:9]) == [0x0200, 0x0600, 0x8200]                          # 2^-15, 3 * 2^-15, -2^-15: subnormals
        else:
            assert ((ties.astype(np.uint32) << 16).view(np.float32) != inexact).all()


PAIRS16 = [(BF16, BF16), (BF16, Q32), (Q32, BF16), (F16, F16), (F16, Q32), (Q32, F16)]


@pytest.mark.parametrize("IN,OUT", PAIRS16, ids=[f"{NAMES[i]}-{NAMES[o]}" for i, o in PAIRS16])
def test_two_byte_kinds(gpu, IN, OUT):
    """all 6 pairs x R = 1..8 x two sizes x grid caps 0, 1, 2; at R = 1 and 5
    also with every pointer 1 and 3 elements past a 16-B boundary (k_stream16_scalar
    throughout; the tail of every aligned call takes it as well)"""
    from container_inc_amd import inccl
    orc = _orc()
    kind = IN if IN != Q32 else OUT
    for n in N16:
        hs, qs = _inputs16(kind, n)
        bits = [(qs[r].view(np.uint32) if IN == Q32 else hs[r]) for r in range(8)]
        for shift in (0, 1, 3):
            srcs = [_Buf(gpu, IN, n, bits[r], shift) for r in range(8 if shift == 0 else 5)]
            for R in (range(1, 9) if shift == 0 else (1, 5)):
                want = _want16(orc, IN, OUT, hs, qs, R)
                if IN == Q32:
                    _assert_constructed_cases(orc, kind, want, n)
                for cap in (0, 1, 2):
                    out = _Buf(gpu, OUT, n, shift=shift)
                    with _tuning(cap):
                        inccl.stream_op(IN, OUT, [s.t for s in srcs[:R]], out=out.t,
                                        scale_exp=K16_OUT if IN == Q32 else K16_IN)
                    np.testing.assert_array_equal(out.bits(), want, err_msg=f"n {n} R {R} cap {cap} shift {shift}")


# ---- past the grid caps, from the device's CU count ----
@pytest.mark.parametrize("IN,OUT,R", [(F32, F32, 2), (Q32BE, Q32, 1), (BF16, BF16, 3), (Q32, F16, 2)],
                         ids=["F32-F32-R2", "Q32BE-Q32-R1", "BF16-BF16-R3", "Q32-F16-R2"])
def test_element_kernels_past_the_cap(gpu, IN, OUT, R):
    """every pointer one element past 16 B, n = 2048 * CUs + 1003: the last 1003
    elements are the second pass of k_stream_scalar / k_stream16_scalar"""
    from container_inc_amd import inccl
    orc = _orc()
    n = 2048 * _cus() + 1003
    if IN in (F32, Q32BE):
        fs, qs = _inputs4(n)
        bits = [_src_bits4(orc, IN, fs, qs, r) for r in range(R)]
        want, k = _want4(orc, IN, OUT, fs, qs, R), K32
    else:
        kind = IN if IN != Q32 else OUT
        hs, qs = _inputs16(kind, n)
        bits = [(qs[r].view(np.uint32) if IN == Q32 else hs[r]) for r in range(R)]
        want, k = _want16(orc, IN, OUT, hs, qs, R), K16_OUT if IN == Q32 else K16_IN
    srcs = [_Buf(gpu, IN, n, b, shift=1) for b in bits]
    out = _Buf(gpu, OUT, n, shift=1)
    inccl.stream_op(IN, OUT, [s.t for s in srcs], out=out.t, scale_exp=k)
    got = out.bits()
    np.testing.assert_array_equal(got[2048 * _cus():], want[2048 * _cus():], err_msg="the second pass")
    np.testing.assert_array_equal(got, want)


AM = {"f32": (F32, 4), "bf16": (BF16, 8), "f16": (F16, 8)}
AM_VALUES = {"f32": {"max": 0xC0F00000, "inf": 0xFF800000, "nan": 0x7FC00001},     # -7.5, -Inf, a NaN
             "bf16": {"max": 0xC0F0, "inf": 0xFF80, "nan": 0x7FC1},
             "f16": {"max": 0xC780, "inf": 0xFC00, "nan": 0x7E01}}


@functools.lru_cache(maxsize=None)
def _absmax_base(fmt, dev):
    """8 buckets of magnitudes below 1, n = EPQ * (2048 * CUs + 100) + 3: (host bit patterns, device buffers)"""
    kind, epq = AM[fmt]
    n = epq * (2048 * _cus() + 100) + 3
    rng = np.random.default_rng(epq)
    host = []
    for _ in range(8):
        x = rng.uniform(-0.99, 0.99, n).astype(np.float32)
        host.append(x.view(np.uint32) if fmt == "f32" else _bits16(kind, x))
    return host, [_Buf(dev, kind, n, h) for h in host]


def _orc_absmax(orc, fmt, hs, flagged):
    if flagged:
        return orc.absmax_word_flagged([h.view(np.float32) for h in hs] if fmt == "f32" else hs, fmt)
    f = {"f32": lambda: orc.absmax([h.view(np.float32) for h in hs]), "bf16": lambda: orc.absmax_bf16(hs),
         "f16": lambda: orc.absmax_f16(hs)}[fmt]()
    return int(np.array([f], np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("what", ["max_in_second_pass", "max_in_tail", "inf_in_second_pass", "nan_in_second_pass"])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
def test_absmax_past_the_cap(gpu, fmt, R, what):
    """One planted element of the last bucket decides the word: in the quads of
    the second pass (element index >= EPQ * 2048 * CUs), or in the 3-element
    tail.  The word is the oracle's, with INCCL_ABSMAX_FLAG_NONFINITE
    (absmax_word_flagged: an Inf or a NaN sets bit 31) and without (a NaN is
    ignored, an Inf is the maximum)."""
    import torch
    from container_inc_amd import inccl
    orc = _orc()
    kind, epq = AM[fmt]
    host, dev = _absmax_base(fmt, gpu)
    n = host[0].size
    at = n - 2 if what == "max_in_tail" else epq * 2048 * _cus() + epq * 37 + 1
    assert (at >= epq * (n // epq)) == (what == "max_in_tail") and at >= epq * 2048 * _cus()
    hs = list(host[:R])
    hs[R - 1] = hs[R - 1].copy()
    hs[R - 1][at] = AM_VALUES[fmt][what[:3]]
    last = _Buf(gpu, kind, n, hs[R - 1])
    ts = [b.t for b in dev[:R - 1]] + [last.t]
    plain, flagged = _orc_absmax(orc, fmt, hs, False), _orc_absmax(orc, fmt, hs, True)
    if what.startswith("max"):
        assert plain == flagged == 0x40F00000          # 7.5, widened
    elif what.startswith("inf"):
        assert plain == 0x7F800000 and flagged == 0xFF800000
    else:
        assert plain < 0x3F800000 and flagged >> 31 == 1
    assert inccl.absmax_bits(ts, nonfinite_flag=False) == plain
    assert inccl.absmax_bits(ts, nonfinite_flag=True) == flagged
    torch.cuda.synchronize()


@pytest.mark.parametrize("index_base", [0, 2 ** 32 - 1000])
def test_checksum_past_the_cap(gpu, index_base):
    """n = 4 * (2048 * CUs + 100) + 3 full-range int32 against the oracle;
    index_base 2^32 - 1000: the 32-bit weight wraps inside the array"""
    from container_inc_amd import inccl
    orc = _orc()
    n = 4 * (2048 * _cus() + 100) + 3
    q = np.random.default_rng(5).integers(INT32_MIN, INT32_MAX, n, dtype=np.int64, endpoint=True).astype(np.int32)
    buf = _Buf(gpu, Q32, n, q.view(np.uint32))
    assert inccl.checksum_q32(buf.t, index_base) == orc.checksum_q32(q, index_base)
    # the first pass alone gives another sum: the reference sees the second pass
    first = 4 * 2048 * _cus()
    assert orc.checksum_q32(q[:first], index_base) != orc.checksum_q32(q, index_base)


# ---- the tuning does not leak ----
def test_tuning_is_restored_after_a_failure(monkeypatch):
    """_tuning() puts (0, True) back when its body raises (no GPU call here: the calls are recorded)"""
    from container_inc_amd import inccl
    calls = []
    monkeypatch.setattr(inccl, "set_tuning", lambda cap=0, nt=True: calls.append((cap, nt)))
    with pytest.raises(AssertionError):
        with _tuning(2, False):
            raise AssertionError("a failing comparison")
    assert calls == [(2, False), (0, True)]


def test_default_grid_after_the_module(gpu):
    """the last test of the module: outside any _tuning(), one default-grid
    case (F32 -> F32, R = 2: one workgroup per tile, nontemporal loads) is bit-equal"""
    from container_inc_amd import inccl
    orc = _orc()
    n = N4[0]
    fs, qs = _inputs4(n)
    srcs = [_Buf(gpu, F32, n, fs[r].view(np.uint32)) for r in range(2)]
    out = _Buf(gpu, F32, n)
    inccl.stream_op(F32, F32, [s.t for s in srcs], out=out.t, scale_exp=K32)
    np.testing.assert_array_equal(out.bits(), _want4(orc, F32, F32, fs, qs, 2))
