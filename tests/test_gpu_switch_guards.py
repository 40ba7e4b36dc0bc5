"""What the switch dataplane must NOT write (gpu): every output of every call --
out, out_len, action, psn, the ICRC words -- lives in a tests/guarded.py buffer,
so its allocation's guards and every byte of `out` the oracle does not send are
checked against the sentinel they were filled with.

inccl_switch_egress's contract (include/inccl_amd.h): out_len[row] is the
frame's bytes or 0; a row that is not sent keeps what the buffer held; bytes
past a frame, up to its 16-byte rounded length, are written as zero or left as
they were; nothing further is touched.  The frames, ports and templates are
inputs and must only be read.

The geometry is varied on its own here: out_stride apart from stride, and the
bases of `frames` and `out` 0 / 4 / 8 / 12 bytes past a 16-byte boundary -- the
16-byte egress path (`out` and out_stride both 16-byte aligned) and the wide
ingress path (`frames` and stride both) are chosen independently, each by the
pointer as well as by the stride.  out_stride 1104 is the one at which a
WRITE_FIRST row's second 16-byte store ends exactly at the row's end.  Ingress
takes a frame whose payload fits the row, 54 + 16 wf + 1024 <= stride: the
input strides either side of that for both kinds of frame, for the switch and
for the standalone ICRC (14 + ip_total <= stride).

Expected actions and frames: the oracle's serial pipeline() on the same frame
sequence, byte for byte.  Every batch test runs both ways of driving the
switch (test_gpu_switch.MODES)."""
import numpy as np
import pytest

from guarded import SENT, Buf
from test_gpu_switch import ACK, MODES, WF_OPS, _host_frame, _random_op, _rows_host, _run, _templates
from test_gpu_switch_nonroot import _amap, _batch_items

gpu_test = pytest.mark.gpu   # every test but the checker's self-check, which the CPU suite runs
SENT_BYTE = SENT[4] & 0xFF
assert SENT[4] == SENT_BYTE * 0x01010101   # every byte of a guarded i32 buffer starts as SENT_BYTE
PER_BATCH = 8                              # PSNs per batch: 8 b .. 8 b + 7


def _round16(n):
    return (n + 15) & ~15


def _egress_chunk(fan_in):
    """input frames per egress wave at a time: a copy of egress_chunk() in
    inccl_frames.hip, which says so there -- change both together"""
    return 4 if fan_in <= 8 else 16


def _check_rows(expected, rows, out, out_len, out_stride, tag):
    """The checker.  expected[i] = (action, [the bytes the oracle sends to row
    c, or None]) for input frame i; out [count * rows, out_stride] uint8 and
    out_len [count * rows] as the GPU left buffers that held the sentinel.
    A row the oracle does not send: out_len 0 and all out_stride bytes the
    sentinel.  A row of L bytes: out_len L, bytes [0, L) the oracle's, bytes
    [L, round_up(L, 16)) each zero or the sentinel, the rest the sentinel."""
    assert out.shape == (len(expected) * rows, out_stride) and out_len.shape == (len(expected) * rows,)
    for i, (_, outs) in enumerate(expected):
        assert len(outs) == rows
        for c in range(rows):
            row = i * rows + c
            got = out[row]
            if outs[c] is None:
                assert out_len[row] == 0, (tag, i, c, "out_len of a row that is not sent", int(out_len[row]))
                bad = np.nonzero(got != SENT_BYTE)[0]
                assert bad.size == 0, (tag, i, c, "a row that is not sent was written at bytes", bad[:8].tolist())
                continue
            L = len(outs[c])
            assert L in (62, 1082, 1098), (tag, i, c, L)
            assert out_len[row] == L, (tag, i, c, int(out_len[row]), L)
            assert got[:L].tobytes() == outs[c], (tag, i, c, "frame bytes differ")
            end = min(_round16(L), out_stride)
            slack = got[L:end]
            assert ((slack == 0) | (slack == SENT_BYTE)).all(), (tag, i, c, "bytes past the frame", slack.tolist())
            bad = np.nonzero(got[end:] != SENT_BYTE)[0]
            assert bad.size == 0, (tag, i, c, "written past the frame's 16-byte rounded length at bytes",
                                   (bad[:8] + end).tolist())


def _root_items(rng, fan_in, b, per_batch=PER_BATCH):
    """One root batch, as test_switch_batches builds it: PSNs per_batch b ..,
    first copies from every port, a quarter of them again, three late copies of
    the previous batch, ACKs, an ignored opcode, a port past the last; shuffled.
    Every copy carries its own opcode (SEND / WRITE / WRITE_FIRST mixed in a PSN)."""
    keys = [(p, port) for p in range(b * per_batch, (b + 1) * per_batch) for port in range(fan_in)]
    dups = [keys[i] for i in rng.choice(len(keys), size=len(keys) // 4, replace=False)]
    old = [(p, port) for p in range(max(0, (b - 1) * per_batch), b * per_batch) for port in range(fan_in)]
    olds = [old[i] for i in rng.choice(len(old), size=min(3, len(old)), replace=False)] if old else []
    items = [(p, port, _random_op(rng)) for (p, port) in keys + dups + olds]
    items += [(int(rng.integers(0, 1 << 24)), int(rng.integers(0, fan_in)), ACK) for _ in range(fan_in + 2)]
    items += [(b * per_batch, 0, 0x64), (b * per_batch + 1, fan_in, 0x07)]
    return [items[i] for i in rng.permutation(len(items))]


def _plan(orc, rng, fan_in, nonroot, batches, stride):
    """`batches` batches of one switch: [(items, frames cut to the row)].  A
    non-root's batch is test_nonroot_batches' (parent results among the
    children's copies, some before the children complete), then the parent's
    result for every PSN of the batch before and three late copies from
    children after it: at a large fan-in the shuffled ones alone rarely follow
    their PSN's last child, and DOWN and REPLAY would not occur."""
    plan, prev = [], []
    for b in range(batches):
        psns = list(range(b * PER_BATCH, (b + 1) * PER_BATCH))
        if nonroot:
            items = _batch_items(rng, fan_in, psns, prev)
            items += [(p, fan_in, _random_op(rng)) for p in prev]
            items += [(int(rng.choice(prev)), int(rng.integers(0, fan_in)), _random_op(rng)) for _ in range(3 if prev else 0)]
        else:
            items = _root_items(rng, fan_in, b)
        prev = psns
        plan.append((items, [_host_frame(orc, rng, p, port, op)[:stride] for (p, port, op) in items]))
    return plan


def _oracle(ref, tmpl, frames, ports, stride):
    """[(action, rows sent)] of the oracle's serial pipeline() over one batch"""
    return [ref.pipeline(tmpl, port, f, stride) for f, port in zip(frames, ports)]


def _gpu_batch(gpu, inccl, orc, sw, mode, tmpl_buf, items, frames, expected, stride, out_stride, fshift, oshift, tag):
    """One batch through the GPU switch with every buffer guarded, then the
    checker, the actions and PSNs, the allocation guards and the inputs."""
    import torch
    count, rows = len(items), sw.rows
    ports = [port for (_, port, _) in items]
    fr = Buf(gpu, "i32", count * stride // 4, _rows_host(frames, stride).reshape(-1), shift=fshift)
    pt = Buf(gpu, "i32", count, np.array(ports, np.int32))
    out = Buf(gpu, "i32", count * rows * out_stride // 4, shift=oshift)
    out_len, action, psn = Buf(gpu, "i32", count * rows), Buf(gpu, "i32", count), Buf(gpu, "i32", count)
    _run(sw, mode, fr.t.view(torch.uint8).view(count, stride), pt.t, tmpl_buf.t.view(torch.uint8),
         out_stride=out_stride, out=out.t.view(torch.uint8).view(count * rows, out_stride), out_len=out_len.t,
         action=action.t, psn=psn.t)
    torch.cuda.synchronize()
    act, q = action.bits().view(np.int32), psn.bits()
    amap = _amap(orc, inccl)
    for i, ((p, port, op), (rc, _)) in enumerate(zip(items, expected)):
        assert int(act[i]) == amap[rc], (tag, i, port, op, int(act[i]), amap[rc])
        if port < rows:   # (as the existing tests: the header promises no PSN for a port the switch does not have)
            assert int(q[i]) == p, (tag, i, int(q[i]), p)
    _check_rows(expected, rows, out.bits().view(np.uint8).reshape(count * rows, out_stride),
                out_len.bits().view(np.int32), out_stride, tag)
    for b in (fr, pt, tmpl_buf):
        b.assert_unchanged()


def _tally(expected, total):
    for rc, _ in expected:
        total[rc] = total.get(rc, 0) + 1


# stride -> out_stride, the words `frames` / `out` start past 16 B (x 4 bytes), fan-in, non-root flags (None: root)
MATRIX = [
    (1152, 1104, 0, 0, 2, None),    # the 16-byte egress at its smallest stride
    (1152, 1104, 0, 0, 20, None),   # ... with the children loop, chunks of 16
    (1152, 1104, 0, 0, 3, 3),       # ... non-root
    (1152, 1100, 0, 0, 4, None),    # wide ingress with dword egress
    (1100, 1152, 0, 0, 8, None),    # narrow ingress with 16-byte egress
    (1152, 1152, 1, 0, 2, None),    # narrow by the pointer alone
    (1152, 1152, 0, 2, 2, None),    # dword egress by the pointer alone
    (1152, 1152, 3, 3, 5, 0),       # both by the pointer, children loop, non-root
    (1104, 1240, 0, 0, 3, None),    # strides that are no multiple of 64
    (1104, 1240, 0, 1, 31, 1),      # ... non-root, the parent's RETH past the keeper prefetch
]


@gpu_test
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride,out_stride,fshift,oshift,fan_in,flags", MATRIX)
def test_switch_writes_only_what_it_reports(gpu, orc, stride, out_stride, fshift, oshift, fan_in, flags, mode):
    from container_inc_amd import inccl
    nonroot = flags is not None
    rng = np.random.default_rng(2000 + 37 * fan_in + stride + out_stride + 4 * fshift + oshift)
    batches = 2 if fan_in >= 20 else 3
    sw = inccl.GpuSwitch(fan_in, 64, nonroot=nonroot, flags=flags or 0)
    ref = orc.Switch(fan_in, 64, nonroot=nonroot, flags=flags or 0)
    tmpl = _templates(sw.rows)
    tmpl_buf = Buf(gpu, "i32", 7 * sw.rows, tmpl.view(np.uint32))
    plan = _plan(orc, rng, fan_in, nonroot, batches, stride)
    # a partial last chunk: the out_len store loop's bound is then inside the chunk
    assert any(len(items) % _egress_chunk(fan_in) for items, _ in plan)
    total = {}
    for b, (items, frames) in enumerate(plan):
        expected = _oracle(ref, tmpl, frames, [port for (_, port, _) in items], stride)
        _tally(expected, total)
        _gpu_batch(gpu, inccl, orc, sw, mode, tmpl_buf, items, frames, expected, stride, out_stride, fshift, oshift, b)
    want = [orc.SW_REPLAY, orc.SW_DROPPED, orc.SW_ACK, orc.SW_IGNORED, orc.SW_INVALID, orc.SW_ABSORBED]
    want += [orc.SW_FORWARD, orc.SW_DOWN] if nonroot else [orc.SW_BROADCAST]
    for k in want:
        assert total.get(k, 0) > 0, (k, total)
    sw.destroy()


@gpu_test
@pytest.mark.parametrize("mode", MODES)
def test_switch_single_frame_batches(gpu, orc, mode):
    """Batches of one frame (one lane of one chunk) on the 16-byte egress at
    out_stride 1104: a first copy (nothing sent), the copy that completes the
    PSN (both rows, 1098 B: the row's last byte), a late copy (one row), an
    ACK (62 B) and a port past the last."""
    from container_inc_amd import inccl
    rng = np.random.default_rng(2100)
    sw, ref = inccl.GpuSwitch(2, 16), orc.Switch(2, 16)
    tmpl = _templates(2)
    tmpl_buf = Buf(gpu, "i32", 7 * 2, tmpl.view(np.uint32))
    seq = [(5, 0, 0x07), (5, 1, 0x06), (5, 0, 0x0A), (9, 1, ACK), (5, 2, 0x07)]
    want = [orc.SW_ABSORBED, orc.SW_BROADCAST, orc.SW_REPLAY, orc.SW_ACK, orc.SW_INVALID]
    for b, (item, rc) in enumerate(zip(seq, want)):
        frames = [_host_frame(orc, rng, *item)]
        expected = _oracle(ref, tmpl, frames, [item[1]], 1152)
        assert expected[0][0] == rc, (b, expected[0][0])
        _gpu_batch(gpu, inccl, orc, sw, mode, tmpl_buf, [item], frames, expected, 1152, 1104, 0, 0, b)
    sw.destroy()


# stride: (a frame without a RETH is counted, a WRITE_FIRST / ONLY frame is counted):
# 54 + 1024 = 1078 and 70 + 1024 = 1094 bytes must fit the row
EDGE_STRIDES = {1076: (False, False), 1080: (True, False), 1088: (True, False), 1092: (True, False),
                1096: (True, True), 1104: (True, True)}


@gpu_test
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("stride", sorted(EDGE_STRIDES))
def test_switch_input_stride_edges(gpu, orc, stride, mode):
    """Rows that end just before and just after a frame's payload (frames cut
    off at the row's end; root, fan-in 2, out_stride 1152).  1088 and 1104 are
    16-byte rows: lane 63 of the wide payload load reads the row's last bytes.
    The actions are known answers, which the oracle must give before the GPU
    is asked; ACKs are reflected at every stride, and where a PSN completes its
    rows (summed from rows that end 2 or 8 bytes after the payload) go through
    the checker."""
    from container_inc_amd import inccl
    plain_ok, wf_ok = EDGE_STRIDES[stride]
    fan_in = 2
    rng = np.random.default_rng(2200 + stride)
    sw, ref = inccl.GpuSwitch(fan_in, 64), orc.Switch(fan_in, 64)
    tmpl = _templates(fan_in)
    tmpl_buf = Buf(gpu, "i32", 7 * fan_in, tmpl.view(np.uint32))
    counted = (orc.SW_ABSORBED, orc.SW_BROADCAST, orc.SW_DROPPED, orc.SW_REPLAY)
    total = {}
    for b, (items, frames) in enumerate(_plan(orc, rng, fan_in, False, 3, stride)):
        expected = _oracle(ref, tmpl, frames, [port for (_, port, _) in items], stride)
        for (p, port, op), (rc, _) in zip(items, expected):
            if port >= fan_in:
                assert rc == orc.SW_INVALID
            elif op == ACK:
                assert rc == orc.SW_ACK
            elif op == 0x64:
                assert rc == orc.SW_IGNORED
            elif wf_ok if op in WF_OPS else plain_ok:
                assert rc in counted, (stride, op, rc)
            else:
                assert rc == orc.SW_INVALID, (stride, op, rc)
        _tally(expected, total)
        _gpu_batch(gpu, inccl, orc, sw, mode, tmpl_buf, items, frames, expected, stride, 1152, 0, 0, b)
    assert total.get(orc.SW_ACK, 0) > 0 and total.get(orc.SW_INVALID, 0) > 0, total
    if plain_ok:   # some PSN's copies were all without a RETH: it completed
        assert total.get(orc.SW_BROADCAST, 0) > 0 and total.get(orc.SW_ABSORBED, 0) > 0, total
    else:
        assert not any(total.get(k, 0) for k in counted), total
    if wf_ok:
        assert total.get(orc.SW_REPLAY, 0) > 0 and total.get(orc.SW_DROPPED, 0) > 0, total
    sw.destroy()


@gpu_test
@pytest.mark.parametrize("stride,fshift", [(s, 0) for s in sorted(EDGE_STRIDES)] + [(1104, 1), (1104, 3)])
def test_icrc_input_stride_edges(gpu, orc, stride, fshift):
    """inccl_icrc_frames on rows of the same strides holding 1082-B and 1098-B
    frames cut off at the row's end: the ICRC where the whole frame lies inside
    the row (14 + ip_total <= stride), else 0.  Once more with `frames` 4 and
    12 bytes past a 16-byte boundary; an odd count (the two-frames-per-wave
    kernel's lone last frame) into a guarded result buffer."""
    import torch
    from container_inc_amd import inccl
    rng = np.random.default_rng(2300 + stride + fshift)
    ops = [0x07, 0x06, 0x0A, 0x08, 0x06, 0x07, 0x04]
    full = [_host_frame(orc, rng, int(rng.integers(0, 1 << 24)), 0, op) for op in ops]
    assert sorted({len(f) for f in full}) == [1082, 1098]
    count = len(full)
    fr = Buf(gpu, "i32", count * stride // 4, _rows_host(full, stride).reshape(-1), shift=fshift)
    out = Buf(gpu, "i32", count)
    got = inccl.icrc_frames(fr.t.view(torch.uint8).view(count, stride), out=out.t)
    assert got.data_ptr() == out.t.data_ptr()
    res = out.bits()
    inside = {1082: stride >= 1082, 1098: stride >= 1098}
    assert inside[1082] == (stride >= 1088) and inside[1098] == (stride == 1104)   # of the strides of this test
    for i, f in enumerate(full):
        want = orc.icrc(f) if inside[len(f)] else 0
        assert int(res[i]) == want, (stride, i, len(f), int(res[i]), want)
        assert orc.icrc(f) == int.from_bytes(f[-4:], "little") != 0
    fr.assert_unchanged()


def test_checker_catches_a_touched_row():
    """The checker itself, without the GPU: a correct buffer passes; one byte
    changed at a frame's 16-byte rounded length, inside a row that is not sent,
    a byte other than zero in the slack, and a changed out_len of a row that
    is not sent each fail."""
    rng = np.random.default_rng(2400)
    for L, out_stride in ((1082, 1104), (1098, 1104), (1098, 1100), (62, 1152)):
        frame = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        expected = [(0, [frame, None]), (0, [None, None])]
        out = np.full((4, out_stride), SENT_BYTE, np.uint8)
        out[0, :L] = np.frombuffer(frame, np.uint8)
        out[0, L:min(L + 2, out_stride)] = 0
        out_len = np.array([L, 0, 0, 0], np.int32)
        _check_rows(expected, 2, out, out_len, out_stride, "good")
        muts = [(1, 0, 0), (3, out_stride - 1, 0), (0, L, 1)]
        if _round16(L) < out_stride:
            muts += [(0, _round16(L), 0), (0, out_stride - 1, 0)]
        for row, at, val in muts:
            bad = out.copy()
            bad[row, at] = val
            with pytest.raises(AssertionError):
                _check_rows(expected, 2, bad, out_len, out_stride, "bad")
        for row, val in ((1, 62), (3, SENT[4])):
            bad_len = out_len.copy()
            bad_len[row] = val
            with pytest.raises(AssertionError):
                _check_rows(expected, 2, out, bad_len, out_stride, "bad")
