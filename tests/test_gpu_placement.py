"""GPU tier: every single-object call on every memory placement.

One matrix, operation x placement, every cell checked byte for byte against the
CPU oracle (for leo_amd_verify: the expected mismatch set and count, and that
no piece changed).

Operations: leo_encode, leo_decode, leo_amd_update, leo_amd_repair,
leo_amd_verify.  Placements of the pieces:

* device      rows of torch tensors on the GPU;
* direct      rows of one numpy array per piece array (a few row runs: direct
              SDMA copies between the caller's memory and device rows);
* ring        one allocation per piece, handed over in descending address
              order, so no two pieces of an array form a run and the call has
              more than 16 runs (two arrays that happen to follow each other in
              memory can merge one run at their seam: at most three fewer, and
              the smallest call here has 21): the gather / scatter ring;
* registered  as direct, every array in whole pages of its own and registered
              with leo_amd_register_host;
* fanout      as direct with leo_amd_set_fanout(3) on 12,352-byte pieces (193
              blocks of 64 bytes: three ranges that cannot be equal).  Encode
              and decode split their columns over the workers; update and
              verify run on one device and must simply stay correct.  (Repair
              fans out too, but has no cell here: see test_repair.)
"""
import contextlib
import functools
import mmap

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

FILL = 0x5A   # sentinel of every output buffer
JUNK = 0xEE   # what the buffers of lost pieces hold (never passed to the library)

# field -> K, R, piece bytes, lost originals, lost recovery pieces, changed originals of an update
SHAPES = {"gf8": (100, 10, 2560, 4, 6, [7, 99]), "gf16": (1000, 200, 128, 64, 136, [0, 999])}
FANOUT_BYTES = 12352
PLACEMENTS = ["device", "direct", "ring", "registered", "fanout"]
matrix = pytest.mark.parametrize("field,placement", [(f, p) for f in SHAPES for p in PLACEMENTS])

# Above 4 MiB of staged rows the ring cuts at least four column slices.  100+10:
# encode stages 110 rows, decode 100 + 4, repair 100 + 10, verify 109 or 110, so
# 40,960-byte pieces do it; update stages C + 2R = 22 rows, and 190,656 bytes
# (2979 blocks) is the first multiple of 64 with 22 rows above 4 MiB.
MULTI_SLICE_BYTES = 40960
MULTI_SLICE_UPDATE_BYTES = 190656
assert 104 * MULTI_SLICE_BYTES > 4 << 20 and 22 * MULTI_SLICE_UPDATE_BYTES > 4 << 20 >= 22 * (MULTI_SLICE_UPDATE_BYTES - 64)


@functools.lru_cache(maxsize=None)
def _codeword(k, r, b):
    """(originals, recovery) of one shape; shared between tests, never modified."""
    data = np.random.default_rng(17 * k + r + b).integers(0, 256, (k, b), dtype=np.uint8)
    rec = np.bitwise_xor.reduce(data, axis=0, keepdims=True) if r == 1 else ol.oracle().encode(data, r)
    data.setflags(write=False)
    rec.setflags(write=False)
    return data, rec


@functools.lru_cache(maxsize=None)
def _updated(k, r, b, idx):
    """(deltas, recovery of the originals with original idx[t] ^= deltas[t])."""
    data, _ = _codeword(k, r, b)
    deltas = np.random.default_rng(k + 3 * b).integers(0, 256, (len(idx), b), dtype=np.uint8)
    new = data.copy()
    new[list(idx)] ^= deltas
    rec = ol.oracle().encode(new, r)
    deltas.setflags(write=False)
    rec.setflags(write=False)
    return deltas, rec


def _pattern(k, r, nlo, nlr):
    rng = np.random.default_rng(13 * k + r + 101 * nlo + nlr)
    return sorted(rng.choice(k, nlo, replace=False).tolist()), sorted(rng.choice(r, nlr, replace=False).tolist())


class _Rows:
    """The pieces of one array of a call: .ptrs (addresses) and .numpy() (contents now)."""

    def __init__(self, kind, src):
        self.kind = kind
        if kind == "device":
            import torch
            self.t = torch.from_numpy(src).to("cuda:0")
            self.ptrs = [self.t[i].data_ptr() for i in range(len(src))]
        elif kind == "ring":
            self.v = sorted((np.empty(src.shape[1], dtype=np.uint8) for _ in range(len(src))),
                            key=lambda x: -x.ctypes.data)
            for dst, row in zip(self.v, src):
                dst[:] = row
            self.ptrs = [x.ctypes.data for x in self.v]
        else:
            self.a = src
            self.ptrs = [src[i].ctypes.data for i in range(len(src))]

    def numpy(self):
        if self.kind == "device":
            import torch
            torch.cuda.synchronize()
            return self.t.cpu().numpy()
        return np.stack(self.v) if self.kind == "ring" else self.a


class _Place:
    """One placement for the length of a call: rows() lays an array out."""

    def __init__(self, leo, placement, regs):
        self.leo, self.placement, self.regs = leo, placement, regs

    def rows(self, fill, n=None, b=None):
        src = np.full((n, b), fill, dtype=np.uint8) if n is not None else np.array(fill)
        if self.placement == "registered":
            # Whole pages of a mapping of its own: registration pins pages, and a page shared with
            # another registered array, or with heap memory that lives on and is later copied to the
            # GPU from, must not be pinned and released under them.
            pages = mmap.mmap(-1, (src.nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE)
            own = np.frombuffer(pages, dtype=np.uint8, count=src.nbytes).reshape(src.shape)
            own[:] = src
            src = own
            assert self.leo.register_host(src.ctypes.data, len(pages)) == self.leo.LeopardResult.Success, \
                self.leo.last_error()
            self.regs.append(src)
        return _Rows(self.placement, src)


@contextlib.contextmanager
def _placed(leo, placement):
    regs = []
    if placement == "fanout":
        leo.set_fanout(3)
    try:
        yield _Place(leo, placement, regs)
    finally:
        leo.set_fanout(0)
        for a in regs:
            assert leo.unregister_host(a.ctypes.data) == leo.LeopardResult.Success


def _masked(ptrs, lost):
    lost = set(lost)
    return [None if i in lost else p for i, p in enumerate(ptrs)]


def _bits(bitmap, r):
    return [j for j in range(r) if (int(bitmap[j >> 5]) >> (j & 31)) & 1]


# ------------------------------------------------------- the five operations --
# Each takes a placement and a shape, runs the call and checks every byte.

def _encode(leo, p, k, r, b):
    data, rec = _codeword(k, r, b)
    wc = leo.leo_encode_work_count(k, r)
    orig, work = p.rows(data), p.rows(FILL, wc, b)
    assert leo.leo_encode(b, k, r, wc, orig.ptrs, work.ptrs) == leo.LeopardResult.Success, leo.last_error()
    assert np.array_equal(work.numpy()[:r], rec)
    assert np.array_equal(orig.numpy(), data), "an original changed"


def _lossy(p, k, r, b, lo, lr):
    """The received pieces of a codeword (lost rows hold JUNK and are never passed)."""
    data, rec = _codeword(k, r, b)
    h_orig, h_rec = np.array(data), np.array(rec)
    h_orig[lo] = JUNK
    h_rec[lr] = JUNK
    return data, rec, h_orig, h_rec, p.rows(h_orig), p.rows(h_rec)


def _decode(leo, p, k, r, b, nlo, nlr):
    lo, lr = _pattern(k, r, nlo, nlr)
    data, _, h_orig, h_rec, orig, recv = _lossy(p, k, r, b, lo, lr)
    wc = leo.leo_decode_work_count(k, r)
    work = p.rows(FILL, wc, b)
    res = leo.leo_decode(b, k, r, wc, _masked(orig.ptrs, lo), _masked(recv.ptrs, lr), work.ptrs)
    assert res == leo.LeopardResult.Success, leo.last_error()
    assert np.array_equal(work.numpy()[lo], data[lo])
    assert np.array_equal(orig.numpy(), h_orig) and np.array_equal(recv.numpy(), h_rec), "a received piece changed"


def _update(leo, p, k, r, b, idx, cols=None):
    """cols = (offset, bytes): leo_amd_update_slice; bytes outside keep the old recovery."""
    _, rec = _codeword(k, r, b)
    deltas, new = _updated(k, r, b, tuple(idx))
    d, rv = p.rows(deltas), p.rows(rec)
    if cols is None:
        res = leo.leo_amd_update(b, k, r, len(idx), idx, d.ptrs, rv.ptrs)
        expect = new
    else:
        res = leo.leo_amd_update_slice(b, cols[0], cols[1], k, r, len(idx), idx, d.ptrs, rv.ptrs)
        expect = np.array(rec)
        expect[:, cols[0]:cols[0] + cols[1]] = new[:, cols[0]:cols[0] + cols[1]]
    assert res == leo.LeopardResult.Success, leo.last_error()
    assert np.array_equal(rv.numpy(), expect)
    assert np.array_equal(d.numpy(), deltas), "a delta changed"


def _repair(leo, p, k, r, b, nlo, nlr, cols=None):
    """Every lost recovery piece is requested; work and recovery_out hold the
    sentinel wherever the call has nothing to write (cols: outside the slice)."""
    lo, lr = _pattern(k, r, nlo, nlr)
    data, rec, h_orig, h_rec, orig, recv = _lossy(p, k, r, b, lo, lr)
    wc = leo.leo_decode_work_count(k, r)
    work, rout = p.rows(FILL, k, b), p.rows(FILL, r, b)
    args = (k, r, wc, _masked(orig.ptrs, lo), _masked(recv.ptrs, lr), work.ptrs + [None] * (wc - k), rout.ptrs)
    res = leo.leo_amd_repair(b, *args) if cols is None else leo.leo_amd_repair_slice(b, cols[0], cols[1], *args)
    assert res == leo.LeopardResult.Success, leo.last_error()
    c0, c1 = (0, b) if cols is None else (cols[0], cols[0] + cols[1])
    exp_work, exp_rout = np.full((k, b), FILL, dtype=np.uint8), np.full((r, b), FILL, dtype=np.uint8)
    exp_work[lo, c0:c1] = data[lo, c0:c1]
    exp_rout[lr, c0:c1] = rec[lr, c0:c1]
    assert np.array_equal(work.numpy(), exp_work)
    assert np.array_equal(rout.numpy(), exp_rout)
    assert np.array_equal(orig.numpy(), h_orig) and np.array_equal(recv.numpy(), h_rec), "a received piece changed"


def _verify(leo, p, k, r, b, flips, skip=(), cols=None):
    """flips: (stored piece, byte) pairs with one bit flipped; skip: pieces not checked."""
    data, rec = _codeword(k, r, b)
    stored = np.array(rec)
    for j, col in flips:
        stored[j, col] ^= 0x40
    orig, st = p.rows(data), p.rows(stored)
    args = (k, r, orig.ptrs, _masked(st.ptrs, skip))
    res, count, bitmap = leo.leo_amd_verify(b, *args) if cols is None else \
        leo.leo_amd_verify_slice(b, cols[0], cols[1], *args)
    assert res == leo.LeopardResult.Success, leo.last_error()
    c0, c1 = (0, b) if cols is None else (cols[0], cols[0] + cols[1])
    expect = sorted({j for j, col in flips if j not in skip and c0 <= col < c1})
    assert (_bits(bitmap, r), count) == (expect, len(expect))
    assert np.array_equal(orig.numpy(), data) and np.array_equal(st.numpy(), stored), "a piece changed"


def _flips(r, b):
    """Pieces 1 and R - 1 differ (first and last byte); piece 2 differs but is not checked."""
    return [(1, 0), (r - 1, b - 1), (2, 17)], (2, 5)


def _shape(field, placement):
    k, r, b, nlo, nlr, idx = SHAPES[field]
    return k, r, FANOUT_BYTES if placement == "fanout" else b, nlo, nlr, idx


# ----------------------------------------------------------------- the matrix --

@matrix
def test_encode(leo, field, placement):
    k, r, b, _, _, _ = _shape(field, placement)
    with _placed(leo, placement) as p:
        _encode(leo, p, k, r, b)


@matrix
def test_decode(leo, field, placement):
    k, r, b, nlo, nlr, _ = _shape(field, placement)
    with _placed(leo, placement) as p:
        _decode(leo, p, k, r, b, nlo, nlr)


@matrix
def test_update(leo, field, placement):
    k, r, b, _, _, idx = _shape(field, placement)
    with _placed(leo, placement) as p:
        _update(leo, p, k, r, b, idx)


@pytest.mark.parametrize("field,placement", [(f, p) for f in SHAPES for p in PLACEMENTS if p != "fanout"])
def test_repair(leo, field, placement):
    """No fan-out cell yet: a leo_amd_repair call under fan-out (100+10 x 12,352 B,
    4 + 6 lost, three ranges) has ended in a GPU memory fault of unknown cause, so
    no test runs that path until the cause is known."""
    k, r, b, nlo, nlr, _ = _shape(field, placement)
    with _placed(leo, placement) as p:
        _repair(leo, p, k, r, b, nlo, nlr)


@matrix
def test_verify(leo, field, placement):
    k, r, b, _, _, _ = _shape(field, placement)
    with _placed(leo, placement) as p:
        _verify(leo, p, k, r, b, *_flips(r, b))


@pytest.mark.parametrize("placement", ["ring", "registered"])
def test_one_recovery_piece(leo, placement):
    """R = 1, 20+1 x 192 B: the XOR of the pieces, one original lost on decode."""
    with _placed(leo, placement) as p:
        _encode(leo, p, 20, 1, 192)
        _decode(leo, p, 20, 1, 192, 1, 0)


@pytest.mark.parametrize("op", ["encode", "decode", "update", "repair", "verify"])
def test_ring_of_several_slices(leo, op):
    """100+10 with more than 4 MiB of staged rows: the ring cuts at least four slices."""
    k, r, b, nlo, nlr, idx = SHAPES["gf8"]
    b = MULTI_SLICE_UPDATE_BYTES if op == "update" else MULTI_SLICE_BYTES
    with _placed(leo, "ring") as p:
        if op == "encode":
            _encode(leo, p, k, r, b)
        elif op == "decode":
            _decode(leo, p, k, r, b, nlo, nlr)
        elif op == "update":
            _update(leo, p, k, r, b, idx)
        elif op == "repair":
            _repair(leo, p, k, r, b, nlo, nlr)
        else:
            _verify(leo, p, k, r, b, *_flips(r, b))


def test_verify_ring_last_block_of_last_slice(leo):
    """One bit in the last 64-byte block of the last ring slice: exactly that piece."""
    k, r, b = 100, 10, MULTI_SLICE_BYTES
    with _placed(leo, "ring") as p:
        _verify(leo, p, k, r, b, [(7, b - 37)])


# ------------------------------------------------------ slices on host memory --
# *_slice at a non-zero 64-byte-aligned offset, ring placement: bytes outside
# the slice stay as they were.

SLICE = (640, 1280)  # of 2560-byte pieces


def test_update_slice_on_the_ring(leo):
    k, r, b, _, _, idx = SHAPES["gf8"]
    with _placed(leo, "ring") as p:
        _update(leo, p, k, r, b, idx, cols=SLICE)


def test_repair_slice_on_the_ring(leo):
    k, r, b, nlo, nlr, _ = SHAPES["gf8"]
    with _placed(leo, "ring") as p:
        _repair(leo, p, k, r, b, nlo, nlr, cols=SLICE)


def test_verify_slice_on_the_ring(leo):
    """Differences in front of, inside and behind the slice: only the one inside is reported."""
    k, r, b, _, _, _ = SHAPES["gf8"]
    with _placed(leo, "ring") as p:
        _verify(leo, p, k, r, b, [(0, 639), (4, 640), (9, 1920)], cols=SLICE)


# ------------------------------------------------- NULL outputs on host memory --

@pytest.mark.parametrize("fanout", [0, 3])
def test_null_output_piece_on_host_memory(leo, fanout):
    """A NULL destination of a piece the call writes, host memory, with and without fan-out
    (FANOUT_BYTES pieces: three ranges).

    * leo_encode: InvalidInput, last_error names work_data[j]; decided where the work is
      done, so under fan-out it is a worker's error that reaches the caller.
    * leo_decode: the same for the work piece of a lost original.
    * leo_amd_repair: InvalidInput naming work_data[i], decided in the validation, before
      any routing (so fan-out plays no part); a NULL recovery_out entry of a lost piece is
      no error: that piece is not requested, and the others are rebuilt.
    * leo_amd_update: InvalidInput naming recovery_data[j], decided in the validation."""
    k, r, b, nlo, nlr, idx = SHAPES["gf8"]
    b = FANOUT_BYTES
    inv = leo.LeopardResult.InvalidInput
    lo, lr = _pattern(k, r, nlo, nlr)
    with _placed(leo, "direct") as p:
        data, rec, _, _, orig, recv = _lossy(p, k, r, b, lo, lr)
        full = p.rows(data)
        wc, dwc = leo.leo_encode_work_count(k, r), leo.leo_decode_work_count(k, r)
        work = p.rows(FILL, dwc, b)
        rout = p.rows(FILL, r, b)
        deltas, _ = _updated(k, r, b, tuple(idx))
        d, rv = p.rows(deltas), p.rows(rec)
        leo.set_fanout(fanout)
        try:
            assert leo.leo_encode(b, k, r, wc, full.ptrs, _masked(work.ptrs[:wc], [r - 1])) == inv
            assert f"work_data[{r - 1}]" in leo.last_error(), leo.last_error()
            po, pr = _masked(orig.ptrs, lo), _masked(recv.ptrs, lr)
            assert leo.leo_decode(b, k, r, dwc, po, pr, _masked(work.ptrs, [lo[1]])) == inv
            assert f"work_data[{lo[1]}]" in leo.last_error(), leo.last_error()
            assert leo.leo_amd_repair(b, k, r, dwc, po, pr, _masked(work.ptrs, [lo[1]]), rout.ptrs) == inv
            assert f"work_data[{lo[1]}]" in leo.last_error(), leo.last_error()
            assert leo.leo_amd_update(b, k, r, len(idx), idx, d.ptrs, _masked(rv.ptrs, [3])) == inv
            assert "recovery_data[3]" in leo.last_error(), leo.last_error()
            assert np.all(work.numpy() == FILL) and np.array_equal(rv.numpy(), rec), "a failed call wrote"
        finally:
            leo.set_fanout(0)
        res = leo.leo_amd_repair(b, k, r, dwc, po, pr, work.ptrs, _masked(rout.ptrs, [lr[0]]))  # (no fan-out)
        assert res == leo.LeopardResult.Success, leo.last_error()
        exp_rout = np.full((r, b), FILL, dtype=np.uint8)
        exp_rout[lr[1:]] = rec[lr[1:]]
        assert np.array_equal(rout.numpy(), exp_rout)
        assert np.array_equal(work.numpy()[lo], data[lo])
