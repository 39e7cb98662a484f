"""GPU tier: leo_amd_verify / _slice / _batch against the CPU oracle.  A checked
recovery piece j is expected in the verdict exactly when the piece as passed
differs from oracle.encode(originals as passed, R)[j] (K = 1: the original;
R = 1: the XOR of the originals).  Every call's bitmap starts as all ones (the
wrapper pre-fills it), so stale bits cannot pass; after every call the piece
buffers hold what they held before."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _encode(data, r):
    k = data.shape[0]
    if k == 1:
        return np.repeat(data, r, axis=0)  # leopard.cpp:144-149
    if r == 1:
        return np.bitwise_xor.reduce(data, axis=0, keepdims=True)  # leopard.cpp:152-160
    return ol.oracle().encode(np.ascontiguousarray(data), r)


@functools.lru_cache(maxsize=None)
def _codeword(k, r, b, seed=17):
    """(originals, recovery) of one shape; shared between tests, never modified."""
    rng = np.random.default_rng(seed + 7 * k + r)
    data = rng.integers(0, 256, (k, b), dtype=np.uint8)
    rec = _encode(data, r)
    data.setflags(write=False)
    rec.setflags(write=False)
    return data, rec


def _bits(bitmap, r):
    words = np.asarray(bitmap, dtype=np.uint32).reshape(-1)
    assert words.size == (r + 31) // 32
    got = {j for j in range(32 * words.size) if (int(words[j >> 5]) >> (j & 31)) & 1}
    assert all(j < r for j in got), f"bits past recovery_count are set: {sorted(got)[-4:]}"
    return got


class Stripe:
    """One object on the GPU (or in host memory) with host mirrors of what is
    passed: the expected verdict is computed from the mirrors by the oracle."""

    def __init__(self, k, r, b, host=False, seed=17):
        import torch
        self.k, self.r, self.b, self.host = k, r, b, host
        data, rec = _codeword(k, r, b, seed)
        self.clean_rec = rec
        self.h_orig, self.h_rec = np.array(data), np.array(rec)
        self.expect_rec = rec  # the oracle's encode of the originals as passed
        if host:
            self.orig, self.rec = self.h_orig.copy(), self.h_rec.copy()
        else:
            self.orig = torch.from_numpy(self.h_orig).to("cuda:0")
            self.rec = torch.from_numpy(self.h_rec).to("cuda:0")

    def _addr(self, a, i):
        return a[i].ctypes.data if self.host else a[i].data_ptr()

    def flip(self, which, i, pos, bit=0):
        """Flip one bit of original / recovery piece i, on the device and in the mirror."""
        dst, mirror = (self.orig, self.h_orig) if which == "orig" else (self.rec, self.h_rec)
        mirror[i, pos] ^= np.uint8(1 << bit)
        if self.host:
            dst[i, pos] ^= np.uint8(1 << bit)
        else:
            dst[i, pos] = int(mirror[i, pos])
        if which == "orig":
            self.expect_rec = _encode(self.h_orig, self.r)

    def expected(self, have):
        return {j for j in have if not np.array_equal(self.h_rec[j], self.expect_rec[j])}

    def ptrs(self, have=None):
        have = set(range(self.r)) if have is None else set(have)
        return ([self._addr(self.orig, i) for i in range(self.k)],
                [self._addr(self.rec, j) if j in have else None for j in range(self.r)])

    def unchanged(self):
        if self.host:
            return np.array_equal(self.orig, self.h_orig) and np.array_equal(self.rec, self.h_rec)
        return (np.array_equal(self.orig.cpu().numpy(), self.h_orig) and
                np.array_equal(self.rec.cpu().numpy(), self.h_rec))


def _verify(leo, st, have=None, cols=None, mismatch=True):
    """One call; returns (set of flagged pieces or None, count)."""
    po, pr = st.ptrs(have)
    if cols is None:
        res, count, bm = leo.leo_amd_verify(st.b, st.k, st.r, po, pr, mismatch)
    else:
        res, count, bm = leo.leo_amd_verify_slice(st.b, cols[0], cols[1] - cols[0], st.k, st.r, po, pr, mismatch)
    assert res == leo.LeopardResult.Success, leo.last_error()
    got = None if bm is None else _bits(bm, st.r)
    if got is not None:
        assert count == len(got)
    return got, count


def _positions(b):
    """Byte 0, byte 3, the last byte, and for every strip width of the kernels
    (64-byte lane groups and GF(2^16) blocks, 128-byte narrow strips, 256-byte
    tiles, 512-byte GF(2^16) tiles, 1 KiB bit-sliced tiles) the last byte of the
    first full strip and the first byte of the tail strip."""
    pos = {0, 3, b - 1}
    for s in (64, 128, 256, 512, 1024):
        if b > s:
            pos.add(s - 1)
            pos.add((b - 1) // s * s)
    return sorted(pos)


def _pieces(r):
    """0, R - 1 and one index per bit of the piece number: the tile registers
    (low bits) and the waves (high bits) of every kernel."""
    js = {0, r - 1, r // 2, r // 3}
    bit = 1
    while bit < r:
        js.add(bit)
        js.add(r - 1 - bit)
        bit <<= 1
    return sorted(j for j in js if 0 <= j < r)


SHAPES = [
    # GF(2^8), the general tile
    (7, 3, 64), (3, 2, 64), (33, 9, 64), (40, 20, 64), (250, 6, 64), (100, 10, 65600), (5, 3, 64 * 17), (192, 64, 64),
    # launch_ff8_encode picks lane groups G = 0 at every size in the product build; by piece size it
    # changes the tile: the wide 7-bit tile from 256 KiB pieces
    (128, 120, 256 << 10),
    # dense form; from 512 KiB pieces the single call takes the bit-sliced tile
    (16, 16, 64), (64, 64, 64 * 33), (128, 128, 128), (128, 128, 512 << 10),
    # edge paths
    (1, 1, 64), (5, 1, 192),
    # matrix route
    (100, 10, 2560),
    # GF(2^16): single tile, narrow strips, three passes
    (129, 127, 64), (300, 37, 128), (200, 100, 65536), (300, 100, 61504), (600, 300, 64), (2000, 1000, 128),
    # GF(2^16), the other instantiations of the verify forms.  The single tile at every width m = 2, 4, 8, 16,
    # 32, and m = 128, 256 on pieces past the narrow strips' 256 KiB:
    (300, 2, 64), (300, 3, 64), (300, 5, 64), (300, 9, 64), (300, 17, 64 * 9), (300, 65, (256 << 10) + 64),
    (130, 129, (256 << 10) + 64),
    # narrow strips at m = 256 (one chunk-serial workgroup per strip from 256 strips of 128 bytes on)
    (1000, 200, (32 << 10) + 64),
    # the final pass's 32-piece form (more than 256 workgroups: 129 column tiles x 2 piece tiles)
    (300, 300, 65600),
]


@pytest.mark.parametrize("k,r,b", SHAPES, ids=[f"{k}+{r}x{b}" for k, r, b in SHAPES])
def test_shape(leo, k, r, b):
    st = Stripe(k, r, b)
    every = range(r)
    # 1. a clean codeword
    assert _verify(leo, st) == (set(), 0)
    # 2. one flipped bit in one recovery piece
    positions = _positions(b)
    n = 0
    for j in _pieces(r):
        for pos in (positions if j == 0 else [positions[(n + t) % len(positions)] for t in range(2)]):
            n += 1
            st.flip("rec", j, pos, bit=n % 8)
            assert st.expected(every) == {j}
            assert _verify(leo, st) == ({j}, 1), (j, pos)
            st.flip("rec", j, pos, bit=n % 8)
    assert _verify(leo, st) == (set(), 0)
    # 5. no bitmap: the count alone
    st.flip("rec", r - 1, b - 1)
    assert _verify(leo, st, mismatch=None) == (None, 1)
    st.flip("rec", r - 1, b - 1)
    # 4. every other piece not at hand; garbage in one present and one absent piece
    have = list(range(0, r, 2))
    if r >= 2:
        present, absent = have[-1], 1
        st.flip("rec", present, b // 2)
        st.flip("rec", absent, 0)
        assert st.expected(have) == {present}
        assert _verify(leo, st, have) == ({present}, 1)
        st.flip("rec", present, b // 2)
        st.flip("rec", absent, 0)
        assert _verify(leo, st, have) == (set(), 0)
    # 3. one byte of one original: the oracle's verdict (for these codes, every checked piece)
    st.flip("orig", k // 2, min(b - 1, 70), bit=5)
    exp = st.expected(every)
    assert len(exp) == r
    assert _verify(leo, st) == (exp, r)
    assert _verify(leo, st, have) == (st.expected(have), len(have))
    # 6. verify writes nothing
    assert st.unchanged()


def test_no_piece_to_check(leo):
    st = Stripe(7, 3, 64)
    assert _verify(leo, st, have=[]) == (set(), 0)


def test_torch_helper(leo):
    st = Stripe(33, 9, 64)
    assert leo.verify(st.orig, st.rec) == []
    st.flip("rec", 4, 9)
    st.flip("rec", 7, 63)
    assert leo.verify(st.orig, st.rec) == [4, 7]
    assert leo.verify(st.orig, st.rec, have_recovery=[0, 7]) == [7]


@pytest.mark.parametrize("cols", [(0, 64), (0, 4096), (4096, 4096 + 8192), (32768, 32768 + 64), (65536 - 192, 65600),
                                  (65536, 65600)])
def test_slice(leo, cols):
    k, r, b = 100, 10, 65600
    st = Stripe(k, r, b)
    spots = {0: 0, 1: 63, 2: 64, 3: 4095, 4: 4096, 5: 12287, 6: 32768 + 31, 7: 65536 - 193, 8: 65536, 9: b - 1}
    assert _verify(leo, st, cols=cols) == (set(), 0)
    for j, pos in spots.items():
        st.flip("rec", j, pos, bit=j % 8)
    inside = {j for j, pos in spots.items() if cols[0] <= pos < cols[1]}
    assert _verify(leo, st, cols=cols) == (inside, len(inside))
    assert _verify(leo, st) == (set(spots), r)
    assert st.unchanged()


# ------------------------------------------------------------------ batches --

def shipped_strip() -> int:
    """S of the product build's bit-sliced tile: 256 << LAMD_BS_WB (rs_ff8_bs.hip)."""
    with open(os.path.join(REPO, "leopard_amd", "csrc", "rs_ff8_bs.hip")) as f:
        m = re.search(r"^#define LAMD_BS_WB (\d)", f.read(), re.M)
    assert m, "rs_ff8_bs.hip defines LAMD_BS_WB"
    return 256 << int(m.group(1))


class Batch:
    """count objects of one shape, built from `distinct` oracle codewords.  slab:
    an object's pieces are rows of one tensor; else they are scattered rows."""

    def __init__(self, count, k, r, b, slab=True, distinct=3):
        import torch
        self.count, self.k, self.r, self.b = count, k, r, b
        words = [_codeword(k, r, b, seed=100 + d) for d in range(min(distinct, count))]
        h_orig = np.stack([words[o % len(words)][0] for o in range(count)])
        self.h_clean = np.stack([words[o % len(words)][1] for o in range(count)])
        self.h_rec = self.h_clean.copy()
        if slab:
            self.orig = torch.from_numpy(h_orig).to("cuda:0")
            self.rec = torch.from_numpy(self.h_rec).to("cuda:0")
            self.row_o = lambda o, i: self.orig[o, i]
            self.row_r = lambda o, j: self.rec[o, j]
        else:  # piece rows in a shuffled order inside one pool: no equal spacing
            rng = np.random.default_rng(count * 1000 + k)
            perm = rng.permutation(count * (k + r))
            pool = torch.empty((count * (k + r), b), dtype=torch.uint8, device="cuda:0")
            flat = np.concatenate([np.concatenate([h_orig[o], self.h_rec[o]]) for o in range(count)])
            pool[torch.from_numpy(perm).to("cuda:0")] = torch.from_numpy(flat).to("cuda:0")
            self.pool = pool
            self.row_o = lambda o, i: pool[int(perm[o * (k + r) + i])]
            self.row_r = lambda o, j: pool[int(perm[o * (k + r) + k + j])]
        self.snapshot = None

    def flip(self, o, j, pos, bit=0):
        self.h_rec[o, j, pos] ^= np.uint8(1 << bit)
        self.row_r(o, j)[pos] = int(self.h_rec[o, j, pos])

    def expected(self, o, have=None):
        have = range(self.r) if have is None else have
        return {j for j in have if not np.array_equal(self.h_rec[o, j], self.h_clean[o, j])}

    def run(self, leo, have=None):
        """have: per-object lists of checked pieces (default: all).  Returns [set per object]."""
        import torch
        po = [[self.row_o(o, i).data_ptr() for i in range(self.k)] for o in range(self.count)]
        pr = [[self.row_r(o, j).data_ptr() if have is None or j in have[o] else None for j in range(self.r)]
              for o in range(self.count)]
        before = [t.clone() for t in self.tensors()]
        res, counts, bm = leo.leo_amd_verify_batch(self.b, self.k, self.r, po, pr)
        assert res == leo.LeopardResult.Success, leo.last_error()
        got = [_bits(bm[o], self.r) for o in range(self.count)]
        assert counts == [len(g) for g in got]
        for t, t0 in zip(self.tensors(), before):
            assert torch.equal(t, t0), "verify changed a piece"
        return got

    def tensors(self):
        return [self.pool] if hasattr(self, "pool") else [self.orig, self.rec]


def _bs_batch(leo, count, b, clean=(), last_strip=False):
    """Object o has recovery piece o % 128 corrupted at a pseudo-random column."""
    bt = Batch(count, 128, 128, b)
    rng = np.random.default_rng(b + count)
    for o in range(count):
        if o in clean:
            continue
        pos = int(rng.integers(b - 64, b)) if last_strip else int(rng.integers(0, b))
        bt.flip(o, o % 128, pos, bit=o % 8)
    got = bt.run(leo)
    for o in range(count):
        assert got[o] == (set() if o in clean else {o % 128}), (o, sorted(got[o])[:8])
    return got


@pytest.mark.parametrize("which", range(3))
def test_batch_bit_sliced_128_objects(leo, which):
    """128 slab-laid 128+128 objects (two launches of 64), pieces of S - 64, S, 2 S + 192 bytes."""
    s = shipped_strip()
    _bs_batch(leo, 128, [s - 64, s, 2 * s + 192][which], clean=(5, 77))


def test_batch_bit_sliced_queue_first_round(leo):
    _bs_batch(leo, 9, shipped_strip(), clean=(4,))


def test_batch_bit_sliced_queue_rounds(leo):
    """Pieces of 8 KiB + 64 and enough objects for a second round of the tile
    queue (test_gpu_bs_waves.py: run_queue_rounds); corruption in the last 64 bytes."""
    import torch
    s = shipped_strip()
    b = 8192 + 64
    strips = -(-b // s)
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    count = min(64, -(-(waves // (s // 256) + 64) // strips))
    _bs_batch(leo, count, b, clean=(0, count - 1), last_strip=True)


@pytest.mark.parametrize("k,r,b,count", [(100, 10, 2560, 6), (7, 3, 64, 5)])
def test_batch_pointer_tables(leo, k, r, b, count):
    """Objects whose pieces are not equally spaced; clean and corrupt objects mixed,
    some pieces not at hand."""
    bt = Batch(count, k, r, b, slab=False)
    bt.flip(1, 0, 0)
    bt.flip(1, r - 1, b - 1, bit=7)
    bt.flip(3, r // 2, b // 2, bit=3)
    bt.flip(count - 1, 1, 63)
    got = bt.run(leo)
    assert got == [bt.expected(o) for o in range(count)]
    assert got[0] == set() and got[1] == {0, r - 1} and got[count - 1] == {1}
    have = [list(range(r))] * count
    have[1] = [0]            # piece r - 1 of object 1 is not at hand
    have[3] = []             # nothing of object 3 is checked
    got = bt.run(leo, have)
    assert got == [bt.expected(o, have[o]) for o in range(count)]
    assert got[1] == {0} and got[3] == set()


@pytest.mark.parametrize("k,r,count", [(200, 100, 8), (300, 200, 4)])  # m = 128, 256: the two narrow batch tiles
def test_batch_gf16(leo, k, r, count):
    b = 2560
    bt = Batch(count, k, r, b)
    bt.flip(0, r - 1, 2559, bit=7)
    bt.flip(2, 0, 0)
    bt.flip(2, 31, 128)
    bt.flip(2, 32, 2432)
    bt.flip(count - 1, 64, 1000)
    got = bt.run(leo)
    assert got == [bt.expected(o) for o in range(count)]
    assert got[2] == {0, 31, 32} and got[1] == set() and got[0] == {r - 1}
    have = [list(range(r))] * count
    have[2] = [31, 33]       # pieces 0 and 32 of object 2 are not at hand
    got = bt.run(leo, have)
    assert got == [bt.expected(o, have[o]) for o in range(count)]
    assert got[2] == {31}


def test_too_much_data(leo):
    """Step 5 of the validation order: initialised, every array and original given, n > 65536."""
    import torch
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    k = r = 40000  # next_pow2(next_pow2(r) + k) = 131072
    res, count, bm = leo.leo_amd_verify(64, k, r, [buf.data_ptr()] * k, [buf.data_ptr()] * r, True)
    assert res == leo.LeopardResult.TooMuchData


# -------------------------------------------------------------- host memory --

@pytest.mark.parametrize("k,r,b", [(128, 128, 1024), (1000, 200, 256)])
def test_host_memory_pageable(leo, k, r, b):
    st = Stripe(k, r, b, host=True)
    assert _verify(leo, st) == (set(), 0)
    st.flip("rec", r - 2, b - 1, bit=6)
    assert _verify(leo, st) == ({r - 2}, 1)
    assert _verify(leo, st, have=[0, 1]) == (set(), 0)
    assert st.unchanged()


def test_host_memory_registered(leo):
    st = Stripe(3, 2, 64, host=True)
    regs = [st.orig, st.rec]
    for a in regs:
        assert leo.register_host(a.ctypes.data, a.nbytes) == leo.LeopardResult.Success, leo.last_error()
    try:
        assert _verify(leo, st) == (set(), 0)
        st.flip("rec", 1, 17)
        assert _verify(leo, st) == ({1}, 1)
    finally:
        for a in regs:
            assert leo.unregister_host(a.ctypes.data) == leo.LeopardResult.Success
    assert st.unchanged()


@pytest.mark.parametrize("k,r,b", [(128, 128, 320), (100, 10, 65600), (1000, 200, 128)])
def test_async_on_a_stream(leo, k, r, b):
    """The reports are host memory: valid on return, async mode or not."""
    import torch
    st = Stripe(k, r, b)
    st.flip("rec", r - 1, b - 1)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    try:
        leo.set_stream(stream.cuda_stream)
        leo.set_async(True)
        assert _verify(leo, st) == ({r - 1}, 1)  # read before any synchronisation by the caller
    finally:
        leo.set_async(False)
        leo.set_stream(None)
        stream.synchronize()
        leo.release_stream(stream.cuda_stream)


# ------------------------------------------------------------ forced routes --

_REDUCED = [(7, 3, 64), (40, 20, 64), (100, 10, 65600), (128, 128, 128), (100, 10, 2560), (300, 37, 128),
            (300, 100, 61504), (600, 300, 64)]


def reduced_verdicts(leo):
    """One shape per kernel family and the bit-sliced batch at S: the verdicts as text."""
    out = []
    for k, r, b in _REDUCED:
        st = Stripe(k, r, b)
        out.append((k, r, b, "clean", sorted(_verify(leo, st)[0])))
        st.flip("rec", r - 1, b - 1, bit=7)
        st.flip("rec", 0, 3)
        out.append((k, r, b, "rec", sorted(_verify(leo, st)[0])))
        st.flip("orig", 1, 0)
        out.append((k, r, b, "orig", sorted(_verify(leo, st, have=range(0, r, 2))[0])))
    got = _bs_batch(leo, 66, shipped_strip(), clean=(5, 65))
    out.append(("batch", [sorted(g) for g in got]))
    return repr(out)


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import leopard_amd as leo
import test_gpu_verify as t
assert leo.leo_init() == leo.LeopardResult.Success, leo.last_error()
print("verdicts", t.reduced_verdicts(leo))
print("child ok")
"""


def _child(env):
    code = _CHILD.format(repo=REPO, tests=HERE)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=170)
    assert p.returncode == 0 and "child ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    return [line.split(" ", 1)[1] for line in p.stdout.splitlines() if line.startswith("verdicts ")]


def test_forced_composition_gives_the_same_verdicts(leo):
    assert _child(dict(os.environ, LEO_AMD_VERIFY_COMPOSE="1")) == [reduced_verdicts(leo)]


def test_forced_fused_gives_the_same_verdicts(leo):
    """The experiment build keeps every call that has a fused route on it."""
    lib = os.path.join(REPO, "leopard_amd", "lib", "exp", "libleopard_amd.so")
    assert os.path.exists(lib), "make -C leopard_amd builds lib/exp"
    env = dict(os.environ, LEOPARD_AMD_LIB=lib, LEO_AMD_VERIFY_COMPOSE="0")
    assert _child(env) == [reduced_verdicts(leo)]
