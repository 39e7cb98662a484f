"""GPU tier: leo_amd_update (in-place recovery update from original-piece
deltas), bit-exact against the CPU oracle.  Start state: oracle.encode(D, R)
uploaded; expectation: oracle.encode(D', R) with D' = D with the deltas XORed
in.  Every case also checks that the delta buffers are unchanged."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _start(k, r, b, seed):
    """(originals, their recovery) of one shape; shared between tests, never modified."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (k, b), dtype=np.uint8)
    rec = ol.oracle().encode(data, r)
    data.setflags(write=False)
    rec.setflags(write=False)
    return data, rec


def _deltas(seed, count, b):
    return np.random.default_rng(seed).integers(0, 256, (count, b), dtype=np.uint8)


def _apply(data, indices, deltas):
    new = data.copy()
    for t, i in enumerate(indices):
        new[i] ^= deltas[t]
    return new


def _expect(data, r, indices, deltas):
    new = _apply(data, indices, deltas)
    return new, ol.oracle().encode(new, r)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")  # a writable copy (the shared start states are read-only)


def _update_checked(leo, rec_dev, k, indices, deltas):
    """leo.update on the device with `deltas` (numpy) uploaded; checks the delta buffers afterwards."""
    import torch
    dd = _dev(deltas)
    out = leo.update(rec_dev, k, indices, dd)
    torch.cuda.synchronize()
    assert out is rec_dev
    assert np.array_equal(dd.cpu().numpy(), deltas), "delta buffers changed"
    return out


PARITY = [
    # GF(2^8)
    (2, 2, 64, [1]),
    (7, 5, 128, [0, 6]),
    (100, 10, 64 * 17, [3]),            # column tail that is not a whole strip
    (128, 128, 64, [0, 127]),
    (250, 6, 64, [249]),
    (64, 64, 64 * 33, list(range(32))),  # 32 changed, the maximum
    (128, 128, 65536, [5]),
    # GF(2^16)
    (129, 127, 64, [128]),
    (300, 300, 128, [299]),
    (1000, 200, 64 * 5, [0, 512, 999]),
    (1000, 200, 61504, [17]),
    (700, 256, 128, list(range(100, 132))),  # 32 changed
    (5000, 3000, 64, [0, 4999]),             # multi-pass encoder generating the coefficients
    # edge paths (K == 1, R == 1)
    (1, 1, 64, [0]),
    (7, 1, 128, [2, 5]),
    (1000, 1, 64, [999]),
]


@pytest.mark.parametrize("k,r,b,indices", PARITY, ids=[f"{k}+{r}x{b}c{len(i)}" for k, r, b, i in PARITY])
def test_parity(leo, k, r, b, indices):
    data, rec = _start(k, r, b, 11)
    deltas = _deltas(k * 31 + r, len(indices), b)
    _, expect = _expect(data, r, indices, deltas)
    got = _update_checked(leo, _dev(rec), k, indices, deltas)
    assert np.array_equal(got.cpu().numpy(), expect)


def test_cache_reuse_and_overlap(leo):
    k, r, b = 1000, 200, 128
    data, rec = _start(k, r, b, 12)
    rec_dev = _dev(rec)
    cur = data
    steps = [(k, r, [3, 700, 41]), (k, r, [3, 700, 41]), (k, r, [41, 5, 999, 3])]
    for n, (_, _, idx) in enumerate(steps):
        deltas = _deltas(100 + n, len(idx), b)
        cur, expect = _expect(cur, r, idx, deltas)
        _update_checked(leo, rec_dev, k, idx, deltas)
        assert np.array_equal(rec_dev.cpu().numpy(), expect), f"step {n}"
    # a different (K, R) with the same indices must not hit the first shape's columns
    k2, r2 = 900, 200
    data2, rec2 = _start(k2, r2, b, 13)
    d2 = _deltas(200, 3, b)
    _, expect2 = _expect(data2, r2, [3, 700, 41], d2)
    got2 = _update_checked(leo, _dev(rec2), k2, [3, 700, 41], d2)
    assert np.array_equal(got2.cpu().numpy(), expect2)
    # the first shape again
    deltas = _deltas(300, 3, b)
    cur, expect = _expect(cur, r, [3, 700, 41], deltas)
    _update_checked(leo, rec_dev, k, [3, 700, 41], deltas)
    assert np.array_equal(rec_dev.cpu().numpy(), expect)


@pytest.mark.parametrize("k,r,b,indices", [(100, 10, 192, [7, 99]), (1000, 200, 192, [0, 640])])
def test_same_delta_twice_restores(leo, k, r, b, indices):
    _, rec = _start(k, r, b, 14)
    rec_dev = _dev(rec)
    deltas = _deltas(5, len(indices), b)
    _update_checked(leo, rec_dev, k, indices, deltas)
    assert not np.array_equal(rec_dev.cpu().numpy(), rec)
    _update_checked(leo, rec_dev, k, indices, deltas)
    assert np.array_equal(rec_dev.cpu().numpy(), rec)


_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import leopard_amd as leo, oracle_lib as ol
assert leo.leo_init() == leo.LeopardResult.Success, leo.last_error()
k, r, b = 1000, 200, 256
rng = np.random.default_rng(21)
cur = rng.integers(0, 256, (k, b), dtype=np.uint8)
rec = torch.from_numpy(ol.oracle().encode(cur, r)).to("cuda:0")
calls = [list(range(0, 8)), list(range(500, 508)), list(range(992, 1000)), list(range(0, 8))]
for n, idx in enumerate(calls):
    d = rng.integers(0, 256, (8, b), dtype=np.uint8)
    dd = torch.from_numpy(d).to("cuda:0")
    leo.update(rec, k, idx, dd)
    torch.cuda.synchronize()
    for t, i in enumerate(idx):
        cur[i] ^= d[t]
    assert np.array_equal(dd.cpu().numpy(), d), "delta buffers changed"
    assert np.array_equal(rec.cpu().numpy(), ol.oracle().encode(cur, r)), "call %d differs" % n
print("child ok")
"""


@pytest.mark.parametrize("cache_kb", ["1", "0"])
def test_cache_bound(cache_kb):
    """A cache too small for one column (1 KiB) and no cache at all: every call
    builds its columns in scratch of its own and still succeeds."""
    env = dict(os.environ, LEO_AMD_UPDATE_CACHE_KB=cache_kb)
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("k,r,b", [(120, 12, 256), (1000, 200, 128)])
def test_accumulation(leo, k, r, b):
    data, rec = _start(k, r, b, 15)
    rec_dev = _dev(rec)
    cur = data
    for n, idx in enumerate([[0, 1, 2], [k - 1, 50], [60, 61, 62, 63, 64, 65, 66, 67, 68]]):
        deltas = _deltas(40 + n, len(idx), b)
        cur = _apply(cur, idx, deltas)
        _update_checked(leo, rec_dev, k, idx, deltas)
    assert np.array_equal(rec_dev.cpu().numpy(), ol.oracle().encode(cur, r))


@pytest.mark.parametrize("k,r,b", [(100, 20, 128), (1000, 200, 64)])
def test_decode_after_update(leo, k, r, b):
    import torch
    data, rec = _start(k, r, b, 16)
    indices = [4, k - 2]
    deltas = _deltas(6, 2, b)
    new = _apply(data, indices, deltas)
    rec_dev = _update_checked(leo, _dev(rec), k, indices, deltas)
    lost = sorted({4} | set(np.random.default_rng(7).choice(np.arange(5, k), r - 1, replace=False).tolist()))
    assert len(lost) == r
    got = leo.decode(_dev(new), rec_dev, lost, [])
    torch.cuda.synchronize()
    for i in lost:
        assert np.array_equal(got[i].cpu().numpy(), new[i]), f"lost original {i}"


@pytest.mark.parametrize("k,r,b,indices,register", [(128, 128, 1024, [3], False), (1000, 200, 256, [0, 999], False),
                                                    (1000, 200, 256, [0, 999], True)])
def test_host_memory(leo, k, r, b, indices, register):
    data, rec = _start(k, r, b, 17)
    deltas = _deltas(8, len(indices), b)
    keep = deltas.copy()
    _, expect = _expect(data, r, indices, deltas)
    host = rec.copy()  # pageable numpy memory, updated in place
    regs = [host, deltas] if register else []
    for a in regs:
        assert leo.register_host(a.ctypes.data, a.nbytes) == leo.LeopardResult.Success, leo.last_error()
    try:
        res = leo.leo_amd_update(b, k, r, len(indices), indices, [deltas[t].ctypes.data for t in range(len(indices))],
                                 [host[j].ctypes.data for j in range(r)])
        assert res == leo.LeopardResult.Success, leo.last_error()
    finally:
        for a in regs:
            assert leo.unregister_host(a.ctypes.data) == leo.LeopardResult.Success
    assert np.array_equal(deltas, keep), "delta buffers changed"
    assert np.array_equal(host, expect)


@pytest.mark.parametrize("k,r", [(100, 10), (1000, 200)])
def test_slice(leo, k, r):
    import torch
    b = 192
    data, rec = _start(k, r, b, 18)
    indices = [1, k - 1]
    deltas = _deltas(9, 2, b)
    _, expect = _expect(data, r, indices, deltas)
    dd = _dev(deltas)
    rec_dev = _dev(rec)
    dp = [dd[t].data_ptr() for t in range(2)]
    rp = [rec_dev[j].data_ptr() for j in range(r)]
    # 192-byte pieces in two "halves" of whole 64-byte blocks
    assert leo.leo_amd_update_slice(b, 0, 64, k, r, 2, indices, dp, rp) == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    half = rec_dev.cpu().numpy()
    assert np.array_equal(half[:, :64], expect[:, :64])
    assert np.array_equal(half[:, 64:], rec[:, 64:]), "bytes outside the slice were touched"
    assert leo.leo_amd_update_slice(b, 64, 128, k, r, 2, indices, dp, rp) == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(rec_dev.cpu().numpy(), expect)
    whole = _update_checked(leo, _dev(rec), k, indices, deltas)
    assert torch.equal(whole, rec_dev)
    assert np.array_equal(dd.cpu().numpy(), deltas), "delta buffers changed"


@pytest.mark.parametrize("k,r,b", [(100, 10, 320), (1000, 200, 128)])
def test_scattered_pointers_on_a_stream(leo, k, r, b):
    import torch
    data, rec = _start(k, r, b, 19)
    indices = [2, 77]
    deltas = _deltas(10, 2, b)
    _, expect = _expect(data, r, indices, deltas)
    pieces = [_dev(rec[j]) for j in range(r)]  # separately allocated recovery pieces
    pad = [torch.empty(64 * (1 + j % 3), dtype=torch.uint8, device="cuda:0") for j in range(4)]  # break any regular spacing
    dd = [_dev(deltas[t]) for t in range(2)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    try:
        leo.set_stream(stream.cuda_stream)
        leo.set_async(True)
        res = leo.leo_amd_update(b, k, r, 2, indices, [d.data_ptr() for d in dd], [p.data_ptr() for p in pieces])
        assert res == leo.LeopardResult.Success, leo.last_error()
        stream.synchronize()
    finally:
        leo.set_async(False)
        leo.set_stream(None)
        leo.release_stream(stream.cuda_stream)
    del pad
    for j in range(r):
        assert np.array_equal(pieces[j].cpu().numpy(), expect[j]), f"recovery piece {j}"
    for t in range(2):
        assert np.array_equal(dd[t].cpu().numpy(), deltas[t]), "delta buffers changed"
