"""GPU tier: leo_amd_repair (lost originals and lost recovery pieces rebuilt in
the decode pass), bit-exact against the CPU oracle: oracle.encode(data, R) for
recovery pieces, the data itself for originals.  Every input is a codeword.
Every case also checks that each received piece, each recovery_out buffer that
was not requested (or belongs to a received piece) and each work buffer of a
received original still holds what it held before the call."""
import functools
import hashlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A   # sentinel of every output buffer
JUNK = 0xEE   # what the buffers of lost pieces hold (never passed to the library)


@functools.lru_cache(maxsize=None)
def _codeword(k, r, b, seed=31):
    """(originals, recovery) of one shape; shared between tests, never modified."""
    rng = np.random.default_rng(seed + 7 * k + r)
    data = rng.integers(0, 256, (k, b), dtype=np.uint8)
    if k == 1:
        rec = np.repeat(data, r, axis=0)  # leopard.cpp:144-149
    elif r == 1:
        rec = np.bitwise_xor.reduce(data, axis=0, keepdims=True)  # leopard.cpp:152-160
    else:
        rec = ol.oracle().encode(data, r)
    data.setflags(write=False)
    rec.setflags(write=False)
    return data, rec


def _pattern(k, r, nlo, nlr, seed=5):
    rng = np.random.default_rng(seed + 13 * k + r + 101 * nlo + nlr)
    lo = sorted(rng.choice(k, nlo, replace=False).tolist()) if nlo < k else list(range(k))
    lr = sorted(rng.choice(r, nlr, replace=False).tolist()) if nlr < r else list(range(r))
    return lo, lr


def _setup(leo, k, r, b, lo, lr, want=None, host=False, seed=31):
    """Buffers of one object: the received pieces (lost rows hold JUNK and are not
    passed), sentinel-filled work [K, B] and recovery_out [R, B].  Every work row
    is passed; recovery_out rows are passed for the requested pieces and for the
    received ones (which the call must ignore)."""
    import torch
    data, rec = _codeword(k, r, b, seed)
    want = list(lr) if want is None else list(want)
    o = types.SimpleNamespace(k=k, r=r, b=b, lo=lo, lr=lr, want=want, data=data, rec=rec, host=host)
    o.h_orig, o.h_rec = np.array(data), np.array(rec)
    o.h_orig[lo] = JUNK
    o.h_rec[lr] = JUNK
    work = np.full((k, b), FILL, dtype=np.uint8)
    rout = np.full((r, b), FILL, dtype=np.uint8)
    if host:
        o.orig, o.recv, o.work, o.rout = o.h_orig.copy(), o.h_rec.copy(), work, rout
        addr = lambda a, i: a[i].ctypes.data  # noqa: E731
    else:
        o.orig, o.recv, o.work, o.rout = (torch.from_numpy(a).to("cuda:0") for a in (o.h_orig, o.h_rec, work, rout))
        addr = lambda a, i: a[i].data_ptr()  # noqa: E731
    los, lrs, ws = set(lo), set(lr), set(want)
    o.wc = leo.leo_decode_work_count(k, r)
    o.p_orig = [None if i in los else addr(o.orig, i) for i in range(k)]
    o.p_rec = [None if j in lrs else addr(o.recv, j) for j in range(r)]
    o.p_work = [addr(o.work, i) for i in range(k)] + [None] * (o.wc - k)
    o.p_rout = [None if (j in lrs and j not in ws) else addr(o.rout, j) for j in range(r)]
    return o


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _check(o, cols=None):
    """Outputs equal the codeword over columns `cols` (default: all) and hold the
    sentinel everywhere else; nothing else changed."""
    work, rout = _np(o.work), _np(o.rout)
    lo_c, hi_c = (0, o.b) if cols is None else cols
    exp_work = np.full((o.k, o.b), FILL, dtype=np.uint8)
    exp_work[o.lo, lo_c:hi_c] = o.data[o.lo, lo_c:hi_c]
    exp_rout = np.full((o.r, o.b), FILL, dtype=np.uint8)
    exp_rout[o.want, lo_c:hi_c] = o.rec[o.want, lo_c:hi_c]
    bad = np.flatnonzero((work != exp_work).any(axis=1))
    assert bad.size == 0, f"work rows {bad[:8].tolist()} (lost originals {o.lo[:8]}...)"
    bad = np.flatnonzero((rout != exp_rout).any(axis=1))
    assert bad.size == 0, f"recovery_out rows {bad[:8].tolist()} (requested {o.want[:8]}...)"
    assert np.array_equal(_np(o.orig), o.h_orig), "an original's buffer changed"
    assert np.array_equal(_np(o.recv), o.h_rec), "a recovery piece's buffer changed"


def _repair(leo, o):
    import torch
    res = leo.leo_amd_repair(o.b, o.k, o.r, o.wc, o.p_orig, o.p_rec, o.p_work, o.p_rout)
    torch.cuda.synchronize()
    return res


def _run(leo, k, r, b, nlo, nlr, want=None, host=False):
    lo, lr = _pattern(k, r, nlo, nlr)
    o = _setup(leo, k, r, b, lo, lr, want, host)
    assert _repair(leo, o) == leo.LeopardResult.Success, leo.last_error()
    _check(o)
    return o


CASES = [
    # GF(2^8), the general tile (n != 2m)
    (7, 3, 64, 1, 2), (7, 3, 64, 0, 3), (7, 3, 64, 3, 0),
    (100, 10, 2560, 4, 6),    # matrix path
    (100, 10, 65600, 4, 6),   # tile path, column tail
    (192, 64, 64, 30, 34),    # Tn = 8
    # GF(2^8), n = 2m (the split and half decoders cannot serve)
    (2, 2, 64, 1, 1),
    (6, 5, 128, 2, 3),
    (128, 128, 64, 57, 71), (128, 128, 64, 1, 127), (128, 128, 64, 0, 128), (128, 128, 64, 0, 1),
    (128, 128, 320, 57, 71), (128, 128, 320, 1, 127), (128, 128, 320, 0, 128), (128, 128, 320, 0, 1),
    (128, 128, 65536, 32, 32),
    # GF(2^16), the three-pass decoder
    (129, 100, 64, 98, 2),    # Tn = 9
    (300, 300, 128, 246, 54), (300, 300, 128, 300, 0), (300, 300, 128, 0, 17),  # n = 2m
    (1000, 200, 64, 64, 136), (1000, 200, 2560, 64, 136),  # narrow columns
    (1000, 200, 61504, 100, 100),
    (129, 100, 65536, 98, 2), (300, 300, 65536, 246, 54),  # wide columns at Tn = 9, 10: the three passes by default
    (5000, 3000, 64, 1000, 2000),
    (20000, 9000, 64, 1, 8999),   # n = 65536
    (32768, 32768, 64, 20000, 12768),
    # edge paths
    (1, 1, 64, 0, 1), (1, 1, 64, 1, 0),
    (7, 1, 128, 0, 1), (7, 1, 128, 1, 0),
    (3000, 1, 64, 0, 1),
]


@pytest.mark.parametrize("k,r,b,nlo,nlr", CASES, ids=[f"{k}+{r}x{b}-{a}o{c}r" for k, r, b, a, c in CASES])
def test_parity(leo, k, r, b, nlo, nlr):
    _run(leo, k, r, b, nlo, nlr)


def test_nothing_requested_equals_leo_decode(leo):
    """128+128 x 64, every original lost, no recovery piece lost: the decoder's own route."""
    import torch
    k = r = 128
    o = _run(leo, k, r, 64, 128, 0)
    got = leo.decode(o.orig, o.recv, o.lo, [])
    torch.cuda.synchronize()
    for i in o.lo:
        assert torch.equal(got[i], o.work[i]), f"original {i}"


def test_partial_request(leo):
    """40 recovery pieces lost, 5 requested: the other 35 recovery_out entries are NULL."""
    k = r = 128
    lo, lr = _pattern(k, r, 20, 40)
    want = lr[3::8]
    assert len(want) == 5
    o = _setup(leo, k, r, 320, lo, lr, want)
    assert sum(p is None for p in o.p_rout) == 35
    assert _repair(leo, o) == leo.LeopardResult.Success, leo.last_error()
    _check(o)


@pytest.mark.parametrize("k,r,b", [(100, 10, 128), (1000, 200, 64)])
def test_results_after_the_init_check(leo, k, r, b):
    # lost originals + lost recovery = R + 1
    lo, lr = _pattern(k, r, r // 2, r - r // 2 + 1)
    o = _setup(leo, k, r, b, lo, lr)
    assert _repair(leo, o) == leo.LeopardResult.NeedMoreData
    _check(types.SimpleNamespace(**{**vars(o), "lo": [], "want": []}))
    # ... = R is enough; a wrong work_count is InvalidCounts
    lo, lr = _pattern(k, r, r // 2, r - r // 2)
    o = _setup(leo, k, r, b, lo, lr)
    res = leo.leo_amd_repair(b, k, r, o.wc // 2, o.p_orig, o.p_rec, o.p_work, o.p_rout)
    assert res == leo.LeopardResult.InvalidCounts
    # a lost original without a work buffer
    p_work = list(o.p_work)
    p_work[lo[-1]] = None
    assert leo.leo_amd_repair(b, k, r, o.wc, o.p_orig, o.p_rec, p_work, o.p_rout) == leo.LeopardResult.InvalidInput
    assert f"work_data[{lo[-1]}]" in leo.last_error()
    # work buffers of received originals may be NULL
    import torch
    torch.cuda.synchronize()
    _check(types.SimpleNamespace(**{**vars(o), "lo": [], "want": []}))
    los = set(lo)
    p_work = [p if i in los else None for i, p in enumerate(o.p_work)]
    assert leo.leo_amd_repair(b, k, r, o.wc, o.p_orig, o.p_rec, p_work, o.p_rout) == leo.LeopardResult.Success
    torch.cuda.synchronize()
    _check(o)


def test_nothing_to_do_touches_nothing(leo):
    k, r, b = 100, 10, 128
    for lo, lr, want in (([], [], None), ([], [2, 7], [])):
        o = _setup(leo, k, r, b, lo, lr, want)
        assert _repair(leo, o) == leo.LeopardResult.Success
        _check(o)


@pytest.mark.parametrize("k,r,nlo,nlr", [(100, 10, 4, 6), (1000, 200, 64, 136)])
def test_slice(leo, k, r, nlo, nlr):
    import torch
    b = 256
    lo, lr = _pattern(k, r, nlo, nlr)
    o = _setup(leo, k, r, b, lo, lr)
    res = leo.leo_amd_repair_slice(b, 64, 128, k, r, o.wc, o.p_orig, o.p_rec, o.p_work, o.p_rout)
    assert res == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    _check(o, cols=(64, 192))  # bytes outside the slice keep their sentinel


def _batch(leo, objs):
    import torch
    o0 = objs[0]
    res = leo.leo_amd_repair_batch(o0.b, o0.k, o0.r, o0.wc, [o.p_orig for o in objs], [o.p_rec for o in objs],
                                   [o.p_work for o in objs], [o.p_rout for o in objs])
    torch.cuda.synchronize()
    assert res == leo.LeopardResult.Success, leo.last_error()
    for o in objs:
        _check(o)


def _same_as_single(leo, objs):
    """Every object of the batch equals its single-call result."""
    for o in objs:
        s = _setup(leo, o.k, o.r, o.b, o.lo, o.lr, o.want, seed=o.seed)
        assert _repair(leo, s) == leo.LeopardResult.Success, leo.last_error()
        assert np.array_equal(_np(s.work), _np(o.work)) and np.array_equal(_np(s.rout), _np(o.rout))


def _objects(leo, k, r, b, specs):
    objs = []
    for n, (nlo, nlr, nwant) in enumerate(specs):
        lo, lr = _pattern(k, r, nlo, nlr, seed=40 + n)
        o = _setup(leo, k, r, b, lo, lr, lr[:nwant] if nwant is not None else None, seed=60 + n)
        o.seed = 60 + n
        objs.append(o)
    return objs


def test_batch_gf8(leo):
    objs = _objects(leo, 128, 128, 320, [(57, 71, None), (1, 127, 9), (0, 128, None), (100, 0, None)])
    _batch(leo, objs)
    _same_as_single(leo, objs)


def test_batch_gf8_general_tile(leo):
    """n != 2m: the batch stays on the general decoder tile, one launch."""
    objs = _objects(leo, 100, 10, 320, [(4, 6, None), (1, 9, 2), (9, 1, None), (3, 3, 3), (10, 0, None)])
    _batch(leo, objs)
    _same_as_single(leo, objs)


def test_batch_gf8_small_objects(leo):
    """Few strips: the n = 2m batch stays on the general tile as well."""
    objs = _objects(leo, 6, 5, 128, [(2, 3, None), (1, 4, 2), (5, 0, None)])
    _batch(leo, objs)
    _same_as_single(leo, objs)


def test_batch_gf16(leo):
    objs = _objects(leo, 1000, 200, 128, [(64, 136, None), (0, 17, 3), (200, 0, None)])
    _batch(leo, objs)
    _same_as_single(leo, objs)


@pytest.mark.parametrize("k,r,b", [(128, 128, 320), (1000, 200, 128)])
def test_batch_with_an_object_that_lost_nothing(leo, k, r, b):
    objs = _objects(leo, k, r, b, [(3, 5, None), (0, 0, None), (0, 4, 0), (2, 2, 1)])
    _batch(leo, objs)
    _same_as_single(leo, objs)


@pytest.mark.parametrize("k,r,b,nlo,nlr", [(100, 10, 2560, 4, 6), (1000, 200, 128, 64, 136)])
@pytest.mark.parametrize("register", [False, True])
def test_host_memory(leo, k, r, b, nlo, nlr, register):
    lo, lr = _pattern(k, r, nlo, nlr)
    o = _setup(leo, k, r, b, lo, lr, host=True)
    regs = [o.orig, o.recv, o.work, o.rout] if register else []
    for a in regs:
        assert leo.register_host(a.ctypes.data, a.nbytes) == leo.LeopardResult.Success, leo.last_error()
    try:
        res = leo.leo_amd_repair(b, k, r, o.wc, o.p_orig, o.p_rec, o.p_work, o.p_rout)
        assert res == leo.LeopardResult.Success, leo.last_error()
    finally:
        for a in regs:
            assert leo.unregister_host(a.ctypes.data) == leo.LeopardResult.Success
    _check(o)


@pytest.mark.parametrize("k,r,b,nlo,nlr", [(128, 128, 320, 57, 71), (1000, 200, 128, 64, 136),
                                            (1000, 200, 65536, 64, 136)])
def test_async_on_a_stream(leo, k, r, b, nlo, nlr):
    import torch
    lo, lr = _pattern(k, r, nlo, nlr)
    o = _setup(leo, k, r, b, lo, lr)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    try:
        leo.set_stream(stream.cuda_stream)
        leo.set_async(True)
        res = leo.leo_amd_repair(b, k, r, o.wc, o.p_orig, o.p_rec, o.p_work, o.p_rout)
        assert res == leo.LeopardResult.Success, leo.last_error()
        stream.synchronize()
    finally:
        leo.set_async(False)
        leo.set_stream(None)
        leo.release_stream(stream.cuda_stream)
    _check(o)


@pytest.mark.parametrize("k,r,b,nlo,nlr", [(100, 10, 2560, 4, 6), (100, 10, 65600, 4, 6), (128, 128, 320, 57, 71),
                                            (1000, 200, 128, 64, 136), (300, 300, 128, 246, 54),
                                            (1000, 200, 65536, 64, 136)])
def test_decode_repair_decode(leo, k, r, b, nlo, nlr):
    """One erasure pattern on one thread: the cached locator, pyramid and matrix
    state of leo_decode and of repair are keyed apart."""
    import torch
    lo, lr = _pattern(k, r, nlo, nlr)
    o = _setup(leo, k, r, b, lo, lr)
    first = {i: t.clone() for i, t in leo.decode(o.orig, o.recv, lo, lr).items()}
    torch.cuda.synchronize()
    assert _repair(leo, o) == leo.LeopardResult.Success, leo.last_error()
    _check(o)
    again = leo.decode(o.orig, o.recv, lo, lr)
    torch.cuda.synchronize()
    for i in lo:
        assert torch.equal(first[i], again[i]), f"original {i} differs between the two decodes"
        assert np.array_equal(again[i].cpu().numpy(), o.data[i]), f"original {i}"
    # and repair again, after the decoder's state was the last one used
    o2 = _setup(leo, k, r, b, lo, lr)
    assert _repair(leo, o2) == leo.LeopardResult.Success, leo.last_error()
    _check(o2)


def _digest(o):
    return hashlib.sha256(_np(o.work).tobytes() + _np(o.rout).tobytes()).hexdigest()


_COMPOSE_SHAPES = [(128, 128, 320, 57, 71), (1000, 200, 128, 64, 136)]

_CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import leopard_amd as leo
import test_gpu_repair as t
assert leo.leo_init() == leo.LeopardResult.Success, leo.last_error()
for shape in t._COMPOSE_SHAPES:
    print("digest", t._digest(t._run(leo, *shape)))
print("child ok")
"""


def test_forced_composition_gives_the_same_bytes(leo):
    env = dict(os.environ, LEO_AMD_REPAIR_COMPOSE="1")
    code = _CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "child ok" in p.stdout, p.stdout + p.stderr
    theirs = [line.split()[1] for line in p.stdout.splitlines() if line.startswith("digest ")]
    ours = [_digest(_run(leo, *shape)) for shape in _COMPOSE_SHAPES]
    assert theirs == ours
