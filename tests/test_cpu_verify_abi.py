"""CPU tier: leo_amd_verify / leo_amd_verify_slice / leo_amd_verify_batch are
exported and bound, and decide their validation results in the header's order
(include/leopard_amd.h): InvalidSize (slice form: the slice checks first),
InvalidCounts, InvalidInput for a NULL array or a NULL original with its name
or index in leo_amd_last_error(), then CallInitialize.  No call below may touch
a piece or a report."""
import ctypes

import numpy as np
import pytest

K, R, B = 7, 3, 128
FILL = 0xA5
STALE = 0xDEADBEEF  # what the caller's bitmap holds before a call that fails


@pytest.fixture(scope="module")
def leo():
    import leopard_amd
    return leopard_amd


@pytest.fixture()
def bufs(leo):
    """Sentinel-filled host pieces: K originals, R recovery pieces (piece 1 not at hand)."""
    pieces = [(ctypes.c_uint8 * B)(*([FILL] * B)) for _ in range(K + R)]
    ptrs = [ctypes.addressof(p) for p in pieces]
    orig, rec = ptrs[:K], ptrs[K:]
    rec[1] = None
    return pieces, orig, rec


def _untouched(pieces):
    return all(bytes(p) == bytes([FILL]) * B for p in pieces)


def _gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _stale(objects=1):
    return np.full(objects * ((R + 31) // 32), STALE, dtype=np.uint32)


def test_symbols_are_exported_and_bound(leo):
    for name in ("leo_amd_verify", "leo_amd_verify_slice", "leo_amd_verify_batch"):
        fn = getattr(leo.lib, name)  # AttributeError: the .so does not export it
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert len(leo.lib.leo_amd_verify.argtypes) == 7
    assert len(leo.lib.leo_amd_verify_slice.argtypes) == 9
    assert len(leo.lib.leo_amd_verify_batch.argtypes) == 8


def test_python_names(leo):
    for name in ("leo_amd_verify", "leo_amd_verify_slice", "leo_amd_verify_batch", "verify"):
        assert callable(getattr(leo, name)) and name in leo.__all__


@pytest.mark.parametrize("nbytes", [0, 1, 63, 65, 96])
def test_invalid_size(leo, bufs, nbytes):
    pieces, orig, rec = bufs
    bm = _stale()
    assert leo.leo_amd_verify(nbytes, K, R, orig, rec, bm)[0] == leo.LeopardResult.InvalidSize
    # size precedes counts and NULL arrays
    assert leo.leo_amd_verify(nbytes, K, 0, None, None, None, count=False)[0] == leo.LeopardResult.InvalidSize
    assert leo.leo_amd_verify_batch(nbytes, K, 0, [None], [None], None, count=False)[0] == leo.LeopardResult.InvalidSize
    assert _untouched(pieces) and (bm == STALE).all()


@pytest.mark.parametrize("off,length", [(0, 0), (0, 32), (32, 64), (64, 128), (128, 64), (0, 192)])
def test_slice_invalid_size(leo, bufs, off, length):
    pieces, orig, rec = bufs
    bm = _stale()
    assert leo.leo_amd_verify_slice(B, off, length, K, R, orig, rec, bm)[0] == leo.LeopardResult.InvalidSize
    # the slice checks precede counts and NULL arrays too
    res = leo.leo_amd_verify_slice(B, off, length, K, 0, None, None, None, count=False)[0]
    assert res == leo.LeopardResult.InvalidSize
    assert _untouched(pieces) and (bm == STALE).all()


def test_slice_checks_the_buffer_size_too(leo, bufs):
    pieces, orig, rec = bufs
    assert leo.leo_amd_verify_slice(100, 0, 64, K, R, orig, rec)[0] == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


@pytest.mark.parametrize("k,r", [(7, 0), (7, 8)])
def test_invalid_counts(leo, bufs, k, r):
    pieces, orig, rec = bufs
    # counts precede every pointer check: NULL arrays are not looked at
    assert leo.leo_amd_verify(B, k, r, None, None, None, count=False)[0] == leo.LeopardResult.InvalidCounts
    res = leo.leo_amd_verify_slice(B, 0, 64, k, r, None, None, None, count=False)[0]
    assert res == leo.LeopardResult.InvalidCounts
    assert leo.leo_amd_verify_batch(B, k, r, [None], [None], None, count=False)[0] == leo.LeopardResult.InvalidCounts
    assert _untouched(pieces)


@pytest.mark.parametrize("which,name", [(0, "original_data"), (1, "recovery_data")])
def test_null_array(leo, bufs, which, name):
    pieces, orig, rec = bufs
    args = [orig, rec]
    args[which] = None
    bm = _stale()
    assert leo.leo_amd_verify(B, K, R, *args, bm)[0] == leo.LeopardResult.InvalidInput
    assert name in leo.last_error()
    assert leo.leo_amd_verify_slice(B, 0, 64, K, R, *args, bm)[0] == leo.LeopardResult.InvalidInput
    assert name in leo.last_error()
    assert _untouched(pieces) and (bm == STALE).all()


def test_null_mismatch_count(leo, bufs):
    pieces, orig, rec = bufs
    bm = _stale()
    res, count, _ = leo.leo_amd_verify(B, K, R, orig, rec, bm, count=False)
    assert res == leo.LeopardResult.InvalidInput and count is None
    assert "mismatch_count" in leo.last_error()
    assert leo.leo_amd_verify_slice(B, 64, 64, K, R, orig, rec, bm, count=False)[0] == leo.LeopardResult.InvalidInput
    assert "mismatch_count" in leo.last_error()
    assert leo.leo_amd_verify_batch(B, K, R, [orig], [rec], bm, count=False)[0] == leo.LeopardResult.InvalidInput
    assert "mismatch_count" in leo.last_error()
    assert _untouched(pieces) and (bm == STALE).all()


@pytest.mark.parametrize("i", [0, 4, K - 1])
def test_null_original_is_named(leo, bufs, i):
    pieces, orig, rec = bufs
    orig = list(orig)
    orig[i] = None
    bm = _stale()
    assert leo.leo_amd_verify(B, K, R, orig, rec, bm)[0] == leo.LeopardResult.InvalidInput
    assert f"original_data[{i}]" in leo.last_error()
    assert leo.leo_amd_verify_slice(B, 0, 64, K, R, orig, rec, bm)[0] == leo.LeopardResult.InvalidInput
    assert f"original_data[{i}]" in leo.last_error()
    assert leo.leo_amd_verify_batch(B, K, R, [orig], [rec], bm)[0] == leo.LeopardResult.InvalidInput
    assert f"original_data[{i}]" in leo.last_error()
    assert _untouched(pieces) and (bm == STALE).all()


@pytest.mark.skipif(_gpu(), reason="CPU-only behaviour")
def test_call_initialize_comes_after_the_input_checks(leo, bufs):
    pieces, orig, rec = bufs
    bm = _stale()
    assert leo.leo_init() == leo.LeopardResult.Platform
    assert leo.leo_amd_verify(B, K, R, orig, rec, bm)[0] == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_verify_slice(B, 64, 64, K, R, orig, rec, bm)[0] == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_verify_batch(B, K, R, [orig], [rec], bm)[0] == leo.LeopardResult.CallInitialize
    # ... with no piece to check too (validation comes first), and ahead of TooMuchData
    assert leo.leo_amd_verify(B, K, R, orig, [None] * R, bm)[0] == leo.LeopardResult.CallInitialize
    big = [orig[0]] * 40000
    assert leo.leo_amd_verify(B, 40000, 30000, big, [None] * 30000, None)[0] == leo.LeopardResult.CallInitialize
    # ... and behind the NULL arrays and the NULL original
    assert leo.leo_amd_verify(B, K, R, orig, None, bm)[0] == leo.LeopardResult.InvalidInput
    assert leo.leo_amd_verify(B, K, R, [None] + orig[1:], rec, bm)[0] == leo.LeopardResult.InvalidInput
    assert _untouched(pieces) and (bm == STALE).all()


def test_batch_returns_the_first_failing_objects_result(leo, bufs):
    pieces, orig, rec = bufs
    good = (orig, rec)
    no_rec = (orig, None)
    no_orig = (None, rec)
    hole = (orig[:3] + [None] + orig[4:], rec)
    bm = _stale(2)

    def batch(*objs):
        return leo.leo_amd_verify_batch(B, K, R, [o[0] for o in objs], [o[1] for o in objs], bm)[0]

    assert batch(no_rec, no_orig) == leo.LeopardResult.InvalidInput
    assert "recovery_data" in leo.last_error()
    assert batch(no_orig, no_rec) == leo.LeopardResult.InvalidInput
    assert "original_data" in leo.last_error()
    assert batch(hole, no_rec) == leo.LeopardResult.InvalidInput
    assert "original_data[3]" in leo.last_error()
    if _gpu():  # the second object is the invalid one: nothing runs, no report is written
        assert leo.leo_init() == leo.LeopardResult.Success
        assert batch(good, no_rec) == leo.LeopardResult.InvalidInput
        assert "recovery_data" in leo.last_error()
        assert batch(good, hole) == leo.LeopardResult.InvalidInput
        assert "original_data[3]" in leo.last_error()
    else:  # object 0 passes the input checks and fails first, at the init check
        assert batch(good, no_rec) == leo.LeopardResult.CallInitialize
    # a NULL outer array
    counts = (ctypes.c_uint * 1)()
    assert leo.lib.leo_amd_verify_batch(1, B, K, R, None, None, None, counts) == leo.LeopardResult.InvalidInput
    assert "original_data" in leo.last_error()
    assert _untouched(pieces) and (bm == STALE).all()


def test_batch_lists_must_agree(leo, bufs):
    pieces, orig, rec = bufs
    with pytest.raises(ValueError):
        leo.leo_amd_verify_batch(B, K, R, [orig, orig], [rec])


def test_tensor_helper_rejects_mismatched_shapes(leo):
    import torch
    orig = torch.zeros((K, B), dtype=torch.uint8)
    with pytest.raises(ValueError):
        leo.verify(orig, torch.zeros((R, B + 64), dtype=torch.uint8))
    with pytest.raises(ValueError):
        leo.verify(orig, torch.zeros((R * B,), dtype=torch.uint8))
    with pytest.raises(ValueError):
        leo.verify(orig, torch.zeros((R, B), dtype=torch.uint8), have_recovery=[R])
