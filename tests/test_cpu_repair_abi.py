"""CPU tier: leo_amd_repair / leo_amd_repair_slice / leo_amd_repair_batch decide
their validation results in the header's order (include/leopard_amd.h):
InvalidSize (slice form: the slice checks first), InvalidCounts, InvalidInput
for a NULL array with its name in leo_amd_last_error(), then CallInitialize.
No call below may touch a buffer."""
import ctypes

import pytest

K, R, B = 7, 3, 128
FILL = 0xA5


@pytest.fixture(scope="module")
def leo():
    import leopard_amd
    return leopard_amd


@pytest.fixture()
def bufs(leo):
    """Sentinel-filled host pieces: K originals, R recovery, work and recovery_out buffers."""
    wc = leo.leo_decode_work_count(K, R)
    pieces = [(ctypes.c_uint8 * B)(*([FILL] * B)) for _ in range(K + R + wc + R)]
    ptrs = [ctypes.addressof(p) for p in pieces]
    orig, rec = ptrs[:K], ptrs[K:K + R]
    work, rout = ptrs[K + R:K + R + wc], ptrs[K + R + wc:]
    orig[2] = None  # one original and one recovery piece lost
    rec[1] = None
    return pieces, wc, orig, rec, work, rout


def _untouched(pieces):
    return all(bytes(p) == bytes([FILL]) * B for p in pieces)


def _gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_python_names(leo):
    for name in ("leo_amd_repair", "leo_amd_repair_slice", "leo_amd_repair_batch", "repair"):
        assert callable(getattr(leo, name)) and name in leo.__all__
    for name in ("leo_amd_repair", "leo_amd_repair_slice", "leo_amd_repair_batch"):
        assert getattr(leo.lib, name).argtypes is not None


@pytest.mark.parametrize("nbytes", [0, 1, 63, 65, 96])
def test_invalid_size(leo, bufs, nbytes):
    pieces, wc, orig, rec, work, rout = bufs
    assert leo.leo_amd_repair(nbytes, K, R, wc, orig, rec, work, rout) == leo.LeopardResult.InvalidSize
    # size precedes counts and NULL arrays
    assert leo.leo_amd_repair(nbytes, K, 0, wc, None, None, None, None) == leo.LeopardResult.InvalidSize
    assert leo.leo_amd_repair_batch(nbytes, K, 0, wc, [None], [None], [None], [None]) == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


@pytest.mark.parametrize("off,length", [(0, 0), (0, 32), (32, 64), (64, 128), (128, 64), (0, 192)])
def test_slice_invalid_size(leo, bufs, off, length):
    pieces, wc, orig, rec, work, rout = bufs
    assert leo.leo_amd_repair_slice(B, off, length, K, R, wc, orig, rec, work, rout) == leo.LeopardResult.InvalidSize
    # the slice checks precede counts and NULL arrays too
    assert leo.leo_amd_repair_slice(B, off, length, K, 0, wc, None, None, None, None) == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


def test_slice_checks_the_buffer_size_too(leo, bufs):
    pieces, wc, orig, rec, work, rout = bufs
    assert leo.leo_amd_repair_slice(100, 0, 64, K, R, wc, orig, rec, work, rout) == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


@pytest.mark.parametrize("k,r", [(7, 0), (7, 8)])
def test_invalid_counts(leo, bufs, k, r):
    pieces, wc, orig, rec, work, rout = bufs
    # counts precede every pointer check: NULL arrays are not looked at
    assert leo.leo_amd_repair(B, k, r, wc, None, None, None, None) == leo.LeopardResult.InvalidCounts
    assert leo.leo_amd_repair_slice(B, 0, 64, k, r, wc, None, None, None, None) == leo.LeopardResult.InvalidCounts
    assert leo.leo_amd_repair_batch(B, k, r, wc, [None], [None], [None], [None]) == leo.LeopardResult.InvalidCounts
    assert _untouched(pieces)


@pytest.mark.parametrize("which,name", [(0, "original_data"), (1, "recovery_data"), (2, "work_data"),
                                        (3, "recovery_out")])
def test_null_array(leo, bufs, which, name):
    pieces, wc, orig, rec, work, rout = bufs
    args = [orig, rec, work, rout]
    args[which] = None
    assert leo.leo_amd_repair(B, K, R, wc, *args) == leo.LeopardResult.InvalidInput
    assert name in leo.last_error()
    assert leo.leo_amd_repair_slice(B, 0, 64, K, R, wc, *args) == leo.LeopardResult.InvalidInput
    assert name in leo.last_error()
    assert _untouched(pieces)


@pytest.mark.skipif(_gpu(), reason="CPU-only behaviour")
def test_call_initialize_comes_after_the_input_checks(leo, bufs):
    pieces, wc, orig, rec, work, rout = bufs
    assert leo.leo_init() == leo.LeopardResult.Platform
    assert leo.leo_amd_repair(B, K, R, wc, orig, rec, work, rout) == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_repair_slice(B, 64, 64, K, R, wc, orig, rec, work, rout) == leo.LeopardResult.CallInitialize
    # ... ahead of NeedMoreData, the work count and a NULL work piece, as in leo_decode
    assert leo.leo_amd_repair(B, K, R, wc, [None] * K, rec, work, rout) == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_repair(B, K, R, wc + 1, orig, rec, work, rout) == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_repair(B, K, R, wc, orig, rec, [None] * wc, rout) == leo.LeopardResult.CallInitialize
    # ... and behind the NULL arrays
    assert leo.leo_amd_repair(B, K, R, wc, orig, rec, work, None) == leo.LeopardResult.InvalidInput
    assert _untouched(pieces)


def test_batch_returns_the_first_failing_objects_result(leo, bufs):
    pieces, wc, orig, rec, work, rout = bufs
    good = (orig, rec, work, rout)
    no_rout = (orig, rec, work, None)
    no_orig = (None, rec, work, rout)

    def batch(*objs):
        return leo.leo_amd_repair_batch(B, K, R, wc, *[[o[n] for o in objs] for n in range(4)])

    assert batch(no_rout, no_orig) == leo.LeopardResult.InvalidInput
    assert "recovery_out" in leo.last_error()
    assert batch(no_orig, no_rout) == leo.LeopardResult.InvalidInput
    assert "original_data" in leo.last_error()
    if not _gpu():  # object 0 passes the input checks and fails first, at the init check
        assert batch(good, no_rout) == leo.LeopardResult.CallInitialize
    # a NULL outer array
    assert leo.lib.leo_amd_repair_batch(1, B, K, R, wc, None, None, None, None) == leo.LeopardResult.InvalidInput
    assert "original_data" in leo.last_error()
    assert _untouched(pieces)


def test_batch_lists_must_agree(leo, bufs):
    pieces, wc, orig, rec, work, rout = bufs
    with pytest.raises(ValueError):
        leo.leo_amd_repair_batch(B, K, R, wc, [orig, orig], [rec], [work], [rout])


def test_tensor_helper_rejects_mismatched_shapes(leo):
    import torch
    orig = torch.zeros((K, B), dtype=torch.uint8)
    with pytest.raises(ValueError):
        leo.repair(orig, torch.zeros((R, B + 64), dtype=torch.uint8), [2], [1])
    with pytest.raises(ValueError):
        leo.repair(orig, torch.zeros((R * B,), dtype=torch.uint8), [2], [1])
    with pytest.raises(ValueError):
        leo.repair(orig, torch.zeros((R, B), dtype=torch.uint8), [K], [1])
    with pytest.raises(ValueError):  # a piece that is not lost cannot be requested
        leo.repair(orig, torch.zeros((R, B), dtype=torch.uint8), [2], [1], want_recovery=[0])
