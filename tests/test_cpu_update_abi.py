"""CPU tier: leo_amd_update / leo_amd_update_slice decide every validation
result before any GPU call, in check_encode's order (include/leopard_amd.h):
InvalidSize, InvalidCounts, changed_count == 0 (Success, nothing touched),
InvalidInput with the offending position in leo_amd_last_error(), then
CallInitialize."""
import ctypes

import pytest

K, R, B = 7, 3, 128


@pytest.fixture(scope="module")
def leo():
    import leopard_amd
    return leopard_amd


@pytest.fixture()
def bufs():
    """Host pieces: 2 deltas and R recovery pieces with a known fill (no call below may touch them)."""
    pieces = [(ctypes.c_uint8 * B)(*([17 + n] * B)) for n in range(2 + R)]
    ptrs = [ctypes.addressof(p) for p in pieces]
    return pieces, ptrs[:2], ptrs[2:]


def _untouched(pieces):
    return all(bytes(p) == bytes([17 + n]) * B for n, p in enumerate(pieces))


def _gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_python_names(leo):
    for name in ("leo_amd_update", "leo_amd_update_slice", "update"):
        assert callable(getattr(leo, name)) and name in leo.__all__
    assert leo.UPDATE_MAX_CHANGED == 32
    assert leo.lib.leo_amd_update.argtypes is not None and leo.lib.leo_amd_update_slice.argtypes is not None


@pytest.mark.parametrize("nbytes", [0, 1, 63, 65, 96, 64 * 3 + 32])
def test_invalid_size(leo, bufs, nbytes):
    pieces, d, r = bufs
    assert leo.leo_amd_update(nbytes, K, R, 2, [0, 1], d, r) == leo.LeopardResult.InvalidSize
    # size precedes counts and NULL arrays
    assert leo.leo_amd_update(nbytes, K, 0, 40, None, None, None) == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


@pytest.mark.parametrize("off,length", [(0, 0), (0, 32), (32, 64), (64, 128), (128, 64), (0, 192)])
def test_slice_invalid_size(leo, bufs, off, length):
    pieces, d, r = bufs
    assert leo.leo_amd_update_slice(B, off, length, K, R, 2, [0, 1], d, r) == leo.LeopardResult.InvalidSize
    assert _untouched(pieces)


def test_slice_checks_the_buffer_size_too(leo, bufs):
    pieces, d, r = bufs
    assert leo.leo_amd_update_slice(100, 0, 64, K, R, 2, [0, 1], d, r) == leo.LeopardResult.InvalidSize


@pytest.mark.parametrize("k,r,c", [(7, 0, 1), (7, 8, 1), (1, 2, 1), (64, 64, 33), (1000, 200, 1000)])
def test_invalid_counts(leo, bufs, k, r, c):
    pieces, d, rec = bufs
    # counts precede every pointer check: NULL arrays are not looked at
    assert leo.leo_amd_update(B, k, r, c, None, None, None) == leo.LeopardResult.InvalidCounts
    assert leo.leo_amd_update_slice(B, 0, 64, k, r, c, None, None, None) == leo.LeopardResult.InvalidCounts
    assert _untouched(pieces)


def test_changed_count_33_with_valid_arrays(leo):
    deltas = [(ctypes.c_uint8 * 64)() for _ in range(33)]
    rec = [(ctypes.c_uint8 * 64)() for _ in range(64)]
    res = leo.leo_amd_update(64, 64, 64, 33, list(range(33)), [ctypes.addressof(p) for p in deltas],
                             [ctypes.addressof(p) for p in rec])
    assert res == leo.LeopardResult.InvalidCounts


def test_nothing_changed_is_success_before_the_init_check(leo, bufs):
    pieces, d, r = bufs
    # no leo_init() needed, NULL arrays allowed, nothing touched
    assert leo.leo_amd_update(B, K, R, 0, None, None, None) == leo.LeopardResult.Success
    assert leo.leo_amd_update(B, K, R, 0, [], d, r) == leo.LeopardResult.Success
    assert leo.leo_amd_update_slice(B, 64, 64, K, R, 0, None, None, None) == leo.LeopardResult.Success
    # ... but sizes and counts are still checked
    assert leo.leo_amd_update(B + 1, K, R, 0, None, None, None) == leo.LeopardResult.InvalidSize
    assert leo.leo_amd_update(B, K, K + 1, 0, None, None, None) == leo.LeopardResult.InvalidCounts
    assert _untouched(pieces)


@pytest.mark.parametrize("which,name", [(0, "changed_index"), (1, "delta_data"), (2, "recovery_data")])
def test_null_array(leo, bufs, which, name):
    pieces, d, r = bufs
    args = [[0, 1], d, r]
    args[which] = None
    assert leo.leo_amd_update(B, K, R, 2, *args) == leo.LeopardResult.InvalidInput
    assert name in leo.last_error()
    assert leo.leo_amd_update_slice(B, 0, 64, K, R, 2, *args) == leo.LeopardResult.InvalidInput
    assert _untouched(pieces)


def test_null_element(leo, bufs):
    pieces, d, r = bufs
    assert leo.leo_amd_update(B, K, R, 2, [0, 1], [d[0], None], r) == leo.LeopardResult.InvalidInput
    assert "delta_data[1]" in leo.last_error()
    assert leo.leo_amd_update(B, K, R, 2, [0, 1], d, [r[0], r[1], None]) == leo.LeopardResult.InvalidInput
    assert "recovery_data[2]" in leo.last_error()
    assert _untouched(pieces)


def test_index_out_of_range(leo, bufs):
    pieces, d, r = bufs
    assert leo.leo_amd_update(B, K, R, 2, [0, K], d, r) == leo.LeopardResult.InvalidInput
    assert "changed_index[1]" in leo.last_error() and str(K) in leo.last_error()
    assert leo.leo_amd_update(B, K, R, 1, [2 ** 32 - 1], d[:1], r) == leo.LeopardResult.InvalidInput
    assert "changed_index[0]" in leo.last_error()
    assert _untouched(pieces)


def test_repeated_index(leo, bufs):
    pieces, d, r = bufs
    assert leo.leo_amd_update(B, K, R, 2, [4, 4], d, r) == leo.LeopardResult.InvalidInput
    assert "changed_index[1]" in leo.last_error() and "changed_index[0]" in leo.last_error()
    assert _untouched(pieces)


@pytest.mark.skipif(_gpu(), reason="CPU-only behaviour")
def test_call_initialize_comes_after_the_input_checks(leo, bufs):
    pieces, d, r = bufs
    assert leo.leo_init() == leo.LeopardResult.Platform
    assert leo.leo_amd_update(B, K, R, 2, [0, 1], d, r) == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_update_slice(B, 64, 64, K, R, 2, [0, 1], d, r) == leo.LeopardResult.CallInitialize
    # the codeword-length check comes after it, as in leo_encode
    big = [(ctypes.c_uint8 * 64)() for _ in range(2)]
    assert leo.leo_amd_update(64, 60000, 2, 1, [5], [ctypes.addressof(big[0])],
                              [ctypes.addressof(p) for p in big]) == leo.LeopardResult.CallInitialize
    assert leo.leo_amd_update(B, K, R, 2, [0, K], d, r) == leo.LeopardResult.InvalidInput
    assert _untouched(pieces)


def test_tensor_helper_rejects_mismatched_shapes(leo):
    import torch
    rec = torch.zeros((R, B), dtype=torch.uint8)
    with pytest.raises(ValueError):
        leo.update(rec, K, [0, 1], torch.zeros((1, B), dtype=torch.uint8))
    with pytest.raises(ValueError):
        leo.update(rec, K, [0], torch.zeros((1, B + 64), dtype=torch.uint8))
