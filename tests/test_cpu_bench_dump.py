"""CPU tier for bench.py --dump-outputs (dump_last_step): the files, their
types and sizes, and that the same buffers give the same files, on stand-in
buffer sets in host memory."""
import os
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _sets(k, r, nbytes, n, wc):
    g = torch.Generator().manual_seed(5)
    mk = lambda: [torch.randint(0, 256, (wc, nbytes), dtype=torch.uint8, generator=g) for _ in range(n)]  # noqa: E731
    return types.SimpleNamespace(k=k, r=r, nbytes=nbytes, orig=[torch.zeros(1)] * n, enc_work=mk(), dec_work=mk())


@pytest.mark.parametrize("k,r,nbytes", [(4, 3, 256), (128, 128, 32768)])
def test_dump_last_step_files(tmp_path, k, r, nbytes):
    import bench
    sets = _sets(k, r, nbytes, 3, 2 * max(k, r))
    ids = [2, 0]
    info = bench.dump_last_step(torch, str(tmp_path / "a"), sets, ids, 0, 1)
    again = bench.dump_last_step(torch, str(tmp_path / "b"), sets, ids, 0, 1)
    assert info["files"] == again["files"] == ["decoded.npy", "decoded_sums.npy", "recovery.npy", "recovery_sums.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == info["files"]
    total = 0
    for f in info["files"]:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == (np.float64 if f.endswith("_sums.npy") else np.float32)
        assert a.shape[0] == len(ids) and np.array_equal(a, b)
        total += a.nbytes
    assert total == info["bytes"] <= bench.DUMP_LIMIT
    for name, bufs, rows in (("recovery", sets.enc_work, r), ("decoded", sets.dec_work, k)):
        sums = np.load(tmp_path / "a" / (name + "_sums.npy"))
        sample = np.load(tmp_path / "a" / (name + ".npy"))
        for j, i in enumerate(ids):
            want = bufs[i][:rows].numpy()
            assert np.array_equal(sums[j], want.sum(axis=1, dtype=np.int64).astype(np.float64))
            pos = bench.dump_positions(want.size, len(ids))
            assert (len(pos) == want.size) == (nbytes == 256)  # small pieces: every byte; large: a sample
            assert np.array_equal(sample[j], want.reshape(-1)[pos].astype(np.float32))


def test_dump_last_step_names_ranks(tmp_path):
    import bench
    info = bench.dump_last_step(torch, str(tmp_path), _sets(2, 2, 64, 1, 4), [0], 1, 2)
    assert info["files"] == ["decoded_rank1.npy", "decoded_sums_rank1.npy", "recovery_rank1.npy",
                             "recovery_sums_rank1.npy"]
    assert sorted(os.listdir(tmp_path)) == info["files"]
