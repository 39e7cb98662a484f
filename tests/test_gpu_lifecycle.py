"""GPU tier: library state over many threads and streams, the multi-GPU host
fan-out, and the column-sharded path run by separate rank processes.

* Scratch lifetime (include/leopard_amd.h, leo_amd_release_stream): the
  reference holds no per-call state (SURVEY.md 8(b) "Ownership"); ours keeps
  per (thread, device, stream) scratch, which must be bounded and freed when a
  thread exits or a stream is released -- device memory returns to where it was.
* Fan-out (leo_amd_set_fanout): a host-memory call split
  into 64-byte-aligned column ranges, each coded by its own worker; the result
  must equal the oracle whatever the split (ranges need not be equal).
* Rank processes: two spawned processes share the one GPU,
  each codes its column range of the object through leo_amd_*_slice; the union
  carries the reference library's digests.
"""
import hashlib
import json
import os
import socket
import threading

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MiB = 1 << 20


def _free_mem():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # torch's cached blocks are not the library's
    return torch.cuda.mem_get_info()[0]


def _settled(base, tol=8 * MiB, wait_s=5.0):
    """Device memory in use above `base`, once released scratch is back: a
    thread's scratch is freed by its thread-exit destructors, which run after
    Python's Thread.join() has returned, so give them a moment."""
    import time
    t0 = time.perf_counter()
    while True:
        used = base - _free_mem()
        if used <= tol or time.perf_counter() - t0 > wait_s:
            return used
        time.sleep(0.05)


def _warm(leo, d_data, d_rec, lost, work):
    """One call on this thread first: device tables and code objects are loaded
    once per process and stay (they are not per-call scratch)."""
    assert _device_decode(leo, d_data, d_rec, lost, work) == leo.LeopardResult.Success, leo.last_error()


def _decode_case(k=1000, r=200, b=4096, seed=3):
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (k, b), dtype=np.uint8)
    rec = ol.oracle().encode(data, r)
    lost = sorted(rng.choice(k, r, replace=False).tolist())
    return data, rec, lost


def _device_decode(leo, d_data, d_rec, lost, work):
    k, b = d_data.shape
    r = d_rec.shape[0]
    los = set(lost)
    res = leo.leo_decode(b, k, r, work.shape[0], [None if i in los else d_data[i].data_ptr() for i in range(k)],
                         [d_rec[i].data_ptr() for i in range(r)], [work[i].data_ptr() for i in range(work.shape[0])])
    return res


def test_scratch_freed_when_threads_exit(leo):
    """100 short-lived threads each run a 1000+200 decode (GF(2^16): device arena,
    decoder state, pinned staging); their scratch is freed when they exit.  A
    thread's scratch for this call is several MiB, so a per-thread leak grows
    with the thread count: memory in use after the second 50 threads must equal
    that after the first 50 (the HIP runtime and the stream-ordered pool keep
    up to a few segments of their own, seen as a constant 0 or 16 MiB on
    different boxes), and stay within 32 MiB of where it started."""
    data, rec, lost = _decode_case()
    d_data, d_rec = torch.from_numpy(data).cuda(), torch.from_numpy(rec).cuda()
    k, b = data.shape
    wc = leo.leo_decode_work_count(k, rec.shape[0])
    works = [torch.zeros((wc, b), dtype=torch.uint8, device="cuda") for _ in range(100)]
    _warm(leo, d_data, d_rec, lost, works[0])
    base = _free_mem()
    results = [None] * 100

    def run(j):
        results[j] = _device_decode(leo, d_data, d_rec, lost, works[j])

    def batch(first):
        for wave in range(5):  # 10 threads at a time
            ts = [threading.Thread(target=run, args=(first + wave * 10 + t,)) for t in range(10)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()

    batch(0)
    used1 = _settled(base, tol=0, wait_s=2.0)
    batch(50)
    used2 = _settled(base, tol=used1, wait_s=5.0)
    assert all(r == leo.LeopardResult.Success for r in results), (results, leo.last_error())
    for w in works:
        for i in lost:
            assert torch.equal(w[i], d_data[i])
    assert used2 <= used1 + 4 * MiB, f"scratch grows with the number of threads: {used1} -> {used2} bytes"
    assert used2 <= 32 * MiB, f"device memory not returned after the threads exited: {used2} bytes"


def test_scratch_bounded_over_fresh_streams(leo):
    """50 fresh streams on one thread: at most 8 scratch sets are kept (least
    recently used freed first), and leo_amd_release_stream returns the rest."""
    data, rec, lost = _decode_case(seed=4)
    d_data, d_rec = torch.from_numpy(data).cuda(), torch.from_numpy(rec).cuda()
    k, b = data.shape
    wc = leo.leo_decode_work_count(k, rec.shape[0])
    work = torch.zeros((wc, b), dtype=torch.uint8, device="cuda")
    _warm(leo, d_data, d_rec, lost, work)
    # torch creates its pool of streams once, and the HIP runtime sets up a
    # stream's own device state (kernel-argument buffers) on its first launch:
    # neither is the library's scratch, so use every pool stream once first
    for _ in range(64):
        with torch.cuda.stream(torch.cuda.Stream()):
            work.add_(0)
    leo.release_stream(-1)
    base = _free_mem()
    used = {}
    try:
        for j in range(50):
            s = torch.cuda.Stream()
            leo.set_stream(s.cuda_stream)
            work.zero_()
            torch.cuda.synchronize()
            assert _device_decode(leo, d_data, d_rec, lost, work) == leo.LeopardResult.Success, leo.last_error()
            s.synchronize()
            for i in lost:
                assert torch.equal(work[i], d_data[i]), (j, i)
            if j % 2:  # every other stream is released by the caller before it goes away
                leo.release_stream(s.cuda_stream)
            used[j] = base - _free_mem()
            del s
        # bounded: no growth with the number of streams seen (the stream-ordered
        # pool may hold a few segments more than the 8 kept scratch sets)
        assert used[49] <= used[24] + 32 * MiB, (used[24], used[49])
    finally:
        leo.set_stream(None)
        leo.release_stream(-1)
    assert _settled(base) <= 8 * MiB, "device memory not returned by leo_amd_release_stream"


def test_large_host_call_returns_its_device_rows(leo):
    """A pageable host call whose direct-copy rows exceed the kept budget
    (128 + 128 pieces of 2 MiB: 512 MiB of device rows) frees them after the
    call, and the library's memory pool hands them back to the device (its
    release threshold is finite, 256 MiB): device memory in use afterwards
    stays within that budget of where it started.  The recovery data equals a
    device-resident encode of the same pieces."""
    k = r = 128
    b = 2 * MiB
    data = np.random.default_rng(11).integers(0, 256, (k, b), dtype=np.uint8)
    work = np.zeros((leo.leo_encode_work_count(k, r), b), dtype=np.uint8)
    d_data = torch.from_numpy(data).cuda()
    d_work = torch.zeros(work.shape, dtype=torch.uint8, device="cuda")
    assert leo.leo_encode(b, k, r, work.shape[0], [d_data[i].data_ptr() for i in range(k)],
                          [d_work[i].data_ptr() for i in range(work.shape[0])]) == leo.LeopardResult.Success
    base = _free_mem()
    assert leo.leo_encode(b, k, r, work.shape[0], [data[i].ctypes.data for i in range(k)],
                          [work[i].ctypes.data for i in range(work.shape[0])]) == leo.LeopardResult.Success, \
        leo.last_error()
    used = _settled(base, tol=300 * MiB)
    assert used <= 300 * MiB, f"{used / MiB:.0f} MiB of device memory still held after a 512 MiB host call"
    assert np.array_equal(work[:r], d_work[:r].cpu().numpy())


def test_async_calls_then_release_wait_for_the_work(leo):
    """Release right after async calls: the scratch is freed only after the
    queued kernels that read it are done (results stay correct)."""
    data, rec, lost = _decode_case(k=600, r=300, b=8192, seed=5)
    d_data, d_rec = torch.from_numpy(data).cuda(), torch.from_numpy(rec).cuda()
    k, b = data.shape
    wc = leo.leo_decode_work_count(k, rec.shape[0])
    s = torch.cuda.Stream()
    works = [torch.zeros((wc, b), dtype=torch.uint8, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    leo.set_stream(s.cuda_stream)
    leo.set_async(True)
    try:
        for w in works:
            assert _device_decode(leo, d_data, d_rec, lost, w) == leo.LeopardResult.Success
        leo.release_stream(s.cuda_stream)
        s.synchronize()
    finally:
        leo.set_async(False)
        leo.set_stream(None)
    for w in works:
        for i in lost:
            assert torch.equal(w[i], d_data[i])


# ------------------------------------------------------------------ fan-out --

FANOUT_CASES = [  # (K, R, B, losses): B is not a multiple of 64 x ranges
    (128, 128, 64 * 1001, 128), (100, 30, 64 * 333, 17), (1000, 200, 64 * 517, 200), (300, 300, 64 * 129, 300),
]


@pytest.mark.parametrize("ranges", [2, 3, 4, -1])
@pytest.mark.parametrize("k,r,b,loss", FANOUT_CASES)
def test_host_fanout_matches_oracle(leo, k, r, b, loss, ranges):
    rng = np.random.default_rng(k * 7 + b + ranges)
    data = rng.integers(0, 256, (k, b), dtype=np.uint8)
    expect = ol.oracle().encode(data, r)
    wc, dwc = leo.leo_encode_work_count(k, r), leo.leo_decode_work_count(k, r)
    work = np.zeros((wc, b), dtype=np.uint8)
    leo.set_fanout(ranges)
    try:
        res = leo.leo_encode(b, k, r, wc, [data[i].ctypes.data for i in range(k)],
                             [work[i].ctypes.data for i in range(wc)])
        assert res == leo.LeopardResult.Success, leo.last_error()
        assert np.array_equal(work[:r], expect)
        lost_o = sorted(rng.choice(k, loss, replace=False).tolist())
        lost_r = sorted(rng.choice(r, r - loss, replace=False).tolist())
        los, lrs = set(lost_o), set(lost_r)
        dwork = np.zeros((dwc, b), dtype=np.uint8)
        res = leo.leo_decode(b, k, r, dwc, [None if i in los else data[i].ctypes.data for i in range(k)],
                             [None if i in lrs else expect[i].ctypes.data for i in range(r)],
                             [dwork[i].ctypes.data for i in range(dwc)])
        assert res == leo.LeopardResult.Success, leo.last_error()
        for i in lost_o:
            assert np.array_equal(dwork[i], data[i]), i
    finally:
        leo.set_fanout(0)


def test_host_fanout_worker_error_reaches_caller(leo):
    """A failure inside a fan-out worker comes back as the caller's result and
    last_error: a lost original without a work piece is checked per column
    range, i.e. on the workers of a fanned-out call."""
    k, r, b = 20, 10, 64 * 40
    data = np.zeros((k, b), dtype=np.uint8)
    rec = ol.oracle().encode(data, r)
    dwc = leo.leo_decode_work_count(k, r)
    dwork = np.zeros((dwc, b), dtype=np.uint8)
    pw = [dwork[i].ctypes.data for i in range(dwc)]
    pw[3] = None  # lost original 3 has no output buffer
    for ranges in (2, 0):
        leo.set_fanout(ranges)
        try:
            res = leo.leo_decode(b, k, r, dwc, [None if i == 3 else data[i].ctypes.data for i in range(k)],
                                 [rec[i].ctypes.data for i in range(r)], pw)
        finally:
            leo.set_fanout(0)
        assert res == leo.LeopardResult.InvalidInput, (ranges, res)
        assert "work_data[3]" in leo.last_error(), leo.last_error()


# ----------------------------------------------------- rank processes ------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_main(rank, world, port, shared, results):
    """One rank: its column range of each object through leo_amd_*_slice
    (leopard_amd.sharding), on the one GPU both ranks share; gloo carries only
    the barrier and the max of the elapsed times (no data-path collective).
    The rank copies its columns of the outputs into the test's shared host
    tensors (the test-side gather)."""
    import sys
    import time
    import torch as th
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        import oracle_lib as olr
        import leopard_amd as leo
        from leopard_amd.sharding import decode_shard, encode_shard, max_over_ranks, shard_for_rank
        th.cuda.set_device(0)
        assert leo.leo_init() == 0, leo.last_error()
        for (k, r, b) in [(1000, 200, 65536), (32768, 32768, 65536)]:
            off, size = shard_for_rank(b, rank, world)
            data = olr.hash_bytes_torch(7, k, b, "cuda")
            wc, dwc = leo.leo_encode_work_count(k, r), leo.leo_decode_work_count(k, r)
            work = th.empty((wc, b), dtype=th.uint8, device="cuda")
            po = [data[i].data_ptr() for i in range(k)]
            pw = [work[i].data_ptr() for i in range(wc)]
            dist.barrier()
            t0 = time.perf_counter()
            assert encode_shard(b, rank, world, k, r, po, pw) == 0, leo.last_error()
            th.cuda.synchronize()
            el = max_over_ranks(time.perf_counter() - t0)
            shared[f"rec_{k}"][:, off:off + size].copy_(work[:r, off:off + size].cpu())
            dwork = th.empty((dwc, b), dtype=th.uint8, device="cuda")
            pd = [dwork[i].data_ptr() for i in range(dwc)]
            pr = [work[i].data_ptr() for i in range(r)]
            if k == r:  # full loss of the originals: rebuilt exactly
                assert decode_shard(b, rank, world, k, r, [None] * k, pr, pd) == 0, leo.last_error()
                th.cuda.synchronize()
                ok = bool(th.equal(dwork[:k, off:off + size], data[:, off:off + size]))
            else:  # the decoder's exact map on non-codeword input (reference decode digest)
                junk = olr.hash_bytes_torch(8, r, b, "cuda")
                lo, lr = olr.benchmark_losses(k, r, r, seed=2, trial=0)
                los, lrs = set(lo), set(lr)
                assert decode_shard(b, rank, world, k, r, [None if i in los else po[i] for i in range(k)],
                                    [None if i in lrs else junk[i].data_ptr() for i in range(r)], pd) == 0
                th.cuda.synchronize()
                idx = th.tensor(lo, device="cuda")
                shared[f"dec_{k}"][:, off:off + size].copy_(dwork.index_select(0, idx)[:, off:off + size].cpu())
                ok = True
            out[k] = (ok, el)
            del data, work, dwork
            th.cuda.empty_cache()
        results.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.slow
def test_two_rank_processes_share_the_gpu_sliced(leo):
    import torch.multiprocessing as mp
    with open(os.path.join(GOLDEN, "golden_digests.json")) as f:
        dig = json.load(f)
    shared = {"rec_1000": torch.zeros((200, 65536), dtype=torch.uint8).share_memory_(),
              "dec_1000": torch.zeros((200, 65536), dtype=torch.uint8).share_memory_(),
              "rec_32768": torch.zeros((32768, 65536), dtype=torch.uint8).share_memory_()}
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(rk, 2, port, shared, q)) for rk in range(2)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(2):
        rank, out = q.get(timeout=110)
        got[rank] = out
    for p in procs:
        p.join(timeout=30)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    for rank in (0, 1):
        assert got[rank][1000][0] and got[rank][32768][0], got
        assert got[rank][32768][1] == got[1 - rank][32768][1]  # max over ranks agrees
    sha = lambda t: hashlib.sha256(t.numpy().tobytes()).hexdigest()  # noqa: E731
    assert sha(shared["rec_1000"]) == dig["hash_digests"]["1000_200_65536"]
    assert sha(shared["dec_1000"]) == dig["decode_hash_digests"]["1000_200_65536"]
    assert sha(shared["rec_32768"]) == dig["hash_digests"]["32768_32768_65536"]


_TUNED_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import leopard_amd as leo, oracle_lib as ol, torch
assert leo.leo_init() == 0, leo.last_error()
o = ol.oracle()
# GF(2^16) multi-pass (m = 1024, n = 4096): LEO_AMD_SLICE_MB=1 cuts 4096-byte columns into 512-byte slices
k, r, b = 2000, 1000, 4096
data = ol.pcg_bytes(11, k, k, b)
dev = torch.from_numpy(data).cuda()
rec = leo.encode(dev, r)
torch.cuda.synchronize()
exp = o.encode(data, r)
assert np.array_equal(rec.cpu().numpy(), exp), "sliced encode"
lost = list(range(0, k, 3))[:r]
got = leo.decode(dev, rec, lost, [])
torch.cuda.synchronize()
assert all(torch.equal(got[i], dev[i]) for i in lost), "sliced decode"
# host ring with LEO_AMD_SLOT_MB=1: scattered pageable pieces, many slices
k, r, b = 128, 64, 65536
data = ol.pcg_bytes(12, k, k, b)
din = [np.zeros(b, dtype=np.uint8) for _ in range(k)]
din.sort(key=lambda x: -x.ctypes.data)  # descending addresses: no row runs, so the ring takes the call
for i in range(k):
    din[i][:] = data[i]
wc = leo.leo_encode_work_count(k, r)
work = [np.zeros(b, dtype=np.uint8) for _ in range(wc)]
work.sort(key=lambda x: -x.ctypes.data)
assert leo.leo_encode(b, k, r, wc, [x.ctypes.data for x in din], [x.ctypes.data for x in work]) == 0, leo.last_error()
assert np.array_equal(np.stack(work[:r]), o.encode(data, r)), "ring encode"
print("tuned ok")
"""


def test_tuning_switches_at_non_default_values():
    """LEO_AMD_SLICE_MB (device scratch per GF(2^16) multi-pass slice) and
    LEO_AMD_SLOT_MB (host ring slot) at small non-default values: many column
    slices, results equal to the oracle.  Read once per process, so they run in
    a child process with the variables set."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, LEO_AMD_SLICE_MB="1", LEO_AMD_SLOT_MB="1")
    code = _TUNED_SCRIPT.format(repo=os.path.dirname(here), tests=here)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0 and "tuned ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_bench_line_batch_timing_small():
    """bench.py --full end to end at a small size (4 objects in launches of 2, 2
    streams): one JSON line whose roofline launch time comes from the events
    inside the timed region (GPU time per launch <= a launch's own span;
    achieved = algorithmic bytes / launch time)."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
                        "--objects", "4", "--launch-objects", "2", "--sets", "8", "--no-host", "--no-cpu-baseline",
                        "--no-sharded", "--no-secondary"], capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    r = d["roofline"]
    assert d["value"] > 0 and d["config"]["mode"] == "batch" and d["config"]["objects_per_launch"] == 2
    span = max(r["launch_span_encode_us"], r["launch_span_decode_us"])
    assert 0 < r["launch_us"] <= span * 1.05
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / r["launch_us"] / 1e3) <= 0.01 * r["achieved"] + 0.01
    assert r["frac"] < 1.0


@pytest.mark.gpu
def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run at a small size (4 objects in launches of 2): the
    headline line alone, value = input bytes of the timed steps over their time,
    ms_per_step that time per step; --dump-outputs writes what the last timed
    step computed (buffer sets 0..3 here): the decoded originals are the inputs,
    the recovery pieces the oracle's."""
    import json
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import bench  # the repository root is on sys.path (conftest.py)
    p = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--objects", "4", "--launch-objects", "2", "--sets", "8", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1
    assert not {"roofline", "modes", "cpu_baseline", "sharded_object", "host_e2e", "secondary", "breadth"} & set(d)
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    k = r = 128
    b = 65536
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(4 * k * b / (d["ms_per_step"] * 1e-3) / 1e9, rel=0.01)
    files = {f: np.load(tmp_path / f) for f in d["dump_outputs"]["files"]}
    assert sorted(files) == sorted(os.listdir(tmp_path))
    assert sum(a.nbytes for a in files.values()) <= 64_000_000
    pos = bench.dump_positions(k * b, 4)
    for j in range(4):
        orig = ol.hash_bytes(7 + j, k, b)
        assert np.array_equal(files["decoded.npy"][j], orig.reshape(-1)[pos].astype(np.float32))
        assert np.array_equal(files["decoded_sums.npy"][j], orig.sum(axis=1, dtype=np.int64).astype(np.float64))
    rec = ol.oracle().encode(ol.hash_bytes(7, k, b), r)
    assert np.array_equal(files["recovery.npy"][0], rec.reshape(-1)[pos].astype(np.float32))
    assert np.array_equal(files["recovery_sums.npy"][0], rec.sum(axis=1, dtype=np.int64).astype(np.float64))
