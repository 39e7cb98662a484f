"""The workgroup-cooperative bit-sliced tile (rs_ff8_bs.hip, WB wave bits: the
1 << WB waves of a workgroup share one tile of 128 pieces x S bytes, S = 256 <<
WB): 128 + 128 slab batches through leo_amd_encode_batch / leo_amd_decode_batch,
encode against the oracle, the full-loss decode back to the originals.  The
shapes are the smallest at which the tile's new parts can go wrong: partial
strips (whole waves' lanes past the piece's end), fewer than 8 workgroups
(static assignment), the tile queue with and without a second round, and
every wave's code variant.  The product library runs its shipped tile; the
experiment library (lib/exp) runs each of them, forced, in a child process."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
K = R = 128


def shipped_strip() -> int:
    """S of the product build: 256 << LAMD_BS_WB (rs_ff8_bs.hip)."""
    with open(os.path.join(REPO, "leopard_amd", "csrc", "rs_ff8_bs.hip")) as f:
        m = re.search(r"^#define LAMD_BS_WB (\d)", f.read(), re.M)
    assert m, "rs_ff8_bs.hip defines LAMD_BS_WB"
    return 256 << int(m.group(1))


def _roundtrip(leo, data, check):
    """data: (count, 128, b) uint8 on the GPU.  Encode as one batch, compare the
    objects in `check` with the oracle; full-loss decode, compare every object
    with its originals."""
    count, _, b = data.shape
    wc, dwc = leo.leo_encode_work_count(K, R), leo.leo_decode_work_count(K, R)
    works = torch.zeros((count, wc, b), dtype=torch.uint8, device="cuda")
    res = leo.leo_amd_encode_batch(b, K, R, wc, [[data[o, i].data_ptr() for i in range(K)] for o in range(count)],
                                   [[works[o, i].data_ptr() for i in range(wc)] for o in range(count)])
    assert res == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    for o in check:
        assert np.array_equal(works[o, :R].cpu().numpy(), ol.oracle().encode(data[o].cpu().numpy(), R)), (b, o)
    dworks = torch.zeros((count, dwc, b), dtype=torch.uint8, device="cuda")
    res = leo.leo_amd_decode_batch(b, K, R, dwc, [[None] * K] * count,
                                   [[works[o, i].data_ptr() for i in range(R)] for o in range(count)],
                                   [[dworks[o, i].data_ptr() for i in range(dwc)] for o in range(count)])
    assert res == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    for o in range(count):
        assert torch.equal(dworks[o, :K], data[o]), (b, o)


def _data(count, b):
    gen = torch.Generator(device="cuda").manual_seed(1000 * count + b)
    return torch.randint(0, 256, (count, K, b), dtype=torch.uint8, device="cuda", generator=gen)


def partial_strip_sizes(s):
    return [64, s - 64, s, s + 64, 2 * s + 192]


def run_partial_strips(leo, s, b):
    _roundtrip(leo, _data(3, b), range(3))


def run_static(leo, s):
    _roundtrip(leo, _data(1, s), range(1))  # one workgroup tile: fewer than 8 workgroups, no queue


def run_queue_first_round(leo, s):
    _roundtrip(leo, _data(9, s), range(9))  # 9 tiles: the queue, every workgroup's answer is "no more"


def run_queue_rounds(leo, s):
    """Pieces of 8 KiB + 64 (a last strip of 64 bytes) and enough objects that
    the tiles exceed the persistent grid by 8 per queue where 64 objects (one
    launch) allow: on 256 CUs, 64 objects = 576 tiles of 1 KiB on 512
    workgroups.  Encode and decode use the two counter sets in turn."""
    b = 8192 + 64
    strips = -(-b // s)
    waves = 8 * torch.cuda.get_device_properties(0).multi_processor_count  # 2 per SIMD
    slots = waves // (s // 256)  # workgroup tiles in the first round
    count = min(64, -(-(slots + 64) // strips))
    assert count >= 16
    step = (count - 1) / 15
    check = sorted({round(i * step) for i in range(16)})  # first, last and across the rounds
    assert len(check) == 16 and check[0] == 0 and check[-1] == count - 1
    _roundtrip(leo, _data(count, b), check)


def run_all(leo, s):
    for b in partial_strip_sizes(s):
        run_partial_strips(leo, s, b)
    run_static(leo, s)
    run_queue_first_round(leo, s)
    run_queue_rounds(leo, s)


@pytest.mark.parametrize("which", range(5))
def test_bs_waves_partial_strips(leo, which):
    """Case 1: 3 objects of 64, S - 64, S, S + 64, 2 S + 192 bytes a piece."""
    s = shipped_strip()
    run_partial_strips(leo, s, partial_strip_sizes(s)[which])


def test_bs_waves_static_assignment(leo):
    """Case 2: one object of S bytes a piece."""
    run_static(leo, shipped_strip())


def test_bs_waves_queue_first_round_only(leo):
    """Case 3: 9 objects of S bytes a piece."""
    run_queue_first_round(leo, shipped_strip())


def test_bs_waves_queue_rounds(leo):
    """Case 4: up to 64 objects of 8 KiB + 64 bytes a piece."""
    run_queue_rounds(leo, shipped_strip())


_FORCED = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import leopard_amd as leo, test_gpu_bs_waves as t
assert leo.leo_init() == 0
t.run_all(leo, {strip})
print("forced ok")
"""


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_bs_waves_forced_forms(waves):
    """Case 5: the experiment build (lib/exp, LAMD_EXPERIMENT_ENV) with
    LEO_AMD_FF8_BS_WAVES = 1, 2, 4 on the shapes of cases 1-4 for that tile's
    strip, in a child process each, so the tiles not shipped stay correct."""
    lib = os.path.join(REPO, "leopard_amd", "lib", "exp", "libleopard_amd.so")
    assert os.path.exists(lib), "make -C leopard_amd builds lib/exp"
    env = dict(os.environ, LEOPARD_AMD_LIB=lib, LEO_AMD_FF8_BS_WAVES=str(waves))
    p = subprocess.run([sys.executable, "-c", _FORCED.format(repo=REPO, tests=HERE, strip=256 * waves)], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0 and "forced ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
