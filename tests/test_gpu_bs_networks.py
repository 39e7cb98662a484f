"""The synthesized XOR networks of the bit-sliced tile on the GPU (rs_ff8_bs.hip,
gf8_net.h): 128 + 128 batches through leo_amd_encode_batch against the oracle
and leo_amd_decode_batch back to the originals, at the smallest shapes that run
every network: one object of 64-byte pieces (the one-wave tile, every twist),
one of 1024-byte pieces (one four-wave workgroup tile: every wave's code
variant, every layer, both directions) and three of 1088-byte pieces (whole and
partial strips).  Inputs: random bytes, and a basis input in which piece j holds
the single byte 1 << (j & 7) in column j (modulo the piece length) and zeros
elsewhere, so that a wrong gate shows as a wrong column of the code."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
K = R = 128
CASES = [(1, 64), (1, 1024), (3, 1088)]


def _random(count, b):
    rng = np.random.default_rng(77 * count + b)
    return rng.integers(0, 256, (count, K, b), dtype=np.uint8)


def _basis(count, b):
    data = np.zeros((count, K, b), dtype=np.uint8)
    for o in range(count):
        for j in range(K):
            data[o, j, (j + 41 * o) % b] = 1 << (j & 7)
    return data


@pytest.mark.parametrize("make", [_random, _basis], ids=["random", "basis"])
@pytest.mark.parametrize("count,b", CASES)
def test_bs_networks_encode_and_decode(leo, count, b, make):
    host = make(count, b)
    data = torch.from_numpy(host).to("cuda")
    wc, dwc = leo.leo_encode_work_count(K, R), leo.leo_decode_work_count(K, R)
    works = torch.zeros((count, wc, b), dtype=torch.uint8, device="cuda")
    res = leo.leo_amd_encode_batch(b, K, R, wc, [[data[o, i].data_ptr() for i in range(K)] for o in range(count)],
                                   [[works[o, i].data_ptr() for i in range(wc)] for o in range(count)])
    assert res == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    got = works[:, :R].cpu().numpy()
    for o in range(count):
        expect = ol.oracle().encode(host[o], R)
        wrong = np.argwhere(got[o] != expect)
        assert wrong.size == 0, f"object {o}: first wrong (piece, column) {wrong[:4].tolist()} of {len(wrong)}"
    dworks = torch.zeros((count, dwc, b), dtype=torch.uint8, device="cuda")
    res = leo.leo_amd_decode_batch(b, K, R, dwc, [[None] * K] * count,
                                   [[works[o, i].data_ptr() for i in range(R)] for o in range(count)],
                                   [[dworks[o, i].data_ptr() for i in range(dwc)] for o in range(count)])
    assert res == leo.LeopardResult.Success, leo.last_error()
    torch.cuda.synchronize()
    assert torch.equal(dworks[:, :K], data)
