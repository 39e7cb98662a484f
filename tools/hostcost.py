#!/usr/bin/env python3
"""Host cost per single-object call (device pointers, async): calls queued
behind a spin kernel, so the GPU never back-pressures the host.  leo_amd_verify
returns its report, so it synchronises: its figure is the latency of a call on
an idle GPU (no spin kernel in front)."""
import ctypes
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import leopard_amd as leo  # noqa: E402
from bench import Sets, ptrs  # noqa: E402


def main():
    k, r, b = 128, 128, 65536
    assert leo.leo_init() == 0
    leo.set_async(True)
    st = torch.cuda.current_stream()
    leo.set_stream(st.cuda_stream)
    sets = Sets(leo, torch, k, r, b, 16, "cuda")
    lib = leo.lib
    enc = lambda i: lib.leo_encode(b, k, r, sets.enc_wc, sets.p_orig[i], sets.p_encw[i])
    dec = lambda i: lib.leo_decode(b, k, r, sets.dec_wc, sets.p_null[i], sets.p_rec[i], sets.p_decw[i])
    nop = lambda i: lib.leo_encode_work_count(k, r)
    setst = lambda i: leo.set_stream(st.cuda_stream)
    # update: one changed original; repair: 32 originals and 32 recovery pieces lost, all rebuilt
    one = (ctypes.c_uint * 1)(5)
    lo, lr = range(32), range(r - 32, r)
    p_olost = [ptrs(o, lost=lo) for o in sets.orig]
    p_rlost = [ptrs(w, r, lost=lr) for w in sets.enc_work]
    words, count = (ctypes.c_uint32 * ((r + 31) // 32))(), ctypes.c_uint()
    upd = lambda i: lib.leo_amd_update(b, k, r, 1, one, sets.p_orig[i], sets.p_rec[i])
    rep = lambda i: lib.leo_amd_repair(b, k, r, sets.dec_wc, p_olost[i], p_rlost[i], sets.p_decw[i], sets.p_rec[i])
    ver = lambda i: lib.leo_amd_verify(b, k, r, sets.p_orig[i], sets.p_rec[i], words, ctypes.byref(count))
    for name, fn in [("work_count (ctypes floor)", nop), ("set_stream", setst), ("encode", enc), ("decode", dec),
                     ("update", upd), ("repair", rep), ("verify (synchronises)", ver)]:
        for j in range(20):
            assert not fn(j % 16) or fn in (nop, setst)
        torch.cuda.synchronize()
        if fn is not ver:
            torch.cuda._sleep(200_000_000)
        n = 200
        t0 = time.perf_counter()
        for j in range(n):
            fn(j % 16)
        dt = (time.perf_counter() - t0) / n
        torch.cuda.synchronize()
        print(f"{name:28s} {dt * 1e6:7.2f} us/call", flush=True)


if __name__ == "__main__":
    main()
