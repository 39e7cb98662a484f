"""leo_amd_update against the alternative a caller had before it: a full
leo_encode of the same object.  One JSON line per shape.

usage: python tools/bench_update.py [K,R,B,C ...] [--iters N] [--rounds M]

Per shape, in one process: GPU time per call with HIP events on the call
stream (a spin kernel holds the stream while the host enqueues the calls, as
bench.run_shape), ROUNDS rounds that alternate ITERS updates and ITERS
encodes after a warm-up of both, over buffer sets rotated so that the bytes
the update touches exceed the 256 MiB MALL.  update_us is warm (columns
cached); update_cold_us comes from a fresh child process run with
LEO_AMD_UPDATE_CACHE_KB=0, where every call builds its columns again (one
64-byte encoder run and the table kernel in front of the update kernel).
hbm_frac = (2 R + C) B / update_us / 8 TB/s: the bytes the update must move
(R pieces read and written, C deltas read) over the HBM peak."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8e12
DEFAULT_SHAPES = ["128,128,65536,1", "1000,200,65536,1", "1000,200,65536,8", "32768,32768,65536,1"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cold-child", action="store_true", help="internal: time the update only, print {shape: us}")
    return ap.parse_args()


def measure(args, with_encode):
    import torch

    import leopard_amd as leo

    assert leo.leo_init() == 0, leo.last_error()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    leo.set_stream(s.cuda_stream)
    leo.set_async(True)
    lib = leo.lib
    vp = ctypes.c_void_p

    def ptrs(t, n):
        return (vp * n)(*[t[i].data_ptr() for i in range(n)])

    def timed(fn, n, nsets):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.synchronize()
        torch.cuda._sleep(20_000_000)
        a.record(s)
        for j in range(n):
            assert fn(j % nsets) == 0, leo.last_error()
        z.record(s)
        z.synchronize()
        return a.elapsed_time(z) * 1e3 / n  # us per call

    out = []
    for spec in args.shapes:
        k, r, b, c = (int(x) for x in spec.split(","))
        ewc = leo.leo_encode_work_count(k, r)
        touched = (2 * r + c) * b
        m = 1 << (r - 1).bit_length()
        field = "GF(2^8)" if 1 << (m + k - 1).bit_length() <= 256 else "GF(2^16)"
        set_bytes = ((k if with_encode else 0) + ewc + c) * b
        nsets = max(1, min(64, -(-(512 << 20) // touched), (24 << 30) // set_bytes))
        idx = [(i * (k - 1)) // max(c - 1, 1) for i in range(c)] if c > 1 else [k // 2]
        ci = (ctypes.c_uint * c)(*idx)
        sets = []
        for j in range(nsets):
            g = torch.Generator(device=dev).manual_seed(100 + j)
            work = torch.randint(0, 256, (ewc, b), dtype=torch.uint8, device=dev, generator=g)
            delta = torch.randint(0, 256, (c, b), dtype=torch.uint8, device=dev, generator=g)
            orig = torch.randint(0, 256, (k, b), dtype=torch.uint8, device=dev, generator=g) if with_encode else None
            sets.append((work, delta, orig, ptrs(work, ewc), ptrs(delta, c), ptrs(orig, k) if with_encode else None))

        def upd(j):
            return lib.leo_amd_update(b, k, r, c, ci, sets[j][4], sets[j][3])

        def enc(j):
            return lib.leo_encode(b, k, r, ewc, sets[j][5], sets[j][3])

        timed(upd, max(nsets, 5), nsets)  # warm-up of every set (and of the column cache)
        if with_encode:
            timed(enc, max(nsets, 5), nsets)
        tu, te = [], []
        for _ in range(args.rounds):
            tu.append(timed(upd, args.iters, nsets))
            if with_encode:
                te.append(timed(enc, args.iters, nsets))
        res = {"shape": f"{k}+{r} x {b} B", "changed": c, "field": field,
               "update_us": round(sum(tu) / len(tu), 2), "update_us_rounds": [round(x, 2) for x in tu],
               "buffer_sets": nsets, "timed_calls": args.iters * args.rounds}
        if with_encode:
            res["encode_us"] = round(sum(te) / len(te), 2)
            res["encode_us_rounds"] = [round(x, 2) for x in te]
            res["encode_over_update"] = round(res["encode_us"] / res["update_us"], 2)
        res["update_bytes"] = touched
        res["hbm_frac"] = round(touched / (res["update_us"] * 1e-6) / HBM_PEAK, 4)
        out.append((spec, res))
        del sets
        torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.cold_child:
        print(json.dumps({spec: res["update_us"] for spec, res in measure(args, False)}))
        return
    # the cold figures first, in a fresh child of their own (no cache: every call builds its columns)
    env = dict(os.environ, LEO_AMD_UPDATE_CACHE_KB="0")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--cold-child", "--iters", str(args.iters),
                            "--rounds", str(args.rounds)] + list(args.shapes), env=env, capture_output=True, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stdout + child.stderr)
        raise SystemExit("cold child failed")
    cold = json.loads(child.stdout.strip().splitlines()[-1])
    for spec, res in measure(args, True):
        res["update_cold_us"] = cold[spec]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
