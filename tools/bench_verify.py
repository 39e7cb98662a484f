"""leo_amd_verify: the fused routes against the composition a caller had before
(the encoder into scratch, then a compare) and against the plain encoder of the
same shape.  One JSON line per shape.

usage: python tools/bench_verify.py [K,R,B[,OBJECTS] ...] [--iters N] [--rounds M]

Per shape, in one process on the experiment build (lib/exp/libleopard_amd.so,
whose leo_amd_exp_verify_route switches the route between calls): every route
warmed over every buffer set, then ROUNDS rounds that alternate ITERS fused
verifies, ITERS forced-composed verifies and ITERS leo_encode calls
(leo_amd_encode_batch with OBJECTS > 1), over buffer sets rotated so that the
bytes a call touches exceed the 256 MiB MALL.  A verify call returns only when
its report is in host memory, so calls cannot be queued behind each other: each
call is timed with a pair of HIP events of its own on the call stream (clear of
the report, kernels, read-back of the report; for the encoder its kernels), and
the figure is the mean over a round's calls; *_rounds are the rounds' means,
wall_us the host time per verify call (launch, synchronisation and read-back
latency included).  shipped_us is the product library's own dispatch, timed the
same way in the parent process.
bytes = (K + R) x B x OBJECTS: what a scrub must read; hbm_frac = bytes /
fused_us / 8 TB/s.  Every stripe is clean: the verdict is asserted to be zero."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8e12
DEFAULT_SHAPES = ["128,128,65536", "128,128,65536,64", "128,128,1048576", "100,10,2560", "1000,200,65536",
                  "1000,200,2560", "32768,32768,65536"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help="internal: the alternating rounds on the experiment build")
    return ap.parse_args()


def measure(args, alternate):
    import torch

    import leopard_amd as leo

    assert leo.leo_init() == 0, leo.last_error()
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev)
    leo.set_stream(s.cuda_stream)
    leo.set_async(True)
    lib = leo.lib
    vp = ctypes.c_void_p
    pp = ctypes.POINTER(vp)
    if alternate:
        lib.leo_amd_exp_verify_route.argtypes = [ctypes.c_int]
        lib.leo_amd_exp_verify_route.restype = None

    def arr(ptrs):
        return (vp * max(len(ptrs), 1))(*ptrs)

    def outer(arrs):
        return (pp * len(arrs))(*[ctypes.cast(a, pp) for a in arrs])

    def timed(fn, n, nsets):
        """Mean GPU time (event pair per call) and mean host time per call, us."""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        s.synchronize()
        t0 = time.perf_counter()
        for j in range(n):
            ev[j][0].record(s)
            assert fn(j % nsets) == 0, leo.last_error()
            ev[j][1].record(s)
        s.synchronize()
        wall = (time.perf_counter() - t0) * 1e6 / n
        return sum(a.elapsed_time(z) for a, z in ev) * 1e3 / n, wall

    out = []
    for spec in args.shapes:
        f = [int(x) for x in spec.split(",")]
        k, r, b = f[:3]
        nobj = f[3] if len(f) > 3 else 1
        ewc = leo.leo_encode_work_count(k, r)
        m = 1 << (r - 1).bit_length()
        field = "GF(2^8)" if 1 << (m + k - 1).bit_length() <= 256 else "GF(2^16)"
        touched = (k + r) * b * nobj
        obj_bytes = (k + 2 * r) * b
        nsets = max(1, min(64, -(-(512 << 20) // touched), (24 << 30) // (obj_bytes * nobj)))
        words = (r + 31) // 32
        bitmap = (ctypes.c_uint32 * (words * nobj))()
        counts = (ctypes.c_uint * nobj)()
        sets = []
        for j in range(nsets):
            objs = []
            for o in range(nobj):
                g = torch.Generator(device=dev).manual_seed(1000 * j + o)
                orig = torch.randint(0, 256, (k, b), dtype=torch.uint8, device=dev, generator=g)
                rec = leo.encode(orig, r)[:r].clone()  # a codeword
                scratch = torch.empty((r, b), dtype=torch.uint8, device=dev)
                objs.append(dict(keep=(orig, rec, scratch), orig=arr([orig[i].data_ptr() for i in range(k)]),
                                 rec=arr([rec[i].data_ptr() for i in range(r)]),
                                 enc=arr([scratch[i].data_ptr() for i in range(r)] + [None] * (ewc - r))))
            st = dict(objs=objs)
            if nobj > 1:
                for name in ("orig", "rec", "enc"):
                    st[name] = outer([o[name] for o in objs])
            sets.append(st)
        torch.cuda.synchronize()

        def clean():
            return all(c == 0 for c in counts) and not any(bitmap)

        if nobj == 1:
            def ver(j):
                o = sets[j]["objs"][0]
                res = lib.leo_amd_verify(b, k, r, o["orig"], o["rec"], bitmap, counts)
                return res or (0 if clean() else 99)

            def enc(j):
                o = sets[j]["objs"][0]
                return lib.leo_encode(b, k, r, ewc, o["orig"], o["enc"])
        else:
            def ver(j):
                t = sets[j]
                res = lib.leo_amd_verify_batch(nobj, b, k, r, t["orig"], t["rec"], bitmap, counts)
                return res or (0 if clean() else 99)

            def enc(j):
                t = sets[j]
                return lib.leo_amd_encode_batch(nobj, b, k, r, ewc, t["orig"], t["enc"])

        def route(which):
            if alternate:
                lib.leo_amd_exp_verify_route(which)

        res = {"shape": f"{k}+{r} x {b} B", "objects": nobj, "field": field, "bytes": touched, "buffer_sets": nsets,
               "timed_calls_per_route": args.iters * args.rounds}
        routes = [("fused", 0), ("composed", 1)] if alternate else [("shipped", -1)]
        for _, which in routes:  # warm-up of every route over every set
            route(which)
            timed(ver, max(nsets, 3), nsets)
        timed(enc, max(nsets, 3), nsets)
        rounds = {name: [] for name, _ in routes}
        walls = {name: [] for name, _ in routes}
        rounds["encode"] = []
        for _ in range(args.rounds):
            for name, which in routes:
                route(which)
                g, w = timed(ver, args.iters, nsets)
                rounds[name].append(g)
                walls[name].append(w)
            rounds["encode"].append(timed(enc, args.iters, nsets)[0])
        route(-1)
        for name, v in rounds.items():
            res[name + "_us"] = round(sum(v) / len(v), 2)
            res[name + "_us_rounds"] = [round(x, 2) for x in v]
        for name, v in walls.items():
            res[name + "_wall_us"] = round(sum(v) / len(v), 2)
        out.append((spec, res))
        del sets
        torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.child:
        print(json.dumps({spec: res for spec, res in measure(args, True)}))
        return
    exp_lib = os.path.join(REPO, "leopard_amd", "lib", "exp", "libleopard_amd.so")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters),
                            "--rounds", str(args.rounds)] + list(args.shapes),
                           env=dict(os.environ, LEOPARD_AMD_LIB=exp_lib), capture_output=True, text=True)
    if child.returncode != 0:
        sys.stderr.write(child.stdout + child.stderr)
        raise SystemExit("the experiment-build child failed")
    alt = json.loads(child.stdout.strip().splitlines()[-1])
    for spec, shipped in measure(args, False):
        res = alt[spec]
        res["shipped_us"] = shipped["shipped_us"]
        res["shipped_us_rounds"] = shipped["shipped_us_rounds"]
        res["shipped_wall_us"] = shipped["shipped_wall_us"]
        res["encode_us_product"] = shipped["encode_us"]
        res["composed_over_fused"] = round(res["composed_us"] / res["fused_us"], 3)
        res["fused_over_encode"] = round(res["fused_us"] / res["encode_us"], 3)
        res["hbm_frac"] = round(res["bytes"] / (res["fused_us"] * 1e-6) / HBM_PEAK, 4)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
