"""leo_amd_repair against the route a caller had before it: leo_decode for the
lost originals, then a full leo_encode into scratch for the lost recovery
pieces (the encode alone when no original is lost).  One JSON line per shape.

usage: python tools/bench_repair.py [K,R,B,LOST_ORIG,LOST_REC[,OBJECTS] ...] [--iters N] [--rounds M]

Per shape, in one process: GPU time per call with HIP events on the call
stream (a spin kernel holds the stream while the host enqueues the calls, as
bench.run_shape), every route warmed over every buffer set first, then ROUNDS
rounds that alternate ITERS repairs and ITERS runs of the old route, over
buffer sets rotated so that the bytes a call touches exceed the 256 MiB MALL.
compose_us is the same repair call in a fresh child process run with
LEO_AMD_REPAIR_COMPOSE=1 (the switch is read once per process), fused_us in
one run with LEO_AMD_REPAIR_COMPOSE=0 on the experiment build
(lib/exp/libleopard_amd.so), which keeps every call on the fused routes:
repair_us, the shipped dispatch, should be the smaller of the two.  With OBJECTS
> 1 the calls are leo_amd_repair_batch against leo_amd_decode_batch +
leo_amd_encode_batch, and the times are per batch.
bytes = (received + rebuilt pieces) x B: what a repair must read and write;
hbm_frac = bytes / repair_us / 8 TB/s."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK = 8e12
DEFAULT_SHAPES = ["128,128,65536,32,32", "128,128,65536,0,64", "100,10,2560,4,6", "1000,200,65536,100,100",
                  "1000,200,2560,100,100", "32768,32768,65536,16384,16384", "128,128,65536,32,32,64"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=DEFAULT_SHAPES)
    ap.add_argument("--iters", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--child", action="store_true", help="internal: time the repair only, print {shape: us}")
    return ap.parse_args()


def measure(args, with_old_route):
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

    def arr(ptrs):
        return (vp * max(len(ptrs), 1))(*ptrs)

    def outer(arrs):
        return (pp * len(arrs))(*[ctypes.cast(a, pp) for a in arrs])

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
        f = [int(x) for x in spec.split(",")]
        k, r, b, nlo, nlr = f[:5]
        nobj = f[5] if len(f) > 5 else 1
        ewc, dwc = leo.leo_encode_work_count(k, r), leo.leo_decode_work_count(k, r)
        m = 1 << (r - 1).bit_length()
        field = "GF(2^8)" if 1 << (m + k - 1).bit_length() <= 256 else "GF(2^16)"
        # evenly spread losses (the same pattern in every set: the decoder state is cached, as in a rebuild)
        lo = [(i * k) // nlo for i in range(nlo)]
        lr = [(j * r) // nlr for j in range(nlr)]
        los, lrs = set(lo), set(lr)
        touched = (k + r) * b * nobj  # received pieces read, lost ones written
        obj_bytes = (k + 2 * r + nlo + nlr) * b
        nsets = max(1, min(64, -(-(512 << 20) // touched), (40 << 30) // (obj_bytes * nobj)))
        sets = []
        for j in range(nsets):
            objs = []
            for o in range(nobj):
                g = torch.Generator(device=dev).manual_seed(1000 * j + o)
                orig = torch.randint(0, 256, (k, b), dtype=torch.uint8, device=dev, generator=g)
                rec = leo.encode(orig, r)[:r].clone()  # a codeword
                out_o = torch.empty((max(nlo, 1), b), dtype=torch.uint8, device=dev)
                out_r = torch.empty((max(nlr, 1), b), dtype=torch.uint8, device=dev)
                scratch = torch.empty((r, b), dtype=torch.uint8, device=dev) if with_old_route else None
                p_orig = [None if i in los else orig[i].data_ptr() for i in range(k)]
                p_rec = [None if i in lrs else rec[i].data_ptr() for i in range(r)]
                p_work = [None] * dwc
                for n, i in enumerate(lo):
                    p_work[i] = out_o[n].data_ptr()
                p_rout = [None] * r
                for n, i in enumerate(lr):
                    p_rout[i] = out_r[n].data_ptr()
                p_full = [p_orig[i] if p_orig[i] is not None else p_work[i] for i in range(k)]
                p_enc = ([scratch[i].data_ptr() for i in range(r)] + [None] * (ewc - r)) if with_old_route else []
                objs.append(dict(keep=(orig, rec, out_o, out_r, scratch), orig=arr(p_orig), rec=arr(p_rec),
                                 work=arr(p_work), rout=arr(p_rout), full=arr(p_full), enc=arr(p_enc)))
            st = dict(objs=objs)
            if nobj > 1:
                for name in ("orig", "rec", "work", "rout", "full", "enc"):
                    st[name] = outer([o[name] for o in objs])
            sets.append(st)
        torch.cuda.synchronize()

        if nobj == 1:
            def rep(j):
                o = sets[j]["objs"][0]
                return lib.leo_amd_repair(b, k, r, dwc, o["orig"], o["rec"], o["work"], o["rout"])

            def old(j):
                o = sets[j]["objs"][0]
                res = lib.leo_decode(b, k, r, dwc, o["orig"], o["rec"], o["work"]) if nlo else 0
                return res or lib.leo_encode(b, k, r, ewc, o["full"], o["enc"])
        else:
            def rep(j):
                t = sets[j]
                return lib.leo_amd_repair_batch(nobj, b, k, r, dwc, t["orig"], t["rec"], t["work"], t["rout"])

            def old(j):
                t = sets[j]
                res = lib.leo_amd_decode_batch(nobj, b, k, r, dwc, t["orig"], t["rec"], t["work"]) if nlo else 0
                return res or lib.leo_amd_encode_batch(nobj, b, k, r, ewc, t["full"], t["enc"])

        timed(rep, max(nsets, 5), nsets)  # warm-up of every set and of the cached decoder state
        if with_old_route:
            timed(old, max(nsets, 5), nsets)
        tr, to = [], []
        for _ in range(args.rounds):
            tr.append(timed(rep, args.iters, nsets))
            if with_old_route:
                to.append(timed(old, args.iters, nsets))
        res = {"shape": f"{k}+{r} x {b} B", "lost": [nlo, nlr], "objects": nobj, "field": field,
               "repair_us": round(sum(tr) / len(tr), 2), "repair_us_rounds": [round(x, 2) for x in tr],
               "buffer_sets": nsets, "timed_calls": args.iters * args.rounds}
        if with_old_route:
            res["old_route"] = ("decode + encode" if nlo else "encode") + (" (batch calls)" if nobj > 1 else "")
            res["old_us"] = round(sum(to) / len(to), 2)
            res["old_us_rounds"] = [round(x, 2) for x in to]
            res["old_over_repair"] = round(res["old_us"] / res["repair_us"], 2)
        res["bytes"] = touched
        res["hbm_frac"] = round(touched / (res["repair_us"] * 1e-6) / HBM_PEAK, 4)
        out.append((spec, res))
        del sets
        torch.cuda.empty_cache()
    return out


def main():
    args = parse()
    if args.child:
        print(json.dumps({spec: res["repair_us"] for spec, res in measure(args, False)}))
        return
    # the forced routes first, each in a fresh child of its own
    forced = {}
    exp_lib = os.path.join(REPO, "leopard_amd", "lib", "exp", "libleopard_amd.so")
    for name, extra in (("compose", {"LEO_AMD_REPAIR_COMPOSE": "1"}),
                        ("fused", {"LEO_AMD_REPAIR_COMPOSE": "0", "LEOPARD_AMD_LIB": exp_lib})):
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(args.iters),
                                "--rounds", str(args.rounds)] + list(args.shapes), env=dict(os.environ, **extra),
                               capture_output=True, text=True)
        if child.returncode != 0:
            sys.stderr.write(child.stdout + child.stderr)
            raise SystemExit(f"{name} child failed")
        forced[name] = json.loads(child.stdout.strip().splitlines()[-1])
    for spec, res in measure(args, True):
        res["compose_us"] = forced["compose"][spec]
        res["fused_us"] = forced["fused"][spec]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
