"""Adaptive encode (bjxa_hip_encode_adaptive*, DESIGN.md §3 "Adaptive
encode"): what the search costs on the GPU and on one CPU core, where the
two routes of the host entry cross, and what it buys in squared error.  One
process, one GPU.

  kernel     bjxa_hip_encode_adaptive_async alone on C3-shaped PCM (5M
             stereo eblocks, device-resident), bits 4/6/8 at sync 64, a sync
             sweep (16/64/256) at 6 bits, and the profile-0
             bjxa_hip_encode_async on the same PCM for context; hipEvents,
             warm-up, medians of --repeats
  cpu        bjxa__cpu_encode_adaptive through the host entry (threshold at
             its maximum), one thread, on a 1/64 slice of that PCM
  host       the host entry end to end on 2M stereo eblocks, both routes
             (the CPU route at 6 bits only, once: it takes over a minute)
  crossover  both routes over eblocks 1..4096, stereo and mono, 6 bits; the
             first size from which the GPU route stays ahead
  quality    sum of squared error of decode(adaptive) over that of
             decode(reference encode) per test signal and bit depth (CPU
             only; --quality-only computes just this, no GPU needed)

usage: python tools/bench_encode_adaptive.py [--eblocks 5000000] [--repeats 9]
           [--host-eblocks 2000000] [--quality-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEVER = 2 ** 63 - 1


def median(v):
    return float(np.median(v))


def quality(bjxa_amd):
    """SSE(adaptive) / SSE(reference) per signal kind; 256 mono blocks each,
    sync 64, CPU route."""
    import oracle
    import xa_adaptive_model as model
    eb = 256
    n = np.arange(eb * 32)
    sig = model.kinds(n, np.random.default_rng(11)).astype(np.int16)
    old = bjxa_amd.offload_threshold(2, NEVER)
    rows = []
    try:
        for name, pcm in zip(model.KINDS, sig):
            pcm = np.ascontiguousarray(pcm)
            for bits in (4, 6, 8):
                xa = bjxa_amd.encode_adaptive(pcm, eb * 32, bits, 1, 64)
                ours = oracle.decode(xa, eb, bits, 1)[0].astype(np.int64)
                ref = oracle.decode(oracle.encode(pcm, eb * 32, bits, 1), eb, bits,
                                    1)[0].astype(np.int64)
                x = pcm.astype(np.int64)
                a, r = int(((x - ours) ** 2).sum()), int(((x - ref) ** 2).sum())
                rows.append({"signal": name, "bits": bits, "sse_adaptive": a,
                             "sse_reference": r,
                             "ratio": float("%.3g" % (a / r)) if r else None})
    finally:
        bjxa_amd.offload_threshold(2, old)
    return rows


def timed(torch, f, repeats, warm=2):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def kernel_alone(torch, bjxa_amd, eblocks, repeats):
    ch = 2
    frames = eblocks * 32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    pcm = torch.randint(-32768, 32768, (frames * ch,), dtype=torch.int16, device="cuda",
                        generator=gen)
    out = torch.zeros(eblocks * ch * 33, dtype=torch.uint8, device="cuda")
    sh = torch.cuda.current_stream().cuda_stream
    rows = []
    for bits, sync in [(4, 64), (6, 64), (8, 64), (6, 16), (6, 256)]:
        ms = timed(torch, lambda: bjxa_amd.encode_adaptive_device(
            pcm.data_ptr(), frames, bits, ch, out.data_ptr(), sync, sh), repeats)
        rows.append({"entry": "adaptive", "bits": bits, "sync": sync, "ms": round(median(ms), 4),
                     "ms_min": round(min(ms), 4),
                     "samples_per_s": round(frames * ch / median(ms) * 1e3)})
        print("kernel", rows[-1], flush=True)
    for bits in (4, 6, 8):
        ms = timed(torch, lambda: bjxa_amd.encode_device(
            pcm.data_ptr(), frames, bits, ch, out.data_ptr(), sh), repeats)
        rows.append({"entry": "profile0", "bits": bits, "ms": round(median(ms), 4),
                     "ms_min": round(min(ms), 4),
                     "samples_per_s": round(frames * ch / median(ms) * 1e3)})
        print("kernel", rows[-1], flush=True)
    # CPU baseline: 1/64 of the same PCM, one thread, and the same bytes
    sl = eblocks // 64
    host = pcm[:sl * 32 * ch].cpu().numpy()
    cpu = []
    old = bjxa_amd.offload_threshold(2, NEVER)
    try:
        for bits in (4, 6, 8):
            t0 = time.perf_counter()
            xa = bjxa_amd.encode_adaptive(host, sl * 32, bits, ch, 64)
            dt = time.perf_counter() - t0
            bjxa_amd.encode_adaptive_device(pcm.data_ptr(), sl * 32, bits, ch, out.data_ptr(),
                                            64, sh)
            torch.cuda.synchronize()
            same = bool(np.array_equal(out[:xa.size].cpu().numpy(), xa))
            cpu.append({"bits": bits, "eblocks": sl, "s": round(dt, 4),
                        "samples_per_s": round(sl * 32 * ch / dt), "gpu_bytes_equal": same})
            print("cpu", cpu[-1], flush=True)
    finally:
        bjxa_amd.offload_threshold(2, old)
    return rows, cpu


def host_entry(bjxa_amd, eblocks):
    ch = 2
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32768, eblocks * 32 * ch, dtype=np.int16)
    rows = []
    old = bjxa_amd.offload_threshold(2, 0)
    try:
        ref = None
        for bits in (4, 6, 8):
            ts = []
            for _ in range(4):
                t0 = time.perf_counter()
                xa = bjxa_amd.encode_adaptive(pcm, eblocks * 32, bits, ch, 64)
                ts.append(time.perf_counter() - t0)
            if bits == 6:
                ref = xa
            rows.append({"route": "gpu", "bits": bits, "eblocks": eblocks,
                         "first_s": round(ts[0], 4), "s": round(median(ts[1:]), 4)})
            print("host", rows[-1], flush=True)
        bjxa_amd.offload_threshold(2, NEVER)
        t0 = time.perf_counter()
        xa = bjxa_amd.encode_adaptive(pcm, eblocks * 32, 6, ch, 64)
        dt = time.perf_counter() - t0
        rows.append({"route": "cpu", "bits": 6, "eblocks": eblocks, "s": round(dt, 4),
                     "routes_equal": bool(np.array_equal(xa, ref))})
        print("host", rows[-1], flush=True)
    finally:
        bjxa_amd.offload_threshold(2, old)
    return rows


def crossover(bjxa_amd):
    rng = np.random.default_rng(9)
    res = {}
    old = bjxa_amd.offload_threshold(2)
    try:
        for ch in (2, 1):
            rows = []
            for eb in [1 << k for k in range(13)]:
                pcm = rng.integers(-32768, 32768, eb * 32 * ch, dtype=np.int16)
                t = {}
                for route, thr in (("gpu", 0), ("cpu", NEVER)):
                    bjxa_amd.offload_threshold(2, thr)
                    ts = []
                    for _ in range(12):
                        t0 = time.perf_counter()
                        bjxa_amd.encode_adaptive(pcm, eb * 32, 6, ch, 64)
                        ts.append(time.perf_counter() - t0)
                    t[route] = median(ts[2:])
                rows.append({"eblocks": eb, "gpu_us": round(t["gpu"] * 1e6, 1),
                             "cpu_us": round(t["cpu"] * 1e6, 1)})
            ahead = [r["eblocks"] for r in rows if r["gpu_us"] < r["cpu_us"]]
            behind = [r["eblocks"] for r in rows if r["gpu_us"] >= r["cpu_us"]]
            first = min(e for e in ahead if not behind or e > max(behind)) if ahead else None
            res["stereo" if ch == 2 else "mono"] = {"rows": rows, "gpu_ahead_from": first}
            print("crossover", ch, first, flush=True)
    finally:
        bjxa_amd.offload_threshold(2, old)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eblocks", type=int, default=5_000_000)
    ap.add_argument("--host-eblocks", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_adaptive.json"))
    args = ap.parse_args()
    if args.quality_only:
        import bjxa_amd
        res = {"quality": quality(bjxa_amd)}
    else:
        import torch
        import bjxa_amd
        if not torch.cuda.is_available():
            sys.exit("bench_encode_adaptive: no GPU (use --quality-only without one)")
        res = {"device": torch.cuda.get_device_name(0), "library": bjxa_amd.version(),
               "threshold_default": bjxa_amd.offload_threshold(2),
               "eblocks": args.eblocks, "channels": 2, "repeats": args.repeats}
        res["kernel"], res["cpu_core"] = kernel_alone(torch, bjxa_amd, args.eblocks,
                                                      args.repeats)
        torch.cuda.empty_cache()
        res["crossover"] = crossover(bjxa_amd)
        res["host_entry"] = host_entry(bjxa_amd, args.host_eblocks)
        res["quality"] = quality(bjxa_amd)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
