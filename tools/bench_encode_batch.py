"""Batched encode A/B (bjxa_hip_enc_batch_*, bjxa_hip_encode_files) on the
shapes of bench.py's C5 and C4 batch configurations, one process, one GPU.

Part 1, device-resident PCM, arms interleaved, hipEvents around each arm,
medians of --repeats runs:
  A  n bjxa_hip_encode_async calls back to back on one stream (one launch
     per stream: what a caller has without the batch entry point)
  B  one EncodeBatch.encode() (one launch)
  C  one bjxa_hip_encode_async over a single stream of the same total PCM
     and format (C5 shape only): the streaming ceiling
The three arms read the same PCM image; A and B must leave identical XA
images, and on the C5 shape C's as well.

Part 2, files: n C5-shaped WAV files in host memory through
bjxa_hip_encode_files against a loop of bjxa_amd.encode_wav (bjxa_encode
per file, default offload threshold), with the PCIe-bound estimate (all
bytes moved over ~56 GB/s, csrc/xa_files.hip).

usage: python tools/bench_encode_batch.py [--streams 1024] [--repeats 20]
           [--files 1024] [--no-files] [--commit HASH] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import bjxa_amd  # noqa: E402
import oracle  # noqa: E402
from bench import batch_specs  # noqa: E402

PCIE_GBS = 56.0


def xa_len(eb, bits, ch):
    return eb * ch * (bits * 4 + 1)


def median(v):
    return float(np.median(v))


def device_ab(name, nstreams, repeats, dev):
    """Arms A, B (and C on the C5 shape) over `name`'s streams."""
    specs = batch_specs(name, nstreams)
    sh = torch.cuda.current_stream(dev).cuda_stream
    ioff, ooff, ipos, opos = [], [], 0, 0
    for bits, ch, eb in specs:
        ioff.append(ipos)
        ipos += eb * 64 * ch                     # a multiple of 16
        ooff.append(opos)
        opos += (xa_len(eb, bits, ch) + 15) & ~15
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    pcm = torch.randint(-32768, 32768, (ipos // 2,), dtype=torch.int16, device=dev,
                        generator=gen)
    out = {k: torch.zeros(opos, dtype=torch.uint8, device=dev) for k in "AB"}
    lib = bjxa_amd.lib()
    calls = [(pcm.data_ptr() + i, eb * 32, bits, ch, o)
             for (bits, ch, eb), i, o in zip(specs, ioff, ooff)]

    def arm_a():
        base = out["A"].data_ptr()
        for p, frames, bits, ch, o in calls:
            if lib.bjxa_hip_encode_async(p, frames, bits, ch, base + o, sh) != 0:
                raise RuntimeError("bjxa_hip_encode_async failed")

    batch = bjxa_amd.EncodeBatch(
        [{"d_pcm": p, "d_xa": out["B"].data_ptr() + o, "frames": f, "bits": b, "channels": c}
         for p, f, b, c, o in calls], sh)
    arms = {"A": arm_a, "B": lambda: batch.encode(sh)}
    uniform = len(set((b, c) for b, c, _ in specs)) == 1
    if uniform:
        bits, ch, _ = specs[0]
        frames = ipos // (2 * ch)
        out["C"] = torch.zeros(xa_len(frames // 32, bits, ch), dtype=torch.uint8, device=dev)
        arms["C"] = lambda: bjxa_amd.encode_device(pcm.data_ptr(), frames, bits, ch,
                                                   out["C"].data_ptr(), sh)
    for f in arms.values():                      # warm-up
        f()
        f()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    for _ in range(repeats):
        for k, f in arms.items():                # interleaved
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ms[k].append(e0.elapsed_time(e1))
    same = bool(torch.equal(out["A"], out["B"]))
    if uniform:
        # whole-block streams: the single stream's XA is the streams' XA in a row
        n0 = xa_len(specs[0][2], *specs[0][:2])
        packed = torch.cat([out["B"][o:o + n0] for o in ooff])
        same = same and bool(torch.equal(packed, out["C"]))
    # three streams against the oracle
    exact = True
    for k in (0, len(specs) // 2, len(specs) - 1):
        bits, ch, eb = specs[k]
        p = pcm[ioff[k] // 2: ioff[k] // 2 + eb * 32 * ch].cpu().numpy()
        got = out["B"][ooff[k]: ooff[k] + xa_len(eb, bits, ch)].cpu().numpy()
        exact = exact and bool(np.array_equal(got, oracle.encode(p, eb * 32, bits, ch)))
    batch.close()
    alg = ipos + sum(xa_len(eb, b, c) for b, c, eb in specs)
    res = {"shape": name, "streams": len(specs), "pcm_bytes": ipos, "alg_bytes": alg,
           "repeats": repeats, "arms_agree": same, "oracle_exact": exact}
    for k in arms:
        res["%s_ms" % k] = round(median(ms[k]), 4)
        res["%s_ms_min" % k] = round(min(ms[k]), 4)
        res["%s_wall_ms" % k] = round(median(wall[k]), 4)
        res["%s_GBs" % k] = round(alg / median(ms[k]) / 1e6, 1)
    res["B_over_A"] = round(res["B_ms"] / res["A_ms"], 4)
    if uniform:
        res["B_over_C"] = round(res["B_ms"] / res["C_ms"], 4)
    return res


def files_ab(nfiles, repeats):
    """bjxa_hip_encode_files against a loop of encode_wav, C5-shaped files."""
    bits, ch, eb = batch_specs("C5", nfiles)[0]
    data_len = eb * 64 * ch
    wlen, xlen = 44 + data_len, 32 + xa_len(eb, bits, ch)
    rng = np.random.default_rng(9)
    base = rng.integers(0, 65536, data_len // 2, dtype=np.uint16)
    hdr = np.frombuffer(oracle.riff_header(ch, 44100, data_len), np.uint8)
    wavs = np.empty((nfiles, wlen), dtype=np.uint8)
    for i in range(nfiles):
        wavs[i, :44] = hdr
        wavs[i, 44:] = (base ^ np.uint16(i * 257 & 0xFFFF)).view(np.uint8)
    xas = np.zeros((nfiles, xlen), dtype=np.uint8)       # pages touched
    wv = (ctypes.c_void_p * nfiles)(*[wavs[i].ctypes.data for i in range(nfiles)])
    wl = (ctypes.c_size_t * nfiles)(*[wlen] * nfiles)
    ba = (ctypes.c_uint8 * nfiles)(*[bits] * nfiles)
    xa = (ctypes.c_void_p * nfiles)(*[xas[i].ctypes.data for i in range(nfiles)])
    xl = (ctypes.c_size_t * nfiles)(*[xlen] * nfiles)
    st = (ctypes.c_int * nfiles)()
    lib = bjxa_amd.lib()
    t_files = []
    for _ in range(repeats + 1):                 # the first call sets the context up
        t0 = time.perf_counter()
        r = lib.bjxa_hip_encode_files(wv, wl, ba, xa, xl, st, nfiles)
        t_files.append(time.perf_counter() - t0)
        if r != nfiles:
            raise RuntimeError("bjxa_hip_encode_files: %d of %d" % (r, nfiles))
    t_loop, exact = [], True
    for rep in range(repeats):
        t0 = time.perf_counter()
        for i in range(nfiles):
            one = bjxa_amd.encode_wav(wavs[i].data, bits)
            if rep == 0 and i % 97 == 0:
                exact = exact and one == xas[i].tobytes()
        t_loop.append(time.perf_counter() - t0)
    moved = nfiles * (data_len + xa_len(eb, bits, ch))
    return {"shape": "C5 files", "files": nfiles, "wav_bytes": nfiles * wlen,
            "xa_bytes": nfiles * xlen, "repeats": repeats,
            "encode_files_first_s": round(t_files[0], 4),
            "encode_files_s": round(median(t_files[1:]), 4),
            "encode_wav_loop_s": round(median(t_loop), 4),
            "pcie_bound_s": round(moved / (PCIE_GBS * 1e9), 4),
            "loop_matches_files": exact}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--files", type=int, default=1024)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--commit", default=None, help="recorded in the result")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"commit": args.commit, "device": torch.cuda.get_device_name(dev),
           "library": bjxa_amd.version(),
           "device_resident": [device_ab(n, args.streams, args.repeats, dev)
                               for n in ("C5", "C4")]}
    torch.cuda.empty_cache()
    if not args.no_files:
        res["files"] = files_ab(args.files, args.file_repeats)
    text = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
