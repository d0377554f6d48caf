"""bjxa_hip_encode_files: many WAV files -> XA files in one batched pass,
each byte-identical to what `bjxa encode --bits N` makes of it (the XA
header plus the oracle's encode; the reference's own SHA-1s for the golden
WAVs), with per-file status for refused inputs."""
import ctypes
import errno
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bjxa_amd
import oracle
from bjxa_amd import synth

FORMATS = [(8, 2), (6, 2), (4, 2), (8, 1), (6, 1), (4, 1)]
FRAMES = [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 32769,
          100003]
RATES = [8000, 22050, 44100]
CANARY = 0xC7


def wav_file(frames, ch, rate, seed):
    pcm = synth.pcm(frames, ch, seed=seed)
    return oracle.riff_header(ch, rate, pcm.nbytes) + pcm.tobytes(), pcm


def xa_file(pcm, frames, bits, ch, rate):
    xa = oracle.encode(pcm, frames, bits, ch)
    return bjxa_amd.xa_header(xa.size, frames, rate, bits, ch) + xa.tobytes()


def raw_encode_files(files, bits, out_sizes):
    """bjxa_hip_encode_files on canary-filled output buffers of the given
    sizes; returns (return value, statuses, output bytes)."""
    n = len(files)
    bufs = [ctypes.create_string_buffer(f, len(f)) for f in files]
    outs = [ctypes.create_string_buffer(bytes([CANARY]) * s, s) for s in out_sizes]
    wv = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
    wl = (ctypes.c_size_t * n)(*[len(f) for f in files])
    ba = (ctypes.c_uint8 * n)(*bits)
    xa = (ctypes.c_void_p * n)(*[ctypes.addressof(o) for o in outs])
    xl = (ctypes.c_size_t * n)(*out_sizes)
    st = (ctypes.c_int * n)()
    ret = bjxa_amd.lib().bjxa_hip_encode_files(wv, wl, ba, xa, xl, st, n)
    return ret, [int(s) for s in st], [o.raw for o in outs]


@pytest.mark.gpu
def test_encode_files_reference_sha1(built, golden, manifest):
    """The two golden WAVs at every width in one call: the reference
    encoder's own bytes."""
    names = ["square-mono.wav", "square-stereo.wav"]
    files = [golden(n) for n in names for _ in (4, 6, 8)]
    res = bjxa_amd.encode_files(files, [4, 6, 8] * 2)
    for k, (xa, st) in enumerate(res):
        assert st == 0
        assert hashlib.sha1(xa).hexdigest() == \
            manifest["encode"][names[k // 3]][str([4, 6, 8][k % 3])], k


@pytest.mark.gpu
def test_encode_files_good_and_broken(built):
    rng = np.random.default_rng(17)
    files, bits, want = [], [], []
    for i in range(30):
        b, ch = FORMATS[i % 6]
        frames = FRAMES[int(rng.integers(0, len(FRAMES)))]
        rate = RATES[i % 3]
        wav, pcm = wav_file(frames, ch, rate, 500 + i)
        files.append(wav)
        bits.append(b)
        want.append(xa_file(pcm, frames, b, ch, rate))
    sizes = [len(w) for w in want]
    status = [0] * 30
    wav, pcm = wav_file(5000, 2, 44100, 540)
    good = xa_file(pcm, 5000, 6, 2, 44100)

    def add(f, b, size, st, expect=None):
        files.append(f)
        bits.append(b)
        sizes.append(size)
        status.append(st)
        want.append(expect)

    add(b"RIFX" + wav[4:], 6, len(good), errno.EPROTO)
    add(wav[:40] + bytes(4) + wav[44:], 6, len(good), errno.EPROTO)    # data length 0
    add(wav[:-100], 6, len(good), errno.ENOBUFS)
    add(wav, 6, len(good) - 1, errno.ENOBUFS)
    add(wav, 5, len(good), errno.EINVAL)
    junk = bytes(rng.integers(0, 256, 1000, dtype=np.uint8))
    add(wav + junk, 6, len(good), 0, good)
    add(wav, 6, len(good), 0, good)

    ret, st, outs = raw_encode_files(files, bits, sizes)
    assert st == status
    assert ret == sum(s == 0 for s in status) == 32
    for k, (o, w) in enumerate(zip(outs, want)):
        if w is None:
            assert o == bytes([CANARY]) * len(o), k     # refused: untouched
        else:
            assert o == w, k
    # the same through the convenience wrapper: b"" for a refused file
    res = bjxa_amd.encode_files(files[30:], bits[30:])
    assert [s for _, s in res] == [errno.EPROTO, errno.EPROTO, errno.ENOBUFS, 0, errno.EINVAL,
                                   0, 0]
    assert [x for x, _ in res] == [b"", b"", b"", good, b"", good, good]


@pytest.mark.gpu
def test_encode_files_slab_cut(built):
    """About 70 MB of PCM, just over one 64 MiB staging slab: a file of odd
    size straddles the cut, the second slab is gathered while the first
    uploads, and every file is still exact."""
    files, want, bits = [], [], []
    total, i = 0, 0
    sizes = [1_234_567, 2_000_001, 987_653, 1_500_003]        # frames, stereo
    while total < 70_000_000:
        b, ch = FORMATS[i % 6]
        frames = sizes[i % 4] * (2 // ch) + i
        wav, pcm = wav_file(frames, ch, RATES[i % 3], 700 + i)
        files.append(wav)
        bits.append(b)
        want.append(xa_file(pcm, frames, b, ch, RATES[i % 3]))
        total += pcm.nbytes
        i += 1
    assert 64 << 20 < total < 80_000_000 and 10 <= len(files) <= 16
    # some file's PCM image [lo, hi) holds the cut
    pos, straddles = 0, 0
    for f in files:
        n = (len(f) - 44 + 15) & ~15
        straddles += pos < (64 << 20) < pos + n
        pos += n
    assert straddles == 1
    res = bjxa_amd.encode_files(files, bits)
    for k, ((xa, st), w) in enumerate(zip(res, want)):
        assert st == 0, k
        assert xa == w, k


@pytest.mark.gpu
def test_encode_files_round_trip(built):
    """decode_files(encode_files(wavs, 8)) gives the WAVs back with the low
    byte of every sample cleared."""
    wavs, want = [], []
    for i, frames in enumerate([1, 33, 4097, 8193, 32769, 100003]):
        ch = 1 + i % 2
        wav, pcm = wav_file(frames, ch, RATES[i % 3], 800 + i)
        wavs.append(wav)
        want.append(wav[:44] + (pcm & np.int16(-256)).tobytes())
    enc = bjxa_amd.encode_files(wavs, 8)
    assert [s for _, s in enc] == [0] * len(wavs)
    dec = bjxa_amd.decode_files([xa for xa, _ in enc])
    assert [s for _, s in dec] == [0] * len(wavs)
    assert [w for w, _ in dec] == want


HOST_PROBE = r"""
import errno, sys
sys.path.insert(0, sys.argv[1])
import bjxa_amd, oracle
good = oracle.riff_header(1, 8000, 64) + bytes(64)
res = bjxa_amd.encode_files([b"RIFX" + good[4:], good[:40], good[:-1], good,
                             good[:40] + bytes(4)], [8, 8, 8, 5, 8])
print([s for _, s in res], [x for x, _ in res] == [b""] * 5)
import ctypes
bad = ctypes.create_string_buffer(b"RIFX" + good[4:], len(good))
out = ctypes.create_string_buffer(65)
one = lambda t, v: (t * 1)(v)
print(bjxa_amd.lib().bjxa_hip_encode_files(
    one(ctypes.c_void_p, ctypes.addressof(bad)), one(ctypes.c_size_t, len(good)),
    one(ctypes.c_uint8, 8), one(ctypes.c_void_p, ctypes.addressof(out)),
    one(ctypes.c_size_t, 65), one(ctypes.c_int, -1), 1), out.raw == bytes(65))
try:
    bjxa_amd.encode_files([good, b"RIFX" + good[4:]], 4)
    print("no error")
except bjxa_amd.BjxaError as e:
    print(e.errno)
def err(streams):
    try:
        bjxa_amd.EncodeBatch(streams)
    except bjxa_amd.BjxaError as e:
        return e.errno
    return 0
ok = {"d_pcm": 0x10000, "d_xa": 0x20000, "frames": 3200, "bits": 8, "channels": 2}
res = [err([]), err([dict(ok, bits=5)]), err([dict(ok, channels=3)]),
       err([dict(ok, d_pcm=0x10008)]), err([dict(ok, d_xa=0x20002)]),
       err([ok, dict(ok, frames=0)]), err([dict(ok, d_pcm=0)]),
       err([ok, dict(ok, frames=32 << 32)]), err([ok, dict(ok, bits=4, channels=1, d_xa=0x30004)])]
print(" ".join(str(r) for r in res))
"""


def test_encode_files_host_checks(built):
    """Without a GPU: files refused by their headers get their errno, yield
    b"" and need no device; a batch with an encodable file fails with
    ENODEV; bjxa_hip_enc_batch_new validates every descriptor (EINVAL)
    before it needs the device (ENODEV)."""
    from conftest import ROOT
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", HOST_PROBE, ROOT], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    assert lines[0] == "%s True" % [errno.EPROTO, errno.ENOBUFS, errno.ENOBUFS, errno.EINVAL,
                                    errno.EPROTO]
    assert lines[1] == "0 True"        # every file refused: 0, nothing written, no device
    assert lines[2] == str(errno.ENODEV)
    assert [int(v) for v in lines[3].split()] == [errno.EINVAL] * 8 + [errno.ENODEV]
