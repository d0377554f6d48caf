"""Batched encode (bjxa_hip_enc_batch_*): many PCM streams of mixed formats
per launch, each byte-exact against the oracle's encode (src/libbjxa.c:
665-691, 759-819 per stream), with every boundary the stream's own: nothing
written outside a stream's XA, nothing taken from a neighbour's PCM."""
import numpy as np
import pytest

import bjxa_amd
import oracle
from bjxa_amd import synth
from gpu_util import dev_encode, require_gpu

pytestmark = pytest.mark.gpu

FORMATS = [(8, 2), (6, 2), (4, 2), (8, 1), (6, 1), (4, 1)]
# edges of one lane (4/ch eblocks), of one wave (4,096 stereo or 8,192 mono
# frames) and of one workgroup (four waves); 100003 spans several workgroups
FRAMES = [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 32769,
          100003]

_cache = {}


def stream(frames, bits, ch, seed):
    """(pcm int16, expected XA uint8) of one stream, computed once."""
    key = (frames, bits, ch, seed)
    if key not in _cache:
        pcm = synth.pcm(frames, ch, seed=seed)
        xa = oracle.encode(pcm, frames, bits, ch)
        pcm.setflags(write=False)
        xa.setflags(write=False)
        _cache[key] = (pcm, xa)
    return _cache[key]


def mixed_specs():
    """60 streams: every length with several formats, every format."""
    specs = [(FRAMES[i % 16], *FORMATS[(i + i // 16) % 6], 200 + i) for i in range(60)]
    assert {(b, c) for _, b, c, _ in specs} == set(FORMATS)
    return specs


def xa_len(frames, bits, ch):
    return (frames + 31) // 32 * ch * (bits * 4 + 1)


def run_packed(specs, align, repeat=1):
    """Encode `specs` (frames, bits, ch, seed) with every PCM input carved
    from one buffer at 16-byte aligned offsets, the slack filled with 0x7F7F
    samples, and every XA output carved from one 0xA5-filled buffer at the
    previous stream's end rounded up to `align` bytes.  Checks every stream
    against the oracle and every byte outside the streams; returns the
    output image."""
    torch = require_gpu()
    ioff, ooff = [], []
    ipos = opos = 0
    for frames, bits, ch, seed in specs:
        ioff.append(ipos)
        ipos += (frames * ch * 2 + 15) & ~15
        opos = (opos + align - 1) & ~(align - 1)
        ooff.append(opos)
        opos += xa_len(frames, bits, ch)
    img = np.full(ipos + 64, 0x7F, dtype=np.uint8)
    for (frames, bits, ch, seed), o in zip(specs, ioff):
        img[o:o + frames * ch * 2] = stream(frames, bits, ch, seed)[0].view(np.uint8)
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.full((opos + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    sh = torch.cuda.current_stream().cuda_stream
    descs = [{"d_pcm": d_in.data_ptr() + i, "d_xa": d_out.data_ptr() + o, "frames": f,
              "bits": b, "channels": c} for (f, b, c, _), i, o in zip(specs, ioff, ooff)]
    with bjxa_amd.EncodeBatch(descs, sh) as batch:
        for r in range(repeat):
            if r:
                torch.cuda.synchronize()
                check_image(specs, ooff, d_out.cpu().numpy())
                d_out.fill_(0xA5)
            batch.encode(sh)
        torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    check_image(specs, ooff, out)
    return out


def check_image(specs, ooff, out):
    covered = np.zeros(out.size, dtype=bool)
    for k, ((frames, bits, ch, seed), o) in enumerate(zip(specs, ooff)):
        want = stream(frames, bits, ch, seed)[1]
        assert np.array_equal(out[o:o + want.size], want), \
            "stream %d (%d frames, %d-bit, %dch)" % (k, frames, bits, ch)
        covered[o:o + want.size] = True
    # the padding gaps and the 64 bytes after the last stream
    assert (out[~covered] == 0xA5).all()
    assert (~covered).sum() >= 64


def test_mixed_batch(built):
    """All six formats and every edge length in one launch, each stream in
    an allocation of its own."""
    torch = require_gpu()
    specs = mixed_specs()
    srcs, dsts, descs = [], [], []
    for frames, bits, ch, seed in specs:
        s = torch.from_numpy(np.array(stream(frames, bits, ch, seed)[0])).cuda()
        d = torch.full((xa_len(frames, bits, ch) + 64,), 0xA5, dtype=torch.uint8,
                       device="cuda")
        srcs.append(s)
        dsts.append(d)
        descs.append({"d_pcm": s.data_ptr(), "d_xa": d.data_ptr(), "frames": frames,
                      "bits": bits, "channels": ch})
    sh = torch.cuda.current_stream().cuda_stream
    with bjxa_amd.EncodeBatch(descs, sh) as batch:
        batch.encode(sh)
        torch.cuda.synchronize()
    for k, ((frames, bits, ch, seed), d) in enumerate(zip(specs, dsts)):
        out = d.cpu().numpy()
        n = xa_len(frames, bits, ch)
        assert np.array_equal(out[:n], stream(frames, bits, ch, seed)[1]), \
            "stream %d (%d frames, %d-bit, %dch)" % (k, frames, bits, ch)
        assert (out[n:] == 0xA5).all(), k


@pytest.mark.parametrize("align", [4, 16])
def test_packed_outputs(built, align):
    """Neighbouring streams in one allocation: with 4-byte offsets most
    streams start off a 16-byte boundary (dword and byte stores, gaps of 0
    to 3 bytes), with 16-byte offsets full waves take the wide stores.  No
    byte outside a stream's XA changes, and the 0x7F7F samples between the
    PCM inputs never reach a stream's zero-padded last block."""
    specs = mixed_specs()
    run_packed(specs, align)
    if align == 4:
        pos, starts = 0, []
        for frames, bits, ch, _ in specs:
            pos = (pos + 3) & ~3
            starts.append(pos)
            pos += xa_len(frames, bits, ch)
        assert sum(s % 16 != 0 for s in starts) > len(starts) // 2


def test_formats_mixed_in_workgroup(built):
    """One-wave streams alternating four formats: every workgroup of four
    waves runs four different cases side by side."""
    fmts = [(4, 1), (8, 2), (6, 1), (6, 2)]
    full = {1: 8192, 2: 4096}      # frames of one whole wave
    specs = []
    for i in range(24):
        bits, ch = fmts[i % 4]
        frames = [full[ch], full[ch] - 1, full[ch] - 33, 37, full[ch] // 2 + 5,
                  full[ch]][i // 4]
        specs.append((frames, bits, ch, 300 + i))
    assert all((f + 31) // 32 * c <= 256 for f, _, c, _ in specs)
    run_packed(specs, 4)
    run_packed(specs, 16)


def test_repeat_and_single(built):
    """One batch object encodes again and again (outputs re-poisoned in
    between); a batch of one stream equals bjxa_hip_encode_async."""
    specs = mixed_specs()[:20]
    run_packed(specs, 4, repeat=2)
    for frames, bits, ch, seed in [(100003, 8, 2, 263), (4097, 4, 1, 261)]:
        pcm = np.array(stream(frames, bits, ch, seed)[0])
        out = run_packed([(frames, bits, ch, seed)], 4)
        assert np.array_equal(out[:xa_len(frames, bits, ch)],
                              dev_encode(pcm, frames, bits, ch))


def test_round_trip_through_decode_batch(built):
    """EncodeBatch then Batch: the PCM comes back with the low 16-bits bits
    cleared and every profile byte is 0 (DESIGN.md §6's identity)."""
    torch = require_gpu()
    specs = [(20011 + 1000 * i, bits, ch, 400 + i) for i, (bits, ch) in enumerate(FORMATS)]
    sh = torch.cuda.current_stream().cuda_stream
    pcms, xas, backs, enc, dec = [], [], [], [], []
    for frames, bits, ch, seed in specs:
        eb = (frames + 31) // 32
        p = torch.from_numpy(np.array(stream(frames, bits, ch, seed)[0])).cuda()
        x = torch.full((xa_len(frames, bits, ch),), 0xA5, dtype=torch.uint8, device="cuda")
        d = torch.full((eb * 64 * ch,), 0x5A, dtype=torch.uint8, device="cuda")
        pcms.append(p)
        xas.append(x)
        backs.append(d)
        enc.append({"d_pcm": p.data_ptr(), "d_xa": x.data_ptr(), "frames": frames,
                    "bits": bits, "channels": ch})
        dec.append({"d_src": x.data_ptr(), "d_dst": d.data_ptr(), "eblocks": eb,
                    "bits": bits, "channels": ch, "frames": frames})
    status = torch.zeros(len(specs) * bjxa_amd.STATUS_WORDS, dtype=torch.int32, device="cuda")
    with bjxa_amd.EncodeBatch(enc, sh) as eb_, bjxa_amd.Batch(dec, stream=sh) as db:
        eb_.encode(sh)
        db.decode(status.data_ptr(), sh)
        torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint32).reshape(len(specs), -1)
    for i, (frames, bits, ch, seed) in enumerate(specs):
        xa = xas[i].cpu().numpy()
        assert (xa.reshape(-1, bits * 4 + 1)[:, 0] == 0).all(), i
        assert st[i][0] == bjxa_amd.NO_ERROR, i
        back = backs[i].cpu().numpy().view(np.int16)[:frames * ch]
        want = stream(frames, bits, ch, seed)[0] & np.int16(~((1 << (16 - bits)) - 1))
        assert np.array_equal(back, want), i
