"""The adaptive encoder's specification (DESIGN.md §3 "Adaptive encode")
restated in numpy, and the signals its tests use.  TEST INFRASTRUCTURE ONLY: an independent model
the library is compared against byte for byte; it shares no code with
bjxa_amd/.  Vectorised over channels and candidates, 32 steps per block."""
import functools

import numpy as np

K = np.array([[0, 0], [240, 0], [460, -208], [392, -220], [488, -240]], np.int64)

# (sync, eblocks) of the byte-for-byte checks; frames = 32 * eblocks - k
SHAPES = [(1, 5), (4, 1), (4, 3), (4, 4), (4, 5), (4, 17), (64, 70), (1000, 40)]
CUTS = [0, 1, 31]


KINDS = ["sine", "noise_full", "noise_40", "square_full", "zeros"]


def kinds(n, rng):
    """The five signals (KINDS) at sample positions n, int64 (5, n.size)."""
    return np.stack([
        12000 * np.sin(n * (2 * np.pi / 53.0)) + rng.integers(-30, 31, n.size),
        rng.integers(-32768, 32768, n.size),
        rng.integers(-40, 41, n.size),
        np.where((n // 7) % 2 == 0, 32767, -32768),
        np.zeros(n.size),
    ]).astype(np.int64)


def signal(frames, ch, seed):
    """int16 PCM, channels interleaved: block by block a seeded mix of sine
    plus a little noise, full-scale uniform noise (clamps), +-40 LSB noise
    (high ranges), full-scale square (predictor overshoot into the clamp)
    and zeros; the right channel runs two kinds ahead of the left."""
    rng = np.random.default_rng(seed)
    eb = (frames + 31) // 32
    n = np.arange(eb * 32)
    sig = kinds(n, rng)
    out = np.empty((eb * 32, ch), np.int16)
    for c in range(ch):
        kind = (n // 32 + 2 * c + seed) % 5
        out[:, c] = sig[kind, n]
    return np.ascontiguousarray(out[:frames]).reshape(-1)


def padded(pcm, frames, ch):
    """(32 * eblocks, ch) int64: the PCM followed by zeros."""
    eb = (frames + 31) // 32
    x = np.zeros((eb * 32, ch), np.int64)
    x[:frames] = np.asarray(pcm, np.int16).reshape(-1, ch)[:frames]
    return x


def encode(pcm, frames, bits, ch, sync):
    """XA blocks (uint8) of the specification's encoder."""
    eb = (frames + 31) // 32
    x = padded(pcm, frames, ch)
    R = min(16 - bits, 11)
    nc = 5 * (R + 1)
    f = np.repeat(np.arange(5), R + 1)
    r = np.tile(np.arange(R + 1), 5)
    s = 16 - bits - r
    k0, k1 = K[f, 0], K[f, 1]
    half = (1 << s) >> 1
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    cand = np.arange(nc)
    shifts = np.arange(bits - 1, -1, -1)
    out = np.zeros((eb, ch, 4 * bits + 1), np.uint8)
    p0 = np.zeros(ch, np.int64)
    p1 = np.zeros(ch, np.int64)
    chans = np.arange(ch)
    for b in range(eb):
        P0 = np.repeat(p0[:, None], nc, 1)
        P1 = np.repeat(p1[:, None], nc, 1)
        sse = np.zeros((ch, nc), np.int64)
        codes = np.empty((ch, nc, 32), np.int64)
        for n in range(32):
            xs = x[b * 32 + n][:, None]
            g = P0 * k0 + P1 * k1
            pred = np.sign(g) * (np.abs(g) // 256)      # C division
            q = np.clip((xs - pred + half) >> s, lo, hi)
            y = np.clip(q * (1 << s) + pred, -32768, 32767)
            sse += (xs - y) ** 2
            P1, P0 = P0, y
            codes[:, :, n] = q
        key = sse * 64 + cand
        if b % sync == 0:
            key[:, f != 0] = np.iinfo(np.int64).max
        w = np.argmin(key, axis=1)
        p0, p1 = P0[chans, w], P1[chans, w]
        for c in range(ch):
            out[b, c, 0] = (f[w[c]] << 4) | r[w[c]]
            code = codes[c, w[c]] & ((1 << bits) - 1)
            # big-endian bit stream of the codes, first sample first
            out[b, c, 1:] = np.packbits(((code[:, None] >> shifts) & 1).astype(np.uint8))
    return out.reshape(-1)


@functools.lru_cache(maxsize=None)
def case(bits, ch, sync, eblocks, cut):
    """(pcm, frames, model XA) of one shape; computed once per session and
    shared by the tests that need it -- treat as read-only."""
    frames = 32 * eblocks - cut
    pcm = signal(frames, ch, seed=bits + 3 * ch + eblocks)
    xa = encode(pcm, frames, bits, ch, sync)
    pcm.setflags(write=False)
    xa.setflags(write=False)
    return pcm, frames, xa


def block_sse(pcm, frames, ch, decoded):
    """Squared error per (eblock, channel) of `decoded` (int16, 32 * eblocks
    frames) against the zero-padded input."""
    x = padded(pcm, frames, ch)
    y = np.asarray(decoded, np.int16).astype(np.int64).reshape(-1, ch)
    return ((x - y) ** 2).reshape(-1, 32, ch).sum(axis=1)
