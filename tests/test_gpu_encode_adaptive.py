"""Adaptive encode (LIBBJXA_HIP_0.5) on the MI355X: the device entry byte
for byte against the numpy model of the specification
(tests/xa_adaptive_model.py), with guard bytes round an output that is 4-byte
but not 16-byte aligned; the host entry's GPU route against its CPU route;
two launches back to back; the CLI on the GPU route."""
import os
import subprocess

import numpy as np
import pytest

import bjxa_amd
import xa_adaptive_model as model
from gpu_util import require_gpu
from test_encode_adaptive_host import BJXA, NEVER, NO_GPU, cut_wav

pytestmark = pytest.mark.gpu

GUARD = 64
# host shapes, plus more runs than one workgroup holds and a run that flushes
# its staging several times with a short last run
SHAPES = model.SHAPES + [(4, 280), (64, 130)]
CASES = [(bits, ch, sync, eb, cut) for bits in (4, 6, 8) for ch in (1, 2)
         for sync, eb in SHAPES for cut in model.CUTS
         if (sync, eb) != (4, 280) or ch == 2]


def launch(torch, pcm, frames, bits, ch, sync):
    """Queue one device encode; returns (output tensor, offset, length)."""
    src = torch.from_numpy(np.array(pcm, dtype=np.int16)).cuda()
    n = (frames + 31) // 32 * ch * (bits * 4 + 1)
    # torch allocations are at least 256-B aligned: offset 64 + 4 is 4-byte
    # but not 16-byte aligned
    off = GUARD + 4
    dst = torch.full((off + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert dst.data_ptr() % 16 == 0
    bjxa_amd.encode_adaptive_device(src.data_ptr(), frames, bits, ch, dst.data_ptr() + off,
                                    sync, torch.cuda.current_stream().cuda_stream)
    return src, dst, off, n


def collect(dst, off, n):
    out = dst.cpu().numpy()
    assert (out[:off] == 0xA5).all() and (out[off + n:] == 0xA5).all()
    return out[off:off + n]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "b%d-c%d-s%d-e%d-k%d" % c)
def test_device_equals_model(built, c):
    torch = require_gpu()
    bits, ch, sync, eb, cut = c
    pcm, frames, want = model.case(*c)
    _, dst, off, n = launch(torch, pcm, frames, bits, ch, sync)
    torch.cuda.synchronize()
    assert np.array_equal(collect(dst, off, n), want)


@pytest.mark.parametrize("c", [(4, 2, 4, 17, 1), (8, 1, 64, 70, 31)])
def test_host_entry_routes_agree(built, c):
    require_gpu()
    bits, ch, sync, eb, cut = c
    pcm, frames, want = model.case(*c)
    d = bjxa_amd.OFFLOAD_ENCODE_ADAPTIVE
    old = bjxa_amd.offload_threshold(d, 0)
    try:
        gpu = bjxa_amd.encode_adaptive(pcm, frames, bits, ch, sync)
        bjxa_amd.offload_threshold(d, NEVER)
        cpu = bjxa_amd.encode_adaptive(pcm, frames, bits, ch, sync)
    finally:
        bjxa_amd.offload_threshold(d, old)
    assert np.array_equal(gpu, want) and np.array_equal(cpu, want)


def test_two_launches_back_to_back(built):
    torch = require_gpu()
    a = (6, 2, 64, 70, 1)
    b = (4, 1, 4, 17, 31)
    runs = []
    for c in (a, b):
        pcm, frames, want = model.case(*c)
        runs.append((launch(torch, pcm, frames, c[0], c[1], c[2]), want))
    torch.cuda.synchronize()
    for (_, dst, off, n), want in runs:
        assert np.array_equal(collect(dst, off, n), want)


def test_cli_gpu_route(built, golden):
    require_gpu()
    wav = cut_wav(golden("square-stereo.wav"), 200 * 32 - 5, 2)
    outs = []
    for env in (dict(BJXA_OFFLOAD_ENCODE_ADAPTIVE="0"), NO_GPU):
        p = subprocess.run([BJXA, "encode", "--adaptive", "--bits", "4"], input=wav,
                           capture_output=True, env=dict(os.environ, **env), timeout=120)
        assert p.returncode == 0, p.stderr.decode(errors="replace")
        outs.append(p.stdout)
    assert outs[0] == outs[1] and len(outs[0]) == 32 + 200 * 34
