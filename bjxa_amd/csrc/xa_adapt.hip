/*
 * xa_adapt.hip -- gfx950 adaptive XA encode (LIBBJXA_HIP_0.5).
 *
 * The reference encoder (src/libbjxa.c:665-691) writes profile 0 for every
 * block.  This one searches, per channel block, every predictor f in 0..4
 * and range r in 0..R, R = min(16 - bits, 11), in a closed loop, and keeps
 * the candidate of least squared error (ties: smallest f * (R + 1) + r).
 * The specification is DESIGN.md §3 "Adaptive encode"; the CPU statement of
 * it is bjxa__cpu_encode_adaptive (xa_cpu.c), which writes the same bytes.
 *
 * Shape: one wave per (run, channel), lane = candidate.  A run is `sync`
 * consecutive channel blocks; its first block takes f = 0 only, so nothing
 * of it depends on the blocks before and runs are independent work items.
 * A workgroup is the 1 or 2 waves (channels) of one run and walks a
 * grid-stride loop over runs.  The 32 samples of a block are the same for
 * every lane and come through scalar loads; each lane runs its candidate's
 * 32 dependent steps keeping the codes packed in `bits` registers; a
 * butterfly min over sse * 64 + candidate picks the winner, whose packed
 * block goes to an LDS slot and whose exit state is broadcast.  Every
 * XA_ADAPT_FLUSH blocks the workgroup copies its slots -- both channels, so
 * the eblock-major byte range is contiguous -- to global memory with dword
 * stores between byte-exact edges.  No workgroup waits on another.
 */
#include <errno.h>

#include "xa_common.h"
#include "xa_decode.h"
#include "xa_gpu.h"

#define XA_ADAPT_FLUSH	16	/* blocks per channel staged between flushes */
#define XA_ADAPT_GRID	(1u << 20)	/* workgroups at most; runs beyond stride */

struct xa_adapt_args {
	const uint8_t *src;	/* PCM frames, 16-bit, channels interleaved */
	uint8_t *dst;		/* XA blocks */
	uint64_t frames;	/* valid frames; later ones encode as zero */
	uint32_t eblocks;	/* ceil(frames / 32) */
	uint32_t sync;		/* blocks per run, >= 1 */
	uint32_t nruns;		/* ceil(eblocks / sync) */
};

typedef const __attribute__((address_space(4))) uint32_t *xa_cu32p;

/*
 * The 32 samples of channel c of eblock b, sign-extended.  Wave-uniform
 * addresses in the constant address space: scalar loads.  A block wholly
 * inside the stream is read as it lies; the last one dword by dword, no
 * further than the dword holding the last sample, the rest zero.
 */
template <int CH>
__device__ __forceinline__ void
adapt_samples(const xa_adapt_args &a, const uint64_t b, const int c,
    int32_t x[XA_FRAMES])
{
	constexpr int NDW = 16 * CH;
	const uint64_t base = b * (uint64_t)(64 * CH);
	const uint64_t pcm_bytes = a.frames * (uint64_t)(2 * CH);
	xa_cu32p p = (xa_cu32p)(a.src + base);
	uint32_t w[NDW];

	if (base + 64 * CH <= pcm_bytes) {
#pragma unroll
		for (int i = 0; i < NDW; i++)
			w[i] = p[i];
	} else {
#pragma unroll
		for (int i = 0; i < NDW; i++) {
			const uint64_t o = base + 4u * i;
			w[i] = 0;
			if (o < pcm_bytes)
				w[i] = p[i] & (o + 2u < pcm_bytes ? 0xffffffffu :
				    0xffffu);
		}
	}
#pragma unroll
	for (int n = 0; n < XA_FRAMES; n++) {
		if (CH == 2)
			x[n] = (int32_t)(w[n] << (16 - 16 * c)) >> 16;
		else
			x[n] = (int32_t)(w[n >> 1] << (16 - 16 * (n & 1))) >> 16;
	}
}

template <int BITS, int CH>
__global__ __launch_bounds__(64 * CH) void
xa_adapt_runs(xa_adapt_args a)
{
	constexpr int BSZ = BITS * 4 + 1;
	constexpr int R1 = (16 - BITS < 11 ? 16 - BITS : 11) + 1;
	constexpr int NC = 5 * R1;		/* candidates: 60, 55, 45 */
	constexpr int SLOT = BITS + 1;		/* dwords per staged block */
	constexpr int F = XA_ADAPT_FLUSH;
	constexpr int QLO = -(1 << (BITS - 1)), QHI = (1 << (BITS - 1)) - 1;
	/*
	 * Slot k = (block * CH + channel): dword 0 holds the profile in its
	 * last byte, dwords 1..BITS the data in memory order, so the block's
	 * BSZ bytes lie together from byte 3 of the slot.
	 */
	__shared__ uint32_t stage[F * CH * SLOT];

	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
	/* lanes past the last candidate redo it and stay out of the argmin */
	const int cand = lane < NC ? lane : NC - 1;
	const int f = cand / R1, r = cand % R1;
	const int s = 16 - BITS - r;
	const int32_t half = (1 << s) >> 1;
	int32_t k0, k1;
	xa_gain((uint32_t)f, k0, k1);

	for (uint64_t run = blockIdx.x; run < a.nruns; run += gridDim.x) {
		const uint64_t b0 = run * a.sync;
		const uint64_t left = (uint64_t)a.eblocks - b0;
		const uint32_t nb = left < a.sync ? (uint32_t)left : a.sync;
		int32_t p0 = 0, p1 = 0;

		for (uint32_t j0 = 0; j0 < nb; j0 += F) {
			const uint32_t nf = nb - j0 < (uint32_t)F ? nb - j0 :
			    (uint32_t)F;

			for (uint32_t j = 0; j < nf; j++) {
				int32_t x[XA_FRAMES];
				uint32_t acc[BITS];
				uint64_t sse = 0;
				int32_t q0 = p0, q1 = p1;

				adapt_samples<CH>(a, b0 + j0 + j, c, x);
#pragma unroll
				for (int i = 0; i < BITS; i++)
					acc[i] = 0;
#pragma unroll
				for (int n = 0; n < XA_FRAMES; n++) {
					const int32_t g = __mul24(q0, k0) +
					    __mul24(q1, k1);
					const int32_t pred = (g + (int32_t)(
					    (uint32_t)(g >> 31) >> 24)) >> 8;
					int32_t q = (x[n] - pred + half) >> s;
					q = min(max(q, QLO), QHI);
					int32_t y = (int32_t)((uint32_t)q << s) + pred;
					y = min(max(y, -32768), 32767);
					const int32_t e = x[n] - y;
					/* |e| <= 65535: the square fits 32 bits */
					sse += (uint32_t)__mul24(e, e);
					q1 = q0;
					q0 = y;
					/* big-endian bit stream of the codes
					 * (src/libbjxa.c:349-391) */
					const uint32_t code = (uint32_t)q &
					    ((1u << BITS) - 1u);
					const int pos = n * BITS, wi = pos >> 5;
					const int room = 32 - (pos & 31);
					if (room >= BITS) {
						acc[wi] |= code << (room - BITS);
					} else {
						acc[wi] |= code >> (BITS - room);
						acc[wi + 1] |= code <<
						    (32 - (BITS - room));
					}
				}

				/* a run's first block: f = 0 only */
				uint64_t key = (sse << 6) | (uint32_t)cand;
				if (lane >= NC || (j0 + j == 0 && f != 0))
					key = ~0ull;
#pragma unroll
				for (int m = 32; m >= 1; m >>= 1) {
					const uint64_t o = __shfl_xor(key, m);
					key = o < key ? o : key;
				}
				const int win = __builtin_amdgcn_readfirstlane(
				    (int)((uint32_t)key & 63u));
				p0 = __builtin_amdgcn_readlane(q0, win);
				p1 = __builtin_amdgcn_readlane(q1, win);
				if (lane == win) {
					uint32_t *slot = stage + (j * CH + c) * SLOT;
					slot[0] = (uint32_t)(f << 4 | r) << 24;
#pragma unroll
					for (int i = 0; i < BITS; i++)
						slot[1 + i] = __builtin_bswap32(acc[i]);
				}
			}
			__syncthreads();

			/* this workgroup's bytes of blocks b0+j0 .. +nf, both
			 * channels: one contiguous range inside the stream */
			uint8_t *out = a.dst + (b0 + j0) * (uint64_t)(CH * BSZ);
			const uint32_t total = nf * (uint32_t)(CH * BSZ);
			const uint8_t *sb = (const uint8_t *)stage;
#define STAGED(i) sb[((i) / BSZ) * (SLOT * 4) + 3 + (i) % BSZ]
			uint32_t head = (uint32_t)(-(uintptr_t)out & 3u);
			if (head > total)
				head = total;
			const uint32_t ndw = (total - head) >> 2;
			const uint32_t tail = head + 4u * ndw;
			if ((uint32_t)tid < head)
				out[tid] = STAGED((uint32_t)tid);
			for (uint32_t k = (uint32_t)tid; k < ndw; k += 64 * CH) {
				const uint32_t i = head + 4u * k;
				*(uint32_t *)(out + i) = (uint32_t)STAGED(i) |
				    (uint32_t)STAGED(i + 1) << 8 |
				    (uint32_t)STAGED(i + 2) << 16 |
				    (uint32_t)STAGED(i + 3) << 24;
			}
			if (tail + (uint32_t)tid < total)
				out[tail + tid] = STAGED(tail + (uint32_t)tid);
#undef STAGED
			__syncthreads();
		}
	}
}

static hipError_t
xa_adapt_launch(const xa_adapt_args &a, unsigned bits, unsigned ch,
    hipStream_t st)
{
	const unsigned grid = a.nruns < XA_ADAPT_GRID ? a.nruns : XA_ADAPT_GRID;
#define L(B, C) hipLaunchKernelGGL((xa_adapt_runs<B, C>), dim3(grid), \
    dim3(64 * C), 0, st, a)
	if (ch == 1) {
		if (bits == 8) L(8, 1); else if (bits == 6) L(6, 1); else L(4, 1);
	} else {
		if (bits == 8) L(8, 2); else if (bits == 6) L(6, 2); else L(4, 2);
	}
#undef L
	return hipGetLastError();
}

extern "C" int
bjxa_hip_encode_adaptive_async(const void *d_pcm, uint64_t frames,
    unsigned bits, unsigned channels, uint32_t sync, void *d_xa, void *stream)
{
	if (d_pcm == NULL || d_xa == NULL || frames == 0 ||
	    (bits != 4 && bits != 6 && bits != 8) ||
	    (channels != 1 && channels != 2) || sync == 0 ||
	    frames > 32 * (uint64_t)0xffffffffu ||
	    ((uintptr_t)d_pcm & 15u) != 0 || ((uintptr_t)d_xa & 3u) != 0) {
		errno = EINVAL;
		return -1;
	}
	if (!bjxa__gpu_present()) {
		errno = ENODEV;
		return -1;
	}
	xa_adapt_args a;
	a.src = (const uint8_t *)d_pcm;
	a.dst = (uint8_t *)d_xa;
	a.frames = frames;
	a.eblocks = (uint32_t)((frames + 31) / 32);
	a.sync = sync;
	a.nruns = (uint32_t)(((uint64_t)a.eblocks + sync - 1) / sync);
	if (xa_adapt_launch(a, bits, channels, (hipStream_t)stream) !=
	    hipSuccess) {
		(void)hipGetLastError();
		errno = EIO;
		return -1;
	}
	return 0;
}

/*
 * bjxa_hip_encode_adaptive's device route (xa_gpu.h): one allocation holding
 * the PCM and the XA, copy in, one launch, copy out.  The copies are
 * synchronous on the null stream, so the call returns with `dst` complete.
 */
extern "C" int
bjxa__gpu_encode_adaptive(const void *src, uint64_t frames, unsigned bits,
    unsigned ch, uint32_t sync, void *dst)
{
	const size_t in_bytes = (size_t)frames * 2u * ch;
	const size_t in_room = (in_bytes + 255) & ~(size_t)255;
	const size_t out_bytes = (size_t)((frames + 31) / 32) * ch *
	    (bits * 4u + 1u);
	uint8_t *d = NULL;
	int rc = -1;

	if (!bjxa__gpu_present()) {
		errno = ENODEV;
		return -1;
	}
	if (hipMalloc((void **)&d, in_room + out_bytes) != hipSuccess) {
		(void)hipGetLastError();
		errno = ENOMEM;
		return -1;
	}
	if (hipMemcpy(d, src, in_bytes, hipMemcpyHostToDevice) != hipSuccess) {
		errno = EIO;
	} else if (bjxa_hip_encode_adaptive_async(d, frames, bits, ch, sync,
	    d + in_room, NULL) < 0) {
		/* errno set */
	} else if (hipMemcpy(dst, d + in_room, out_bytes,
	    hipMemcpyDeviceToHost) != hipSuccess) {
		errno = EIO;
	} else {
		rc = 0;
	}
	if (rc < 0) {
		const int e = errno;
		(void)hipGetLastError();
		errno = e;
	}
	{
		const int e = errno;
		(void)hipFree(d);
		errno = e;
	}
	return rc;
}
