/*
 * test_encode_files.c -- the host half of bjxa_hip_encode_files
 * (libbjxa.c), linked with xa_cpu.c and xa_gpu_none.c into one program and
 * run under ASan/UBSan (tests/test_encode_files_host.py): argument errors,
 * every per-file status, exact-size and one-byte-short buffers, and that a
 * refused file's output keeps its canary bytes.  No device exists here, so
 * a batch with an accepted file ends in ENODEV -- after the framing of every
 * file has run -- and a batch of refused files returns 0.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

#include "bjxa.h"
#include "bjxa_hip.h"

#define CANARY	0xC7

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, \
	__LINE__, #c); exit(1); } } while (0)

static void
put32(uint8_t *p, uint32_t v)
{
	for (int i = 0; i < 4; i++)
		p[i] = (uint8_t)(v >> (8 * i));
}

static void
put16(uint8_t *p, uint32_t v)
{
	p[0] = (uint8_t)v;
	p[1] = (uint8_t)(v >> 8);
}

/* a heap WAV file of exactly 44 + data_len + extra bytes */
static uint8_t *
make_wav(uint32_t frames, unsigned ch, uint32_t rate, size_t extra, size_t *len)
{
	const uint32_t data_len = frames * ch * 2u;
	uint8_t *w = malloc(44 + (size_t)data_len + extra);

	CHECK(w != NULL);
	memcpy(w, "RIFF", 4);
	put32(w + 4, 36 + data_len);
	memcpy(w + 8, "WAVEfmt ", 8);
	put32(w + 16, 16);
	put16(w + 20, 1);
	put16(w + 22, ch);
	put32(w + 24, rate);
	put32(w + 28, rate * ch * 2u);
	put16(w + 32, ch * 2u);
	put16(w + 34, 16);
	memcpy(w + 36, "data", 4);
	put32(w + 40, data_len);
	for (size_t i = 0; i < (size_t)data_len + extra; i++)
		w[44 + i] = (uint8_t)(i * 7 + 3);
	*len = 44 + (size_t)data_len + extra;
	return (w);
}

static size_t
xa_size(uint32_t frames, unsigned ch, unsigned bits)
{
	return (32 + (size_t)((frames + 31) / 32) * ch * (bits * 4 + 1));
}

static uint8_t *
canary_buf(size_t len)
{
	uint8_t *p = malloc(len);

	CHECK(p != NULL);
	memset(p, CANARY, len);
	return (p);
}

static int
all_canary(const uint8_t *p, size_t len)
{
	for (size_t i = 0; i < len; i++)
		if (p[i] != CANARY)
			return (0);
	return (1);
}

static void
argument_errors(void)
{
	size_t wl, xl = xa_size(100, 2, 8);
	uint8_t *w = make_wav(100, 2, 8000, 0, &wl), *x = canary_buf(xl);
	const void *wav[1] = { w };
	void *xa[1] = { x };
	uint8_t bits[1] = { 8 };
	int st[1] = { -1 };

#define ARGS(a, b, c, d, e, f, n) \
	bjxa_hip_encode_files(a, b, c, d, e, f, n)
	errno = 0;
	CHECK(ARGS(NULL, &wl, bits, xa, &xl, st, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, NULL, bits, xa, &xl, st, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, &wl, NULL, xa, &xl, st, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, &wl, bits, NULL, &xl, st, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, &wl, bits, xa, NULL, st, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, &wl, bits, xa, &xl, NULL, 1) == -1 && errno == EFAULT);
	errno = 0;
	CHECK(ARGS(wav, &wl, bits, xa, &xl, st, 0) == -1 && errno == EINVAL);
#undef ARGS
	CHECK(st[0] == -1);
	CHECK(all_canary(x, xl));
	free(w);
	free(x);
}

enum { F_NULL_WAV, F_NULL_XA, F_SHORT_HDR, F_RIFX, F_EMPTY, F_BITS5, F_BITS0,
    F_BODY_SHORT, F_BODY_SHORT1, F_OUT_SHORT, F_OUT_TINY, F_CH3, F_N };

static void
refused_only(void)
{
	static const int want[F_N] = { EFAULT, EFAULT, ENOBUFS, EPROTO, EPROTO,
	    EINVAL, EINVAL, ENOBUFS, ENOBUFS, ENOBUFS, ENOBUFS, EPROTO };
	const void *wav[F_N];
	void *xa[F_N];
	uint8_t *w[F_N], *x[F_N], bits[F_N];
	size_t wl[F_N], xl[F_N];
	int st[F_N];

	for (int i = 0; i < F_N; i++) {
		w[i] = make_wav(1000 + i, 1 + i % 2, 22050, 0, &wl[i]);
		bits[i] = (uint8_t)(4 + 2 * (i % 3));
		xl[i] = xa_size(1000 + i, 1 + i % 2, bits[i]);
		x[i] = canary_buf(xl[i]);
		wav[i] = w[i];
		xa[i] = x[i];
		st[i] = -1;
	}
	wav[F_NULL_WAV] = NULL;
	xa[F_NULL_XA] = NULL;
	wl[F_SHORT_HDR] = 43;
	memcpy(w[F_RIFX], "RIFX", 4);
	put32(w[F_EMPTY] + 40, 0);
	bits[F_BITS5] = 5;
	bits[F_BITS0] = 0;
	wl[F_BODY_SHORT] -= 100;
	wl[F_BODY_SHORT1] -= 1;
	/* one byte short: a fresh allocation, so that ASan sees a write to
	 * the byte that is not there */
	free(x[F_OUT_SHORT]);
	xl[F_OUT_SHORT] -= 1;
	xa[F_OUT_SHORT] = x[F_OUT_SHORT] = canary_buf(xl[F_OUT_SHORT]);
	free(x[F_OUT_TINY]);
	xl[F_OUT_TINY] = 31;
	xa[F_OUT_TINY] = x[F_OUT_TINY] = canary_buf(31);
	put16(w[F_CH3] + 22, 3);

	errno = 0;
	CHECK(bjxa_hip_encode_files(wav, wl, bits, xa, xl, st, F_N) == 0);
	for (int i = 0; i < F_N; i++) {
		if (st[i] != want[i]) {
			fprintf(stderr, "file %d: status %d, want %d\n", i, st[i],
			    want[i]);
			exit(1);
		}
		CHECK(all_canary(x[i], xl[i]));
		free(w[i]);
		free(x[i]);
	}
}

/* accepted files reach the device, which this build does not have */
static void
accepted(void)
{
	enum { N = 5 };
	static const uint32_t frames[N] = { 1, 32, 33, 4097, 1000 };
	const void *wav[N];
	void *xa[N];
	uint8_t *w[N], *x[N], bits[N];
	size_t wl[N], xl[N];
	int st[N];

	for (int i = 0; i < N; i++) {
		const unsigned ch = 1 + i % 2;
		/* file 3 carries junk after its PCM; file 4 is refused */
		w[i] = make_wav(frames[i], ch, 44100, i == 3 ? 1000 : 0, &wl[i]);
		bits[i] = (uint8_t)(4 + 2 * (i % 3));
		xl[i] = xa_size(frames[i], ch, bits[i]);	/* exact */
		x[i] = canary_buf(xl[i]);
		wav[i] = w[i];
		xa[i] = x[i];
		st[i] = -1;
	}
	memcpy(w[4] + 8, "WAVX", 4);
	errno = 0;
	CHECK(bjxa_hip_encode_files(wav, wl, bits, xa, xl, st, N) == -1);
	CHECK(errno == ENODEV);
	for (int i = 0; i < 4; i++) {
		CHECK(st[i] == 0);
		/* the header is in place, the blocks were never written */
		CHECK(memcmp(x[i], "KWD1", 4) == 0);
		CHECK(x[i][14] == bits[i] && x[i][15] == 1 + i % 2);
		CHECK(all_canary(x[i] + 32, xl[i] - 32));
	}
	CHECK(st[4] == EPROTO);
	CHECK(all_canary(x[4], xl[4]));
	for (int i = 0; i < N; i++) {
		free(w[i]);
		free(x[i]);
	}
}

int
main(void)
{
	argument_errors();
	refused_only();
	accepted();
	printf("test_encode_files: ok\n");
	return (0);
}
