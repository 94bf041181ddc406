/*
 * legacy_drop_in.c -- the legacy face used from plain C99 through lz4.h alone, the way Streamly.Internal.LZ4 calls it: one
 * LZ4_stream_t and one LZ4_streamDecode_t for the whole stream, every block in an allocation of its own, compressed into
 * LZ4_compressBound(n) bytes and decoded into exactly n.  Built and run by tests/test_c_example.py.
 */
#include "lz4.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define N_BLOCKS 40

static int fail(const char *what, int block, int value)
{
    fprintf(stderr, "legacy_drop_in: %s (block %d, value %d)\n", what, block, value);
    return 1;
}

/* repetitive text whose length and wording change from block to block */
static int make_block(char *p, int k)
{
    static const char *words[] = {"stream ", "of ", "arrays ", "compressed ", "block ", "by ", "the ", "quick ", "brown ", "fox "};
    const int n = 200 + 977 * k;
    unsigned x = 12345u + 7919u * (unsigned)k;
    int pos = 0;
    while (pos < n) {
        const char *w;
        int len;
        x = x * 1103515245u + 12345u;
        w = words[(x >> 16) % 10u];
        len = (int)strlen(w);
        if (len > n - pos) len = n - pos;
        memcpy(p + pos, w, (size_t)len);
        pos += len;
    }
    return n;
}

int main(void)
{
    static const int sizes[] = {0, 1, 12, 13, 254, 255, 256, 65535, 65536, 65537, 1048576, 0x7DFFFFFF, 0x7E000000, 0x7E000001};
    LZ4_stream_t *cs;
    LZ4_streamDecode_t *ds;
    char *prevBack = NULL;
    size_t i;
    int k;

    for (i = 0; i < sizeof(sizes) / sizeof(sizes[0]); i++)
        if (LZ4_COMPRESSBOUND(sizes[i]) != LZ4_compressBound(sizes[i])) return fail("LZ4_COMPRESSBOUND differs from LZ4_compressBound", -1, sizes[i]);
    if (LZ4_compressBound(0x7E000001) != 0 || LZ4_compressBound(-1) != 0 || LZ4_compressBound(0) != 16)
        return fail("LZ4_compressBound", -1, 0);

    cs = LZ4_createStream();
    ds = LZ4_createStreamDecode();
    if (!cs || !ds) return fail("create", -1, 0);
    for (k = 0; k < N_BLOCKS; k++) {
        char *src = (char *)malloc((size_t)(200 + 977 * k));
        const int n = make_block(src, k);
        const int bound = LZ4_compressBound(n);
        char *comp = (char *)malloc((size_t)bound);
        char *back = (char *)malloc((size_t)n);
        int c, d;
        if (!src || !comp || !back) return fail("malloc", k, n);
        c = LZ4_compress_fast_continue(cs, src, comp, n, bound, 1);
        if (c <= 0 || c > bound) return fail("LZ4_compress_fast_continue", k, c);
        d = LZ4_decompress_safe_continue(ds, comp, back, c, n);
        if (d != n) return fail("LZ4_decompress_safe_continue", k, d);
        if (memcmp(src, back, (size_t)n) != 0) return fail("bytes differ", k, n);
        free(src);
        free(comp);
        free(prevBack);                                  /* the previous output is kept alive one step, as the caller does */
        prevBack = back;
    }
    free(prevBack);
    LZ4_freeStream(cs);
    LZ4_freeStreamDecode(ds);
    printf("legacy round trip ok: %d blocks\n", N_BLOCKS);
    return 0;
}
