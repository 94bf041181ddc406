/* fill_model.c -- a CPU restatement of LZ4_compress_destSize (the reference's fill mode) in this project's own words: what
 * streamly-lz4_amd/csrc/encode_fill.hpp computes with one wavefront, written as plain serial C over positions, so that the GPU
 * tests have a spec that needs no reference build.  tests/test_pages_host.py holds it to tests/golden/pages_vectors.json (the
 * reference's recorded results) on the whole grid of tests/pages_cases.py, and to the reference itself where oracle/_ref exists.
 *
 * Built by the tests:   gcc -O2 -shared -fPIC -o libfillmodel.so fill_model.c
 * and stand-alone:      gcc -O1 -g -fsanitize=address,undefined -DFILL_MODEL_MAIN -o fill_model_san fill_model.c
 *
 * Besides the bytes it reports which fill rule ended a page: the first of the four that fired (a rewind is always followed by the
 * last run, and a shortened match leaves six bytes of room, so the first one decides how the page ends). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>

enum { RULE_NONE = 0, RULE_LITERAL_REWIND = 1, RULE_TOKEN_REWIND = 2, RULE_SHORT_MATCH = 3, RULE_ADAPTED_LAST_RUN = 4 };

#define MINMATCH 4
#define LASTLITERALS 5
#define MFLIMIT 12
#define MAXDIST 65535u
#define LIMIT_64K 65547           /* below it: 16-bit table entries, 4-byte hash of 13 bits, no distance test */
#define MAX_INPUT 0x7E000000

static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t rd64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

static uint32_t hash_at(const uint8_t *p, int small)
{
    if (small) return (rd32(p) * 2654435761u) >> (32 - 13);
    return (uint32_t)(((rd64(p) << 24) * 889523592379ULL) >> (64 - 12));
}

static int bound_of(int n) { return (unsigned)n > (unsigned)MAX_INPUT ? 0 : n + n / 255 + 16; }

/* a literal run: token position kept, length field, bytes; returns the token's high nibble */
static uint32_t put_run(uint8_t *dst, long *op, long *tokenAt, const uint8_t *from, uint32_t lit)
{
    uint32_t token;
    *tokenAt = (*op)++;
    if (lit >= 15) {
        uint32_t rest = lit - 15;
        token = 15u << 4;
        for (; rest >= 255; rest -= 255) dst[(*op)++] = 255;
        dst[(*op)++] = (uint8_t)rest;
    } else {
        token = lit << 4;
    }
    memcpy(dst + *op, from, lit);
    *op += lit;
    return token;
}

/* One page from a zeroed table: src[0..n), n > 0, into dst[0..cap).  fill = 0: the output is not limited (cap >= bound_of(n)). */
static int encode_page(uint32_t *tab, const uint8_t *src, int n, uint8_t *dst, int cap, int fill, int *used, int *rule)
{
    const int small = n < LIMIT_64K;
    const long mfl1 = (long)n - MFLIMIT + 1, matchlimit = (long)n - LASTLITERALS, olimit = cap;
    long ip = 0, anchor = 0, op = 0, match = 0, tokenAt = 0;
    uint32_t token = 0, fh;
    int first = RULE_NONE;

    *used = n;
    *rule = RULE_NONE;
    if (fill && cap < 1) return 0;
    if (n < 13) goto last;
    tab[hash_at(src, small)] = 0;
    ip = 1;
    fh = hash_at(src + 1, small);
    for (;;) {
        long fwd = ip;
        uint32_t step = 1, tries = 1u << 6;
        for (;;) {
            const uint32_t h = fh, cur = (uint32_t)fwd, cand = tab[h];
            ip = fwd;
            fwd += step;
            step = tries++ >> 6;
            if (fwd > mfl1) goto last;
            fh = hash_at(src + fwd, small);
            tab[h] = cur;
            if (!small && cand + MAXDIST < cur) continue;
            if (rd32(src + cand) == rd32(src + ip)) { match = cand; break; }
        }
        while (ip > anchor && match > 0 && src[ip - 1] == src[match - 1]) { ip--; match--; }
        {
            const uint32_t lit = (uint32_t)(ip - anchor);
            /* rule 1: the run, an offset, a token and eight last literals no longer fit */
            if (fill && op + 1 + (lit + 240) / 255 + lit + 2 + 1 + MFLIMIT - MINMATCH > olimit) {
                if (!first) first = RULE_LITERAL_REWIND;
                goto last;
            }
            token = put_run(dst, &op, &tokenAt, src + anchor, lit);
        }
    again:
        /* rule 2: a sequence without literals whose offset, token and eight last literals no longer fit */
        if (fill && op + 2 + 1 + MFLIMIT - MINMATCH > olimit) {
            if (!first) first = RULE_TOKEN_REWIND;
            op = tokenAt;
            goto last;
        }
        dst[op++] = (uint8_t)(ip - match);
        dst[op++] = (uint8_t)((ip - match) >> 8);
        {
            uint32_t mc = 0;
            const uint8_t *a = src + ip + MINMATCH, *b = src + match + MINMATCH;
            while (a + mc < src + matchlimit && a[mc] == b[mc]) mc++;
            ip += (long)mc + MINMATCH;
            /* rule 3: the length field would run into the last run's six bytes: cut the match to what the room encodes */
            if (fill && op + 1 + LASTLITERALS + (mc + 240) / 255 > olimit) {
                const uint32_t shorter = 14 + ((uint32_t)(olimit - op) - 1 - LASTLITERALS) * 255;
                if (!first) first = RULE_SHORT_MATCH;
                ip -= (long)(mc - shorter);
                mc = shorter;
            }
            if (mc >= 15) {
                token += 15;
                mc -= 15;
                for (; mc >= 255; mc -= 255) dst[op++] = 255;
                dst[op++] = (uint8_t)mc;
            } else {
                token += mc;
            }
            dst[tokenAt] = (uint8_t)token;
        }
        anchor = ip;
        if (ip >= mfl1) break;
        tab[hash_at(src + ip - 2, small)] = (uint32_t)(ip - 2);
        {
            const uint32_t h = hash_at(src + ip, small), cur = (uint32_t)ip, cand = tab[h];
            tab[h] = cur;
            if ((small || cand + MAXDIST >= cur) && rd32(src + cand) == rd32(src + ip)) {
                match = cand;
                tokenAt = op++;
                token = 0;
                goto again;
            }
        }
        fh = hash_at(src + (++ip), small);
    }
last:
    {
        uint32_t lastRun = (uint32_t)(n - anchor);
        /* rule 4: the last run takes what is left of the page */
        if (fill && op + lastRun + 1 + (lastRun + 240) / 255 > olimit) {
            if (!first) first = RULE_ADAPTED_LAST_RUN;
            lastRun = (uint32_t)(olimit - op) - 1;
            lastRun -= (lastRun + 241) / 256;
        }
        token = put_run(dst, &op, &tokenAt, src + anchor, lastRun);
        dst[tokenAt] = (uint8_t)token;
        *used = (int)(anchor + lastRun);
    }
    *rule = first;
    return (int)op;
}

/* LZ4_compress_destSize: as much of src[0..n) as fits into dst[0..target).  Returns the page's size; *consumed is only
 * changed where the reference stores through srcSizePtr (it stays n otherwise).  dst needs max(target, 1) bytes. */
int fill_model_page(const uint8_t *src, int n, uint8_t *dst, int target, int *consumed, int *rule)
{
    static uint32_t tab[8192];
    int used = n, r = RULE_NONE, c;
    const int fill = !(target >= bound_of(n));
    *consumed = n;
    *rule = RULE_NONE;
    if ((unsigned)n > (unsigned)MAX_INPUT) return 0;
    if (n == 0) {
        if (fill && target <= 0) return 0;
        dst[0] = 0;
        if (fill) *consumed = 0;
        return 1;
    }
    memset(tab, 0, sizeof tab);
    c = encode_page(tab, src, n, dst, target, fill, &used, &r);
    if (c > 0 && fill) *consumed = used;
    *rule = r;
    return c;
}

/* The chain of one input, as mi355lz4_compress_pages_device lays it out: page k at pages + k * stride behind a header of
 * headerKind bytes.  Returns the pages written; srcLen[], compLen[], rules[] have maxPages entries. */
int fill_model_chain(const uint8_t *src, int n, int pageSize, int maxPages, int headerKind, uint8_t *pages, size_t stride,
                     int32_t *srcLen, int32_t *compLen, int32_t *rules, int32_t *consumedOut)
{
    int pos = 0, k = 0;
    while (k < maxPages) {
        int used, rule;
        uint8_t *page = pages + (size_t)k * stride;
        const int c = fill_model_page(src + pos, n - pos, page + headerKind, pageSize, &used, &rule);
        if (c <= 0) break;
        if (headerKind >= 4) { const int32_t v = c; memcpy(page, &v, 4); }
        if (headerKind == 8) { const int32_t v = used; memcpy(page + 4, &v, 4); }
        srcLen[k] = used; compLen[k] = c; rules[k] = rule;
        k++;
        pos += used;
        if (pos >= n || used == 0) break;
    }
    *consumedOut = pos;
    return k;
}

#ifdef FILL_MODEL_MAIN
/* strict decode of one block into out[0..cap): the decoded size, or -1 */
static int decode_block(const uint8_t *in, int inLen, uint8_t *out, int cap)
{
    int ip = 0, op = 0;
    for (;;) {
        uint32_t tok, len, off;
        if (ip >= inLen) return -1;
        tok = in[ip++];
        len = tok >> 4;
        if (len == 15) { uint32_t b; do { if (ip >= inLen) return -1; b = in[ip++]; len += b; } while (b == 255); }
        if ((long)ip + len > inLen || (long)op + len > cap) return -1;
        memcpy(out + op, in + ip, len); ip += (int)len; op += (int)len;
        if (ip == inLen) return op;
        if (ip + 2 > inLen) return -1;
        off = in[ip] | ((uint32_t)in[ip + 1] << 8); ip += 2;
        if (off == 0 || off > (uint32_t)op) return -1;
        len = tok & 15;
        if (len == 15) { uint32_t b; do { if (ip >= inLen) return -1; b = in[ip++]; len += b; } while (b == 255); }
        len += MINMATCH;
        if ((long)op + len > cap) return -1;
        for (uint32_t i = 0; i < len; i++, op++) out[op] = out[op - (int)off];
    }
}

static uint32_t lcg(uint32_t *s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

static void make_input(int kind, uint8_t *b, int n, uint32_t seed)
{
    static const char *words[] = {"page", "sector", "cluster", "frame", "record", "the", "of", "table", "store", "a"};
    int i = 0;
    switch (kind) {
    case 0: memset(b, 0, (size_t)n); break;
    case 1: for (i = 0; i < n; i++) b[i] = (uint8_t)lcg(&seed); break;
    case 2: while (i < n) { const char *w = words[lcg(&seed) % 10]; for (; *w && i < n; w++) b[i++] = (uint8_t)*w; if (i < n) b[i++] = ' '; } break;
    case 3: for (i = 0; i < n; i++) b[i] = (uint8_t)"abcdefg"[i % 7]; break;
    default:
        for (i = 0; i < n && i < 300; i++) b[i] = (uint8_t)lcg(&seed);
        for (; i < n && i < 1000; i++) b[i] = 0;
        make_input(2, b + i, n - i, seed);
    }
}

/* part of the grid under the sanitizers: every page of every chain lies in a buffer of exactly its size, decodes to exactly the
 * bytes it says it holds, and the chain consumes the input */
int main(void)
{
    static const int lens[] = {0, 1, 12, 13, 14, 100, 2048, 65000, 70000};
    long pagesSeen = 0, counts[5] = {0, 0, 0, 0, 0};
    for (int kind = 0; kind < 5; kind++)
        for (unsigned li = 0; li < sizeof lens / sizeof lens[0]; li++) {
            const int n = lens[li];
            uint8_t *src = (uint8_t *)malloc((size_t)n + 1), *dec = (uint8_t *)malloc((size_t)n + 1);
            make_input(kind, src, n, 12345u + (uint32_t)kind);
            const int step = n > 4096 ? 37 : 1;
            for (int T = 0; T <= 600; T += step) {
                uint8_t *page = (uint8_t *)malloc((size_t)(T > 0 ? T : 1));     /* exactly the page: a byte past it is an ASan report */
                int pos = 0;
                for (int k = 0; k < 100000; k++) {
                    int used = -1, rule = -1;
                    const int c = fill_model_page(src + pos, n - pos, page, T, &used, &rule);
                    if (T < 1) { if (c != 0) { printf("FAIL: T=%d returned %d\n", T, c); return 1; } break; }
                    if (c < 1 || c > T || used < 0 || used > n - pos) { printf("FAIL: kind %d n %d T %d page %d: c %d used %d\n", kind, n, T, k, c, used); return 1; }
                    if (decode_block(page, c, dec, used) != used || memcmp(dec, src + pos, (size_t)used)) {
                        printf("FAIL: kind %d n %d T %d page %d does not decode to its %d bytes\n", kind, n, T, k, used);
                        return 1;
                    }
                    if (used < n - pos && T > 1 && used < (T - 1) - (T + 240) / 256) { printf("FAIL: progress, T %d used %d\n", T, used); return 1; }
                    pagesSeen++; counts[rule]++;
                    pos += used;
                    if (pos >= n || used == 0) break;
                }
                if (T > 1 && pos != n) { printf("FAIL: kind %d n %d T %d: chain consumed %d\n", kind, n, T, pos); return 1; }
                free(page);
            }
            free(src); free(dec);
        }
    printf("fill_model: %ld pages ok; rules none %ld literal-rewind %ld token-rewind %ld short-match %ld adapted-last-run %ld\n",
           pagesSeen, counts[0], counts[1], counts[2], counts[3], counts[4]);
    return 0;
}
#endif
