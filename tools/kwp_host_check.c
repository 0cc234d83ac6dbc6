/*
 * kwp_host_check.c -- the host layer's key wrap with padding (uaesh_kwp_wrap / uaesh_kwp_unwrap, csrc/uaes_host.c) in a
 * program of its own, for a sanitizer build: uaes_host.c links without the engine, given the tables and a key schedule,
 * which this file makes itself (GF(2^8) S-box, FIPS-197 key expansion and the equivalent inverse cipher's keys).
 *
 *   cc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I micro-aes_amd/csrc \
 *      tools/kwp_host_check.c micro-aes_amd/csrc/uaes_host.c -o kwp_host_check && ./kwp_host_check
 *
 * Every buffer is malloc'ed at exactly its documented size, so a byte read behind a short secret or written behind the
 * 8 ceil(len / 8) + 8 bytes of a wrapped form is reported.  Checked: the two vectors of RFC 5649 section 6; every
 * length 1 .. 40 under the three key sizes, wrap, unwrap and the in-place form; every forgery class (a wrong constant,
 * RFC 3394's constant, a length indicator of 0, 8 (n - 1), 8 n + 1, 2^32 - 1, a non-zero byte at the first and the last
 * position of the fill, a flipped bit in A, in the last semiblock and in the key); the refused lengths.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "uaes_host.h"

static uint8_t sbox[256];
static uint32_t te0[256], td0[256];

static uint8_t xtime(uint8_t x) { return (uint8_t)((x << 1) ^ ((x >> 7) * 0x1b)); }

static uint8_t gmul(uint8_t a, uint8_t b)
{
    uint8_t r = 0;
    for (; b; b >>= 1, a = xtime(a)) if (b & 1) r ^= a;
    return r;
}

static void make_tables(void)
{
    uint8_t isbox[256];
    int i, k;
    for (i = 0; i < 256; ++i) {
        uint8_t inv = 0, s, r;
        for (k = 1; k < 256 && i; ++k) if (gmul((uint8_t)i, (uint8_t)k) == 1) { inv = (uint8_t)k; break; }
        s = r = inv;
        for (k = 0; k < 4; ++k) { r = (uint8_t)((r << 1) | (r >> 7)); s ^= r; }
        sbox[i] = s ^ 0x63;
        isbox[sbox[i]] = (uint8_t)i;
    }
    for (i = 0; i < 256; ++i) {
        const uint8_t s = sbox[i], v = isbox[i];
        te0[i] = (uint32_t)gmul(s, 2) | (uint32_t)s << 8 | (uint32_t)s << 16 | (uint32_t)gmul(s, 3) << 24;
        td0[i] = (uint32_t)gmul(v, 14) | (uint32_t)gmul(v, 9) << 8 | (uint32_t)gmul(v, 13) << 16 | (uint32_t)gmul(v, 11) << 24;
    }
    uaesh_tables_init(te0, td0);
}

static uint32_t subword(uint32_t w)
{
    return (uint32_t)sbox[w & 255] | (uint32_t)sbox[(w >> 8) & 255] << 8 | (uint32_t)sbox[(w >> 16) & 255] << 16 |
           (uint32_t)sbox[w >> 24] << 24;
}

static uint32_t inv_mix(uint32_t w)
{
    uint32_t r = 0;
    int b;
    for (b = 0; b < 4; ++b) {
        const uint8_t x = (uint8_t)(w >> (8 * b));
        const uint32_t t = (uint32_t)gmul(x, 14) | (uint32_t)gmul(x, 9) << 8 | (uint32_t)gmul(x, 13) << 16 | (uint32_t)gmul(x, 11) << 24;
        r ^= b ? (t << (8 * b)) | (t >> (32 - 8 * b)) : t;
    }
    return r;
}

typedef struct { uint32_t ek[60], dk[60]; uaesh_key k; } sched;

static void expand(sched *s, const uint8_t *key, int bits)
{
    const int nk = bits / 32, nr = nk + 6;
    uint8_t rcon = 1;
    int i, c;
    memset(s, 0, sizeof *s);
    memcpy(s->ek, key, (size_t)(4 * nk));               /* little-endian hosts only, as the engine */
    for (i = nk; i < 4 * (nr + 1); ++i) {
        uint32_t t = s->ek[i - 1];
        if (i % nk == 0) { t = subword((t >> 8) | (t << 24)) ^ rcon; rcon = xtime(rcon); }
        else if (nk == 8 && i % nk == 4) t = subword(t);
        s->ek[i] = s->ek[i - nk] ^ t;
    }
    for (c = 0; c < 4; ++c) { s->dk[c] = s->ek[4 * nr + c]; s->dk[4 * nr + c] = s->ek[c]; }
    for (i = 1; i < nr; ++i)
        for (c = 0; c < 4; ++c) s->dk[4 * i + c] = inv_mix(s->ek[4 * (nr - i) + c]);
    s->k.ek = s->ek; s->k.dk = s->dk; s->k.nr = nr;
}

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static void *dup_exact(const void *p, size_t n)
{
    void *q = malloc(n ? n : 1);
    if (n) memcpy(q, p, n);
    return q;
}

/* RFC 5649's wrap with ANY A and ANY whole semiblocks (n of them at `padded`): what forgeries are made of */
static void wrap_raw(const uaesh_key *k, const uint8_t a8[8], const uint8_t *padded, size_t n, uint8_t *out)
{
    uint8_t b[16];
    size_t i, j;
    int x;
    memcpy(b, a8, 8);
    if (n == 1) { memcpy(b + 8, padded, 8); uaesh_encrypt(k->ek, k->nr, b, out); return; }
    memcpy(out + 8, padded, 8 * n);
    for (j = 0; j < 6; ++j)
        for (i = 0; i < n; ++i) {
            uint64_t t = n * j + i + 1;
            memcpy(b + 8, out + 8 + 8 * i, 8);
            uaesh_encrypt(k->ek, k->nr, b, b);
            for (x = 7; x >= 0; --x, t >>= 8) b[x] ^= (uint8_t)t;
            memcpy(out + 8 + 8 * i, b + 8, 8);
        }
    memcpy(out, b, 8);
}

static void must_fail(const uaesh_key *k, const uint8_t *w, size_t wl)
{
    uint8_t *in = dup_exact(w, wl), *out = malloc(wl - 8);
    uint32_t mli = 77;
    CHECK(uaesh_kwp_unwrap(k, in, wl, out, &mli) == 0x1A && mli == 0);
    free(in); free(out);
}

static void forge(const uaesh_key *k, const uint8_t *secret, size_t m)
{
    const size_t n = (m + 7) / 8, wl = 8 * n + 8;
    uint8_t *padded = calloc(n, 8), *w = malloc(wl), a[8] = { 0xA6, 0x59, 0x59, 0xA6 };
    const uint32_t mlis[5] = { (uint32_t)m, 0, (uint32_t)(8 * (n - 1)), (uint32_t)(8 * n + 1), 0xFFFFFFFFu };
    int i;
    memcpy(padded, secret, m);
    for (i = 0; i < 5; ++i) {
        a[4] = (uint8_t)(mlis[i] >> 24); a[5] = (uint8_t)(mlis[i] >> 16); a[6] = (uint8_t)(mlis[i] >> 8); a[7] = (uint8_t)mlis[i];
        if (i == 0) {                                  /* the right length indicator: a wrong constant, a dirty fill */
            a[3] ^= 1; wrap_raw(k, a, padded, n, w); must_fail(k, w, wl); a[3] ^= 1;
            if (m < 8 * n) {
                padded[m] = 1; wrap_raw(k, a, padded, n, w); must_fail(k, w, wl); padded[m] = 0;
                padded[8 * n - 1] = 0x80; wrap_raw(k, a, padded, n, w); must_fail(k, w, wl); padded[8 * n - 1] = 0;
            }
            wrap_raw(k, a, padded, n, w);              /* and the real thing, with a bit flipped in A and in R_n */
            w[0] ^= 0x20; must_fail(k, w, wl); w[0] ^= 0x20;
            w[wl - 1] ^= 0x40; must_fail(k, w, wl); w[wl - 1] ^= 0x40;
        } else {
            wrap_raw(k, a, padded, n, w); must_fail(k, w, wl);
        }
    }
    memset(a, 0xA6, 8); wrap_raw(k, a, padded, n, w); must_fail(k, w, wl);
    free(padded); free(w);
}

int main(void)
{
    static const uint8_t rfc_kek[24] = { 0x58, 0x40, 0xdf, 0x6e, 0x29, 0xb0, 0x2a, 0xf1, 0xab, 0x49, 0x3b, 0x70, 0x5b, 0xf1, 0x6e, 0xa1,
                                         0xae, 0x83, 0x38, 0xf4, 0xdc, 0xc1, 0x76, 0xa8 };
    static const uint8_t rfc_20[20] = { 0xc3, 0x7b, 0x7e, 0x64, 0x92, 0x58, 0x43, 0x40, 0xbe, 0xd1, 0x22, 0x07, 0x80, 0x89, 0x41, 0x15,
                                        0x50, 0x68, 0xf7, 0x38 };
    static const uint8_t rfc_20w[32] = { 0x13, 0x8b, 0xde, 0xaa, 0x9b, 0x8f, 0xa7, 0xfc, 0x61, 0xf9, 0x77, 0x42, 0xe7, 0x22, 0x48, 0xee,
                                         0x5a, 0xe6, 0xae, 0x53, 0x60, 0xd1, 0xae, 0x6a, 0x5f, 0x54, 0xf3, 0x73, 0xfa, 0x54, 0x3b, 0x6a };
    static const uint8_t rfc_7[7] = { 0x46, 0x6f, 0x72, 0x50, 0x61, 0x73, 0x69 };
    static const uint8_t rfc_7w[16] = { 0xaf, 0xbe, 0xb0, 0xf0, 0x7d, 0xfb, 0xf5, 0x41, 0x92, 0x00, 0xf2, 0xcc, 0xb5, 0x0b, 0xb2, 0x4f };
    sched s;
    uint8_t key[32], w32[32];
    uint32_t mli = 0, seed = 5649;
    int bits, i;
    size_t m;
    make_tables();
    expand(&s, rfc_kek, 192);
    CHECK(uaesh_kwp_wrap(&s.k, rfc_20, 20, w32) == 0 && !memcmp(w32, rfc_20w, 32));
    CHECK(uaesh_kwp_wrap(&s.k, rfc_7, 7, w32) == 0 && !memcmp(w32, rfc_7w, 16));
    CHECK(uaesh_kwp_wrap(&s.k, rfc_7, 0, w32) == 1 && uaesh_kwp_unwrap(&s.k, rfc_7w, 8, w32, &mli) == 1);
    CHECK(uaesh_kwp_unwrap(&s.k, rfc_20w, 20, w32, &mli) == 1 && uaesh_kwp_unwrap(&s.k, rfc_20w, 0, w32, &mli) == 1);
    for (bits = 128; bits <= 256; bits += 64) {
        for (i = 0; i < 32; ++i) { seed = seed * 1664525u + 1013904223u; key[i] = (uint8_t)(seed >> 24); }
        expand(&s, key, bits);
        for (m = 1; m <= 40; ++m) {
            const size_t wl = 8 * ((m + 7) / 8) + 8;
            uint8_t *secret = malloc(m), *wrapped = malloc(wl), *back = malloc(wl - 8), *both = malloc(wl), *flip;
            sched s2;
            for (i = 0; i < (int)m; ++i) { seed = seed * 1664525u + 1013904223u; secret[i] = (uint8_t)(seed >> 24); }
            CHECK(uaesh_kwp_wrap(&s.k, secret, m, wrapped) == 0);
            CHECK(uaesh_kwp_unwrap(&s.k, wrapped, wl, back, &mli) == 0 && mli == m && !memcmp(back, secret, m));
            for (i = (int)m; i < (int)(wl - 8); ++i) CHECK(back[i] == 0);
            memset(both, 0x5c, wl);                    /* in place: the secret 8 bytes into the wrapped buffer */
            memcpy(both + 8, secret, m);
            CHECK(uaesh_kwp_wrap(&s.k, both + 8, m, both) == 0 && !memcmp(both, wrapped, wl));
            CHECK(uaesh_kwp_unwrap(&s.k, both, wl, both + 8, &mli) == 0 && mli == m && !memcmp(both + 8, secret, m));
            forge(&s.k, secret, m);
            key[2] ^= 2; expand(&s2, key, bits); key[2] ^= 2;          /* a bit flipped in the key */
            flip = dup_exact(wrapped, wl);
            CHECK(uaesh_kwp_unwrap(&s2.k, flip, wl, back, &mli) == 0x1A && mli == 0);
            free(secret); free(wrapped); free(back); free(both); free(flip);
        }
    }
    printf(failures ? "kwp_host_check: %d FAILED\n" : "kwp_host_check: ok\n", failures);
    return failures != 0;
}
