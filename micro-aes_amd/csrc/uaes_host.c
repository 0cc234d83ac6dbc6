/*
 * uaes_host.c -- the engine's OWN host data path: portable C, table-driven, re-entrant, run-time key size.
 *
 * NOT the default path and not a silent fallback: every entry point of libuaes_hip.so runs on the GPU and fails loudly
 * without one unless the deployer has switched this path on (uaes_set_host_policy / UAES_HOST_MAX, UAES_HOST_CHAINS,
 * UAES_HOST_FALLBACK; include/uaes_hip.h).  It exists for the three places where a GPU cannot serve a caller of the
 * reference well (SURVEY.md 8b "Errors"): host-pointer calls too short to amortise a launch, ONE serial
 * chain (CBC / CFB encryption, OFB, CMAC, CCM's CBC-MAC, key wrap, FF1: a latency-bound single wave on the GPU), and a `void` function
 * of the drop-in API on a box whose GPU has gone away.
 *
 * Product code, parity-tested like a kernel (tests/test_host_path.py runs the reference-held vectors and the golden
 * fixtures through it); it shares nothing with oracle/ (test infrastructure).  The arithmetic is the classic 32-bit
 * T-table formulation on the tables the engine derives from GF(2^8) anyway (uaes_engine.c, build_host_tables) and a
 * 4-bit-table GHASH; the semantics are the reference's, cited function by function.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "uaes_host.h"

/* ---- tables ------------------------------------------------------------ */
static uint32_t TE[4][256], TD[4][256];
static uint8_t  SB[256], ISB[256];

static uint32_t rol32(uint32_t v, unsigned n) { return n ? (v << n) | (v >> (32 - n)) : v; }

/* te0[x] = bytes {2S, S, S, 3S}[x], td0[x] = bytes {14Si, 9Si, 13Si, 11Si}[x] (little-endian words: byte 0 lowest).
 * Te_k = rotl(Te0, 8k) serves the byte of row k; S and Si fall out of the tables themselves.                       */
void uaesh_tables_init(const uint32_t te0[256], const uint32_t td0[256])
{
    unsigned x, k;
    for (x = 0; x < 256; ++x) {
        for (k = 0; k < 4; ++k) {
            TE[k][x] = rol32(te0[x], 8 * k);
            TD[k][x] = rol32(td0[x], 8 * k);
        }
        SB[x] = (uint8_t)(te0[x] >> 8);
    }
    for (x = 0; x < 256; ++x) ISB[SB[x]] = (uint8_t)x;
}

static uint32_t ld32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
static void st32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

/* ---- the block cipher (rijndaelEncrypt / rijndaelDecrypt, micro_aes.c:242-259, :315-332) ------------------------
 * State = four little-endian column words (byte r of word c = state[c][r], FIPS-197 order, a1 of SURVEY.md 8a).  One
 * round = SubBytes + ShiftRows + MixColumns as four lookups per column + AddRoundKey; the last round has no MixColumns. */
void uaesh_encrypt(const uint32_t *ek, int nr, const uint8_t in[16], uint8_t out[16])
{
    uint32_t s0 = ld32(in) ^ ek[0], s1 = ld32(in + 4) ^ ek[1], s2 = ld32(in + 8) ^ ek[2], s3 = ld32(in + 12) ^ ek[3];
    uint32_t t0, t1, t2, t3;
    int r;
    for (r = 1; r < nr; ++r) {
        const uint32_t *k = ek + 4 * r;
        t0 = TE[0][s0 & 255] ^ TE[1][(s1 >> 8) & 255] ^ TE[2][(s2 >> 16) & 255] ^ TE[3][s3 >> 24] ^ k[0];
        t1 = TE[0][s1 & 255] ^ TE[1][(s2 >> 8) & 255] ^ TE[2][(s3 >> 16) & 255] ^ TE[3][s0 >> 24] ^ k[1];
        t2 = TE[0][s2 & 255] ^ TE[1][(s3 >> 8) & 255] ^ TE[2][(s0 >> 16) & 255] ^ TE[3][s1 >> 24] ^ k[2];
        t3 = TE[0][s3 & 255] ^ TE[1][(s0 >> 8) & 255] ^ TE[2][(s1 >> 16) & 255] ^ TE[3][s2 >> 24] ^ k[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    {
        const uint32_t *k = ek + 4 * nr;
        t0 = ((uint32_t)SB[s0 & 255] | (uint32_t)SB[(s1 >> 8) & 255] << 8 | (uint32_t)SB[(s2 >> 16) & 255] << 16 | (uint32_t)SB[s3 >> 24] << 24) ^ k[0];
        t1 = ((uint32_t)SB[s1 & 255] | (uint32_t)SB[(s2 >> 8) & 255] << 8 | (uint32_t)SB[(s3 >> 16) & 255] << 16 | (uint32_t)SB[s0 >> 24] << 24) ^ k[1];
        t2 = ((uint32_t)SB[s2 & 255] | (uint32_t)SB[(s3 >> 8) & 255] << 8 | (uint32_t)SB[(s0 >> 16) & 255] << 16 | (uint32_t)SB[s1 >> 24] << 24) ^ k[2];
        t3 = ((uint32_t)SB[s3 & 255] | (uint32_t)SB[(s0 >> 8) & 255] << 8 | (uint32_t)SB[(s1 >> 16) & 255] << 16 | (uint32_t)SB[s2 >> 24] << 24) ^ k[3];
    }
    st32(out, t0); st32(out + 4, t1); st32(out + 8, t2); st32(out + 12, t3);
}

/* the equivalent inverse cipher (FIPS-197 5.3.5) on dk[0] = ek[nr], dk[i] = InvMixColumns(ek[nr - i]), dk[nr] = ek[0]:
 * column c takes row r from column (c - r) mod 4                                                                    */
void uaesh_decrypt(const uint32_t *dk, int nr, const uint8_t in[16], uint8_t out[16])
{
    uint32_t s0 = ld32(in) ^ dk[0], s1 = ld32(in + 4) ^ dk[1], s2 = ld32(in + 8) ^ dk[2], s3 = ld32(in + 12) ^ dk[3];
    uint32_t t0, t1, t2, t3;
    int r;
    for (r = 1; r < nr; ++r) {
        const uint32_t *k = dk + 4 * r;
        t0 = TD[0][s0 & 255] ^ TD[1][(s3 >> 8) & 255] ^ TD[2][(s2 >> 16) & 255] ^ TD[3][s1 >> 24] ^ k[0];
        t1 = TD[0][s1 & 255] ^ TD[1][(s0 >> 8) & 255] ^ TD[2][(s3 >> 16) & 255] ^ TD[3][s2 >> 24] ^ k[1];
        t2 = TD[0][s2 & 255] ^ TD[1][(s1 >> 8) & 255] ^ TD[2][(s0 >> 16) & 255] ^ TD[3][s3 >> 24] ^ k[2];
        t3 = TD[0][s3 & 255] ^ TD[1][(s2 >> 8) & 255] ^ TD[2][(s1 >> 16) & 255] ^ TD[3][s0 >> 24] ^ k[3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    {
        const uint32_t *k = dk + 4 * nr;
        t0 = ((uint32_t)ISB[s0 & 255] | (uint32_t)ISB[(s3 >> 8) & 255] << 8 | (uint32_t)ISB[(s2 >> 16) & 255] << 16 | (uint32_t)ISB[s1 >> 24] << 24) ^ k[0];
        t1 = ((uint32_t)ISB[s1 & 255] | (uint32_t)ISB[(s0 >> 8) & 255] << 8 | (uint32_t)ISB[(s3 >> 16) & 255] << 16 | (uint32_t)ISB[s2 >> 24] << 24) ^ k[1];
        t2 = ((uint32_t)ISB[s2 & 255] | (uint32_t)ISB[(s1 >> 8) & 255] << 8 | (uint32_t)ISB[(s0 >> 16) & 255] << 16 | (uint32_t)ISB[s3 >> 24] << 24) ^ k[2];
        t3 = ((uint32_t)ISB[s3 & 255] | (uint32_t)ISB[(s2 >> 8) & 255] << 8 | (uint32_t)ISB[(s1 >> 16) & 255] << 16 | (uint32_t)ISB[s0 >> 24] << 24) ^ k[3];
    }
    st32(out, t0); st32(out + 4, t1); st32(out + 8, t2); st32(out + 12, t3);
}

static void xor16(uint8_t *d, const uint8_t *a, const uint8_t *b)
{
    int i;
    for (i = 0; i < 16; ++i) d[i] = a[i] ^ b[i];
}

/* ---- ECB (AES_ECB_encrypt / _decrypt, micro_aes.c:636-680; padBlock :610-621; N1) ------------------------------- */
void uaesh_ecb_encrypt(const uaesh_key *k, int padding, const uint8_t *in, size_t len, uint8_t *out)
{
    const size_t nfull = len / 16, rem = len % 16;
    size_t i;
    for (i = 0; i < nfull; ++i) uaesh_encrypt(k->ek, k->nr, in + 16 * i, out + 16 * i);
    if (rem || padding) {                           /* zeros behind a partial block; PKCS#7 / ISO 7816-4 always append */
        uint8_t b[16];
        const uint8_t n = (uint8_t)(16 - rem);
        memcpy(b, in + 16 * nfull, rem);
        memset(b + rem, padding == 1 ? n : 0, n);
        if (padding == 2) b[rem] = 0x80;
        uaesh_encrypt(k->ek, k->nr, b, out + 16 * nfull);
    }
}

void uaesh_ecb_decrypt(const uaesh_key *k, const uint8_t *in, size_t len, uint8_t *out)
{
    const size_t nfull = len / 16;
    size_t i;
    for (i = 0; i < nfull; ++i) uaesh_decrypt(k->dk, k->nr, in + 16 * i, out + 16 * i);
    if (len % 16 && out != in) memmove(out + 16 * nfull, in + 16 * nfull, len % 16);   /* the tail passes through (:664) */
}

/* ---- CTR (CTR_cipher micro_aes.c:919-950; incBlock :421-427; N2, N3) --------------------------------------------- */
/* counter block of stream block i: bytes 0..8 of ctr0 fixed, bytes 9..15 a 56-bit big-endian integer + block_offset + i */
static void ctr_block(uint8_t c[16], const uint8_t ctr0[16], uint64_t v)
{
    int i;
    memcpy(c, ctr0, 9);
    for (i = 15; i >= 9; --i, v >>= 8) c[i] = (uint8_t)v;
}

void uaesh_ctr(const uaesh_key *k, const uint8_t ctr0[16], uint64_t block_offset, const uint8_t *in, size_t len, uint8_t *out)
{
    uint64_t v = 0;
    uint8_t c[16], ks[16];
    size_t off, i;
    for (i = 9; i < 16; ++i) v = (v << 8) | ctr0[i];
    v += block_offset;
    for (off = 0; off < len; off += 16, ++v) {
        const size_t n = len - off < 16 ? len - off : 16;
        ctr_block(c, ctr0, v & 0x00FFFFFFFFFFFFFFull);
        uaesh_encrypt(k->ek, k->nr, c, ks);
        for (i = 0; i < n; ++i) out[off + i] = in[off + i] ^ ks[i];
    }
}

/* ---- XTS (XTS_cipher micro_aes.c:1008-1055; doubleLblock :449-458; N5) -------------------------------------------- */
static void xts_double(uint8_t t[16])
{
    unsigned c = 0;
    int i;
    for (i = 0; i < 16; ++i) {
        c |= (unsigned)t[i] << 1;
        t[i] = (uint8_t)c;
        c >>= 8;
    }
    t[0] ^= (uint8_t)(c * 0x87);
}

static void xex(const uaesh_key *k1, int encrypt, const uint8_t t[16], const uint8_t *in, uint8_t *out)
{
    uint8_t b[16];
    xor16(b, in, t);
    if (encrypt) uaesh_encrypt(k1->ek, k1->nr, b, b); else uaesh_decrypt(k1->dk, k1->nr, b, b);
    xor16(out, b, t);
}

/* one data unit, len >= 16; tweak = the sixteen raw bytes of the unit's identifier */
void uaesh_xts_unit(const uaesh_key *k1, const uaesh_key *k2, int encrypt, const uint8_t tweak[16],
                    const uint8_t *in, size_t len, uint8_t *out)
{
    const size_t r = len % 16, n = len / 16 - (r ? 1 : 0);
    uint8_t t[16];
    size_t i;
    uaesh_encrypt(k2->ek, k2->nr, tweak, t);
    for (i = 0; i < n; ++i) {
        xex(k1, encrypt, t, in + 16 * i, out + 16 * i);
        xts_double(t);
    }
    if (r) {                                        /* ciphertext stealing: decryption uses the last two tweaks swapped */
        uint8_t l[16], x[16], last[16];
        const uint8_t *px = in + 16 * n;
        uint8_t *py = out + 16 * n;
        memcpy(l, t, 16);
        xts_double(encrypt ? t : l);                /* encrypt: L = T_n, T = T_{n+1}; decrypt: L = T_{n+1}, T = T_n */
        xex(k1, encrypt, l, px, x);                 /* the last full block under L */
        memcpy(last, px + 16, r);                   /* the ragged chunk ... */
        memcpy(last + r, x + r, 16 - r);            /* ... completed with the tail it 'steals' */
        memcpy(py + 16, x, r);                      /* head of X becomes the final partial chunk */
        xex(k1, encrypt, t, last, py);
    }
}

void uaesh_xts_sectors(const uaesh_key *k1, const uaesh_key *k2, int encrypt, uint64_t first_sector, size_t sector_bytes,
                       size_t nsectors, const uint8_t *in, uint8_t *out)
{
    size_t s;
    for (s = 0; s < nsectors; ++s) {
        uint8_t tw[16] = { 0 };
        uint64_t id = first_sector + s;
        int i;
        for (i = 0; i < 8; ++i, id >>= 8) tw[i] = (uint8_t)id;          /* LE128(sector id): copyLint, :399-404 */
        uaesh_xts_unit(k1, k2, encrypt, tw, in + s * sector_bytes, sector_bytes, out + s * sector_bytes);
    }
}

/* ---- GHASH (mulGF128 micro_aes.c:476-493, xMac :551-570, gHash :1127-1137; N6) ------------------------------------
 * GCM's field: bit 0 of byte 0 is the coefficient of x^0, so "times x" is a right shift of the big-endian 128-bit
 * value, folding 0xE1 << 120 in when a bit falls off.  4-bit tables: M[n] = n(x) * H for the sixteen nibble values
 * (nibble bit 8 = the lowest power); Y * H = Horner over the 32 nibbles from the last one down, Z <- Z * x^4 ^ M[n].   */
typedef struct { uint64_t hi, lo; } gf128;
typedef struct { gf128 m[16]; uint64_t red[16]; } ghash_key;

static gf128 gf_mulx(gf128 v)
{
    const uint64_t carry = v.lo & 1;
    v.lo = (v.lo >> 1) | (v.hi << 63);
    v.hi = (v.hi >> 1) ^ (carry ? 0xE100000000000000ull : 0);
    return v;
}

static uint64_t be64(const uint8_t *p)
{
    uint64_t v = 0;
    int i;
    for (i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}

static void put_be64(uint8_t *p, uint64_t v)
{
    int i;
    for (i = 7; i >= 0; --i, v >>= 8) p[i] = (uint8_t)v;
}

static void ghash_setup(ghash_key *g, const uint8_t h[16])
{
    gf128 v;
    unsigned n, b;
    v.hi = be64(h); v.lo = be64(h + 8);
    memset(g, 0, sizeof *g);
    g->m[8] = v;                                    /* x^0 */
    v = gf_mulx(v); g->m[4] = v;
    v = gf_mulx(v); g->m[2] = v;
    v = gf_mulx(v); g->m[1] = v;
    for (n = 3; n < 16; ++n) {
        if ((n & (n - 1)) == 0) continue;
        for (b = 1; b < 16; b <<= 1)
            if (n & b) { g->m[n].hi ^= g->m[b].hi; g->m[n].lo ^= g->m[b].lo; }
    }
    for (n = 0; n < 16; ++n) {                      /* what four bits falling off the low end fold back in */
        gf128 r;
        r.hi = 0; r.lo = n;
        r = gf_mulx(gf_mulx(gf_mulx(gf_mulx(r))));
        g->red[n] = r.hi;
    }
}

static void ghash_mul(const ghash_key *g, uint8_t y[16])
{
    gf128 z;
    int i;
    z = g->m[y[15] & 15];
    for (i = 15; i >= 0; --i) {
        unsigned rem;
        if (i != 15) {
            rem = (unsigned)z.lo & 15;
            z.lo = (z.lo >> 4) | (z.hi << 60);
            z.hi = (z.hi >> 4) ^ g->red[rem];
            z.hi ^= g->m[y[i] & 15].hi; z.lo ^= g->m[y[i] & 15].lo;
        }
        rem = (unsigned)z.lo & 15;
        z.lo = (z.lo >> 4) | (z.hi << 60);
        z.hi = (z.hi >> 4) ^ g->red[rem];
        z.hi ^= g->m[y[i] >> 4].hi; z.lo ^= g->m[y[i] >> 4].lo;
    }
    put_be64(y, z.hi); put_be64(y + 8, z.lo);
}

/* absorb: every 16 bytes Y <- (Y ^ X) * H; a partial last block is zero padded (xMac) */
static void ghash_absorb(const ghash_key *g, uint8_t y[16], const uint8_t *x, size_t len)
{
    size_t i;
    while (len >= 16) {
        for (i = 0; i < 16; ++i) y[i] ^= x[i];
        ghash_mul(g, y);
        x += 16; len -= 16;
    }
    if (len) {
        for (i = 0; i < len; ++i) y[i] ^= x[i];
        ghash_mul(g, y);
    }
}

static void ghash_lengths(const ghash_key *g, uint8_t y[16], uint64_t aad_len, uint64_t ct_len)
{
    uint8_t l[16];
    put_be64(l, aad_len * 8);
    put_be64(l + 8, ct_len * 8);
    ghash_absorb(g, y, l, 16);
}

void uaesh_ghash(const uint8_t h[16], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len, uint8_t out[16])
{
    ghash_key g;
    ghash_setup(&g, h);
    memset(out, 0, 16);
    ghash_absorb(&g, out, aad, aad_len);
    ghash_absorb(&g, out, ct, ct_len);
    ghash_lengths(&g, out, aad_len, ct_len);
    memset(&g, 0, sizeof g);
}

static int differ(const uint8_t *a, const uint8_t *b, size_t n)         /* constant time */
{
    unsigned d = 0;
    size_t i;
    for (i = 0; i < n; ++i) d |= (unsigned)(a[i] ^ b[i]);
    return d != 0;
}

/* ---- GCM (GCMsetup micro_aes.c:1140-1152, AES_GCM_encrypt :1164-1179, _decrypt :1192-1212; N4, N7) ----------------
 * J0 = nonce || 00000001 for a 12-byte nonce, else GHASH(nonce); keystream block i under J0 + 1 + i with the reference's
 * 56-bit increment; tag = Enc(J0) ^ GHASH(aad, ct), tag_len bytes of it.  decrypt: in = ct || tag; returns 0x1A and
 * writes nothing when the tag does not match.                                                                       */
int uaesh_gcm(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
              const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out)
{
    ghash_key g;
    uint8_t h[16] = { 0 }, j0[16] = { 0 }, ej0[16], y[16] = { 0 };
    int rc = 0;
    uaesh_encrypt(k->ek, k->nr, h, h);
    ghash_setup(&g, h);
    if (nonce_len == 12) {
        memcpy(j0, nonce, 12);
        j0[15] = 1;
    } else {
        ghash_absorb(&g, j0, nonce, nonce_len);
        ghash_lengths(&g, j0, 0, nonce_len);
    }
    uaesh_encrypt(k->ek, k->nr, j0, ej0);
    if (!decrypt) {
        uaesh_ctr(k, j0, 1, in, len, out);
        ghash_absorb(&g, y, aad, aad_len);
        ghash_absorb(&g, y, out, len);
        ghash_lengths(&g, y, aad_len, len);
        xor16(y, y, ej0);
        memcpy(out + len, y, tag_len);
    } else {
        ghash_absorb(&g, y, aad, aad_len);
        ghash_absorb(&g, y, in, len);
        ghash_lengths(&g, y, aad_len, len);
        xor16(y, y, ej0);
        if (differ(y, in + len, tag_len)) rc = 0x1A;
        else uaesh_ctr(k, j0, 1, in, len, out);
    }
    memset(&g, 0, sizeof g); memset(h, 0, 16); memset(ej0, 0, 16);
    return rc;
}

/* ---- CBC (AES_CBC_encrypt micro_aes.c:697-744, _decrypt :746-782) ------------------------------------------------- */
/* cts != 0: CS3 ciphertext stealing -- the last two blocks are always swapped, a text shorter than one block is
 * M_DATALENGTH_ERROR (1).  cts == 0: the CTS 0 build, last chunk padded like ECB's (padding = AES_PADDING).          */
int uaesh_cbc_encrypt(const uaesh_key *k, const uint8_t iv[16], int cts, int padding, const uint8_t *in, size_t len, uint8_t *out)
{
    size_t n = len / 16, r = len % 16, i;
    uint8_t chain[16], b[16];
    if (cts) {
        if (n > 1 && r == 0) { --n; r = 16; }
        if (n == 0) return 1;
    }
    memcpy(chain, iv, 16);
    for (i = 0; i < n; ++i) {
        xor16(b, in + 16 * i, chain);
        uaesh_encrypt(k->ek, k->nr, b, chain);
        if (!(cts && r && i == n - 1)) memcpy(out + 16 * i, chain, 16);
    }
    if (cts) {
        if (r) {                                    /* C_{n-1} = chain: its head goes LAST, Enc(C_{n-1} ^ pad0(P_n)) takes its place */
            uint8_t last[16] = { 0 };
            memcpy(last, in + 16 * n, r);
            xor16(b, last, chain);
            uaesh_encrypt(k->ek, k->nr, b, b);
            memcpy(last, chain, r);                 /* (in may be out: everything of block n has been read) */
            memcpy(out + 16 * (n - 1), b, 16);
            memcpy(out + 16 * n, last, r);
        }
    } else if (r || padding) {
        const uint8_t pad = (uint8_t)(16 - r);
        memcpy(b, in + 16 * n, r);
        memset(b + r, padding == 1 ? pad : 0, pad);
        if (padding == 2) b[r] = 0x80;
        xor16(b, b, chain);
        uaesh_encrypt(k->ek, k->nr, b, out + 16 * n);
    }
    return 0;
}

int uaesh_cbc_decrypt(const uaesh_key *k, const uint8_t iv[16], int cts, const uint8_t *in, size_t len, uint8_t *out)
{
    size_t n = len / 16, r = len % 16, i;
    uint8_t chain[16], c[16], b[16];
    if (cts) {
        if (n > 1 && r == 0) { --n; r = 16; }
        if (n == 0) return 1;
    } else if (r) {
        return 1;
    }
    if (r) --n;                                     /* the last two blocks are the stolen pair */
    memcpy(chain, iv, 16);
    for (i = 0; i < n; ++i) {
        memcpy(c, in + 16 * i, 16);
        uaesh_decrypt(k->dk, k->nr, c, b);
        xor16(out + 16 * i, b, chain);
        memcpy(chain, c, 16);
    }
    if (r) {                                        /* {X full, Z r bytes}: Y = Dec(X); P_n = Z ^ Y; P_{n-1} = Dec(Z | tail of Y) ^ chain */
        uint8_t x[16], z[16], y[16], p2[16];
        memcpy(x, in + 16 * n, 16);
        memcpy(z, in + 16 * n + 16, r);
        uaesh_decrypt(k->dk, k->nr, x, y);
        for (i = 0; i < r; ++i) p2[i] = y[i] ^ z[i];
        memcpy(z + r, y + r, 16 - r);
        uaesh_decrypt(k->dk, k->nr, z, b);
        xor16(out + 16 * n, b, chain);
        memcpy(out + 16 * n + 16, p2, r);
    }
    return 0;
}

/* ---- CFB (CFB_cipher micro_aes.c:799-817) and OFB (AES_OFB_encrypt :861-885) -------------------------------------- */
void uaesh_cfb(const uaesh_key *k, const uint8_t iv[16], int encrypt, const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t chain[16], ks[16], c[16];
    size_t off, i;
    memcpy(chain, iv, 16);
    for (off = 0; off < len; off += 16) {
        const size_t n = len - off < 16 ? len - off : 16;
        uaesh_encrypt(k->ek, k->nr, chain, ks);
        memcpy(c, in + off, n);
        for (i = 0; i < n; ++i) out[off + i] = c[i] ^ ks[i];
        memcpy(chain, encrypt ? out + off : c, n);  /* the next input of the cipher is the CIPHERTEXT block */
    }
}

void uaesh_ofb(const uaesh_key *k, const uint8_t iv[16], const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t chain[16];
    size_t off, i;
    memcpy(chain, iv, 16);
    for (off = 0; off < len; off += 16) {
        const size_t n = len - off < 16 ? len - off : 16;
        uaesh_encrypt(k->ek, k->nr, chain, chain);
        for (i = 0; i < n; ++i) out[off + i] = in[off + i] ^ chain[i];
    }
}

/* ---- CMAC (AES_CMAC micro_aes.c:1108-1118, cMac :576-591, getSubkeys :594-605, doubleBblock :432-443) ------------- */
static void cmac_double(uint8_t b[16])
{
    unsigned c = 0;
    int i;
    for (i = 15; i >= 0; --i) {
        c |= (unsigned)b[i] << 1;
        b[i] = (uint8_t)c;
        c >>= 8;
    }
    b[15] ^= (uint8_t)(c * 0x87);
}

void uaesh_cmac(const uaesh_key *k, const uint8_t *data, size_t len, uint8_t mac[16])
{
    uint8_t k1[16] = { 0 }, k2[16], last[16] = { 0 };
    const size_t s = len ? (len - 1) % 16 + 1 : 0;  /* bytes of the last block: 1..16, 0 for the empty message */
    size_t off, i;
    uaesh_encrypt(k->ek, k->nr, k1, k1);
    cmac_double(k1);
    memcpy(k2, k1, 16);
    cmac_double(k2);
    memset(mac, 0, 16);
    for (off = 0; off + s < len; off += 16) {
        for (i = 0; i < 16; ++i) mac[i] ^= data[off + i];
        uaesh_encrypt(k->ek, k->nr, mac, mac);
    }
    memcpy(last, data + (len - s), s);
    if (s < 16) last[s] = 0x80;
    for (i = 0; i < 16; ++i) mac[i] ^= last[i] ^ (s < 16 ? k2[i] : k1[i]);
    uaesh_encrypt(k->ek, k->nr, mac, mac);
    memset(k1, 0, 16); memset(k2, 0, 16);
}

/* ---- CCM (CCMtag micro_aes.c:1226-1262, AES_CCM_encrypt :1268-1282, _decrypt :1294-1314) -------------------------- */
static void cbcmac_absorb(const uaesh_key *k, uint8_t m[16], const uint8_t *x, size_t len)
{
    size_t i;
    while (len) {
        const size_t n = len < 16 ? len : 16;
        for (i = 0; i < n; ++i) m[i] ^= x[i];
        uaesh_encrypt(k->ek, k->nr, m, m);
        x += n; len -= n;
    }
}

static void ccm_tag(const uaesh_key *k, const uint8_t iv[16], size_t tag_len, const uint8_t *aad, size_t aad_len,
                    const uint8_t *text, size_t len, uint8_t tag[16])
{
    uint8_t m[16], a[16] = { 0 }, s0[16];
    size_t v = len;
    int pos = 15;
    memcpy(m, iv, 16);
    m[0] |= (uint8_t)((tag_len - 2) << 2);
    do m[pos--] ^= (uint8_t)v; while ((v >>= 8) != 0);                  /* the text length, big-endian, ending at byte 15 */
    if (aad_len) {
        size_t p = 1, take;
        m[0] |= 0x40;
        uaesh_encrypt(k->ek, k->nr, m, m);
        if (aad_len > 0xFEFFu) { p = 5; a[0] = 0xFF; a[1] = 0xFE; }
        v = aad_len; pos = (int)p;
        do a[pos--] ^= (uint8_t)v; while ((v >>= 8) != 0);              /* the AAD length in front of the AAD */
        ++p;
        take = aad_len < 16 - p ? aad_len : 16 - p;
        memcpy(a + p, aad, take);
        cbcmac_absorb(k, m, a, 16);
        cbcmac_absorb(k, m, aad + take, aad_len - take);
    } else {
        cbcmac_absorb(k, m, a, 16);                                     /* the reference digests its zero A block (xMac of 16 bytes) */
    }
    cbcmac_absorb(k, m, text, len);
    uaesh_encrypt(k->ek, k->nr, iv, s0);
    xor16(tag, m, s0);
}

/* decrypt: in = ct || tag; like the reference it decrypts first and authenticates the result: 0x1A leaves the
 * unauthenticated text in `out` (the engine's wipe switch is the caller's business)                              */
int uaesh_ccm(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
              const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t iv[16] = { 0 }, tag[16], given[16];
    iv[0] = (uint8_t)(14 - nonce_len);
    memcpy(iv + 1, nonce, nonce_len);
    if (!decrypt) {
        ccm_tag(k, iv, tag_len, aad, aad_len, in, len, tag);            /* over the plaintext, before in may be overwritten */
        uaesh_ctr(k, iv, 1, in, len, out);
        memcpy(out + len, tag, tag_len);
        return 0;
    }
    memcpy(given, in + len, tag_len);
    uaesh_ctr(k, iv, 1, in, len, out);
    ccm_tag(k, iv, tag_len, aad, aad_len, out, len, tag);
    return differ(tag, given, tag_len) ? 0x1A : 0;
}

/* ---- EAX (AES_EAX_encrypt / _decrypt micro_aes.c:1560-1648, oMac :1531-1548) and SIV, RFC 5297 (S2V :1323-1361,
 *      AES_SIV_encrypt / _decrypt :1373-1411) ------------------------------------------------------------------------ */
typedef struct { uint8_t k1[16], k2[16]; } cmac_keys;

static void cmac_keys_of(const uaesh_key *k, cmac_keys *s)
{
    memset(s->k1, 0, 16);
    uaesh_encrypt(k->ek, k->nr, s->k1, s->k1);
    cmac_double(s->k1);
    memcpy(s->k2, s->k1, 16);
    cmac_double(s->k2);
}

/* the CMAC chain m continued over len >= 1 bytes: whole blocks, then the last one with K1, or 10* padding and K2 */
static void cmac_continue(const uaesh_key *k, const cmac_keys *s, uint8_t m[16], const uint8_t *x, size_t len)
{
    const size_t last = (len - 1) % 16 + 1;
    size_t i;
    cbcmac_absorb(k, m, x, len - last);
    x += len - last;
    for (i = 0; i < 16; ++i) m[i] ^= (i < last ? x[i] : i == last ? 0x80 : 0) ^ (last < 16 ? s->k2[i] : s->k1[i]);
    uaesh_encrypt(k->ek, k->nr, m, m);
}

/* OMAC^t(x) = CMAC([t]_16 || x) */
static void eax_omac(const uaesh_key *k, const cmac_keys *s, unsigned t, const uint8_t *x, size_t len, uint8_t out[16])
{
    memset(out, 0, 16);
    out[15] = (uint8_t)t;
    if (!len) {
        xor16(out, out, s->k1);
        uaesh_encrypt(k->ek, k->nr, out, out);
        return;
    }
    uaesh_encrypt(k->ek, k->nr, out, out);
    cmac_continue(k, s, out, x, len);
}

/* decrypt: in = ct || tag; the tag is checked first and `out` stays untouched on 0x1A */
int uaesh_eax(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
              const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out)
{
    cmac_keys s;
    uint8_t n[16], h[16], c[16], tag[16];
    int rc = 0;
    cmac_keys_of(k, &s);
    eax_omac(k, &s, 0, nonce, nonce_len, n);
    eax_omac(k, &s, 1, aad, aad_len, h);
    if (decrypt) {
        eax_omac(k, &s, 2, in, len, c);
        xor16(tag, n, h);
        xor16(tag, tag, c);
        if (differ(tag, in + len, tag_len)) rc = 0x1A;
        else uaesh_ctr(k, n, 0, in, len, out);
    } else {
        uaesh_ctr(k, n, 0, in, len, out);
        eax_omac(k, &s, 2, out, len, c);
        xor16(tag, n, h);
        xor16(tag, tag, c);
        memcpy(out + len, tag, tag_len);
    }
    memset(&s, 0, sizeof s);
    return rc;
}

/* EAX' (the reference built with EAXP 1, :1523-1648): D = dblLE(Enc(0)) and Q = dblLE(D) (xts_double is doubleLblock)
 * are CMAC's subkeys, the chain of N = CMAC'(nonce) starts at D and the one of C' = CMAC'(ciphertext) at Q; an empty
 * string is one padded empty block (cMac :579-589), but an empty ciphertext gives C' = 0 (oMac :1535-1539) */
static void eaxp_cmac(const uaesh_key *k, const cmac_keys *s, int text, const uint8_t *x, size_t len, uint8_t out[16])
{
    memset(out, 0, 16);
    if (text && !len) return;
    memcpy(out, text ? s->k2 : s->k1, 16);
    if (len) { cmac_continue(k, s, out, x, len); return; }
    out[0] ^= 0x80;
    xor16(out, out, s->k2);
    uaesh_encrypt(k->ek, k->nr, out, out);
}

/* decrypt: in = ct || 4-byte mac; the mac is checked first and `out` stays untouched on 0x1A */
int uaesh_eaxp(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, const uint8_t *in, size_t len, uint8_t *out)
{
    cmac_keys s;
    uint8_t n[16], c[16], mac[4];
    int i, rc = 0;
    memset(s.k1, 0, 16);
    uaesh_encrypt(k->ek, k->nr, s.k1, s.k1);
    xts_double(s.k1);
    memcpy(s.k2, s.k1, 16);
    xts_double(s.k2);
    eaxp_cmac(k, &s, 0, nonce, nonce_len, n);
    memcpy(mac, n + 12, 4);
    n[12] &= 0x7F;                                                      /* N' (:1581-1582) */
    n[14] &= 0x7F;
    if (decrypt) {
        eaxp_cmac(k, &s, 1, in, len, c);
        for (i = 0; i < 4; ++i) mac[i] ^= c[12 + i];
        if (differ(mac, in + len, 4)) rc = 0x1A;
        else uaesh_ctr(k, n, 0, in, len, out);
    } else {
        uaesh_ctr(k, n, 0, in, len, out);
        eaxp_cmac(k, &s, 1, out, len, c);
        for (i = 0; i < 4; ++i) out[len + i] = mac[i] ^ c[12 + i];
    }
    memset(&s, 0, sizeof s);
    memset(n, 0, sizeof n);
    return rc;
}

/* V = S2V(S_1 .. S_nad, p), RFC 5297 section 2.4: the nad components lie back to back at aad, ad_lens[i] bytes each; an
 * empty one is a component all the same (CMAC("") = Enc(10* ^ K2)), nad == 0 is no header unit at all.  Y is XORed
 * into the last 16 bytes of a text of 16 bytes or more, a shorter one gets dbl(Y) ^ pad(p) */
static void s2v(const uaesh_key *k, size_t nad, const size_t *ad_lens, const uint8_t *aad, const uint8_t *p, size_t len,
                uint8_t v[16])
{
    cmac_keys s;
    uint8_t y[16] = { 0 }, d[16], t[16];
    size_t i, c;
    cmac_keys_of(k, &s);
    xor16(y, y, s.k1);
    uaesh_encrypt(k->ek, k->nr, y, y);                                  /* CMAC(0^128) */
    for (c = 0; c < nad; ++c) {
        memset(d, 0, 16);
        if (ad_lens[c]) {
            cmac_continue(k, &s, d, aad, ad_lens[c]);
            aad += ad_lens[c];
        } else {
            d[0] = 0x80;
            xor16(d, d, s.k2);
            uaesh_encrypt(k->ek, k->nr, d, d);
        }
        cmac_double(y);
        xor16(y, y, d);
    }
    memset(v, 0, 16);
    if (len < 16) {
        cmac_double(y);
        for (i = 0; i < 16; ++i) t[i] = y[i] ^ (i < len ? p[i] : i == len ? 0x80 : 0) ^ s.k1[i];
        uaesh_encrypt(k->ek, k->nr, t, v);
    } else {
        const size_t last = (len - 1) % 16 + 1, head = len - 16;       /* Y covers bytes head .. len-1 */
        cbcmac_absorb(k, v, p, len - last - (last < 16 ? 16 : 0));
        for (i = len - last - (last < 16 ? 16 : 0); i < len; i += 16) {
            const size_t n = len - i < 16 ? len - i : 16;
            size_t j;
            for (j = 0; j < 16; ++j) {
                const size_t at = i + j;
                uint8_t b = j < n ? p[at] : j == n ? 0x80 : 0;
                if (j < n && at >= head) b ^= y[at - head];
                if (i + 16 >= len) b ^= n < 16 ? s.k2[j] : s.k1[j];
                v[j] ^= b;
            }
            uaesh_encrypt(k->ek, k->nr, v, v);
        }
    }
    memset(&s, 0, sizeof s);
    memset(y, 0, 16);
}

static void s2v_ctr(const uaesh_key *k, const uint8_t v[16], const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t c[16];
    memcpy(c, v, 16);
    c[8] &= 0x7F;
    c[12] &= 0x7F;
    uaesh_ctr(k, c, 0, in, len, out);
}

/* k = K_s2v, kc = K_ctr; decrypt: CTR first, then S2V over the plaintext, 0x1A on a mismatch (the text stays) */
int uaesh_siv(const uaesh_key *k, const uaesh_key *kc, int decrypt, uint8_t iv[16], size_t nad, const size_t *ad_lens,
              const uint8_t *aad, const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t v[16];
    if (!decrypt) {
        s2v(k, nad, ad_lens, aad, in, len, v);
        s2v_ctr(kc, v, in, len, out);
        memcpy(iv, v, 16);
        return 0;
    }
    memcpy(v, iv, 16);
    s2v_ctr(kc, v, in, len, out);
    s2v(k, nad, ad_lens, aad, out, len, v);
    return differ(v, iv, 16) ? 0x1A : 0;
}

/* ---- GCM-SIV (RFC 8452; GCM_SIVsetup micro_aes.c:1434-1449, polyval :1421-1432, GCM_SIVtag :1452-1459,
 *      GCM_SIV_encrypt :1473-1485, _decrypt :1494-1515; CTR flavour SIVGCM_CTR :935-938) --------------------------------
 * POLYVAL runs through the GHASH tables above: POLYVAL(H, X_1..X_n) = ByteReverse(GHASH(mulX(ByteReverse(H)),
 * ByteReverse(X_1) .. ByteReverse(X_n)))  (RFC 8452 appendix A).                                                      */
static void rev16(uint8_t d[16], const uint8_t s[16])
{
    uint8_t t[16];
    int i;
    for (i = 0; i < 16; ++i) t[i] = s[15 - i];
    memcpy(d, t, 16);
}

static void polyval_absorb(const ghash_key *g, uint8_t y[16], const uint8_t *x, size_t len)
{
    uint8_t b[16];
    while (len) {
        const size_t n = len < 16 ? len : 16;
        memset(b, 0, 16);
        memcpy(b, x, n);
        rev16(b, b);
        ghash_absorb(g, y, b, 16);
        x += n; len -= n;
    }
}

static void put_le64(uint8_t *p, uint64_t v)
{
    int i;
    for (i = 0; i < 8; ++i, v >>= 8) p[i] = (uint8_t)v;
}

/* the 32-bit little-endian counter of the GCM-SIV keystream: bytes 0..3 of the block, wrapping mod 2^32 */
static void siv_ctr(const uint32_t *ek, int nr, const uint8_t tag[16], const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t c[16], ks[16];
    uint32_t v;
    size_t off, i;
    memcpy(c, tag, 16);
    c[15] |= 0x80;
    v = ld32(c);
    for (off = 0; off < len; off += 16, ++v) {
        const size_t n = len - off < 16 ? len - off : 16;
        st32(c, v);
        uaesh_encrypt(ek, nr, c, ks);
        for (i = 0; i < n; ++i) out[off + i] = in[off + i] ^ ks[i];
    }
}

/* expand: the engine's key schedule for the derived message-encryption key (ek words out) */
int uaesh_gcmsiv(const uaesh_key *master, int keybits, int decrypt, const uint8_t nonce[12],
                 const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out,
                 int (*expand)(int keybits, const uint8_t *key, uint32_t ek[60], uint32_t dk[60]))
{
    uint8_t blk[16], derived[16 + 32], hg[16], y[16] = { 0 }, pv[16], tag[16], lens[16];
    uint32_t ek[60], dk[60];
    ghash_key g;
    const unsigned nblk = 2u + (unsigned)keybits / 64u;     /* two for the authentication key, keybits / 64 for the cipher key */
    unsigned i;
    int nr, rc = 0;
    for (i = 0; i < nblk; ++i) {                    /* Enc_master(LE32(i) || nonce), the first eight bytes of each */
        uint8_t e[16];
        st32(blk, i);
        memcpy(blk + 4, nonce, 12);
        uaesh_encrypt(master->ek, master->nr, blk, e);
        memcpy(derived + 8 * i, e, 8);
    }
    nr = expand(keybits, derived + 16, ek, dk);
    if (nr < 0) return nr;
    /* GHASH key of POLYVAL's H: mulX(ByteReverse(H)) */
    {
        gf128 v;
        rev16(hg, derived);
        v.hi = be64(hg); v.lo = be64(hg + 8);
        v = gf_mulx(v);
        put_be64(hg, v.hi); put_be64(hg + 8, v.lo);
        ghash_setup(&g, hg);
    }
    if (decrypt) {                                  /* the tag is the counter: decrypt first, authenticate the result */
        memcpy(tag, in + len, 16);
        siv_ctr(ek, nr, tag, in, len, out);
    }
    polyval_absorb(&g, y, aad, aad_len);
    polyval_absorb(&g, y, decrypt ? out : in, len);
    put_le64(lens, (uint64_t)aad_len * 8);
    put_le64(lens + 8, (uint64_t)len * 8);
    polyval_absorb(&g, y, lens, 16);
    rev16(pv, y);
    for (i = 0; i < 12; ++i) pv[i] ^= nonce[i];
    pv[15] &= 0x7F;
    uaesh_encrypt(ek, nr, pv, pv);
    if (decrypt) {
        rc = differ(pv, tag, 16) ? 0x1A : 0;
    } else {
        siv_ctr(ek, nr, pv, in, len, out);
        memcpy(out + len, pv, 16);
    }
    memset(ek, 0, sizeof ek); memset(dk, 0, sizeof dk); memset(derived, 0, sizeof derived); memset(&g, 0, sizeof g);
    return rc;
}

/* ---- OCB (RFC 7253; OCB_cipher micro_aes.c:1693-1762, getDelta :1662-1680, AES_OCB_encrypt :1774-1784,
 *      _decrypt :1797-1811) -------------------------------------------------------------------------------------------
 * Offsets are chained here (Offset_i = Offset_{i-1} ^ L_ntz(i)); L_* = Enc(0), L_$ = 2 L_*, L_0 = 2 L_$, L_{k+1} = 2 L_k.  */
typedef struct { uint8_t star[16], dollar[16], l[64][16]; int have; } ocb_l;

static const uint8_t *ocb_lk(ocb_l *t, unsigned k)
{
    while (t->have <= (int)k) {
        memcpy(t->l[t->have], t->have ? t->l[t->have - 1] : t->dollar, 16);
        cmac_double(t->l[t->have]);
        t->have++;
    }
    return t->l[k];
}

static unsigned ntz64(uint64_t v)
{
    unsigned n = 0;
    while (!(v & 1)) { v >>= 1; ++n; }
    return n;
}

static void ocb_hash(const uaesh_key *k, ocb_l *t, const uint8_t *aad, size_t aad_len, uint8_t sum[16])
{
    uint8_t off[16] = { 0 }, b[16];
    uint64_t i;
    size_t j;
    memset(sum, 0, 16);
    for (i = 1; aad_len >= 16; ++i, aad += 16, aad_len -= 16) {
        xor16(off, off, ocb_lk(t, ntz64(i)));
        xor16(b, aad, off);
        uaesh_encrypt(k->ek, k->nr, b, b);
        xor16(sum, sum, b);
    }
    if (aad_len) {
        xor16(off, off, t->star);
        memset(b, 0, 16);
        memcpy(b, aad, aad_len);
        b[aad_len] = 0x80;
        for (j = 0; j < 16; ++j) b[j] ^= off[j];
        uaesh_encrypt(k->ek, k->nr, b, b);
        xor16(sum, sum, b);
    }
}

/* decrypt: in = ct || tag; like the reference the text is written either way and 0x1A reports a mismatch */
int uaesh_ocb(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
              const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out)
{
    ocb_l *t = (ocb_l *)calloc(1, sizeof *t);
    uint8_t kt[24], off[16], sum[16] = { 0 }, b[16], tag[16], given[16], hash[16];
    const unsigned bottom = nonce[nonce_len - 1] & 63u;
    size_t nfull = len / 16, rem = len % 16, j;
    uint64_t i;
    int rc = 0;
    if (!t) return -1;
    uaesh_encrypt(k->ek, k->nr, t->star, t->star);                       /* L_* = Enc(0) */
    memcpy(t->dollar, t->star, 16);
    cmac_double(t->dollar);
    /* Nonce block: taglen (bits) mod 128 in the top seven bits, zeros, a one bit, the nonce; its last six bits cleared */
    memset(kt, 0, sizeof kt);
    memcpy(kt + 16 - nonce_len, nonce, nonce_len);
    kt[0] |= (uint8_t)(tag_len << 4);
    kt[15 - nonce_len] |= 1;
    kt[15] &= 0xC0;
    uaesh_encrypt(k->ek, k->nr, kt, kt);                                  /* Ktop */
    for (j = 0; j < 8; ++j) kt[16 + j] = kt[j] ^ kt[j + 1];               /* Stretch = Ktop || (Ktop[0..7] ^ Ktop[1..8]) */
    for (j = 0; j < 16; ++j) {                                            /* Offset_0 = Stretch << bottom, top 128 bits */
        const unsigned v = ((unsigned)kt[j + bottom / 8] << 8) | kt[j + bottom / 8 + 1];
        off[j] = (uint8_t)(v >> (8 - bottom % 8));
    }
    if (decrypt) memcpy(given, in + len, tag_len);
    for (i = 1; i <= nfull; ++i, in += 16, out += 16) {
        xor16(off, off, ocb_lk(t, ntz64(i)));
        if (!decrypt) {
            xor16(sum, sum, in);
            xor16(b, in, off);
            uaesh_encrypt(k->ek, k->nr, b, b);
            xor16(out, b, off);
        } else {
            xor16(b, in, off);
            uaesh_decrypt(k->dk, k->nr, b, b);
            xor16(out, b, off);
            xor16(sum, sum, out);
        }
    }
    if (rem) {
        uint8_t pad[16], p[16] = { 0 };
        xor16(off, off, t->star);
        uaesh_encrypt(k->ek, k->nr, off, pad);
        if (!decrypt) memcpy(p, in, rem);
        for (j = 0; j < rem; ++j) out[j] = in[j] ^ pad[j];
        if (decrypt) memcpy(p, out, rem);
        p[rem] = 0x80;
        xor16(sum, sum, p);
        out += rem;
    }
    for (j = 0; j < 16; ++j) b[j] = sum[j] ^ off[j] ^ t->dollar[j];
    uaesh_encrypt(k->ek, k->nr, b, tag);
    ocb_hash(k, t, aad, aad_len, hash);
    xor16(tag, tag, hash);
    if (decrypt) rc = differ(tag, given, tag_len) ? 0x1A : 0;
    else memcpy(out, tag, tag_len);
    memset(t, 0, sizeof *t);
    free(t);
    return rc;
}

/* ---- Poly1305-AES (AES_Poly1305, micro_aes.c:1955-1997): h = (h + c_i) r mod 2^130 - 5 in five 26-bit limbs ---- */
static uint32_t load32le(const uint8_t *p)
{
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
static void store32le(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

static void poly_limbs(const uint8_t b[16], uint32_t hibit, uint32_t l[5])
{
    const uint32_t w0 = load32le(b), w1 = load32le(b + 4), w2 = load32le(b + 8), w3 = load32le(b + 12);
    l[0] = w0 & 0x3ffffff;
    l[1] = ((w0 >> 26) | (w1 << 6)) & 0x3ffffff;
    l[2] = ((w1 >> 20) | (w2 << 12)) & 0x3ffffff;
    l[3] = ((w2 >> 14) | (w3 << 18)) & 0x3ffffff;
    l[4] = (w3 >> 8) | (hibit << 24);
}

void uaesh_poly1305(const uaesh_key *k, const uint8_t r16[16], const uint8_t nonce[16], const uint8_t *data, size_t len,
                    uint8_t mac[16])
{
    uint8_t rb[16], blk[16];
    uint32_t r[5], h[5] = { 0, 0, 0, 0, 0 }, c[5], g[5], s[4], mask;
    uint64_t d[5], t;
    int i, j;
    uaesh_encrypt(k->ek, k->nr, nonce, blk);
    if (!len) { memcpy(mac, blk, 16); memset(blk, 0, sizeof blk); return; }
    for (i = 0; i < 4; ++i) s[i] = load32le(blk + 4 * i);
    memcpy(rb, r16, 16);
    rb[3] &= 15; rb[7] &= 15; rb[11] &= 15; rb[15] &= 15; rb[4] &= 252; rb[8] &= 252; rb[12] &= 252;
    poly_limbs(rb, 0, r);
    while (len) {
        const size_t n = len < 16 ? len : 16;
        memset(blk, 0, sizeof blk);
        memcpy(blk, data, n);
        if (n < 16) blk[n] = 1;
        poly_limbs(blk, n == 16, c);
        for (i = 0; i < 5; ++i) h[i] += c[i];
        for (i = 0; i < 5; ++i) {                    /* d_i = sum_j h_j r_(i-j), the wrapped terms times 5 */
            d[i] = 0;
            for (j = 0; j < 5; ++j) d[i] += (uint64_t)h[j] * (j <= i ? r[i - j] : 5 * r[i - j + 5]);
        }
        for (i = 0; i < 4; ++i) { d[i + 1] += d[i] >> 26; h[i] = (uint32_t)d[i] & 0x3ffffff; }
        h[4] = (uint32_t)d[4] & 0x3ffffff;
        t = h[0] + (d[4] >> 26) * 5;
        h[0] = (uint32_t)t & 0x3ffffff;
        h[1] += (uint32_t)(t >> 26);
        data += n;
        len -= n;
    }
    for (j = 0; j < 2; ++j) {                        /* fully carried: h < 2^130 */
        for (i = 0; i < 4; ++i) { h[i + 1] += h[i] >> 26; h[i] &= 0x3ffffff; }
        t = h[4] >> 26; h[4] &= 0x3ffffff; h[0] += (uint32_t)t * 5;
    }
    h[1] += h[0] >> 26; h[0] &= 0x3ffffff;
    g[0] = h[0] + 5;                                 /* h - p = h + 5 - 2^130, kept when it does not borrow */
    for (i = 1; i < 5; ++i) { g[i] = h[i] + (g[i - 1] >> 26); g[i - 1] &= 0x3ffffff; }
    g[4] -= 1u << 26;
    mask = (g[4] >> 31) - 1u;
    for (i = 0; i < 5; ++i) h[i] = (h[i] & ~mask) | (g[i] & mask);
    t = (uint64_t)(h[0] | (h[1] << 26)) + s[0];                 store32le(mac, (uint32_t)t);
    t = (t >> 32) + (uint32_t)((h[1] >> 6) | (h[2] << 20)) + s[1];  store32le(mac + 4, (uint32_t)t);
    t = (t >> 32) + (uint32_t)((h[2] >> 12) | (h[3] << 14)) + s[2]; store32le(mac + 8, (uint32_t)t);
    t = (t >> 32) + (uint32_t)((h[3] >> 18) | (h[4] << 8)) + s[3];  store32le(mac + 12, (uint32_t)t);
    {                                                /* r, s and h do not outlive the call */
        volatile uint32_t *v = r; for (i = 0; i < 5; ++i) v[i] = 0;
        v = h; for (i = 0; i < 5; ++i) v[i] = 0;
        v = s; for (i = 0; i < 4; ++i) v[i] = 0;
        volatile uint8_t *vb = rb; for (i = 0; i < 16; ++i) vb[i] = 0;
        vb = blk; for (i = 0; i < 16; ++i) vb[i] = 0;
    }
}

/* ---- key wrap, RFC 3394 (AES_KEY_wrap micro_aes.c:1829-1855, AES_KEY_unwrap :1865-1894; xorBEint with MIDST) ------- */
/* the step counter, big-endian, ending at byte 7 of A */
static void kw_xor_step(uint8_t a[16], uint64_t t)
{
    int i;
    for (i = 7; i >= 0 && t; --i, t >>= 8) a[i] ^= (uint8_t)t;
}

/* W of SP 800-38F over the n semiblocks at r0, 6 n steps; A = a[0..7] on entry and on return (a[8..15] is scratch) */
static void kw_chain(const uaesh_key *k, uint8_t a[16], uint8_t *r0, size_t n)
{
    uint8_t *r = r0, *const last = r0 + 8 * (n - 1);
    uint64_t t;
    for (t = 1; t <= 6 * (uint64_t)n; ++t) {
        memcpy(a + 8, r, 8);
        uaesh_encrypt(k->ek, k->nr, a, a);
        memcpy(r, a + 8, 8);
        kw_xor_step(a, t);
        r = r == last ? r0 : r + 8;
    }
}

/* its inverse */
static void kw_chain_inv(const uaesh_key *k, uint8_t a[16], uint8_t *r0, size_t n)
{
    uint8_t *r = r0, *const end = r0 + 8 * n;
    uint64_t t;
    for (t = 6 * (uint64_t)n; t; --t) {
        r = (r == r0 ? end : r) - 8;
        kw_xor_step(a, t);
        memcpy(a + 8, r, 8);
        uaesh_decrypt(k->dk, k->nr, a, a);
        memcpy(r, a + 8, 8);
    }
}

/* secret and wrapped are disjoint, or secret == wrapped + 8 (the reference's own in-place form) */
int uaesh_kw_wrap(const uaesh_key *k, const uint8_t *secret, size_t len, uint8_t *wrapped)
{
    const size_t n = len / 8;
    uint8_t a[16];
    if (n < 2 || len % 8) return 1;                     /* M_DATALENGTH_ERROR */
    memset(a, 0xA6, 8);
    memmove(wrapped + 8, secret, len);
    kw_chain(k, a, wrapped + 8, n);
    memcpy(wrapped, a, 8);
    memset(a, 0, sizeof a);
    return 0;
}

/* the secret is written whatever the verdict, like the reference; 0x1A = M_AUTHENTICATION_ERROR */
int uaesh_kw_unwrap(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret)
{
    const size_t n = wrap_len / 8;
    uint8_t a[16], bad = 0;
    int i;
    if (n < 3 || wrap_len % 8) return 1;
    memcpy(a, wrapped, 8);
    memmove(secret, wrapped + 8, wrap_len - 8);
    kw_chain_inv(k, a, secret, n - 1);
    for (i = 0; i < 8; ++i) bad |= a[i] ^ 0xA6;
    memset(a, 0, sizeof a);
    return bad ? 0x1A : 0;
}

/* ---- key wrap with padding, RFC 5649 / SP 800-38F KWP (the reference has none) ----------------------------------------- */
/* A = A6 59 59 A6 || len (32 bits, big-endian) over the secret zero-filled to n = ceil(len / 8) semiblocks: the chain
 * above for n >= 2, one block of the cipher for n = 1.  Writes 8 n + 8 bytes; the zero fill lands in `wrapped` first, so
 * the in-place form works.  1 for len = 0 or above 2^32 - 1, nothing written */
int uaesh_kwp_wrap(const uaesh_key *k, const uint8_t *secret, size_t len, uint8_t *wrapped)
{
    const size_t n = (len + 7) / 8;
    uint8_t a[16];
    if (len == 0 || (uint64_t)len > 0xFFFFFFFFu) return 1;
    a[0] = a[3] = 0xA6; a[1] = a[2] = 0x59;
    a[4] = (uint8_t)(len >> 24); a[5] = (uint8_t)(len >> 16); a[6] = (uint8_t)(len >> 8); a[7] = (uint8_t)len;
    if (n == 1) {
        memset(a + 8, 0, 8);
        memcpy(a + 8, secret, len);                     /* read before anything is written */
        uaesh_encrypt(k->ek, k->nr, a, a);
        memcpy(wrapped, a, 16);
    } else {
        memmove(wrapped + 8, secret, len);
        memset(wrapped + 8 + len, 0, 8 * n - len);
        kw_chain(k, a, wrapped + 8, n);
        memcpy(wrapped, a, 8);
    }
    memset(a, 0, sizeof a);
    return 0;
}

/* writes the wrap_len - 8 bytes the chain makes whatever the verdict; *secret_len = the length indicator of an authentic
 * secret, 0 otherwise.  The three conditions -- the constant, 8 (n - 1) < MLI <= 8 n, zeros behind the secret -- are all
 * evaluated and ORed: one verdict, no early exit.  1 for a length that is no multiple of 8, below 16 or beyond what the
 * indicator can describe */
int uaesh_kwp_unwrap(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret, uint32_t *secret_len)
{
    const size_t n = wrap_len / 8 - 1;
    const uint64_t top = 8 * (uint64_t)n;
    uint8_t a[16];
    uint64_t mli;
    unsigned bad, pad, i;
    if (wrap_len % 8 || wrap_len < 16 || top > (uint64_t)1 << 32) return 1;
    if (n == 1) {
        memcpy(a, wrapped, 16);
        uaesh_decrypt(k->dk, k->nr, a, a);
        memcpy(secret, a + 8, 8);
    } else {
        memcpy(a, wrapped, 8);
        memmove(secret, wrapped + 8, wrap_len - 8);
        kw_chain_inv(k, a, secret, n);
    }
    mli = ((uint32_t)a[4] << 24) | ((uint32_t)a[5] << 16) | ((uint32_t)a[6] << 8) | a[7];
    bad = (unsigned)(a[0] ^ 0xA6) | (unsigned)(a[1] ^ 0x59) | (unsigned)(a[2] ^ 0x59) | (unsigned)(a[3] ^ 0xA6);
    bad |= (unsigned)(mli + 8 <= top) | (unsigned)(mli > top);
    pad = (unsigned)(top - mli) & 7u;                   /* meaningful when the indicator is in range */
    for (i = 0; i < 8; ++i) bad |= secret[8 * (n - 1) + i] & (0u - (unsigned)(i + pad >= 8));
    *secret_len = bad ? 0 : (uint32_t)mli;
    memset(a, 0, sizeof a);
    return bad ? 0x1A : 0;
}

/* ---- FF1, SP 800-38G (FF1_cipher micro_aes.c:2091-2147, FPE_cipher :2267-2314) ---------------------------------------- */
/* the smallest n with radix^n >= 1 000 000 (the reference's MINLEN for every radix 2..256); 0 for a radix out of range */
unsigned uaesh_ff1_minlen(unsigned radix)
{
    unsigned n = 0;
    uint64_t p = 1;
    if (radix < 2 || radix > 256) return 0;
    while (p < 1000000u) { p *= radix; ++n; }
    return n;
}

/* b = ceil(bits(radix^v - 1) / 8), exactly: a power of two has v log2(radix) bits in radix^v - 1, any other radix as
 * many as radix^v itself, which is multiplied out in 32-bit limbs (v <= UAES_FF1_MAX / 2: at most 512 of them) */
size_t uaesh_ff1_b(unsigned radix, size_t v)
{
    uint32_t w[516];
    size_t n = 1, i, j, bits;
    if (radix < 2 || radix > 256 || v == 0 || v > 2048) return 0;
    if ((radix & (radix - 1)) == 0) {
        unsigned lg = 0;
        while ((1u << lg) < radix) ++lg;
        return (v * lg + 7) / 8;
    }
    w[0] = 1;
    for (i = 0; i < v; ++i) {
        uint64_t c = 0;
        for (j = 0; j < n; ++j) { c += (uint64_t)w[j] * radix; w[j] = (uint32_t)c; c >>= 32; }
        if (c) w[n++] = (uint32_t)c;
    }
    bits = 32 * (n - 1);
    while (w[n - 1]) { ++bits; w[n - 1] >>= 1; }
    return (bits + 7) / 8;
}

/* The alphabet of FF1 and FF3-1, radix = 2..256 distinct bytes (NULL: the digit values themselves): inv = byte -> digit
 * value, fwd = digit value -> byte.  A byte that is no numeral keeps inv 0xFF, which is >= radix unless every byte is a
 * numeral.  Returns -1, or the byte that occurs twice (its first occurrence is a digit below 0xFF: not the last). */
int uaesh_fpe_alphabet(unsigned radix, const uint8_t *alphabet, uint8_t inv[256], uint8_t fwd[256])
{
    unsigned i;
    memset(inv, 0xFF, 256);
    for (i = 0; i < radix; ++i) {
        const uint8_t a = alphabet ? alphabet[i] : (uint8_t)i;
        if (inv[a] != 0xFF) return a;
        inv[a] = (uint8_t)i;
        fwd[i] = a;
    }
    return -1;
}

#define FF1_MAX   4096u
#define FF1_HALF  (FF1_MAX / 2)

/* NUM_radix of n digits, most significant first, as nl 32-bit limbs, least significant first */
static void ff1_num(const uint8_t *s, size_t n, unsigned radix, uint32_t *limb, size_t nl)
{
    size_t i, j, top = 0;
    memset(limb, 0, nl * sizeof *limb);
    for (i = 0; i < n; ++i) {
        uint64_t c = s[i];
        for (j = 0; j < top; ++j) { c += (uint64_t)limb[j] * radix; limb[j] = (uint32_t)c; c >>= 32; }
        if (c && top < nl) limb[top++] = (uint32_t)c;
    }
}

/* the d bytes of S (a multiple of 4), a big-endian number, to m digits: what strRadix does a byte at a time, four at
 * a time; a longer number is cut to S mod radix^m, which is all FF1 wants of it */
static void ff1_str(const uint8_t *num, size_t d, unsigned radix, uint8_t *s, size_t m)
{
    size_t k, i;
    memset(s, 0, m);
    for (k = 0; k < d; k += 4) {
        uint64_t x = (uint64_t)num[k] << 24 | (uint64_t)num[k + 1] << 16 | (uint64_t)num[k + 2] << 8 | num[k + 3];
        for (i = m; i--; x /= radix) {
            x += (uint64_t)s[i] << 32;
            s[i] = (uint8_t)(x % radix);
        }
    }
}

int uaesh_ff1(const uaesh_key *k, int decrypt, unsigned radix, const uint8_t *alphabet,
              const uint8_t *tweak, size_t tweak_len, const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t x[FF1_MAX], y[FF1_HALF], q[FF1_HALF + 64], inv[256], fwd[256], p[16], r[16], blk[16];
    uint32_t limb[FF1_HALF / 4 + 1];
    const size_t u = len / 2, v = len - u, tfull = tweak_len & ~(size_t)15, trem = tweak_len & 15;
    size_t b, d, z, i, j, tail;
    int round, step;
    if (radix < 2 || radix > 256) return -2;
    if (len < uaesh_ff1_minlen(radix) || len > FF1_MAX || (uint64_t)tweak_len >> 32) return 1;
    if (uaesh_fpe_alphabet(radix, alphabet, inv, fwd) >= 0) return -2;
    for (i = 0; i < len; ++i) {                               /* every numeral is looked up before anything is written */
        if (inv[in[i]] >= radix) return decrypt ? 0x1D : 0x1E;
        x[i] = inv[in[i]];
    }
    b = uaesh_ff1_b(radix, v);
    d = 4 * ((b + 3) / 4) + 4;
    z = (16 - (tweak_len + b + 1) % 16) % 16;
    tail = trem + z + 1 + b;                                  /* a multiple of 16 */
    p[0] = 1; p[1] = 2; p[2] = 1; p[3] = (uint8_t)(radix >> 16); p[4] = (uint8_t)(radix >> 8); p[5] = (uint8_t)radix;
    p[6] = 10; p[7] = (uint8_t)u;
    for (i = 0; i < 4; ++i) { p[8 + i] = (uint8_t)(len >> (24 - 8 * i)); p[12 + i] = (uint8_t)(tweak_len >> (24 - 8 * i)); }
    uaesh_encrypt(k->ek, k->nr, p, p);                         /* the PRF over P and the tweak's full blocks: once */
    for (i = 0; i < tfull; i += 16) {
        for (j = 0; j < 16; ++j) p[j] ^= tweak[i + j];
        uaesh_encrypt(k->ek, k->nr, p, p);
    }
    memset(q, 0, trem + z);
    if (trem) memcpy(q, tweak + tfull, trem);
    for (step = 0; step < 10; ++step) {
        const size_t nl = (b + 3) / 4;
        round = decrypt ? 9 - step : step;
        {   /* even rounds: the first u numerals take F(the last v); odd rounds the other way round */
            uint8_t *a = round & 1 ? x + u : x;
            const uint8_t *bb = round & 1 ? x : x + u;
            const size_t m = round & 1 ? v : u, n = round & 1 ? u : v;
            unsigned c;
            ff1_num(bb, n, radix, limb, nl);
            q[trem + z] = (uint8_t)round;
            for (i = 0; i < b; ++i) q[trem + z + 1 + i] = (uint8_t)(limb[(b - 1 - i) / 4] >> (8 * ((b - 1 - i) % 4)));
            memcpy(r, p, 16);
            for (i = 0; i < tail; i += 16) {
                for (j = 0; j < 16; ++j) r[j] ^= q[i + j];
                uaesh_encrypt(k->ek, k->nr, r, r);
            }
            memcpy(q + trem + z, r, 16);                      /* S = R | E(R ^ [1]) | ... behind the tweak's tail */
            for (i = 1; 16 * i < d; ++i) {
                memcpy(blk, r, 16);
                blk[15] ^= (uint8_t)i; blk[14] ^= (uint8_t)(i >> 8);
                uaesh_encrypt(k->ek, k->nr, blk, q + trem + z + 16 * i);
            }
            ff1_str(q + trem + z, d, radix, y, m);
            if (!decrypt)
                for (i = m, c = 0; i--; c /= radix) { c += (unsigned)a[i] + y[i]; a[i] = (uint8_t)(c % radix); }
            else
                for (i = m, c = 1; i--; c /= radix) { c += radix - 1 + a[i] - y[i]; a[i] = (uint8_t)(c % radix); }
        }
    }
    for (i = 0; i < len; ++i) out[i] = fwd[x[i]];
    memset(x, 0, sizeof x); memset(y, 0, sizeof y); memset(q, 0, sizeof q);
    memset(limb, 0, sizeof limb); memset(p, 0, sizeof p); memset(r, 0, sizeof r);
    return 0;
}

/* ---- FF3-1, SP 800-38G revision 1 (FF3_cipher micro_aes.c:2150-2248, FPE_cipher :2267-2314 with FF_X 3) ------------------ */
typedef unsigned __int128 u128;

/* 2 * the largest k with radix^k <= 2^96: the specification's maxlen, which the reference's 2 * (int)(96.000001 / LOGRDX)
 * (micro_fpe.h:145) equals */
size_t uaesh_ff3_maxlen(unsigned radix)
{
    const u128 lim = (u128)1 << 96;
    u128 p = 1;
    size_t k = 0;
    if (radix < 2 || radix > 256) return 0;
    while (p * radix <= lim) { p *= radix; ++k; }
    return 2 * k;
}

/* Both halves stay NUMBERS (numeral 0 the least significant digit, below radix^m <= 2^96) through the eight rounds; with
 * the specification's REV and REVB folded in, a round's block is NUM(the other half) least significant byte first, then
 * the tweak half reversed with the round number in its last byte, and y is the cipher's output read the same way. */
int uaesh_ff3(const uaesh_key *k, int decrypt, unsigned radix, const uint8_t *alphabet, const uint8_t *tweak,
              const uint8_t *in, size_t len, uint8_t *out)
{
    uint8_t inv[256], fwd[256], blk[16], w[2][4];
    const size_t u = (len + 1) / 2;
    u128 num[2] = { 0, 0 }, mod[2] = { 1, 1 };
    size_t i;
    int step;
    if (radix < 2 || radix > 256) return -2;
    if (len < uaesh_ff1_minlen(radix) || len > uaesh_ff3_maxlen(radix)) return 1;
    if (uaesh_fpe_alphabet(radix, alphabet, inv, fwd) >= 0) return -2;
    for (i = 0; i < len; ++i)                                 /* every numeral is looked up before anything is written */
        if (inv[in[i]] >= radix) return decrypt ? 0x1D : 0x1E;
    for (i = u; i-- > 0;) { num[0] = num[0] * radix + inv[in[i]]; mod[0] *= radix; }
    for (i = len; i-- > u;) { num[1] = num[1] * radix + inv[in[i]]; mod[1] *= radix; }
    w[0][0] = (uint8_t)(tweak[3] << 4); w[0][1] = tweak[6]; w[0][2] = tweak[5]; w[0][3] = tweak[4];     /* TR reversed */
    w[1][0] = tweak[3] & 0xF0; w[1][1] = tweak[2]; w[1][2] = tweak[1]; w[1][3] = tweak[0];              /* TL reversed */
    for (step = 0; step < 8; ++step) {
        const int round = decrypt ? 7 - step : step, odd = round & 1;      /* an even round changes the first half */
        u128 y = 0, t = num[!odd];
        for (i = 0; i < 12; ++i, t >>= 8) blk[i] = (uint8_t)t;
        memcpy(blk + 12, w[odd], 4);
        blk[12] ^= (uint8_t)round;
        uaesh_encrypt(k->ek, k->nr, blk, blk);
        for (i = 16; i-- > 0;) y = y << 8 | blk[i];
        y %= mod[odd];
        num[odd] = (decrypt ? num[odd] + mod[odd] - y : num[odd] + y) % mod[odd];
    }
    for (i = 0; i < len; ++i) {
        const int h = i >= u;
        const unsigned dgt = (unsigned)(num[h] % radix);
        num[h] /= radix;
        out[i] = fwd[dgt];
    }
    memset(blk, 0, sizeof blk); memset(w, 0, sizeof w);
    num[0] = num[1] = 0;
    return 0;
}
