/*
 * uaes_host.h -- the engine's own host data path (uaes_host.c): what the entry points in uaes_engine_*.c call when the deployer has
 * switched it on (uaes_set_host_policy, include/uaes_hip.h).  Plain C, host memory only, re-entrant; key schedules are
 * the engine's (little-endian words of the FIPS-197 byte stream: ek = encryption round keys, dk = the equivalent
 * inverse cipher's).  Every function states the reference function it follows (paths relative to the reference).
 */
#ifndef UAES_HOST_H_
#define UAES_HOST_H_

#include <stddef.h>
#include <stdint.h>

typedef struct {
    const uint32_t *ek, *dk;
    int nr;                                         /* 10 / 12 / 14 */
} uaesh_key;

/* once per process, from the engine's GF(2^8)-derived Te0 / Td0 */
void uaesh_tables_init(const uint32_t te0[256], const uint32_t td0[256]);

void uaesh_encrypt(const uint32_t *ek, int nr, const uint8_t in[16], uint8_t out[16]);          /* micro_aes.c:242-259 */
void uaesh_decrypt(const uint32_t *dk, int nr, const uint8_t in[16], uint8_t out[16]);          /* :315-332 */

void uaesh_ecb_encrypt(const uaesh_key *k, int padding, const uint8_t *in, size_t len, uint8_t *out);      /* :636-652 */
void uaesh_ecb_decrypt(const uaesh_key *k, const uint8_t *in, size_t len, uint8_t *out);                   /* :663-680 */
void uaesh_ctr(const uaesh_key *k, const uint8_t ctr0[16], uint64_t block_offset,
               const uint8_t *in, size_t len, uint8_t *out);                                                /* :919-950 */
void uaesh_xts_unit(const uaesh_key *k1, const uaesh_key *k2, int encrypt, const uint8_t tweak[16],
                    const uint8_t *in, size_t len, uint8_t *out);                                           /* :1008-1055 */
void uaesh_xts_sectors(const uaesh_key *k1, const uaesh_key *k2, int encrypt, uint64_t first_sector,
                       size_t sector_bytes, size_t nsectors, const uint8_t *in, uint8_t *out);
void uaesh_ghash(const uint8_t h[16], const uint8_t *aad, size_t aad_len, const uint8_t *ct, size_t ct_len,
                 uint8_t out[16]);                                                                          /* :1127-1137 */
int  uaesh_gcm(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
               const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out);            /* :1140-1212 */
int  uaesh_cbc_encrypt(const uaesh_key *k, const uint8_t iv[16], int cts, int padding,
                       const uint8_t *in, size_t len, uint8_t *out);                                        /* :697-744 */
int  uaesh_cbc_decrypt(const uaesh_key *k, const uint8_t iv[16], int cts,
                       const uint8_t *in, size_t len, uint8_t *out);                                        /* :746-782 */
void uaesh_cfb(const uaesh_key *k, const uint8_t iv[16], int encrypt, const uint8_t *in, size_t len, uint8_t *out);   /* :799-817 */
void uaesh_ofb(const uaesh_key *k, const uint8_t iv[16], const uint8_t *in, size_t len, uint8_t *out);     /* :861-885 */
void uaesh_cmac(const uaesh_key *k, const uint8_t *data, size_t len, uint8_t mac[16]);                      /* :1108-1118 */
int  uaesh_ccm(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
               const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out);            /* :1226-1314 */
/* EAX: any nonce length, tag_len 1..16 (decrypt: in = ct || tag, `out` untouched on 0x1A);
 * SIV: k = K_s2v, kc = K_ctr, iv = the synthesized IV (out) / the IV to check (in); aad = nad components of
 * ad_lens[i] bytes back to back (RFC 5297's vector; the reference's one aData is nad = aDataLen ? 1 : 0)        */
int  uaesh_eax(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
               const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out);            /* :1560-1648 */
/* EAX' (the reference built with EAXP 1): any nonce length, a 4-byte mac (decrypt: in = ct || mac, `out` untouched on 0x1A) */
int  uaesh_eaxp(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len,
                const uint8_t *in, size_t len, uint8_t *out);                                               /* :1523-1648 */
int  uaesh_siv(const uaesh_key *k, const uaesh_key *kc, int decrypt, uint8_t iv[16], size_t nad, const size_t *ad_lens,
               const uint8_t *aad, const uint8_t *in, size_t len, uint8_t *out);                            /* :1323-1411 */

/* r = the r half of the key pair (clamped here), AES_k(nonce) with k; len 0: mac = AES_k(nonce) */
void uaesh_poly1305(const uaesh_key *k, const uint8_t r[16], const uint8_t nonce[16], const uint8_t *data, size_t len,
                    uint8_t mac[16]);                                                                       /* :1955-1997 */

/* expand = the engine's key schedule (uaes_expand_key): GCM-SIV derives its message key per nonce */
int  uaesh_gcmsiv(const uaesh_key *master, int keybits, int decrypt, const uint8_t nonce[12],
                  const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out,
                  int (*expand)(int keybits, const uint8_t *key, uint32_t ek[60], uint32_t dk[60]));      /* :1418-1516 */
int  uaesh_ocb(const uaesh_key *k, int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
               const uint8_t *aad, size_t aad_len, const uint8_t *in, size_t len, uint8_t *out);            /* :1693-1811 */

/* RFC 3394 key wrap: 0, 1 (M_DATALENGTH_ERROR: no multiple of 8 bytes, or fewer than two semiblocks of secret; nothing
 * written) or, from unwrap, 0x1A (the secret is written all the same); secret == wrapped + 8 works in place */
int  uaesh_kw_wrap(const uaesh_key *k, const uint8_t *secret, size_t len, uint8_t *wrapped);                  /* :1829-1855 */
int  uaesh_kw_unwrap(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret);           /* :1865-1894 */

/* RFC 5649 key wrap with padding over the same chain (the reference has none): a secret of 1 .. 2^32 - 1 bytes becomes
 * 8 ceil(len / 8) + 8 bytes.  unwrap writes wrap_len - 8 bytes (the secret and its zero fill) whatever the verdict and
 * *secret_len = the length indicator / 0.  0, 1 (the length; nothing written) or 0x1A; in place as above */
int  uaesh_kwp_wrap(const uaesh_key *k, const uint8_t *secret, size_t len, uint8_t *wrapped);
int  uaesh_kwp_unwrap(const uaesh_key *k, const uint8_t *wrapped, size_t wrap_len, uint8_t *secret, uint32_t *secret_len);

/* FF1, SP 800-38G: len numerals of one byte each (digit values, or bytes of `alphabet` = radix distinct bytes), in
 * place allowed.  0; 1 (len below uaesh_ff1_minlen(radix), above 4096, or a tweak of 2^32 bytes or more); -2 (radix
 * outside 2..256, a repeated alphabet byte); 0x1E / 0x1D (encrypt / decrypt: a byte that is no numeral).  Nothing is
 * written unless it returns 0.  uaesh_ff1_b = the b of the specification for a half of v numerals, exact integers. */
unsigned uaesh_ff1_minlen(unsigned radix);
int  uaesh_fpe_alphabet(unsigned radix, const uint8_t *alphabet, uint8_t inv[256], uint8_t fwd[256]);   /* uaes_host.c */
size_t   uaesh_ff1_b(unsigned radix, size_t v);
int  uaesh_ff1(const uaesh_key *k, int decrypt, unsigned radix, const uint8_t *alphabet, const uint8_t *tweak,
               size_t tweak_len, const uint8_t *in, size_t len, uint8_t *out);                               /* :2091-2147, :2267-2314 */

/* FF3-1, SP 800-38G revision 1: as uaesh_ff1 with a tweak of exactly seven bytes; k = the schedule of the key with its
 * BYTES REVERSED.  1 for len below uaesh_ff1_minlen(radix) or above uaesh_ff3_maxlen(radix) = 2 floor(log_radix 2^96)
 * (exact integers; 0 for a radix outside 2..256). */
size_t   uaesh_ff3_maxlen(unsigned radix);
int  uaesh_ff3(const uaesh_key *k, int decrypt, unsigned radix, const uint8_t *alphabet, const uint8_t *tweak7,
               const uint8_t *in, size_t len, uint8_t *out);                                                 /* :2150-2248, :2267-2314 */

#endif
