/*
 * uaes_device.h -- interface between the C host layer (uaes_engine*.c) and the
 * HIP kernels (uaes_kernels.hip).  Plain C types only; every entry point is a
 * thin launcher that enqueues gfx950 kernels on the given stream and returns
 * the hipError_t value (0 = success).  Nothing here touches host data.
 */
#ifndef UAES_DEVICE_H_
#define UAES_DEVICE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Expanded key as little-endian words of the FIPS-197 byte stream.
 * ek = encryption round keys; dk = equivalent-inverse-cipher round keys
 * (dk[0] = ek[nr], dk[i] = InvMixColumns(ek[nr-i]), dk[nr] = ek[0]).      */
typedef struct {
    uint32_t w[60];
} uaesk_rk;

/* Read-only device tables uploaded once per context by the host layer. */
typedef struct {
    const uint32_t *te0;   /* 256 words: bytes {2S,S,S,3S}[x]              */
    const uint32_t *td0;   /* 256 words: bytes {14Si,9Si,13Si,11Si}[x] (their XOR is Si[x]) */
    /* GHASH: x -> x^(2^k) in GF(2^128) is GF(2)-linear with a matrix that depends on the field
     * only.  frob[(k-1)*256 + 2p .. +1] = the (hi, lo) input mask of output bit p (p < 64: bit p of
     * the big-endian high half, else bit p-64 of the low half), k = 1..63.  May be NULL (the
     * setup kernel then squares k times).                                                     */
    const uint64_t *frob;
} uaesk_tables;

/* 56-bit big-endian counter description (reference: incBlock with index 15
 * carries through bytes 15..9 only, micro_aes.c:421-427).                 */
typedef struct {
    uint32_t w0, w1;       /* counter-block bytes 0..7 as LE words         */
    uint32_t b8;           /* counter-block byte 8 (never changes)         */
    uint64_t v0;           /* bytes 9..15 as a 56-bit big-endian integer   */
    /* le32 != 0: the GCM-SIV flavour of CTR_cipher (SIVGCM_CTR, micro_aes.c:935-938):
     * a 32-bit LITTLE-endian counter in bytes 0..3 (w0, wraps mod 2^32), the other
     * twelve bytes (w1, w2, w3) fixed.  b8 / v0 are ignored.                 */
    uint32_t le32, w2, w3;
} uaesk_ctr;

/* ECB: nfull whole blocks, plus (enc only) one padded tail block built from the
 * `rem` trailing bytes (reference N1, micro_aes.c:648-651).  padding = the
 * reference's AES_PADDING (padBlock, micro_aes.c:610-621): 0 zeros and only when
 * rem != 0, 1 PKCS#7, 2 ISO/IEC 7816-4 -- the latter two always add a block.  */
int uaesk_ecb(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *keys,
              int decrypt, const void *in, void *out, size_t nfull, unsigned rem, unsigned padding);

/* CTR keystream xor over len bytes (whole blocks + byte-granular tail).
 * If gate != NULL the kernel does nothing unless *gate == 0 (used by GCM
 * decrypt: authenticate first, micro_aes.c:1204-1208).                     */
int uaesk_ctr_xcrypt(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                     const uaesk_ctr *ctr, const void *in, void *out, size_t len,
                     const int *gate);
/* the generic CTR kernel with its key schedule and counter description in DEVICE memory (made by an earlier kernel
 * of the same stream) */
int uaesk_ctr_xcrypt_ind(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *d_rk,
                         const uaesk_ctr *d_ctr, const void *in, void *out, size_t len);

/* XTS over nsectors data units of sector_bytes each (>= 16).  Unit i has the
 * tweak block LE128(first_sector+i), or, if tweak16 != NULL (single unit),
 * the raw 16 bytes at tweak16 (a HOST pointer, copied into the launch).
 * scratch must hold uaesk_xts_scratch_bytes().                            */
size_t uaesk_xts_scratch_bytes(size_t sector_bytes, size_t nsectors);
int uaesk_xts(void *stream, const uaesk_tables *tb, int nr,
              const uaesk_rk *k1, const uaesk_rk *k2_enc, int decrypt,
              const uint8_t *tweak16, uint64_t first_sector,
              size_t sector_bytes, size_t nsectors,
              const void *in, void *out, void *scratch);

/* GCM.  All pointers are device pointers except j0_16 (host): the initial counter block J0 =
 * nonce || 00000001 for a 12-byte nonce, else the 16 bytes uaesk_gcm_j0 computed (GHASH of the
 * nonce, micro_aes.c:1145-1149).
 * scratch must hold uaesk_gcm_scratch_bytes().  encrypt: CTR then GHASH, tag
 * written at out+len.  decrypt: GHASH over in[0..len), compare with the tag
 * at in+len, *status = 0 / 0x1A, CTR gated on *status.                     */
size_t uaesk_gcm_scratch_bytes(void);
size_t uaesk_gcm_stream_scratch_bytes(void);     /* what the streamed API needs (no fused-pass buffers) */
int uaesk_gcm_j0(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                 const void *d_iv, size_t iv_len, void *scratch, void *j0_out16);
/* decrypt: 0 = encrypt; 1 = decrypt, nothing written unless the tag matches (two passes over the text);
 * 2 = decrypt, long texts in one pass: `out` is written before the tag is known and zeroed if it
 * turns out wrong (for callers that accept a wiped buffer, or whose `out` is private staging).
 * keyed != 0 promises that uaesk_gcm_key_tables has filled `scratch` under this key and nothing but uaesk_gcm calls
 * with keyed != 0 under the same key has written it since: per message only Enc(J0) is computed then, unless the
 * text needs a size-dependent bulk table.  One call at a time per buffer.                            */
int uaesk_gcm(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
              int decrypt, const uint8_t *j0_16,
              const void *aad, size_t aad_len,
              const void *in, size_t len, void *out,
              void *scratch, int *status, int keyed);

/* decrypt == 3: just the tag of (aad, `in` as ciphertext), 16 bytes written at `status`; the
 * host layer compares a truncated tag (GCM_TAG_LEN < 16) itself and then calls uaesk_gcm_ctr for the text */
int uaesk_gcm_ctr(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                  const uint8_t *j0_16, const void *in, size_t len, void *out);

/* Key context: every table that depends on the key only, into a scratch buffer (uaesk_gcm_scratch_bytes()) */
int uaesk_gcm_key_tables(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, void *key_scratch);

/* Many short messages under one key context in one launch (k_gcm_records): record r = rec_len bytes at
 * in + r * in_stride under nonce nonces12 + 12 r with the AAD at aad + r * aad_stride (stride 0: shared);
 * encrypt writes text || tag at out + r * out_stride; decrypt reads text || tag, writes the text of the records
 * whose tag matches, verdicts[r] = 0 / 0x1A (may be NULL) and ORs 0x1A into *status (zero it first).
 * in, out and the strides are multiples of 16; rec_len <= uaesk_gcm_record_max(aad_len).  Reads the key
 * context's tables only: any number of these calls may share one context.                               */
size_t uaesk_gcm_record_max(size_t aad_len);
int uaesk_gcm_records(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                      const void *nonces12, const void *aad, size_t aad_len, size_t aad_stride,
                      const void *in, size_t rec_len, size_t in_stride, void *out, size_t out_stride,
                      size_t nrec, const void *key_scratch, unsigned char *verdicts, int *status,
                      const void *lens /* NULL: every record rec_len bytes; else uint32 lens[nrec], record r = min(lens[r], rec_len) bytes */);

/* Sharded GCM: the weighted partial GHASH of one 16-byte-aligned ciphertext
 * shard (first shard: + AAD and Enc(J0); last shard: + length block).  The tag
 * of the whole message is the XOR of all shards' 16-byte results.           */
int uaesk_gcm_partial(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                      const uint8_t *nonce12, const void *aad, uint64_t total_aad_len,
                      const void *ct_shard, size_t shard_len, uint64_t shard_offset,
                      uint64_t total_len, void *scratch, void *partial16);
/* ... and the shard's CTR pass with it (one process driving several GPUs, uaes_mgpu_gcm_*): mode 0 encrypts
 * in -> out (keystream from J0 + 1 + shard_offset / 16) and hashes `out`; mode 1 = uaesk_gcm_partial (`out` unused);
 * mode 2 decrypts in -> out and hashes `in` -- `out` is written before any tag is known, the caller owns N7.
 * Every shard but the last is a multiple of 16 bytes.  A long shard runs CTR and GHASH in one pass.          */
int uaesk_gcm_shard(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mode,
                    const uint8_t *nonce12, const void *aad, uint64_t total_aad_len,
                    const void *in, size_t shard_len, uint64_t shard_offset,
                    uint64_t total_len, void *out, void *scratch, void *partial16);

/* Streamed GCM: the running GHASH value stays in `scratch` (one
 * scratch buffer per stream).  absorb kind 0 = AAD (restarts the hash), 1 = a piece of
 * ciphertext (multiple of 16 bytes unless last), 2 = the length block.  tag:
 * write Y ^ Enc(J0) to tag_io, or compare with it (*status = 0 / 0x1A).       */
int uaesk_gcm_stream_absorb(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                            const uint8_t *nonce12, int kind, const void *data, size_t len,
                            uint64_t total_aad_len, uint64_t total_ct_len, void *scratch,
                            unsigned *plan_state);   /* per stream, starts at 0: which tables scratch holds */
/* one piece of the text, CTR + GHASH in one pass: the striped kernel when it is long enough, one launch of chunk
 * workgroups + finisher from 16 KiB (needs done_word: zero between calls); returns 1 when neither applies (run
 * uaesk_ctr_xcrypt + uaesk_gcm_stream_absorb instead); the scratch must hold uaesk_gcm_scratch_bytes() */
int uaesk_gcm_stream_piece(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
                           const uint8_t *nonce12, int decrypt, const void *in, size_t len,
                           uint64_t done_bytes, void *out, void *scratch, unsigned *plan_state, unsigned *done_word);
int uaesk_gcm_stream_tag(void *stream, void *scratch, int compare, void *tag_io, int *status);

/* short GCM-SIV message in one launch; -1 = not applicable (too long): take the general path */
int uaesk_gcmsiv_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *master_ek, int decrypt,
                       const uint8_t *nonce12,
                       const void *aad, size_t aad_len, const void *in, size_t len, void *out, int *status);

/* GCM-SIV of a message of any length without a host round trip: key derivation, key expansion, tag and counter stay
 * in `scratch` (uaesk_gcm_scratch_bytes()); *status (decrypt) = 0 / 0x1A, the plaintext is written either way */
int uaesk_gcmsiv_long(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *master_ek, int decrypt,
                      const uint8_t *nonce12, const void *aad, size_t aad_len,
                      const void *in, size_t len, void *out, void *scratch, int *status);

/* Batch: nmsg GCM-SIV records under one MASTER key, sixteen lanes per record (k_gcmsiv_batch, uaes_gcmsiv_batch.hip); all
 * device pointers.  Record m: text at in / out + m msg_bytes (msg_bytes <= UAES_GCMSIV_BATCH_MAX), its first lens[m]
 * bytes (lens NULL: msg_bytes), nonce at nonces + 12 m, AAD at aad + m aad_bytes (<= UAES_GCMSIV_BATCH_MAX), tag at
 * tags + 16 m.  The per-nonce keys are derived and expanded in the kernel.  decrypt writes verdicts[m] (1 = authentic)
 * and ORs 1 into *bad for a forgery, whose output stays as decrypted or is zeroed when wipe != 0. */
int uaesk_gcmsiv_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *master_ek, int decrypt, int wipe,
                       const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                       const void *lens, const void *in, void *out, void *tags, void *verdicts, int *bad);

/* Batch: nmsg GCM records, EACH UNDER ITS OWN KEY, sixteen lanes per record (k_gcm_multikey, uaes_gcm_multikey.hip);
 * all device pointers, the keys included.  Record m: key at keys + m * 4 (nr - 6) bytes (any byte offset), text at in /
 * out + m msg_bytes (msg_bytes <= UAES_GCM_MULTIKEY_BATCH_MAX), its first lens[m] bytes (lens NULL: msg_bytes), nonce at
 * nonces + 12 m, AAD at aad + m aad_bytes (<= UAES_GCM_MULTIKEY_BATCH_MAX), the first tag_len (1..16) bytes of the tag
 * at tags + m tag_len.  Every schedule is expanded in the kernel, into LDS.  decrypt writes verdicts[m] (1 = authentic)
 * and ORs 1 into *bad for a forgery, whose output is not written at all. */
int uaesk_gcm_multikey_batch(void *stream, const uaesk_tables *tb, int nr, int decrypt, size_t tag_len,
                             const void *keys, const void *nonces, const void *aad, size_t aad_bytes,
                             size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out,
                             void *tags, void *verdicts, int *bad);

/* one block as little-endian column words, by value into a kernel's arguments */
typedef struct {
    uint32_t w[4];
} uaesk_block;

/* Batch: nmsg XAES-256-GCM records (C2SP) under one MASTER AES-256 key, sixteen lanes per record (k_xaes_gcm_batch,
 * uaes_xaes.hip); all device pointers.  k1 = CMAC's first subkey under the master key (2 AES_K(0) in GF(2^128)).  Record
 * m: text at in / out + m msg_bytes (msg_bytes <= UAES_XAES_GCM_BATCH_MAX), its first lens[m] bytes (lens NULL:
 * msg_bytes), nonce at nonces + 24 m (any byte offset), AAD at aad + m aad_bytes (<= UAES_XAES_GCM_BATCH_MAX), tag at
 * tags + 16 m.  The per-nonce key is derived and expanded in the kernel, into LDS.  decrypt writes verdicts[m] (1 =
 * authentic; verdicts may be NULL) and ORs 1 into *bad for a forgery, whose output is not written at all. */
int uaesk_xaes_gcm_batch(void *stream, const uaesk_tables *tb, const uaesk_rk *master_ek, const uaesk_block *k1,
                         int decrypt, const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg,
                         size_t msg_bytes, const void *lens, const void *in, void *out, void *tags, void *verdicts,
                         int *bad);

/* GHASH only: gh = GHASH_H(aad, ct) with H given (device), for tests.      */
int uaesk_ghash(void *stream, const uaesk_tables *tb, const uint8_t *H_host,
                const void *aad, size_t aad_len, const void *ct, size_t ct_len,
                void *scratch, void *gh_out16);

/* CMAC (AES_CMAC, micro_aes.c:1108): mac16 <- CMAC_K(data); all device pointers. */
int uaesk_cmac(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
               const void *data, size_t len, void *mac16);

/* CCM (AES_CCM_encrypt/decrypt, micro_aes.c:1268-1314), nonce (host) of nonce_len = 7..13 bytes,
 * tag_len (even, 4..16) bytes of tag at out+len / in+len; decrypt writes *status = 0 / 0x1A.   */
int uaesk_ccm(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek,
              int decrypt, const uint8_t *nonce, size_t nonce_len, size_t tag_len,
              const void *aad, size_t aad_len,
              const void *in, size_t len, void *out, int *status);
/* Batch: nmsg records under one key, sixteen lanes per record (k_ccm_batch); all device pointers.  Record m: text at
 * in / out + m msg_bytes (msg_bytes <= UAES_CCM_BATCH_MAX), its first lens[m] bytes (lens NULL: msg_bytes), nonce at
 * nonces + m nonce_len, AAD at aad + m aad_bytes (<= 0xFEFF), tag at tags + m tag_len.  decrypt writes verdicts[m]
 * (1 = authentic) and ORs 1 into *bad for a forgery, whose output stays as decrypted or is zeroed when wipe != 0. */
int uaesk_ccm_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt, int wipe,
                    const void *nonces, size_t nonce_len, size_t tag_len, const void *aad, size_t aad_bytes,
                    size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out, void *tags,
                    void *verdicts, int *bad);

/* Feedback modes (micro_aes.c:697-893).  mode: 0 CBC encrypt (CS3 stealing),
 * 1 CBC decrypt, 2 CFB encrypt, 3 CFB decrypt, 4 OFB.  iv16 is a host pointer.
 * The block-parallel directions (1, 3) need in != out.                       */
int uaesk_feedback(void *stream, const uaesk_tables *tb, int nr,
                   const uaesk_rk *ek, const uaesk_rk *dk, int mode, const uint8_t *iv16,
                   const void *in, size_t len, void *out);

/* Batches of independent serial chains, one lane per message (all device pointers).
 * mac == 0: AES_CBC_encrypt (CS3) of nmsg messages of msg_bytes (multiple of 16) each, message m
 * at in + m*msg_bytes with IV ivs[m]; mac != 0: AES_CMAC of each message into out + 16 m.    */
int uaesk_chain_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mac,
                      const void *ivs, size_t nmsg, size_t msg_bytes, const void *in, void *out);

/* Batches of the plain cipher modes, sixteen lanes per record (k_cipher_batch, uaes_cipher_batch.hip); all device
 * pointers at any byte offset (lens: 4-byte aligned).  mode = enum uaes_cipher_batch_mode (uaes_plan.h).  Record m: text
 * at in / out + m msg_bytes, its first lens[m] bytes (lens NULL: msg_bytes; the three CBC modes ignore lens and want
 * msg_bytes a multiple of 16, >= 16), IV -- CTR: first counter block -- at ivs + 16 m.  ek / dk: encryption /
 * equivalent-inverse keys (the two decrypting CBC modes read dk, the others ek).  in == out is fine in every mode.
 * The plan (uaesk_plan_cipher_batch, uaes_plan.h) is one row, cipher.batch. */
int uaesk_cipher_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int mode,
                       const void *ivs, size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out);

/* Batches of XTS data units, sixteen lanes per unit (k_xts_batch, uaes_xts_batch.hip); all device pointers at any byte
 * offset (lens: 4-byte aligned).  Unit m: text at in / out + m msg_bytes (16 <= msg_bytes <= UINT32_MAX), its first
 * lens[m] bytes (lens NULL: msg_bytes), tweak at tweaks + m tweak_bytes: 16 raw bytes, or 8, a sector number whose
 * LE128 is the tweak.  k1: key 1's encryption schedule, decrypting its equivalent-inverse one; k2: key 2's encryption
 * schedule.  A unit whose length is below 16 is left unwritten and sets bit 0 of *bad; bad is not touched without lens.
 * in == out is fine.  The plan (uaesk_plan_xts_batch, uaes_plan.h) is one row, xts.batch. */
int uaesk_xts_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *k1, const uaesk_rk *k2, int decrypt,
                    const void *tweaks, unsigned tweak_bytes, size_t nmsg, size_t msg_bytes, const void *lens,
                    const void *in, void *out, int *bad);

/* OCB (AES_OCB_encrypt/decrypt, micro_aes.c:1693-1811): nonce (host) of nonce_len = 1..15 bytes, tag_len
 * (1..16) bytes of tag at out+len (encrypt) / read at in+len (decrypt, *status = 0 / 0x1A; the text
 * is written either way, as in the reference).  dk = equivalent-inverse keys.  ONE launch; done_word = a device
 * word that is zero between calls and that nothing else writes (the launch's workgroups count themselves in on it
 * and the last one to arrive computes the tag and puts the zero back).  */
size_t uaesk_ocb_scratch_bytes(void);
int uaesk_ocb(void *stream, const uaesk_tables *tb, int nr,
              const uaesk_rk *ek, const uaesk_rk *dk, int decrypt, const uint8_t *nonce,
              size_t nonce_len, size_t tag_len,
              const void *aad, size_t aad_len, const void *in, size_t len, void *out,
              void *scratch, unsigned *done_word, int *status);
/* Batch: nmsg records under one key, sixteen lanes per record (k_ocb_batch); all device pointers.  Record m: text at
 * in / out + m msg_bytes (msg_bytes <= UAES_OCB_BATCH_MAX), its first lens[m] bytes (lens NULL: msg_bytes), nonce at
 * nonces + m nonce_len (1..15), AAD at aad + m aad_bytes (<= UAES_OCB_BATCH_MAX), tag at tags + m tag_len (1..16).
 * dk = equivalent-inverse keys (read when decrypting).  decrypt writes verdicts[m] (1 = authentic) and ORs 1 into *bad
 * for a forgery, whose output stays as decrypted or is zeroed when wipe != 0. */
int uaesk_ocb_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int decrypt,
                    int wipe, const void *nonces, size_t nonce_len, size_t tag_len, const void *aad, size_t aad_bytes,
                    size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out, void *tags,
                    void *verdicts, int *bad);

/* A ticket can also ride on the call's ONLY kernel (saves the second launch: 8.9 -> 7 us for an empty kernel,
 * tools/ubench/threadfloor.hip).  The host layer arms one for the calling thread right before a kernel-level call
 * whose last launch may take it (ECB, generic CTR, a one-launch XTS unit, a one-launch GCM encryption); the launcher
 * that does take it makes the kernel release `seq` to *flag when its last workgroup is done (d_count: a zeroed
 * device word for that count).  uaesk_ticket_disarm() = 1 if nobody took it (the host then sends k_ticket).   */
typedef struct {
    unsigned *flag;                 /* pinned host word the host spins on; NULL = no ticket */
    unsigned *count;                /* device word, zero between launches                    */
    unsigned  seq;
} uaesk_done;
void uaesk_ticket_arm(void *pinned_flag, void *d_count, unsigned seq);
/* a device word that is zero between calls and that nothing else writes, for the calling thread's NEXT kernel-level
 * call (uaesk_gcm takes it: with it a medium-sized text is one launch); NULL disarms */
void uaesk_done_word_arm(unsigned *w);
/* test hooks: the preparing workgroup's bounded look (100 MHz ticks; 0 = count in without looking) and the number of
 * folds a CHUNK workgroup has done on the current device (uaes_gcm.hip, "FOLD") */
void uaesk_debug_gcm_look(unsigned long long ticks);
int uaesk_debug_gcm_chunk_folds(unsigned *out);
int  uaesk_ticket_disarm(void);

/* Completion ticket of a synchronous call: a one-wave kernel behind the call's kernels copies nbytes (a multiple
 * of 4, <= 64) from d_src to pinned_dst and then stores seq to *pinned_flag with system-scope release.   */
int uaesk_ticket(void *stream, void *pinned_flag, unsigned seq, const void *d_src, void *pinned_dst, unsigned nbytes);

/* measurement: one wave spins for ticks_100mhz periods of the constant 100 MHz counter and writes
 * { shader cycles, reference ticks } (two 64-bit words) to d_out16                               */
int uaesk_clock_probe(void *stream, void *d_out16, unsigned long long ticks_100mhz);

/* Poly1305-AES (uaes_poly1305.hip).  r16 = the r half of the key pair and nonce16 are HOST memory (clamped and
 * passed as launch arguments); data, mac16 and scratch device memory.  scratch holds uaesk_poly1305_scratch_bytes(len)
 * (0 for the one-workgroup arrangement: NULL is fine then); the call leaves it zeroed.  The batch form takes nmsg
 * messages of msg_bytes each back to back, nonces (16 bytes each) and macs in device memory.                   */
size_t uaesk_poly1305_scratch_bytes(size_t len);
int uaesk_poly1305(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uint8_t *r16,
                   const uint8_t *nonce16, const void *data, size_t len, void *mac16, void *scratch);
int uaesk_poly1305_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uint8_t *r16,
                         const void *nonces, size_t nmsg, size_t msg_bytes, const void *data, void *macs);

/* EAX and SIV, RFC 5297 (uaes_eax_siv.hip); every pointer device memory unless noted.
 * uaesk_eax_small: a text of <= UAES_EAX_SIV_SMALL_MAX bytes in one launch; encrypt writes tag_len (1..16) bytes of
 * tag to tag_io, decrypt compares them with tag_io, writes *status = 0 / 0x1A and writes `out` only when authentic.
 * uaesk_eax_macs: mode 0 = N || H into res48 (N at +16, N ^ H at +32); 1 = N || H || C, the tag compared with tag_io
 * (status at +0, N at +16); 2 = C only over ct, the tag (C ^ N ^ H from res48) to tag_io.
 * uaesk_s2v_small: iv16 (host; decrypt only) = the IV to check; encrypt writes V to iv_out (16 bytes).
 * uaesk_s2v_macs: S2V over text (the plaintext) into res48 (+16; encrypt) or its status against iv16 (+0; decrypt).
 * Batches: record m's text at in / out + m msg_bytes, nonce at nonces + m nonce_len, AAD at aad + m aad_bytes, tag / V
 * at tags / ivs + 16 m; decrypt writes verdicts[m] (1 = authentic) and ORs 1 into *bad for a forgery.            */
int uaesk_eax_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                    const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                    const void *in, size_t len, void *out, void *tag_io, unsigned tag_len, int *status);
int uaesk_eax_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mode,
                   const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                   const void *ct, size_t len, void *tag_io, unsigned tag_len, void *res48);
int uaesk_s2v_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                    int decrypt, const uint8_t *iv16, const void *aad, size_t aad_len,
                    const void *in, size_t len, void *out, void *iv_out, int *status);
int uaesk_s2v_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, int decrypt,
                   const uint8_t *iv16, const void *aad, size_t aad_len, const void *text, size_t len, void *res48);
int uaesk_eax_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                    const void *nonces, size_t nonce_len, const void *aad, size_t aad_bytes,
                    size_t nmsg, size_t msg_bytes, const void *in, void *out, void *tags, void *verdicts, int *bad);
int uaesk_s2v_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                    int decrypt, int wipe, const void *aad, size_t aad_bytes,
                    size_t nmsg, size_t msg_bytes, const void *in, void *out, void *ivs, void *verdicts, int *bad);
/* EAX' (the reference built with EAXP 1; uaes_eax_siv.hip), the same three forms without associated data and with a
 * 4-byte mac at any byte offset.  uaesk_eaxp_small: as uaesk_eax_small (len <= UAES_EAX_SIV_SMALL_MAX).
 * uaesk_eaxp_macs: mode 0 = N into res48 (the counter block N' at +16, N's last four bytes at +32); 1 = N || C', the mac
 * compared with mac_io (status at +0, N' at +16); 2 = C' only over ct, the mac (with +32 of res48) to mac_io.
 * uaesk_eaxp_batch: record m's nonce is the first nlens[m] bytes at nonces + m nonce_bytes, its text the first lens[m]
 * bytes at in / out + m msg_bytes (NULL: the whole slot; else 4-byte aligned device memory, a longer entry counts as the
 * slot), its mac at macs + 4 m; verdicts may be NULL; a forged record's output is not written. */
int uaesk_eaxp_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                     const void *nonce, size_t nonce_len, const void *in, size_t len, void *out, void *mac_io, int *status);
int uaesk_eaxp_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mode,
                    const void *nonce, size_t nonce_len, const void *ct, size_t len, void *mac_io, void *res48);
int uaesk_eaxp_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                     const void *nonces, size_t nonce_bytes, const void *nlens, size_t nmsg, size_t msg_bytes,
                     const void *lens, const void *in, void *out, void *macs, void *verdicts, int *bad);
/* S2V over nad components of associated data (RFC 5297 section 2.4).  uaesk_s2v_v: component i is aad[ends[i - 1] ..
 * ends[i]) with ends = nad running totals of the lengths, uint64 each, device memory, 8-byte aligned (nad <=
 * UAES_S2V_AD_MAX; an empty component is one); ctr != 0: a text of <= UAES_EAX_SIV_SMALL_MAX bytes and CTR in the same
 * launch (uaesk_s2v_small's part), ctr == 0: the chains alone, over `in` (encrypt) or the plaintext in `out` (decrypt;
 * uaesk_s2v_macs' part); res48: the status at +0 (decrypt), V at +16 (encrypt).
 * uaesk_s2v_batch_v: uaesk_s2v_batch with every record's AAD slot cut into nad <= UAES_S2V_BATCH_AD_MAX components of
 * ad_lens[i] bytes (host memory) and lens as uaesk_ccm_batch has it (NULL, or 4-byte aligned device memory). */
int uaesk_s2v_v(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                int decrypt, int ctr, const uint8_t *iv16, const void *aad, const void *ends, unsigned nad,
                const void *in, size_t len, void *out, void *res48);
int uaesk_s2v_batch_v(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                      int decrypt, int wipe, const void *aad, unsigned nad, const size_t *ad_lens,
                      size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out, void *ivs,
                      void *verdicts, int *bad);

/* AES key wrap, RFC 3394 (pad 0; AES_KEY_wrap / AES_KEY_unwrap, micro_aes.c:1829-1894), and key wrap with padding,
 * RFC 5649 (pad 1; the reference has none): uaes_kw.hip; device pointers at any byte offset.  ek / dk: encryption /
 * equivalent-inverse keys (wrap reads ek, unwrap dk).  in and out are disjoint, or the secret sits 8 bytes into the
 * wrapped buffer.
 * pad 0: len = bytes of the secret (a multiple of 8, >= 16) in both directions.  wrap: in = the secret, out receives
 * len + 8 bytes; unwrap: in = the wrapped form (len + 8 bytes), out receives the secret whatever the verdict and
 * *status = 0 / 0x1A.
 * pad 1: wrap: in = the secret of len bytes (1 .. 2^32 - 1), out receives 8 ceil(len / 8) + 8 bytes.  unwrap: in = the
 * wrapped form, len = its bytes - 8 (a multiple of 8), out receives len bytes whatever the verdict, status[0] = 0 / 0x1A
 * and status[1] = the length indicator of an authentic secret / 0.  No byte beyond the len bytes of a short secret is read.
 * Batch, pad 0: nkeys records of rec bytes of secret (<= UAES_KW_BATCH_MAX) back to back, wrapped record m at
 * m (rec + 8); lens and lens_out are not read (NULL).
 * Batch, pad 1: nkeys slots.  wrap: rec = bytes per secret slot (1 .. UAES_KW_BATCH_MAX), the wrapped slot is
 * 8 ceil(rec / 8) + 8; lens (NULL: every record fills its slot) = u32 per record, 1 .. rec, else the record is skipped and
 * 2 is ORed into *bad.  unwrap: rec = the wrapped slot - 8; lens = bytes of each wrapped record (NULL: the slot), a
 * multiple of 8 in 16 .. rec + 8, else the record fails unwritten; lens_out[m] = the length indicator / 0.  lens and
 * lens_out are 4-byte aligned.
 * Either batch: unwrap writes verdicts[m] (1 = authentic), ORs 1 into *bad for a record that fails and zeroes a forged
 * record when wipe. */
int uaesk_kw(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int pad, int unwrap,
             const void *in, size_t len, void *out, int *status);
int uaesk_kw_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk, int pad,
                   int unwrap, int wipe, size_t nkeys, size_t rec, const void *lens, const void *in, void *out,
                   void *lens_out, void *verdicts, int *bad);

/* FF1, SP 800-38G (uaes_ff1.hip; AES_FPE_encrypt / AES_FPE_decrypt with FF_X 1, micro_aes.c:2091-2147, :2267-2314).
 * What depends on (radix, len, tweak length, alphabet) alone is made once on the host: b and d with exact integers,
 * the P block as four little-endian column words, inv = byte -> digit value (0xFF: no numeral; every byte is one at
 * radix 256) and fwd = digit value -> byte.  nrec 0: one text of q->len numerals (a batch of one up to
 * UAES_FF1_BATCH_MAX, a wave of its own beyond); nrec >= 1: records back to back, record m's tweak at tweaks +
 * m * tweak_stride (0: one tweak for all).  Device pointers at any byte offset; in == out is fine.  verdicts (may be
 * NULL) receives 1 / 0 per record; a record with a byte that is no numeral is left unwritten and ORs 1 into *bad. */
typedef struct {
    unsigned           radix, len, b, d;
    unsigned long long tweak_len, tweak_stride;
    unsigned           p[4];
    unsigned char      inv[256], fwd[256];
} uaesk_ff1;
int uaesk_ff1_run(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt, const uaesk_ff1 *q,
                  const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad);

/* FF3-1, SP 800-38G revision 1 (uaes_ff3.hip; AES_FPE_encrypt / AES_FPE_decrypt with FF_X 3, micro_aes.c:2150-2248,
 * :2267-2314).  ek = the round keys of the key with its BYTES REVERSED (the host reverses it before expansion); inv and
 * fwd as in uaesk_ff1.  nrec 0: one text of q->len numerals, a batch of one; nrec >= 1: records back to back, record m's
 * seven-byte tweak at tweaks + m * tweak_stride (0: one tweak for all).  Device pointers at any byte offset; in == out
 * is fine.  verdicts (may be NULL) receives 1 / 0 per record; a record with a byte that is no numeral is left unwritten
 * and ORs 1 into *bad. */
typedef struct {
    unsigned           radix, len;
    unsigned long long tweak_stride;
    unsigned char      inv[256], fwd[256];
} uaesk_ff3;
int uaesk_ff3_run(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt, const uaesk_ff3 *q,
                  const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad);

/* Device self-test of the primitives; writes a bitmask of failures.        */
int uaesk_selftest(void *stream, const uaesk_tables *tb, const uaesk_rk *ek128,
                   const uaesk_rk *dk128, unsigned *d_result);

#ifdef __cplusplus
}
#endif
#endif
