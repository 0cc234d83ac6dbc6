/*
 * uaes_hip.h -- C ABI of the MI355X-native AES engine (libuaes_hip.so).
 *
 * This is the drop-in boundary for the hot path of polfosol/micro-AES: the
 * block-parallel mode drivers ECB / CTR / XTS / GCM.  Every entry point below
 * names the reference interface it replaces (paths relative to the reference
 * checkout).  Differences from the reference API, all of them additive:
 *
 *   - the key size is a run-time argument (`keybits` = 128/192/256) instead of
 *     the compile-time macro AES___ (micro_aes.h:17).  include/micro_aes.h
 *     restores the macro API on top of these functions;
 *   - no global state: the reference keeps one static RoundKey
 *     (micro_aes.c:72) and is not re-entrant; this library is thread-safe AND concurrent:
 *     every host thread runs its synchronous calls on its own HIP stream with its own staging,
 *     so calls from different threads overlap on the GPU (no lock is held while it works);
 *   - data pointers may be HOST or DEVICE (HIP) pointers.  Host buffers are
 *     staged through device memory; device buffers are used in place.
 *     Keys, IVs, nonces and tweaks are always host pointers (<= 64 bytes);
 *   - `in == out` is allowed everywhere (the reference memcpy()s in -> out and
 *     works in place, micro_aes.h:520-526); partial overlap is undefined;
 *   - *_dev variants enqueue on a caller-supplied hipStream_t and return
 *     without synchronising: the form bench.py and multi-GPU sharding use.
 *
 * By DEFAULT every call runs on the GPU and there is no CPU fallback: if no HIP
 * device is usable every call fails loudly (UAES_E_HIP, message in
 * uaes_last_error()).  A deployer may switch on the engine's own host data path
 * for short host-pointer calls, single serial chains and GPU-less boxes:
 * uaes_set_host_policy() below -- opt-in, never silent.
 *
 * Return values: 0 on success; the reference's codes (micro_aes.h:469-476)
 * for the reference's error conditions; negative for engine failures.
 */
#ifndef UAES_HIP_H_
#define UAES_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAES_OK                0
#define UAES_E_DATALENGTH      1      /* M_DATALENGTH_ERROR     (0x1L)  */
#define UAES_E_AUTHENTICATION  0x1A   /* M_AUTHENTICATION_ERROR         */
#define UAES_E_DECRYPTION      0x1D   /* M_DECRYPTION_ERROR             */
#define UAES_E_ENCRYPTION      0x1E   /* M_ENCRYPTION_ERROR             */
#define UAES_E_HIP            (-1)    /* HIP runtime / device failure   */
#define UAES_E_ARG            (-2)    /* bad keybits / NULL / alignment */

/* ---- housekeeping ------------------------------------------------------ */
/* Initialise the engine on the calling thread's current HIP device (idempotent;
 * every other call does this lazily).                                        */
int         uaes_init(void);
/* Give back everything the library holds on every device: the per-thread lanes of the synchronous
 * API (stream, staging, pinned bounce buffers, scratch), the slice pipeline's streams and buffers,
 * the per-stream scratch of the *_dev API and the tables.  Waits for the devices' outstanding work.
 * No other call may be in flight; the next call after it sets the library up again.  Key contexts
 * and GCM streams are the caller's objects and are not touched.                               */
int         uaes_shutdown(void);
/* Run the on-device primitive self test (FIPS-197 C.1 both directions, byte
 * permute semantics, tweak arithmetic).  0 = pass, >0 = failure bitmask.     */
int         uaes_selftest(void);
/* Measurement aid: one wave on `stream` spins for spin_us microseconds of the constant 100 MHz counter and writes
 * { shader cycles elapsed, 100 MHz ticks elapsed } (two uint64) to d_out16 -- the shader clock the chip really runs
 * at while other streams load it (bench.py reports it beside the roofline).  Enqueue only.                    */
int         uaes_clock_probe_dev(void *d_out16, unsigned spin_us, void *stream);
/* Thread-local description of the last negative return value.               */
const char *uaes_last_error(void);
/* "uaes-hip <version> gfx950"                                               */
const char *uaes_version(void);
/* What CCM / GCM-SIV / OCB decryption leaves in pntxt when the tag is wrong.  These three
 * modes decrypt before they authenticate; the reference's default build then returns 0x1A
 * WITH the unauthenticated text in place (SABOTAGE is a no-op, micro_aes.c:1306-1312,
 * :1500-1511, :1803-1810) and that is this library's default too, so results are
 * bit-identical.  on != 0 selects the reference's INCREASE_SECURITY behaviour instead: the
 * buffer is zeroed.  Process-wide; returns the previous setting.  (The *_dev calls of those
 * three modes report through d_status and leave the decision to the caller.)
 * GCM never releases unauthenticated text (N7) and is not affected by this switch.               */
int         uaes_set_wipe_on_auth_failure(int on);
/* GCM decryption into a caller's DEVICE buffer reads the ciphertext twice by default (GHASH, tag check, then
 * CTR: 1.5x the traffic), because nothing may be written before the tag is known (N7, micro_aes.c:1204-1210).
 * on != 0: a long text is decrypted and hashed in ONE pass (8 % faster at 1 GiB) and, when the tag turns out
 * wrong, everything written is zeroed before 0x1A / a non-zero *d_status is reported -- between the launch and that
 * moment the buffer holds unauthenticated plaintext, which other streams could observe: that is what the caller
 * accepts by switching this on.  Process-wide; returns the previous setting.  Host-memory callers get the one-pass
 * kernel regardless: their plaintext is produced in a private staging buffer that is copied out only after the
 * tag has been verified.                                                                                   */
int         uaes_set_gcm_one_pass_decrypt(int on);
/* The *_dev calls keep a device scratch buffer (GHASH tables, XTS chunk tweaks) per
 * hipStream_t they have been used with (8 per device; beyond that the least recently
 * used one is recycled after a device-wide drain).  Call this when a stream will not
 * be used with the library any more -- before or after hipStreamDestroy -- to give
 * its buffer back.  Waits for the device's outstanding work.                       */
int         uaes_stream_release(void *stream);

/* The engine's own HOST data path (micro-aes_amd/csrc/uaes_host.c: portable table-driven C, re-entrant, bit-identical to
 * the kernels and parity-tested like them).  OFF by default -- max_bytes 0, chains 0, fallback 0: every call runs on the
 * GPU and fails loudly without one.  Three independent, process-wide switches for the cases a GPU serves badly:
 *   max_bytes  calls whose data pointers are HOST memory and whose text is at most this long run on the host: a
 *              launch costs 12-20 us whatever the size, one host core needs that long for ~1 KiB (GCM ~200 B);
 *   chains     ONE serial chain in host memory -- CBC / CFB encryption, OFB, CMAC, CCM, key wrap, FF1, FF3-1 -- runs on the host whatever
 *              its length (a chain is a latency-bound single wave on the GPU: 36 MiB/s; uaes_*_batch are the GPU's form);
 *   fallback   with NO usable HIP device the calls below run on the host instead of returning UAES_E_HIP -- the
 *              reference's `void` functions cannot report an error.
 * Covered: every synchronous one-message call of this header -- ECB, CTR, XTS (unit and sectors), GCM (any nonce / tag
 * length), CBC (CTS and CTS-0 forms), CFB, OFB, CMAC, CCM, GCM-SIV, OCB, KW, KWP, FF1, FF3-1.  Not covered (always GPU): the *_dev / *_batch
 * / record / key-context / stream / mgpu calls, uaes_ghash, and any call that is handed a device pointer.
 * Environment, read at first use: UAES_HOST_MAX=<bytes>, UAES_HOST_CHAINS=1, UAES_HOST_FALLBACK=1; or
 * UAES_HOST_POLICY=recommended = (4096, 1, 1), the measured crossover on the builder's hosts (profiles/r05_host_policy.md),
 * which the three variables then refine.                                                                           */
int uaes_set_host_policy(size_t max_bytes, int chains, int fallback);
int uaes_get_host_policy(size_t *max_bytes, int *chains, int *fallback);

/* Host-side key schedule (KeyExpansion, micro_aes.c:144-178) as the kernels
 * receive it: (nr+1)*4 little-endian words of encryption round keys and of
 * the equivalent-inverse-cipher keys.  Returns nr (10/12/14) or a negative
 * error.  Diagnostic: needs no GPU.                                         */
int uaes_expand_key(int keybits, const uint8_t *key,
                    uint32_t enc_words[60], uint32_t dec_words[60]);

/* ---- ECB: replaces AES_ECB_encrypt / AES_ECB_decrypt --------------------
 * micro_aes.h:173-181, micro_aes.c:636-680.  encrypt writes ceil(len/16)*16
 * bytes (a trailing partial block is zero padded, AES_PADDING 0); decrypt
 * processes floor(len/16) blocks, copies a ragged tail through unchanged and
 * returns UAES_E_DECRYPTION if len % 16 != 0.                               */
int uaes_ecb_encrypt(int keybits, const uint8_t *key,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_ecb_decrypt(int keybits, const uint8_t *key,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
/* padding = the reference's compile-time AES_PADDING (micro_aes.h:79; padBlock,
 * micro_aes.c:610-621): 0 as above; 1 PKCS#7 (n bytes of value n), 2 ISO/IEC 7816-4
 * (0x80, zeros).  1 and 2 always append a block: (ptextLen / 16 + 1) * 16 bytes are
 * written.  Decryption does not strip padding (nor does the reference's, :676-679). */
int uaes_ecb_encrypt_padded(int keybits, const uint8_t *key, int padding,
                            const void *pntxt, size_t ptextLen, void *crtxt);

/* ---- CTR: replaces AES_CTR_encrypt / AES_CTR_decrypt --------------------
 * micro_aes.h:256-266, micro_aes.c:962-990.  iv = 12 bytes (CTR_IV_LENGTH);
 * counter block = iv || 00000001 (CTR_START_VALUE); the counter is the
 * reference's 56-bit big-endian integer in bytes 9..15 (incBlock,
 * micro_aes.c:421-427).  Decrypt is the same function.                      */
int uaes_ctr_xcrypt(int keybits, const uint8_t *key, const uint8_t *iv,
                    const void *in, size_t len, void *out);
/* the same of a reference build with other CTR_IV_LENGTH / CTR_START_VALUE (micro_aes.h:98-99): counter block =
 * iv[0..ivLen) || zeros, startValue XORed in big-endian ending at byte 15 (micro_aes.c:968-971); ivLen <= 16     */
int uaes_ctr_xcrypt_iv(int keybits, const uint8_t *key, const uint8_t *iv, size_t ivLen, uint64_t startValue,
                       const void *in, size_t len, void *out);
/* Sharding extension: full 16-byte initial counter block (what the reference
 * builds internally, or takes directly when PRESET_COUNTER is 1,
 * micro_aes.h:100) plus a block offset added with the same 56-bit carry.
 * Rank g of a sharded stream passes block_offset = g * blocks_per_shard.    */
int uaes_ctr_xcrypt_at(int keybits, const uint8_t *key, const uint8_t ctr0[16],
                       uint64_t block_offset,
                       const void *in, size_t len, void *out);
/* Batch: nmsg records in slots of msg_bytes, a counter block each, one launch -- a cipher batch; its conventions (lens,
 * memory, in place, refusals) stand with uaes_cbc_decrypt_batch below.  ctrs + 16 m = record m's first counter block,
 * as uaes_ctr_xcrypt_at(.., ctr0, 0, ..): 56-bit counter in bytes 9..15, with the reference's carry and wrap; bytes
 * 0..8 never change.  Any record length: there is no cap on a record's blocks. */
int uaes_ctr_xcrypt_batch(int keybits, const uint8_t *key, const uint8_t *ctrs, size_t nmsg,
                          size_t msg_bytes, const uint32_t *lens, const void *in, void *out);

/* ---- XTS: replaces AES_XTS_encrypt / AES_XTS_decrypt --------------------
 * micro_aes.h:239-249, micro_aes.c:1008-1093.  keys = key1 || key2
 * (2*keybits/8 bytes; key2 encrypts the tweak).  tweak = 16 raw bytes, or
 * NULL for data unit 0.  len < 16 -> UAES_E_DATALENGTH, output untouched.
 * Ciphertext stealing when len % 16 != 0.                                   */
int uaes_xts_encrypt(int keybits, const uint8_t *keys, const uint8_t *tweak,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_xts_decrypt(int keybits, const uint8_t *keys, const uint8_t *tweak,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batch extension: nsectors data units of sector_bytes each in one call; unit
 * i uses the tweak block LE128(first_sector + i) -- the reference's own
 * `sectid` convention (XTS_cipher, micro_aes.c:1017-1021).                  */
int uaes_xts_sectors(int keybits, const uint8_t *keys, uint64_t first_sector,
                     size_t sector_bytes, size_t nsectors,
                     const void *in, void *out, int encrypt);
/* Batches: nmsg data units in slots of msg_bytes, a tweak each, one launch (k_xts_batch: sixteen GPU lanes per unit).
 * The conventions are the cipher batches' (uaes_ctr_xcrypt_batch): unit m lies at m * msg_bytes in both texts, the calls
 * always run on the GPU (no host policy), every array is host or device memory, in == out works (partial overlap is
 * undefined); there are no *_dev and no uaes_mgpu_* forms.  keys = key1 || key2 in host memory.
 * tweaks = nmsg * 16 raw bytes at any byte offset: unit m is bit for bit what uaes_xts_encrypt / uaes_xts_decrypt give
 * for it with the tweak at tweaks + 16 m, ciphertext stealing included when its length is no multiple of 16.
 * lens = NULL (every unit is msg_bytes long) or nmsg 32-bit lengths (device memory: 4-byte aligned, else UAES_E_ARG):
 * unit m is the first lens[m] bytes of its slot, an entry above msg_bytes counts as msg_bytes, the rest of an output
 * slot is not written (a host output is copied in first, so it stays the caller's).  An entry below 16, zero included,
 * writes nothing for that unit; every other unit is finished and the call returns UAES_E_DATALENGTH, as
 * uaes_kwp_wrap_batch has it.  Without lens no status word is armed or fetched.
 * Refusals, in this order and before the device is touched: msg_bytes > UINT32_MAX or a size that overflows ->
 * UAES_E_ARG; a NULL key pair or keybits other than 128 / 192 / 256 -> UAES_E_ARG; nmsg == 0 -> 0, nothing else looked
 * at; msg_bytes < 16 -> UAES_E_DATALENGTH, output untouched; a NULL tweaks / text pointer -> UAES_E_ARG.
 * uaes_xts_sector_list is the storage form: unit m's tweak is LE128(sectors[m]), eight bytes per unit instead of
 * sixteen; the sectors come in any order and may repeat (a block layer's request list); every unit is sector_bytes long
 * (520 steals per unit) and there is no lens.  A contiguous ascending list gives what uaes_xts_sectors gives -- and a
 * contiguous run of equal sectors remains that call's job: it spreads a unit's blocks over many lanes, where a batch
 * walks a unit on sixteen.
 * Measured (profiles/xts_batch_rate.md; device-resident arrays, synchronous calls, AES-128, AES-256 in brackets): 2^10
 * units of 16 bytes take 21.2 (21.6) us as ONE call, decrypting 22.4 (22.8), against 14.1 (16.2) us for EACH of 2^10
 * one-unit uaes_xts_encrypt calls.  2^20 units of 16 / 64 / 512 / 1024 / 4096 bytes encrypt in 226 / 302 / 1148 / 2211 /
 * 8935 us (248 / 349 / 1453 / 2817 / 11317), 4.6 G units/s at 16 bytes and 434 .. 452 GiB/s from 512 bytes on; decrypting
 * takes 0 .. 4 % longer and the sector list as long as the batch.  Against uaes_ctr_xcrypt_batch at the same shape that
 * is 1.25 / 1.19 / 1.08 / 1.06 / 1.05 x its time, where the row steps alone would give 2 / 1.5 / 1.06 / 1.03 / 1.01.
 * For a CONTIGUOUS run of 2^20 equal sectors uaes_xts_sectors wins from 64 bytes per unit on (83 us against 302 at 64
 * bytes, 443 against 1148 at 512, 3070 against 8935 at 4096); only at 16-byte units is the batch the faster call. */
int uaes_xts_encrypt_batch(int keybits, const uint8_t *keys, const uint8_t *tweaks, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *pntxt, void *crtxt);
int uaes_xts_decrypt_batch(int keybits, const uint8_t *keys, const uint8_t *tweaks, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *crtxt, void *pntxt);
int uaes_xts_sector_list(int keybits, const uint8_t *keys, const uint64_t *sectors, size_t nsectors,
                         size_t sector_bytes, const void *in, void *out, int encrypt);

/* ---- GCM: replaces AES_GCM_encrypt / AES_GCM_decrypt --------------------
 * micro_aes.h:294-308, micro_aes.c:1164-1212.  12-byte nonce (GCM_NONCE_LEN),
 * 16-byte tag (GCM_TAG_LEN) appended at crtxt + ptextLen.  decrypt takes
 * CT || tag with crtxtLen excluding the tag, authenticates BEFORE decrypting
 * and on mismatch returns UAES_E_AUTHENTICATION leaving pntxt untouched.     */
int uaes_gcm_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_gcm_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
/* The same with a nonce of any length >= 1 -- the reference's compile-time GCM_NONCE_LEN
 * (micro_aes.h:108): 12 is the default above; otherwise J0 = GHASH_H(nonce) (GCMsetup,
 * micro_aes.c:1145-1149), and the keystream steps it with the reference's 56-bit incBlock.
 * J0 is computed on the GPU and read back (16 bytes), so these are synchronous calls.      */
int uaes_gcm_encrypt_iv(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_gcm_decrypt_iv(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt);
/* ... and with the reference's compile-time GCM_TAG_LEN (micro_aes.h:109) as tagLen = 1..16: tagLen bytes of the
 * tag are appended at crtxt + ptextLen / compared (micro_aes.c:1178, :1204).  A truncated tag is compared on the
 * host (constant time) after the device has produced the full one; nothing is decrypted before that (N7).    */
int uaes_gcm_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_gcm_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batches with A KEY PER RECORD -- what GCM is terminated in bulk for (TLS, QUIC, IPsec ESP, SRTP, per-object storage
 * keys) is many short packets of which almost every one belongs to another session and so has another key; one
 * uaes_gcm_encrypt per packet redoes the key schedule, H and its table kernel every time, and a uaes_gcm_key context
 * per session with one *_records launch each costs the same when a session has a handful of packets.  Here every record
 * expands its own key schedule and hashes under its own H, all in the kernel (csrc/uaes_gcm_multikey.hip).  The
 * conventions are those of the CCM, GCM-SIV and OCB batches: nmsg records in slots of msg_bytes back to back (record m
 * at m * msg_bytes), sixteen GPU lanes per record, one kernel launch, always on the GPU (the host policy does not
 * apply).  keys = nmsg * keybits / 8 bytes, PACKED: record m works under the key at keys + m * keybits / 8, and one
 * keybits serves the whole call.  keys may be host OR DEVICE memory at any byte offset -- the first key argument of this
 * header that may be device memory.  A table of keys with per-record indices is out of scope: the caller gathers the
 * keys into the packed array.  A host key array travels through the engine's device scratch, and that copy is cleared
 * in stream order before the call returns; on the device a schedule exists only in LDS and registers.  nonces = nmsg *
 * 12 bytes (J0 = nonce || 00000001), aData = nmsg * aad_bytes (aad_bytes 0: no AAD, the pointer may be NULL), tags =
 * nmsg * tagLen bytes (tagLen 1..16: the first tagLen bytes of each tag), PACKED, not appended to the texts.  lens (may
 * be NULL: every record is msg_bytes long) = nmsg 32-bit lengths: record m is the first lens[m] <= msg_bytes bytes of
 * its slot (a longer entry is taken as msg_bytes) and the bytes of an output slot beyond lens[m] are not written.  Every
 * record is bit for bit what uaes_gcm_encrypt_ex / uaes_gcm_decrypt_ex give for it under its key with nonceLen 12 and
 * this tagLen, at all three key sizes.  Decrypt keeps N7 per record, as uaes_gcm_key_decrypt_records does: a record is
 * hashed first and its text is written only if the tag matches, so a forged record's output slot is UNTOUCHED (with
 * crtxt == pntxt it stays ciphertext); verdicts[m] = 1 (authentic) / 0 (required), the call returns 0 when every record
 * is authentic, else UAES_E_AUTHENTICATION, and uaes_set_wipe_on_auth_failure does not apply.  UAES_E_ARG (before the
 * device is touched): key bits other than 128 / 192 / 256, tagLen outside 1..16, msg_bytes or aad_bytes > 65535
 * (UAES_GCM_MULTIKEY_BATCH_MAX, csrc/uaes_plan.h: a record then has at most 4096 counter blocks; beyond it a key
 * context per key is the right tool), a size product that overflows, a needed pointer that is NULL (keys and verdicts
 * included).  nmsg == 0 returns 0 after the length and key-size checks.  Every array host or device memory at any byte
 * offset (lens: 4-byte aligned device memory, or host memory); crtxt == pntxt works.  A host-memory output of a
 * decryption, or of any call with lens, is copied in first, so that what the kernel leaves unwritten stays the caller's.
 * Measured on an MI355X (tools/gcm_multikey_rate.py -> profiles/gcm_multikey_batch_rate.md; device-resident arrays and
 * keys, 12 bytes of AAD, 16-byte tags; synchronous calls, the host round trip included), AES-128 and AES-256, encrypt /
 * decrypt:
 *   2^10 records of 16 B     22.3 / 37.3 and 22.8 / 37.8 us per call  (2^10 uaes_gcm_encrypt calls, a key each: 16.6 / 17.3 us EACH)
 *   2^20 records of 16 B     2.29 / 1.84 and 2.06 / 1.69 G records per second
 *   2^20 records of 64 B     1.58 / 1.35 and 1.41 / 1.21 G records per second
 *   2^20 records of 1024 B   0.204 / 0.211 and 0.177 / 0.188 G records per second
 * 0.70 .. 1.07x the time of uaes_gcmsiv_encrypt_batch / _decrypt_batch under ONE key at the same shape, and 0.24 .. 0.36x
 * that of uaes_gcm_key_encrypt_records / _decrypt_records under one key at 16 and 64 bytes, 1.03 .. 1.09x at 1024. */
int uaes_gcm_multikey_encrypt_batch(int keybits, const uint8_t *keys, size_t tagLen,
                                    size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                    const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                    const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_gcm_multikey_decrypt_batch(int keybits, const uint8_t *keys, size_t tagLen,
                                    size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                    const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                    const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);
/* XAES-256-GCM, the C2SP specification c2sp.org/XAES-256-GCM: AES-256-GCM with a 192-bit nonce.  RANDOM 24-BYTE NONCES
 * ARE THE POINT: GCM's 96-bit nonce makes a caller with random nonces stop at about 2^32 messages per key, and many
 * senders -- the workload the batches were built for -- cannot share a nonce counter.  Here the first half of the nonce
 * makes a fresh AES-256 key, Kx = CMAC_K(00 01 58 00 || N[0:12]) || CMAC_K(00 02 58 00 || N[0:12]) (SP 800-108, counter
 * mode), and plain AES-256-GCM runs under Kx with N[12:24] as its nonce.  The bound on messages per key is therefore
 * the specification's (2^80 messages of random nonces for a collision risk of 2^-32), not GCM's.  The key is always 32
 * bytes, the nonce 24, the tag 16: the specification has nothing else, so nothing else is offered (no *_dev variants,
 * no key contexts -- the working key belongs to the nonce -- and the reference has no such call to be compatible with).
 *   uaes_xaes256gcm_derive   kx <- Kx; three blocks of the host cipher, no device is touched.
 *   uaes_xaes256gcm_encrypt / _decrypt   arguments, return codes, host or device pointers and what a failed
 *       authentication leaves behind as uaes_gcm_encrypt / uaes_gcm_decrypt: crtxt receives ptextLen + 16 bytes, crtxt of
 *       a decryption holds crtxtLen + 16.  Kx is derived on the host and the call then IS the one-call GCM path under it:
 *       the fused kernels for a long text, the host data path for a short one where uaes_set_host_policy switched it on.
 *       Kx, K1 and both schedules are wiped on every way out.  UAES_E_ARG for a NULL key or nonce, before any device is
 *       touched.
 *   uaes_xaes256gcm_encrypt_batch / _decrypt_batch   nmsg records under one master key in ONE launch, sixteen GPU
 *       lanes per record (csrc/uaes_xaes.hip): every record derives Kx, expands it and runs GCM under it in the kernel,
 *       where Kx lives in LDS and registers only.  Array layout, lens, placement (every array host or device memory at
 *       any byte offset; lens 4-byte aligned device memory, or host memory) and return codes as uaes_gcmsiv_*_batch, with
 *       nonces = nmsg * 24 bytes and tags = nmsg * 16.  Decrypt as uaes_gcm_multikey_decrypt_batch: a record is hashed
 *       first and written only if its tag matches, so a forged record's output slot is UNTOUCHED whatever
 *       uaes_set_wipe_on_auth_failure says; verdicts[m] = 1 / 0 (verdicts may be NULL: the return code still
 *       tells); the call returns UAES_E_AUTHENTICATION if any record was forged.  UAES_E_ARG (before the device is
 *       touched): msg_bytes or aad_bytes > 65535 (UAES_XAES_GCM_BATCH_MAX, csrc/uaes_plan.h: the multi-key bound, for the
 *       same reason), a size product that overflows, a needed pointer that is NULL.  nmsg == 0 returns 0.  Always on the
 *       GPU: the host policy does not apply.  Every record is bit for bit what uaes_xaes256gcm_encrypt / _decrypt give
 *       for it.  Measured on an MI355X (tools/gcm_multikey_rate.py --xaes -> profiles/xaes_gcm_batch_rate.md; device-
 *       resident arrays, 12 bytes of AAD; synchronous calls), encrypt / decrypt: 2^20 records of 16 B 1.80 / 1.53, of 64 B
 *       1.29 / 1.13, of 1024 B 0.176 / 0.187 G records per second: 1.14 .. 1.01x the time of
 *       uaes_gcm_multikey_encrypt_batch / _decrypt_batch at AES-256 on the same texts (one more two-block step a record). */
int uaes_xaes256gcm_derive(const uint8_t key[32], const uint8_t nonce[24], uint8_t kx[32]);
int uaes_xaes256gcm_encrypt(const uint8_t key[32], const uint8_t nonce[24], const void *aData, size_t aDataLen,
                            const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_xaes256gcm_decrypt(const uint8_t key[32], const uint8_t nonce[24], const void *aData, size_t aDataLen,
                            const void *crtxt, size_t crtxtLen, void *pntxt);
int uaes_xaes256gcm_encrypt_batch(const uint8_t key[32], size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                  const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                  const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_xaes256gcm_decrypt_batch(const uint8_t key[32], size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                                  const uint8_t *nonces, const void *aData, size_t aad_bytes,
                                  const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);
/* GHASH_H(aData, crtxt) of micro_aes.c:1127-1137 with an explicit H (test
 * hook for the carry-less-multiply kernels); gh receives 16 bytes.           */
int uaes_ghash(const uint8_t H[16], const void *aData, size_t aDataLen,
               const void *crtxt, size_t crtxtLen, uint8_t gh[16]);

/* ---- CMAC: replaces AES_CMAC ----------------------------------------------
 * micro_aes.h (CMAC section), micro_aes.c:1108-1118.  A CBC-MAC chain is serial:
 * one GPU lane walks it (kept on the device so that no cipher code runs on the
 * host); ~36 MiB/s for one message (latency-bound); uaes_cmac_batch for many.          */
int uaes_cmac(int keybits, const uint8_t *key,
              const void *data, size_t dataSize, uint8_t mac[16]);

/* ---- CCM: replaces AES_CCM_encrypt / AES_CCM_decrypt ----------------------
 * micro_aes.c:1268-1314.  11-byte nonce (CCM_NONCE_LEN), 16-byte tag
 * (CCM_TAG_LEN) appended at crtxt + ptextLen.  Like the reference, decrypt
 * runs CTR first and authenticates the result: on a mismatch it returns
 * UAES_E_AUTHENTICATION and the (unauthenticated) text is left in pntxt.     */
int uaes_ccm_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_ccm_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt);

/* The same with the reference's compile-time CCM_NONCE_LEN (7..13) and CCM_TAG_LEN (even, 4..16), micro_aes.h:103-104 */
int uaes_ccm_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_ccm_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batches under one key -- CCM's usual workload is many short packets, and one call per packet costs 13.6-16.8 us
 * whatever its size.  nmsg records in slots of msg_bytes back to back (record m at m * msg_bytes), sixteen GPU lanes
 * per record, one kernel launch, always on the GPU (the host policy does not apply).  nonces = nmsg * nonceLen bytes,
 * aData = nmsg * aad_bytes (aad_bytes 0: no AAD), tags = nmsg * tagLen bytes, PACKED (a CCM tag is defined by its
 * length), not appended to the texts.  lens (may be NULL: every record is msg_bytes long) = nmsg 32-bit lengths:
 * record m is the first lens[m] <= msg_bytes bytes of its slot (a longer entry is taken as msg_bytes) and the bytes of
 * an output slot beyond lens[m] are not written.  Every record is bit for bit what uaes_ccm_encrypt_ex /
 * uaes_ccm_decrypt_ex give for it.  Decrypt follows the reference per record: the text is written before the tag is
 * known, verdicts[m] = 1 (authentic) / 0, the call returns 0 when every record is authentic, else
 * UAES_E_AUTHENTICATION, and a forged record's output is left as decrypted, or zeros under
 * uaes_set_wipe_on_auth_failure(1).  UAES_E_ARG (before the device is touched): nonceLen outside 7..13, tagLen odd or
 * outside 4..16, msg_bytes > 65535 (UAES_CCM_BATCH_MAX, csrc/uaes_plan.h: the longest text whose length every nonce
 * length can encode), aad_bytes > 0xFEFF (only the two-byte form of the AAD length header is built; the reference's
 * six-byte form for longer AAD is left to the one-message calls), a size product that overflows, a needed pointer that
 * is NULL.  nmsg == 0 returns 0.  key: host memory; every array host or device memory at any byte offset (lens:
 * 4-byte aligned device memory, or host memory); crtxt == pntxt works.  With lens, a host-memory output is copied in
 * first, so that the unwritten remainder of a slot stays the caller's.
 * Measured on an MI355X (tools/ccm_rate.py -> profiles/ccm_batch_rate.md; AES-128, device-resident, 13-byte nonces,
 * 8-byte tags, 13 bytes of AAD; synchronous calls, the host round trip included), encrypt / decrypt:
 *   2^10 records of 16 B     22.8 / 37.6 us per call        (2^10 uaes_ccm_encrypt_ex calls: 18.0 us EACH)
 *   2^20 records of 16 B     3.17 / 2.84 G records per second
 *   2^20 records of 64 B     2.24 / 2.08 G records per second  (134 / 124 GiB/s of text)
 *   2^20 records of 1024 B   0.290 / 0.286 G records per second  (277 / 273 GiB/s of text)
 * 0.79 .. 0.92x the time of uaes_eax_encrypt_batch at the same shape (decrypt: 0.66 .. 0.89x of uaes_eax_decrypt_batch);
 * a decrypting call costs about 15 us more than the encrypting one whatever its size: it clears and fetches the
 * word that says whether any record failed.                                                                     */
int uaes_ccm_encrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_ccm_decrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);

/* ---- EAX and SIV (RFC 5297): replace AES_EAX_* / AES_SIV_* ----------------
 * micro_aes.c:1560-1648 (EAX) and :1323-1411 (SIV).  Host or device pointers, as CCM; the host policy applies.
 * EAX: nonce of any length (0 included; the reference's EAX_NONCE_LEN), tagLen = 1..16 (EAX_TAG_LEN) bytes of
 * N ^ H ^ C appended at crtxt + ptextLen.  Decrypt checks the tag BEFORE it writes: on a mismatch it returns
 * UAES_E_AUTHENTICATION and pntxt is untouched (the wipe switch does not apply).
 * SIV: keys = K_s2v || K_ctr (keybits / 8 bytes each), iv = the 16-byte synthesized IV (out / in); an empty AAD is
 * no header unit.  Decrypt runs CTR first and authenticates the result: on a mismatch it returns
 * UAES_E_AUTHENTICATION and leaves the text in pntxt unless uaes_set_wipe_on_auth_failure(1).
 * in == out works for both.  A text of at most 16 KiB is one kernel launch; a longer one runs its independent CMAC
 * chains at the same time (one launch), reads the counter block back and runs CTR -- the call takes about as long
 * as its longest chain (~0.42 us per AES-128 block).                                                           */
int uaes_eax_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                     const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_eax_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                     const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt);
int uaes_siv_encrypt(int keybits, const uint8_t *keys, const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, uint8_t iv[16], void *crtxt);
int uaes_siv_decrypt(int keybits, const uint8_t *keys, const uint8_t iv[16], const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batches under one key: nmsg records of msg_bytes each back to back (record m at m * msg_bytes), sixteen GPU lanes
 * per record.  EAX: nonces = nmsg * nonce_len bytes, tags = nmsg * 16 (the whole tag); SIV: ivs = nmsg * 16.
 * aData = nmsg * aad_bytes (aad_bytes 0: no AAD).  Decrypt writes verdicts[m] = 1 (authentic) / 0 and returns 0 when
 * every record is authentic, else UAES_E_AUTHENTICATION; EAX leaves a forged record's plaintext untouched, SIV
 * follows the wipe switch per record.  Every array host or device memory.                                      */
int uaes_eax_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_eax_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                           const uint8_t *nonces, size_t nonce_len, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);
int uaes_siv_encrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const void *pntxt, uint8_t *ivs, void *crtxt);
int uaes_siv_decrypt_batch(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes,
                           const void *aData, size_t aad_bytes, const uint8_t *ivs, const void *crtxt, void *pntxt,
                           uint8_t *verdicts);
/* SIV with RFC 5297's VECTOR of associated data (S2V, section 2.4): nad components, then the text.  This is what
 * OpenSSL (AES-128-SIV with several AAD updates), Go, miscreant and Python `cryptography` compute, and nonce-based SIV
 * (section 3, example A.2) is simply the nonce as the LAST component.  aData = the components back to back, host or
 * device memory at any byte offset; adLens[nad] = their lengths, host memory.  Order and boundaries are bound:
 * ("ab","c"), ("a","bc") and ("abc") give three different IVs.
 *   nad == 0                   no component: bit for bit uaes_siv_encrypt with aDataLen == 0
 *   nad == 1, adLens[0] > 0    bit for bit uaes_siv_encrypt
 *   a component of length 0    IS a component: it contributes CMAC("") = Enc(10* ^ K2), so nad == 1 with adLens[0] == 0
 *                              differs from nad == 0.  The one-aData calls' "an empty AAD is no header unit" keeps meaning
 *                              nad == 0 and cannot express this.
 * Everything else is uaes_siv_encrypt / uaes_siv_decrypt: keys, iv, the host policy, in == out, and decrypt runs CTR
 * first, authenticates after, returns UAES_E_AUTHENTICATION on a mismatch and leaves the text unless
 * uaes_set_wipe_on_auth_failure(1).  UAES_E_ARG before the device is touched, in this order: nad > UAES_SIV_AD_MAX,
 * nad != 0 with adLens NULL, lengths whose sum overflows, key bits other than 128 / 192 / 256 (or keys NULL), a NULL
 * iv or text pointer that is needed, a non-zero sum with aData NULL.
 * On the GPU the component CMACs are independent chains: a text of at most 16 KiB is one launch of one workgroup whose
 * sixty rows of sixteen lanes (all but the four of the wave that walks the text) take the components round-robin and
 * leave their CMACs in LDS, then one row folds them, Y_i = dbl(Y_{i-1}) ^ CMAC(S_i); a longer text runs the same kernel
 * without its CTR part beside the positioned CTR kernels, in either direction.  The call costs its longest chain, not
 * the sum.  Measured on an MI355X, AES-128, device-resident arrays, synchronous calls (profiles/siv_v_rate.md): one
 * call with 64 B of text and 1 / 4 / 16 / 64 / 126 components of 64 B takes 49 / 49 / 50 / 56 / 62 us, where
 * uaes_siv_encrypt over the same bytes as one aData (another IV) takes 45 / 50 / 70 / 152 / 262 us.  With ONE component
 * the call takes about 5 us longer than uaes_siv_encrypt at every size measured (49.2 against 43.8 us at 64 B, 494.6
 * against 489.7 us at 16 KiB, 499.7 against 491.5 us at 16 KiB + 1): the running totals are one more copy to the device. */
#define UAES_SIV_AD_MAX        126   /* RFC 5297: S2V takes at most 127 strings, the text included */
#define UAES_SIV_BATCH_AD_MAX    8
int uaes_siv_encrypt_v(int keybits, const uint8_t *keys, size_t nad, const size_t *adLens, const void *aData,
                       const void *pntxt, size_t ptextLen, uint8_t iv[16], void *crtxt);
int uaes_siv_decrypt_v(int keybits, const uint8_t *keys, const uint8_t iv[16], size_t nad, const size_t *adLens,
                       const void *aData, const void *crtxt, size_t crtxtLen, void *pntxt);
/* The batches with the component vector and a length per record: the conventions of uaes_siv_encrypt_batch plus lens.
 * aData = nmsg slots of aad_bytes = sum(adLens) bytes; every slot is cut into the same nad <= UAES_SIV_BATCH_AD_MAX
 * components (adLens: host memory; the lengths go to the kernel by value), so record m is uaes_siv_encrypt_v of its
 * slot's components and its text, bit for bit; with nad == 1 and lens NULL the call is uaes_siv_encrypt_batch byte
 * for byte.  lens has the CCM batch's meaning: NULL (every record is msg_bytes long) or nmsg 32-bit lengths, host
 * memory or 4-byte aligned device memory; record m is the first lens[m] bytes of its slot, an entry above msg_bytes
 * counts as msg_bytes, the rest of an output slot is not written, and a host-memory output is copied in first so that
 * this rest stays the caller's.  A zero length writes no text but still its IV / verdict (SIV of the empty string is
 * defined).  Decrypt writes verdicts[m], follows the wipe switch per record (over the record's lens[m] bytes) and
 * returns UAES_E_AUTHENTICATION if any record fails, as uaes_siv_decrypt_batch.  UAES_E_ARG before the device is
 * touched, in this order: nad > UAES_SIV_BATCH_AD_MAX, nad != 0 with adLens NULL, lengths whose sum overflows,
 * msg_bytes > UINT32_MAX, a misaligned device lens, a size product that overflows, key bits other than 128 / 192 / 256
 * (or keys NULL); then nmsg == 0 returns 0; then a needed pointer that is NULL (aData with a non-zero sum included).
 * A record's row walks its components one after another (they are short), then its text.
 * Measured on an MI355X, AES-128, device-resident arrays (profiles/siv_v_rate.md): 2^20 records of 64 B with the
 * components (13 B, a 16 B nonce) take 615 us in one call, 1.7 G records per second; 2^10 uaes_siv_encrypt_v calls take
 * 43.6 us EACH, so 2^20 of them would take 45.7 s -- the batch is 74 000 times faster.  With one component and no lens
 * the call takes 340 / 591 / 4807 us for 2^20 records of 16 / 64 / 1024 B where uaes_siv_encrypt_batch takes 453 / 739 /
 * 4784 us: CMAC(0^128) is made once per workgroup, not once per record, and the row walks ask for 8 blocks ahead, not 16. */
int uaes_siv_encrypt_batch_v(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                             size_t nad, const size_t *adLens, const void *aData,
                             const void *pntxt, uint8_t *ivs, void *crtxt);
int uaes_siv_decrypt_batch_v(int keybits, const uint8_t *keys, size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                             size_t nad, const size_t *adLens, const void *aData,
                             const uint8_t *ivs, const void *crtxt, void *pntxt, uint8_t *verdicts);

/* ---- EAX' (ANSI C12.22 / IEEE Std 1703): replace AES_EAX_* of a reference built with EAXP 1 ----
 * micro_aes.c:1523-1648.  With L = Enc_K(0^128), D = dblLE(L), Q = dblLE(D) (little-endian doubling, doubleLblock) and
 * CMAC'(start, X) = CMAC with subkeys D / Q whose chaining value starts at `start`:
 *   N = CMAC'(D, nonce), N' = N with bit 7 of bytes 12 and 14 cleared, C = CTR(N', P) with the 56-bit counter,
 *   C' = CMAC'(Q, C) (0^128 for an empty C), mac = N[12..15] ^ C'[12..15], four bytes appended at crtxt + ptextLen.
 * There is no associated data: in C12.22 the cleartext header IS the nonce, of any length (0 and a NULL pointer
 * included).  Host or device pointers, in == out works, the host policy applies to these two calls.  Decrypt reads the
 * mac at crtxt + crtxtLen and checks it BEFORE it writes: on a mismatch it returns UAES_E_AUTHENTICATION and pntxt is
 * untouched (the wipe switch does not apply).  UAES_E_ARG: NULL key, bad keybits, a needed pointer that is NULL.
 * SECURITY: Minematsu, Lucks, Morita and Iwata ("Attacks and Security Proofs of EAX-Prime", FSE 2013) forge EAX' when
 * nonce and text are BOTH at most one block (16 bytes).  The standard's own messages never are; do not use the mode
 * outside it.  Such inputs are not refused, because the reference does not refuse them. */
int uaes_eaxp_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                      const void *pntxt, size_t ptextLen, void *crtxt);    /* writes ptextLen + 4 */
int uaes_eaxp_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen,
                      const void *crtxt, size_t crtxtLen, void *pntxt);    /* crtxt holds crtxtLen + 4 */
/* Batches under one key, always on the GPU, sixteen lanes per record, one launch: record m has its nonce in the slot at
 * nonces + m * nonce_bytes and its text in the slot at m * msg_bytes, its mac at macs + 4 m.  nlens / lens (either may
 * be NULL: every record fills its slot) = nmsg 32-bit lengths, nlens[m] <= nonce_bytes and lens[m] <= msg_bytes: in
 * host memory an entry above its slot is UAES_E_ARG before the device is touched; in (4-byte aligned) device memory the
 * kernel alone reads them and takes such an entry as the slot.  The bytes of an output slot beyond lens[m] are not
 * written.  Every record is bit for bit what the single call gives.  Decrypt writes verdicts[m] = 1 (authentic) / 0
 * (verdicts may be NULL), writes only authentic records (a host-memory output is copied in first; the wipe switch does
 * not apply) and returns UAES_E_AUTHENTICATION if any record is forged.  UAES_E_ARG: a slot above UINT32_MAX bytes, a
 * size product that overflows, NULL key, bad keybits, a needed pointer that is NULL.  nmsg == 0 returns 0.  key: host
 * memory; every array host or device memory at any byte offset; crtxt == pntxt works.
 * Measured on an MI355X (tools/eaxp_rate.py -> profiles/eaxp_batch_rate.md; AES-128, 2^20 device-resident records,
 * 32-byte nonces; synchronous calls, the host round trip included), encrypt / decrypt:
 *   records of 16 B     3.50 / 2.42 G records per second   (0.78 / 0.83x the time of uaes_eax_*_batch at the same shape)
 *   records of 64 B     1.87 / 1.43 G records per second   (0.90 / 0.92x; 112 / 85 GiB/s of text)
 *   records of 1024 B   0.264 / 0.216 G records per second (0.99 / 1.01x; 251 / 206 GiB/s of text) */
int uaes_eaxp_encrypt_batch(int keybits, const uint8_t *key, size_t nmsg,
                            size_t nonce_bytes, const uint32_t *nlens, const uint8_t *nonces,
                            size_t msg_bytes, const uint32_t *lens,
                            const void *pntxt, void *crtxt, uint8_t *macs);         /* macs: nmsg * 4 */
int uaes_eaxp_decrypt_batch(int keybits, const uint8_t *key, size_t nmsg,
                            size_t nonce_bytes, const uint32_t *nlens, const uint8_t *nonces,
                            size_t msg_bytes, const uint32_t *lens,
                            const void *crtxt, const uint8_t *macs, void *pntxt, uint8_t *verdicts);

/* ---- CBC / CFB / OFB: replace AES_CBC_*, AES_CFB_*, AES_OFB_* -------------
 * micro_aes.c:697-782 (CBC with CS3 ciphertext stealing, CTS 1: the last two
 * blocks are always swapped, len < 16 -> UAES_E_DATALENGTH), :799-845 (CFB),
 * :861-893 (OFB; decrypt is the same function).  iVec = 16 bytes.  The
 * decrypt directions of CBC and CFB are block-parallel kernels; the encrypt
 * directions and OFB are serial chains: one wave walks the chain, the sixteen lanes of a
 * DPP row share each block encryption (~0.42 us per AES-128 block, 36 MiB/s, latency-bound: a single
 * stream reaches 0.8x of the reference's CPU loop -- use the *_batch calls below when there
 * are many independent messages).                                                */
int uaes_cbc_encrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_cbc_decrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
/* CBC as a reference build with CTS 0 does it (micro_aes.h:56; micro_aes.c:704-733, :753-761): no stealing, no
 * minimum length; the last chunk is padded like ECB's -- padding = AES_PADDING: 0 zeros behind a partial chunk,
 * 1 PKCS#7 / 2 ISO 7816-4 always append -- so crtxt receives 16 * (ptextLen / 16 + (ptextLen % 16 || padding))
 * bytes; decryption wants whole blocks (else UAES_E_DATALENGTH), is block-parallel, and leaves the padding.    */
int uaes_cbc_encrypt_padded(int keybits, const uint8_t *key, const uint8_t *iVec, int padding,
                            const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_cbc_decrypt_blocks(int keybits, const uint8_t *key, const uint8_t *iVec,
                            const void *crtxt, size_t crtxtLen, void *pntxt);
int uaes_cfb_encrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_cfb_decrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                     const void *crtxt, size_t crtxtLen, void *pntxt);
int uaes_ofb_xcrypt(int keybits, const uint8_t *key, const uint8_t *iVec,
                    const void *in, size_t len, void *out);

/* Batches of INDEPENDENT chains, sixteen GPU lanes per message (up to 81 919 messages) or one (above) -- where
 * a GPU serves the serial modes well.  nmsg messages of msg_bytes each, stored back to back (message m at
 * m * msg_bytes).  uaes_cbc_encrypt_batch: crtxt[m] = AES_CBC_encrypt(key, ivs + 16 m, message
 * m) bit for bit, CS3 swap included; msg_bytes must be a multiple of 16.  uaes_cmac_batch:
 * macs + 16 m = AES_CMAC(key, message m), any msg_bytes.  Data pointers host or device; ivs
 * host, or 16-byte aligned device memory.                                              */
int uaes_cbc_encrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const void *pntxt, void *crtxt);
int uaes_cmac_batch(int keybits, const uint8_t *key, size_t nmsg, size_t msg_bytes,
                    const void *data, uint8_t *macs);
/* Cipher batches -- the decrypt counterpart of uaes_cbc_encrypt_batch, ordinary CBC (no swap) in both directions, and
 * CFB and OFB over many short records with an IV each (uaes_ctr_xcrypt_batch stands with CTR above).  The conventions
 * are those of the AEAD record batches (uaes_ccm_encrypt_batch): nmsg records in slots of msg_bytes back to back
 * (record m at m * msg_bytes), sixteen GPU lanes per record, four records per wave, one kernel launch
 * (csrc/uaes_cipher_batch.hip) at any number of records, always on the GPU (the host policy does not apply).  key: host
 * memory.  ivs = nmsg * 16 bytes and the texts: host or device memory at any byte offset.  out == in works in every
 * mode, the block-parallel decrypting ones included.  Every record is bit for bit what the one-message call of its mode
 * gives for it, at all three key sizes:
 *   uaes_cbc_decrypt_batch         uaes_cbc_decrypt: the inverse of uaes_cbc_encrypt_batch, CS3 swap included (the last
 *                                  two blocks of a record of two or more arrive swapped; a one-block record has none)
 *   uaes_cbc_encrypt_blocks_batch  uaes_cbc_encrypt_padded with padding 0: ordinary CBC, which interoperates
 *   uaes_cbc_decrypt_blocks_batch  uaes_cbc_decrypt_blocks
 *   uaes_cfb_encrypt_batch / uaes_cfb_decrypt_batch / uaes_ofb_xcrypt_batch
 *                                  uaes_cfb_encrypt / uaes_cfb_decrypt / uaes_ofb_xcrypt
 * The CBC forms take whole blocks only and have no lens: msg_bytes < 16 or msg_bytes % 16 -> UAES_E_ARG.  The others
 * take any msg_bytes from 0 to UINT32_MAX and lens (may be NULL: every record is msg_bytes long) = nmsg 32-bit
 * lengths with the CCM batch's meaning: record m is the first lens[m] <= msg_bytes bytes of its slot (a longer entry is
 * taken as msg_bytes, a zero length writes nothing), the bytes of an output slot beyond lens[m] are not written, and a
 * host-memory output is copied in first, so that this remainder stays the caller's; lens is host memory or 4-byte
 * aligned device memory (else UAES_E_ARG).  UAES_E_ARG before the device is touched: a size product that overflows, a
 * needed pointer that is NULL, key bits other than 128 / 192 / 256.  nmsg == 0 returns 0.  There are no verdicts and no
 * status word.  Row steps per record: one per block in the serial directions (CBC encrypt, CFB encrypt, OFB: the pace
 * of uaes_cbc_encrypt_batch's sixteen-lane form), one per TWO blocks where blocks do not wait for each other (CBC
 * decrypt, CFB decrypt, CTR).
 * Measured on an MI355X (tools/cipher_batch_rate.py -> profiles/cipher_batch_rate.md; device-resident arrays,
 * synchronous calls, the host round trip included), AES-128 and AES-256:
 *   2^10 records of 16 B     18.9 .. 19.2 and 19.8 .. 20.0 us per call, the two CBC decrypts 22.1 .. 22.2 and 21.1 .. 21.2
 *                            (2^10 one-message calls of the same mode: 12.5 .. 14.7 and 12.4 .. 14.2 us EACH)
 *   2^20 records of 16 / 64 / 1024 B, G records per second:
 *     CBC decrypt            5.72 / 4.24 / 0.564 and 5.46 / 3.72 / 0.419      over blocks 6.15 / 4.44 / 0.584 and 5.70 / 3.80 / 0.444
 *     CBC encrypt over blocks 6.30 / 4.10 / 0.480 and 5.84 / 3.45 / 0.362
 *     CFB encrypt            6.09 / 4.00 / 0.476 and 5.58 / 3.37 / 0.360      decrypt 5.98 / 4.37 / 0.577 and 5.62 / 3.81 / 0.441
 *     OFB                    6.04 / 4.01 / 0.484 and 5.60 / 3.37 / 0.366
 *     CTR                    5.87 / 4.11 / 0.503 and 5.52 / 3.59 / 0.390
 * The CTR batch takes 0.51 .. 0.58x the time of uaes_ccm_encrypt_batch at these 2^20-record shapes, 0.58 .. 0.69x at 2^16
 * records and 0.86x at 2^10 (two CCM runs of one shape differ by at most 0.8 us up to 2^16 records and by at most 0.4 %
 * at 2^20).  uaes_cbc_encrypt_blocks_batch is NOT within that spread of uaes_cbc_encrypt_batch: where both run sixteen
 * lanes per record (2^10 and 2^16 records) it takes 2.1 .. 5.6 us per call more whatever the work (16 .. 191 us per call:
 * the same chain at the same pace, and a host side that ends in a stream synchronise where uaes_cbc_encrypt_batch spins
 * on a ticket and waits once less for the caller's stream; not timed apart), and at 2^20 records uaes_cbc_encrypt_batch
 * is its one-lane-per-record arrangement, which these batches do not have, and is 2.5 .. 5.8x faster.  For 2^17 records
 * and more that want CS3, or can swap the last two blocks themselves, it remains the faster call. */
int uaes_cbc_decrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const void *crtxt, void *pntxt);
int uaes_cbc_encrypt_blocks_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                                  size_t msg_bytes, const void *pntxt, void *crtxt);
int uaes_cbc_decrypt_blocks_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                                  size_t msg_bytes, const void *crtxt, void *pntxt);
int uaes_cfb_encrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *pntxt, void *crtxt);
int uaes_cfb_decrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                           size_t msg_bytes, const uint32_t *lens, const void *crtxt, void *pntxt);
int uaes_ofb_xcrypt_batch(int keybits, const uint8_t *key, const uint8_t *ivs, size_t nmsg,
                          size_t msg_bytes, const uint32_t *lens, const void *in, void *out);

/* ---- KW: replaces AES_KEY_wrap / AES_KEY_unwrap (RFC 3394, SP 800-38F KW) ------
 * micro_aes.c:1829-1894.  kek = the key-encryption key (host memory).  wrap writes secretLen + 8 bytes: A || R_1..R_n
 * after 6 n chained block encryptions over the n = secretLen / 8 semiblocks; secretLen % 8 != 0 or n < 2 ->
 * UAES_E_DATALENGTH, wrapped untouched.  unwrap runs the chain backwards with the inverse cipher and writes
 * wrapLen - 8 bytes; wrapLen % 8 != 0 or wrapLen / 8 < 3 -> UAES_E_DATALENGTH, secret untouched; if A does not come
 * out as A6 x 8 it returns UAES_E_AUTHENTICATION and, like the reference, leaves what the chain made in secret (zeros
 * under uaes_set_wipe_on_auth_failure(1)).  Data pointers host or device memory at any byte offset; the buffers are
 * disjoint, or the secret sits 8 bytes into the wrapped buffer (secret == (uint8_t *)wrapped + 8, the reference's own
 * in-place form); any other overlap is undefined.  The host policy applies (one serial chain: `chains`).
 * One wave walks the chain, sixteen lanes per block: a secret of up to 4 KiB keeps its semiblocks in LDS, a longer one
 * is worked on in place in device memory with its loads issued a chunk of steps ahead.  Measured (tools/kw_rate.py,
 * profiles/kw_rate.md, AES-128): 23 .. 25 us for one 32-byte secret, 72 us to wrap and 80 us to unwrap 65 536 of them in
 * one batch, 0.46 / 0.48 us per chain step.
 * Batches: nkeys records of one length under one kek, back to back -- secret m at m * secret_bytes, wrapped record m at
 * m * (secret_bytes + 8) -- sixteen GPU lanes per record, always on the GPU; a record holds at most 256 bytes of secret
 * (UAES_E_ARG beyond; a 2048-bit secret fits), lengths as above (UAES_E_DATALENGTH).  unwrap_batch sets verdicts[m] =
 * 1 (authentic) / 0 for every record, returns UAES_E_AUTHENTICATION if any record failed and follows the wipe switch
 * per record, as uaes_siv_decrypt_batch does.  Arrays host or device memory; the batches have no in-place form.      */
int uaes_kw_wrap(int keybits, const uint8_t *kek, const void *secret, size_t secretLen, void *wrapped);
int uaes_kw_unwrap(int keybits, const uint8_t *kek, const void *wrapped, size_t wrapLen, void *secret);
int uaes_kw_wrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t secret_bytes,
                       const void *secrets, void *wrapped);
int uaes_kw_unwrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t wrapped_bytes,
                         const void *wrapped, void *secrets, uint8_t *verdicts);

/* ---- KWP: key wrap with padding (RFC 5649, SP 800-38F KWP; PKCS#11 CKM_AES_KEY_WRAP_KWP) ------
 * The reference has none: this goes past it, for the secrets KW cannot take -- any length from 1 to 2^32 - 1 bytes (a
 * PKCS#8 blob, a 66-byte P-521 scalar, a PIN).  The secret is zero-filled to n = ceil(secretLen / 8) semiblocks and A
 * starts as A6 59 59 A6 || secretLen (32 bits, big-endian: the MLI).  n >= 2 runs KW's chain of 6 n blocks with that A;
 * n = 1 is one block of the cipher over A || the filled semiblock, no chain.
 *   wrap      writes uaes_kwp_wrapped_len(secretLen) = 8 n + 8 bytes; secretLen 0 or above 2^32 - 1 -> UAES_E_DATALENGTH,
 *             wrapped untouched.
 *   unwrap    wrapLen % 8 != 0, wrapLen < 16 or wrapLen - 8 > 2^32 (more than an MLI can describe) -> UAES_E_DATALENGTH,
 *             secret untouched.  `secret` holds wrapLen - 8 bytes and ALL of them are written: the secret and, behind
 *             *secretLen, its zero fill.  A 16-byte input is one inverse block, a longer one the inverse chain.  Then
 *             three conditions must hold: MSB32(A) = A65959A6; 8 (n - 1) < MLI <= 8 n; the 8 n - MLI bytes behind the
 *             secret are zero.  All three are evaluated and combined without an early exit, and the outcome is ONE
 *             verdict that does not say which failed: UAES_E_AUTHENTICATION with *secretLen = 0 and, as uaes_kw_unwrap,
 *             what the chain made left in secret (zeros under uaes_set_wipe_on_auth_failure(1)).  On the GPU the
 *             verdict is computed by the kernel.
 * kek: host memory.  Data pointers host or device memory at any byte offset; the buffers are disjoint, or the in-place
 * form secret == (uint8_t *)wrapped + 8 (a wrap then writes the zero fill into `wrapped`; a wrap of at most 8 bytes reads
 * its input before it writes); any other overlap is undefined.  No byte behind the secretLen bytes of `secret` is read.
 * The host policy applies as for KW (`chains`).  Checks in KW's order: the key, the lengths, NULL pointers (secretLen
 * included), all before the device is touched.  Arrangements as KW's, by the padded length (uaes_debug_plan_kwp).
 * Batches: always on the GPU, one launch, sixteen lanes per record, a length per record.
 *   wrap_batch    secret m at m * secret_bytes, secret_bytes = 1 .. 256 and need not be a multiple of 8 (UAES_E_ARG
 *                 otherwise); wrapped record m at m * uaes_kwp_wrapped_len(secret_bytes).  lens == NULL: every secret is
 *                 secret_bytes long.  Else lens[m] = 1 .. secret_bytes (host memory, or 4-byte-aligned device memory),
 *                 record m writes uaes_kwp_wrapped_len(lens[m]) bytes and the rest of its slot is not written (a host
 *                 output is copied in first, as the CCM batch does).  An entry of 0 or above secret_bytes writes nothing
 *                 for that record; every other record is finished and the call returns UAES_E_DATALENGTH.
 *   unwrap_batch  wrapped_bytes = a multiple of 8 in 16 .. 264 (UAES_E_ARG otherwise); wrapped record m at
 *                 m * wrapped_bytes, secret m at m * (wrapped_bytes - 8).  wlens == NULL: every record is wrapped_bytes
 *                 long; else an entry that is no multiple of 8, below 16 or above wrapped_bytes makes that record fail
 *                 unwritten.  lens_out[m] = the MLI of an authentic record, 0 otherwise; verdicts[m] = 1 / 0;
 *                 UAES_E_AUTHENTICATION if any record failed.  A record writes its wlens[m] - 8 bytes (zeros for a
 *                 failed one under the wipe switch).
 * nkeys == 0 returns 0.  Arrays host or device memory; no in-place form; no byte outside the arrays is read or written
 * (a secret whose last semiblock is short is loaded bytewise, never rounded up).  Measured beside KW (profiles/kw_rate.md):
 * 13 .. 15 us for one secret of 7 bytes, 19 .. 25 us at 20 and 32 bytes; 2^20 records of 32 bytes wrap in 0.91 ms and
 * unwrap in 0.88 ms, 1.07 and 1.02 times the KW batch of that shape. */
#ifndef UAES_STATIC_INLINE
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 199901L)
#define UAES_STATIC_INLINE static inline
#else
#define UAES_STATIC_INLINE static __inline
#endif
#endif
/* 8 * ceil(len / 8) + 8; 0 for len == 0 or len > 2^32 - 1 */
UAES_STATIC_INLINE size_t uaes_kwp_wrapped_len(size_t secretLen)
{
    const uint64_t m = secretLen;
    return m == 0 || m > 0xFFFFFFFFu ? 0 : (size_t)((m + 7) / 8 * 8 + 8);
}
int uaes_kwp_wrap(int keybits, const uint8_t *kek, const void *secret, size_t secretLen, void *wrapped);
int uaes_kwp_unwrap(int keybits, const uint8_t *kek, const void *wrapped, size_t wrapLen, void *secret, size_t *secretLen);
int uaes_kwp_wrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t secret_bytes,
                        const uint32_t *lens, const void *secrets, void *wrapped);
int uaes_kwp_unwrap_batch(int keybits, const uint8_t *kek, size_t nkeys, size_t wrapped_bytes,
                          const uint32_t *wlens, const void *wrapped, void *secrets,
                          uint32_t *lens_out, uint8_t *verdicts);

/* ---- FF1: replaces AES_FPE_encrypt / AES_FPE_decrypt (SP 800-38G, FF_X 1) ------
 * micro_aes.c:2091-2147, :2267-2347.  Format-preserving encryption of len numerals, ONE BYTE PER NUMERAL.  radix =
 * 2..256; alphabet = radix distinct bytes (input bytes are looked up in it, output digits mapped through it), or NULL:
 * the bytes are the digit values 0..radix-1 themselves.  key, alphabet: host memory; tweak, in, out: host or device
 * memory at any byte offset; out == in works (every numeral is looked up before anything is written).  No NUL is
 * appended at this level.
 *   lengths   len at least the smallest n with radix^n >= 1 000 000 (6 for decimal; the reference's MINLEN for every
 *             radix), at most UAES_FF1_MAX = 4096, tweakLen below 2^32; otherwise UAES_E_DATALENGTH, out untouched.
 *             The cap departs from the reference, which takes any length: the radix conversions are quadratic in the
 *             length (the reference needs 43 s for 100 000 digits on one host core).
 *   errors    radix outside 2..256 or a byte twice in the alphabet: UAES_E_ARG.  A byte of `in` that is no numeral:
 *             UAES_E_ENCRYPTION from encrypt, UAES_E_DECRYPTION from decrypt, out untouched (the reference's 'C',
 *             micro_aes.c:2294-2300).
 * b = ceil(bits(radix^v - 1) / 8) is computed with exact integers, as SP 800-38G states it.  The reference's
 * floating-point form agrees for radix 10 at every length this call takes; where v log2(radix) is a multiple of 8 at 136
 * bits or more (radix 2 from v = 128, radix 64 from v = 24, radix 256 from v = 16; v = len - len / 2) it is one too
 * large, and the engine follows the specification there.
 * Ten Feistel rounds, each a CBC-MAC of one to a few blocks and two radix conversions: a chain like key wrap, so the
 * host policy applies (`chains`), and the GPU's form is the batch: nrec records of len numerals back to back under
 * one key, sixteen GPU lanes per record, always on the GPU.  tweak_stride 0: one tweak for all records; otherwise
 * record m's tweak is at tweaks + m * tweak_stride.  A record holds at most UAES_FF1_BATCH_MAX = 128 numerals
 * (UAES_E_DATALENGTH beyond).  A record with a byte that is no numeral is left unwritten and gets verdicts[m] = 0,
 * the others 1 (verdicts may be NULL, host or device memory); the call completes every good record and then returns
 * the encryption / decryption error if any record was bad.  nrec == 0 returns 0.  A single call of up to
 * UAES_FF1_BATCH_MAX numerals runs as a batch of one, a longer one on a wave of its own.
 * Rates (profiles/ff1_rate.md: tools/ff1_rate.py on an MI355X, AES-128, 16-digit decimal records, device-resident):
 * 2^20 records 5.02 ms = 2.09e8 records/s, 2^16 records 0.35 ms, 2^10 records 0.10 ms, shared or per-record tweaks,
 * either direction; one 16-digit call 108 us; one 4096-digit call 20 ms.  One host core: the reference 2.58e5
 * records/s, the engine's host path 4.46e5.                                                                       */
int uaes_ff1_encrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, size_t tweakLen, const void *in, size_t len, void *out);
int uaes_ff1_decrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak, size_t tweakLen, const void *in, size_t len, void *out);
int uaes_ff1_encrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweakLen, size_t tweak_stride,
                           size_t nrec, size_t len, const void *in, void *out, uint8_t *verdicts);
int uaes_ff1_decrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweakLen, size_t tweak_stride,
                           size_t nrec, size_t len, const void *in, void *out, uint8_t *verdicts);

/* ---- FF3-1: replaces AES_FPE_encrypt / AES_FPE_decrypt built with FF_X 3 (SP 800-38G revision 1) ------
 * micro_aes.c:2150-2248, :2267-2347.  Format-preserving encryption of len numerals, ONE BYTE PER NUMERAL, under a tweak
 * of exactly SEVEN bytes (the withdrawn 64-bit-tweak FF3 is not served).  radix, alphabet, key and the memory rules are
 * FF1's: radix = 2..256; alphabet = radix distinct bytes or NULL (the bytes are the digit values); key, alphabet: host
 * memory; tweak, in, out: host or device memory at any byte offset; out == in works.  No NUL is appended at this level.
 *   lengths   len at least the smallest n with radix^n >= 1 000 000 (FF1's minimum), at most uaes_ff3_maxlen(radix) =
 *             2 floor(log_radix 2^96), computed with exact integers (192 at radix 2, 56 decimal, 40 at radix 26, 36 at
 *             36, 32 at 62 and 64, 24 at 256; 0 for a radix outside 2..256): the reference's floating-point MAXLEN
 *             (micro_fpe.h:145) is the same number.  Otherwise UAES_E_DATALENGTH, out untouched.
 *   errors    radix outside 2..256 or a byte twice in the alphabet: UAES_E_ARG.  A byte of `in` that is no numeral:
 *             UAES_E_ENCRYPTION from encrypt, UAES_E_DECRYPTION from decrypt, out untouched.
 * Eight Feistel rounds of one AES block each under the byte-reversed key; every number stays below 2^96 on the way into
 * the cipher and 2^128 on the way out.  One call is a chain, so the host policy applies (`chains`); the GPU's form is
 * the batch: nrec records of len numerals back to back under one key, sixteen GPU lanes per record, always on the GPU.
 * tweak_stride 0: one tweak for all records; otherwise record m's tweak is the seven bytes at tweaks + m * tweak_stride.
 * A record with a byte that is no numeral is left unwritten and gets verdicts[m] = 0, the others 1 (verdicts may be
 * NULL, host or device memory); the call completes every good record and then returns the encryption / decryption
 * error if any record was bad.  nrec == 0 returns 0.  A single call that goes to the GPU runs as a batch of one.
 * Rates (profiles/ff3_rate.md: tools/ff3_rate.py on an MI355X, AES-128, 16-digit decimal records, device-resident):
 * 2^20 records 2.64 ms = 3.97e8 records/s, 2^16 records 0.19 ms, 2^10 records 0.066 ms, shared or per-record tweaks,
 * either direction -- the FF1 batch of the same shape in the same run: 5.04 ms, 0.35 ms, 0.10 ms.  One 16-digit call
 * 94 us from host memory, 75 us from device memory.  The engine's host path on one core: 5.47e5 records/s. */
size_t uaes_ff3_maxlen(unsigned radix);
int uaes_ff3_encrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak /* 7 bytes */, const void *in, size_t len, void *out);
int uaes_ff3_decrypt(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                     const uint8_t *tweak /* 7 bytes */, const void *in, size_t len, void *out);
int uaes_ff3_encrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweak_stride, size_t nrec, size_t len,
                           const void *in, void *out, uint8_t *verdicts);
int uaes_ff3_decrypt_batch(int keybits, const uint8_t *key, unsigned radix, const uint8_t *alphabet,
                           const uint8_t *tweaks, size_t tweak_stride, size_t nrec, size_t len,
                           const void *in, void *out, uint8_t *verdicts);

/* Poly1305-AES (micro_aes.c:1955-1997): keys = k (keybits / 8 bytes) || r (16 bytes), mac = (h + AES_k(nonce)) mod
 * 2^128 with h the Poly1305 polynomial in the clamped r.  Block-parallel on the VALU (uaes_poly1305.hip): one
 * workgroup for a short message, chunk workgroups + a fold kernel beyond; AES_k(nonce) runs on the device too.
 * data may be NULL when dataSize is 0 (mac = AES_k(nonce)).  uaes_poly1305 takes host or device data (device data
 * produced on another stream: uaes_set_producer_stream) and follows the host policy; uaes_poly1305_dev enqueues on
 * `stream` (a hipStream_t, NULL = default) and returns: d_data, d_mac device memory, keys and nonce host memory, the
 * per-stream scratch goes back with uaes_stream_release, and the call can be captured into a graph.
 * uaes_poly1305_batch: one key pair, nmsg nonces (16 bytes each) and nmsg messages of msg_bytes each back to back,
 * one wave per message; nonces, data and macs host or device memory, macs = nmsg * 16 bytes. */
int uaes_poly1305(int keybits, const uint8_t *keys, const uint8_t nonce[16],
                  const void *data, size_t dataSize, uint8_t mac[16]);
int uaes_poly1305_dev(int keybits, const uint8_t *keys, const uint8_t nonce[16],
                      const void *d_data, size_t len, void *d_mac, void *stream);
int uaes_poly1305_batch(int keybits, const uint8_t *keys, const uint8_t *nonces, size_t nmsg,
                        size_t msg_bytes, const void *data, uint8_t *macs);

/* ---- GCM-SIV: replaces GCM_SIV_encrypt / GCM_SIV_decrypt ---------------------
 * RFC 8452; micro_aes.c:1418-1516.  12-byte nonce, 16-byte tag appended.  Per-
 * nonce keys are derived with AES (GCM_SIVsetup), the tag is AES over POLYVAL
 * (run through the GHASH kernels with byte-reversed blocks), the text is CTR
 * with a 32-bit little-endian counter seeded by the tag.  decrypt returns
 * UAES_E_AUTHENTICATION on a mismatch and, like the reference, leaves the
 * decrypted text in pntxt.                                                   */
int uaes_gcmsiv_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_gcmsiv_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batches under one MASTER key -- GCM-SIV exists for many short messages under one long-lived key, with nonces that may
 * repeat, and one call per message costs 22 us at 16 bytes and about 30 at 4 KiB.  The conventions are those of the CCM batches,
 * word for word: nmsg records in slots of msg_bytes back to back (record m at m * msg_bytes), sixteen GPU lanes per
 * record, one kernel launch, always on the GPU (the host policy does not apply).  nonces = nmsg * 12 bytes, aData =
 * nmsg * aad_bytes (aad_bytes 0: no AAD, the pointer may be NULL), tags = nmsg * 16 bytes, PACKED, not appended to the
 * texts.  lens (may be NULL: every record is msg_bytes long) = nmsg 32-bit lengths: record m is the first lens[m] <=
 * msg_bytes bytes of its slot (a longer entry is taken as msg_bytes) and the bytes of an output slot beyond lens[m] are
 * not written.  Every record is bit for bit what uaes_gcmsiv_encrypt / uaes_gcmsiv_decrypt give for it, at all three
 * key sizes (192 bits: the reference's five derivation blocks, which RFC 8452 does not define).  The GCM record batch
 * cannot serve here: both working keys belong to the nonce, so every record derives its keys, expands its own key
 * schedule and hashes under its own POLYVAL key, all in the kernel (csrc/uaes_gcmsiv_batch.hip).  Decrypt follows the
 * reference per record: the keystream comes from the received tag and the text is written before the tag is known,
 * verdicts[m] = 1 (authentic) / 0, the call returns 0 when every record is authentic, else UAES_E_AUTHENTICATION, and a
 * forged record's output is left as decrypted, or zeros under uaes_set_wipe_on_auth_failure(1).  UAES_E_ARG (before
 * the device is touched): key bits other than 128 / 192 / 256, msg_bytes or aad_bytes > 65535 (UAES_GCMSIV_BATCH_MAX,
 * csrc/uaes_plan.h: a record is a serial POLYVAL chain on sixteen lanes, and beyond the cap the one-message
 * arrangements, siv.chunks from 32 736 B, are the right tool), a size product that overflows, a needed pointer that is
 * NULL, verdicts included.  nmsg == 0 returns 0 after the length and key checks.  key: host memory; every array host
 * or device memory at any byte offset (lens: 4-byte aligned device memory, or host memory); crtxt == pntxt works.
 * With lens, a host-memory output is copied in first, so that the unwritten remainder of a slot stays the caller's.
 * Measured on an MI355X (tools/gcmsiv_rate.py -> profiles/gcmsiv_batch_rate.md; device-resident, 12 bytes of AAD;
 * synchronous calls, the host round trip included), AES-128 and AES-256, encrypt / decrypt:
 *   2^10 records of 16 B     23.9 / 35.3 and 25.2 / 36.2 us per call  (2^10 uaes_gcmsiv_encrypt calls: 22.5 / 25.2 us EACH)
 *   2^20 records of 16 B     1.78 / 1.99 and 1.44 / 1.57 G records per second
 *   2^20 records of 64 B     1.32 / 1.44 and 1.09 / 1.16 G records per second
 *   2^20 records of 1024 B   0.215 / 0.206 and 0.189 / 0.175 G records per second  (205 / 196 and 180 / 167 GiB/s of text)
 * 1.15 .. 1.97x the time of uaes_ccm_encrypt_batch at the same shape (a CCM record has no keys to make), and 0.27 ..
 * 0.41x that of uaes_gcm_key_encrypt_records / _decrypt_records at 16 and 64 bytes, 0.99 .. 1.11x at 1024. */
int uaes_gcmsiv_encrypt_batch(int keybits, const uint8_t *key,
                              size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                              const uint8_t *nonces, const void *aData, size_t aad_bytes,
                              const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_gcmsiv_decrypt_batch(int keybits, const uint8_t *key,
                              size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                              const uint8_t *nonces, const void *aData, size_t aad_bytes,
                              const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);

/* ---- OCB: replaces AES_OCB_encrypt / AES_OCB_decrypt --------------------------
 * RFC 7253; micro_aes.c:1693-1811.  12-byte nonce, 16-byte tag appended.  Block-
 * parallel in both directions: Offset_i is computed per lane from the Gray code of
 * i instead of being chained.  decrypt returns UAES_E_AUTHENTICATION on a mismatch
 * and, like the reference, leaves the decrypted text in pntxt.                  */
int uaes_ocb_encrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_ocb_decrypt(int keybits, const uint8_t *key, const uint8_t *nonce,
                     const void *aData, size_t aDataLen,
                     const void *crtxt, size_t crtxtLen, void *pntxt);

/* The same with the reference's compile-time OCB_NONCE_LEN (1..15) and OCB_TAG_LEN (1..16), micro_aes.h:115-116 */
int uaes_ocb_encrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_ocb_decrypt_ex(int keybits, const uint8_t *key, const uint8_t *nonce, size_t nonceLen, size_t tagLen,
                        const void *aData, size_t aDataLen,
                        const void *crtxt, size_t crtxtLen, void *pntxt);
/* Batches under one key -- OCB's usual workload is many short packets, and one call per packet costs 21 us whatever
 * its size.  The conventions of the CCM batches with OCB's lengths: nmsg records in slots of msg_bytes back to back
 * (record m at m * msg_bytes), sixteen GPU lanes per record, one kernel launch, always on the GPU (the host policy does
 * not apply).  nonces = nmsg * nonceLen bytes (nonceLen 1..15), aData = nmsg * aad_bytes (aad_bytes 0: no AAD, the
 * pointer may be NULL), tags = nmsg * tagLen bytes (tagLen 1..16), PACKED, not appended to the texts.  lens (may be
 * NULL: every record is msg_bytes long) = nmsg 32-bit lengths: record m is the first lens[m] <= msg_bytes bytes of its
 * slot (a longer entry is taken as msg_bytes) and the bytes of an output slot beyond lens[m] are not written.  Every
 * record is bit for bit what uaes_ocb_encrypt_ex / uaes_ocb_decrypt_ex give for it, at all three key sizes.  Decrypt
 * follows the reference per record (micro_aes.c:1803-1810): the text is written before the tag is known, verdicts[m] =
 * 1 (authentic) / 0, the call returns 0 when every record is authentic, else UAES_E_AUTHENTICATION, and a forged
 * record's output is left as decrypted, or zeros under uaes_set_wipe_on_auth_failure(1).  UAES_E_ARG (before the device
 * is touched): key bits other than 128 / 192 / 256, nonceLen outside 1..15, tagLen outside 1..16, msg_bytes or
 * aad_bytes > 65535 (UAES_OCB_BATCH_MAX, csrc/uaes_plan.h; beyond it the one-message calls are the right tool), a size
 * product that overflows, a needed pointer that is NULL (verdicts included).  nmsg == 0 returns 0 after the length and
 * key checks.  key: host memory; every array host or device memory at any byte offset (lens: 4-byte aligned device
 * memory, or host memory); crtxt == pntxt works.  With lens, a host-memory output is copied in first, so that the
 * unwritten remainder of a slot stays the caller's.
 * Measured on an MI355X (tools/ocb_rate.py -> profiles/ocb_batch_rate.md; AES-128, device-resident, 12-byte nonces,
 * 16-byte tags, 12 bytes of AAD; synchronous calls, the host round trip included), encrypt / decrypt:
 *   2^10 records of 16 B     22.7 / 37.8 us per call        (2^10 uaes_ocb_encrypt_ex calls: 20.0 us EACH)
 *   2^20 records of 16 B     3.33 / 3.26 G records per second
 *   2^20 records of 64 B     2.66 / 2.71 G records per second  (159 / 161 GiB/s of text)
 *   2^20 records of 1024 B   0.507 / 0.479 G records per second  (484 / 457 GiB/s of text)
 * Against uaes_ccm_*_batch at the same shape in the same run: 0.97 .. 1.05x its time at 16-byte records, 0.78 .. 1.03x
 * at 64 bytes, 0.58 .. 0.85x at 1024 bytes, where an OCB record has half the row steps (2^16 records and more: 0.58 ..
 * 0.65x).  A decrypting call costs 13 .. 20 us more than the encrypting one at up to 2^16 records, as CCM's does (it
 * clears and fetches the word that says whether any record failed).                                              */
int uaes_ocb_encrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *pntxt, void *crtxt, uint8_t *tags);
int uaes_ocb_decrypt_batch(int keybits, const uint8_t *key, size_t nonceLen, size_t tagLen,
                           size_t nmsg, size_t msg_bytes, const uint32_t *lens,
                           const uint8_t *nonces, const void *aData, size_t aad_bytes,
                           const void *crtxt, const uint8_t *tags, void *pntxt, uint8_t *verdicts);

/* ---- streamed GCM: one message fed in pieces -----------------
 * For texts larger than device (or host) memory: state = key schedule, block
 * position of the counter and the running GHASH value, which stays on the GPU
 * (Y <- Y * H^m ^ GHASH(piece), m = blocks in the piece).  The result is
 * bit-identical to one AES_GCM_encrypt / AES_GCM_decrypt call over the whole
 * text (micro_aes.c:1164-1212).  Every piece but the last must be a multiple of
 * 16 bytes; buffers may be host or device memory.  A decrypting stream releases
 * text before the tag is checked -- unlike AES_GCM_decrypt (N7) -- so the caller
 * must discard it if finish() returns UAES_E_AUTHENTICATION.  finish() and abort()
 * free the stream.                                                           */
typedef struct uaes_gcm_stream uaes_gcm_stream;
int  uaes_gcm_stream_begin(uaes_gcm_stream **s, int keybits, const uint8_t *key, const uint8_t *nonce,
                           const void *aData, size_t aDataLen, int decrypt);
int  uaes_gcm_stream_update(uaes_gcm_stream *s, const void *in, size_t len, void *out);
/* encrypting stream: tag <- the 16-byte tag; decrypting stream: tag = the received tag */
int  uaes_gcm_stream_finish(uaes_gcm_stream *s, uint8_t tag[16]);
void uaes_gcm_stream_abort(uaes_gcm_stream *s);

/* A synchronous call that is handed DEVICE memory first waits for the work the caller may have in
 * flight on the default stream (hipStreamSynchronize(NULL)), then runs on the calling thread's own
 * stream and returns when it is done -- the ordering a default-stream launch used to give.        */

/* ... or, when the caller's device data is produced on a stream of its own (one made with hipStreamNonBlocking does
 * not synchronise with the default stream), for the stream named here.  Thread-local; NULL = the default stream.  */
int uaes_set_producer_stream(void *stream);

/* ---- asynchronous, device-resident variants -----------------------------
 * All data pointers are device pointers, 16-byte aligned; `stream` is a
 * hipStream_t (NULL = default stream).  The call only enqueues work.  Scratch
 * (GHASH tables, XTS chunk tweaks, OCB offsets) is kept per stream, so calls on
 * different streams may overlap; up to 8 streams per device without a drain.
 * Calls that target the SAME stream must not be issued from two threads at once
 * (a call enqueues several dependent kernels).                                  */
int uaes_ecb_dev(int keybits, const uint8_t *key, int decrypt,
                 const void *d_in, size_t len, void *d_out, void *stream);
int uaes_ctr_xcrypt_at_dev(int keybits, const uint8_t *key, const uint8_t ctr0[16],
                           uint64_t block_offset,
                           const void *d_in, size_t len, void *d_out, void *stream);
int uaes_xts_sectors_dev(int keybits, const uint8_t *keys, uint64_t first_sector,
                         size_t sector_bytes, size_t nsectors,
                         const void *d_in, void *d_out, int encrypt, void *stream);
int uaes_gcm_encrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out, void *stream);
/* d_status (device int) receives 0 or UAES_E_AUTHENTICATION                 */
int uaes_gcm_decrypt_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, size_t aad_len,
                         const void *d_in, size_t len, void *d_out,
                         int *d_status, void *stream);

/* decrypt != 0: d_in = CT || tag, d_status (device int) receives 0 or 0x1A    */
int uaes_ocb_dev(int keybits, const uint8_t *key, const uint8_t *nonce, int decrypt,
                 const void *d_aad, size_t aad_len,
                 const void *d_in, size_t len, void *d_out, int *d_status, void *stream);

/* ---- GCM key context -----------------------------------------------------------
 * The reference redoes GCMsetup in every call (micro_aes.c:1140-1152) and so do the one-shot
 * functions above: key schedule, H = Enc(0), the GHASH multiplication tables of H (a 20 us
 * kernel).  A caller that sends many messages under one key builds them ONCE:
 *   uaes_gcm_key_new    key schedule + every key-dependent table, on the current device
 *   uaes_gcm_key_encrypt / _decrypt        = uaes_gcm_encrypt / _decrypt, bit for bit (12-byte
 *                                            nonce; host or device pointers; synchronous)
 *   uaes_gcm_key_encrypt_dev / _decrypt_dev  enqueue on a stream
 * Per message only Enc(J0) is computed (a one-wave kernel).  The context holds per-message
 * state too: ONE call at a time per context (calls on one stream are ordered; use one context
 * per stream for concurrency).  uaes_gcm_key_free wipes the tables.                          */
typedef struct uaes_gcm_key uaes_gcm_key;
int  uaes_gcm_key_new(uaes_gcm_key **out, int keybits, const uint8_t *key);
void uaes_gcm_key_free(uaes_gcm_key *k);
int  uaes_gcm_key_encrypt(uaes_gcm_key *k, const uint8_t *nonce, const void *aData, size_t aDataLen,
                          const void *pntxt, size_t ptextLen, void *crtxt);
int  uaes_gcm_key_decrypt(uaes_gcm_key *k, const uint8_t *nonce, const void *aData, size_t aDataLen,
                          const void *crtxt, size_t crtxtLen, void *pntxt);
int  uaes_gcm_key_encrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                              const void *d_in, size_t len, void *d_out, void *stream);
int  uaes_gcm_key_decrypt_dev(uaes_gcm_key *k, const uint8_t *nonce, const void *d_aad, size_t aad_len,
                              const void *d_in, size_t len, void *d_out, int *d_status, void *stream);

/* Many short messages under one key context in ONE launch (the GCM counterpart of uaes_xts_encrypt_sectors;
 * the reference has a message per call, AES_GCM_encrypt micro_aes.c:1164-1179, and a call costs ~12 us on a GPU
 * whatever its size).  Record r: rec_len bytes at in + r * in_stride, 12-byte nonce nonces + 12 r, AAD
 * aad + r * aad_stride (aad_stride 0: the same aad_len bytes for every record).
 *   encrypt: out + r * out_stride receives ciphertext || 16-byte tag   (out_stride >= rec_len + 16)
 *   decrypt: the record is ciphertext || tag (in_stride >= rec_len + 16), out + r * out_stride receives the
 *            plaintext of every record whose tag matches; the others are left untouched (N7), verdicts[r]
 *            (may be NULL) = 0 / 0x1A, and the call returns UAES_E_AUTHENTICATION if any record failed.
 * Byte for byte what uaes_gcm_key_encrypt / _decrypt give record by record.  Strides are multiples of 16,
 * in / out 16-byte aligned (device flavour), rec_len <= uaes_gcm_record_max(aad_len) (32 KiB - 48 without AAD).
 * The *_dev flavour takes device pointers for everything, enqueues on `stream`, and reports through
 * d_verdicts / *d_status (zeroed by the call, 0x1A ORed in); any number of record calls may share one context.
 * Empty records (rec_len 0: a batch of GMACs) take up to 16 * 2045 bytes of AAD; uaes_gcm_record_max is 0 from there
 * on, and more AAD is UAES_E_ARG like a record that is too long.  nrec == 0 returns 0 and looks at no pointer.      */
size_t uaes_gcm_record_max(size_t aad_len);
int  uaes_gcm_key_encrypt_records(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                  const void *aad, size_t aad_len, size_t aad_stride,
                                  const void *in, size_t rec_len, size_t in_stride, void *out, size_t out_stride);
int  uaes_gcm_key_decrypt_records(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                  const void *aad, size_t aad_len, size_t aad_stride,
                                  const void *in, size_t rec_len, size_t in_stride, void *out, size_t out_stride,
                                  uint8_t *verdicts);
int  uaes_gcm_key_encrypt_records_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                      const void *d_aad, size_t aad_len, size_t aad_stride,
                                      const void *d_in, size_t rec_len, size_t in_stride,
                                      void *d_out, size_t out_stride, void *stream);
int  uaes_gcm_key_decrypt_records_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                      const void *d_aad, size_t aad_len, size_t aad_stride,
                                      const void *d_in, size_t rec_len, size_t in_stride,
                                      void *d_out, size_t out_stride, uint8_t *d_verdicts, int *d_status, void *stream);
/* ... with records of DIFFERENT lengths in slots of one size (packet buffers): record r is lens[r] <= max_len bytes at
 * the start of slot r (uint32 lengths; the device flavour clamps a longer one to max_len), its tag follows its own text;
 * strides >= max_len (+ 16 where the tag is).  The other bytes of a slot's first max_len + 16 output bytes are
 * unspecified afterwards.  The arrangement of the launch is the one the longest record needs.                   */
int  uaes_gcm_key_encrypt_records_v(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                    const void *aad, size_t aad_len, size_t aad_stride,
                                    const void *in, const uint32_t *lens, size_t max_len, size_t in_stride,
                                    void *out, size_t out_stride);
int  uaes_gcm_key_decrypt_records_v(uaes_gcm_key *k, size_t nrec, const uint8_t *nonces,
                                    const void *aad, size_t aad_len, size_t aad_stride,
                                    const void *in, const uint32_t *lens, size_t max_len, size_t in_stride,
                                    void *out, size_t out_stride, uint8_t *verdicts);
int  uaes_gcm_key_encrypt_records_v_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                        const void *d_aad, size_t aad_len, size_t aad_stride,
                                        const void *d_in, const uint32_t *d_lens, size_t max_len, size_t in_stride,
                                        void *d_out, size_t out_stride, void *stream);
int  uaes_gcm_key_decrypt_records_v_dev(uaes_gcm_key *k, size_t nrec, const uint8_t *d_nonces,
                                        const void *d_aad, size_t aad_len, size_t aad_stride,
                                        const void *d_in, const uint32_t *d_lens, size_t max_len, size_t in_stride,
                                        void *d_out, size_t out_stride, uint8_t *d_verdicts, int *d_status, void *stream);

/* (The uaes_mgpu_* calls below start one worker thread per device ordinal the first time it is named; the workers live
 * until the process ends -- they hold nothing but their lane -- so a process that has made such a call must not
 * dlclose() the library.)                                                                                          */
/* ---- one process, several GPUs -------------------------------------------------
 * The text is cut into aligned slices, one per device; one host thread per device
 * runs the single-device call on its slice with the counter / sector offset
 * advanced (the 56-bit add of incBlock, micro_aes.c:421-427; the sectid convention
 * of XTS_cipher, :1017-1021), so the result is the single-device result.  devices
 * = ndev HIP device ordinals, or NULL for 0..ndev-1.  With host buffers every
 * slice travels over its own device's PCIe link.  Pointers may be host memory
 * or memory any of the devices can reach.                                      */
int uaes_mgpu_ctr_xcrypt_at(int ndev, const int *devices, int keybits, const uint8_t *key,
                            const uint8_t ctr0[16], uint64_t block_offset,
                            const void *in, size_t len, void *out);
int uaes_mgpu_xts_sectors(int ndev, const int *devices, int keybits, const uint8_t *keys,
                          uint64_t first_sector, size_t sector_bytes, size_t nsectors,
                          const void *in, void *out, int encrypt);

/* ECB over several GPUs (AES_ECB_encrypt / AES_ECB_decrypt, micro_aes.c:636-680: any partition of the blocks).  The
 * whole blocks are dealt out evenly; the last device also takes the ragged tail and the padding (padding = the
 * reference's AES_PADDING as in uaes_ecb_encrypt_padded), so the bytes written, and decryption's UAES_E_DECRYPTION
 * for a length that is no multiple of 16, are those of the one-device call.                                     */
int uaes_mgpu_ecb_encrypt(int ndev, const int *devices, int keybits, const uint8_t *key, int padding,
                          const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_mgpu_ecb_decrypt(int ndev, const int *devices, int keybits, const uint8_t *key,
                          const void *crtxt, size_t crtxtLen, void *pntxt);

/* GCM over several GPUs (AES_GCM_encrypt / AES_GCM_decrypt, micro_aes.c:1164-1212; gHash :1127-1137), the C host's
 * form of the sharded GCM described further down: device i runs CTR over its 16-byte aligned slice at keystream block
 * J0 + 1 + slice_start / 16 FUSED with the slice's weighted share of Enc(J0) ^ GHASH (one pass over the text; the
 * first slice carries aData and Enc(J0), the last one the length block); the host XORs the ndev 16-byte shares -- the
 * only exchange GCM needs, and it needs no collective in one process.  12-byte nonce, 16-byte tag at crtxt + ptextLen
 * / read at crtxt + crtxtLen, bit for bit what uaes_gcm_encrypt / _decrypt give on one device.
 * decrypt keeps N7 across devices: every device hashes its slice of the INPUT, the host compares the tag, and only
 * then is anything written; a forgery returns UAES_E_AUTHENTICATION with every slice of pntxt untouched.  (Host
 * buffers: each slice is decrypted inside a private device buffer during the hashing pass and copied out after the
 * verdict, so the text crosses each device's link once per direction.  Device buffers: two passes, or -- under
 * uaes_set_gcm_one_pass_decrypt -- one pass and zeroed slices on a forgery.)                                      */
int uaes_mgpu_gcm_encrypt(int ndev, const int *devices, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *pntxt, size_t ptextLen, void *crtxt);
int uaes_mgpu_gcm_decrypt(int ndev, const int *devices, int keybits, const uint8_t *key, const uint8_t *nonce,
                          const void *aData, size_t aDataLen, const void *crtxt, size_t crtxtLen, void *pntxt);

/* The same split WITHOUT a change in the caller: with a device list configured -- here, or by the environment
 * variable UAES_DEVICES=all | 0,1,2,... read at first use -- the synchronous uaes_ecb_* / uaes_ctr_xcrypt* /
 * uaes_xts_sectors / uaes_gcm_encrypt / uaes_gcm_decrypt calls (and so the AES_* symbols of include/micro_aes.h) hand
 * a text that lies in HOST memory and is at least min_bytes long (UAES_DEVICES_MIN_MIB, default 64 MiB) to the
 * uaes_mgpu_* functions above, every device staging its slice over its own PCIe link; the bytes produced are the
 * one-device call's.  ndev = 0 switches it off (the default), -1 = every visible device, devices NULL = 0..ndev-1,
 * min_bytes 0 = keep the threshold.  Device-pointer calls and short texts are never split.                       */
int uaes_set_devices(int ndev, const int *devices, size_t min_bytes);

/* BASELINE configs[4] in one call: the plaintext lies sharded over ndev GPUs (d_in[i] on devices[i] holds the slice
 * uaes_mgpu_ctr_xcrypt_at would give device i: blocks [B*i/ndev, B*(i+1)/ndev) of the B = ceil(len/16) blocks), every
 * device encrypts its slice with the counter advanced by its block offset (incBlock's 56-bit add, micro_aes.c:421-427;
 * CTR_cipher :943-949 -- the reference has no collective), and the ciphertext slices are gathered into
 * d_full_on_root (len bytes on devices[root]) by RCCL over xGMI: grouped ncclSend / ncclRecv, one per peer, each slice
 * over its own link.  d_out[i] = device i's own ciphertext shard buffer (required for every device other than the root's;
 * on the root's device NULL means "encrypt straight into place").  RCCL is loaded with dlopen on first use with ndev > 1 (librccl.so.1,
 * or $UAES_RCCL_LIB): without it the call fails with UAES_E_HIP and uaes_last_error() says why; ndev = 1 needs no RCCL.
 * The communicators of the last device list are cached for the life of the process (ncclCommInitAll costs seconds). */
int uaes_mgpu_ctr_encrypt_gather(int ndev, const int *devices, int keybits, const uint8_t *key,
                                 const uint8_t ctr0[16], uint64_t block_offset,
                                 const void *const *d_in, size_t len, void *const *d_out,
                                 int root, void *d_full_on_root);

/* Test hooks of the gather (the one-GPU evidence that the RCCL code runs; tests/test_gpu_robustness.py, bench.py
 * --force-collective).  Environment, read on every call:
 *   UAES_GATHER_FORCE_RCCL=1   slices on the root's OWN device that were encrypted into shard buffers (d_out[i] given)
 *                              also travel by ncclSend / ncclRecv -- rank r to rank r on the cached communicator, which
 *                              RCCL allows inside a group -- instead of hipMemcpy; ndev = 1 then loads RCCL too.
 *   UAES_GATHER_FAIL_SEND=k    the k-th ncclSend of the call names a peer the communicator does not have: RCCL itself
 *                              refuses it with the group open.  The call returns UAES_E_HIP, every gather stream is
 *                              drained before it returns, and the communicators are aborted and rebuilt on the next call.
 * out[0..4] = ncclSend calls accepted, ncclRecv calls accepted, groups opened, ncclCommInitAll runs, failed gathers --
 * since the library was loaded. */
void uaes_debug_gather_stats(unsigned long out[5]);

/* ---- the table of arrangements, as data ------------------------------------------------------------------------
 * Which kernels a call runs is decided in ONE place per mode (csrc/uaes_plan.h holds the table and the names; the
 * launchers switch on the same functions).  uaes_debug_plan() returns that decision without running anything:
 *   mode   0 ECB, 1 CTR, 2 XTS, 3 GCM, 4 OCB, 5 GCM-SIV
 *   dir    0 encrypt, 1 decrypt (GCM: tag first, N7), 2 GCM decrypt in one pass, 3 GCM tag only
 *   a, b   bytes of text, bytes of associated data (XTS: bytes per data unit, number of units)
 *   flags  bit 0 key context, bit 1 explicit XTS tweak, bit 2 no counter word (two-launch forms), bit 3 LE32 counter
 *   out    [0] arrangement id (uaes_debug_arrangement_name), [1] kernel launches, [2] workgroups of the main kernel,
 *          [3] GHASH positions per thread (chunk arrangements)
 * Works without a device (answers for a 256-CU MI355X).  uaes_debug_plan_disable(mask): arrangements whose bit
 * (1u << id) is set are passed over wherever another one can take the call (measurement and tests; environment
 * UAES_PLAN_DISABLE gives the initial mask).  tests/test_gpu_plan.py derives its parity cases from this table.
 * Under UAES_GCM_FOLD=0 the answer is the two-launch form the call then takes (GCM-SIV: the levels).
 * uaes_debug_plan_at(): the same for a call whose keystream starts from counter16 -- the CTR call's first counter
 * block, or the GCM call's J0 (GHASH of the nonce for a nonce that is not 12 bytes long).  The low byte of that
 * counter decides where the text's groups of 256 counters and its stripes fall, and a text in which counter bits
 * 40..47 move is not one striped launch (CTR: 2 launches; GCM: not gcm.striped).  counter16 = NULL is
 * uaes_debug_plan(): a 12-byte CTR IV with start value 1, a 12-byte GCM nonce.  Other modes ignore it. */
int uaes_debug_plan(int mode, int dir, size_t a, size_t b, unsigned flags, int out[4]);
int uaes_debug_plan_at(int mode, int dir, size_t a, size_t b, unsigned flags, const uint8_t counter16[16], int out[4]);
const char *uaes_debug_arrangement_name(int id);
void uaes_debug_plan_disable(unsigned mask);
/* Poly1305's planner (csrc/uaes_plan.h, its own rows): the arrangement name ("poly.small" / "poly.chunks" /
 * "poly.batch") for one message of len bytes (nmsg <= 1) or a batch of nmsg >= 2 such messages; out (may be NULL)
 * = launches, workgroups of the main kernel, blocks per thread.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_poly1305(size_t len, size_t nmsg, int out[3]);
/* EAX / SIV's planner (csrc/uaes_plan.h, its own rows): "eax.small" / "eax.long" / "eax.batch" (siv = 0) or
 * "s2v.small" / "s2v.long" / "s2v.batch" (siv = 1) for one text of len bytes (nmsg <= 1) or a batch of nmsg >= 2,
 * dir 0 encrypt / 1 decrypt; out (may be NULL) = launches, workgroups of the main kernel, UAES_EAX_SIV_SMALL_MAX
 * (the longest text of the small arrangement).  NULL for arguments that make no sense. */
const char *uaes_debug_plan_eax_siv(int siv, int dir, size_t len, size_t nmsg, int out[3]);
/* The same for the calls with a vector of associated data: "s2v.small.v" / "s2v.long.v" for uaes_siv_*_v with a text of
 * len bytes and nad components (nmsg <= 1), "s2v.batch.v" for uaes_siv_*_batch_v with nmsg >= 2 records; out (may be
 * NULL) = launches, workgroups of the main kernel, the rows of sixteen lanes the components are dealt over (a batch
 * record's one row walks its own: 1).  NULL for a dir other than 0 / 1 or more components than the call takes. */
const char *uaes_debug_plan_siv_v(int dir, size_t len, size_t nad, size_t nmsg, int out[3]);
/* The planner of EAX' (csrc/uaes_plan.h): "eaxp.small" / "eaxp.long" / "eaxp.batch", out as uaes_debug_plan_eax_siv; NULL for a
 * dir other than 0 / 1.  Works without a device. */
const char *uaes_debug_plan_eaxp(int dir, size_t len, size_t nmsg, int out[3]);
/* The planners of the feedback modes, the CBC-MAC modes and the batches of chains (csrc/uaes_plan.h, their own rows):
 *   what   0 CBC with CS3 stealing, 1 CFB, 2 OFB, 3 CMAC, 4 CCM, 5 uaes_cbc_encrypt_batch, 6 uaes_cmac_batch,
 *          7 CBC without stealing (uaes_cbc_encrypt_padded / uaes_cbc_decrypt_blocks), 9 uaes_ccm_*_batch
 *          (8 is not assigned)
 *   dir    0 encrypt (or the MAC), 1 decrypt
 *   a, b   bytes of text (batches: bytes per message), messages of a batch (ignored otherwise)
 *   out    (may be NULL) launches, workgroups of the main kernel, its threads per workgroup
 * Returns "chain.serial" (one wave walks the chain), "fbdec.single" / "fbdec.tiled" (the block-parallel decrypt with
 * one / four blocks per lane), "ccm.fused" / "ccm.split", "batch.row" / "batch.lane" (sixteen lanes / one lane per
 * message), "ccm.batch" (sixteen lanes per record), or NULL for arguments that make no sense.  Works without a device (a 256-CU MI355X).
 * tests/test_gpu_chains.py derives its sizes and message counts from this. */
const char *uaes_debug_plan_chain(int what, int dir, size_t a, size_t b, int out[3]);
/* The planner of key wrap (csrc/uaes_plan.h, its own rows): dir 0 wrap / 1 unwrap; len = bytes of the SECRET in either
 * direction; nkeys 0 = uaes_kw_wrap / uaes_kw_unwrap, nkeys >= 1 = a batch of that many records.  out (may be NULL)
 * receives { launches, workgroups, threads per workgroup } (a batch: sixteen threads per record).  Returns "kw.lds"
 * (the semiblocks in LDS), "kw.global" (in place in the output buffer) or "kw.batch", or NULL for arguments that make
 * no sense: a length that is no multiple of 8 or below 16, a batch record above the limit.  Works without a device (a
 * 256-CU MI355X).  tests/test_gpu_kw.py finds the two boundaries by walking this. */
const char *uaes_debug_plan_kw(int dir, size_t len, size_t nkeys, int out[3]);
/* The planner of key wrap with padding (csrc/uaes_plan.h): dir 0 wrap / 1 unwrap; len = bytes of the secret for a wrap,
 * wrapLen - 8 for an unwrap; nkeys 0 = uaes_kwp_wrap / uaes_kwp_unwrap, nkeys >= 1 = a batch of that many slots of len
 * bytes.  out as above.  Returns "kwp.block" (padded length 8: one block, no chain), "kwp.lds", "kwp.global" or
 * "kwp.batch", or NULL: a length of 0 or beyond the MLI's range, an unwrap length that is no multiple of 8, a batch slot
 * above the limit.  Works without a device.  tests/test_gpu_kwp.py takes its boundaries from this. */
const char *uaes_debug_plan_kwp(int dir, size_t len, size_t nkeys, int out[3]);
/* The planner of FF1 (csrc/uaes_plan.h, its own rows): dir 0 encrypt / 1 decrypt; len = numerals of one text; nrec 0 =
 * uaes_ff1_encrypt / uaes_ff1_decrypt, nrec >= 1 = a batch of that many records.  out (may be NULL) receives
 * { launches, workgroups, threads per workgroup } (a batch: sixteen threads per record).  Returns "ff1.batch" (sixteen
 * lanes per record; one text within the batch limit is a batch of one), "ff1.wave" (one text on a wave of its own), or
 * NULL for arguments that make no sense: a radix outside 2..256, a length below the radix's minimum or above the
 * limit.  Works without a device (a 256-CU MI355X).  tests/test_gpu_ff1.py finds the boundary by walking this. */
const char *uaes_debug_plan_ff1(int dir, unsigned radix, size_t len, size_t nrec, int out[3]);
/* The planner of FF3-1 (csrc/uaes_plan.h): arguments and `out` as for FF1.  Returns "ff3.batch" (the one arrangement:
 * sixteen lanes per record, one text is a batch of one), or NULL for a dir other than 0 / 1, a radix outside 2..256, a
 * length below the radix's minimum or above uaes_ff3_maxlen(radix).  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_ff3(int dir, unsigned radix, size_t len, size_t nrec, int out[3]);
/* The planner of the GCM-SIV batches (csrc/uaes_plan.h): dir 0 encrypt / 1 decrypt; len = bytes per record, nmsg =
 * records; `out` as for FF1.  Returns "gcmsiv.batch" (the one arrangement: sixteen lanes per record, the same grid and
 * threads as "ccm.batch" for the same number of records), or NULL for a dir other than 0 / 1 or a length above
 * UAES_GCMSIV_BATCH_MAX.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_gcmsiv_batch(int dir, size_t len, size_t nmsg, int out[3]);
/* The planner of the multi-key GCM batches (csrc/uaes_plan.h): dir 0 encrypt / 1 decrypt; len = bytes per record, nmsg =
 * records; `out` as for FF1.  Returns "gcm.multikey" (the one arrangement: sixteen lanes per record, the same grid and
 * threads as "ccm.batch" for the same number of records), or NULL for a dir other than 0 / 1 or a length above
 * UAES_GCM_MULTIKEY_BATCH_MAX.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_gcm_multikey_batch(int dir, size_t len, size_t nmsg, int out[3]);
/* The planner of the XAES-256-GCM batches (csrc/uaes_plan.h): dir 0 encrypt / 1 decrypt; len = bytes per record, nmsg =
 * records; `out` as for FF1.  Returns "xaes.gcm" (the one arrangement: sixteen lanes per record, the same grid and
 * threads as "gcmsiv.batch" for the same number of records), or NULL for a dir other than 0 / 1 or a length above
 * UAES_XAES_GCM_BATCH_MAX.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_xaes256gcm_batch(int dir, size_t len, size_t nmsg, int out[3]);
/* The launch shape of OCB (csrc/uaes_plan.h, uaesk_plan_ocb_shape): dir 0 encrypt / 1 decrypt; len / aad_len = bytes of
 * text / of associated data; aad_aligned = whether the associated data starts at a multiple of 16 bytes in device
 * memory.  Returns "ocb.small" (one workgroup; out untouched) or "ocb.runs", for which out (may be NULL) receives
 * { run, run_aad, threads per workgroup, workgroups, hash_blocks }: the consecutive 256-block chunks a wave takes at
 * once over the text and over long associated data, and the whole blocks of associated data that all workgroups hash
 * (0: one workgroup hashes all of it -- short, or not aligned; INT_MAX from 32 GiB on).  NULL for a dir other than 0 / 1.  Works without a
 * device (a 256-CU MI355X).  tests/test_gpu_ocb.py finds the first text of every run length by walking this. */
const char *uaes_debug_plan_ocb(int dir, size_t len, size_t aad_len, int aad_aligned, int out[5]);
/* The launch shape of XTS (csrc/uaes_plan.h, uaesk_plan_xts_shape): sector_bytes = bytes per data unit, nsectors = units,
 * explicit_tweak = whether the call gives a 16-byte tweak (uaes_xts_encrypt / _decrypt) and not unit numbers.  Returns
 * "xts.small", "xts.packed" or "xts.bulk" as uaes_debug_plan does; out (may be NULL) receives { threads per workgroup,
 * workgroups, chunks_per_sector, nmain, chunks in all, serial, aligned, all-full } of the call's main kernel: the
 * 256-block chunks of a unit (the one with the first block of a stealing pair included), the chunks the kernel's main
 * loop takes a chunk per wave and all chunks (the rest goes by quarters), and whether one thread walks a unit's chunk
 * tweaks, every block lies at a multiple of 16 bytes, every chunk is whole.  NULL for a unit below 16 bytes or no unit.
 * Works without a device (a 256-CU MI355X).  tests/test_gpu_xts.py takes its unit counts from this. */
const char *uaes_debug_plan_xts(size_t sector_bytes, size_t nsectors, int explicit_tweak, uint64_t out[8]);
/* The planner of the OCB batches (csrc/uaes_plan.h): dir 0 encrypt / 1 decrypt; len = bytes per record, nmsg = records;
 * out (may be NULL) receives { launches, workgroups, threads per workgroup }.  Returns "ocb.batch" (the one
 * arrangement: sixteen lanes per record, the same grid and threads as "ccm.batch" for the same number of records), or
 * NULL for a dir other than 0 / 1 or a length above UAES_OCB_BATCH_MAX.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_ocb_batch(int dir, size_t len, size_t nmsg, int out[3]);
/* The planner of the cipher batches (csrc/uaes_plan.h): mode 0 uaes_cbc_decrypt_batch, 1 uaes_cbc_decrypt_blocks_batch,
 * 2 uaes_cbc_encrypt_blocks_batch, 3 uaes_cfb_encrypt_batch, 4 uaes_cfb_decrypt_batch, 5 uaes_ofb_xcrypt_batch,
 * 6 uaes_ctr_xcrypt_batch; len = bytes per record, nmsg = records; out (may be NULL) receives { launches, workgroups,
 * threads per workgroup }.  Returns "cipher.batch" (the one arrangement: sixteen lanes per record, the same grid and
 * threads as "ccm.batch" for the same number of records), or NULL for another mode, a CBC record that is not a whole
 * number of blocks or a record of the other modes above UINT32_MAX bytes.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_cipher_batch(int mode, size_t len, size_t nmsg, int out[3]);
/* The planner of the XTS batches and sector lists (csrc/uaes_plan.h): len = bytes per unit's slot, nmsg = units; out (may
 * be NULL) receives { launches, workgroups, threads per workgroup, units per workgroup }.  Returns "xts.batch" (the one
 * arrangement: sixteen lanes per unit, the same grid and threads as "ccm.batch" for the same number of records), or NULL
 * for a unit below 16 or above UINT32_MAX bytes.  Works without a device (a 256-CU MI355X). */
const char *uaes_debug_plan_xts_batch(size_t len, size_t nmsg, int out[4]);
/* The plan of one piece of a streamed GCM message (csrc/uaes_plan.h, uaesk_plan_gcm_piece: the function
 * uaes_gcm_stream_update's kernel layer switches on): decrypt 0 / 1; len = bytes of the piece; done_bytes = text the
 * stream has taken before it (a multiple of 16), which decides where the piece's groups of 256 counters fall.  The
 * stream is taken to use a 12-byte nonce and to have made its first absorb.  out = { arrangement id, launches,
 * workgroups, GHASH positions per thread } as for uaes_debug_plan; the arrangement "gcm.levels" (launches 0) means that
 * the piece is not taken: the CTR kernel and the GHASH levels run (the absorb path).  Returns 0, or UAES_E_ARG for a
 * done_bytes that is no multiple of 16.  Works without a device (a 256-CU MI355X).  tests/gcm_stream_cases.py derives
 * its piece lengths from this. */
int uaes_debug_plan_gcm_piece(int decrypt, size_t len, uint64_t done_bytes, int out[4]);
/* The table cache of a stream (plan_state): bit 31 = the tables of the stream's key are in its scratch, low byte = logA
 * of the bulk GHASH table there (0: none), bit 8 = the B table is there, bit 9 = the striped kernel's tables are there. */
unsigned uaes_debug_gcm_stream_tables(const uaes_gcm_stream *s);

/* Test hooks of the one-launch GCM / GCM-SIV / streamed-piece arrangements (chunk workgroups + one preparing workgroup
 * in ONE launch; whoever of them arrives last on a counter word folds the chunk hashes and makes the tag -- nobody
 * waits for anybody, DESIGN.md "GCM").  The preparing workgroup looks at the counter for a bounded time before it
 * counts itself in (default 1 ms; environment UAES_GCM_LOOK_TICKS): uaes_debug_gcm_look(0) makes it count in at
 * once, so that a chunk workgroup is usually the last and the fold runs THERE.  uaes_debug_gcm_chunk_folds: how many
 * folds a chunk workgroup has done on the current device.  UAES_GCM_FOLD=0 in the environment switches the
 * one-launch arrangements off altogether (chunks, then k_gcm_combine as a second launch). */
void uaes_debug_gcm_look(unsigned long long ticks_100mhz);
int uaes_debug_gcm_chunk_folds(unsigned *out);

/* Test hook of the key wipe: how many expanded key schedules the process holds at this moment.  Every call expands
 * its key into a schedule on its own stack and wipes it on every way out, so between calls the count is the number
 * of open key contexts (uaes_gcm_key) and streams (uaes_gcm_stream).  Works without a device. */
int uaes_debug_live_key_schedules(void);

/* ---- sharded GCM (multi-GPU) ------------------------------------------------
 * One message, cut into 16-byte aligned ciphertext shards, one per GPU.  Each
 * rank encrypts its shard with uaes_ctr_xcrypt_at_dev(ctr0 = nonce || 00000001,
 * block_offset = 1 + shard_offset/16) -- the CCM_GCM pre-increment of CTR_cipher
 * (micro_aes.c:939-941) -- and calls this function on the resulting ciphertext.
 * It returns 16 bytes: the shard's share of  Enc(J0) ^ GHASH(aData, crtxt)
 * (gHash, micro_aes.c:1127-1137; the first shard carries aData and Enc(J0), the
 * last one the length block).  The tag of AES_GCM_encrypt is the XOR of all
 * shards' shares -- a 16-byte-per-GPU exchange (RCCL all-gather), the only
 * collective GCM needs.  All data pointers are device pointers.               */
int uaes_gcm_partial_dev(int keybits, const uint8_t *key, const uint8_t *nonce,
                         const void *d_aad, uint64_t total_aad_len,
                         const void *d_ct_shard, size_t shard_len, uint64_t shard_offset,
                         uint64_t total_len, void *d_partial16, void *stream);

/* ... and the shard's CTR pass with it, in ONE pass over the text (what uaes_mgpu_gcm_* run per device): mode 0
 * encrypts d_in -> d_out (keystream block J0 + 1 + shard_offset / 16 onwards) and hashes d_out; mode 1 = the call
 * above (d_out unused); mode 2 decrypts d_in -> d_out and hashes d_in -- d_out is written before any tag is known: a
 * caller that must keep N7 (micro_aes.c:1200-1208) runs mode 1 on every shard first, compares the XOR of the shares
 * with the tag, and only then decrypts (uaes_ctr_xcrypt_at_dev at block offset 1 + shard_offset / 16).  Every shard
 * but the last is a multiple of 16 bytes; d_in == d_out is allowed.  Enqueue only.                               */
int uaes_gcm_shard_dev(int keybits, const uint8_t *key, const uint8_t *nonce, int mode,
                       const void *d_aad, uint64_t total_aad_len,
                       const void *d_in, size_t shard_len, uint64_t shard_offset, uint64_t total_len,
                       void *d_out, void *d_partial16, void *stream);

#ifdef __cplusplus
}
#endif
#endif
