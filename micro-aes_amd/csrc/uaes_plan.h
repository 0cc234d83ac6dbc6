/* uaes_plan.h -- the ONE table of arrangements: which kernels a call runs, by mode, direction and size.
 *
 * Every launcher of the kernel layer asks a planner of this file's family (uaesk_plan_ecb / _ctr / _xts / _gcm /
 * _ocb / _siv, defined next to the kernels they plan for) and switches on the answer; uaes_debug_plan() in the C ABI
 * (include/uaes_hip.h) returns the same answer as data, and tests/test_gpu_plan.py derives its parity cases from it:
 * it walks the sizes, finds every boundary b at which the answer changes and checks b - 16, b, b + 16 in both
 * directions (and a forged tag) against the oracle.  There is no other place where a size threshold decides what
 * runs.  Three switches are read from the environment, and none of them moves a threshold: UAES_PLAN_DISABLE (the
 * initial mask of uaesk_plan_disable below), UAES_GCM_FOLD=0 (no counter word reaches the kernels, so the one-launch GCM forms become
 * their two-launch forms and GCM-SIV takes the levels; the planners answer the same) and UAES_GCM_LOOK_TICKS (how long
 * the one-launch GCM kernel's preparing workgroup looks at the arrival counter; it does not change the arrangement).
 *
 *   mode  arrangement           kernels (launches)                                         reached when
 *   ----  --------------------  ---------------------------------------------------------  ---------------------------------
 *   ECB   ECB_SINGLE            k_ecb<U=1>                                          (1)    < half the CUs' worth of 4-block tiles
 *         ECB_TILED             k_ecb<U=4>                                          (1)    otherwise
 *   CTR   CTR_SINGLE            k_ctr<U=1>                                          (1)    < half the CUs' worth of tiles
 *         CTR_QUAD              k_ctr<U=4>                                          (1)    < one grid of 8-group stripes, or LE32 counter
 *         CTR_STRIPED           k_ctr_shared2 (rounds 1-2 shared per 256 counters)  (1)    >= one grid of stripes (8 MiB on 256 CUs)
 *   XTS   XTS_SMALL             k_xts_small [+ k_xts_cts]                           (1-2)  one unit <= 8 MiB, or <= 4 MiB of whole-block units
 *         XTS_PACKED            k_xts_tweaks + k_xts<PACKED>                        (2)    units shorter than a chunk, whole blocks
 *         XTS_BULK              k_xts_tweaks [+ k_xts_expand] + k_xts [+ k_xts_cts] (2-4)  everything else (C3: 2^20 sectors of 4 KiB)
 *         xts.batch             k_xts_batch (sixteen lanes per unit, four per wave; a tweak per unit) (1)  uaes_xts_*_batch, uaes_xts_sector_list: any number of units
 *   GCM   GCM_SMALL             k_gcm_small                                      (1)    <= 2046 GHASH positions (~32 KiB)
 *         GCM_CHUNKS            k_gcm_chunks<FOLD> [+ gated k_ctr*]                 (1-2)  encrypt <= 16 MiB; tag-first decrypt <= 512 MiB
 *                               (k_gcm_chunks + k_gcm_combine without a counter word or for a one-pass decrypt)
 *         GCM_TWOPHASE          k_ctr_shared2, then hash-only k_gcm_chunks<FOLD>    (2)    encrypt / one-pass decrypt, 16 .. 128 MiB
 *         GCM_STRIPED           k_gcm_setup | k_gcm_ej0, k_gcm_fused, k_ghash_final (3)    encrypt / one-pass decrypt beyond (C4: 1 GiB)
 *         GCM_LEVELS            k_gcm_setup, k_ctr*, k_ghash_pass x0-2, k_ghash_final (3-5) whatever is left (tag-only; > 512 MiB tag-first)
 *         gcm.multikey          k_gcm_multikey (sixteen lanes per record, four per wave; a key per record) (1)  uaes_gcm_multikey_*_batch, records <= UAES_GCM_MULTIKEY_BATCH_MAX (65535 B)
 *         xaes.gcm              k_xaes_gcm_batch (sixteen lanes per record, four per wave; a key per nonce) (1)  uaes_xaes256gcm_*_batch, records <= UAES_XAES_GCM_BATCH_MAX (65535 B)
 *   OCB   OCB_SMALL             k_ocb_small                                         (1)    <= OCB_SMALL_BLOCKS blocks and short AAD
 *         OCB_RUNS              k_ocb (last workgroup to arrive makes the tag)      (1)    otherwise
 *         ocb.batch             k_ocb_batch (sixteen lanes per record, four per wave) (1)  uaes_ocb_*_batch, records <= UAES_OCB_BATCH_MAX (65535 B)
 *   SIV   SIV_SMALL             k_siv_small                                         (1)    <= 2046 POLYVAL positions
 *         SIV_CHUNKS            k_siv_prep, hash-only k_gcm_chunks<FOLD>, k_ctr*    (3)    <= 512 MiB
 *         SIV_LEVELS            k_siv_prep, k_ghash_pass.., k_siv_tag, k_ctr*       (4-6)  beyond
 *         gcmsiv.batch          k_gcmsiv_batch (sixteen lanes per record, four per wave) (1)  uaes_gcmsiv_*_batch, records <= UAES_GCMSIV_BATCH_MAX (65535 B)
 *   POLY  poly.small            k_poly_small (one workgroup, AES_k(nonce) inside)   (1)    one message <= UAES_POLY_SMALL_MAX (128 KiB)
 *         poly.chunks           k_poly_chunks, k_poly_fold (+ AES_k(nonce))         (2)    one message beyond
 *         poly.batch            k_poly_batch (one wave per message)                 (1)    uaes_poly1305_batch
 *   EAX   eax.small             k_eax_small (N || H, CTR, C; decrypt: N || H || C, CTR)  (1)  text <= UAES_EAX_SIV_SMALL_MAX
 *         eax.long              k_eax_macs, CTR (k_ctr*) [, k_eax_macs C]           (3)    beyond (the counter block and the
 *                                                                                          verdict come back to the host)
 *         eax.batch             k_eax_batch (sixteen lanes per record)              (1)    uaes_eax_*_batch
 *   EAX'  eaxp.small            k_eaxp_small (N, CTR, C'; decrypt: N || C', CTR)    (1)    text <= UAES_EAX_SIV_SMALL_MAX
 *         eaxp.long             k_eaxp_macs, CTR (k_ctr*) [, k_eaxp_macs C']        (2-3)  beyond (as eax.long)
 *         eaxp.batch            k_eaxp_batch (sixteen lanes per record; nlens, lens) (1)   uaes_eaxp_*_batch
 *   S2V   s2v.small             k_s2v_small (Y || lead blocks, then CTR)            (1)    text <= UAES_EAX_SIV_SMALL_MAX
 *         s2v.long              k_s2v_macs and CTR (k_ctr*), in either order        (2)    beyond
 *         s2v.batch             k_s2v_batch (sixteen lanes per record)              (1)    uaes_siv_*_batch
 *         s2v.small.v           k_s2v_v<CTR> (components over 60 rows || lead blocks, fold, CTR) (1)  uaes_siv_*_v, text <= UAES_EAX_SIV_SMALL_MAX
 *         s2v.long.v            k_s2v_v and CTR (k_ctr*), in either order           (2)    uaes_siv_*_v beyond
 *         s2v.batch.v           k_s2v_batch_v (sixteen lanes per record; lens)      (1)    uaes_siv_*_batch_v
 *   CBC   chain.serial          k_chain_serial (one wave walks the chain)           (1)    CBC encrypt, CFB encrypt, OFB: any length
 *   CFB   fbdec.single          k_fb_dec<U=1> (the CS3 pair / CFB tail: one lane)   (1)    CBC / CFB decrypt, < half the CUs' worth of
 *   OFB                                                                                    4-block tiles (<= 8 MiB on 256 CUs)
 *         fbdec.tiled           k_fb_dec<U=4>                                       (1)    CBC / CFB decrypt beyond
 *   CMAC  chain.serial          k_cmac (one wave)                                   (1)    any length
 *   CCM   ccm.fused             k_ccm (MAC rows and keystream rows share the wave)  (1)    text <= UAES_CCM_FUSED_MAX (256 B)
 *         ccm.split             k_ccm_tag and CTR (k_ctr*), decrypt: CTR first      (2+)   beyond
 *         ccm.batch             k_ccm_batch (sixteen lanes per record, four per wave) (1)  uaes_ccm_*_batch, records <= UAES_CCM_BATCH_MAX (65535 B)
 *   batch batch.row             k_chain_batch_row (sixteen lanes per message)       (1)    uaes_cbc_encrypt_batch / uaes_cmac_batch,
 *                                                                                          <= UAES_BATCH_ROW_MAX messages (81 919)
 *         batch.lane            k_chain_batch (one lane per message)                (1)    more messages
 *         cipher.batch          k_cipher_batch (sixteen lanes per record, four per wave) (1)  uaes_cbc_decrypt_batch, uaes_cbc_*_blocks_batch,
 *                                                                                          uaes_cfb_*_batch, uaes_ofb_xcrypt_batch,
 *                                                                                          uaes_ctr_xcrypt_batch: any number of records
 *   KW    kw.lds                k_kw<LDS> (one wave; the semiblocks in LDS)         (1)    secret <= UAES_KW_LDS_MAX (4 KiB)
 *         kw.global             k_kw<in place> (one wave; loads a chunk ahead)      (1)    beyond
 *         kw.batch              k_kw_batch (sixteen lanes per record)               (1)    uaes_kw_*_batch, <= UAES_KW_BATCH_MAX (256 B)
 *   KWP   kwp.block             k_kw<block, padded> (one wave; one block, no chain) (1)    secret <= 8 B (padded length 8)
 *         kwp.lds               k_kw<LDS, padded>                                   (1)    padded length <= UAES_KW_LDS_MAX (4 KiB)
 *         kwp.global            k_kw<in place, padded>                              (1)    beyond
 *         kwp.batch             k_kw_batch<padded> (lengths per record)             (1)    uaes_kwp_*_batch, <= UAES_KW_BATCH_MAX (256 B)
 *   FF1   ff1.batch             k_ff1<16> (sixteen lanes per record, four per wave) (1)    uaes_ff1_*_batch; one text of <= UAES_FF1_BATCH_MAX (128) numerals
 *         ff1.wave              k_ff1<64> (one wave per text)                       (1)    one longer text, <= UAES_FF1_MAX (4096) numerals
 *   FF3-1 ff3.batch             k_ff3 (sixteen lanes per record, four per wave)     (1)    uaes_ff3_*_batch; one text (<= 192 numerals) is a batch of one
 * The Poly1305 rows have a planner of their own (uaesk_plan_poly1305, uaes_poly1305.hip) and ids outside enum
 * uaes_arrangement (uaes_debug_plan_poly1305 names them); a larger message never goes back to a smaller row.
 * So do the EAX and SIV (RFC 5297) rows (uaesk_plan_eax_siv and, for the .v rows, uaesk_plan_siv_v, uaes_eax_siv.hip;
 * uaes_debug_plan_eax_siv, uaes_debug_plan_siv_v; the EAX' rows: uaesk_plan_eaxp, uaes_debug_plan_eaxp), and the
 * CBC / CFB / OFB / CMAC / CCM / batch rows (uaesk_plan_chain, uaes_chain.hip, and uaesk_plan_mac / uaesk_plan_ccm_batch,
 * uaes_mac.hip; uaes_debug_plan_chain); tests/test_gpu_chains.py derives its sizes and message counts from them.  Key wrap has
 * uaesk_plan_kw (uaes_kw.hip; uaes_debug_plan_kw), and tests/test_gpu_kw.py finds its two boundaries by walking it; key
 * wrap with padding has uaesk_plan_kwp beside it (uaes_debug_plan_kwp; tests/test_gpu_kwp.py).
 * FF1 has uaesk_plan_ff1 (uaes_ff1.hip; uaes_debug_plan_ff1); tests/test_gpu_ff1.py walks it likewise.
 * FF3-1 has uaesk_plan_ff3 (uaes_ff3.hip; uaes_debug_plan_ff3): one row, whose limits depend on the radix.
 * The GCM-SIV batches have uaesk_plan_gcmsiv_batch (uaes_gcmsiv_batch.hip; uaes_debug_plan_gcmsiv_batch): one row.
 * The XTS rows say which kernels run; the shape they are launched with -- workgroups, the main loop's share of the chunks,
 * which form of k_xts -- is uaesk_plan_xts_shape (uaes_kernels.hip; uaes_debug_plan_xts), and tests/test_gpu_xts.py takes its
 * unit counts from it.
 * OCB_RUNS is one row whose launch shape moves with the size: uaesk_plan_ocb_shape (uaes_ocb.hip; uaes_debug_plan_ocb),
 * and tests/test_gpu_ocb.py takes its sizes from walking it.  The OCB batches have uaesk_plan_ocb_batch (uaes_ocb.hip;
 * uaes_debug_plan_ocb_batch): one row, with an id outside enum uaes_arrangement.  So do the multi-key GCM batches:
 * uaesk_plan_gcm_multikey_batch (uaes_gcm_multikey.hip; uaes_debug_plan_gcm_multikey_batch), and the batches of the plain
 * cipher modes: uaesk_plan_cipher_batch (uaes_cipher_batch.hip; uaes_debug_plan_cipher_batch), and the XAES-256-GCM
 * batches: uaesk_plan_xaes_gcm_batch (uaes_xaes.hip; uaes_debug_plan_xaes256gcm_batch), and the XTS batches and sector
 * lists: uaesk_plan_xts_batch (uaes_xts_batch.hip; uaes_debug_plan_xts_batch).
 * The rows that say "sixteen lanes per record / message / unit" -- eax.batch, eaxp.batch, s2v.batch, ccm.batch, gcmsiv.batch, gcm.multikey, xaes.gcm, ocb.batch, batch.row,
 * xts.batch, cipher.batch, kw.batch, kwp.batch, ff1.batch, ff3.batch -- are the row batches: grid and threads per workgroup are uaesk_row_shape's (uaes_launch.hip.h), the same
 * for the same number of records in every one of them.
 */
#ifndef UAES_PLAN_H
#define UAES_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum uaes_plan_mode { UAES_PLAN_ECB = 0, UAES_PLAN_CTR = 1, UAES_PLAN_XTS = 2, UAES_PLAN_GCM = 3, UAES_PLAN_OCB = 4, UAES_PLAN_SIV = 5 };

enum uaes_arrangement {
    UAES_ARR_ECB_SINGLE = 0,
    UAES_ARR_ECB_TILED,
    UAES_ARR_CTR_SINGLE,
    UAES_ARR_CTR_QUAD,
    UAES_ARR_CTR_STRIPED,
    UAES_ARR_XTS_SMALL,
    UAES_ARR_XTS_PACKED,
    UAES_ARR_XTS_BULK,
    UAES_ARR_GCM_SMALL,
    UAES_ARR_GCM_CHUNKS,
    UAES_ARR_GCM_TWOPHASE,
    UAES_ARR_GCM_STRIPED,
    UAES_ARR_GCM_LEVELS,
    UAES_ARR_OCB_SMALL,
    UAES_ARR_OCB_RUNS,
    UAES_ARR_SIV_SMALL,
    UAES_ARR_SIV_CHUNKS,
    UAES_ARR_SIV_LEVELS,
    UAES_ARR_COUNT
};

/* directions: 0 = encrypt, 1 = decrypt (GCM: tag first, N7), 2 = GCM decrypt in one pass (uaes_set_gcm_one_pass_decrypt),
 * 3 = GCM tag only (truncated tags: the host layer compares) */

/* a planner's answer */
typedef struct {
    int      arrangement;        /* enum uaes_arrangement */
    int      launches;           /* kernels the call enqueues */
    unsigned grid, steps;        /* workgroups of the main kernel; CHUNKS / TWOPHASE: GHASH positions per thread */
} uaes_plan;

/* Test / measurement hook: arrangements whose bit (1u << id) is set are not chosen where another one can take the
 * call (GCM_LEVELS, XTS_BULK, CTR_QUAD, ECB_TILED, OCB_RUNS and SIV_LEVELS take everything and cannot be switched
 * off).  Process-wide; UAES_PLAN_DISABLE in the environment (a number, e.g. 0x1c00) is its initial value. */
void     uaesk_plan_disable(unsigned mask);
unsigned uaesk_plan_disabled(void);

/* a = bytes of text (XTS: bytes per data unit), b = bytes of associated data (XTS: number of units; ECB / CTR: unused),
 * flags bit 0: GCM with a key context, bit 1: XTS with an explicit 16-byte tweak, bit 2: no counter word armed (the
 * two-launch form of the one-launch arrangements), bit 3: CTR with the little-endian 32-bit counter (GCM-SIV).
 * The number of CUs decides most boundaries; without a device the answer is the one for a 256-CU MI355X.  Returns 0
 * and fills *p, or a HIP error code for arguments that make no sense. */
int uaesk_plan(int mode, int dir, size_t a, size_t b, unsigned flags, uaes_plan *p);
/* the same for a call whose keystream starts from a given counter: counter16 = the CTR call's first counter block
 * (ctr0 at block offset 0) or the GCM call's J0 (the keystream starts at J0 + 1).  Where a CTR or GCM text's groups of
 * 256 counters and its stripes fall depends on the counter's low byte, and a text in which counter bits 40..47 move
 * cannot be one striped launch (CTR: two launches; GCM: not gcm.striped).  NULL = uaesk_plan (CTR: a 12-byte IV and
 * start value 1; GCM: a 12-byte nonce).  Other modes ignore it. */
int uaesk_plan_at(int mode, int dir, size_t a, size_t b, unsigned flags, const uint8_t *counter16, uaes_plan *p);

/* one piece of a streamed GCM message (uaes_gcm.hip's gcm_piece_plan, which uaesk_gcm_stream_piece switches on;
 * uaes_debug_plan_gcm_piece): len bytes of text behind done_bytes (a multiple of 16) already taken, under a 12-byte
 * nonce, in a stream that has its counter word and the tables of its first absorb.  A piece has no small arrangement
 * and no AAD; where its stripes fall depends on done_bytes (the first counter is 2 + done_bytes / 16).  GCM_LEVELS
 * (launches 0) = not taken: the caller runs the CTR kernel and uaesk_gcm_stream_absorb.  tests/gcm_stream_cases.py
 * derives its piece lengths from this. */
int uaesk_plan_gcm_piece(int decrypt, size_t len, uint64_t done_bytes, uaes_plan *p);

const char *uaesk_arrangement_name(int id);

/* OCB's runs arrangement answers ("ocb.runs", 1, 0, 0) at every size; the shape k_ocb is launched with is a table of
 * its own (uaes_ocb.hip's ocb_shape, which launch_ocb launches from; uaes_debug_plan_ocb).  dir: 0 encrypt, 1 decrypt;
 * aad_aligned: whether the associated data starts at a multiple of 16 bytes in device memory (only then do all
 * workgroups hash it).  out = { run, run_aad, threads per workgroup, workgroups, hash_blocks }: the consecutive
 * 256-block chunks a wave takes at once on the walk over the text and on the walk over long associated data (powers
 * of two up to 16; 1 below 8 runs per wave), and the whole blocks of associated data that walk hashes (0: the finishing
 * workgroup hashes all of it).  Returns 0, or 1 with out untouched where the call is OCB_SMALL's, or a HIP error code
 * for a dir other than 0 / 1.  tests/test_gpu_ocb.py finds the first text of every run length by walking this. */
int uaesk_plan_ocb_shape(int dir, size_t len, size_t aad_len, int aad_aligned, int out[5]);

/* The XTS rows answer ("xts.bulk", n, 0, 0) and ("xts.packed", 2, 0, 0) at every size; the shape their main kernel is
 * launched with is uaes_kernels.hip's xts_shape, which launch_xts launches from (uaes_debug_plan_xts).  out = { threads
 * per workgroup, workgroups, chunks_per_sector, nmain, chunks in all, serial, aligned, all-full }: of k_xts_small for
 * XTS_SMALL, else of k_xts (0 threads and workgroups where a unit is a stealing pair and nothing else).  A chunk is 256
 * blocks.  chunks_per_sector counts the chunk that holds the first block of the stealing pair, which is one more than
 * the chunks with blocks of k_xts's when that block is the first of a chunk.  k_xts takes chunks [0, nmain) a chunk per
 * wave and [nmain, chunks in all) by quarters (XTS_PACKED numbers the chunks of the whole text, the others unit by
 * unit); serial: k_xts_tweaks walks a unit's chunk tweaks itself (else k_xts_expand); aligned: every block at a
 * multiple of 16 bytes; all-full: every chunk has 256 blocks.  Returns 0, or a HIP error code for a unit below 16 bytes
 * or no unit. */
int uaesk_plan_xts_shape(size_t sector_bytes, size_t nsectors, int explicit_tweak, uint64_t out[8]);

/* Poly1305-AES: len = bytes of one message; nmsg >= 2 = a batch of nmsg messages of len bytes each (nmsg 0 / 1: the
 * one-message calls).  grid = workgroups of the main kernel, steps = blocks per thread (at most). */
enum uaes_poly_arrangement { UAES_POLY_SMALL = 0, UAES_POLY_CHUNKS = 1, UAES_POLY_BATCH = 2 };
int uaesk_plan_poly1305(size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_poly1305_arrangement_name(int id);

/* EAX and SIV (RFC 5297): a text of at most UAES_EAX_SIV_SMALL_MAX bytes is one launch of one workgroup; a longer one
 * runs its independent CMAC chains in one launch, fetches the counter block and the verdict in one round trip and
 * then runs the positioned CTR kernels.  siv: 0 = EAX, 1 = SIV; dir: 0 encrypt, 1 decrypt; nmsg >= 2 = a batch.
 * launches = kernels the call enqueues; grid = workgroups of the main kernel. */
#define UAES_EAX_SIV_SMALL_MAX ((size_t)16384)
enum uaes_eax_siv_arrangement { UAES_EAX_SMALL = 0, UAES_EAX_LONG, UAES_EAX_BATCH, UAES_S2V_SMALL, UAES_S2V_LONG, UAES_S2V_BATCH,
                                UAES_S2V_SMALL_V, UAES_S2V_LONG_V, UAES_S2V_BATCH_V, UAES_EAXP_SMALL, UAES_EAXP_LONG, UAES_EAXP_BATCH };
int uaesk_plan_eax_siv(int siv, int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_eax_siv_arrangement_name(int id);
/* EAX' (uaes_eaxp_*): the same boundary and the same three forms; it has no associated data, so a longer decryption is
 * two launches and a longer encryption three.  Returns a HIP error code for a dir other than 0 / 1. */
int uaesk_plan_eaxp(int dir, size_t len, size_t nmsg, uaes_plan *p);
/* SIV with a vector of associated data (uaes_siv_*_v, uaes_siv_*_batch_v): the same boundary, with nad components of
 * associated data, at most UAES_S2V_AD_MAX in a single call (RFC 5297: S2V takes 127 strings, the text included) and
 * UAES_S2V_BATCH_AD_MAX in a batch record (their lengths travel by value).  steps = the rows of the workgroup the
 * components are dealt over, round-robin (a batch record's one row walks its own: 1).  Returns a HIP error code for a
 * dir other than 0 / 1 or more components than the call takes. */
#define UAES_S2V_AD_MAX       126
#define UAES_S2V_BATCH_AD_MAX 8
int uaesk_plan_siv_v(int dir, size_t len, size_t nad, size_t nmsg, uaes_plan *p);

/* The feedback modes, the CBC-MAC modes and the batches of chains.  what = enum uaes_chain_what; dir: 0 encrypt (or
 * the MAC), 1 decrypt; a = bytes of text (batches: bytes per message), b = messages of a batch (other rows ignore it).
 * launches = kernels the call enqueues (ccm.split: k_ccm_tag plus what the CTR planner answers for a text of a bytes
 * whose counter does not carry into bits 40..47); grid = workgroups of the main kernel, steps = its threads per
 * workgroup; every launcher of the two files takes its launch shape from these answers.  uaesk_plan_chain
 * (uaes_chain.hip) answers for CBC / CFB / OFB and the two batches, uaesk_plan_mac (uaes_mac.hip) for CMAC and CCM
 * (the launchers use its static core, which does not ask the CTR planner); either returns a HIP error code for a `what` of the other's or arguments that make
 * no sense (CBC with stealing below 16 bytes, a batched CBC message that is not whole blocks).
 * uaesk_plan_ccm_batch (uaes_mac.hip) answers for the batches of CCM records (UAES_WHAT_CCM_BATCH): len = bytes per
 * record, nmsg = records; a row batch at any number of records.  A record is at most
 * UAES_CCM_BATCH_MAX bytes: the longest text whose length every nonce length 7..13 can still encode in B0 (two bytes
 * are left behind a 13-byte nonce), so that no record's counter can leave its field.
 * UAES_WHAT_CCM_BATCH is 9, not 8: 8 was UAES_WHAT_COUNT, the one value past the end that the plan test keeps asking
 * for and expects no plan for; it stays unassigned. */
#define UAES_CCM_FUSED_MAX ((size_t)256)
#define UAES_BATCH_ROW_MAX ((size_t)81919)
#define UAES_CCM_BATCH_MAX ((size_t)65535)
enum uaes_chain_what { UAES_WHAT_CBC = 0, UAES_WHAT_CFB, UAES_WHAT_OFB, UAES_WHAT_CMAC, UAES_WHAT_CCM, UAES_WHAT_CBC_BATCH,
                       UAES_WHAT_CMAC_BATCH, UAES_WHAT_CBC_NOCTS, UAES_WHAT_CCM_BATCH = 9, UAES_WHAT_COUNT };
enum uaes_chain_arrangement { UAES_CHAIN_SERIAL = 0, UAES_FBDEC_SINGLE, UAES_FBDEC_TILED, UAES_CCM_FUSED, UAES_CCM_SPLIT,
                              UAES_BATCH_ROW, UAES_BATCH_LANE, UAES_CCM_BATCH };
int uaesk_plan_chain(int what, int dir, size_t a, size_t b, uaes_plan *p);
int uaesk_plan_mac(int what, int dir, size_t a, uaes_plan *p);
int uaesk_plan_ccm_batch(int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_chain_arrangement_name(int id);

/* AES key wrap (RFC 3394; uaes_kw.hip).  dir: 0 wrap, 1 unwrap; len = bytes of the SECRET in either direction (the
 * wrapped form is 8 bytes longer); nkeys 0 = the one-secret calls, nkeys >= 1 = a batch of nkeys records of len bytes.
 * One secret is one wave: up to UAES_KW_LDS_MAX bytes its semiblocks live in LDS behind the row tables, a longer one
 * is worked on in place in the output buffer (a semiblock is next touched n - 1 chain steps after it was stored, far
 * longer than a store and a load take, so its load is requested a chunk of steps ahead and never sits on the chain;
 * below the boundary that distance would be too short, and 4 KiB of LDS cost nothing).  A batch record is at most
 * UAES_KW_BATCH_MAX bytes: 64 records of a workgroup keep their semiblocks in the 31 KiB of LDS the row4 tables leave
 * (a 2048-bit secret still fits).  grid = workgroups, steps = threads per workgroup (batch: sixteen per record).
 * Returns a HIP error code for a length that is no multiple of 8 or below 16, or a batch record above the limit. */
#define UAES_KW_LDS_MAX   ((size_t)4096)
#define UAES_KW_BATCH_MAX ((size_t)256)
/* one enum for both planners (block: uaesk_plan_kwp alone); each has its own names, kw.* and kwp.* */
enum uaes_kw_arrangement { UAES_KW_BLOCK = 0, UAES_KW_LDS, UAES_KW_GLOBAL, UAES_KW_BATCH };
int uaesk_plan_kw(int dir, size_t len, size_t nkeys, uaes_plan *p);
const char *uaesk_kw_arrangement_name(int id);

/* AES key wrap with padding (RFC 5649, SP 800-38F KWP; uaes_kw.hip).  dir: 0 wrap, 1 unwrap; len = bytes of the secret
 * for a wrap (1 .. UAES_KWP_MAX, what the 32-bit length indicator can say) and bytes of the wrapped form - 8 for an
 * unwrap (a multiple of 8); nkeys 0 = the one-secret calls, nkeys >= 1 = a batch whose slots hold len bytes (at most
 * UAES_KW_BATCH_MAX).  A padded length of 8 is one block of the cipher and no chain; beyond that the arrangements are
 * key wrap's, decided by the padded length with key wrap's limits.  Returns a HIP error code for a length of 0, an
 * unwrap length that is no multiple of 8, a length beyond the indicator's range or a batch slot above the limit. */
#define UAES_KWP_MAX ((size_t)0xFFFFFFFFu)
int uaesk_plan_kwp(int dir, size_t len, size_t nkeys, uaes_plan *p);
const char *uaesk_kwp_arrangement_name(int id);

/* FF1, SP 800-38G (uaes_ff1.hip).  dir: 0 encrypt, 1 decrypt; len = numerals of one text (one byte each); nrec 0 = the
 * one-text calls, nrec >= 1 = a batch of nrec records of len numerals.  A text is at most UAES_FF1_MAX numerals: the
 * reference takes any length, but the radix conversions are quadratic in it.  A record of a batch is at most
 * UAES_FF1_BATCH_MAX numerals: the largest power of two at which the 64 records of a workgroup keep their numerals,
 * the number NUM(B) / the bytes of S and the digits of S in the 31 KiB of LDS the row4 tables leave (uaes_ff1.hip
 * asserts it).  One text within that limit runs as a batch of one, a longer one on a whole wave.  grid = workgroups,
 * steps = threads per workgroup.  Returns a HIP error code for a radix outside 2..256, a length below the radix's
 * minimum (radix^len >= 1 000 000) or above the limit. */
#define UAES_FF1_MAX       ((size_t)4096)
#define UAES_FF1_BATCH_MAX ((size_t)128)
enum uaes_ff1_arrangement { UAES_FF1_BATCH = 0, UAES_FF1_WAVE };
int uaesk_plan_ff1(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p);
const char *uaesk_ff1_arrangement_name(int id);

/* FF3-1, SP 800-38G revision 1 (uaes_ff3.hip).  dir, len, nrec as for FF1; the tweak is always UAES_FF3_TWEAK bytes.  One
 * arrangement: a text is at most maxlen(radix) = 2 floor(log_radix 2^96) numerals (192 at radix 2, 56 decimal, 24 at
 * radix 256), so the 64 records of a workgroup always fit the LDS the row4 tables leave (uaes_ff3.hip asserts it) and
 * one text is a batch of one.  grid = workgroups, steps = threads per workgroup.  Returns a HIP error code for a dir
 * other than 0 / 1, a radix outside 2..256, a length below the radix's minimum (radix^len >= 1 000 000) or above its
 * maximum. */
#define UAES_FF3_TWEAK 7
enum uaes_ff3_arrangement { UAES_FF3_BATCH = 0 };
int uaesk_plan_ff3(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p);
const char *uaesk_ff3_arrangement_name(int id);

/* The batches of GCM-SIV records (RFC 8452; uaes_gcmsiv_batch.hip).  dir: 0 encrypt, 1 decrypt; len = bytes per record,
 * nmsg = records; one arrangement, a row batch at any number of records.  A record is a serial POLYVAL chain and a
 * serial keystream on sixteen lanes, with a key derivation and a key expansion of its own in front: it is at most
 * UAES_GCMSIV_BATCH_MAX bytes (the same number as UAES_CCM_BATCH_MAX, and the most AAD a record takes); beyond it the
 * one-message arrangements above (SIV_CHUNKS from 32 736 B) are the right tool.  grid = workgroups, steps = threads
 * per workgroup.  Returns a HIP error code for a dir other than 0 / 1 or a length above the limit. */
#define UAES_GCMSIV_BATCH_MAX ((size_t)65535)
enum uaes_gcmsiv_batch_arrangement { UAES_GCMSIV_BATCH = 0 };
int uaesk_plan_gcmsiv_batch(int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_gcmsiv_batch_arrangement_name(int id);

/* The batches of OCB records (RFC 7253; k_ocb_batch, uaes_ocb.hip).  dir: 0 encrypt, 1 decrypt; len = bytes per record,
 * nmsg = records; one arrangement, a row batch at any number of records.  A record is walked by sixteen lanes, two
 * blocks per step: it is at most UAES_OCB_BATCH_MAX bytes (the same number as UAES_CCM_BATCH_MAX and
 * UAES_GCMSIV_BATCH_MAX, and the most AAD a record takes), so that its offsets never need more than L_11; beyond it
 * OCB_SMALL / OCB_RUNS above are the right tool.  grid = workgroups, steps = threads per workgroup.  Returns a HIP
 * error code for a dir other than 0 / 1 or a length above the limit. */
#define UAES_OCB_BATCH_MAX ((size_t)65535)
enum uaes_ocb_batch_arrangement { UAES_OCB_BATCH = 0 };
int uaesk_plan_ocb_batch(int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_ocb_batch_arrangement_name(int id);

/* The batches of GCM records with a key per record (k_gcm_multikey, uaes_gcm_multikey.hip).  dir: 0 encrypt, 1 decrypt;
 * len = bytes per record, nmsg = records; one arrangement, a row batch at any number of records.  A record is a key
 * expansion, a serial hash and a serial keystream on sixteen lanes: it is at most UAES_GCM_MULTIKEY_BATCH_MAX bytes (the
 * same number as the other batch caps, and the most AAD a record takes); beyond it a uaes_gcm_key context per key is the
 * right tool.  A record then has at most 4096 blocks and its counters are J0 + 1 .. J0 + 4096 with J0 = nonce ||
 * 00000001: the 32-bit counter stays below 2^16, so only bytes 14..15 of the counter block ever change (asserted
 * below; the kernel builds the counter's column from them).  grid = workgroups, steps = threads per workgroup.  Returns
 * a HIP error code for a dir other than 0 / 1 or a length above the limit. */
#define UAES_GCM_MULTIKEY_BATCH_MAX ((size_t)65535)
typedef char uaes_gcm_multikey_counter_stays_in_bytes_14_15[(UAES_GCM_MULTIKEY_BATCH_MAX + 15) / 16 + 1 <= 0xFFFF ? 1 : -1];
enum uaes_gcm_multikey_arrangement { UAES_GCM_MULTIKEY = 0 };
int uaesk_plan_gcm_multikey_batch(int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_gcm_multikey_arrangement_name(int id);

/* The batches of XAES-256-GCM records (C2SP; k_xaes_gcm_batch, uaes_xaes.hip).  dir: 0 encrypt, 1 decrypt; len = bytes
 * per record, nmsg = records; one arrangement, a row batch at any number of records.  A record is a key derivation and
 * a key expansion in front of the multi-key batch's record (gcm_row_record, uaes_gcm_row.hip.h), so its cap is that
 * batch's, for the same reason: at most 4096 counter blocks, J0 + 1 .. J0 + 4096 with J0 = N[12:24] || 00000001, and only
 * bytes 14..15 of the counter block ever change (asserted below).  It is also the most AAD a record takes.  grid =
 * workgroups, steps = threads per workgroup.  Returns a HIP error code for a dir other than 0 / 1 or a length above the
 * limit. */
#define UAES_XAES_GCM_BATCH_MAX ((size_t)65535)
typedef char uaes_xaes_gcm_counter_stays_in_bytes_14_15[(UAES_XAES_GCM_BATCH_MAX + 15) / 16 + 1 <= 0xFFFF ? 1 : -1];
enum uaes_xaes_gcm_arrangement { UAES_XAES_GCM = 0 };
int uaesk_plan_xaes_gcm_batch(int dir, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_xaes_gcm_arrangement_name(int id);

/* The batches of the plain cipher modes (k_cipher_batch, uaes_cipher_batch.hip).  mode = enum uaes_cipher_batch_mode;
 * len = bytes per record, nmsg = records; one arrangement, a row batch at any number of records and any record length
 * (the walk over a record counts its blocks in 64 bits, and CTR's counter is the 56-bit one of the one-message call).
 * grid = workgroups, steps = threads per workgroup.  Returns a HIP error code for a mode outside the enum, a CBC record
 * that is not a whole number of blocks (at least one), or a record of the other modes above UINT32_MAX bytes (what a
 * 32-bit length can say). */
enum uaes_cipher_batch_mode { UAES_CB_CBC_DEC = 0, UAES_CB_CBC_DEC_BLOCKS, UAES_CB_CBC_ENC_BLOCKS, UAES_CB_CFB_ENC,
                              UAES_CB_CFB_DEC, UAES_CB_OFB, UAES_CB_CTR, UAES_CB_MODES };
enum uaes_cipher_batch_arrangement { UAES_CIPHER_BATCH = 0 };
int uaesk_plan_cipher_batch(int mode, size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_cipher_batch_arrangement_name(int id);

/* The batches of XTS data units (k_xts_batch, uaes_xts_batch.hip): uaes_xts_encrypt_batch, uaes_xts_decrypt_batch and
 * uaes_xts_sector_list.  len = bytes per unit's slot, nmsg = units; one arrangement, a row batch at any number of units,
 * with an id outside enum uaes_arrangement (uaes_debug_plan_xts_batch names it).  A unit is walked by sixteen lanes, two
 * blocks per step, so a contiguous run of equal sectors stays with the XTS rows above, which spread a unit over many
 * lanes.  grid = workgroups, steps = threads per workgroup.  Returns a HIP error code for a unit below 16 bytes (XTS has
 * none) or above UINT32_MAX (what a 32-bit length can say). */
enum uaes_xts_batch_arrangement { UAES_XTS_BATCH = 0 };
int uaesk_plan_xts_batch(size_t len, size_t nmsg, uaes_plan *p);
const char *uaesk_xts_batch_arrangement_name(int id);

#ifdef __cplusplus
}
#endif
#endif
