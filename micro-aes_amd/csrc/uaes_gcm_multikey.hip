/*
 * uaes_gcm_multikey.hip -- many short GCM records (SP 800-38D; AES_GCM_encrypt / _decrypt, micro_aes.c), EVERY RECORD
 * UNDER A KEY OF ITS OWN, in one launch: the packets of many TLS / QUIC / ESP / SRTP sessions at once.
 *
 *   k_gcm_multikey   sixteen lanes (a DPP row) per record, four records per wave, on the row4 tables.
 *
 * Nothing but the tables is shared: there is no master key, so the kernel fills the tables alone
 * (row4_fill_tables_only) and the records' schedule slots start where the other row batches keep the call's round keys,
 * right behind the tables at 128 KiB.  Per record the row
 *   1. loads the key's NK words into every lane (any byte offset: words when the key is 4-byte aligned, bytes
 *      otherwise) and expands them into the record's own LDS slot (gsb_expand, uaes_perkey.hip.h); row4_lane<NR>(slot)
 *      is then the record's RowLane.  From here on the record is gcm_row_record (uaes_gcm_row.hip.h), which
 *      k_xaes_gcm_batch (uaes_xaes.hip) runs too, behind a key derivation:
 *   2. encrypts the zero block and J0 = nonce || 00000001 together (one row_encrypt2 step): H and the tag's mask EJ0;
 *   3. hashes.  GHASH_H(X_1 ..) = rev(POLYVAL_K(rev(X_1) ..)) with K = mulX(rev(H)) (RFC 8452 appendix A; k_siv_prep
 *      uses the relation in the other direction), so the hash is uaes_perkey.hip.h's POLYVAL in registers, pv_lane over
 *      mulX(rev(H)), fed byte-reversed blocks: the lane of column c needs the byte-swapped word of column 3 - c, which
 *      the lane opposite in the row holds -- one row_mirror DPP move and one v_perm_b32 a block (gmk_rev).  The state
 *      stays in POLYVAL's form throughout; AAD and text tails are zero padded; the length block BE64(8 aad) || BE64(8
 *      len) reversed is LE64(8 len) || LE64(8 aad); the tag is gmk_rev(S) ^ EJ0, its first tagLen bytes;
 *   4. encrypt: ONE walk over the text -- keystream block, store, pv_step on the ciphertext just made -- then the
 *      length block and the tag;
 *   5. decrypt keeps N7 per record, as uaes_gcm_key_decrypt_records does: walk 1 hashes the ciphertext, the row compares
 *      tagLen bytes (row_keep's mask, row_any), row_verdict; walk 2 (CTR and store) runs only for an authentic record,
 *      so a forged record's output slot is untouched.  Two walks because the text may not be written before the tag is
 *      known; the second reads the ciphertext again (a short record: from the cache).
 * The counter blocks are J0 + 1 .. J0 + 4096 at most (UAES_GCM_MULTIKEY_BATCH_MAX, uaes_plan.h): only bytes 14..15 ever
 * change, so block i's column 3 is the byte-swapped i + 2 and columns 0..2 are the nonce's words, one register.
 *
 * A record costs, in row steps (one row_encrypt or one POLYVAL block each): the expansion (10 / 8 / 13 serial
 * SubWords), one step for H and EJ0, the POLYVAL key, then ceil(aad / 16) + ceil(len / 16) + 1 POLYVAL blocks and
 * ceil(len / 16) keystream blocks.
 *
 * gfx950, -O3 (tools/kernel_resources.py, profiles/gcm_multikey_resources.txt): encrypt 110 / 116 / 121 VGPRs at AES-128 /
 * 192 / 256 and 90 SGPRs, decrypt 110 / 112 / 114 and 102 SGPRs, no scratch, no spills in any of the twelve instances (a
 * 16-wave workgroup leaves 128 VGPRs a lane).  The record's RowLane (20 registers) and the 32 of the hash leave room for
 * a text chunk of four blocks ahead where the keystream and the hash share the walk (row_walk's CH: encrypt, as the
 * GCM-SIV decrypt kernel) and eight on either of decrypt's walks; the nonce's word and EJ0 stay in a register each.
 * LDS is dynamic: 146 432 bytes at 1024 threads (row4 tables 131 072, 64 slots of 240), 134 912 at 256 threads.
 * A host key array reaches the device through the lane's scratch and the host layer clears that copy in stream order
 * (gcm_multikey_batch, uaes_engine_modes.c); here a schedule lives only in its LDS slot and in registers.
 * Rates on an MI355X (profiles/gcm_multikey_batch_rate.md, tools/gcm_multikey_rate.py; device-resident arrays and keys, 12
 * bytes of AAD, 16-byte tags, AES-128): 2^10 records of 16 bytes 22.3 us encrypting / 37.3 decrypting as one call; 2^20
 * records of 16 / 64 / 1024 bytes 2.29 / 1.58 / 0.204 G records/s encrypting, 1.84 / 1.35 / 0.211 decrypting.  DESIGN.md
 * section 5, "Multi-key GCM batches".
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_perkey.hip.h"
#include "uaes_gcm_row.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

#define GMK_KEYS_AT   131072u                             /* the slots: where the other row batches keep the call's round keys */
#define GMK_LDS(wg)   (GMK_KEYS_AT + ((wg) / 16u) * GSB_SLOT)

static_assert(GMK_KEYS_AT % 16u == 0 && GMK_LDS(UAES_WG) <= 160u * 1024u, "64 schedules fit behind the row4 tables, 16-byte aligned");
static_assert(UAES_GCM_MULTIKEY_BATCH_MAX <= 0x1fffffffu, "8 len fits the 32-bit word the length block is built from");

/* the NK little-endian words of the key at kp, in every lane */
template <u32 NK>
__device__ __forceinline__ void gmk_load_key(u32 (&key)[NK], const unsigned char *kp)
{
    if ((((uintptr_t)kp) & 3u) == 0) {
#pragma unroll
        for (u32 i = 0; i < NK; ++i) key[i] = ((const u32 *)kp)[i];
    } else {
#pragma unroll
        for (u32 i = 0; i < NK; ++i)
            key[i] = (u32)kp[4u * i] | ((u32)kp[4u * i + 1u] << 8) | ((u32)kp[4u * i + 2u] << 16) | ((u32)kp[4u * i + 3u] << 24);
    }
}

/* Record m: key at keys + 4 NK m, text at in / out + m msg_bytes (its first lens[m] <= msg_bytes bytes; lens == NULL:
 * all of it), nonce at nonces + 12 m, AAD at aad + m aad_bytes, the first tag_len bytes of the tag at tags + m tag_len.
 * Decrypt: verdicts[m] = 1 if authentic, else 0 and bad[0] |= 1 (a vector atomic), and nothing of a forged record is
 * written.  in == out works: a block is loaded before it is stored.  A row never reads a lane or a slot of another
 * record.  A4: text 4-byte aligned. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_gcm_multikey(uaesk_tables tb, u32 tag_len, const unsigned char *keys,
                                                          const unsigned char *nonces,
                                                          const unsigned char *aad, u32 aad_bytes,
                                                          u64 nmsg, u32 msg_bytes, const u32 *lens,
                                                          const unsigned char *in, unsigned char *out,
                                                          unsigned char *tags, unsigned char *verdicts, int *bad)
{
    constexpr u32 NK = NR - 6;
    row4_fill_tables_only(tb.te0);
    __syncthreads();
    const u32 li = threadIdx.x & 15u, c = li >> 2;
    const u32 slot = GMK_KEYS_AT + (threadIdx.x >> 4) * GSB_SLOT;
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u32 len = msg_bytes;
        if (lens) { len = lens[m]; if (len > msg_bytes) len = msg_bytes; }
        const unsigned char *np = nonces + m * 12u;
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        {
            /* SubWord's lane constants: what row4_lane gives a RowLane, before there is a schedule to load one from */
            const u32 r = li & 3u, q = (threadIdx.x >> 4) & 3u;
            const u32 tlast = 65536u + 64u * q + 4u * li, sel = 0x0c020000u | ((4u + r) << 8);
            const u32 lsel = (0x0c0c0c0cu & ~(0xffu << (8u * r))) | ((4u + r) << (8u * r));
            u32 key[NK];
            gmk_load_key<NK>(key, keys + m * (4u * NK));
            gsb_expand<NR>(key, slot, li, tlast, sel, lsel);
        }
        GSB_PHASE();
        gcm_row_record<NR, DEC, A4>(slot, li, c, np, tag_len, aad, aad_bytes, m, len, src, dst, tags, verdicts, bad);
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
/* gcm.multikey: a row batch at any number of records (uaesk_row_shape) */
extern "C" int uaesk_plan_gcm_multikey_batch(int dir, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || len > UAES_GCM_MULTIKEY_BATCH_MAX) return (int)hipErrorInvalidValue;
    uaesk_row_plan(UAES_GCM_MULTIKEY, nmsg, p);
    return 0;
}

extern "C" const char *uaesk_gcm_multikey_arrangement_name(int id)
{
    return id == UAES_GCM_MULTIKEY ? "gcm.multikey" : "?";
}

/* ---- launcher -------------------------------------------------------------------------------------------------------- */
template <int NR>
static int launch_gcm_multikey(hipStream_t st, const uaesk_tables *tb, int decrypt, size_t tag_len, const void *keys,
                               const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                               const void *lens, const void *in, void *out, void *tags, void *verdicts, int *bad)
{
    uaes_plan p;
    uaesk_row_plan(UAES_GCM_MULTIKEY, nmsg, &p);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_gcm_multikey<NR, decltype(DEC)::value, decltype(A4)::value>, p.grid, p.steps, GMK_LDS(p.steps), st,
                            *tb, tag_len, keys, nonces, aad, aad_bytes, nmsg, msg_bytes, lens, in, out, tags, verdicts, bad); }); });
}

extern "C" int uaesk_gcm_multikey_batch(void *stream, const uaesk_tables *tb, int nr, int decrypt, size_t tag_len,
                                        const void *keys, const void *nonces, const void *aad, size_t aad_bytes,
                                        size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out,
                                        void *tags, void *verdicts, int *bad)
{
    if (msg_bytes > UAES_GCM_MULTIKEY_BATCH_MAX || aad_bytes > UAES_GCM_MULTIKEY_BATCH_MAX || tag_len < 1 || tag_len > 16)
        return (int)hipErrorInvalidValue;
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_gcm_multikey<NR>(S(stream), tb, decrypt, tag_len, keys, nonces, aad, aad_bytes, nmsg,
                                                    msg_bytes, lens, in, out, tags, verdicts, bad)));
    return 0;
}
