/*
 * uaes_xaes.hip -- many short XAES-256-GCM records (C2SP, c2sp.org/XAES-256-GCM: AES-256-GCM with a 192-bit nonce)
 * under one MASTER key in one launch.
 *
 *   k_xaes_gcm_batch   sixteen lanes (a DPP row) per record, four records per wave, on the row4 tables.
 *
 * XAES-256-GCM(K, N) is AES-256-GCM(Kx, N[12:24]) with Kx = CMAC_K(00 01 58 00 || N[0:12]) || CMAC_K(00 02 58 00 ||
 * N[0:12]), the SP 800-108 counter-mode derivation.  Both messages are one whole block, so each CMAC is one block of
 * the cipher over the message XORed with CMAC's first subkey K1 = 2 AES_K(0^128) in GF(2^128).  K1 belongs to the
 * call, not to the record: the host computes it once (xaes_k1, uaes_engine_gcm.c) and it travels by value next to
 * the master's schedule.  So a record is a GCM-SIV batch's "derive and expand a key per record" in front of the
 * multi-key GCM batch's record body, and the kernel is exactly that, in k_gcmsiv_batch's slot layout.  Per record the row
 *   1. derives: in a scope of its own it loads the master's RowLane, builds this lane's column of M1 ^ K1 and M2 ^ K1
 *      (column 0 is the constant 00 0i 58 00, columns 1..3 the first twelve nonce bytes, read bytewise: a record's
 *      nonce starts at any address) and encrypts both in ONE row_encrypt2 step: the two halves of Kx;
 *   2. expands: the eight key words are gathered into every lane (gsb_from_col) and gsb_expand<14> writes the schedule
 *      into the record's LDS slot behind the tables and the master's round keys.  The master's RowLane is dead from here;
 *   3. runs GCM: gcm_row_record (uaes_gcm_row.hip.h), the body k_gcm_multikey runs, with the nonce pointer at the
 *      second twelve bytes and a 16-byte tag.  Decrypt hashes first and writes an authentic record only.
 * Kx exists in the slot and in registers only; nothing of it reaches memory.
 *
 * A record costs, in row steps: one two-block step for Kx, the expansion (13 serial SubWords), one step for H and EJ0,
 * the POLYVAL key, then ceil(aad / 16) + ceil(len / 16) + 1 POLYVAL blocks and ceil(len / 16) keystream blocks: one
 * two-block step more than a record of k_gcm_multikey<14>, and a 24-byte nonce in place of a 32-byte key load.
 *
 * NR is 14 throughout: four instances.  gfx950, -O3 (tools/kernel_resources.py, profiles/xaes_gcm_resources.txt): no
 * scratch and no spills in any of them at 1024 threads; LDS is dynamic, GSB_LDS: 146 688 bytes at 1024 threads, as
 * k_gcmsiv_batch.  Rates on an MI355X (profiles/xaes_gcm_batch_rate.md, tools/gcm_multikey_rate.py --xaes; device-resident
 * arrays, 12 bytes of AAD): 2^20 records of 16 / 64 / 1024 bytes 1.80 / 1.29 / 0.176 G records/s encrypting, 1.53 / 1.13 /
 * 0.187 decrypting; 1.14 .. 1.01 times the time of k_gcm_multikey<14> on the same texts.  DESIGN.md section 5,
 * "XAES-256-GCM batches".
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_perkey.hip.h"
#include "uaes_gcm_row.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

static_assert(UAES_XAES_GCM_BATCH_MAX <= 0x1fffffffu, "8 len fits the 32-bit word the length block is built from");

/* Record m: text at in / out + m msg_bytes (its first lens[m] <= msg_bytes bytes; lens == NULL: all of it), nonce at
 * nonces + 24 m, AAD at aad + m aad_bytes, tag at tags + 16 m.  mk = the schedule of the MASTER key, k1 = CMAC's first
 * subkey under it as little-endian column words.  Decrypt: verdicts[m] = 1 if authentic, else 0 (verdicts may be NULL)
 * and bad[0] |= 1, and nothing of a forged record is written.  in == out works.  A row never reads a lane or a slot of
 * another record.  A4: text 4-byte aligned. */
template <bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_xaes_gcm_batch(uaesk_rk mk, uaesk_block k1, uaesk_tables tb,
                                                            const unsigned char *nonces,
                                                            const unsigned char *aad, u32 aad_bytes,
                                                            u64 nmsg, u32 msg_bytes, const u32 *lens,
                                                            const unsigned char *in, unsigned char *out,
                                                            unsigned char *tags, unsigned char *verdicts, int *bad)
{
    constexpr int NR = 14;
    row4_fill_tables(tb.te0, mk);
    const u32 li = threadIdx.x & 15u, c = li >> 2;
    const u32 slot = UAES_LDS_ROW4 + (threadIdx.x >> 4) * GSB_SLOT;
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u32 len = msg_bytes;
        if (lens) { len = lens[m]; if (len > msg_bytes) len = msg_bytes; }
        const unsigned char *np = nonces + m * 24u;
        {
            const RowLane<NR> M = row4_lane<NR>();               /* the master key's lane: dead after the derivation */
            u32 nd = 0;                                          /* the first nonce half as column words in bytes 4..15 */
#pragma unroll
            for (u32 k = 0; k < 4; ++k)
                if (c > 0u) nd |= (u32)np[4u * (c - 1u) + k] << (8u * k);
            const u32 kc = row_pick(k1.w, c);
            u32 a = (c == 0u ? 0x00580100u : nd) ^ kc;           /* 00 01 58 00 || N[0:12], ^ K1 */
            u32 b = (c == 0u ? 0x00580200u : nd) ^ kc;           /* 00 02 58 00 || N[0:12], ^ K1 */
            row_encrypt2<NR>(a, b, M, M);
            u32 key[8];
#pragma unroll
            for (u32 j = 0; j < 4; ++j) { key[j] = gsb_from_col(a, j); key[4 + j] = gsb_from_col(b, j); }
            gsb_expand<NR>(key, slot, li, M.tlast, M.sel, M.lsel);
        }
        GSB_PHASE();
        gcm_row_record<NR, DEC, A4, true>(slot, li, c, np + 12, 16u, aad, aad_bytes, m, len, in + m * msg_bytes,
                                          out + m * msg_bytes, tags, verdicts, bad);
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
/* xaes.gcm: a row batch at any number of records (uaesk_row_shape) */
extern "C" int uaesk_plan_xaes_gcm_batch(int dir, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || len > UAES_XAES_GCM_BATCH_MAX) return (int)hipErrorInvalidValue;
    uaesk_row_plan(UAES_XAES_GCM, nmsg, p);
    return 0;
}

extern "C" const char *uaesk_xaes_gcm_arrangement_name(int id)
{
    return id == UAES_XAES_GCM ? "xaes.gcm" : "?";
}

/* ---- launcher -------------------------------------------------------------------------------------------------------- */
extern "C" int uaesk_xaes_gcm_batch(void *stream, const uaesk_tables *tb, const uaesk_rk *master_ek, const uaesk_block *k1,
                                    int decrypt, const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg,
                                    size_t msg_bytes, const void *lens, const void *in, void *out, void *tags,
                                    void *verdicts, int *bad)
{
    uaes_plan p;
    if (msg_bytes > UAES_XAES_GCM_BATCH_MAX || aad_bytes > UAES_XAES_GCM_BATCH_MAX) return (int)hipErrorInvalidValue;
    if (nmsg == 0) return 0;
    uaesk_row_plan(UAES_XAES_GCM, nmsg, &p);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_xaes_gcm_batch<decltype(DEC)::value, decltype(A4)::value>, p.grid, p.steps, GSB_LDS(p.steps), S(stream),
                            *master_ek, *k1, *tb, nonces, aad, aad_bytes, nmsg, msg_bytes, lens, in, out, tags, verdicts, bad); }); });
}
