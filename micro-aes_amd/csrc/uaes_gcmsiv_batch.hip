/*
 * uaes_gcmsiv_batch.hip -- many short GCM-SIV messages (RFC 8452; GCM_SIV_encrypt / _decrypt, micro_aes.c:1421-1515) under
 * one MASTER key in one launch.
 *
 *   k_gcmsiv_batch   sixteen lanes (a DPP row) per record, four records per wave, on the row4 tables.
 *
 * What sets it apart from every other row batch: both working keys belong to the NONCE, not to the key, so nothing but
 * the tables and the master key's schedule is shared.  Per record the row
 *   1. derives the keys: blocks LE32(i) || nonce, i < 2 + keybits / 64, under the master key (row_encrypt2, in pairs);
 *      the low eight bytes of each are the lanes of columns 0 and 1.  Blocks 0-1 give the message-authentication key H,
 *      the rest the message-encryption key (192 bits: the reference's five blocks, which RFC 8452 does not define);
 *   2. expands that key into the record's own LDS slot behind the tables (GSB_SLOT bytes).  SubWord is one lookup step:
 *      the last-round region holds S[x] in byte r for the lane of row r, so the four lanes of a quad substitute the four
 *      bytes of a word at once and OR them together with two quad permutes.  row4_lane<NR>(slot) then gives the record's
 *      RowLane; the master's is dead by then (it is loaded inside the record loop, in a scope of its own);
 *   3. runs POLYVAL under its own H (below), the tag Enc((S ^ nonce) with bit 127 cleared), and CTR from the tag with
 *      byte 15 |= 0x80, block j adding j to the little-endian word in bytes 0..3 modulo 2^32 (no carry leaves it).
 *      Encrypt needs the tag before the keystream: hash, tag, CTR -- two walks over the text.  Decrypt takes the keystream
 *      from the RECEIVED tag and hashes what it produced in the same walk; like the reference it writes the text before
 *      the tag is known.
 *
 * (gsb_expand and the POLYVAL below are in uaes_perkey.hip.h, which uaes_gcm_multikey.hip shares.)
 *
 * POLYVAL without a table in LDS.  S' = (S ^ X) H x^-128 in GF(2^128) = GF(2)[x] / (x^128 + x^127 + x^126 + x^121 + 1),
 * blocks little-endian (bit j of the polynomial = bit j % 32 of word j / 32: the column words as they are loaded).
 * Lane i of the row owns byte i of the multiplicand S ^ X (byte i % 4 of the column word it holds anyway) and keeps
 *     K_i x^b  =  H x^(8 i - 128 + b)  mod P,   b = 0..7,
 * reduced, in 32 registers, made once per record.  A step is then: eight masks from the lane's byte, 32 masked XORs into
 * four words (an 8 x 128-bit carry-less product that needs no reduction), and the XOR of the sixteen partial products
 * across the row with DPP rotations by 8, 4, 2, 1 -- every lane ends up with the whole of S' and takes the word of its
 * column.  About 95 VALU instructions and no memory access per block; exact, nothing is approximated.
 * The negative powers cost no chain of single-bit steps: P is 1 modulo x^121, so for k <= 120
 *     a x^-k  =  (a ^ (a mod x^k) P) / x^k  =  (a >> k) ^ (a mod x^k) (x^(128-k) + x^(127-k) + x^(126-k) + x^(121-k)),
 * a shift and four shifted copies of the low bits (pv_div32, pv_div8); lane i takes 16 - i byte steps as up to four
 * word steps and three byte steps, all lanes in step.
 *
 * A record costs, in row steps (one row_encrypt or one POLYVAL block each):  2 + keybits / 64 derivation blocks in
 * pairs, the expansion (10 / 8 / 13 serial SubWords), the POLYVAL key, then ceil(aad / 16) + ceil(len / 16) + 1 POLYVAL
 * blocks, one tag block and ceil(len / 16) keystream blocks.
 *
 * gfx950, -O3 (the compiler's resource-usage remark): encrypt 115 / 119 / 123 VGPRs at AES-128 / 192 / 256, decrypt 122 /
 * 126 / 128, 84 to 86 SGPRs, no scratch, no spills in any of the twelve instances (a 16-wave workgroup leaves 128
 * VGPRs a lane).  What it took: the record's RowLane (20 registers) and the 32 of POLYVAL leave room for a text chunk of
 * eight blocks ahead encrypting and four decrypting, where the keystream and the hash share the walk (row_walk's CH;
 * with the sixteen of the other row batches the decrypt kernels spilled 19 to 25 registers), and the nonce is read a
 * second time for the tag's block instead of being kept through the walk.  LDS is dynamic: 146 688 bytes at 1024
 * threads (row4 tables and the master's round keys 131 328, 64 slots of 240), 135 168 at 256 threads.
 * Rates: profiles/gcmsiv_batch_rate.md (tools/gcmsiv_rate.py); DESIGN.md section 5, "GCM-SIV batches".
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_perkey.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

#define GSB_CH        8u                                  /* row_walk's chunk: a step here is a block of the cipher and one of POLYVAL */

static_assert(UAES_GCMSIV_BATCH_MAX <= 0x1fffffffu, "8 len fits the 32-bit word the length block is built from");

/* this lane's column of the block the tag is the encryption of: (S ^ nonce) with bit 127 cleared */
__device__ __forceinline__ u32 gsb_tag_block(u32 s, const unsigned char *np, u32 c)
{
    if (c == 3u) return s & 0x7fffffffu;
#pragma unroll
    for (u32 k = 0; k < 4; ++k) s ^= (u32)np[4u * c + k] << (8u * k);
    return s;
}

/* Record m: text at in / out + m msg_bytes (its first lens[m] <= msg_bytes bytes; lens == NULL: all of it), nonce at
 * nonces + 12 m, AAD at aad + m aad_bytes, tag at tags + 16 m.  mk = the schedule of the MASTER key.  Decrypt:
 * verdicts[m] = 1 if authentic, else 0 and bad[0] |= 1 (a vector atomic), the output left as decrypted or zeroed when
 * `wipe`.  in == out works: encrypt has read the whole record before it stores (and then a block is loaded before it
 * is stored), decrypt loads a block before it stores it.  A row never reads a lane or a slot of another record.
 * A4: text 4-byte aligned. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_gcmsiv_batch(uaesk_rk mk, uaesk_tables tb, int wipe,
                                                          const unsigned char *nonces,
                                                          const unsigned char *aad, u32 aad_bytes,
                                                          u64 nmsg, u32 msg_bytes, const u32 *lens,
                                                          const unsigned char *in, unsigned char *out,
                                                          unsigned char *tags, unsigned char *verdicts, int *bad)
{
    constexpr u32 NK = NR - 6, NB = 2 + NK / 2;
    row4_fill_tables(tb.te0, mk);
    const u32 li = threadIdx.x & 15u, c = li >> 2;
    const u32 slot = UAES_LDS_ROW4 + (threadIdx.x >> 4) * GSB_SLOT;
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u32 len = msg_bytes;
        if (lens) { len = lens[m]; if (len > msg_bytes) len = msg_bytes; }
        const unsigned char *np = nonces + m * 12u;
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        /* the nonce as column words in bytes 4..15 (the derivation blocks); in bytes 0..11 (the tag's block) it is
         * read again when the hash is done, so that it does not occupy a register through the walk */
        u32 nd = 0;
#pragma unroll
        for (u32 k = 0; k < 4; ++k)
            if (c > 0u) nd |= (u32)np[4u * (c - 1u) + k] << (8u * k);
        PvLane V;
        {
            u32 h[4], key[NK];
            {
                const RowLane<NR> M = row4_lane<NR>();           /* the master key's lane: dead after the derivation */
                u32 e[NB];
#pragma unroll
                for (u32 i = 0; i < NB; ++i) e[i] = c == 0u ? i : nd;
#pragma unroll
                for (u32 i = 0; i + 1 < NB; i += 2) row_encrypt2<NR>(e[i], e[i + 1], M, M);
                if (NB & 1u) e[NB - 1] = row_encrypt<NR>(e[NB - 1], M);
#pragma unroll
                for (u32 i = 0; i < 2; ++i) { h[2 * i] = gsb_from_col(e[i], 0); h[2 * i + 1] = gsb_from_col(e[i], 1); }
#pragma unroll
                for (u32 i = 0; i < NK / 2; ++i) { key[2 * i] = gsb_from_col(e[2 + i], 0); key[2 * i + 1] = gsb_from_col(e[2 + i], 1); }
                gsb_expand<NR>(key, slot, li, M.tlast, M.sel, M.lsel);
            }
            pv_lane(V, h, li);
        }
        GSB_PHASE();
        const RowLane<NR> R = row4_lane<NR>(slot);               /* the record's own key */

        const u32 full = len >> 4, rem = len & 15u;
        u32 s = 0;
        for (u32 i = 0; i < aad_bytes; i += 16) s = pv_step(s, row_load(aad + m * aad_bytes + i, aad_bytes - i, c), V, c);
        const u32 lb = c == 0u ? aad_bytes << 3 : c == 2u ? len << 3 : 0u;      /* LE64(8 aad) || LE64(8 len) */
        if (!DEC) {
            row_walk<A4, GSB_CH>(src, full, c, [&](u64, u32 x) { s = pv_step(s, x, V, c); });
            if (rem) s = pv_step(s, row_load(src + 16 * (u64)full, rem, c), V, c);
            s = pv_step(s, lb, V, c);
            const u32 t = row_encrypt<NR>(gsb_tag_block(s, np, c), R);
            const u32 cb = c == 3u ? t | 0x80000000u : t;        /* the counter block: the tag, byte 15 |= 0x80 */
            row_walk<A4, GSB_CH>(src, full, c, [&](u64 i, u32 x) {
                row_store_full<A4>(dst + 16 * i, x ^ row_encrypt<NR>(c == 0u ? t + (u32)i : cb, R), c);
            });
            if (rem) {
                const u32 x = row_load(src + 16 * (u64)full, rem, c);
                row_put(dst + 16 * (u64)full, x ^ row_encrypt<NR>(c == 0u ? t + full : cb, R), rem, c);
            }
            row_put(tags + m * 16u, t, 16u, c);
        } else {
            const u32 rt = row_load(tags + m * 16u, 16u, c);
            const u32 cb = c == 3u ? rt | 0x80000000u : rt;
            row_walk<A4, 4u>(src, full, c, [&](u64 i, u32 x) {
                const u32 y = x ^ row_encrypt<NR>(c == 0u ? rt + (u32)i : cb, R);
                row_store_full<A4>(dst + 16 * i, y, c);
                s = pv_step(s, y, V, c);
            });
            if (rem) {                                           /* the partial last block: zero padded into the hash, cut in the output */
                const u32 x = row_load(src + 16 * (u64)full, rem, c);
                const u32 y = (x ^ row_encrypt<NR>(c == 0u ? rt + full : cb, R)) & row_keep(rem, c);
                row_put(dst + 16 * (u64)full, y, rem, c);
                s = pv_step(s, y, V, c);
            }
            s = pv_step(s, lb, V, c);
            const u32 t = row_encrypt<NR>(gsb_tag_block(s, np, c), R);
            const bool forged = row_any(t != rt);
            row_verdict(li == 0, verdicts, m, !forged, bad);
            if (forged && wipe)
                for (u32 i = 0; i < len; i += 16) row_put(dst + i, 0u, len - i < 16u ? len - i : 16u, c);
        }
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
/* gcmsiv.batch: a row batch at any number of records (uaesk_row_shape) */
extern "C" int uaesk_plan_gcmsiv_batch(int dir, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || len > UAES_GCMSIV_BATCH_MAX) return (int)hipErrorInvalidValue;
    uaesk_row_plan(UAES_GCMSIV_BATCH, nmsg, p);
    return 0;
}

extern "C" const char *uaesk_gcmsiv_batch_arrangement_name(int id)
{
    return id == UAES_GCMSIV_BATCH ? "gcmsiv.batch" : "?";
}

/* ---- launcher -------------------------------------------------------------------------------------------------------- */
template <int NR>
static int launch_gcmsiv_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *mk, int decrypt, int wipe,
                               const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                               const void *lens, const void *in, void *out, void *tags, void *verdicts, int *bad)
{
    uaes_plan p;
    uaesk_row_plan(UAES_GCMSIV_BATCH, nmsg, &p);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_gcmsiv_batch<NR, decltype(DEC)::value, decltype(A4)::value>, p.grid, p.steps, GSB_LDS(p.steps), st,
                            *mk, *tb, wipe, nonces, aad, aad_bytes, nmsg, msg_bytes, lens, in, out, tags, verdicts, bad); }); });
}

extern "C" int uaesk_gcmsiv_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *master_ek, int decrypt, int wipe,
                                  const void *nonces, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                                  const void *lens, const void *in, void *out, void *tags, void *verdicts, int *bad)
{
    if (msg_bytes > UAES_GCMSIV_BATCH_MAX || aad_bytes > UAES_GCMSIV_BATCH_MAX) return (int)hipErrorInvalidValue;
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_gcmsiv_batch<NR>(S(stream), tb, master_ek, decrypt, wipe, nonces, aad, aad_bytes, nmsg,
                                                    msg_bytes, lens, in, out, tags, verdicts, bad)));
    return 0;
}
