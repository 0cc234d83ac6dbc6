/*
 * uaes_gcm_row.hip.h -- GCM (SP 800-38D) of ONE record on a row of sixteen lanes, under a key schedule that the row has
 * just expanded into its own LDS slot: the record body that k_gcm_multikey (uaes_gcm_multikey.hip; the key belongs to
 * the record) and k_xaes_gcm_batch (uaes_xaes.hip; the key is derived from the first half of the record's nonce) share.
 * The caller fills the row4 tables, expands the record's key (gsb_expand, uaes_perkey.hip.h), waits for the slot
 * (GSB_PHASE) and calls gcm_row_record; what the record then does, why the hash runs in POLYVAL's form and what it
 * costs in registers is in uaes_gcm_multikey.hip's header comment, where this code was written and measured.
 */
#ifndef UAES_GCM_ROW_HIP_H
#define UAES_GCM_ROW_HIP_H

#include "uaes_aes.hip.h"
#include "uaes_perkey.hip.h"

#define GMK_CH_ENC    4u                                  /* row_walk's chunk where a step is a block of the cipher and one of the hash */
#define GMK_CH_HASH   8u                                  /* decrypt's walk 1: a block of the hash */
#define GMK_CH_CTR    8u                                  /* decrypt's walk 2: a block of the cipher */

/* the byte-reversed block: this lane's column word of it, from the column words the row holds (lane 15 - i is a lane
 * of column 3 - c) */
__device__ __forceinline__ u32 gmk_rev(u32 w)
{
    return __builtin_amdgcn_perm(0u, row_dpp<0x140>(w), 0x00010203u);       /* row_mirror, then the four bytes swapped */
}

/* this lane's column of the counter block of text block i: J0 + 1 + i (nw = the nonce's word of columns 0..2) */
__device__ __forceinline__ u32 gmk_ctr(u32 nw, u32 i, u32 c)
{
    return c == 3u ? __builtin_bswap32(i + 2u) : nw;
}

/* Record m under the schedule at LDS address slot: its 12-byte nonce at np, its first len bytes at src / dst, its AAD
 * at aad + m aad_bytes, the first tag_len bytes of its tag at tags + m tag_len.  At most 65535 bytes of text: the
 * counter blocks are J0 + 1 .. J0 + 4096, only bytes 14..15 change.  Decrypt: verdicts[m] = 1 if authentic, else 0 and
 * bad[0] |= 1 (a vector atomic), and nothing of a forged record is written.  src == dst works: a block is loaded
 * before it is stored.  li = the lane's place in its row, c = li / 4 its column.  A4: text 4-byte aligned.  VOPT: verdicts
 * may be NULL (row_verdict's OPTIONAL). */
template <int NR, bool DEC, bool A4, bool VOPT = false>
__device__ __forceinline__ void gcm_row_record(u32 slot, u32 li, u32 c, const unsigned char *np, u32 tag_len,
                                               const unsigned char *aad, u32 aad_bytes, u64 m, u32 len,
                                               const unsigned char *src, unsigned char *dst,
                                               unsigned char *tags, unsigned char *verdicts, int *bad)
{
    const RowLane<NR> R = row4_lane<NR>(slot);               /* the record's own key */
    u32 nw = 0;                                              /* the nonce's word of this column; column 3 has none */
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        if (c < 3u) nw |= (u32)np[4u * c + k] << (8u * k);
    u32 ej0 = c == 3u ? 0x01000000u : nw;                    /* J0 = nonce || 00000001 */
    PvLane V;
    {
        u32 h = 0, hr[4], hk[4];
        row_encrypt2<NR>(h, ej0, R, R);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) hr[j] = __builtin_bswap32(gsb_from_col(h, 3u - j));      /* rev(H), little-endian words */
        pv_mulx(hr, hk);
        pv_lane(V, hk, li);
    }

    const u32 full = len >> 4, rem = len & 15u;
    u32 s = 0;
    for (u32 i = 0; i < aad_bytes; i += 16) s = pv_step(s, gmk_rev(row_load(aad + m * aad_bytes + i, aad_bytes - i, c)), V, c);
    const u32 lb = c == 0u ? len << 3 : c == 2u ? aad_bytes << 3 : 0u;      /* rev(BE64(8 aad) || BE64(8 len)) */
    if (!DEC) {
        row_walk<A4, GMK_CH_ENC>(src, full, c, [&](u64 i, u32 x) {
            const u32 y = x ^ row_encrypt<NR>(gmk_ctr(nw, (u32)i, c), R);
            row_store_full<A4>(dst + 16 * i, y, c);
            s = pv_step(s, gmk_rev(y), V, c);
        });
        if (rem) {                                           /* the partial last block: cut, then zero padded into the hash */
            const u32 x = row_load(src + 16 * (u64)full, rem, c);
            const u32 y = (x ^ row_encrypt<NR>(gmk_ctr(nw, full, c), R)) & row_keep(rem, c);
            row_put(dst + 16 * (u64)full, y, rem, c);
            s = pv_step(s, gmk_rev(y), V, c);
        }
        s = pv_step(s, lb, V, c);
        row_put(tags + m * tag_len, gmk_rev(s) ^ ej0, tag_len, c);
    } else {
        row_walk<A4, GMK_CH_HASH>(src, full, c, [&](u64, u32 x) { s = pv_step(s, gmk_rev(x), V, c); });
        if (rem) s = pv_step(s, gmk_rev(row_load(src + 16 * (u64)full, rem, c)), V, c);
        s = pv_step(s, lb, V, c);
        const u32 t = gmk_rev(s) ^ ej0, rt = row_load(tags + m * tag_len, tag_len, c);
        const bool forged = row_any(((t ^ rt) & row_keep(tag_len, c)) != 0u);
        row_verdict<VOPT>(li == 0, verdicts, m, !forged, bad);
        if (!forged) {
            row_walk<A4, GMK_CH_CTR>(src, full, c, [&](u64 i, u32 x) {
                row_store_full<A4>(dst + 16 * i, x ^ row_encrypt<NR>(gmk_ctr(nw, (u32)i, c), R), c);
            });
            if (rem) {
                const u32 x = row_load(src + 16 * (u64)full, rem, c);
                row_put(dst + 16 * (u64)full, x ^ row_encrypt<NR>(gmk_ctr(nw, full, c), R), rem, c);
            }
        }
    }
}

#endif
