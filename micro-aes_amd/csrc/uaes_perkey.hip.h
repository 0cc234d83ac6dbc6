/*
 * uaes_perkey.hip.h -- what a row batch needs when every record works under keys of its own: k_gcmsiv_batch
 * (uaes_gcmsiv_batch.hip; both keys belong to the nonce) and k_gcm_multikey (uaes_gcm_multikey.hip; the key belongs to
 * the record).  Sixteen lanes per record on the row4 tables (uaes_aes.hip.h):
 *   gsb_expand         KeyExpansion in registers into the record's own LDS slot behind the tables (GSB_SLOT bytes), with
 *                      SubWord as one lookup step of the quad (gsb_subword);
 *   PvLane, pv_lane, pv_step
 *                      GF(2^128) products under the record's own hash key without a table: POLYVAL's form, 32 registers
 *                      a lane, about 95 VALU instructions a block, exact.
 * The derivations are in uaes_gcmsiv_batch.hip's header comment, where this code was written and measured.
 */
#ifndef UAES_PERKEY_HIP_H
#define UAES_PERKEY_HIP_H

#include "uaes_aes.hip.h"

#define GSB_SLOT      240u                                /* a record's key schedule: 16 (NR + 1) bytes at NR = 14 */
#define GSB_LDS(wg)   (UAES_LDS_ROW4 + ((wg) / 16u) * GSB_SLOT)

static_assert(16u * (14u + 1u) <= GSB_SLOT && GSB_SLOT % 16u == 0 && UAES_LDS_ROW4 % 16u == 0, "a slot holds any schedule, 16-byte aligned");
static_assert(GSB_LDS(UAES_WG) <= 160u * 1024u, "64 records share a workgroup: their schedules fit behind the row4 tables");

typedef u32 __attribute__((ext_vector_type(4))) gsb_u32x4;
typedef __attribute__((address_space(3))) gsb_u32x4 lds_u32x4;

/* between two phases: what the row's first lane stored is what the row reads next (one wave: its LDS operations
 * complete in order) */
#define GSB_PHASE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

/* ---- GF(2^128), POLYVAL's own form: w[0] holds x^0..x^31 ------------------------------------------------------------ */
__device__ __forceinline__ void pv_div32(u32 (&a)[4])       /* a x^-32 mod P */
{
    const u32 q = a[0];
    a[0] = a[1];
    a[1] = a[2];
    a[2] = a[3] ^ (q << 31) ^ (q << 30) ^ (q << 25);
    a[3] = q ^ (q >> 1) ^ (q >> 2) ^ (q >> 7);
}

__device__ __forceinline__ void pv_div8(u32 (&a)[4])        /* a x^-8 mod P */
{
    const u32 q = a[0] & 0xffu;
    a[0] = (a[0] >> 8) | (a[1] << 24);
    a[1] = (a[1] >> 8) | (a[2] << 24);
    a[2] = (a[2] >> 8) | (a[3] << 24);
    a[3] = (a[3] >> 8) ^ (q << 24) ^ (q << 23) ^ (q << 22) ^ (q << 17);
}

__device__ __forceinline__ void pv_mulx(const u32 (&a)[4], u32 (&r)[4])     /* r = a x mod P */
{
    const u32 carry = a[3] >> 31;
    r[3] = ((a[3] << 1) | (a[2] >> 31)) ^ ((0u - carry) & 0xC2000000u);
    r[2] = (a[2] << 1) | (a[1] >> 31);
    r[1] = (a[1] << 1) | (a[0] >> 31);
    r[0] = (a[0] << 1) ^ carry;
}

/* what a lane keeps of the record's H: kb[b] = H x^(8 li - 128 + b), and the shift that brings its byte down */
struct PvLane {
    u32 kb[8][4];
    u32 sh;
};

__device__ __forceinline__ void pv_lane(PvLane &V, const u32 (&h)[4], u32 li)
{
    const u32 n = 16u - li, nw = n >> 2, nb = n & 3u;           /* 16 - li bytes down: nw words and nb bytes */
    u32 k[4] = { h[0], h[1], h[2], h[3] };
#pragma unroll
    for (u32 t = 0; t < 4; ++t) {
        u32 d[4] = { k[0], k[1], k[2], k[3] };
        pv_div32(d);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) k[j] = t < nw ? d[j] : k[j];
    }
#pragma unroll
    for (u32 t = 0; t < 3; ++t) {
        u32 d[4] = { k[0], k[1], k[2], k[3] };
        pv_div8(d);
#pragma unroll
        for (u32 j = 0; j < 4; ++j) k[j] = t < nb ? d[j] : k[j];
    }
#pragma unroll
    for (u32 j = 0; j < 4; ++j) V.kb[0][j] = k[j];
#pragma unroll
    for (u32 b = 1; b < 8; ++b) pv_mulx(V.kb[b - 1], V.kb[b]);
    V.sh = 8u * (li & 3u);
}

/* s = this lane's column word of S, x = the same of the next block -> the same of (S ^ X) H x^-128 */
__device__ __forceinline__ u32 pv_step(u32 s, u32 x, const PvLane &V, u32 c)
{
    const u32 a = (s ^ x) >> V.sh;                              /* the lane's byte in bits 0..7 */
    u32 acc[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (u32 b = 0; b < 8; ++b) {
        const u32 m = (u32)((int)(a << (31u - b)) >> 31);       /* bit b of the byte, in every bit */
#pragma unroll
        for (u32 j = 0; j < 4; ++j) acc[j] ^= m & V.kb[b][j];
    }
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        acc[j] ^= row_dpp<0x128>(acc[j]);                       /* row_ror:8 */
        acc[j] ^= row_dpp<0x124>(acc[j]);                       /* row_ror:4 */
        acc[j] ^= row_dpp<0x122>(acc[j]);                       /* row_ror:2 */
        acc[j] ^= row_dpp<0x121>(acc[j]);                       /* row_ror:1: the sum of the sixteen, in every lane */
    }
    return row_pick(acc, c);
}

/* SubWord(t) in every lane of the quad: lane r looks byte r up in the last-round region (S[x] in byte r) */
__device__ __forceinline__ u32 gsb_subword(u32 t, u32 tlast, u32 sel, u32 lsel)
{
    u32 s = __builtin_amdgcn_perm(lds_word(__builtin_amdgcn_perm(t, tlast, sel)), 0u, lsel);
    s |= row_dpp<0xB1>(s);                                      /* quad_perm:[1,0,3,2] */
    s |= row_dpp<0x4E>(s);                                      /* quad_perm:[2,3,0,1] */
    return s;
}

/* KeyExpansion (micro_aes.c:144-178) of the NK key words every lane holds, into the 16 (NR + 1) bytes at LDS address
 * slot.  The schedule grows in registers (fully unrolled: constant indices); the row's first lane stores each round
 * key as it completes. */
template <int NR>
__device__ __forceinline__ void gsb_expand(const u32 *key, u32 slot, u32 li, u32 tlast, u32 sel, u32 lsel)
{
    constexpr u32 NK = NR - 6;
    u32 w[4 * (NR + 1)];
#pragma unroll
    for (u32 i = 0; i < NK; ++i) w[i] = key[i];
    u32 rcon = 1;
#pragma unroll
    for (u32 i = NK; i < 4u * (NR + 1); ++i) {
        u32 t = w[i - 1];
        if (i % NK == 0) {
            t = gsb_subword((t >> 8) | (t << 24), tlast, sel, lsel) ^ rcon;      /* RotWord on little-endian words */
            rcon = ((rcon << 1) ^ ((rcon >> 7) * 0x1bu)) & 0xffu;
        } else if (NK == 8 && i % NK == 4) {
            t = gsb_subword(t, tlast, sel, lsel);
        }
        w[i] = w[i - NK] ^ t;
    }
    if (li == 0) {
#pragma unroll
        for (u32 j = 0; j <= (u32)NR; ++j)
            *(lds_u32x4 *)(uintptr_t)(slot + 16u * j) = gsb_u32x4{ w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3] };
    }
}

/* a value the lanes of column `col` hold, in every lane of the row */
__device__ __forceinline__ u32 gsb_from_col(u32 v, u32 col)
{
    return (u32)__shfl((int)v, (int)(4u * col), 16);
}

#endif
