/*
 * uaes_eax_siv.hip -- the two CMAC-based AEADs:
 *
 *   EAX            <- AES_EAX_encrypt / AES_EAX_decrypt (micro_aes.c:1560-1648), oMac :1531-1548
 *   SIV (RFC 5297) <- AES_SIV_encrypt / AES_SIV_decrypt (:1373-1411), S2V :1323-1361
 *
 * The kernels here are called s2v / eax; `siv` in kernel and plan names means GCM-SIV (uaes_siv.hip).
 *
 * Both modes are CMAC chains plus a CTR pass with the reference's 56-bit increment (incBlock, :421-427).  A chain is
 * serial, so a call costs at least its longest chain; the reference runs its chains one after another, but most of
 * them are independent:
 *   EAX encrypt   N = OMAC_0(nonce) and H = OMAC_1(aad) at the same time, then CTR(N), then C = OMAC_2(ciphertext)
 *   EAX decrypt   N, H and C = OMAC_2(ciphertext) all at the same time; the tag is checked before anything is written
 *   S2V           the AAD chain (Y) and the plaintext's leading blocks at the same time; only the last one or two
 *                 blocks ("xorend") wait for Y
 * Each chain is one wave (sixteen lanes per block, row_encrypt in uaes_aes.hip.h); chains of one call are waves of
 * one workgroup, on different SIMDs.
 *
 *   k_eax_small / k_s2v_small   one launch, one workgroup: chains, then CTR over all 64 rows of the workgroup
 *                               (text <= UAES_EAX_SIV_SMALL_MAX, uaes_plan.h)
 *   k_eax_macs / k_s2v_macs     the chains of a longer message in one launch; the counter block and the verdict go
 *                               back to the host, which runs the existing positioned CTR kernels (uaesk_ctr_xcrypt)
 *   k_eax_batch / k_s2v_batch   nmsg records under one key, sixteen lanes per record (as k_chain_batch_row)
 *
 * EAX' (the reference built with EAXP 1, :1523-1648) has kernels of its own on the same frame, k_eaxp_small /
 * k_eaxp_macs / k_eaxp_batch: see its section below.
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_ctr.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

/* LDS behind the row tables (row_fill_tables: keys at 64 KiB; row4_fill_tables: keys at 128 KiB): a second key
 * schedule (SIV's K_ctr) and four exchange blocks between the waves */
#define ER_KEY2   (65536u + 256u)
#define ER_XCH    (65536u + 512u)
#define ER_LDS    (65536u + 512u + 64u)
#define E4_KEY2   (131072u + 256u)
#define E4_XCH    (131072u + 512u)
#define E4_LDS    (131072u + 512u + 64u)
#define SMALL_WG  1024u

/* ---- block helpers: a block is held as the four column words of a DPP row ------------------------------------- */

/* the block whose column words the sixteen lanes of this lane's row hold, in every lane of the row */
__device__ __forceinline__ void row_gather(u32 w, u32 (&b)[4])
{
    const int base = (int)(threadIdx.x & 48u);
    b[0] = (u32)__shfl((int)w, base + 0);
    b[1] = (u32)__shfl((int)w, base + 4);
    b[2] = (u32)__shfl((int)w, base + 8);
    b[3] = (u32)__shfl((int)w, base + 12);
}

/* big-endian doubling in GF(2^128) (doubleBblock :434-444) */
__device__ __forceinline__ void dbl_be(u32 (&b)[4])
{
    u64 hi = ((u64)bswap32(b[0]) << 32) | bswap32(b[1]);
    u64 lo = ((u64)bswap32(b[2]) << 32) | bswap32(b[3]);
    const u64 carry = hi >> 63;
    hi = (hi << 1) | (lo >> 63);
    lo = (lo << 1) ^ (carry ? 0x87ull : 0ull);
    b[0] = bswap32((u32)(hi >> 32)); b[1] = bswap32((u32)hi);
    b[2] = bswap32((u32)(lo >> 32)); b[3] = bswap32((u32)lo);
}

/* the 56-bit counter of a counter block every lane holds (bytes 9..15 big-endian, N2) */
__device__ __forceinline__ uaesk_ctr ctr_of(const u32 (&b)[4])
{
    uaesk_ctr c;
    c.w0 = b[0];
    c.w1 = b[1];
    c.b8 = b[2] & 0xffu;
    c.v0 = ((u64)(bswap32(b[2]) & 0xffffffu) << 32) | bswap32(b[3]);
    c.le32 = 0; c.w2 = 0; c.w3 = 0;
    return c;
}

__device__ __forceinline__ u32 ctr_col(const uaesk_ctr &ctr, u64 i, u32 c)
{
    u32 w[4];
    ctr_words(ctr, i, w);
    return row_pick(w, c);
}

/* this lane's column of the 10* padding byte at position s (< 16) of a block */
__device__ __forceinline__ u32 pad_col(u32 s, u32 c)
{
    return (s >> 2) == c ? 0x80u << (8u * (s & 3u)) : 0u;
}

/* K1 = 2 Enc(0), K2 = 4 Enc(0) (getSubkeys :593-605): this lane's columns */
template <int NR>
__device__ __forceinline__ void cmac_subkeys(const RowLane<NR> &L, u32 &k1c, u32 &k2c)
{
    u32 b[4];
    row_gather(row_encrypt<NR>(0u, L), b);
    dbl_be(b);
    k1c = row_pick(b, L.c);
    dbl_be(b);
    k2c = row_pick(b, L.c);
}

/* ---- chains ----------------------------------------------------------------------------------------------------- */

/* m <- Enc(m ^ X_i) over nblk whole blocks at p (CH: row_walk's chunk; k_s2v_batch_v, short of registers, asks for 8) */
template <int NR, u32 CH = ROW_CH>
__device__ __forceinline__ u32 cbc_blocks(u32 m, const unsigned char *p, u64 nblk, const RowLane<NR> &L)
{
    if ((((uintptr_t)p) & 3u) == 0) row_walk<true, CH>(p, nblk, L.c, [&](u64, u32 x) { m = row_encrypt<NR>(m ^ x, L); });
    else row_walk<false, CH>(p, nblk, L.c, [&](u64, u32 x) { m = row_encrypt<NR>(m ^ x, L); });
    return m;
}

/* the CMAC chain continued over len >= 1 bytes at p: whole blocks, then the last one with K1, or 10* and K2 (cMac :576-590) */
template <int NR, u32 CH = ROW_CH>
__device__ __forceinline__ u32 cmac_more(u32 m, const unsigned char *p, u64 len, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    const u32 s = (u32)((len - 1) % 16) + 1;
    const u64 full = (len - s) / 16;
    m = cbc_blocks<NR, CH>(m, p, full, L);
    u32 l = row_load(p + 16 * full, s, L.c);
    l ^= s < 16 ? pad_col(s, L.c) ^ k2c : k1c;
    return row_encrypt<NR>(m ^ l, L);
}

/* OMAC^t(p) = CMAC([t]_16 || p); an empty p gives CMAC([t]_16) (oMac :1531-1548) */
template <int NR>
__device__ __forceinline__ u32 omac(u32 t, const unsigned char *p, u64 len, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    const u32 tc = L.c == 3u ? t << 24 : 0u;
    if (!len) return row_encrypt<NR>(tc ^ k1c, L);
    return cmac_more<NR>(row_encrypt<NR>(tc, L), p, len, L, k1c, k2c);
}

/* S2V's header: Y = dbl(CMAC(0^128)) ^ CMAC(aad); no AAD at all is no header unit: Y = CMAC(0^128) (:1333-1344) */
template <int NR>
__device__ __forceinline__ u32 s2v_head(const unsigned char *aad, u64 aad_len, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    const u32 y = row_encrypt<NR>(k1c, L);                   /* CMAC of one zero block = Enc(K1) */
    if (!aad_len) return y;
    u32 b[4];
    row_gather(y, b);
    dbl_be(b);
    return row_pick(b, L.c) ^ cmac_more<NR>(0u, aad, aad_len, L, k1c, k2c);
}

/* whole blocks of the text that S2V chains before it needs Y: all but the last one or two (the last 16 bytes) */
__device__ __forceinline__ u64 s2v_lead(u64 len)
{
    return len >= 16 ? len / 16 - 1 : 0;
}

/* y shifted r bytes up (ya: byte j <- y[j - r]) and the r bytes that fall out (yb: byte j <- y[16 - r + j]), 0 < r < 16 */
__device__ __forceinline__ void xorend_split(const u32 (&y)[4], u32 r, u32 (&ya)[4], u32 (&yb)[4])
{
    const u64 lo = (u64)y[0] | ((u64)y[1] << 32), hi = (u64)y[2] | ((u64)y[3] << 32);
    const u32 sh = 8u * r, sb = 128u - sh;
    u64 alo, ahi, blo, bhi;
    if (sh >= 64) { ahi = lo << (sh - 64); alo = 0; }
    else          { ahi = (hi << sh) | (lo >> (64 - sh)); alo = lo << sh; }
    if (sb >= 64) { blo = hi >> (sb - 64); bhi = 0; }
    else          { blo = (lo >> sb) | (hi << (64 - sb)); bhi = hi >> sb; }
    ya[0] = (u32)alo; ya[1] = (u32)(alo >> 32); ya[2] = (u32)ahi; ya[3] = (u32)(ahi >> 32);
    yb[0] = (u32)blo; yb[1] = (u32)(blo >> 32); yb[2] = (u32)bhi; yb[3] = (u32)(bhi >> 32);
}

/* the end of S2V once Y is known (:1345-1360).  m = the chain over the s2v_lead() blocks; pa = this lane's column of
 * the last whole block, pb = of the zero-padded partial tail (len < 16: of the whole text).
 *   len < 16:       V = Enc(dbl(Y) ^ pad(P) ^ K1)
 *   len % 16 == 0:  V = Enc(m ^ P_last ^ Y ^ K1)
 *   otherwise:      Y is XORed into the last 16 bytes, which span the last whole block and the tail (the K[0] + r trick) */
template <int NR>
__device__ __forceinline__ u32 s2v_finish(u32 m, u64 len, u32 pa, u32 pb, u32 y, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    u32 b[4];
    row_gather(y, b);
    if (len < 16) {
        dbl_be(b);
        return row_encrypt<NR>(row_pick(b, L.c) ^ pb ^ pad_col((u32)len, L.c) ^ k1c, L);
    }
    const u32 r = (u32)(len % 16);
    if (!r) return row_encrypt<NR>(m ^ pa ^ y ^ k1c, L);
    u32 ya[4], yb[4];
    xorend_split(b, r, ya, yb);
    m = row_encrypt<NR>(m ^ pa ^ row_pick(ya, L.c), L);
    return row_encrypt<NR>(m ^ pb ^ row_pick(yb, L.c) ^ pad_col(r, L.c) ^ k2c, L);
}

/* S2V over a text in memory, Y given (pa / pb loaded here) */
template <int NR>
__device__ __forceinline__ u32 s2v_text_end(u32 m, const unsigned char *p, u64 len, u32 y, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    u32 pa = 0, pb;
    if (len >= 16) {
        const u64 nf = len / 16;
        pa = row_load(p + 16 * (nf - 1), 16, L.c);
        pb = row_load(p + 16 * nf, len % 16, L.c);
    } else {
        pb = row_load(p, len, L.c);
    }
    return s2v_finish<NR>(m, len, pa, pb, y, L, k1c, k2c);
}

/* ---- CTR -------------------------------------------------------------------------------------------------------- */

/* out = in ^ keystream over len bytes; the rows of the workgroup take the blocks in turn (a row is active or not as
 * a whole, so the row-local DPP of row_encrypt never reads a lane of another block) */
template <int NR>
__device__ __forceinline__ void ctr_rows(const uaesk_ctr &ctr, const unsigned char *in, unsigned char *out, u64 len,
                                         const RowLane<NR> &L)
{
    const u32 rows = blockDim.x >> 4;
    const u64 nb = (len + 15) / 16;
    for (u64 i = threadIdx.x >> 4; i < nb; i += rows) {
        const u32 ks = row_encrypt<NR>(ctr_col(ctr, i, L.c), L);
        const u64 avail = len - 16 * i;
        const u32 x = row_load(in + 16 * i, avail, L.c);
        row_put(out + 16 * i, x ^ ks, avail < 16 ? (u32)avail : 16u, L.c);
    }
}

/* the same in one row, block after block (batches: a row per record) */
template <int NR, bool A4, u32 CH = ROW_CH>
__device__ __forceinline__ void ctr_row(const uaesk_ctr &ctr, const unsigned char *in, unsigned char *out, u64 len,
                                        const RowLane<NR> &L)
{
    const u64 full = len / 16;
    const u32 rem = (u32)(len % 16);
    row_walk<A4, CH>(in, full, L.c, [&](u64 i, u32 x) {
        row_store_full<A4>(out + 16 * i, x ^ row_encrypt<NR>(ctr_col(ctr, i, L.c), L), L.c);
    });
    if (rem) {
        const u32 x = row_load(in + 16 * full, rem, L.c);
        row_put(out + 16 * full, x ^ row_encrypt<NR>(ctr_col(ctr, full, L.c), L), rem, L.c);
    }
}

/* EAX encryption of one record in one row: C_i = P_i ^ Enc(N + i) and C = OMAC_2(ciphertext) in the same pass; the
 * keystream of block i + 1 is encrypted together with the chain step of block i (row_encrypt2) */
template <int NR, bool A4>
__device__ __forceinline__ u32 eax_text_enc(const uaesk_ctr &ctr, const unsigned char *in, unsigned char *out, u64 len,
                                            const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    const u32 tc = L.c == 3u ? 2u << 24 : 0u;
    if (!len) return row_encrypt<NR>(tc ^ k1c, L);
    const u32 s = (u32)((len - 1) % 16) + 1;
    const u64 full = (len - s) / 16;
    u32 m = tc, ks = ctr_col(ctr, 0, L.c);
    row_encrypt2<NR>(m, ks, L, L);                              /* Enc([2]_16), keystream 0 */
    row_walk<A4>(in, full, L.c, [&](u64 i, u32 x) {
        const u32 y = x ^ ks;
        row_store_full<A4>(out + 16 * i, y, L.c);
        m ^= y;
        ks = ctr_col(ctr, i + 1, L.c);
        row_encrypt2<NR>(m, ks, L, L);
    });
    const u32 y = (row_load(in + 16 * full, s, L.c) ^ ks) & row_keep(s, L.c);
    row_put(out + 16 * full, y, s, L.c);
    return row_encrypt<NR>(m ^ y ^ (s < 16 ? pad_col(s, L.c) ^ k2c : k1c), L);
}

/* SIV decryption of one record in one row: P_i = C_i ^ Enc_ctr(V' + i) written, and S2V's chain over P in the same
 * pass (Ls = K_s2v, Lc = K_ctr); returns the synthesized V */
template <int NR, bool A4, u32 CH = ROW_CH>
__device__ __forceinline__ u32 s2v_text_dec(const uaesk_ctr &ctr, const unsigned char *in, unsigned char *out, u64 len,
                                            u32 y, const RowLane<NR> &Ls, const RowLane<NR> &Lc, u32 k1c, u32 k2c)
{
    const u32 c = Ls.c;
    u32 m = 0, ks = len ? row_encrypt<NR>(ctr_col(ctr, 0, c), Lc) : 0u;
    const u64 lead = s2v_lead(len);
    row_walk<A4, CH>(in, lead, c, [&](u64 i, u32 x) {
        const u32 p = x ^ ks;
        row_store_full<A4>(out + 16 * i, p, c);
        m ^= p;
        ks = ctr_col(ctr, i + 1, c);
        row_encrypt2<NR>(m, ks, Ls, Lc);
    });
    u32 pa = 0, pb = 0;
    if (len >= 16) {
        pa = row_load(in + 16 * lead, 16, c) ^ ks;
        row_put(out + 16 * lead, pa, 16, c);
        const u32 r = (u32)(len % 16);
        if (r) {
            pb = (row_load(in + 16 * (lead + 1), r, c) ^ row_encrypt<NR>(ctr_col(ctr, lead + 1, c), Lc)) & row_keep(r, c);
            row_put(out + 16 * (lead + 1), pb, r, c);
        }
    } else if (len) {
        pb = (row_load(in, len, c) ^ ks) & row_keep((u32)len, c);
        row_put(out, pb, (u32)len, c);
    }
    return s2v_finish<NR>(m, len, pa, pb, y, Ls, k1c, k2c);
}

/* ---- one message, one launch ------------------------------------------------------------------------------------ */

/* EAX of a short message.  Encrypt: wave 0 makes N while wave 1 makes H, all rows run CTR(N), then wave 0 makes
 * OMAC_2 of the ciphertext and writes tag_len bytes of N ^ H ^ C to tag_io.  Decrypt: N, H and C in waves 0-2, the
 * tag is compared with tag_io on the device (*status = 0 / 0x1A) and CTR writes only an authentic text (:1638-1646). */
template <int NR, bool DEC>
__global__ __launch_bounds__(SMALL_WG) void k_eax_small(uaesk_rk rk, uaesk_tables tb,
                                                        const unsigned char *nonce, u64 nonce_len,
                                                        const unsigned char *aad, u64 aad_len,
                                                        const unsigned char *in, u64 len, unsigned char *out,
                                                        unsigned char *tag_io, u32 tag_len, int *status)
{
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    u32 *xch = (u32 *)(uaes_lds + E4_XCH);
    const u32 wave = threadIdx.x >> 6;
    const bool put = (threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0;      /* row 0 of a wave, one lane per column */
    if (wave == 0) {
        const u32 v = omac<NR>(0, nonce, nonce_len, L, k1c, k2c);
        if (put) xch[L.c] = v;
    } else if (wave == 1) {
        const u32 v = omac<NR>(1, aad, aad_len, L, k1c, k2c);
        if (put) xch[4 + L.c] = v;
    } else if (DEC && wave == 2) {
        const u32 v = omac<NR>(2, in, len, L, k1c, k2c);
        if (put) xch[8 + L.c] = v;
    }
    __syncthreads();
    u32 n[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) n[k] = xch[k];
    const uaesk_ctr ctr = ctr_of(n);
    if (DEC) {
        u32 diff = 0;
#pragma unroll
        for (u32 i = 0; i < 16; ++i) {
            const u32 t = (n[i >> 2] ^ xch[4 + (i >> 2)] ^ xch[8 + (i >> 2)]) >> (8 * (i & 3));
            if (i < tag_len) diff |= ((u32)tag_io[i] ^ t) & 0xffu;
        }
        if (threadIdx.x == 0) *status = diff ? 0x1A : 0;
        if (diff) return;                                    /* the same verdict in every thread */
        ctr_rows<NR>(ctr, in, out, len, L);
    } else {
        ctr_rows<NR>(ctr, in, out, len, L);
        __syncthreads();                                     /* the ciphertext is in memory for wave 0 */
        if (wave == 0) {
            const u32 c = omac<NR>(2, out, len, L, k1c, k2c);
            if ((threadIdx.x & 48u) == 0) row_put(tag_io, c ^ xch[L.c] ^ xch[4 + L.c], tag_len, L.c);
        }
    }
}

/* SIV of a short message (K_s2v = rk, K_ctr = rk2).  Encrypt: the AAD chain (wave 0) and the text's leading blocks
 * (wave 1) at the same time, wave 1 finishes with Y, V goes to iv_out and all rows run CTR(V') under K_ctr.
 * Decrypt: CTR(iv') first, then S2V over the plaintext just written, V compared with iv4 (*status = 0 / 0x1A). */
template <int NR, bool DEC>
__global__ __launch_bounds__(SMALL_WG) void k_s2v_small(uaesk_rk rk, uaesk_rk rk2, uaesk_tables tb, uint4 iv4,
                                                        const unsigned char *aad, u64 aad_len,
                                                        const unsigned char *in, u64 len, unsigned char *out,
                                                        unsigned char *iv_out, int *status)
{
    for (u32 i = threadIdx.x; i < 60u; i += blockDim.x) ((u32 *)(uaes_lds + E4_KEY2))[i] = rk2.w[i];
    row4_fill_tables(tb.te0, rk);                            /* (its barrier covers the second schedule too) */
    const RowLane<NR> L = row4_lane<NR>(), Lc = row4_lane<NR>(E4_KEY2);
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    u32 *xch = (u32 *)(uaes_lds + E4_XCH);
    const u32 wave = threadIdx.x >> 6;
    const bool put = (threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0;
    if (DEC) {
        u32 v[4] = { iv4.x, iv4.y, iv4.z & ~0x80u, iv4.w & ~0x80u };   /* c[8] &= 0x7F, c[12] &= 0x7F (:931-934) */
        ctr_rows<NR>(ctr_of(v), in, out, len, Lc);
        __syncthreads();                                     /* the plaintext is in memory for the chains */
    }
    const unsigned char *p = DEC ? out : in;
    u32 m = 0;
    if (wave == 0) {
        const u32 y = s2v_head<NR>(aad, aad_len, L, k1c, k2c);
        if (put) xch[L.c] = y;
    } else if (wave == 1) {
        m = cbc_blocks<NR>(0u, p, s2v_lead(len), L);
    }
    __syncthreads();
    if (wave == 1) {
        const u32 v = s2v_text_end<NR>(m, p, len, xch[L.c], L, k1c, k2c);
        if (put) xch[4 + L.c] = v;
    }
    __syncthreads();
    u32 v[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) v[k] = xch[4 + k];
    if (DEC) {
        if (threadIdx.x == 0)
            *status = ((v[0] ^ iv4.x) | (v[1] ^ iv4.y) | (v[2] ^ iv4.z) | (v[3] ^ iv4.w)) ? 0x1A : 0;
    } else {
        if (threadIdx.x < 4) ((u32 *)iv_out)[threadIdx.x] = v[threadIdx.x];
        v[2] &= ~0x80u;
        v[3] &= ~0x80u;
        ctr_rows<NR>(ctr_of(v), in, out, len, Lc);
    }
}

/* ---- longer messages: the chains in one launch, CTR by the host ------------------------------------------------- */
/* res (device, 48 bytes): int status at 0, the counter block (N, or S2V's V) at 16, N ^ H at 32 */

/* mode 0: N || H (EAX encrypt: res gets N and N ^ H); 1: N || H || C (decrypt: the tag compared with tag_io, res gets
 * the status and N); 2: C only (encrypt, after CTR: tag_len bytes of C ^ (N ^ H) to tag_io).  One wave per chain. */
template <int NR>
__global__ __launch_bounds__(192) void k_eax_macs(uaesk_rk rk, uaesk_tables tb, int mode,
                                                  const unsigned char *nonce, u64 nonce_len,
                                                  const unsigned char *aad, u64 aad_len,
                                                  const unsigned char *ct, u64 len,
                                                  unsigned char *tag_io, u32 tag_len, unsigned char *res)
{
    row_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row_lane<NR>();
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    u32 *xch = (u32 *)(uaes_lds + ER_XCH);
    const u32 wave = threadIdx.x >> 6;
    const u32 slot = mode == 2 ? 2u : wave;                  /* 0 = N, 1 = H, 2 = C */
    u32 v;
    if (slot == 0) v = omac<NR>(0, nonce, nonce_len, L, k1c, k2c);
    else if (slot == 1) v = omac<NR>(1, aad, aad_len, L, k1c, k2c);
    else v = omac<NR>(2, ct, len, L, k1c, k2c);
    if ((threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0) xch[4 * slot + L.c] = v;
    __syncthreads();
    u32 *r32 = (u32 *)res;
    if (mode == 0) {
        if (threadIdx.x < 4) {
            r32[4 + threadIdx.x] = xch[threadIdx.x];
            r32[8 + threadIdx.x] = xch[threadIdx.x] ^ xch[4 + threadIdx.x];
        }
    } else if (mode == 1) {
        if (threadIdx.x < 4) r32[4 + threadIdx.x] = xch[threadIdx.x];
        if (threadIdx.x == 0) {
            u32 diff = 0;
#pragma unroll
            for (u32 i = 0; i < 16; ++i) {
                const u32 t = (xch[i >> 2] ^ xch[4 + (i >> 2)] ^ xch[8 + (i >> 2)]) >> (8 * (i & 3));
                if (i < tag_len) diff |= ((u32)tag_io[i] ^ t) & 0xffu;
            }
            r32[0] = diff ? 0x1Au : 0u;
        }
    } else if (threadIdx.x < 16 && (threadIdx.x & 3u) == 0) {
        row_put(tag_io, v ^ r32[8 + L.c], tag_len, L.c);
    }
}

/* S2V of a longer message: the AAD chain (wave 0) and the text's leading blocks (wave 1) at the same time.  Encrypt:
 * res gets V; decrypt (text = the plaintext CTR has just written): res gets the status of V against iv4. */
template <int NR, bool DEC>
__global__ __launch_bounds__(128) void k_s2v_macs(uaesk_rk rk, uaesk_tables tb, uint4 iv4,
                                                  const unsigned char *aad, u64 aad_len,
                                                  const unsigned char *p, u64 len, unsigned char *res)
{
    row_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row_lane<NR>();
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    u32 *xch = (u32 *)(uaes_lds + ER_XCH);
    const u32 wave = threadIdx.x >> 6;
    const bool put = (threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0;
    u32 m = 0;
    if (wave == 0) {
        const u32 y = s2v_head<NR>(aad, aad_len, L, k1c, k2c);
        if (put) xch[L.c] = y;
    } else {
        m = cbc_blocks<NR>(0u, p, s2v_lead(len), L);
    }
    __syncthreads();
    if (wave == 1) {
        const u32 v = s2v_text_end<NR>(m, p, len, xch[L.c], L, k1c, k2c);
        if (put) xch[4 + L.c] = v;
    }
    __syncthreads();
    u32 *r32 = (u32 *)res;
    if (!DEC) {
        if (threadIdx.x < 4) r32[4 + threadIdx.x] = xch[4 + threadIdx.x];
    } else if (threadIdx.x == 0) {
        r32[0] = ((xch[4] ^ iv4.x) | (xch[5] ^ iv4.y) | (xch[6] ^ iv4.z) | (xch[7] ^ iv4.w)) ? 0x1Au : 0u;
    }
}

/* ---- batches: nmsg records of msg_bytes under one key, sixteen lanes per record ---------------------------------- */
/* Record m: text at in / out + m msg_bytes, its nonce (EAX) at nonces + m nonce_len, its AAD at aad + m aad_bytes,
 * its tag (EAX) / V (SIV) at tags + 16 m.  Decrypt: verdicts[m] = 1 if authentic, else 0 and bad[0] |= 1 (a vector
 * atomic); EAX leaves a failed record's output untouched, SIV zeroes it when `wipe`.  A4: text 4-byte aligned. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_eax_batch(uaesk_rk rk, uaesk_tables tb,
                                                       const unsigned char *nonces, u64 nonce_len,
                                                       const unsigned char *aad, u64 aad_bytes,
                                                       u64 nmsg, u64 msg_bytes, const unsigned char *in, unsigned char *out,
                                                       unsigned char *tags, unsigned char *verdicts, int *bad)
{
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        const u32 n = omac<NR>(0, nonces + m * nonce_len, nonce_len, L, k1c, k2c);
        const u32 h = omac<NR>(1, aad + m * aad_bytes, aad_bytes, L, k1c, k2c);
        u32 nb[4];
        row_gather(n, nb);
        const uaesk_ctr ctr = ctr_of(nb);
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        unsigned char *tg = tags + 16 * m;
        if (!DEC) {
            const u32 c = eax_text_enc<NR, A4>(ctr, src, dst, msg_bytes, L, k1c, k2c);
            row_put(tg, n ^ h ^ c, 16, L.c);
        } else {
            const u32 c = omac<NR>(2, src, msg_bytes, L, k1c, k2c);
            u32 d[4];
            row_gather(n ^ h ^ c ^ row_load(tg, 16, L.c), d);
            const bool ok = (d[0] | d[1] | d[2] | d[3]) == 0;
            row_verdict((threadIdx.x & 15u) == 0, verdicts, m, ok, bad);
            if (ok) ctr_row<NR, A4>(ctr, src, dst, msg_bytes, L);
        }
    }
}

template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_s2v_batch(uaesk_rk rk, uaesk_rk rk2, uaesk_tables tb, int wipe,
                                                       const unsigned char *aad, u64 aad_bytes,
                                                       u64 nmsg, u64 msg_bytes, const unsigned char *in, unsigned char *out,
                                                       unsigned char *ivs, unsigned char *verdicts, int *bad)
{
    for (u32 i = threadIdx.x; i < 60u; i += blockDim.x) ((u32 *)(uaes_lds + E4_KEY2))[i] = rk2.w[i];
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>(), Lc = row4_lane<NR>(E4_KEY2);
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        const u32 y = s2v_head<NR>(aad + m * aad_bytes, aad_bytes, L, k1c, k2c);
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        unsigned char *ivp = ivs + 16 * m;
        u32 vb[4];
        if (!DEC) {
            const u32 chain = cbc_blocks<NR>(0u, src, s2v_lead(msg_bytes), L);
            const u32 v = s2v_text_end<NR>(chain, src, msg_bytes, y, L, k1c, k2c);
            row_put(ivp, v, 16, L.c);
            row_gather(v, vb);
            vb[2] &= ~0x80u;
            vb[3] &= ~0x80u;
            ctr_row<NR, A4>(ctr_of(vb), src, dst, msg_bytes, Lc);
        } else {
            const u32 iv = row_load(ivp, 16, L.c);
            row_gather(iv, vb);
            vb[2] &= ~0x80u;
            vb[3] &= ~0x80u;
            const u32 v = s2v_text_dec<NR, A4>(ctr_of(vb), src, dst, msg_bytes, y, L, Lc, k1c, k2c);
            u32 d[4];
            row_gather(v ^ iv, d);
            const bool ok = (d[0] | d[1] | d[2] | d[3]) == 0;
            row_verdict((threadIdx.x & 15u) == 0, verdicts, m, ok, bad);
            if (!ok && wipe)
                for (u64 i = 0; i < msg_bytes; i += 16) row_put(dst + i, 0u, msg_bytes - i < 16 ? (u32)(msg_bytes - i) : 16u, L.c);
        }
    }
}

/* ---- S2V over a vector of associated data (RFC 5297 section 2.4) -------------------------------------------------- */
/* Y_n = dbl^n(CMAC(0^128)) ^ XOR_i dbl^(n-i)(CMAC(S_i)), folded as Y_0 = CMAC(0^128), Y_i = dbl(Y_{i-1}) ^ CMAC(S_i).
 * The component CMACs are independent chains; only the fold is serial, and it is doublings.  A component may be empty:
 * it still is one, CMAC("") = Enc(10* ^ K2).  No component at all leaves Y_0, which is s2v_head without AAD; one
 * non-empty component gives s2v_head's Y. */

/* LDS behind k_s2v_small's: the CMAC of every component, sixteen bytes each */
#define E4V_MACS  E4_LDS
#define E4V_LDS   (E4_LDS + 16u * (u32)UAES_S2V_AD_MAX)
/* the rows of the workgroup that the components are dealt over: all but wave 1's four, which walk the text */
#define S2V_V_ROWS (SMALL_WG / 16u - 4u)

/* CMAC of a whole string, the empty one included */
template <int NR, u32 CH = ROW_CH>
__device__ __forceinline__ u32 cmac_any(const unsigned char *p, u64 len, const RowLane<NR> &L, u32 k1c, u32 k2c)
{
    if (!len) return row_encrypt<NR>(pad_col(0u, L.c) ^ k2c, L);
    return cmac_more<NR, CH>(0u, p, len, L, k1c, k2c);
}

/* SIV of one message with nad components (K_s2v = rk, K_ctr = rk2); component i is aad[ends[i - 1] .. ends[i]) (ends:
 * nad running totals, 8-byte aligned).  Row r of the workgroup (wave 1's rows apart) takes components r, r + S2V_V_ROWS,
 * ... and leaves their CMACs in LDS; wave 1 walks the text's leading blocks meanwhile, then folds the CMACs in order and
 * finishes as k_s2v_small does.  CTR: the text is short and CTR runs here, before (decrypt) or after (encrypt) the
 * chains, over all rows; without it this is the chains of a longer text (k_s2v_macs' part: CTR by the host, a decrypt's
 * plaintext already in `out`).  V goes to iv_out (encrypt), *status = 0 / 0x1A (decrypt). */
template <int NR, bool DEC, bool CTR>
__global__ __launch_bounds__(SMALL_WG) void k_s2v_v(uaesk_rk rk, uaesk_rk rk2, uaesk_tables tb, uint4 iv4,
                                                    const unsigned char *aad, const u64 *ends, u32 nad,
                                                    const unsigned char *in, u64 len, unsigned char *out,
                                                    unsigned char *iv_out, int *status)
{
    for (u32 i = threadIdx.x; i < 60u; i += blockDim.x) ((u32 *)(uaes_lds + E4_KEY2))[i] = rk2.w[i];
    row4_fill_tables(tb.te0, rk);                            /* (its barrier covers the second schedule too) */
    const RowLane<NR> L = row4_lane<NR>(), Lc = row4_lane<NR>(E4_KEY2);
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    u32 *xch = (u32 *)(uaes_lds + E4_XCH), *macs = (u32 *)(uaes_lds + E4V_MACS);
    const u32 wave = threadIdx.x >> 6, row = threadIdx.x >> 4;
    const bool put = (threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0;
    if (DEC && CTR) {
        u32 v[4] = { iv4.x, iv4.y, iv4.z & ~0x80u, iv4.w & ~0x80u };
        ctr_rows<NR>(ctr_of(v), in, out, len, Lc);
        __syncthreads();                                     /* the plaintext is in memory for the chains */
    }
    const unsigned char *p = DEC ? out : in;
    u32 m = 0, y = 0;
    if (wave == 1) {
        m = cbc_blocks<NR>(0u, p, s2v_lead(len), L);
        y = row_encrypt<NR>(k1c, L);                         /* Y_0 = CMAC of one zero block = Enc(K1) */
    } else {
        for (u32 i = row < 4u ? row : row - 4u; i < nad; i += S2V_V_ROWS) {
            const u64 at = i ? ends[i - 1] : 0;
            const u32 c = cmac_any<NR>(aad + at, ends[i] - at, L, k1c, k2c);
            if ((threadIdx.x & 3u) == 0) macs[4u * i + L.c] = c;
        }
    }
    __syncthreads();
    if (wave == 1) {
        u32 b[4];
        row_gather(y, b);
        for (u32 i = 0; i < nad; ++i) {
            dbl_be(b);
#pragma unroll
            for (u32 k = 0; k < 4; ++k) b[k] ^= macs[4u * i + k];
        }
        const u32 v = s2v_text_end<NR>(m, p, len, row_pick(b, L.c), L, k1c, k2c);
        if (put) xch[4 + L.c] = v;
    }
    __syncthreads();
    u32 v[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) v[k] = xch[4 + k];
    if (DEC) {
        if (threadIdx.x == 0)
            *status = ((v[0] ^ iv4.x) | (v[1] ^ iv4.y) | (v[2] ^ iv4.z) | (v[3] ^ iv4.w)) ? 0x1A : 0;
    } else {
        if (threadIdx.x < 4) ((u32 *)iv_out)[threadIdx.x] = v[threadIdx.x];
        if (CTR) {
            v[2] &= ~0x80u;
            v[3] &= ~0x80u;
            ctr_rows<NR>(ctr_of(v), in, out, len, Lc);
        }
    }
}

/* the lengths of a batch record's components, by value */
struct s2v_adl { u64 n[UAES_S2V_BATCH_AD_MAX]; };

/* k_s2v_batch with every record's AAD slot cut into the same nad components and a length per record: record m is the
 * first lens[m] bytes of its slot (lens NULL: msg_bytes; a longer entry counts as msg_bytes), the rest of its output
 * slot is not written.  The record's row walks its components one after another. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_s2v_batch_v(uaesk_rk rk, uaesk_rk rk2, uaesk_tables tb, int wipe,
                                                         const unsigned char *aad, u64 aad_bytes, u32 nad, s2v_adl adl,
                                                         u64 nmsg, u64 msg_bytes, const u32 *lens,
                                                         const unsigned char *in, unsigned char *out,
                                                         unsigned char *ivs, unsigned char *verdicts, int *bad)
{
    for (u32 i = threadIdx.x; i < 60u; i += blockDim.x) ((u32 *)(uaes_lds + E4_KEY2))[i] = rk2.w[i];
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>(), Lc = row4_lane<NR>(E4_KEY2);
    u32 k1c, k2c;
    cmac_subkeys<NR>(L, k1c, k2c);
    constexpr u32 BCH = 8;                                   /* row_walk's chunk: two key schedules leave no room for 2 x 16 blocks in flight */
    u32 *y0 = (u32 *)(uaes_lds + E4_XCH);                    /* Y_0 = CMAC(0^128) = Enc(K1), the same for every record: kept */
    y0[L.c] = row_encrypt<NR>(k1c, L);                       /* in LDS, not in a register (every lane of a column writes the same word) */
    __syncthreads();
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u32 len = (u32)msg_bytes;                            /* (the host layer refuses slots above UINT32_MAX) */
        if (lens) { len = lens[m]; if (len > msg_bytes) len = (u32)msg_bytes; }
        const unsigned char *a = aad + m * aad_bytes;
        u32 y = y0[L.c];
        for (u32 i = 0; i < nad; ++i) {
            u64 n = 0;
#pragma unroll
            for (u32 k = 0; k < UAES_S2V_BATCH_AD_MAX; ++k)
                if (k == i) n = adl.n[k];
            u32 b[4];
            row_gather(y, b);
            dbl_be(b);
            y = row_pick(b, L.c) ^ cmac_any<NR, BCH>(a, n, L, k1c, k2c);
            a += n;
        }
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        unsigned char *ivp = ivs + 16 * m;
        u32 vb[4];
        if (!DEC) {
            const u32 chain = cbc_blocks<NR, BCH>(0u, src, s2v_lead(len), L);
            const u32 v = s2v_text_end<NR>(chain, src, len, y, L, k1c, k2c);
            row_put(ivp, v, 16, L.c);
            row_gather(v, vb);
            vb[2] &= ~0x80u;
            vb[3] &= ~0x80u;
            ctr_row<NR, A4, BCH>(ctr_of(vb), src, dst, len, Lc);
        } else {
            const u32 iv = row_load(ivp, 16, L.c);
            row_gather(iv, vb);
            vb[2] &= ~0x80u;
            vb[3] &= ~0x80u;
            const u32 v = s2v_text_dec<NR, A4, BCH>(ctr_of(vb), src, dst, len, y, L, Lc, k1c, k2c);
            u32 d[4];
            row_gather(v ^ iv, d);
            const bool ok = (d[0] | d[1] | d[2] | d[3]) == 0;
            row_verdict((threadIdx.x & 15u) == 0, verdicts, m, ok, bad);
            if (!ok && wipe)
                for (u32 i = 0; i < len; i += 16) row_put(dst + i, 0u, len - i < 16 ? len - i : 16u, L.c);
        }
    }
}

/* ---- EAX' (ANSI C12.22 / IEEE 1703; the reference built with EAXP 1, :1523-1648) ---------------------------------- */
/* L = Enc(0), D = dblLE(L), Q = dblLE(D).  CMAC'(start, X) is CMAC with D / Q as its subkeys and a chaining value that
 * starts at `start`; N = CMAC'(D, nonce), N' = N with the top bits of bytes 12 and 14 cleared, C = CTR(N', P) with the
 * 56-bit counter, C' = CMAC'(Q, C) (0^128 for an empty C, oMac :1535-1539), mac = N[12..15] ^ C'[12..15]: column 3.  No
 * associated data, so a call has one chain fewer than EAX.  Minematsu, Lucks, Morita and Iwata (2013) forge EAX' when
 * nonce and text are both at most one block; such inputs are taken all the same, as the reference takes them. */

/* little-endian doubling (doubleLblock :449-458): the block as a little-endian 128-bit integer, 0x87 into byte 0 */
__device__ __forceinline__ void dbl_le(u32 (&b)[4])
{
    const u32 carry = b[3] >> 31;
    b[3] = (b[3] << 1) | (b[2] >> 31);
    b[2] = (b[2] << 1) | (b[1] >> 31);
    b[1] = (b[1] << 1) | (b[0] >> 31);
    b[0] = (b[0] << 1) ^ (carry ? 0x87u : 0u);
}

/* D and Q: this lane's columns */
template <int NR>
__device__ __forceinline__ void cmac_subkeys_le(const RowLane<NR> &L, u32 &dc, u32 &qc)
{
    u32 b[4];
    row_gather(row_encrypt<NR>(0u, L), b);
    dbl_le(b);
    dc = row_pick(b, L.c);
    dbl_le(b);
    qc = row_pick(b, L.c);
}

/* CMAC'(start, p[0 .. len)); the empty string is one padded empty block (cMac :579-589 with dataSize 0) */
template <int NR>
__device__ __forceinline__ u32 cmac_prime(u32 start, const unsigned char *p, u64 len, const RowLane<NR> &L, u32 dc, u32 qc)
{
    if (!len) return row_encrypt<NR>(start ^ pad_col(0u, L.c) ^ qc, L);
    return cmac_more<NR>(start, p, len, L, dc, qc);
}

/* C' of a ciphertext in memory */
template <int NR>
__device__ __forceinline__ u32 eaxp_cmac_text(const unsigned char *p, u64 len, const RowLane<NR> &L, u32 dc, u32 qc)
{
    return len ? cmac_prime<NR>(qc, p, len, L, dc, qc) : 0u;
}

/* N -> the counter of CTR(N'): mac[12] &= 0x7F, mac[14] &= 0x7F (:1581-1582), bits 7 and 23 of the little-endian column 3 */
__device__ __forceinline__ uaesk_ctr eaxp_ctr(const u32 (&n)[4])
{
    const u32 v[4] = { n[0], n[1], n[2], n[3] & ~0x00800080u };
    return ctr_of(v);
}

/* the four bytes of a mac at any byte offset */
__device__ __forceinline__ u32 mac_get(const unsigned char *p)
{
    if ((((uintptr_t)p) & 3u) == 0) return *(const u32 *)p;
    return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24);
}

__device__ __forceinline__ void mac_put(unsigned char *p, u32 w)
{
    if ((((uintptr_t)p) & 3u) == 0) { *(u32 *)p = w; return; }
    p[0] = (unsigned char)w; p[1] = (unsigned char)(w >> 8); p[2] = (unsigned char)(w >> 16); p[3] = (unsigned char)(w >> 24);
}

/* EAX' of a short message.  Encrypt: wave 0 makes N, all rows run CTR(N'), then wave 0 makes C' of the ciphertext and
 * writes the mac to mac_io.  Decrypt: N and C' in waves 0 and 1, the mac compared with mac_io (*status = 0 / 0x1A), and
 * CTR writes only an authentic text (:1631-1644). */
template <int NR, bool DEC>
__global__ __launch_bounds__(SMALL_WG) void k_eaxp_small(uaesk_rk rk, uaesk_tables tb, const unsigned char *nonce, u64 nonce_len,
                                                         const unsigned char *in, u64 len, unsigned char *out,
                                                         unsigned char *mac_io, int *status)
{
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    u32 dc, qc;
    cmac_subkeys_le<NR>(L, dc, qc);
    u32 *xch = (u32 *)(uaes_lds + E4_XCH);
    const u32 wave = threadIdx.x >> 6;
    const bool put = (threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0;      /* row 0 of a wave, one lane per column */
    if (wave == 0) {
        const u32 v = cmac_prime<NR>(dc, nonce, nonce_len, L, dc, qc);
        if (put) xch[L.c] = v;
    } else if (DEC && wave == 1) {
        const u32 v = eaxp_cmac_text<NR>(in, len, L, dc, qc);
        if (put) xch[4 + L.c] = v;
    }
    __syncthreads();
    u32 n[4];
#pragma unroll
    for (u32 k = 0; k < 4; ++k) n[k] = xch[k];
    const uaesk_ctr ctr = eaxp_ctr(n);
    if (DEC) {
        const u32 diff = n[3] ^ xch[7] ^ mac_get(mac_io);
        if (threadIdx.x == 0) *status = diff ? 0x1A : 0;
        if (diff) return;                                    /* the same verdict in every thread */
        ctr_rows<NR>(ctr, in, out, len, L);
    } else {
        ctr_rows<NR>(ctr, in, out, len, L);
        __syncthreads();                                     /* the ciphertext is in memory for wave 0 */
        if (wave == 0) {
            const u32 c = eaxp_cmac_text<NR>(out, len, L, dc, qc);
            if (threadIdx.x == 12) mac_put(mac_io, c ^ n[3]);                   /* column 3 of row 0 */
        }
    }
}

/* The chains of a longer message, one wave per chain; res (device, 48 bytes) as k_eax_macs has it.  mode 0: N (encrypt:
 * res gets the counter block N' at 16 and N's column 3 at 32); 1: N || C' (decrypt: the mac compared with mac_io, res
 * gets the status and N'); 2: C' only (encrypt, after CTR: the mac to mac_io). */
template <int NR>
__global__ __launch_bounds__(128) void k_eaxp_macs(uaesk_rk rk, uaesk_tables tb, int mode, const unsigned char *nonce, u64 nonce_len,
                                                   const unsigned char *ct, u64 len, unsigned char *mac_io, unsigned char *res)
{
    row_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row_lane<NR>();
    u32 dc, qc;
    cmac_subkeys_le<NR>(L, dc, qc);
    u32 *xch = (u32 *)(uaes_lds + ER_XCH);
    const u32 slot = mode == 2 ? 1u : threadIdx.x >> 6;      /* 0 = N, 1 = C' */
    const u32 v = slot == 0 ? cmac_prime<NR>(dc, nonce, nonce_len, L, dc, qc) : eaxp_cmac_text<NR>(ct, len, L, dc, qc);
    if ((threadIdx.x & 63u) < 16u && (threadIdx.x & 3u) == 0) xch[4 * slot + L.c] = v;
    __syncthreads();
    u32 *r32 = (u32 *)res;
    if (mode == 2) {
        if (threadIdx.x == 0) mac_put(mac_io, xch[7] ^ r32[8]);
        return;
    }
    if (threadIdx.x < 4) r32[4 + threadIdx.x] = threadIdx.x == 3 ? xch[3] & ~0x00800080u : xch[threadIdx.x];
    if (threadIdx.x == 0) {
        if (mode == 0) r32[8] = xch[3];
        else r32[0] = (xch[3] ^ xch[7] ^ mac_get(mac_io)) ? 0x1Au : 0u;
    }
}

/* EAX' encryption of one record in one row: C_i = P_i ^ Enc(N' + i) and C' in the same pass, as eax_text_enc */
template <int NR, bool A4>
__device__ __forceinline__ u32 eaxp_text_enc(const uaesk_ctr &ctr, const unsigned char *in, unsigned char *out, u64 len,
                                             const RowLane<NR> &L, u32 dc, u32 qc)
{
    if (!len) return 0u;
    const u32 s = (u32)((len - 1) % 16) + 1;
    const u64 full = (len - s) / 16;
    u32 m = qc, ks = row_encrypt<NR>(ctr_col(ctr, 0, L.c), L);
    row_walk<A4>(in, full, L.c, [&](u64 i, u32 x) {
        const u32 y = x ^ ks;
        row_store_full<A4>(out + 16 * i, y, L.c);
        m ^= y;
        ks = ctr_col(ctr, i + 1, L.c);
        row_encrypt2<NR>(m, ks, L, L);
    });
    const u32 y = (row_load(in + 16 * full, s, L.c) ^ ks) & row_keep(s, L.c);
    row_put(out + 16 * full, y, s, L.c);
    return row_encrypt<NR>(m ^ y ^ (s < 16 ? pad_col(s, L.c) ^ qc : dc), L);
}

/* Batches: record m is the first lens[m] bytes of its text slot (in / out + m msg_bytes) under the first nlens[m] bytes
 * of its nonce slot (nonces + m nonce_bytes); NULL lens / nlens: the whole slot, a longer entry counts as the slot.  Its
 * mac is the four bytes at macs + 4 m.  Decrypt: verdicts (may be NULL) and bad as k_eax_batch, a forged record's output
 * untouched; the rest of an output slot is not written. */
template <int NR, bool DEC, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_eaxp_batch(uaesk_rk rk, uaesk_tables tb, const unsigned char *nonces, u32 nonce_bytes,
                                                        const u32 *nlens, u64 nmsg, u32 msg_bytes, const u32 *lens,
                                                        const unsigned char *in, unsigned char *out,
                                                        unsigned char *macs, unsigned char *verdicts, int *bad)
{
    row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    u32 dc, qc;
    cmac_subkeys_le<NR>(L, dc, qc);
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u32 len = msg_bytes, nl = nonce_bytes;
        if (lens) { len = lens[m]; if (len > msg_bytes) len = msg_bytes; }
        if (nlens) { nl = nlens[m]; if (nl > nonce_bytes) nl = nonce_bytes; }
        const u32 n = cmac_prime<NR>(dc, nonces + m * nonce_bytes, nl, L, dc, qc);
        u32 nb[4], d[4];
        row_gather(n, nb);
        const uaesk_ctr ctr = eaxp_ctr(nb);
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        unsigned char *mac = macs + 4 * m;
        if (!DEC) {
            row_gather(eaxp_text_enc<NR, A4>(ctr, src, dst, len, L, dc, qc), d);
            if ((threadIdx.x & 15u) == 0) mac_put(mac, nb[3] ^ d[3]);
        } else {
            row_gather(eaxp_cmac_text<NR>(src, len, L, dc, qc), d);
            const bool ok = (nb[3] ^ d[3]) == mac_get(mac);
            row_verdict<true>((threadIdx.x & 15u) == 0, verdicts, m, ok, bad);
            if (ok) ctr_row<NR, A4>(ctr, src, dst, len, L);
        }
    }
}

/* ---- launchers ---------------------------------------------------------------------------------------------------- */
static uint4 uint4_of(const uint8_t *b)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (b) memcpy(&v, b, 16);
    return v;
}

template <int NR>
static int launch_eax_small(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, int decrypt,
                            const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                            const void *in, size_t len, void *out, void *tag_io, unsigned tag_len, int *status)
{
    return with_bool(decrypt, [&](auto DEC) {
        return uaesk_launch(k_eax_small<NR, decltype(DEC)::value>, 1, SMALL_WG, E4_LDS, st, *ek, *tb, nonce, nonce_len, aad, aad_len,
                            in, len, out, tag_io, tag_len, status); });
}

extern "C" int uaesk_eax_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                               const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                               const void *in, size_t len, void *out, void *tag_io, unsigned tag_len, int *status)
{
    if (tag_len < 1 || tag_len > 16) return (int)hipErrorInvalidValue;
    DISPATCH_NR(nr, return (launch_eax_small<NR>(S(stream), tb, ek, decrypt, nonce, nonce_len, aad, aad_len, in, len,
                                                 out, tag_io, tag_len, status)));
    return 0;
}

template <int NR>
static int launch_eax_macs(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, int mode,
                           const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                           const void *ct, size_t len, void *tag_io, unsigned tag_len, void *res)
{
    const unsigned waves = mode == 0 ? 2u : mode == 1 ? 3u : 1u;
    return uaesk_launch(k_eax_macs<NR>, 1, 64 * waves, ER_LDS, st, *ek, *tb, mode, nonce, nonce_len, aad, aad_len, ct, len, tag_io,
                        tag_len, res);
}

extern "C" int uaesk_eax_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mode,
                              const void *nonce, size_t nonce_len, const void *aad, size_t aad_len,
                              const void *ct, size_t len, void *tag_io, unsigned tag_len, void *res48)
{
    if (mode < 0 || mode > 2 || tag_len < 1 || tag_len > 16) return (int)hipErrorInvalidValue;
    DISPATCH_NR(nr, return (launch_eax_macs<NR>(S(stream), tb, ek, mode, nonce, nonce_len, aad, aad_len, ct, len,
                                                tag_io, tag_len, res48)));
    return 0;
}

template <int NR>
static int launch_s2v_small(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const uaesk_rk *ek2, int decrypt,
                            uint4 iv, const void *aad, size_t aad_len, const void *in, size_t len, void *out,
                            void *iv_out, int *status)
{
    return with_bool(decrypt, [&](auto DEC) {
        return uaesk_launch(k_s2v_small<NR, decltype(DEC)::value>, 1, SMALL_WG, E4_LDS, st, *ek, *ek2, *tb, iv, aad, aad_len, in, len,
                            out, iv_out, status); });
}

extern "C" int uaesk_s2v_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v,
                               const uaesk_rk *ek_ctr, int decrypt, const uint8_t *iv16, const void *aad, size_t aad_len,
                               const void *in, size_t len, void *out, void *iv_out, int *status)
{
    const uint4 iv = uint4_of(iv16);
    DISPATCH_NR(nr, return (launch_s2v_small<NR>(S(stream), tb, ek_s2v, ek_ctr, decrypt, iv, aad, aad_len, in, len, out,
                                                 iv_out, status)));
    return 0;
}

template <int NR>
static int launch_s2v_macs(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, int decrypt, uint4 iv,
                           const void *aad, size_t aad_len, const void *text, size_t len, void *res)
{
    return with_bool(decrypt, [&](auto DEC) {
        return uaesk_launch(k_s2v_macs<NR, decltype(DEC)::value>, 1, 128, ER_LDS, st, *ek, *tb, iv, aad, aad_len, text, len, res); });
}

extern "C" int uaesk_s2v_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, int decrypt,
                              const uint8_t *iv16, const void *aad, size_t aad_len, const void *text, size_t len, void *res48)
{
    const uint4 iv = uint4_of(iv16);
    DISPATCH_NR(nr, return (launch_s2v_macs<NR>(S(stream), tb, ek_s2v, decrypt, iv, aad, aad_len, text, len, res48)));
    return 0;
}

template <int NR>
static int launch_eax_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, int decrypt, const void *nonces,
                            size_t nonce_len, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                            const void *in, void *out, void *tags, void *verdicts, int *bad)
{
    const RowShape s = uaesk_row_shape(nmsg);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_eax_batch<NR, decltype(DEC)::value, decltype(A4)::value>, s.grid, s.wg, E4_LDS, st, *ek, *tb, nonces,
                            nonce_len, aad, aad_bytes, nmsg, msg_bytes, in, out, tags, verdicts, bad); }); });
}

extern "C" int uaesk_eax_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                               const void *nonces, size_t nonce_len, const void *aad, size_t aad_bytes,
                               size_t nmsg, size_t msg_bytes, const void *in, void *out, void *tags, void *verdicts, int *bad)
{
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_eax_batch<NR>(S(stream), tb, ek, decrypt, nonces, nonce_len, aad, aad_bytes, nmsg,
                                                 msg_bytes, in, out, tags, verdicts, bad)));
    return 0;
}

template <int NR>
static int launch_s2v_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const uaesk_rk *ek2, int decrypt,
                            int wipe, const void *aad, size_t aad_bytes, size_t nmsg, size_t msg_bytes,
                            const void *in, void *out, void *ivs, void *verdicts, int *bad)
{
    const RowShape s = uaesk_row_shape(nmsg);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_s2v_batch<NR, decltype(DEC)::value, decltype(A4)::value>, s.grid, s.wg, E4_LDS, st, *ek, *ek2, *tb, wipe,
                            aad, aad_bytes, nmsg, msg_bytes, in, out, ivs, verdicts, bad); }); });
}

extern "C" int uaesk_s2v_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v,
                               const uaesk_rk *ek_ctr, int decrypt, int wipe, const void *aad, size_t aad_bytes,
                               size_t nmsg, size_t msg_bytes, const void *in, void *out, void *ivs, void *verdicts, int *bad)
{
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_s2v_batch<NR>(S(stream), tb, ek_s2v, ek_ctr, decrypt, wipe, aad, aad_bytes, nmsg,
                                                 msg_bytes, in, out, ivs, verdicts, bad)));
    return 0;
}

template <int NR>
static int launch_s2v_v(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const uaesk_rk *ek2, int decrypt, int ctr,
                        uint4 iv, const void *aad, const void *ends, unsigned nad, const void *in, size_t len, void *out,
                        void *res)
{
    return with_bool(decrypt, [&](auto DEC) { return with_bool(ctr, [&](auto CTR) {
        return uaesk_launch(k_s2v_v<NR, decltype(DEC)::value, decltype(CTR)::value>, 1, SMALL_WG, E4V_LDS, st, *ek, *ek2, *tb, iv,
                            aad, ends, nad, in, len, out, (unsigned char *)res + 16, res); }); });
}

extern "C" int uaesk_s2v_v(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                           int decrypt, int ctr, const uint8_t *iv16, const void *aad, const void *ends, unsigned nad,
                           const void *in, size_t len, void *out, void *res48)
{
    const uint4 iv = uint4_of(iv16);
    if (nad > UAES_S2V_AD_MAX || (nad && (!ends || ((uintptr_t)ends & 7u))) || (ctr && len > UAES_EAX_SIV_SMALL_MAX))
        return (int)hipErrorInvalidValue;
    DISPATCH_NR(nr, return (launch_s2v_v<NR>(S(stream), tb, ek_s2v, ek_ctr, decrypt, ctr, iv, aad, ends, nad, in, len, out, res48)));
    return 0;
}

template <int NR>
static int launch_s2v_batch_v(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const uaesk_rk *ek2, int decrypt,
                              int wipe, const void *aad, size_t aad_bytes, unsigned nad, const s2v_adl &adl, size_t nmsg,
                              size_t msg_bytes, const void *lens, const void *in, void *out, void *ivs, void *verdicts, int *bad)
{
    const RowShape s = uaesk_row_shape(nmsg);
    return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_s2v_batch_v<NR, decltype(DEC)::value, decltype(A4)::value>, s.grid, s.wg, E4_LDS, st, *ek, *ek2, *tb, wipe,
                            aad, aad_bytes, nad, adl, nmsg, msg_bytes, lens, in, out, ivs, verdicts, bad); }); });
}

extern "C" int uaesk_s2v_batch_v(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek_s2v, const uaesk_rk *ek_ctr,
                                 int decrypt, int wipe, const void *aad, unsigned nad, const size_t *ad_lens,
                                 size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out, void *ivs,
                                 void *verdicts, int *bad)
{
    s2v_adl adl;
    size_t aad_bytes = 0;
    if (nad > UAES_S2V_BATCH_AD_MAX || (nad && !ad_lens) || ((uintptr_t)lens & 3u)) return (int)hipErrorInvalidValue;
    memset(&adl, 0, sizeof adl);
    for (unsigned i = 0; i < nad; ++i) { adl.n[i] = ad_lens[i]; aad_bytes += ad_lens[i]; }
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_s2v_batch_v<NR>(S(stream), tb, ek_s2v, ek_ctr, decrypt, wipe, aad, aad_bytes, nad, adl, nmsg,
                                                   msg_bytes, lens, in, out, ivs, verdicts, bad)));
    return 0;
}

extern "C" int uaesk_eaxp_small(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                                const void *nonce, size_t nonce_len, const void *in, size_t len, void *out, void *mac_io, int *status)
{
    if (len > UAES_EAX_SIV_SMALL_MAX) return (int)hipErrorInvalidValue;
    DISPATCH_NR(nr, return with_bool(decrypt, [&](auto DEC) {
        return uaesk_launch(k_eaxp_small<NR, decltype(DEC)::value>, 1, SMALL_WG, E4_LDS, S(stream), *ek, *tb, nonce, nonce_len,
                            in, len, out, mac_io, status); }));
    return 0;
}

extern "C" int uaesk_eaxp_macs(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int mode,
                               const void *nonce, size_t nonce_len, const void *ct, size_t len, void *mac_io, void *res48)
{
    if (mode < 0 || mode > 2) return (int)hipErrorInvalidValue;
    DISPATCH_NR(nr, return uaesk_launch(k_eaxp_macs<NR>, 1, mode == 1 ? 128 : 64, ER_LDS, S(stream), *ek, *tb, mode, nonce, nonce_len,
                                        ct, len, mac_io, res48));
    return 0;
}

extern "C" int uaesk_eaxp_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt,
                                const void *nonces, size_t nonce_bytes, const void *nlens, size_t nmsg, size_t msg_bytes,
                                const void *lens, const void *in, void *out, void *macs, void *verdicts, int *bad)
{
    if (nonce_bytes > UINT32_MAX || msg_bytes > UINT32_MAX || (((uintptr_t)lens | (uintptr_t)nlens) & 3u)) return (int)hipErrorInvalidValue;
    if (nmsg == 0) return 0;
    const RowShape s = uaesk_row_shape(nmsg);
    DISPATCH_NR(nr, return with_bool(decrypt, [&](auto DEC) { return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_eaxp_batch<NR, decltype(DEC)::value, decltype(A4)::value>, s.grid, s.wg, E4_LDS, S(stream), *ek, *tb,
                            nonces, nonce_bytes, nlens, nmsg, msg_bytes, lens, in, out, macs, verdicts, bad); }); }));
    return 0;
}

/* ---- the plan (uaes_plan.h) --------------------------------------------------------------------------------------- */
extern "C" int uaesk_plan_eax_siv(int siv, int dir, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((siv != 0 && siv != 1) || (dir != 0 && dir != 1)) return (int)hipErrorInvalidValue;
    if (nmsg > 1) {
        p->arrangement = siv ? UAES_S2V_BATCH : UAES_EAX_BATCH;
        p->launches = 1;
        p->grid = uaesk_row_shape(nmsg).grid;
        return 0;
    }
    p->grid = 1;
    if (len <= UAES_EAX_SIV_SMALL_MAX) {
        p->arrangement = siv ? UAES_S2V_SMALL : UAES_EAX_SMALL;
        p->launches = 1;
        return 0;
    }
    p->arrangement = siv ? UAES_S2V_LONG : UAES_EAX_LONG;
    p->launches = siv ? 2 : dir ? 2 : 3;            /* EAX decrypt: the CTR launch only for an authentic text */
    return 0;
}

/* the _v calls: steps = the rows a call's components are dealt over (a batch record's row walks its own) */
extern "C" int uaesk_plan_siv_v(int dir, size_t len, size_t nad, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || nad > (nmsg > 1 ? UAES_S2V_BATCH_AD_MAX : UAES_S2V_AD_MAX)) return (int)hipErrorInvalidValue;
    if (nmsg > 1) {
        p->arrangement = UAES_S2V_BATCH_V;
        p->launches = 1;
        p->grid = uaesk_row_shape(nmsg).grid;
        p->steps = 1;
        return 0;
    }
    p->grid = 1;
    p->steps = S2V_V_ROWS;
    p->arrangement = len <= UAES_EAX_SIV_SMALL_MAX ? UAES_S2V_SMALL_V : UAES_S2V_LONG_V;
    p->launches = len <= UAES_EAX_SIV_SMALL_MAX ? 1 : 2;
    return 0;
}

/* EAX': the same boundary; a longer encryption is N, CTR, C', a longer decryption N || C' and CTR for an authentic text */
extern "C" int uaesk_plan_eaxp(int dir, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if (dir != 0 && dir != 1) return (int)hipErrorInvalidValue;
    if (nmsg > 1) {
        p->arrangement = UAES_EAXP_BATCH;
        p->launches = 1;
        p->grid = uaesk_row_shape(nmsg).grid;
        return 0;
    }
    p->grid = 1;
    p->arrangement = len <= UAES_EAX_SIV_SMALL_MAX ? UAES_EAXP_SMALL : UAES_EAXP_LONG;
    p->launches = len <= UAES_EAX_SIV_SMALL_MAX ? 1 : dir ? 2 : 3;
    return 0;
}

extern "C" const char *uaesk_eax_siv_arrangement_name(int id)
{
    static const char *const names[] = { "eax.small", "eax.long", "eax.batch", "s2v.small", "s2v.long", "s2v.batch",
                                         "s2v.small.v", "s2v.long.v", "s2v.batch.v", "eaxp.small", "eaxp.long", "eaxp.batch" };
    return id >= 0 && id < 12 ? names[id] : "?";
}
