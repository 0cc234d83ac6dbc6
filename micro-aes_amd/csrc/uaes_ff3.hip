/*
 * uaes_ff3.hip -- FF3-1 format-preserving encryption, SP 800-38G revision 1 (FF3_cipher micro_aes.c:2150-2248, FPE_cipher
 * :2267-2314 with FF_X 3).
 *
 *   k_ff3   many records of one length under one key: sixteen lanes (a DPP row) per record, four records per wave.
 *           A single call is a batch of one; no text is longer than 192 numerals, so there is no wave-per-text form.
 *
 * A text of len numerals is split into its first u = ceil(len / 2) and its last v = len - u; the tweak is seven bytes,
 * TL = T0 T1 T2 (T3 & F0), TR = T4 T5 T6 (T3 << 4).  Eight Feistel rounds under the key with its bytes reversed (the host
 * reverses it before expansion); round i adds (decryption, rounds 7..0: subtracts) F_i(the other half) to the first half
 * when i is even and to the second when it is odd, modulo radix^m, m the length of the half it changes.  The halves
 * never move (compare k_ff1).  With the specification's REV and REVB folded in everything is little-endian:
 *     block   bytes 0..11 = NUM(the other half), least significant byte first, numeral 0 its least significant digit;
 *             bytes 12..15 = W reversed, W = TR (i even) or TL (i odd) with i XORed into its last byte
 *     y       the forward cipher of that block, read least significant byte first: one AES block per round
 *     half    += / -= y modulo radix^m, digit by digit from numeral 0 with the carry walking forward
 *
 * The radix arithmetic, exact at every step and nothing floating point:
 *   NUM       below 2^96 (radix^m <= 2^96 is what maxlen means): three 32-bit words that EVERY lane of the row
 *             computes for itself by Horner's rule over the numerals in LDS (the same address in sixteen lanes is one
 *             broadcast read); a lane then simply picks the column word of the block it owns.  No communication.
 *   STR_m(y)  fpe_str (uaes_fpe.hip.h) over the 8 16-bit words of y, through the lanes that hold digits only: the
 *             loop is 8 + (those lanes) - 1 iterations.
 *   the sum   m digit steps on lane 0.
 * How this is spread over the lanes decides speed only.
 *
 * LDS of a record (a slot): the numerals X[192] (digit values), the 16-byte block y, the digits C[96], 4 bytes that put
 * neighbouring slots on different banks.  All communication is between lanes of ONE wave, whose LDS operations
 * complete in order: no barrier after the tables are filled, an s_waitcnt (and compiler fence) between phases.  Every
 * loop is bounded by the lengths passed in; no workgroup waits for another.  A record with a byte that is no numeral
 * is computed like any other and not written.
 *
 * gfx950, -O3 (the compiler's resource-usage remark): k_ff3<10> / <12> / <14> use 59 / 60 / 62 VGPRs and 66 SGPRs, no
 * scratch, no spills (8 waves per SIMD by registers).  LDS is dynamic: 151 552 bytes at 1024 threads (row4 tables and
 * round keys 131 328, alphabet 512, 64 slots of 308), 136 768 at 256 threads -- one workgroup per CU either way, so
 * four waves per SIMD in the large shape and one in the small.  Rates (profiles/ff3_rate.md, tools/ff3_rate.py): 2^20
 * 16-digit decimal records in 2.64 ms = 3.97e8 records/s, the FF1 batch of the same shape 5.04 ms in the same run.
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_fpe.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

extern "C" unsigned uaesh_ff1_minlen(unsigned radix);       /* uaes_host.c */
extern "C" size_t uaesh_ff3_maxlen(unsigned radix);

#define FF3_N       192u                                    /* maxlen(2): the longest text */
#define FF3_HALF    (FF3_N / 2u)
#define FF3_SLOT    (FF3_N + 16u + FF3_HALF + 4u)           /* + 4: neighbouring slots start on different banks */
#define FF3_ROOM    (160u * 1024u - UAES_LDS_ROW4 - FPE_ALPHA)

static_assert((UAES_WG / 16u) * FF3_SLOT <= FF3_ROOM, "64 records share a workgroup");
static_assert(FF3_N % 4u == 0 && FF3_SLOT % 4u == 0 && (UAES_LDS_ROW4 + FPE_ALPHA) % 4u == 0, "the block is word aligned");

/* NUM_radix of the n numerals at LDS address src, numeral 0 the least significant, modulo 2^96 (a valid half is below
 * it): n[0] the least significant word.  Every lane computes all of it. */
__device__ __forceinline__ void ff3_num(u32 src, u32 n, u32 radix, u32 (&w)[3])
{
    w[0] = w[1] = w[2] = 0;
    for (u32 k = n; k-- > 0u;) {
        const u64 t0 = (u64)w[0] * radix + fpe_ld8(src + k);
        const u64 t1 = (u64)w[1] * radix + (u32)(t0 >> 32);
        w[0] = (u32)t0;
        w[1] = (u32)t1;
        w[2] = w[2] * radix + (u32)(t1 >> 32);
    }
}

/* nrec records of q.len numerals back to back, record m's tweak (seven bytes) at tweaks + m * q.tweak_stride; rk = the
 * round keys of the byte-reversed key.  verdicts (may be NULL): 1 / 0 per record; *bad |= 1 for a record with a byte
 * that is no numeral, which is left unwritten.  in == out is fine: a record is read whole before it is written. */
template <int NR>
__global__ __launch_bounds__(UAES_WG) void k_ff3(uaesk_rk rk, uaesk_tables tb, uaesk_ff3 q, int decrypt, u64 nrec,
                                                 const unsigned char *tweaks, const unsigned char *in,
                                                 unsigned char *out, unsigned char *verdicts, int *bad)
{
    constexpr u32 AT = UAES_LDS_ROW4;
    fpe_fill_alphabet(AT, q);
    row4_fill_tables(tb.te0, rk);                           /* ends in a barrier */
    const RowLane<NR> L = row4_lane<NR>();
    const u32 grp = threadIdx.x / 16u, li = threadIdx.x % 16u, groups = blockDim.x / 16u;
    const u32 xat = AT + FPE_ALPHA + grp * FF3_SLOT, blk = xat + FF3_N, cd = blk + 16u;
    const u32 radix = q.radix, len = q.len < FF3_N ? q.len : FF3_N, u = (len + 1u) / 2u, v = len - u;
    const u32 recip = (u32)((0x100000000ull + radix - 1u) / radix);
    const bool dec = decrypt != 0;

    for (u64 base = (u64)blockIdx.x * groups; base < nrec; base += (u64)gridDim.x * groups) {
        const bool live = base + grp < nrec;
        const u64 rec = live ? base + grp : 0;              /* a group without a record redoes record 0 and writes nothing */
        const unsigned char *src = in + rec * len, *tw = tweaks + rec * q.tweak_stride;
        const bool good = !row_any(fpe_load<16u>(AT, src, len, radix, xat, li));
        /* bytes 12..15 of the block: W reversed */
        const u32 t3 = tw[3];
        const u32 wr = ((t3 << 4) & 0xffu) | (u32)tw[6] << 8 | (u32)tw[5] << 16 | (u32)tw[4] << 24;
        const u32 wl = (t3 & 0xf0u) | (u32)tw[2] << 8 | (u32)tw[1] << 16 | (u32)tw[0] << 24;
        FPE_PHASE();

        for (u32 step = 0; step < 8u; ++step) {
            const u32 round = dec ? 7u - step : step, odd = round & 1u;
            const u32 m = odd ? v : u, n = odd ? u : v, xa = xat + (odd ? u : 0u), xb = xat + (odd ? 0u : u);
            u32 num[3];
            ff3_num(xb, n, radix, num);
            const u32 word = L.c == 0u ? num[0] : L.c == 1u ? num[1] : L.c == 2u ? num[2] : (odd ? wl : wr) ^ round;
            const u32 y = row_encrypt<NR>(word, L);
            if ((li & 3u) == 0) fpe_st32(blk + 4u * L.c, y);
            FPE_PHASE();
            const u32 per = (m + 15u) / 16u;                 /* y = the 16 bytes at blk, a little-endian number */
            const auto y16 = [blk](u32 s) { return fpe_ld8(blk + 15u - 2u * s) << 8 | fpe_ld8(blk + 14u - 2u * s); };
            fpe_str<16u>(8u, (m + per - 1u) / per, y16, radix, recip, cd, m, li);
            FPE_PHASE();
            if (li == 0) fpe_add<false>(xa, cd, m, radix, dec);
            FPE_PHASE();
        }

        if (live && good) fpe_store<16u>(AT, out + rec * len, len, xat, li);
        row_verdict<true>(live && li == 0, verdicts, rec, good, bad);
        FPE_PHASE();
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
static int plan_ff3(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || radix < 2 || radix > 256 || len < uaesh_ff1_minlen(radix) || len > uaesh_ff3_maxlen(radix))
        return (int)hipErrorInvalidValue;
    const RowShape s = uaesk_row_shape(nrec);              /* one text: a batch of one */
    p->arrangement = UAES_FF3_BATCH;
    p->launches = 1;
    p->grid = nrec ? s.grid : 1;
    p->steps = nrec ? s.wg : 64;
    return 0;
}

extern "C" int uaesk_plan_ff3(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p)
{
    return plan_ff3(dir, radix, len, nrec, p);
}

extern "C" const char *uaesk_ff3_arrangement_name(int id)
{
    return id == UAES_FF3_BATCH ? "ff3.batch" : "?";
}

/* ---- launcher -------------------------------------------------------------------------------------------------------- */
template <int NR>
static int launch_ff3(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, int decrypt, const uaesk_ff3 *q,
                      const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad)
{
    uaes_plan p;
    const int e = plan_ff3(decrypt != 0, q->radix, q->len, nrec, &p);
    if (e) return e;
    return uaesk_launch(k_ff3<NR>, p.grid, p.steps, UAES_LDS_ROW4 + FPE_ALPHA + (p.steps / 16u) * FF3_SLOT, st,
                        *k, *tb, *q, decrypt, nrec ? nrec : 1, tweaks, in, out, verdicts, bad);
}

extern "C" int uaesk_ff3_run(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt, const uaesk_ff3 *q,
                             const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad)
{
    DISPATCH_NR(nr, return (launch_ff3<NR>(S(stream), tb, ek, decrypt, q, tweaks, nrec, in, out, verdicts, bad)));
    return 0;
}
