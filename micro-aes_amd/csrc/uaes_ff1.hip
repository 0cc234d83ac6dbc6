/*
 * uaes_ff1.hip -- FF1 format-preserving encryption, SP 800-38G (FF1_cipher micro_aes.c:2091-2147, FPE_cipher :2267-2314).
 *
 *   k_ff1<16>   many records of one length under one key: sixteen lanes (a DPP row) per record, four records per wave
 *   k_ff1<64>   one text per wave, for the lengths whose slot does not fit beside 63 others
 *
 * A text of len numerals is split into its first u = len / 2 and its last v = len - u.  Ten Feistel rounds; round i
 * adds (decryption, rounds 9..0: subtracts) F_i(the other half) to the first half when i is even and to the second when
 * it is odd, modulo radix^m, m the length of the half it changes.  The halves never move: the swap of the
 * specification is which half a round reads (the reference does the same on one array).  F_i(B):
 *     R = PRF(P | T | 0.. | i | NUM_radix(B) in b bytes)          CBC-MAC under the key, the forward cipher only
 *     S = R | E(R ^ [1]) | E(R ^ [2]) ..                           its first d bytes, as a big-endian number y
 *     STR_m(y mod radix^m)
 * b and d depend on (radix, len) alone; the host passes them in, computed with exact integers (uaesh_ff1_b).  E(P)
 * chained over the tweak's full blocks is the same in all ten rounds: once per record.  A round MACs only the tail --
 * the tweak's last partial block, the zero padding, i, NUM(B) -- with sixteen lanes per block (row_encrypt).
 *
 * The radix arithmetic is the reference's (numRadix, strRadix, addRadix / subRadix: no big-number modulo), spread over
 * the W lanes of a record as two systolic pipelines, exact at every step:
 *   NUM(B)    the number is 16-bit limbs in LDS, least significant first, a run of CL limbs per lane.  Step s (numeral s
 *             of B, most significant first) is N = N * radix + numeral; lane l does step s in iteration s + l, taking
 *             as carry-in what lane l - 1 carried out of the same step one iteration earlier (lane 0: the numeral).
 *   STR_m(y)  fpe_str (uaes_fpe.hip.h) over the d / 2 16-bit words of S, through all W lanes.
 * The digit-wise addition with carry is m steps on lane 0.  How this is spread decides speed only.
 *
 * LDS of a record (a slot): the numerals X[len] (digit values), NS (NUM(B), then the bytes of S), the digits C.  All
 * communication is between lanes of ONE wave, whose LDS operations complete in order: no barrier after the tables are
 * filled, an s_waitcnt (and compiler fence) between phases.  Every loop is bounded by the lengths passed in; no
 * workgroup waits for another.  A record with a byte that is no numeral is computed like any other and not written.
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_fpe.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

extern "C" unsigned uaesh_ff1_minlen(unsigned radix);       /* uaes_host.c */

#define FF1_NS(N, W)   ((N) / 2u + 2u * (W))               /* limbs: <= N/2 + 2W - 2 bytes; S: <= N/2 + 22 */
#define FF1_C(N, W)    ((N) / 2u + (W))                     /* digits: <= N/2 + W - 1 */
#define FF1_SLOT(N, W) ((N) + FF1_NS(N, W) + FF1_C(N, W) + 4u)   /* + 4: neighbouring slots start on different banks */
#define FF1_ROOM16     (160u * 1024u - UAES_LDS_ROW4 - FPE_ALPHA)

static_assert(UAES_FF1_BATCH_MAX >= 64 && (UAES_FF1_BATCH_MAX & (UAES_FF1_BATCH_MAX - 1)) == 0, "a power of two, at least 64");
static_assert((UAES_WG / 16u) * FF1_SLOT((unsigned)UAES_FF1_BATCH_MAX, 16u) <= FF1_ROOM16, "64 records share a workgroup");
static_assert((UAES_WG / 16u) * FF1_SLOT(2u * (unsigned)UAES_FF1_BATCH_MAX, 16u) > FF1_ROOM16, "the largest such power of two");
static_assert(UAES_LDS_ROW + FPE_ALPHA + FF1_SLOT((unsigned)UAES_FF1_MAX, 64u) <= 160u * 1024u, "LDS of one CU");
static_assert(FF1_SLOT((unsigned)UAES_FF1_BATCH_MAX, 16u) % 4u == 0 && UAES_FF1_MAX % 4 == 0, "NS is word aligned");

/* NUM_radix of the n numerals at LDS address src (most significant first) into the limbs at ns: W * cl of them */
template <u32 W>
__device__ __forceinline__ void ff1_num(u32 src, u32 n, u32 radix, u32 ns, u32 cl, u32 li)
{
    const u32 mine = ns + 2u * li * cl;
    for (u32 k = 0; k < cl; ++k) fpe_st16(mine + 2u * k, 0u);
    u32 cout = 0;
    for (u32 it = 0; it < n + W - 1u; ++it) {
        u32 cin = (u32)__shfl_up((int)cout, 1, (int)W);
        if (li == 0) cin = it < n ? fpe_ld8(src + it) : 0u;
        cout = 0;
        if ((int)(it - li) < (int)n) {                      /* before its first step a lane multiplies zeros */
            for (u32 k = 0; k < cl; ++k) {
                const u32 t = fpe_ld16(mine + 2u * k) * radix + cin;
                fpe_st16(mine + 2u * k, t & 0xffffu);
                cin = t >> 16;
            }
            cout = cin;
        }
    }
}

/* W = 16: nrec records back to back, record m's tweak at tweaks + m * stride; W = 64: the same with one record per
 * wave.  verdicts (may be NULL): 1 / 0 per record; *bad |= 1 for a record with a byte that is no numeral, which is
 * left unwritten.  in == out is fine: a record is read whole before it is written. */
template <int NR, u32 W>
__global__ __launch_bounds__(W == 16u ? UAES_WG : 64u) void k_ff1(uaesk_rk rk, uaesk_tables tb, uaesk_ff1 q, int decrypt, u64 nrec,
                                                                 const unsigned char *tweaks, const unsigned char *in,
                                                                 unsigned char *out, unsigned char *verdicts, int *bad)
{
    constexpr u32 NMAX = W == 16u ? (u32)UAES_FF1_BATCH_MAX : (u32)UAES_FF1_MAX;
    constexpr u32 AT = W == 16u ? UAES_LDS_ROW4 : UAES_LDS_ROW;
    fpe_fill_alphabet(AT, q);
    if (W == 16u) row4_fill_tables(tb.te0, rk); else row_fill_tables(tb.te0, rk);        /* ends in a barrier */
    const RowLane<NR> L = W == 16u ? row4_lane<NR>() : row_lane<NR>();
    const u32 grp = threadIdx.x / W, li = threadIdx.x % W, groups = blockDim.x / W;
    const u32 xat = AT + FPE_ALPHA + grp * FF1_SLOT(NMAX, W), ns = xat + NMAX, cd = ns + FF1_NS(NMAX, W);
    const u32 radix = q.radix, len = q.len, u = len / 2u, v = len - u, b = q.b, d = q.d;
    const u32 recip = (u32)((0x100000000ull + radix - 1u) / radix);
    const u64 tfull = q.tweak_len & ~15ull;
    const u32 trem = (u32)(q.tweak_len & 15u), z = (16u - (u32)((q.tweak_len + b + 1u) & 15u)) & 15u, pre = trem + z;
    const u32 nblk = (pre + 1u + b) / 16u, nsb = (d + 15u) / 16u, cl = ((b + 1u) / 2u + W - 1u) / W;
    const bool dec = decrypt != 0;

    for (u64 base = (u64)blockIdx.x * groups; base < nrec; base += (u64)gridDim.x * groups) {
        const bool live = base + grp < nrec;
        const u64 rec = live ? base + grp : 0;              /* a group without a record redoes record 0 and writes nothing */
        const unsigned char *src = in + rec * len, *tw = tweaks + rec * q.tweak_stride;
        const bool foreign = fpe_load<W>(AT, src, len, radix, xat, li);
        const bool good = W == 16u ? !row_any(foreign) : __ballot(foreign) == 0;
        FPE_PHASE();

        u32 y = row_encrypt<NR>(row_pick(q.p, L.c), L);     /* E(P), then the tweak's full blocks */
        for (u64 j = 0; j < tfull; j += 16) y = row_encrypt<NR>(y ^ row_load(tw + j, 16, L.c), L);
        const u32 twtail = trem ? row_load(tw + tfull, trem, L.c) : 0u;

        for (u32 step = 0; step < 10u; ++step) {
            const u32 round = dec ? 9u - step : step, odd = round & 1u;
            const u32 m = odd ? v : u, n = odd ? u : v, xa = xat + (odd ? u : 0u), xb = xat + (odd ? 0u : u);
            ff1_num<W>(xb, n, radix, ns, cl, li);
            FPE_PHASE();
            u32 w = y;
            for (u32 k = 0; k < nblk; ++k) {
                u32 word = k == 0 ? twtail : 0u;
#pragma unroll
                for (u32 j = 0; j < 4u; ++j) {
                    const int tp = (int)(16u * k + 4u * L.c + j) - (int)pre;       /* 0: the round byte; 1..b: NUM(B) */
                    const u32 byte = fpe_ld8(ns + (tp > 0 ? b - (u32)tp : 0u));
                    word |= (tp < 0 ? 0u : tp == 0 ? round : byte) << (8u * j);
                }
                w = row_encrypt<NR>(w ^ word, L);
            }
            FPE_PHASE();
            for (u32 j = 0; j < nsb; ++j) {
                const u32 e = j == 0 ? w : row_encrypt<NR>(w ^ (L.c == 3u ? bswap32(j) : 0u), L);
                if ((li & 3u) == 0) fpe_st32(ns + 16u * j + 4u * L.c, e);
            }
            FPE_PHASE();
            const auto s16 = [ns](u32 s) { return fpe_ld8(ns + 2u * s) << 8 | fpe_ld8(ns + 2u * s + 1u); };
            fpe_str<W>(d / 2u, W, s16, radix, recip, cd, m, li);       /* S = the first d bytes at ns, a big-endian number */
            FPE_PHASE();
            if (li == 0) fpe_add<true>(xa, cd, m, radix, dec);
            FPE_PHASE();
        }

        if (live && good) fpe_store<W>(AT, out + rec * len, len, xat, li);
        row_verdict<true>(live && li == 0, verdicts, rec, good, bad);
        FPE_PHASE();
    }
}

/* ---- the plan (uaes_plan.h) ---------------------------------------------------------------------------------------- */
static int plan_ff1(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if ((dir != 0 && dir != 1) || radix < 2 || radix > 256 || len < uaesh_ff1_minlen(radix) || len > UAES_FF1_MAX)
        return (int)hipErrorInvalidValue;
    p->launches = 1;
    if (nrec == 0) {                                      /* one text: a batch of one, or a wave of its own */
        p->arrangement = len <= UAES_FF1_BATCH_MAX ? UAES_FF1_BATCH : UAES_FF1_WAVE;
        p->grid = 1;
        p->steps = 64;
        return 0;
    }
    if (len > UAES_FF1_BATCH_MAX) return (int)hipErrorInvalidValue;
    const RowShape s = uaesk_row_shape(nrec);
    p->arrangement = UAES_FF1_BATCH;
    p->grid = s.grid;
    p->steps = s.wg;
    return 0;
}

extern "C" int uaesk_plan_ff1(int dir, unsigned radix, size_t len, size_t nrec, uaes_plan *p)
{
    return plan_ff1(dir, radix, len, nrec, p);
}

extern "C" const char *uaesk_ff1_arrangement_name(int id)
{
    static const char *const names[] = { "ff1.batch", "ff1.wave" };
    return id >= 0 && id < 2 ? names[id] : "?";
}

/* ---- launcher -------------------------------------------------------------------------------------------------------- */
template <int NR>
static int launch_ff1(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, int decrypt, const uaesk_ff1 *q,
                      const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad)
{
    uaes_plan p;
    const int e = plan_ff1(decrypt != 0, q->radix, q->len, nrec, &p);
    if (e) return e;
    const u64 n = nrec ? nrec : 1;
    if (p.arrangement == UAES_FF1_WAVE)
        return uaesk_launch(k_ff1<NR, 64u>, p.grid, p.steps, UAES_LDS_ROW + FPE_ALPHA + FF1_SLOT((unsigned)UAES_FF1_MAX, 64u), st,
                            *k, *tb, *q, decrypt, n, tweaks, in, out, verdicts, bad);
    return uaesk_launch(k_ff1<NR, 16u>, p.grid, p.steps,
                        UAES_LDS_ROW4 + FPE_ALPHA + (p.steps / 16u) * FF1_SLOT((unsigned)UAES_FF1_BATCH_MAX, 16u), st,
                        *k, *tb, *q, decrypt, n, tweaks, in, out, verdicts, bad);
}

extern "C" int uaesk_ff1_run(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, int decrypt, const uaesk_ff1 *q,
                             const void *tweaks, size_t nrec, const void *in, void *out, void *verdicts, int *bad)
{
    DISPATCH_NR(nr, return (launch_ff1<NR>(S(stream), tb, ek, decrypt, q, tweaks, nrec, in, out, verdicts, bad)));
    return 0;
}
