/*
 * uaes_fpe.hip.h -- what the FF1 and FF3-1 kernels (uaes_ff1.hip, uaes_ff3.hip) share: LDS access by address, the
 * alphabet block, a record's way in and out, STR_m as a systolic pipeline and the digit-wise sum.  W = the lanes of a
 * record.  All communication is between lanes of ONE wave, whose LDS operations complete in order.
 */
#ifndef UAES_FPE_HIP_H_
#define UAES_FPE_HIP_H_
#include "uaes_aes.hip.h"

typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) unsigned short lds_u16;
typedef __attribute__((address_space(3))) u32 lds_u32;

__device__ __forceinline__ u32 fpe_ld8(u32 a) { return *(lds_u8 *)(uintptr_t)a; }
__device__ __forceinline__ void fpe_st8(u32 a, u32 v) { *(lds_u8 *)(uintptr_t)a = (unsigned char)v; }
__device__ __forceinline__ u32 fpe_ld16(u32 a) { return *(lds_u16 *)(uintptr_t)a; }
__device__ __forceinline__ void fpe_st16(u32 a, u32 v) { *(lds_u16 *)(uintptr_t)a = (unsigned short)v; }
__device__ __forceinline__ void fpe_st32(u32 a, u32 v) { *(lds_u32 *)(uintptr_t)a = v; }

/* between two phases: what the wave's lanes stored is what its lanes read next */
#define FPE_PHASE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

#define FPE_ALPHA 512u                                      /* inv[256] | fwd[256] behind the round keys */

/* q = uaesk_ff1 or uaesk_ff3; the workgroup's barrier after the table fill covers it */
template <class Q>
__device__ __forceinline__ void fpe_fill_alphabet(u32 at, const Q &q)
{
    for (u32 i = threadIdx.x; i < FPE_ALPHA; i += blockDim.x) fpe_st8(at + i, i < 256u ? q.inv[i] : q.fwd[i - 256u]);
}

/* the record's len bytes at src as digit values at xat; true: a byte is no numeral */
template <u32 W>
__device__ __forceinline__ bool fpe_load(u32 at, const unsigned char *src, u32 len, u32 radix, u32 xat, u32 li)
{
    bool foreign = false;
    for (u32 i = li; i < len; i += W) {
        const u32 dg = fpe_ld8(at + src[i]);
        foreign |= dg >= radix;
        fpe_st8(xat + i, dg);
    }
    return foreign;
}

/* the digit values at xat as the alphabet's bytes at dst */
template <u32 W>
__device__ __forceinline__ void fpe_store(u32 at, unsigned char *dst, u32 len, u32 xat, u32 li)
{
    for (u32 i = li; i < len; i += W) dst[i] = (unsigned char)fpe_ld8(at + 256u + fpe_ld8(xat + i));
}

/* STR_m: a number of nw 16-bit words, word(s) its s-th most significant, modulo radix^m, as m digits at cd, least
 * significant first, a run of ceil(m / W) per lane.  Step s is D = D * 65536 + word(s) in radix-radix digits; lane l
 * does step s in iteration s + l, taking as carry-in what lane l - 1 carried out of the same step one iteration
 * earlier.  depth = the lanes the pipeline runs through, at least those that hold digits.  The carry out of digit
 * m - 1 is dropped: the reduction modulo radix^m.  A digit step divides by the radix with a reciprocal (radix <= 256,
 * the dividend below 2^25: the estimate is at most one too large, and is corrected). */
template <u32 W, class Word>
__device__ __forceinline__ void fpe_str(u32 nw, u32 depth, Word word, u32 radix, u32 recip, u32 cd, u32 m, u32 li)
{
    const u32 per = (m + W - 1u) / W, lo = li * per;
    const u32 cnt = lo < m ? (m - lo < per ? m - lo : per) : 0u;
    const u32 mine = cd + lo;
    for (u32 k = 0; k < cnt; ++k) fpe_st8(mine + k, 0u);
    u32 cout = 0;
    for (u32 it = 0; it < nw + depth - 1u; ++it) {
        u32 cin = (u32)__shfl_up((int)cout, 1, (int)W);
        if (li == 0) cin = it < nw ? word(it) : 0u;
        cout = 0;
        if ((int)(it - li) < (int)nw) {                     /* before its first step a lane divides zeros */
            u32 x = cin;                                    /* below 2^17 */
            for (u32 k = 0; k < cnt; ++k) {
                x += fpe_ld8(mine + k) << 16;
                u32 q = __umulhi(x, recip), r = x - q * radix;
                if ((int)r < 0) { --q; r += radix; }
                fpe_st8(mine + k, r);
                x = q;
            }
            cout = x;
        }
    }
}

/* X[xa .. xa + m) += / -= the digits at cd (least significant first), modulo radix^m (addRadix / subRadix); one lane.
 * MSF: X has its most significant numeral first (FF1), else its least (FF3-1). */
template <bool MSF>
__device__ __forceinline__ void fpe_add(u32 xa, u32 cd, u32 m, u32 radix, bool dec)
{
    int carry = 0;
    for (u32 p = 0; p < m; ++p) {
        const u32 at = MSF ? xa + m - 1u - p : xa + p;
        int t = (int)fpe_ld8(at) + (dec ? -(int)fpe_ld8(cd + p) - carry : (int)fpe_ld8(cd + p) + carry);
        carry = dec ? t < 0 : t >= (int)radix;
        if (carry) t += dec ? (int)radix : -(int)radix;
        fpe_st8(at, (u32)t);
    }
}

#endif
