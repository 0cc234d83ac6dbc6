/*
 * uaes_poly1305.hip -- Poly1305-AES (AES_Poly1305, micro_aes.c:1901-1997): a block-parallel MAC on the VALU.
 *
 *   mac = (h + AES_k(nonce)) mod 2^128,  h = sum_{i=1..q} c_i r^(q-i+1) mod p,  p = 2^130 - 5,
 *   c_i = the i-th 16-byte block as a little-endian integer + 2^(8 len_i)   (len_i = 16 but for the last block)
 *
 * Block positions are counted from the END: block e (e = 0 the last) carries r^(e+1).  A lane g of G takes the blocks
 * e = g, g + G, g + 2G, ... and runs Horner from its highest e down with the multiplier r^G, so it ends with
 * sum_j c_(g+jG) r^(jG); weighted by r^(g+1) that is exactly its share of h, whatever the length -- no lane needs to
 * know how many blocks the others have.  Powers are made where they are needed, by square-and-multiply from r.
 *
 *   poly.small    k_poly_small: one workgroup, G = 256, weights r^(t+1), s = AES_k(nonce), the tag      (1 launch)
 *   poly.chunks   k_poly_chunks: G = grid x 256, each workgroup stores sum_t acc_t r^(t+1) = P_w;
 *                 k_poly_fold: sum_w P_w r^(256 w), + s, the tag; zeroes the partials             (2 launches)
 *   poly.batch    k_poly_batch: one wave per message (G = 64), equal lengths back to back, a nonce each (1 launch)
 *
 * Arithmetic: five 26-bit limbs in u32, products and sums in u64 (v_mad_u64_u32); DESIGN.md section 5 has the
 * measured issue costs that chose it over an f64-limb form.
 */
#include <hip/hip_runtime.h>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

#define PT 256u                                   /* threads per workgroup of the one-message kernels */
#define M26 0x3ffffffu

/* the one-workgroup arrangement up to this many bytes (profiles/r07_poly1305_sweep.log: the size sweep
 * of both arrangements); a build may move it (XFLAGS=-DUAES_POLY_SMALL_MAX=...) to measure the other side */
#ifndef UAES_POLY_SMALL_MAX
#define UAES_POLY_SMALL_MAX ((size_t)128 << 10)
#endif
#define POLY_MIN_STEPS  8u                        /* poly.chunks: blocks per lane at least, before the grid grows */
#define POLY_WG_PER_CU  8u                        /* ... and at most this many workgroups per CU                 */

/* a value mod p in five 26-bit limbs, least significant first */
struct P5 {
    u32 v[5];
};
struct PolyR {                                    /* kernel argument: the clamped r, in limbs */
    u32 v[5];
};

__device__ __forceinline__ P5 p5_of(const PolyR &r)
{
    P5 x;
#pragma unroll
    for (int i = 0; i < 5; ++i) x.v[i] = r.v[i];
    return x;
}

__device__ __forceinline__ P5 p5_one()
{
    P5 x = { { 1u, 0u, 0u, 0u, 0u } };
    return x;
}

/* h * m mod p, lazily reduced.
 *
 * Bound.  The usual donna-32 argument leans on a CLAMPED r (limbs 1..4 below 2^24 or so).  Here the multiplier is
 * r^S for a lane stride S -- a product of this function, not clamped, and itself only lazily reduced -- and the
 * accumulator has a block (or a second partial) added on top.  So take the loosest inputs that occur:
 *   multiplier limbs m_k < 2^27 (r itself, or an output of this function: limbs < 2^26, limb 1 < 2^26 + 2^11),
 *   accumulator limbs h_j < 2^28 (an output + a block or a partial: < 2^26 + 2^11 + 2^26).
 * Every product h_j * m_k or h_j * 5 m_k is < 2^28 * 5 * 2^27 < 2^57.33; a d_i sums five of them: < 2^59.66, and
 * the carry it takes in is < 2^34, so no d_i reaches 2^60 < 2^64.  The carry out of d4 is < 2^34, times 5 < 2^36.4,
 * added to a 26-bit h0 in u64; what that pushes into h1 is < 2^11.  Result: limbs 0, 2, 3, 4 < 2^26, limb 1
 * < 2^26 + 2^11, value < 2^130 + 2^37 -- congruent to h*m mod p, not reduced below p (p_finish does that).
 * tests/test_gpu_poly1305.py drives it with r bytes all 0xff (the largest clamped r), all-0xff messages and
 * exponents up to 2^28 blocks.                                                                              */
__device__ __forceinline__ P5 p_mul(const P5 &h, const P5 &m)
{
    const u32 m0 = m.v[0], m1 = m.v[1], m2 = m.v[2], m3 = m.v[3], m4 = m.v[4];
    const u32 s1 = m1 * 5u, s2 = m2 * 5u, s3 = m3 * 5u, s4 = m4 * 5u;       /* < 2^29.4: u32 */
    const u32 h0 = h.v[0], h1 = h.v[1], h2 = h.v[2], h3 = h.v[3], h4 = h.v[4];
    u64 d0 = (u64)h0 * m0 + (u64)h1 * s4 + (u64)h2 * s3 + (u64)h3 * s2 + (u64)h4 * s1;
    u64 d1 = (u64)h0 * m1 + (u64)h1 * m0 + (u64)h2 * s4 + (u64)h3 * s3 + (u64)h4 * s2;
    u64 d2 = (u64)h0 * m2 + (u64)h1 * m1 + (u64)h2 * m0 + (u64)h3 * s4 + (u64)h4 * s3;
    u64 d3 = (u64)h0 * m3 + (u64)h1 * m2 + (u64)h2 * m1 + (u64)h3 * m0 + (u64)h4 * s4;
    u64 d4 = (u64)h0 * m4 + (u64)h1 * m3 + (u64)h2 * m2 + (u64)h3 * m1 + (u64)h4 * m0;
    P5 o;
    d1 += d0 >> 26; o.v[0] = (u32)d0 & M26;
    d2 += d1 >> 26; o.v[1] = (u32)d1 & M26;
    d3 += d2 >> 26; o.v[2] = (u32)d2 & M26;
    d4 += d3 >> 26; o.v[3] = (u32)d3 & M26;
    const u64 t = (u64)o.v[0] + (d4 >> 26) * 5u;
    o.v[4] = (u32)d4 & M26;
    o.v[0] = (u32)t & M26;
    o.v[1] += (u32)(t >> 26);
    return o;
}

/* a + b for two lazily reduced values (limbs < 2^26 + 2^11), carried back to the same form */
__device__ __forceinline__ P5 p_add(const P5 &a, const P5 &b)
{
    P5 o;
    u32 c;
    o.v[0] = a.v[0] + b.v[0];
    o.v[1] = a.v[1] + b.v[1] + (o.v[0] >> 26); o.v[0] &= M26;
    o.v[2] = a.v[2] + b.v[2] + (o.v[1] >> 26); o.v[1] &= M26;
    o.v[3] = a.v[3] + b.v[3] + (o.v[2] >> 26); o.v[2] &= M26;
    o.v[4] = a.v[4] + b.v[4] + (o.v[3] >> 26); o.v[3] &= M26;
    c = o.v[4] >> 26; o.v[4] &= M26;
    o.v[0] += c * 5u;
    o.v[1] += o.v[0] >> 26; o.v[0] &= M26;
    return o;
}

/* a + b without the carries: the Horner step (an output of p_mul plus a block or a partial, limbs < 2^28) */
__device__ __forceinline__ P5 p_add_lazy(const P5 &a, const P5 &b)
{
    P5 o;
#pragma unroll
    for (int i = 0; i < 5; ++i) o.v[i] = a.v[i] + b.v[i];
    return o;
}

/* r^e, e >= 0 */
__device__ __forceinline__ P5 p_pow(const P5 &r, u64 e)
{
    P5 x = p5_one(), b = r;
    while (e) {
        if (e & 1u) x = p_mul(x, b);
        e >>= 1;
        if (e) b = p_mul(b, b);
    }
    return x;
}

/* a 16-byte block (little-endian words) + hibit * 2^128 -> limbs */
__device__ __forceinline__ P5 p_block(uint4 w, u32 hibit)
{
    P5 c;
    c.v[0] = w.x & M26;
    c.v[1] = ((w.x >> 26) | (w.y << 6)) & M26;
    c.v[2] = ((w.y >> 20) | (w.z << 12)) & M26;
    c.v[3] = ((w.z >> 14) | (w.w << 18)) & M26;
    c.v[4] = (w.w >> 8) | (hibit << 24);
    return c;
}

template <bool A16>
__device__ __forceinline__ uint4 ld16(const unsigned char *p)
{
    if (A16) return *(const uint4 *)p;
    u32 w[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (u32 i = 0; i < 16; ++i) w[i >> 2] |= (u32)p[i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

/* the last block when it is partial: its rem bytes, then a 1 (c = m + 2^(8 rem)), no 2^128 */
__device__ __forceinline__ P5 p_tail(const unsigned char *p, u32 rem)
{
    u32 w[4] = { 0, 0, 0, 0 };
#pragma unroll                                    /* constant word indices: w stays in registers */
    for (u32 i = 0; i < 16; ++i) {
        const u32 b = i < rem ? (u32)p[i < rem ? i : 0] : i == rem ? 1u : 0u;
        w[i >> 2] |= b << (8 * (i & 3));
    }
    return p_block(make_uint4(w[0], w[1], w[2], w[3]), 0u);
}

/* Lane g of G over the q blocks of [data, data + len): sum_j c_(g+jG) r^(jG), e counted from the end.
 * RG = r^G.  The lane's blocks, first to last in memory, are 16 G bytes apart; four are requested at a time. */
template <bool A16>
__device__ __forceinline__ P5 lane_horner(const unsigned char *data, u64 len, u64 g, u64 G, const P5 &RG)
{
    P5 acc = { { 0, 0, 0, 0, 0 } };
    const u64 q = (len + 15) >> 4;
    if (g >= q) return acc;
    const u32 rem = (u32)(len & 15u);
    u64 n = (q - 1 - g) / G + 1;                  /* this lane's blocks */
    const bool tail = g == 0 && rem != 0;         /* e = 0 is the partial last block: done after the loop */
    if (tail) --n;
    const unsigned char *p = data + 16 * (q - 1 - g - (n - 1 + (tail ? 1 : 0)) * G);
    const u64 step = 16 * G;
    for (; n >= 4; n -= 4) {
        const uint4 w0 = ld16<A16>(p), w1 = ld16<A16>(p + step), w2 = ld16<A16>(p + 2 * step), w3 = ld16<A16>(p + 3 * step);
        p += 4 * step;
        acc = p_add_lazy(p_mul(acc, RG), p_block(w0, 1u));
        acc = p_add_lazy(p_mul(acc, RG), p_block(w1, 1u));
        acc = p_add_lazy(p_mul(acc, RG), p_block(w2, 1u));
        acc = p_add_lazy(p_mul(acc, RG), p_block(w3, 1u));
    }
    for (; n; --n, p += step) acc = p_add_lazy(p_mul(acc, RG), p_block(ld16<A16>(p), 1u));
    if (tail) acc = p_add_lazy(p_mul(acc, RG), p_tail(data + 16 * (q - 1), rem));
    return acc;
}

/* sum over the 64 lanes of a wave (every lane gets it) */
__device__ __forceinline__ P5 wave_sum(P5 x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        P5 y;
#pragma unroll
        for (int i = 0; i < 5; ++i) y.v[i] = (u32)__shfl_xor((int)x.v[i], m, 64);
        x = p_add(x, y);
    }
    return x;
}

/* sum over the workgroup (blockDim.x = PT); the result is valid in thread 0 */
__device__ __forceinline__ P5 block_sum(P5 x, u32 (*sh)[5])
{
    x = wave_sum(x);
    const u32 wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) sh[wv][i] = x.v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 k = 1; k < PT / 64u; ++k) {
            P5 y;
#pragma unroll
            for (int i = 0; i < 5; ++i) y.v[i] = sh[k][i];
            x = p_add(x, y);
        }
    }
    return x;
}

/* fully reduce h into [0, p), add s mod 2^128, store the 16 bytes */
__device__ __forceinline__ void p_finish(P5 h, const u32 (&s)[4], unsigned char *mac)
{
    u32 c;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {        /* h < 2^130 afterwards, every limb < 2^26 */
        h.v[1] += h.v[0] >> 26; h.v[0] &= M26;
        h.v[2] += h.v[1] >> 26; h.v[1] &= M26;
        h.v[3] += h.v[2] >> 26; h.v[2] &= M26;
        h.v[4] += h.v[3] >> 26; h.v[3] &= M26;
        c = h.v[4] >> 26; h.v[4] &= M26;
        h.v[0] += c * 5u;
    }
    h.v[1] += h.v[0] >> 26; h.v[0] &= M26;        /* (the second pass carried at most 5 into a limb below 2^26) */
    /* g = h + 5 - 2^130: h >= p exactly when that does not borrow, and then h - p = g */
    u32 g[5];
    g[0] = h.v[0] + 5u;           c = g[0] >> 26; g[0] &= M26;
    g[1] = h.v[1] + c;            c = g[1] >> 26; g[1] &= M26;
    g[2] = h.v[2] + c;            c = g[2] >> 26; g[2] &= M26;
    g[3] = h.v[3] + c;            c = g[3] >> 26; g[3] &= M26;
    g[4] = h.v[4] + c - (1u << 26);
    const u32 keep_g = (g[4] >> 31) - 1u;          /* all ones when no borrow */
#pragma unroll
    for (int i = 0; i < 5; ++i) h.v[i] = (h.v[i] & ~keep_g) | (g[i] & keep_g);
    const u32 w0 = h.v[0] | (h.v[1] << 26);
    const u32 w1 = (h.v[1] >> 6) | (h.v[2] << 20);
    const u32 w2 = (h.v[2] >> 12) | (h.v[3] << 14);
    const u32 w3 = (h.v[3] >> 18) | (h.v[4] << 8);
    u64 t = (u64)w0 + s[0];
    u32 o[4];
    o[0] = (u32)t; t = (t >> 32) + w1 + s[1];
    o[1] = (u32)t; t = (t >> 32) + w2 + s[2];
    o[2] = (u32)t; t = (t >> 32) + w3 + s[3];
    o[3] = (u32)t;
#pragma unroll
    for (u32 i = 0; i < 16; ++i) mac[i] = (unsigned char)(o[i >> 2] >> (8 * (i & 3)));
}

/* s = AES_k(nonce), one block through a plain copy of Te0 (every lane of the calling wave reads the same entries) */
template <int NR>
__device__ __forceinline__ void aes_nonce(const u32 *te, const uaesk_rk &rk, uint4 nonce, u32 (&s)[4])
{
    s[0] = nonce.x; s[1] = nonce.y; s[2] = nonce.z; s[3] = nonce.w;
    plain_encrypt<NR>(te, rk, s);
}

__device__ __forceinline__ void load_te(u32 *te, const u32 *te0)
{
    for (u32 i = threadIdx.x; i < 256u; i += blockDim.x) te[i] = te0[i];
}

/* poly.small: the whole message in one workgroup, the tag at the end */
template <int NR, bool A16>
__global__ __launch_bounds__(PT) void k_poly_small(uaesk_rk rk, const u32 *__restrict__ te0, PolyR rr, uint4 nonce,
                                                   const unsigned char *__restrict__ data, u64 len,
                                                   unsigned char *__restrict__ mac)
{
    __shared__ u32 te[256];
    __shared__ u32 sh[PT / 64u][5];
    load_te(te, te0);
    const P5 r = p5_of(rr);
    const P5 RG = p_pow(r, PT);
    P5 acc = lane_horner<A16>(data, len, threadIdx.x, PT, RG);
    acc = p_mul(acc, p_pow(r, threadIdx.x + 1u));
    __syncthreads();                              /* te[] */
    acc = block_sum(acc, sh);
    if (threadIdx.x < 64u) {
        u32 s[4];
        aes_nonce<NR>(te, rk, nonce, s);
        if (threadIdx.x == 0) p_finish(acc, s, mac);
    }
}

/* poly.chunks, first launch: workgroup w stores P_w = sum_t acc_(256 w + t) r^(t+1) (5 words in a 32-byte slot) */
template <bool A16>
__global__ __launch_bounds__(PT) void k_poly_chunks(PolyR rr, const unsigned char *__restrict__ data, u64 len,
                                                    u32 *__restrict__ partial)
{
    __shared__ u32 sh[PT / 64u][5];
    const P5 r = p5_of(rr);
    const u64 G = (u64)gridDim.x * PT;
    const P5 RG = p_pow(r, G);
    P5 acc = lane_horner<A16>(data, len, (u64)blockIdx.x * PT + threadIdx.x, G, RG);
    acc = p_mul(acc, p_pow(r, threadIdx.x + 1u));
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) partial[8u * blockIdx.x + i] = acc.v[i];
    }
}

/* poly.chunks, second launch: h = sum_w P_w r^(256 w) -- the same strided Horner over the partials (thread u takes
 * w = u, u + 256, ... with the multiplier r^(256 * 256), weight r^(256 u)) -- then the tag.  The partials are zeroed
 * behind the reads: nothing derived from r stays in the scratch. */
template <int NR>
__global__ __launch_bounds__(PT) void k_poly_fold(uaesk_rk rk, const u32 *__restrict__ te0, PolyR rr, uint4 nonce,
                                                  u32 *__restrict__ partial, u32 nparts, unsigned char *__restrict__ mac)
{
    __shared__ u32 te[256];
    __shared__ u32 sh[PT / 64u][5];
    load_te(te, te0);
    const P5 r = p5_of(rr);
    const P5 RG = p_pow(r, (u64)PT * PT);
    P5 acc = { { 0, 0, 0, 0, 0 } };
    if (threadIdx.x < nparts) {
        const u32 n = (nparts - 1u - threadIdx.x) / PT + 1u;
#pragma unroll 8                                  /* no store between the loads: they are all in flight at once */
        for (u32 k = n; k-- > 0;) {
            const u32 *p = partial + 8u * (threadIdx.x + k * PT);
            P5 y;
#pragma unroll
            for (int i = 0; i < 5; ++i) y.v[i] = p[i];
            acc = p_add_lazy(p_mul(acc, RG), y);
        }
        for (u32 k = 0; k < n; ++k) {
#pragma unroll
            for (int i = 0; i < 5; ++i) partial[8u * (threadIdx.x + k * PT) + i] = 0u;
        }
        acc = p_mul(acc, p_pow(r, (u64)PT * threadIdx.x));
    }
    __syncthreads();                              /* te[] */
    acc = block_sum(acc, sh);
    if (threadIdx.x < 64u) {
        u32 s[4];
        aes_nonce<NR>(te, rk, nonce, s);
        if (threadIdx.x == 0) p_finish(acc, s, mac);
    }
}

/* poly.batch: message m = msg_bytes at data + m msg_bytes, nonce at nonces + 16 m, tag to macs + 16 m; one wave per
 * message, waves walk the messages grid-strided.  The lane weights r^(t+1) and the stride r^64 are made once. */
template <int NR, bool A16>
__global__ __launch_bounds__(PT) void k_poly_batch(uaesk_rk rk, const u32 *__restrict__ te0, PolyR rr,
                                                   const unsigned char *__restrict__ nonces, u64 nmsg, u64 msg_bytes,
                                                   const unsigned char *__restrict__ data, unsigned char *__restrict__ macs)
{
    __shared__ u32 te[256];
    load_te(te, te0);
    __syncthreads();
    const u32 lane = threadIdx.x & 63u;
    const P5 r = p5_of(rr);
    const P5 R64 = p_pow(r, 64u);
    const P5 W = p_pow(r, lane + 1u);
    const u64 waves = (u64)gridDim.x * (PT / 64u);
    for (u64 m = (u64)blockIdx.x * (PT / 64u) + (threadIdx.x >> 6); m < nmsg; m += waves) {
        P5 acc = lane_horner<A16>(data + m * msg_bytes, msg_bytes, lane, 64u, R64);
        acc = wave_sum(p_mul(acc, W));
        const unsigned char *nb = nonces + 16 * m;
        u32 s[4];
        aes_nonce<NR>(te, rk, ld16<false>(nb), s);
        if (lane == 0) p_finish(acc, s, macs + 16 * m);
    }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* planning and launching                                                                                             */
/* ---------------------------------------------------------------------------------------------------------------- */
extern "C" int uaesk_plan_poly1305(size_t len, size_t nmsg, uaes_plan *p)
{
    const u64 q = ((u64)len + 15) >> 4;
    memset(p, 0, sizeof *p);
    if (nmsg > 1) {
        const u64 cap = (u64)uaesk_cus_or_256() * POLY_WG_PER_CU;
        const u64 want = ((u64)nmsg + PT / 64u - 1) / (PT / 64u);          /* a wave per message */
        p->arrangement = UAES_POLY_BATCH;
        p->launches = 1;
        p->grid = (unsigned)(want < cap ? want : cap);
        p->steps = (unsigned)((q + 63) / 64);
        return 0;
    }
    if (len <= UAES_POLY_SMALL_MAX) {
        p->arrangement = UAES_POLY_SMALL;
        p->launches = 1;
        p->grid = 1;
        p->steps = (unsigned)((q + PT - 1) / PT);
        return 0;
    }
    const u64 cap = (u64)uaesk_cus_or_256() * POLY_WG_PER_CU;
    u64 want = (q + (u64)PT * POLY_MIN_STEPS - 1) / ((u64)PT * POLY_MIN_STEPS);
    if (want > cap) want = cap;
    if (want < 2) want = 2;
    p->arrangement = UAES_POLY_CHUNKS;
    p->launches = 2;
    p->grid = (unsigned)want;
    p->steps = (unsigned)((q + want * PT - 1) / (want * PT));
    return 0;
}

extern "C" const char *uaesk_poly1305_arrangement_name(int id)
{
    static const char *const names[] = { "poly.small", "poly.chunks", "poly.batch" };
    return id >= 0 && id < 3 ? names[id] : "?";
}

extern "C" size_t uaesk_poly1305_scratch_bytes(size_t len)
{
    uaes_plan p;
    uaesk_plan_poly1305(len, 1, &p);
    return p.arrangement == UAES_POLY_CHUNKS ? (size_t)p.grid * 32u : 0;
}

/* the clamped r (micro_aes.c:1971-1976) in 26-bit limbs */
static PolyR clamp_r(const uint8_t r16[16])
{
    uint8_t b[16];
    memcpy(b, r16, 16);
    b[3] &= 15; b[7] &= 15; b[11] &= 15; b[15] &= 15;
    b[4] &= 252; b[8] &= 252; b[12] &= 252;
    u32 w[4];
    memcpy(w, b, 16);
    PolyR r;
    r.v[0] = w[0] & M26;
    r.v[1] = ((w[0] >> 26) | (w[1] << 6)) & M26;
    r.v[2] = ((w[1] >> 20) | (w[2] << 12)) & M26;
    r.v[3] = ((w[2] >> 14) | (w[3] << 18)) & M26;
    r.v[4] = w[3] >> 8;
    volatile uint8_t *vb = b;
    for (int i = 0; i < 16; ++i) vb[i] = 0;
    volatile u32 *vw = w;
    for (int i = 0; i < 4; ++i) vw[i] = 0;
    return r;
}

static void wipe_r(PolyR *r)
{
    volatile u32 *v = r->v;
    for (int i = 0; i < 5; ++i) v[i] = 0;
}

template <int NR>
static int launch_one(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const PolyR &r, uint4 nonce,
                      const unsigned char *data, u64 len, unsigned char *mac, u32 *partial, const uaes_plan &p)
{
    const bool a16 = (((uintptr_t)data) & 15u) == 0;
    if (p.arrangement == UAES_POLY_SMALL)
        return with_bool(a16, [&](auto A16) {
            return uaesk_launch(k_poly_small<NR, decltype(A16)::value>, 1, PT, 0, st, *ek, tb->te0, r, nonce, data, len, mac); });
    const int rc = with_bool(a16, [&](auto A16) {
        return uaesk_launch(k_poly_chunks<decltype(A16)::value>, p.grid, PT, 0, st, r, data, len, partial); });
    if (rc) return rc;
    return uaesk_launch(k_poly_fold<NR>, 1, PT, 0, st, *ek, tb->te0, r, nonce, partial, p.grid, mac);
}

/* one message: data / mac16 / scratch device memory (scratch: uaesk_poly1305_scratch_bytes(len), may be NULL when
 * that is 0); r16 = the r half of the key pair and nonce16 HOST memory (they travel as launch arguments) */
extern "C" int uaesk_poly1305(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uint8_t *r16,
                              const uint8_t *nonce16, const void *data, size_t len, void *mac16, void *scratch)
{
    uaes_plan p;
    uaesk_plan_poly1305(len, 1, &p);
    if ((p.arrangement == UAES_POLY_CHUNKS && !scratch) || (nr != 10 && nr != 12 && nr != 14)) return (int)hipErrorInvalidValue;
    uint4 nonce;
    memcpy(&nonce, nonce16, 16);
    PolyR r = clamp_r(r16);
    int rc;
    DISPATCH_NR(nr, rc = (launch_one<NR>(S(stream), tb, ek, r, nonce, (const unsigned char *)data, (u64)len,
                                         (unsigned char *)mac16, (u32 *)scratch, p)));
    wipe_r(&r);
    return rc;
}

template <int NR>
static int launch_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const PolyR &r, const unsigned char *nonces,
                        u64 nmsg, u64 msg_bytes, const unsigned char *data, unsigned char *macs, unsigned grid)
{
    const bool a16 = ((((uintptr_t)data) | msg_bytes) & 15u) == 0;
    return with_bool(a16, [&](auto A16) {
        return uaesk_launch(k_poly_batch<NR, decltype(A16)::value>, grid, PT, 0, st, *ek, tb->te0, r, nonces, nmsg, msg_bytes, data, macs); });
}

/* nmsg messages of msg_bytes each, back to back; nonces (16 bytes each), data and macs device memory */
extern "C" int uaesk_poly1305_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uint8_t *r16,
                                    const void *nonces, size_t nmsg, size_t msg_bytes, const void *data, void *macs)
{
    if (nmsg == 0) return 0;
    if (nr != 10 && nr != 12 && nr != 14) return (int)hipErrorInvalidValue;      /* (before r is made: DISPATCH_NR) */
    uaes_plan p;
    uaesk_plan_poly1305(msg_bytes, nmsg < 2 ? 2 : nmsg, &p);
    PolyR r = clamp_r(r16);
    int rc;
    DISPATCH_NR(nr, rc = (launch_batch<NR>(S(stream), tb, ek, r, (const unsigned char *)nonces, (u64)nmsg, (u64)msg_bytes,
                                           (const unsigned char *)data, (unsigned char *)macs, p.grid)));
    wipe_r(&r);
    return rc;
}
