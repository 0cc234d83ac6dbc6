/*
 * uaes_cipher_batch.hip -- batches of the plain cipher modes: many records under one key in one launch, an IV (CTR: a
 * first counter block) per record.
 *
 *   CBC decrypt with the CS3 swap          the inverse of uaes_cbc_encrypt_batch       (micro_aes.c:746-782)
 *   CBC over whole blocks, no swap         both directions, a CTS 0 build's CBC        (micro_aes.c:704-733, :753-761)
 *   CFB encrypt / decrypt, OFB             any length                                  (micro_aes.c:799-845, :861-893)
 *   CTR                                    any length, the 56-bit counter of incBlock  (micro_aes.c:421-427, :962-990)
 *
 * One kernel, k_cipher_batch, a row batch (uaes_plan.h): sixteen lanes per record, four records per wave, the row4
 * tables of uaes_aes.hip.h, the launch shape of uaesk_row_shape and a grid-stride loop over the records, so any
 * number of records is one launch.  A record is bit for bit what the one-message call of its mode gives for it.
 */
#include <hip/hip_runtime.h>
#include <type_traits>
#include <string.h>
#include "uaes_aes.hip.h"
#include "uaes_device.h"
#include "uaes_plan.h"

/* the counter block of CTR as column words: bytes 0..8 are ctr0's and never change, bytes 9..15 hold the big-endian
 * 56-bit counter v (make_ctr, uaes_engine.c); w0 = this lane's column of ctr0 */
__device__ __forceinline__ u32 cb_ctr_column(u32 w0, u64 v, u32 c)
{
    if (c < 2u) return w0;
    if (c == 2u) return (w0 & 0xffu) | bswap32((u32)(v >> 32));         /* v < 2^56: the low byte of the swap is zero */
    return bswap32((u32)v);
}

/* Record m: text at in / out + m msg_bytes, its first lens[m] <= msg_bytes bytes (lens NULL: all of it; the CBC modes
 * have no lens and take whole blocks), IV or first counter block at ivs + 16 m (any byte offset).  rk = the encryption
 * schedule, for the two inverse modes the equivalent-inverse one (the tables follow).  Row steps per record of b whole
 * blocks and a ragged one (r = 0 / 1):
 *   CBC encrypt over blocks, CFB encrypt, OFB   b + r        one block per step, each waits for the one before
 *   CBC decrypt over blocks                     ceil(b / 2)  two blocks per step (row_decrypt2)
 *   CBC decrypt with the swap                   ceil((b - 2) / 2) + 1 for b >= 2 (the swapped pair is a step of its
 *                                               own), 1 for b = 1
 *   CFB decrypt, CTR                            ceil((b + r) / 2): two blocks per step (row_encrypt2), a last odd block
 *                                               rides with the ragged one
 * in == out works in every mode: a block is in registers before its place is written -- row_walk asks for the text a
 * chunk ahead, the paired modes keep the previous ciphertext block (CBC, CFB) in a register, and the swapped pair of
 * CS3 and the ragged block are read before the record's first store.  Every instance walks with row_walk's full
 * look-ahead (ROW_CH): with it the widest one, OFB, takes 95 of the 128 registers a 16-wave workgroup has, and none has
 * scratch (profiles/cipher_batch_resources.txt).  A4: every record 4-byte aligned in both texts. */
template <int NR, int MODE, bool A4>
__global__ __launch_bounds__(UAES_WG) void k_cipher_batch(uaesk_rk rk, uaesk_tables tb, const unsigned char *ivs,
                                                          u64 nmsg, u64 msg_bytes, const u32 *lens,
                                                          const unsigned char *in, unsigned char *out)
{
    constexpr bool INV = MODE == UAES_CB_CBC_DEC || MODE == UAES_CB_CBC_DEC_BLOCKS;           /* runs AES^-1 */
    if (INV) row4_fill_tables_dec(tb.td0, rk); else row4_fill_tables(tb.te0, rk);
    const RowLane<NR> L = row4_lane<NR>();
    const u32 c = L.c;
    const u64 rows = blockDim.x >> 4;
    for (u64 m = (u64)blockIdx.x * rows + (threadIdx.x >> 4); m < nmsg; m += (u64)gridDim.x * rows) {
        u64 len = msg_bytes;
        if (lens) { const u64 l = lens[m]; if (l < len) len = l; }
        const unsigned char *src = in + m * msg_bytes;
        unsigned char *dst = out + m * msg_bytes;
        u32 v = row_load(ivs + 16 * m, 16, c);                /* the IV / ctr0: this lane's column */
        const u64 full = len >> 4;
        const u32 rem = (u32)len & 15u;

        if (INV) {
            /* P_i = Dec(C_i) ^ C_{i-1}.  CS3: the last two blocks arrive swapped (the wire holds .., C_{b-1}, C_{b-2}):
             * the blocks before them are walked as they lie, the pair is read first and decrypted last */
            const bool swap = MODE == UAES_CB_CBC_DEC && full > 1;
            const u64 n = swap ? full - 2 : full;
            u32 x1 = 0, x2 = 0;
            if (swap) { x1 = row_load_full<A4>(src + 16 * n, c); x2 = row_load_full<A4>(src + 16 * (n + 1), c); }
            u32 px = 0;                                       /* an even block, waiting for its partner */
            row_walk<A4>(src, n, c, [&](u64 i, u32 x) {
                if (!(i & 1u)) {
                    px = x;
                    if (i + 1 < n) return;
                    row_store_full<A4>(dst + 16 * i, row_decrypt<NR>(x, L) ^ v, c);      /* the last block, alone */
                    v = x;
                    return;
                }
                u32 a = px, b = x;
                row_decrypt2<NR>(a, b, L, L);
                row_store_full<A4>(dst + 16 * (i - 1), a ^ v, c);
                row_store_full<A4>(dst + 16 * i, b ^ px, c);
                v = x;
            });
            if (swap) {                                       /* x1 = C_{b-1}, x2 = C_{b-2}; v = C_{b-3} or the IV */
                u32 a = x2, b = x1;
                row_decrypt2<NR>(a, b, L, L);
                row_store_full<A4>(dst + 16 * n, a ^ v, c);
                row_store_full<A4>(dst + 16 * (n + 1), b ^ x2, c);
            }
        } else if (MODE == UAES_CB_CBC_ENC_BLOCKS) {
            row_walk<A4>(src, full, c, [&](u64 i, u32 x) {
                v = row_encrypt<NR>(v ^ x, L);
                row_store_full<A4>(dst + 16 * i, v, c);
            });
        } else if (MODE == UAES_CB_CFB_ENC) {
            const u32 l0 = rem ? row_load(src + 16 * full, rem, c) : 0u;
            row_walk<A4>(src, full, c, [&](u64 i, u32 x) {
                v = row_encrypt<NR>(v, L) ^ x;                /* C_i = Enc(C_{i-1}) ^ P_i = the next feedback */
                row_store_full<A4>(dst + 16 * i, v, c);
            });
            if (rem) row_put(dst + 16 * full, row_encrypt<NR>(v, L) ^ l0, rem, c);
        } else if (MODE == UAES_CB_OFB) {
            const u32 l0 = rem ? row_load(src + 16 * full, rem, c) : 0u;
            row_walk<A4>(src, full, c, [&](u64 i, u32 x) {
                v = row_encrypt<NR>(v, L);                    /* O_i = Enc(O_{i-1}): it does not wait for the text */
                row_store_full<A4>(dst + 16 * i, v ^ x, c);
            });
            if (rem) row_put(dst + 16 * full, row_encrypt<NR>(v, L) ^ l0, rem, c);
        } else {
            /* CFB decrypt: P_i = C_i ^ Enc(C_{i-1});  CTR: out_i = in_i ^ Enc(counter_i).  The cipher's inputs of a
             * pair are both known before the step; a last odd block waits for the ragged one, or goes alone */
            u64 v0 = 0;
            if (MODE == UAES_CB_CTR) {                        /* every lane needs the whole counter: columns 2 and 3 */
                const u32 k2 = bswap32((u32)__shfl((int)v, 8, 16)), k3 = bswap32((u32)__shfl((int)v, 12, 16));
                v0 = ((u64)(k2 & 0x00ffffffu) << 32) | k3;
            }
            auto feed = [&](u64 i, u32 prev) {                /* what block i's cipher call takes */
                if (MODE == UAES_CB_CTR) return cb_ctr_column(v, (v0 + i) & 0x00ffffffffffffffull, c);
                return prev;
            };
            const u32 l0 = rem ? row_load(src + 16 * full, rem, c) : 0u;
            u32 px = 0;
            row_walk<A4>(src, full, c, [&](u64 i, u32 x) {
                if (!(i & 1u)) { px = x; return; }
                u32 a = feed(i - 1, v), b = feed(i, px);
                row_encrypt2<NR>(a, b, L, L);
                row_store_full<A4>(dst + 16 * (i - 1), a ^ px, c);
                row_store_full<A4>(dst + 16 * i, b ^ x, c);
                if (MODE != UAES_CB_CTR) v = x;
            });
            const bool odd = (full & 1u) != 0;                /* px = block full - 1, not yet done */
            if (odd && rem) {
                u32 a = feed(full - 1, v), b = feed(full, px);
                row_encrypt2<NR>(a, b, L, L);
                row_store_full<A4>(dst + 16 * (full - 1), a ^ px, c);
                row_put(dst + 16 * full, b ^ l0, rem, c);
            } else if (odd) {
                row_store_full<A4>(dst + 16 * (full - 1), row_encrypt<NR>(feed(full - 1, v), L) ^ px, c);
            } else if (rem) {
                row_put(dst + 16 * full, row_encrypt<NR>(feed(full, v), L) ^ l0, rem, c);
            }
        }
    }
}

/* ------------------------------------------------------------------------ */
/* plan and launcher                                                          */
/* ------------------------------------------------------------------------ */
static bool cipher_mode_cbc(int mode)
{
    return mode == UAES_CB_CBC_DEC || mode == UAES_CB_CBC_DEC_BLOCKS || mode == UAES_CB_CBC_ENC_BLOCKS;
}

/* cipher.batch: a row batch at any number of records (uaesk_row_shape) */
extern "C" int uaesk_plan_cipher_batch(int mode, size_t len, size_t nmsg, uaes_plan *p)
{
    memset(p, 0, sizeof *p);
    if (mode < 0 || mode >= UAES_CB_MODES) return (int)hipErrorInvalidValue;
    if (cipher_mode_cbc(mode) ? (len < 16 || len % 16) : len > 0xffffffffull) return (int)hipErrorInvalidValue;
    uaesk_row_plan(UAES_CIPHER_BATCH, nmsg, p);
    return 0;
}

extern "C" const char *uaesk_cipher_batch_arrangement_name(int id)
{
    return id == UAES_CIPHER_BATCH ? "cipher.batch" : "?";
}

template <int NR, int MODE>
static int launch_cipher_batch(hipStream_t st, const uaesk_tables *tb, const uaesk_rk *k, const void *ivs, size_t nmsg,
                               size_t msg_bytes, const void *lens, const void *in, void *out)
{
    uaes_plan p;
    uaesk_row_plan(UAES_CIPHER_BATCH, nmsg, &p);
    return with_bool(uaesk_rows_a4(in, out, msg_bytes), [&](auto A4) {
        return uaesk_launch(k_cipher_batch<NR, MODE, decltype(A4)::value>, p.grid, p.steps, UAES_LDS_ROW4, st, *k, *tb, ivs,
                            nmsg, msg_bytes, lens, in, out); });
}

template <int NR>
static int launch_cipher_mode(int mode, hipStream_t st, const uaesk_tables *tb, const uaesk_rk *ek, const uaesk_rk *dk,
                              const void *ivs, size_t nmsg, size_t msg_bytes, const void *lens, const void *in, void *out)
{
#define CB_CASE(M, K) case M: return launch_cipher_batch<NR, M>(st, tb, K, ivs, nmsg, msg_bytes, lens, in, out)
    switch (mode) {
    CB_CASE(UAES_CB_CBC_DEC, dk);
    CB_CASE(UAES_CB_CBC_DEC_BLOCKS, dk);
    CB_CASE(UAES_CB_CBC_ENC_BLOCKS, ek);
    CB_CASE(UAES_CB_CFB_ENC, ek);
    CB_CASE(UAES_CB_CFB_DEC, ek);
    CB_CASE(UAES_CB_OFB, ek);
    CB_CASE(UAES_CB_CTR, ek);
    default: return (int)hipErrorInvalidValue;
    }
#undef CB_CASE
}

extern "C" int uaesk_cipher_batch(void *stream, const uaesk_tables *tb, int nr, const uaesk_rk *ek, const uaesk_rk *dk,
                                  int mode, const void *ivs, size_t nmsg, size_t msg_bytes, const void *lens,
                                  const void *in, void *out)
{
    uaes_plan p;
    const int e = uaesk_plan_cipher_batch(mode, msg_bytes, nmsg, &p);
    if (e) return e;
    if (cipher_mode_cbc(mode)) lens = nullptr;
    if (nmsg == 0) return 0;
    DISPATCH_NR(nr, return (launch_cipher_mode<NR>(mode, S(stream), tb, ek, dk, ivs, nmsg, msg_bytes, lens, in, out)));
    return 0;
}
